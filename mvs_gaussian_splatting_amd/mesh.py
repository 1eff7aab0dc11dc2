"""The last step from a fused volume to a usable surface: cluster the connected triangles of an indexed mesh and keep
the large clusters, on the HIP path (``csrc/mesh.hip`` behind the ``gsr_mesh_*`` entry points).

    vertices, faces, colors = volume.extract_mesh()
    vertices, faces, colors = clean_mesh(vertices, faces, colors, keep_largest=50, min_faces=50)

The mesh of a trained scene is the surface plus thousands of floaters: every blob of fused depth that crosses zero is a
small closed shell of its own.  2DGS clusters the connected triangles, keeps the ``num_cluster`` largest clusters and
drops the vertices nothing refers to; ``clean_mesh`` is that rule.  The labelling is a lock-free union-find on the device
(init, hook, flatten), the numbering and the compaction are scans (torch) around small kernels; the mesh never leaves the
device.  There is no CPU path.

    vertices, faces, colors = simplify_mesh(vertices, faces, colors, voxel_size=2 * volume.voxel_size)

Marching tetrahedra ties the triangle size to the TSDF voxel, not to the detail of the surface.  ``simplify_mesh`` makes
the mesh smaller by vertex clustering on a uniform grid (``csrc/mesh_simplify.hip`` behind the ``gsr_simplify_*`` entry
points): the vertices of a grid cell become their mean, the faces that collapse or repeat go.  The same
key-sort-run pattern, the same compaction.

    counts = view_counts_for_views(cameras, gaussians, pipe, background, vertices)                  # tsdf.py: renders
    vertices, faces, colors = cull_mesh_by_views(vertices, faces, colors, cameras=[], counts=counts, min_views=1)

The published mesh protocols cull before they score: DTU keeps a vertex where it lands on the dilated object mask of
every view that holds it, the unbounded ones drop what no camera saw.  ``vertex_view_counts`` projects every vertex into
every view and counts, per vertex, the views whose image holds it and those that see it (mask, depth map);
``cull_mesh_by_views`` is the rule on those counts and the same compaction; ``dilate_mask`` is the masks' dilation
(``csrc/mesh_cull.hip`` behind ``gsr_cull_view_counts``, ``gsr_cull_face_keep``, ``gsr_mask_dilate``).

    depth, face_id = rasterize_mesh(vertices, faces, camera)
    vertices, faces, colors = cull_invisible_faces(vertices, faces, colors, cameras=cameras, min_views=1)

Looking at the mesh itself: ``rasterize_mesh`` draws it from a camera into a z-buffer with a face id per pixel,
``face_normal_map`` turns the ids into a normal picture, ``face_view_counts`` counts the views in which a face owns a pixel
and ``cull_invisible_faces`` removes the faces no view sees -- inner walls and back layers that vertex tests keep
(``csrc/mesh_raster.hip`` behind ``gsr_raster_view``, ``gsr_raster_resolve``, ``gsr_raster_count_faces``).
"""
from __future__ import annotations

import ctypes as C
import math
import sys
from typing import Optional, Tuple

import torch

from . import _lib

CONNECTIVITIES = ("edge", "vertex")


def _check_faces(faces, num_vertices: Optional[int], what: str) -> Tuple[int, Optional[int]]:
    if not isinstance(faces, torch.Tensor) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"faces must be an int32 [F,3] tensor, got {getattr(faces, 'dtype', type(faces))} "
                         f"{tuple(getattr(faces, 'shape', ()))}")
    F = int(faces.shape[0])
    if F >= 2 ** 31:
        raise ValueError(f"{what} takes fewer than 2^31 faces, got {F}")
    if num_vertices is not None:
        if isinstance(num_vertices, bool) or not isinstance(num_vertices, int):
            raise ValueError(f"num_vertices must be an int, got {num_vertices!r}")
        if not 0 <= num_vertices < 2 ** 31:
            raise ValueError(f"num_vertices must lie in 0..2^31-1, got {num_vertices}")
        if F > 0 and num_vertices == 0:
            raise ValueError(f"{F} faces refer to vertices, but num_vertices is 0")
    return F, num_vertices


def _check_connectivity(connectivity) -> None:
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {CONNECTIVITIES}, got {connectivity!r}")


def _need_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise _lib.GsrError(f"{what} needs the mesh on a ROCm GPU (no CPU path)")


def _label(faces: torch.Tensor, V: int, connectivity: str, stats: Optional[torch.Tensor] = None):
    """The native part of ``connected_components`` on contiguous device faces, F > 0 -> (face_component, component_faces)."""
    lib, dev = _lib.load(), faces.device
    F = int(faces.shape[0])
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mark = torch.empty(F, dtype=torch.uint8, device=dev)
    st = None if stats is None else stats.data_ptr()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if connectivity == "vertex":
            parent = torch.empty(V, dtype=torch.int32, device=dev)
            first = torch.empty(V, dtype=torch.int32, device=dev)
            face_root = torch.empty(F, dtype=torch.int32, device=dev)
            _lib.check(lib.gsr_mesh_cc_init(V, parent.data_ptr(), first.data_ptr(), stream), "gsr_mesh_cc_init")
            _lib.check(lib.gsr_mesh_cc_hook_faces(faces.data_ptr(), F, V, parent.data_ptr(), status.data_ptr(), st, stream),
                       "gsr_mesh_cc_hook_faces")
            _lib.check(lib.gsr_mesh_cc_flatten(V, parent.data_ptr(), stream), "gsr_mesh_cc_flatten")
            _lib.check(lib.gsr_mesh_cc_mark(faces.data_ptr(), F, V, parent.data_ptr(), first.data_ptr(),
                                            face_root.data_ptr(), mark.data_ptr(), stream), "gsr_mesh_cc_mark")
        else:
            parent = torch.empty(F, dtype=torch.int32, device=dev)
            keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
            owner = torch.empty(3 * F, dtype=torch.int32, device=dev)
            _lib.check(lib.gsr_mesh_cc_init(F, parent.data_ptr(), None, stream), "gsr_mesh_cc_init")
            _lib.check(lib.gsr_mesh_edge_keys(faces.data_ptr(), F, V, keys.data_ptr(), owner.data_ptr(), status.data_ptr(),
                                              stream), "gsr_mesh_edge_keys")
            keys_sorted, order = torch.sort(keys)                                # plumbing: stays in torch
            _lib.check(lib.gsr_mesh_cc_hook_runs(keys_sorted.data_ptr(), order.data_ptr(), owner.data_ptr(), 3 * F, F,
                                                 parent.data_ptr(), status.data_ptr(), st, stream), "gsr_mesh_cc_hook_runs")
            _lib.check(lib.gsr_mesh_cc_flatten(F, parent.data_ptr(), stream), "gsr_mesh_cc_flatten")
            _lib.check(lib.gsr_mesh_cc_mark(None, F, 0, parent.data_ptr(), None, None, mark.data_ptr(), stream),
                       "gsr_mesh_cc_mark")
            face_root = parent
        ends = torch.cumsum(mark, dim=0, dtype=torch.int64)
        K, bad = (int(v) for v in torch.stack((ends[-1], status[0].to(torch.int64))).tolist())       # the one read-back
        if bad:
            raise _lib.GsrError(f"connected_components failed: a face refers to a vertex outside 0..{V - 1}")
        ids = ends - mark                                                        # exclusive scan
        face_component = torch.empty(F, dtype=torch.int32, device=dev)
        component_faces = torch.zeros(K, dtype=torch.int64, device=dev)
        _lib.check(lib.gsr_mesh_cc_label(face_root.data_ptr(), ids.data_ptr(), F, K, face_component.data_ptr(),
                                         component_faces.data_ptr(), stream), "gsr_mesh_cc_label")
    return face_component, component_faces


def connected_components(faces: torch.Tensor, num_vertices: Optional[int] = None, connectivity: str = "edge",
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The connected components of the faces of an indexed triangle mesh ->
    ``(face_component int32 [F], component_faces int64 [K])`` on the device of ``faces`` (int32 ``[F,3]``).

    ``connectivity="edge"`` (the default; Open3D's ``cluster_connected_triangles``, what 2DGS uses): two faces are
    connected when they share an undirected edge ``{a, b}``; an edge of three or more faces joins all of them.
    ``connectivity="vertex"``: two faces are connected when they share a vertex.  Vertices are identified by index (a
    mesh whose faces repeat positions under different indices is not welded here).  Components are numbered ``0..K-1``
    in the order of their smallest face index; ``component_faces[c]`` is the number of faces of component ``c``.  The
    same bits from run to run.

    ``num_vertices``: the number of vertices ``V``; every index must lie in ``0..V-1``, which is checked on the device
    (``GsrError``).  ``None``: ``max(faces) + 1``, one read-back more.  Otherwise one host read-back (``K``, together
    with the range check); everything runs on the current stream.  ``F == 0``: empty tensors and no native call."""
    F, V = _check_faces(faces, num_vertices, "connected_components")
    _check_connectivity(connectivity)
    _need_gpu(faces, "connected_components")
    dev = faces.device
    if F == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    faces = faces.detach().contiguous()
    if V is None:
        V = min(max(int(faces.max()) + 1, 1), 2 ** 31 - 1)            # a negative index is then refused on the device
    return _label(faces, V, connectivity)


def clean_mesh(vertices: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor] = None, *,
               keep_largest: Optional[int] = None, min_faces: int = 0, connectivity: str = "edge",
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Keep the large connected components of a mesh and drop the vertices nothing refers to any more ->
    ``(vertices float32 [V',3], faces int32 [F',3], colors float32 [V',3] or None)``, new tensors on the same device.

    2DGS's post-processing rule.  With the components of ``connected_components(faces, V, connectivity)``:
    ``threshold = max(min_faces, size of the keep_largest-th largest component)``, where the size term counts as 0 when
    ``keep_largest`` is ``None`` or at least ``K``; a face is kept when its component has at least ``threshold`` faces.
    Components that tie with the ``keep_largest``-th largest all survive, so more than ``keep_largest`` components may
    remain.  (2DGS: ``keep_largest=50, min_faces=50``.)

    Kept vertices and kept faces stay in their original order; the kept vertex and colour rows are bit-copies, the kept
    faces are re-indexed.  Nothing is kept: ``[0,3]`` tensors.  Two host read-backs (``K`` with the index check, then
    ``V'`` and ``F'``); everything else stays on the device and on the current stream.  ``F == 0`` makes no native call."""
    if not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.float32 or vertices.dim() != 2 \
            or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be a float32 [V,3] tensor, got {getattr(vertices, 'dtype', type(vertices))} "
                         f"{tuple(getattr(vertices, 'shape', ()))}")
    V = int(vertices.shape[0])
    F, _ = _check_faces(faces, V, "clean_mesh")
    dev = vertices.device
    if faces.device != dev:
        raise ValueError(f"faces must be on the device of vertices ({dev}), got {faces.device}")
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32
                               or tuple(colors.shape) != (V, 3) or colors.device != dev):
        raise ValueError(f"colors must be a float32 [{V},3] tensor on {dev}, got "
                         f"{getattr(colors, 'dtype', type(colors))} {tuple(getattr(colors, 'shape', ()))} on "
                         f"{getattr(colors, 'device', None)}")
    if keep_largest is not None and (isinstance(keep_largest, bool) or not isinstance(keep_largest, int)
                                     or keep_largest < 1):
        raise ValueError(f"keep_largest must be a positive int or None, got {keep_largest!r}")
    if isinstance(min_faces, bool) or not isinstance(min_faces, int) or min_faces < 0:
        raise ValueError(f"min_faces must be a non-negative int, got {min_faces!r}")
    _check_connectivity(connectivity)
    _need_gpu(vertices, "clean_mesh")

    def empty():
        return (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                None if colors is None else torch.empty((0, 3), dtype=torch.float32, device=dev))

    if F == 0:
        return empty()
    lib = _lib.load()
    vertices_c, faces_c = vertices.detach().contiguous(), faces.detach().contiguous()
    colors_c = None if colors is None else colors.detach().contiguous()
    face_component, component_faces = _label(faces_c, V, connectivity)              # read-back 1: K
    K = int(component_faces.shape[0])
    threshold = torch.full((), min_faces, dtype=torch.int64, device=dev)
    if keep_largest is not None and keep_largest < K:
        kth = torch.topk(component_faces, keep_largest, largest=True, sorted=True).values[-1]
        threshold = torch.maximum(threshold, kth)
    keep = (component_faces[face_component.to(torch.int64)] >= threshold).to(torch.uint8)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    return _compact_kept(lib, vertices_c, colors_c, faces_c, keep, status, "clean_mesh") or empty()   # read-back 2: V', F'


def _compact_kept(lib, vertices_c, colors_c, faces_c, keep, status, what):
    """The tail that ``clean_mesh`` and ``cull_mesh_by_views`` share: with ``keep`` uint8 ``[F]`` (0 / 1) over contiguous
    device tensors, F > 0, mark the vertices of the kept faces, scan, read ``V'``, ``F'`` and the status word back (the one
    read-back) and compact -> ``(vertices, faces, colors or None)``, or ``None`` when no face is kept.  A status word that
    is not 0 -- a face index outside ``0..V-1``, here or in the caller's kernels before -- raises ``GsrError``."""
    V, F, dev = int(vertices_c.shape[0]), int(faces_c.shape[0]), vertices_c.device
    vertex_mark = torch.zeros(V, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_mesh_mark_vertices(faces_c.data_ptr(), keep.data_ptr(), F, V, vertex_mark.data_ptr(),
                                              status.data_ptr(), stream), "gsr_mesh_mark_vertices")
        vert_end = torch.cumsum(vertex_mark, dim=0, dtype=torch.int64)
        face_end = torch.cumsum(keep, dim=0, dtype=torch.int64)
        Vk, Fk, bad = (int(v) for v in torch.stack((vert_end[-1], face_end[-1], status[0].to(torch.int64))).tolist())
        if bad:
            raise _lib.GsrError(f"{what} failed: a face refers to a vertex outside 0..{V - 1}")
        if Fk == 0:
            return None
        out_vertices = torch.empty((Vk, 3), dtype=torch.float32, device=dev)
        out_faces = torch.empty((Fk, 3), dtype=torch.int32, device=dev)
        out_colors = None if colors_c is None else torch.empty((Vk, 3), dtype=torch.float32, device=dev)
        vert_offs, face_offs = vert_end - vertex_mark, face_end - keep                              # exclusive scans
        _lib.check(lib.gsr_mesh_compact(vertices_c.data_ptr(), None if colors_c is None else colors_c.data_ptr(),
                                        faces_c.data_ptr(), keep.data_ptr(), vertex_mark.data_ptr(), vert_offs.data_ptr(),
                                        face_offs.data_ptr(), V, F, Vk, Fk, out_vertices.data_ptr(),
                                        None if out_colors is None else out_colors.data_ptr(), out_faces.data_ptr(),
                                        status.data_ptr(), stream), "gsr_mesh_compact")
    return out_vertices, out_faces, out_colors


CELL_BITS = 21                      # bits per axis of a cell key (csrc/mesh_simplify_math.h)
_BAD_INDEX, _NOT_FINITE, _OUT_OF_RANGE = 1, 2, 4       # bits of the status word (include/gsr.h: GSR_SIMPLIFY_*)


def _simplify_status(bad: int, V: int, voxel_size: float) -> None:
    if bad & _BAD_INDEX:
        raise _lib.GsrError(f"simplify_mesh failed: a face refers to a vertex outside 0..{V - 1}")
    if bad & _NOT_FINITE:
        raise _lib.GsrError("simplify_mesh failed: a vertex that a face refers to has a coordinate that is not finite")
    if bad & _OUT_OF_RANGE:
        raise _lib.GsrError(f"simplify_mesh failed: a cell index lies outside 0..2^{CELL_BITS}-1: voxel_size "
                            f"{voxel_size!r} is too small for the extent of the mesh, or the origin lies above a vertex")
    if bad:
        raise _lib.GsrError(f"simplify_mesh failed: status {bad}")


def simplify_mesh(vertices: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor] = None, *,
                  voxel_size: float, origin=None, return_map: bool = False):
    """Simplify a mesh by vertex clustering on a uniform grid (Rossignac-Borrel; Open3D's ``simplify_vertex_clustering``
    with the averaging contraction) -> ``(vertices float32 [V',3], faces int32 [F',3], colors float32 [V',3] or None)``,
    with ``return_map=True`` also ``vertex_cluster int32 [V]``; new tensors on the same device (csrc/mesh_simplify.hip;
    DESIGN.md §7.26).

    The rule, step by step:

    1. Only the vertices that a face refers to take part; the others may hold anything.  A face index outside
       ``0..V-1`` and a referenced coordinate that is not finite raise ``GsrError``.
    2. The cell of a vertex is ``floor(((double)x - origin) / voxel_size)`` per axis, in float64.  ``origin`` (three
       finite floats) defaults to the per-axis minimum of the referenced vertices minus ``voxel_size / 2``.  Every cell
       index must lie in ``0..2^21-1``, or ``GsrError`` says that ``voxel_size`` is too small for the extent or that the
       origin lies above a vertex.  Key: ``ix << 42 | iy << 21 | iz``.
    3. The clusters are the distinct keys, in ascending order.
    4. A cluster's position and colour are the means of its members' float32 rows, summed in float64 in ascending vertex
       index and rounded to float32 once: the same bits from run to run, and a cluster of one member is a bit-copy.
    5. A face becomes the clusters of its corners.  A face with two equal corners is dropped.  Of the faces that have the
       same corners in the same cyclic order the one with the smallest index stays; faces of opposite winding are
       different faces.  The faces that stay keep their relative order and their corner order.
    6. Clusters that no remaining face refers to are dropped; the rest keep their key order.  ``vertex_cluster[v]`` is
       the output vertex that ``v`` went to, ``-1`` for a vertex that took no part or whose cluster was dropped.

    What vertex clustering does not preserve: manifoldness and closedness.  A thin wall whose two sides fall into the
    same cells folds onto itself, a tunnel narrower than a cell closes, an edge may end up in more than two faces, and a
    closed surface may open where faces degenerate.  What it does bound: every output vertex lies within the cell of its
    members, so within ``sqrt(3) * voxel_size`` of each of them.  Triangles larger than a cell pass through untouched.

    Two host read-backs (the number of clusters with the status word, then ``F'`` and ``V'``); the default origin stays
    on the device.  Everything runs on the current stream and no input is written.  ``F == 0``: ``[0,3]`` tensors (and a
    map of ``-1``) without a native call.  There is no CPU path."""
    if not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.float32 or vertices.dim() != 2 \
            or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be a float32 [V,3] tensor, got {getattr(vertices, 'dtype', type(vertices))} "
                         f"{tuple(getattr(vertices, 'shape', ()))}")
    V = int(vertices.shape[0])
    F, _ = _check_faces(faces, V, "simplify_mesh")
    dev = vertices.device
    if faces.device != dev:
        raise ValueError(f"faces must be on the device of vertices ({dev}), got {faces.device}")
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32
                               or tuple(colors.shape) != (V, 3) or colors.device != dev):
        raise ValueError(f"colors must be a float32 [{V},3] tensor on {dev}, got "
                         f"{getattr(colors, 'dtype', type(colors))} {tuple(getattr(colors, 'shape', ()))} on "
                         f"{getattr(colors, 'device', None)}")
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float)) \
            or not 0 < voxel_size <= sys.float_info.max:
        raise ValueError(f"voxel_size must be a finite positive float, got {voxel_size!r}")
    h = float(voxel_size)
    if origin is not None:
        try:
            origin = tuple(float(o) for o in origin)
        except (TypeError, ValueError):
            raise ValueError(f"origin must be None or three finite floats, got {origin!r}") from None
        if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
            raise ValueError(f"origin must be None or three finite floats, got {origin!r}")
    if not isinstance(return_map, bool):
        raise ValueError(f"return_map must be a bool, got {return_map!r}")
    _need_gpu(vertices, "simplify_mesh")

    def empty():
        out = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
               None if colors is None else torch.empty((0, 3), dtype=torch.float32, device=dev))
        return out + (torch.full((V,), -1, dtype=torch.int32, device=dev),) if return_map else out

    if F == 0:
        return empty()
    lib = _lib.load()
    vertices_c, faces_c = vertices.detach().contiguous(), faces.detach().contiguous()
    colors_c = None if colors is None else colors.detach().contiguous()
    ptr = lambda t: None if t is None else t.data_ptr()                                          # noqa: E731
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        # step 1: the vertices that take part are those gsr_mesh_mark_vertices marks with every face kept
        every_face = torch.ones(F, dtype=torch.uint8, device=dev)
        vertex_mark = torch.zeros(V, dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_mesh_mark_vertices(faces_c.data_ptr(), every_face.data_ptr(), F, V, vertex_mark.data_ptr(),
                                              status.data_ptr(), stream), "gsr_mesh_mark_vertices")
        # step 2: cells.  The default origin never leaves the device
        if origin is None:
            origin_dev = torch.empty(3, dtype=torch.float64, device=dev)
            lowest = torch.empty(3, dtype=torch.int32, device=dev)
            _lib.check(lib.gsr_simplify_default_origin(vertices_c.data_ptr(), vertex_mark.data_ptr(), V, h, lowest.data_ptr(),
                                                       origin_dev.data_ptr(), stream), "gsr_simplify_default_origin")
        else:
            origin_dev = torch.tensor(origin, dtype=torch.float64, device=dev)
        keys = torch.empty(V, dtype=torch.int64, device=dev)
        _lib.check(lib.gsr_simplify_cell_keys(vertices_c.data_ptr(), vertex_mark.data_ptr(), V, origin_dev.data_ptr(), h,
                                              keys.data_ptr(), status.data_ptr(), stream), "gsr_simplify_cell_keys")
        # step 3: stable, so that the members of a cell stay in ascending vertex index (plumbing: stays in torch)
        keys_sorted, order = torch.sort(keys, stable=True)
        head = torch.empty(V, dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_simplify_run_heads(keys_sorted.data_ptr(), V, head.data_ptr(), stream), "gsr_simplify_run_heads")
        ends = torch.cumsum(head, dim=0, dtype=torch.int64)
        K, bad = (int(v) for v in torch.stack((ends[-1], status[0].to(torch.int64))).tolist())       # read-back 1
        _simplify_status(bad, V, voxel_size)
        # step 4: the representatives
        start = torch.empty(K + 1, dtype=torch.int32, device=dev)
        means = torch.empty((K, 3), dtype=torch.float32, device=dev)
        mean_colors = None if colors_c is None else torch.empty((K, 3), dtype=torch.float32, device=dev)
        cluster_of_vertex = torch.empty(V, dtype=torch.int32, device=dev)
        _lib.check(lib.gsr_simplify_reduce(vertices_c.data_ptr(), ptr(colors_c), keys_sorted.data_ptr(), order.data_ptr(),
                                           ends.data_ptr(), V, K, start.data_ptr(), means.data_ptr(), ptr(mean_colors),
                                           cluster_of_vertex.data_ptr(), status.data_ptr(), stream), "gsr_simplify_reduce")
        # step 5: the faces.  Three 31-bit indices do not fit one int64 key: two stable sorts, the third index first
        tri = torch.empty((F, 3), dtype=torch.int32, device=dev)
        keep = torch.empty(F, dtype=torch.uint8, device=dev)
        key_first = torch.empty(F, dtype=torch.int64, device=dev)
        key_third = torch.empty(F, dtype=torch.int32, device=dev)
        _lib.check(lib.gsr_simplify_face_keys(faces_c.data_ptr(), cluster_of_vertex.data_ptr(), F, V, K, tri.data_ptr(),
                                              keep.data_ptr(), key_first.data_ptr(), key_third.data_ptr(),
                                              status.data_ptr(), stream), "gsr_simplify_face_keys")
        by_third = torch.sort(key_third, stable=True).indices
        first_sorted, by_first = torch.sort(key_first[by_third], stable=True)
        perm = by_third[by_first]
        _lib.check(lib.gsr_simplify_face_unique(first_sorted.data_ptr(), perm.data_ptr(), key_third.data_ptr(), F,
                                                keep.data_ptr(), status.data_ptr(), stream), "gsr_simplify_face_unique")
        # step 6: compaction, with the cluster means as the vertices
        cluster_mark = torch.zeros(K, dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_mesh_mark_vertices(tri.data_ptr(), keep.data_ptr(), F, K, cluster_mark.data_ptr(),
                                              status.data_ptr(), stream), "gsr_mesh_mark_vertices")
        vert_end = torch.cumsum(cluster_mark, dim=0, dtype=torch.int64)
        face_end = torch.cumsum(keep, dim=0, dtype=torch.int64)
        Vk, Fk, bad = (int(v) for v in torch.stack((vert_end[-1], face_end[-1],
                                                    status[0].to(torch.int64))).tolist())            # read-back 2
        _simplify_status(bad, V, voxel_size)
        if Fk == 0:
            return empty()
        out_vertices = torch.empty((Vk, 3), dtype=torch.float32, device=dev)
        out_faces = torch.empty((Fk, 3), dtype=torch.int32, device=dev)
        out_colors = None if colors_c is None else torch.empty((Vk, 3), dtype=torch.float32, device=dev)
        vert_offs, face_offs = vert_end - cluster_mark, face_end - keep                              # exclusive scans
        _lib.check(lib.gsr_mesh_compact(means.data_ptr(), ptr(mean_colors), tri.data_ptr(), keep.data_ptr(),
                                        cluster_mark.data_ptr(), vert_offs.data_ptr(), face_offs.data_ptr(), K, F, Vk, Fk,
                                        out_vertices.data_ptr(), ptr(out_colors), out_faces.data_ptr(),
                                        status.data_ptr(), stream), "gsr_mesh_compact")
        if not return_map:
            return out_vertices, out_faces, out_colors
        vertex_cluster = torch.empty(V, dtype=torch.int32, device=dev)
        _lib.check(lib.gsr_simplify_vertex_map(cluster_of_vertex.data_ptr(), cluster_mark.data_ptr(), vert_offs.data_ptr(),
                                               V, K, vertex_cluster.data_ptr(), stream), "gsr_simplify_vertex_map")
    return out_vertices, out_faces, out_colors, vertex_cluster


def _check_mesh(vertices, faces, colors, what: str, with_faces: bool = True) -> Tuple[int, int]:
    if not isinstance(vertices, torch.Tensor) or vertices.dtype != torch.float32 or vertices.dim() != 2 \
            or vertices.shape[1] != 3:
        raise ValueError(f"vertices must be a float32 [V,3] tensor, got {getattr(vertices, 'dtype', type(vertices))} "
                         f"{tuple(getattr(vertices, 'shape', ()))}")
    V = int(vertices.shape[0])
    if V >= 2 ** 31:
        raise ValueError(f"{what} takes fewer than 2^31 vertices, got {V}")
    if not with_faces:
        return V, 0
    F, _ = _check_faces(faces, V, what)
    dev = vertices.device
    if faces.device != dev:
        raise ValueError(f"faces must be on the device of vertices ({dev}), got {faces.device}")
    if colors is not None and (not isinstance(colors, torch.Tensor) or colors.dtype != torch.float32
                               or tuple(colors.shape) != (V, 3) or colors.device != dev):
        raise ValueError(f"colors must be a float32 [{V},3] tensor on {dev}, got "
                         f"{getattr(colors, 'dtype', type(colors))} {tuple(getattr(colors, 'shape', ()))} on "
                         f"{getattr(colors, 'device', None)}")
    return V, F


def _view_map(m, H: int, W: int, dev, dtypes, what: str) -> torch.Tensor:
    if not isinstance(m, torch.Tensor) or m.dtype not in dtypes or m.device != dev \
            or tuple(m.shape) not in ((H, W), (1, H, W)):
        names = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{what} must be a {names} [{H},{W}] or [1,{H},{W}] tensor on {dev}, got "
                         f"{getattr(m, 'dtype', type(m))} {tuple(getattr(m, 'shape', ()))} on {getattr(m, 'device', None)}")
    m = m.detach().reshape(H, W).contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _cull_scalars(near, depth_tol) -> Tuple[float, float]:
    for name, v in (("near", near), ("depth_tol", depth_tol)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite float, got {v!r}")
    if not near > 0:
        raise ValueError(f"near must be positive, got {near!r}")
    if depth_tol < 0:
        raise ValueError(f"depth_tol must not be negative, got {depth_tol!r}")
    return float(near), float(depth_tol)


def _per_view(maps, S: int, name: str) -> list:
    if maps is None:
        return [None] * S
    try:
        maps = list(maps)
    except TypeError:
        raise ValueError(f"{name} must be None or a sequence of {S} maps, got {type(maps)}") from None
    if len(maps) != S:
        raise ValueError(f"{len(maps)} {name} for {S} cameras")
    return maps


def dilate_mask(mask: torch.Tensor, radius: int) -> torch.Tensor:
    """The binary dilation of ``mask`` (uint8 or bool ``[H,W]`` on a ROCm GPU; non-zero is set) by a
    ``(2 radius + 1) x (2 radius + 1)`` square -> a new uint8 ``[H,W]`` tensor of 0 / 1 (csrc/mesh_cull.hip, two separable
    passes).  Pixels outside the image count as 0; ``radius = 0`` only normalises the mask; ``radius`` lies in 0..1024.
    2DGS dilates DTU's object masks with a 50 x 50 kernel before it culls: ``radius=25`` here.  Two launches on the current
    stream, nothing is read back."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or mask.dim() != 2 \
            or mask.shape[0] < 1 or mask.shape[1] < 1:
        raise ValueError(f"mask must be a uint8 or bool [H,W] tensor with H, W >= 1, got "
                         f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    H, W = int(mask.shape[0]), int(mask.shape[1])
    if H * W > 2 ** 28:
        raise ValueError(f"a mask of {W} x {H} exceeds 2^28 pixels")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= _lib.DILATE_MAX_RADIUS:
        raise ValueError(f"radius must be an int in 0..{_lib.DILATE_MAX_RADIUS}, got {radius!r}")
    _need_gpu(mask, "dilate_mask")
    lib, dev = _lib.load(), mask.device
    mask_c = _view_map(mask, H, W, dev, (torch.uint8, torch.bool), "mask")
    tmp = torch.empty((H, W), dtype=torch.uint8, device=dev)
    out = torch.empty((H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_mask_dilate(mask_c.data_ptr(), H, W, radius, tmp.data_ptr(), out.data_ptr(), stream),
                   "gsr_mask_dilate")
    return out


def vertex_view_counts(vertices: torch.Tensor, cameras, *, masks=None, depths=None, near: float = 0.2,
                       depth_tol: float = 0.01, counts=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """How many views see each vertex -> ``(in_view int32 [V], visible int32 [V])`` on the device of ``vertices`` (float32
    ``[V,3]`` on a ROCm GPU), in one launch on the current stream (csrc/mesh_cull.hip).

    ``cameras``: up to 65535 of anything with ``world_view_transform``, ``FoVx``, ``FoVy``, ``image_width``,
    ``image_height``.  Per vertex and camera, in float32 with every operation rounded on its own (csrc/mesh_cull_math.h):
    the vertex goes through ``world_view_transform``; a view counts only if ``zv > near``; it lands at
    ``u = fx xv / zv + cx``, ``v = fy yv / zv + cy`` with ``cx = (W - 1) / 2``, and the pixel is ``floor(u + 0.5)``,
    ``floor(v + 0.5)``; a view whose image holds that pixel adds 1 to ``in_view``.  It adds 1 to ``visible`` as well unless
    ``masks[k]`` (uint8 or bool ``[H,W]``; non-zero is object) is 0 there, or ``depths[k]`` (float32 ``[H,W]``; 0 is no
    surface) holds no surface there or one in front of the vertex: ``zv - ds > depth_tol * ds``.  ``masks`` / ``depths``:
    ``None`` or one entry per camera, each ``None`` or a map of that camera's size on the vertices' device.

    ``counts=(in_view, visible)``: two int32 ``[V]`` tensors that the counts are added into (and that are returned), so
    that views can be fed in chunks and each chunk's depth maps freed; counts over chunks equal counts over one call.
    NaN coordinates count nowhere.  The table of views is one small host-to-device copy; nothing is read back."""
    V, _ = _check_mesh(vertices, None, None, "vertex_view_counts", with_faces=False)
    views = _view_table(V, vertices.device, cameras, masks, depths, near, depth_tol, counts)
    _need_gpu(vertices, "vertex_view_counts")
    return _count_views(vertices, views, counts)


def _view_table(V: int, dev, cameras, masks, depths, near, depth_tol, counts):
    """Every check of ``vertex_view_counts`` behind the vertices', on the host, and the table of views ->
    ``(S, table, maps, near, depth_tol)``; ``maps[k] = [mask or None, depth or None]``, the contiguous ``[H,W]`` maps
    whose addresses the rows hold."""
    try:
        cameras = list(cameras)
    except TypeError:
        raise ValueError(f"cameras must be a sequence of cameras, got {type(cameras)}") from None
    S = len(cameras)
    if S > _lib.CULL_MAX_VIEWS:
        raise ValueError(f"at most {_lib.CULL_MAX_VIEWS} views in one call, got {S}: feed them in chunks through counts=")
    near, depth_tol = _cull_scalars(near, depth_tol)
    masks, depths = _per_view(masks, S, "masks"), _per_view(depths, S, "depths")
    if counts is not None:
        if not isinstance(counts, (tuple, list)) or len(counts) != 2 or any(
                not isinstance(c, torch.Tensor) or c.dtype != torch.int32 or tuple(c.shape) != (V,) or c.device != dev
                or not c.is_contiguous() for c in counts) or (V > 0 and counts[0].data_ptr() == counts[1].data_ptr()):
            raise ValueError(f"counts must be two distinct contiguous int32 [{V}] tensors on {dev}")
    from .mvs import _focal
    table = (_lib.GsrCullView * max(S, 1))()
    maps = []
    for k, (cam, m, d) in enumerate(zip(cameras, masks, depths)):
        H, W, fx, fy = _focal(cam)
        if H * W > 2 ** 28 or max(H, W) > 2 ** 24:
            raise ValueError(f"camera {k}: an image of {W} x {H} exceeds 2^28 pixels or 2^24 a side")
        M = cam.world_view_transform.detach().to(device="cpu", dtype=torch.float32)
        if tuple(M.shape) != (4, 4):
            raise ValueError(f"camera {k}: world_view_transform must be 4 x 4, got {tuple(M.shape)}")
        row = table[k]
        row.width, row.height, row.fx, row.fy = W, H, fx, fy
        row.world_to_view[:] = M.reshape(-1).tolist()
        if m is not None:
            m = _view_map(m, H, W, dev, (torch.uint8, torch.bool), f"masks[{k}]")
            row.mask = m.data_ptr()
        if d is not None:
            d = _view_map(d, H, W, dev, (torch.float32,), f"depths[{k}]")
            row.depth = d.data_ptr()
        maps.append([m, d])
    return S, table, maps, near, depth_tol


def _count_views(vertices: torch.Tensor, views, counts) -> Tuple[torch.Tensor, torch.Tensor]:
    """The launch of ``vertex_view_counts`` for the table of ``_view_table``, on device vertices."""
    S, table, maps, near, depth_tol = views
    V, dev = int(vertices.shape[0]), vertices.device
    if counts is None:
        in_view = torch.empty(V, dtype=torch.int32, device=dev)
        visible = torch.empty(V, dtype=torch.int32, device=dev)
    else:
        in_view, visible = counts
    if V == 0:
        return in_view, visible
    lib = _lib.load()
    vertices_c = vertices.detach().contiguous()
    with torch.cuda.device(dev):
        table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev) if S > 0 else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_cull_view_counts(vertices_c.data_ptr(), V, None if table_dev is None else table_dev.data_ptr(), S,
                                            near, depth_tol, 0 if counts is None else 1, in_view.data_ptr(),
                                            visible.data_ptr(), stream), "gsr_cull_view_counts")
    return in_view, visible


def cull_mesh_by_views(vertices: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor] = None, *, cameras,
                       masks=None, depths=None, min_views=1, near: float = 0.2, depth_tol: float = 0.01, dilate: int = 0,
                       counts=None, return_counts: bool = False):
    """Keep the part of a mesh that the views saw -> ``(vertices float32 [V',3], faces int32 [F',3], colors float32 [V',3]
    or None)``, with ``return_counts=True`` also ``(in_view, visible)`` of the input vertices; new tensors on the same
    device (csrc/mesh_cull.hip).

    With ``(in_view, visible) = vertex_view_counts(vertices, cameras, masks=..., depths=..., near=..., depth_tol=...,
    counts=...)``: a vertex is kept when ``visible >= min_views``.  ``min_views="all"`` stands for the vertex's own
    ``in_view``, the number of views that counted it: the vertex must be visible in every view whose image it lands in,
    which with object masks is DTU's rule (2DGS's ``cull_scan``; a vertex no view holds passes it, as it does there).
    ``min_views=1`` without masks and with ``depths`` is the rule of the unbounded protocols: what no camera saw goes.
    ``dilate``: every mask is dilated by that radius first (``dilate_mask``; 2DGS: 25).  ``counts``: counts of earlier
    chunks of views to add to (``vertex_view_counts``); ``cameras`` may then be empty.

    A face is kept when all three of its corners are; then the vertices that no kept face refers to go as well.  Kept
    vertices and faces stay in their original order; the kept vertex and colour rows are bit-copies, the kept faces are
    re-indexed.  Nothing is kept: ``[0,3]`` tensors.  One host read-back (``V'`` and ``F'``, with the check that every
    face index lies in ``0..V-1``, else ``GsrError``); everything else stays on the device and on the current stream.
    ``F == 0`` makes no native call (the counts returned are then the ones given, or zeros).  There is no CPU path."""
    V, F = _check_mesh(vertices, faces, colors, "cull_mesh_by_views")
    if min_views != "all" and (isinstance(min_views, bool) or not isinstance(min_views, int) or min_views < 0):
        raise ValueError(f"min_views must be a non-negative int or \"all\", got {min_views!r}")
    if isinstance(dilate, bool) or not isinstance(dilate, int) or not 0 <= dilate <= _lib.DILATE_MAX_RADIUS:
        raise ValueError(f"dilate must be an int in 0..{_lib.DILATE_MAX_RADIUS}, got {dilate!r}")
    if not isinstance(return_counts, bool):
        raise ValueError(f"return_counts must be a bool, got {return_counts!r}")
    if min_views != "all" and min_views >= 2 ** 31:
        raise ValueError(f"min_views must fit an int32, got {min_views!r}")
    dev = vertices.device

    def result(mesh, in_view=None, visible=None):
        if mesh is None:
            mesh = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                    None if colors is None else torch.empty((0, 3), dtype=torch.float32, device=dev))
        return mesh + ((in_view, visible),) if return_counts else mesh

    views = _view_table(V, dev, cameras, masks, depths, near, depth_tol, counts)
    _need_gpu(vertices, "cull_mesh_by_views")
    if F == 0:                          # nothing to cull and nothing counted: the counts given, or zeros
        zeros = torch.zeros(V, dtype=torch.int32, device=dev)
        return result(None, *(counts if counts is not None else (zeros, zeros.clone())))
    if dilate:
        table, maps = views[1], views[2]
        for k, pair in enumerate(maps):
            if pair[0] is not None:
                pair[0] = dilate_mask(pair[0], dilate)
                table[k].mask = pair[0].data_ptr()
    in_view, visible = _count_views(vertices, views, counts)
    lib = _lib.load()
    vertices_c, faces_c = vertices.detach().contiguous(), faces.detach().contiguous()
    colors_c = None if colors is None else colors.detach().contiguous()
    vkeep = (visible >= (in_view if min_views == "all" else min_views)).to(torch.uint8)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    keep = torch.empty(F, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_cull_face_keep(faces_c.data_ptr(), vkeep.data_ptr(), F, V, keep.data_ptr(), status.data_ptr(),
                                          stream), "gsr_cull_face_keep")
    return result(_compact_kept(lib, vertices_c, colors_c, faces_c, keep, status, "cull_mesh_by_views"), in_view, visible)


def _raster_scalars(near, **flags) -> float:
    if isinstance(near, bool) or not isinstance(near, (int, float)) or not math.isfinite(near):
        raise ValueError(f"near must be a finite float, got {near!r}")
    if not near > 0:
        raise ValueError(f"near must be positive, got {near!r}")
    for name, v in flags.items():
        if not isinstance(v, bool):
            raise ValueError(f"{name} must be a bool, got {v!r}")
    return float(near)


def _raster_rows(cameras):
    """The host rows of the cameras, checked -> a list of ``_lib.GsrCullView``."""
    try:
        cameras = list(cameras)
    except TypeError:
        raise ValueError(f"cameras must be a sequence of cameras, got {type(cameras)}") from None
    from .mvs import _focal
    rows = []
    for k, cam in enumerate(cameras):
        H, W, fx, fy = _focal(cam)
        if H * W > 2 ** 28 or max(H, W) > _lib.RASTER_MAX_SIDE:
            raise ValueError(f"camera {k}: an image of {W} x {H} exceeds 2^28 pixels or 2^14 a side")
        M = cam.world_view_transform.detach().to(device="cpu", dtype=torch.float32)
        if tuple(M.shape) != (4, 4):
            raise ValueError(f"camera {k}: world_view_transform must be 4 x 4, got {tuple(M.shape)}")
        row = _lib.GsrCullView()
        row.width, row.height, row.fx, row.fy = W, H, fx, fy
        row.world_to_view[:] = M.reshape(-1).tolist()
        rows.append(row)
    return rows


class _RasterWorkspace:
    """The key buffer and the queue of the rasterizer for a mesh of F faces and images of up to ``pixels`` pixels."""

    def __init__(self, lib, F: int, pixels: int, dev):
        self.queue_bytes = int(lib.gsr_raster_queue_bytes(F))
        self.queue = torch.empty(self.queue_bytes, dtype=torch.uint8, device=dev)
        self.keys = torch.empty(max(pixels, 1), dtype=torch.int64, device=dev)

    def head(self):
        """(queued, dropped, bad faces) of the last view: a read-back."""
        return self.queue[:12].view(torch.int32).tolist()


def _raster_view(lib, ws, vertices_c, faces_c, row, near: float, flags: int, stream, view_scratch=None) -> None:
    _lib.check(lib.gsr_raster_view(vertices_c.data_ptr(), int(vertices_c.shape[0]), faces_c.data_ptr(),
                                   int(faces_c.shape[0]), C.byref(row), near, flags, ws.keys.data_ptr(), ws.queue.data_ptr(),
                                   ws.queue_bytes, None if view_scratch is None else view_scratch.data_ptr(), stream),
               "gsr_raster_view")


def rasterize_mesh(vertices: torch.Tensor, faces: torch.Tensor, camera, *, near: float = 0.2, cull_backfaces: bool = False,
                   stats: bool = False):
    """Rasterize a mesh from ``camera`` -> ``(depth float32 [H,W], face_id int32 [H,W])`` on the device of ``vertices``
    (float32 ``[V,3]``, ``faces`` int32 ``[F,3]``, on a ROCm GPU), with ``stats=True`` also ``{"dropped": n,
    "bad_faces": m}`` (csrc/mesh_raster.hip).

    ``depth`` is the view-space z of the nearest surface at each pixel centre, 0 where there is none (the convention of
    ``render(return_depth=True)``); ``face_id`` is the face that owns the pixel, -1 where there is none; at equal depth
    the smallest face index owns it.  The rule (csrc/mesh_raster_math.h): corners through ``world_view_transform`` in
    float32; faces clipped against ``z = near``; ``u = fx xv / zv + (W - 1) / 2`` snapped to 1/256 pixel; coverage by
    exact integer edge functions with the top-left rule, so that two faces sharing an edge cover every centre on it
    exactly once; depth interpolated perspective-correctly in float64 and rounded to float32 once.  Both windings are
    drawn unless ``cull_backfaces``.  The result does not depend on the order of the faces and is the same bits from run
    to run.

    Limits: an image of at most 2^14 pixels a side; a piece of a face with a corner farther than 2^21 pixels from the
    image's origin is dropped and counted (``stats``: ``dropped``; a read-back made only then), as is a face with an index
    outside ``0..V-1`` (``bad_faces``).  ``F == 0``: zeros and -1.  Everything runs on the current stream."""
    V, F = _check_mesh(vertices, faces, None, "rasterize_mesh")
    near = _raster_scalars(near, cull_backfaces=cull_backfaces, stats=stats)
    row, = _raster_rows([camera])
    _need_gpu(vertices, "rasterize_mesh")
    lib, dev = _lib.load(), vertices.device
    H, W = row.height, row.width
    vertices_c, faces_c = vertices.detach().contiguous(), faces.detach().contiguous()
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    face_id = torch.empty((H, W), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = _RasterWorkspace(lib, F, H * W, dev)
        flags = _lib.RASTER_CLEAR | (_lib.RASTER_CULL_BACKFACES if cull_backfaces else 0)
        _raster_view(lib, ws, vertices_c, faces_c, row, near, flags, stream)
        _lib.check(lib.gsr_raster_resolve(ws.keys.data_ptr(), H, W, depth.data_ptr(), face_id.data_ptr(), stream),
                   "gsr_raster_resolve")
        if stats:
            _, dropped, bad = ws.head()
            return depth, face_id, {"dropped": dropped, "bad_faces": bad}
    return depth, face_id


def face_normal_map(vertices: torch.Tensor, faces: torch.Tensor, face_id: torch.Tensor, camera) -> torch.Tensor:
    """The view-space unit normal of the face that owns each pixel -> float32 ``[3,H,W]``: ``(b - a) x (c - a)`` of the
    face's corners in view space, normalised, flipped so that it points towards the camera (``n . a <= 0``), and 0 where
    ``face_id < 0`` or the face has no area.  ``face_id``: int32 ``[H,W]`` as ``rasterize_mesh`` gives it.  Plain torch
    gathers on the device of ``vertices``: this one is not hot."""
    V, F = _check_mesh(vertices, faces, None, "face_normal_map")
    row, = _raster_rows([camera])
    dev = vertices.device
    if not isinstance(face_id, torch.Tensor) or face_id.dtype != torch.int32 or face_id.device != dev \
            or tuple(face_id.shape) != (row.height, row.width):
        raise ValueError(f"face_id must be an int32 [{row.height},{row.width}] tensor on {dev}, got "
                         f"{getattr(face_id, 'dtype', type(face_id))} {tuple(getattr(face_id, 'shape', ()))} on "
                         f"{getattr(face_id, 'device', None)}")
    out = torch.zeros((3, row.height, row.width), dtype=torch.float32, device=dev)
    if F == 0:
        return out
    M = camera.world_view_transform.detach().to(device=dev, dtype=torch.float32)
    hit = (face_id >= 0) & (face_id < F)
    corners = vertices.detach()[faces.detach()[face_id[hit].to(torch.int64)].to(torch.int64)]          # [n,3,3]
    corners = corners @ M[:3, :3] + M[3, :3]
    a = corners[:, 0]
    n = torch.cross(corners[:, 1] - a, corners[:, 2] - a, dim=1)
    n = torch.where(((n * a).sum(1) > 0)[:, None], -n, n)
    length = n.norm(dim=1, keepdim=True)
    n = torch.where(length > 0, n / length.clamp_min(1e-38), torch.zeros_like(n))
    out.permute(1, 2, 0)[hit] = n
    return out


def _check_face_counts(counts, F: int, dev) -> None:
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32
                               or tuple(counts.shape) != (F,) or counts.device != dev or not counts.is_contiguous()):
        raise ValueError(f"counts must be a contiguous int32 [{F}] tensor on {dev}")


def _count_face_views(vertices, faces, rows, near: float, counts):
    """The launches of ``face_view_counts`` for the rows of ``_raster_rows``, on a device mesh."""
    F, dev = int(faces.shape[0]), vertices.device
    if counts is None:
        counts = torch.zeros(F, dtype=torch.int32, device=dev)
    if F == 0 or not rows:
        return counts
    lib = _lib.load()
    vertices_c, faces_c = vertices.detach().contiguous(), faces.detach().contiguous()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws = _RasterWorkspace(lib, F, max(r.height * r.width for r in rows), dev)        # one key buffer for every view
        stamp = torch.zeros(F, dtype=torch.int32, device=dev)
        for k, row in enumerate(rows):
            _raster_view(lib, ws, vertices_c, faces_c, row, near, _lib.RASTER_CLEAR, stream)
            _lib.check(lib.gsr_raster_count_faces(ws.keys.data_ptr(), row.height, row.width, F, k + 1, stamp.data_ptr(),
                                                  counts.data_ptr(), stream), "gsr_raster_count_faces")
    return counts


def face_view_counts(vertices: torch.Tensor, faces: torch.Tensor, cameras, *, near: float = 0.2,
                     counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In how many views each face owns at least one pixel -> int32 ``[F]`` on the device of the mesh (a ROCm GPU).

    Every camera rasterizes the whole mesh as ``rasterize_mesh`` does (one key buffer, reused from view to view) and
    every face that owns a pixel of the result -- nearest at that pixel centre, smallest index at equal depth -- counts
    once for that view.  A face that is hidden behind others, covers no pixel centre or lies outside every image counts
    nowhere.  ``counts``: an int32 ``[F]`` tensor the views are added into (and that is
    returned), so that views can be fed in chunks; counts over chunks equal counts over one call.  Integer atomics only:
    the same counts from run to run.  Nothing is read back; everything runs on the current stream."""
    V, F = _check_mesh(vertices, faces, None, "face_view_counts")
    near = _raster_scalars(near)
    rows = _raster_rows(cameras)
    _check_face_counts(counts, F, vertices.device)
    _need_gpu(vertices, "face_view_counts")
    return _count_face_views(vertices, faces, rows, near, counts)


def cull_invisible_faces(vertices: torch.Tensor, faces: torch.Tensor, colors: Optional[torch.Tensor] = None, *, cameras,
                         min_views: int = 1, near: float = 0.2, counts: Optional[torch.Tensor] = None,
                         return_counts: bool = False):
    """Remove the faces that too few views see -> ``(vertices float32 [V',3], faces int32 [F',3], colors float32 [V',3] or
    None)``, with ``return_counts=True`` also the ``face_view_counts`` of the input faces; new tensors on the same device
    (csrc/mesh_raster.hip).

    With ``n = face_view_counts(vertices, faces, cameras, near=near, counts=counts)`` a face is kept when
    ``n >= min_views``; then the vertices that no kept face refers to go as well.  ``min_views=1`` removes what no view
    sees: inner walls, shells inside closed objects, the back of a TSDF's truncation band -- by the mesh's own z-buffer,
    so it needs neither the trained model nor a depth tolerance.  ``counts``: counts of earlier chunks of views to add
    to; ``cameras`` may then be empty.

    Kept vertices and faces stay in their original order; the kept vertex and colour rows are bit-copies, the kept faces
    are re-indexed.  Nothing is kept: ``[0,3]`` tensors.  One host read-back (``V'`` and ``F'``, with the check that every
    face index lies in ``0..V-1``, else ``GsrError``).  ``F == 0`` makes no native call.  There is no CPU path."""
    V, F = _check_mesh(vertices, faces, colors, "cull_invisible_faces")
    if isinstance(min_views, bool) or not isinstance(min_views, int) or not 0 <= min_views < 2 ** 31:
        raise ValueError(f"min_views must be a non-negative int that fits an int32, got {min_views!r}")
    if not isinstance(return_counts, bool):
        raise ValueError(f"return_counts must be a bool, got {return_counts!r}")
    near = _raster_scalars(near)
    rows = _raster_rows(cameras)
    dev = vertices.device
    _check_face_counts(counts, F, dev)
    _need_gpu(vertices, "cull_invisible_faces")

    def result(mesh, n):
        if mesh is None:
            mesh = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev),
                    None if colors is None else torch.empty((0, 3), dtype=torch.float32, device=dev))
        return mesh + (n,) if return_counts else mesh

    n = _count_face_views(vertices, faces, rows, near, counts)
    if F == 0:
        return result(None, n)
    lib = _lib.load()
    vertices_c, faces_c = vertices.detach().contiguous(), faces.detach().contiguous()
    colors_c = None if colors is None else colors.detach().contiguous()
    keep = (n >= min_views).to(torch.uint8)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    return result(_compact_kept(lib, vertices_c, colors_c, faces_c, keep, status, "cull_invisible_faces"), n)


__all__ = ["connected_components", "clean_mesh", "simplify_mesh", "dilate_mask", "vertex_view_counts",
           "cull_mesh_by_views", "rasterize_mesh", "face_normal_map", "face_view_counts", "cull_invisible_faces"]
