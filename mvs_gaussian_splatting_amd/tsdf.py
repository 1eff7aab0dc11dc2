"""From a trained model to a surface: fuse rendered depth maps into a dense truncated-signed-distance volume and extract
a triangle mesh, both on the HIP path (``csrc/tsdf.hip`` behind ``gsr_tsdf_integrate`` / ``gsr_tsdf_mesh_count`` /
``gsr_tsdf_mesh_emit``).

    volume = volume_for_points(gaussians.get_xyz, resolution=256)
    fuse_views(scene.getTrainCameras(), gaussians, pipe, background, volume)
    vertices, faces, colors = volume.extract_mesh()
    ply_io.write_ply_mesh("mesh.ply", vertices, faces, colors)

Grid point ``(i, j, k)`` is the sample at ``origin + voxel_size * (i, j, k)``; the fields are stored ``[nz, ny, nx]``
(x fastest) and are public: a field may be loaded into ``volume.tsdf`` / ``volume.weight`` / ``volume.color`` directly.
The extraction is marching tetrahedra on the Kuhn decomposition of every cube; its definitions and output order are in
``TSDFVolume.extract_mesh``.  There is no CPU path: a volume may be built on the CPU to be filled or inspected, but
``integrate`` and ``extract_mesh`` need it on a ROCm GPU.

Unbounded scenes are fused on a grid in contracted space, 2DGS's ``extract_mesh_unbounded``:

    center, radius = bounding_sphere(scene.getTrainCameras())
    volume = contracted_volume_for_points(gaussians.get_xyz, center, radius, resolution=512)
    fuse_views(scene.getTrainCameras(), gaussians, pipe, background, volume)
    vertices, faces, colors = volume.extract_mesh()              # vertices in world space
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from .surface import blend_plane_depth, plane_depth, surface_depth

_INF = float("inf")
_BLOCK_X, _BLOCK_ROWS = 64, 4          # the launch shape of csrc/tsdf.hip (tsdf_grid_blocks)


def _limit(value: Optional[float], name: str) -> float:
    """A missing ``max_depth`` / ``max_weight`` is no limit: ``+inf`` on the device."""
    if value is None:
        return _INF
    value = float(value)
    if not value > 0.0:
        raise ValueError(f"{name} must be positive, got {value}")
    return value


class TSDFVolume:
    """A dense TSDF volume: ``tsdf`` float32 ``[nz,ny,nx]`` (1 = untouched), ``weight`` float32 ``[nz,ny,nx]`` (0) and,
    with ``with_color``, ``color`` float32 ``[nz,ny,nx,3]`` (0), on ``device``."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], sdf_trunc: float,
                 with_color: bool = True, device="cuda"):
        origin = tuple(float(v) for v in origin)
        dims = tuple(int(v) for v in dims)
        if len(origin) != 3 or len(dims) != 3:
            raise ValueError(f"origin and dims have three entries each, got {origin} and {dims}")
        if any(n <= 0 for n in dims):
            raise ValueError(f"dims must be positive, got {dims}")
        nx, ny, nz = dims
        if 7 * nx * ny * nz >= 2 ** 31:
            raise ValueError(f"a volume of {nx} x {ny} x {nz} points overflows the 32-bit index space of its "
                             f"7 edge slots per point (7 * nx * ny * nz must stay below 2^31)")
        if -(-nx // _BLOCK_X) * -(-(ny * nz) // _BLOCK_ROWS) * _BLOCK_X * _BLOCK_ROWS >= 2 ** 32:
            raise ValueError(f"a volume of {nx} x {ny} x {nz} points needs a launch of 2^32 work-items or more: make x "
                             f"the long axis")
        voxel_size, sdf_trunc = float(voxel_size), float(sdf_trunc)
        if not voxel_size > 0.0 or not math.isfinite(voxel_size):
            raise ValueError(f"voxel_size must be positive, got {voxel_size}")
        if not sdf_trunc > 0.0 or not math.isfinite(sdf_trunc):
            raise ValueError(f"sdf_trunc must be positive, got {sdf_trunc}")
        self.origin, self.voxel_size, self.dims, self.sdf_trunc = origin, voxel_size, dims, sdf_trunc
        self.with_color = bool(with_color)
        self.device = torch.device(device)
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((nz, ny, nx, 3), dtype=torch.float32, device=self.device) if self.with_color else None

    # ---- the native view of the volume -------------------------------------------------------------------------------
    def _fields(self):
        nx, ny, nz = self.dims
        want = {"tsdf": (nz, ny, nx), "weight": (nz, ny, nx)}
        if self.with_color:
            want["color"] = (nz, ny, nx, 3)
        for name, shape in want.items():
            t = getattr(self, name)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape \
                    or not t.is_contiguous() or t.device != self.tsdf.device:
                raise ValueError(f"volume.{name} must be a contiguous float32 {list(shape)} tensor on the volume's device")
        return self.tsdf, self.weight, (self.color if self.with_color else None)

    def _native(self) -> "_lib.GsrTsdfVolume":
        tsdf, weight, color = self._fields()
        v = _lib.GsrTsdfVolume()
        v.nx, v.ny, v.nz = self.dims
        v.origin[0], v.origin[1], v.origin[2] = self.origin
        v.voxel_size, v.sdf_trunc = self.voxel_size, self.sdf_trunc
        v.tsdf, v.weight, v.color = tsdf.data_ptr(), weight.data_ptr(), None if color is None else color.data_ptr()
        return v

    def _need_gpu(self, what: str) -> None:
        if not self.tsdf.is_cuda:
            raise _lib.GsrError(f"{what} needs the volume on a ROCm GPU (no CPU path)")

    # ---- fusion --------------------------------------------------------------------------------------------------------
    def integrate(self, depth: torch.Tensor, camera, color: Optional[torch.Tensor] = None, weight: float = 1.0,
                  max_depth: Optional[float] = None, max_weight: Optional[float] = None) -> None:
        """Fuse one view, in one launch.  ``depth`` float32 ``[H,W]`` or ``[1,H,W]``: the view-space depth of every
        pixel, 0 where there is none.  ``camera``: anything with ``world_view_transform``, ``FoVx``, ``FoVy``,
        ``image_width``, ``image_height``.  ``color`` float32 ``[3,H,W]``, given exactly when the volume has a colour
        field.  Per grid point (float32; the order of operations is the header comment of ``csrc/tsdf.hip``): project
        with the view matrix, skip if ``z <= 0.2``; nearest pixel ``floor(u + 0.5)`` with ``u = fx x / z + (W - 1) / 2``,
        skip outside the image; ``d = depth[py, px]``, skip unless ``0 < d <= max_depth``; ``sdf = d - z``, skip if
        ``sdf < -sdf_trunc``; then ``tsdf`` and the colour become the running averages with ``t = min(1, sdf /
        sdf_trunc)`` and the pixel's colour, and ``weight`` grows by ``weight``, clamped to ``max_weight``.  Skipped
        points are not written.  Asynchronous: nothing is read back."""
        H, W = int(camera.image_height), int(camera.image_width)
        dev = self.tsdf.device
        if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.device != dev \
                or tuple(depth.shape) not in ((H, W), (1, H, W)):
            raise ValueError(f"depth must be a float32 [{H},{W}] or [1,{H},{W}] tensor on {dev}, got "
                             f"{getattr(depth, 'dtype', type(depth))} {tuple(getattr(depth, 'shape', ()))} on "
                             f"{getattr(depth, 'device', None)}")
        if self.with_color != (color is not None):
            raise ValueError("color is given exactly when the volume has a colour field (with_color)")
        if color is not None and (not isinstance(color, torch.Tensor) or color.dtype != torch.float32
                                  or color.device != dev or tuple(color.shape) != (3, H, W)):
            raise ValueError(f"color must be a float32 [3,{H},{W}] tensor on {dev}, got "
                             f"{getattr(color, 'dtype', type(color))} {tuple(getattr(color, 'shape', ()))} on "
                             f"{getattr(color, 'device', None)}")
        if H <= 0 or W <= 0:
            raise ValueError("the camera has an empty image")
        weight = float(weight)
        if not weight > 0.0 or not math.isfinite(weight):
            raise ValueError(f"weight must be positive, got {weight}")
        view = _lib.GsrTsdfView()
        view.width, view.height = W, H
        view.fx = W / (2.0 * math.tan(float(camera.FoVx) * 0.5))
        view.fy = H / (2.0 * math.tan(float(camera.FoVy) * 0.5))
        view.weight, view.max_depth, view.max_weight = weight, _limit(max_depth, "max_depth"), _limit(max_weight, "max_weight")
        vol = self._native()
        self._need_gpu("TSDFVolume.integrate")
        viewmatrix = camera.world_view_transform.detach().to(device=dev, dtype=torch.float32).contiguous()
        depth_c = depth.detach().contiguous()
        color_c = None if color is None else color.detach().contiguous()
        view.viewmatrix, view.depth = viewmatrix.data_ptr(), depth_c.data_ptr()
        view.color = None if color_c is None else color_c.data_ptr()
        with torch.cuda.device(dev):
            self._integrate_native(vol, view, torch.cuda.current_stream(dev).cuda_stream)

    def _integrate_native(self, vol, view, stream) -> None:
        _lib.check(_lib.load().gsr_tsdf_integrate(C.byref(vol), C.byref(view), stream), "gsr_tsdf_integrate")

    # ---- extraction ----------------------------------------------------------------------------------------------------
    def extract_mesh(self, min_weight: float = 1e-6) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """Marching tetrahedra -> ``(vertices float32 [V,3], faces int32 [F,3], colors float32 [V,3] or None)`` on the
        device.  Every cube whose eight corners have ``weight >= min_weight`` is split into the six tetrahedra around
        its diagonal from corner ``(0,0,0)`` to ``(1,1,1)``; a sample is inside when ``tsdf < 0``.  Each grid point owns
        the edges that leave it along ``(1,0,0) (0,1,0) (0,0,1) (1,1,0) (0,1,1) (1,0,1) (1,1,1)``; a crossed edge
        carries one vertex at ``p_a + (p_b - p_a) * t_a / (t_a - t_b)``, ``a`` the owner, colours likewise.  Vertices
        are ordered by (owner's linear index, direction), faces by (cube, tetrahedron, triangle); only referenced
        vertices are emitted; normals point from inside to outside; the same bits from run to run.  One host
        synchronisation (the two sizes).  No crossing: ``[0,3]`` tensors."""
        min_weight = float(min_weight)
        if math.isnan(min_weight):
            raise ValueError("min_weight is NaN")
        vol = self._native()
        self._need_gpu("TSDFVolume.extract_mesh")
        lib, dev = _lib.load(), self.tsdf.device
        nx, ny, nz = self.dims
        n = nx * ny * nz
        counts = torch.empty((3, n), dtype=torch.uint8, device=dev)          # triangles, edge mask, vertices per point
        tri, mask, vert = counts[0], counts[1], counts[2]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.gsr_tsdf_mesh_count(C.byref(vol), min_weight, tri.data_ptr(), mask.data_ptr(), vert.data_ptr(),
                                               stream), "gsr_tsdf_mesh_count")
            vert_end = torch.cumsum(vert, dim=0, dtype=torch.int64)
            tri_end = torch.cumsum(tri, dim=0, dtype=torch.int64)
            V, F = (int(v) for v in torch.stack((vert_end[-1], tri_end[-1])).tolist())     # the one read-back
            vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
            colors = torch.empty((V, 3), dtype=torch.float32, device=dev) if self.with_color else None
            if V == 0 or F == 0:
                return vertices[:0], faces[:0], None if colors is None else colors[:0]
            vert_offs, tri_offs = vert_end - vert, tri_end - tri                            # exclusive scans
            _lib.check(lib.gsr_tsdf_mesh_emit(C.byref(vol), tri.data_ptr(), mask.data_ptr(), vert_offs.data_ptr(),
                                              tri_offs.data_ptr(), V, F, vertices.data_ptr(),
                                              None if colors is None else colors.data_ptr(), faces.data_ptr(), stream),
                       "gsr_tsdf_mesh_emit")
        return vertices, faces, colors


Q_MAX = 1.9                            # 2DGS's bound of the contracted grid; the contraction itself ends at |q| = 2


def _contraction(center, radius, q_max) -> Tuple[Tuple[float, float, float], float, float]:
    center = tuple(float(v) for v in center)
    if len(center) != 3 or not all(math.isfinite(v) for v in center):
        raise ValueError(f"center has three finite entries, got {center}")
    radius, q_max = float(radius), float(q_max)
    if not radius > 0.0 or not math.isfinite(radius):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    if not 1.0 < q_max < 2.0:
        raise ValueError(f"q_max must lie in (1, 2), got {q_max}")
    return center, radius, q_max


def contract(x: torch.Tensor) -> torch.Tensor:
    """The Mip-NeRF 360 contraction of normalised points ``x [...,3]``: ``x`` inside the unit ball,
    ``(2 - 1 / |x|) x / |x|`` outside.  Plain torch, in the dtype of ``x``."""
    m = torch.linalg.norm(x, dim=-1, keepdim=True)
    far = m > 1.0
    safe = torch.where(far, m, torch.ones_like(m))
    return torch.where(far, (2.0 - 1.0 / safe) * (x / safe), x)


class ContractedTSDFVolume(TSDFVolume):
    """A ``TSDFVolume`` whose grid lives in contracted space, for unbounded scenes: grid point
    ``(i, j, k)`` is ``q = origin + voxel_size * (i, j, k)`` and stands for the world point ``center + radius * (q * s)``,
    ``s = 1`` for ``m = |q| <= 1`` and ``1 / ((2 - m) m)`` beyond -- the inverse of ``contract((p - center) / radius)``.
    Same fields, layout and index limits as the base.  ``sdf_trunc`` is in world units as it applies inside the unit
    ball; at ``m > 1`` the truncation is ``sdf_trunc / (2 - m)``.  Grid points with ``|q| >= q_max`` are never touched."""

    def __init__(self, origin: Sequence[float], voxel_size: float, dims: Sequence[int], sdf_trunc: float,
                 center: Sequence[float], radius: float, q_max: float = Q_MAX, with_color: bool = True, device="cuda"):
        self.center, self.radius, self.q_max = _contraction(center, radius, q_max)
        super().__init__(origin, voxel_size, dims, sdf_trunc, with_color=with_color, device=device)

    def _native_contraction(self) -> "_lib.GsrTsdfContraction":
        c = _lib.GsrTsdfContraction()
        c.center[0], c.center[1], c.center[2] = self.center
        c.radius, c.q_max = self.radius, self.q_max
        return c

    def _integrate_native(self, vol, view, stream) -> None:
        con = self._native_contraction()
        _lib.check(_lib.load().gsr_tsdf_integrate_contracted(C.byref(vol), C.byref(con), C.byref(view), stream),
                   "gsr_tsdf_integrate_contracted")

    def extract_mesh(self, min_weight: float = 1e-6, contracted: bool = False):
        """``TSDFVolume.extract_mesh`` on the contracted grid, then every vertex through the inverse contraction, in
        place, in one launch (``gsr_tsdf_uncontract_points``); faces and colours are the base's.  ``contracted=True``
        returns the vertices in grid coordinates, as the base would."""
        vertices, faces, colors = super().extract_mesh(min_weight)
        if not contracted and vertices.shape[0] > 0:
            con = self._native_contraction()
            with torch.cuda.device(vertices.device):
                stream = torch.cuda.current_stream(vertices.device).cuda_stream
                _lib.check(_lib.load().gsr_tsdf_uncontract_points(vertices.data_ptr(), int(vertices.shape[0]),
                                                                  C.byref(con), stream), "gsr_tsdf_uncontract_points")
        return vertices, faces, colors


def bounding_sphere(cameras) -> Tuple[Tuple[float, float, float], float]:
    """2DGS's ``estimate_bounding_sphere``: ``center`` is the least-squares point nearest all optical axes and ``radius``
    the smallest camera distance from it.  Per camera, from ``world_view_transform`` (row-vector convention), ``o`` the
    position and ``d`` the unit view direction: ``A_i = (I - d d^T)^T (I - d d^T)``, ``center = (mean A_i)^-1 mean(A_i o)``.
    Host, float64.  ``ValueError`` for fewer than two cameras and for a singular system (parallel axes)."""
    import numpy as np
    cameras = list(cameras)
    if len(cameras) < 2:
        raise ValueError(f"bounding_sphere needs at least two cameras, got {len(cameras)}")
    A_sum, b_sum, origins = np.zeros((3, 3)), np.zeros(3), []
    for cam in cameras:
        M = cam.world_view_transform.detach().to(device="cpu", dtype=torch.float64).numpy()
        c2w = np.linalg.inv(M[:3, :3])                 # rows: the camera's axes in the world
        o = -M[3, :3] @ c2w
        d = c2w[2] / np.linalg.norm(c2w[2])
        P = np.eye(3) - np.outer(d, d)
        A = P.T @ P
        A_sum += A
        b_sum += A @ o
        origins.append(o)
    A_mean, b_mean = A_sum / len(cameras), b_sum / len(cameras)
    if np.linalg.cond(A_mean) > 1e12:
        raise ValueError("the optical axes are parallel: no point is nearest all of them")
    center = np.linalg.solve(A_mean, b_mean)
    radius = float(np.linalg.norm(np.asarray(origins) - center, axis=1).min())
    if not radius > 0.0:
        raise ValueError("a camera sits at the centre of the optical axes: the sphere has no radius")
    return tuple(float(v) for v in center), radius


def contracted_volume_for_points(xyz: torch.Tensor, center: Sequence[float], radius: float, *, resolution: int = 512,
                                 quantile: float = 0.95, sdf_trunc: Optional[float] = None, q_max: float = Q_MAX,
                                 with_color: bool = True, device=None) -> ContractedTSDFVolume:
    """2DGS's box for an unbounded scene: with ``R = min(quantile of |contract((xyz - center) / radius)| + 0.01, 1.9)``
    (the quantile interpolated linearly between neighbours) the cube ``[-R, R]^3`` of contracted space with
    ``resolution`` samples per side, ``voxel_size = 2 R / (resolution - 1)``.  ``sdf_trunc`` defaults to 5 world voxels,
    ``5 * radius * voxel_size``.  Plain torch; one read-back."""
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"xyz must be [P,3] with P > 0, got {tuple(xyz.shape)}")
    center, radius, q_max = _contraction(center, radius, q_max)
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError("resolution must be at least 2")
    if not 0.0 <= quantile <= 1.0:
        raise ValueError(f"quantile must lie in [0, 1], got {quantile}")
    pts = xyz.detach().to(torch.float32)
    x = (pts - torch.tensor(center, dtype=torch.float32, device=pts.device)) / radius
    norms = torch.sort(torch.linalg.norm(contract(x), dim=-1)).values
    at = quantile * (norms.shape[0] - 1)
    lo_v, hi_v = norms[[int(math.floor(at)), int(math.ceil(at))]].tolist()         # the one read-back
    R = min(lo_v + (hi_v - lo_v) * (at - math.floor(at)) + 0.01, 1.9)
    voxel_size = 2.0 * R / (resolution - 1)
    return ContractedTSDFVolume((-R, -R, -R), voxel_size, (resolution,) * 3,
                                5.0 * radius * voxel_size if sdf_trunc is None else sdf_trunc, center, radius, q_max,
                                with_color=with_color, device=xyz.device if device is None else device)


def render_surface(renderer, camera, model, pipe, bg, alpha_min: float, depth_ratio: float,
                   unbiased_depth: bool = False):
    """One view's surface depth as ``fuse_views`` integrates it -> ``(depth [1,H,W], the renderer's package)``: at
    ``depth_ratio`` 0 the expected depth ``depth / alpha`` where ``alpha >= alpha_min`` and 0 elsewhere, from
    ``renderer(camera, model, pipe, bg, return_depth=True)``; above 0 ``surface.surface_depth`` of a frame rendered with
    ``return_median_depth=True`` as well.  ``unbiased_depth``: the frame is rendered with ``return_plane_depth=True`` and
    PGSR's unbiased depth -- the frame's ``"plane_depth"`` at ``alpha_min`` 0.5, ``surface.plane_depth(normal, distance,
    alpha, ..., alpha_min)`` of its maps otherwise; 0 where it has no surface -- stands where the expected depth stood, the median blended into it by ``surface.blend_plane_depth``."""
    if unbiased_depth:
        pkg = renderer(camera, model, pipe, bg, return_plane_depth=True,
                       **({"return_median_depth": True} if depth_ratio > 0.0 else {}))
        plane = pkg["plane_depth"]                       # render's own map: alpha_min 0.5
        if alpha_min != 0.5:
            plane = plane_depth(pkg["normal"], pkg["distance"], pkg["alpha"], math.tan(camera.FoVx * 0.5),
                                math.tan(camera.FoVy * 0.5), alpha_min)
        return blend_plane_depth(plane, pkg["median_depth"] if depth_ratio > 0.0 else None, depth_ratio), pkg
    if depth_ratio > 0.0:
        pkg = renderer(camera, model, pipe, bg, return_depth=True, return_median_depth=True)
        return surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], depth_ratio, alpha_min), pkg
    pkg = renderer(camera, model, pipe, bg, return_depth=True)
    depth, alpha = pkg["depth"], pkg["alpha"]
    return torch.where(alpha >= alpha_min, depth / alpha, torch.zeros_like(depth)), pkg


def fuse_views(cameras, model, pipe, bg, volume: TSDFVolume, *, alpha_min: float = 0.5,
               max_depth: Optional[float] = None, renderer=None, depth_ratio: float = 0.0,
               consistency: Optional[dict] = None, unbiased_depth: bool = False) -> TSDFVolume:
    """Render every camera with ``renderer(camera, model, pipe, bg, return_depth=True)`` (default: ``render``) under
    ``no_grad`` and integrate its expected depth ``depth / alpha`` where ``alpha >= alpha_min`` (0, invalid, elsewhere)
    with the rendered colour.  No host synchronisation per view.
    depth_ratio (2DGS's, in [0, 1]; it meshes bounded scenes at 1): above 0 the frames are rendered with
    ``return_median_depth=True`` as well and ``surface.surface_depth(depth, alpha, median, depth_ratio, alpha_min)`` is
    integrated -- at 1 the median depth, which lies on a surface at a depth edge where the expected depth floats between
    two.  At 0 the renderer is called with exactly the keyword arguments above.
    consistency (default None: every pixel above is integrated, view by view as it is rendered): a dict with any of
    ``n_sources`` (4), ``min_views`` (2), ``pix_thresh`` (1.0), ``depth_thresh`` (0.01), ``max_angle_deg`` (60.0) turns on
    the multi-view geometric consistency filter of ``mvs.py``, in two passes.  The first renders every
    view and keeps its surface depth and, if the volume has colour, its image on the device: ``N H W (4 + 12)`` bytes
    for ``N`` views of ``H x W`` pixels (``4 N H W`` without colour).  The second checks each view against its
    ``mvs.select_source_views`` and integrates the view's own depth with the pixels of ``count < min_views`` set to 0:
    floaters, depth that hangs between two surfaces at a silhouette and fog in front of a wall, which no neighbour
    confirms, never reach the volume.
    unbiased_depth (default False: exactly the calls above): the frames are rendered with ``return_plane_depth=True`` and
    PGSR's unbiased depth ``surface.plane_depth`` is what is integrated (``render_surface``): on a slanted
    surface it lies on the surface where the expected depth bends towards the camera.  The first frame of each camera
    copies its view matrix and centre to the host (``features.gaussian_planes``): one synchronisation per camera."""
    if not (isinstance(depth_ratio, (int, float)) and 0.0 <= depth_ratio <= 1.0):
        raise ValueError(f"depth_ratio must lie in [0, 1], got {depth_ratio!r}")
    if consistency is not None:
        from .mvs import consistency_options, filter_views
        options = consistency_options(consistency)
    if renderer is None:
        from .renderer import render as renderer
    with torch.no_grad():
        if consistency is None:
            for camera in cameras:
                expected, pkg = render_surface(renderer, camera, model, pipe, bg, alpha_min, depth_ratio,
                                               **({"unbiased_depth": True} if unbiased_depth else {}))
                volume.integrate(expected, camera, color=pkg["render"] if volume.with_color else None, max_depth=max_depth)
            return volume
        cameras = list(cameras)
        depths, colors = [], []
        for camera in cameras:
            expected, pkg = render_surface(renderer, camera, model, pipe, bg, alpha_min, depth_ratio,
                                               **({"unbiased_depth": True} if unbiased_depth else {}))
            depths.append(expected)
            colors.append(pkg["render"] if volume.with_color else None)
        for camera, depth, color, (count, _) in zip(cameras, depths, colors, filter_views(cameras, depths, **options)):
            kept = torch.where((count >= options["min_views"]).view(depth.shape), depth, torch.zeros_like(depth))
            volume.integrate(kept, camera, color=color, max_depth=max_depth)
    return volume


def view_counts_for_views(cameras, model, pipe, bg, vertices: torch.Tensor, *, masks=None, occlusion: bool = True,
                          chunk: int = 16, alpha_min: float = 0.5, renderer=None, depth_ratio: float = 0.0,
                          unbiased_depth: bool = False, near: float = 0.2, depth_tol: float = 0.01):
    """``mesh.vertex_view_counts`` of ``vertices`` over the training views, with each view's own rendered surface as its
    depth map -> ``(in_view int32 [V], visible int32 [V])``: what ``mesh.cull_mesh_by_views(counts=...)`` culls by.
    The views are taken ``chunk`` at a time: a chunk's surfaces are rendered under ``no_grad`` with ``render_surface``
    (``alpha_min``, ``depth_ratio``, ``unbiased_depth`` and ``renderer`` as ``fuse_views`` takes them), counted into the
    running counts and freed, so at most ``chunk`` depth maps are alive and the counts equal those of one table over all
    views.  ``occlusion=False`` renders nothing: only the images' frames and ``masks`` (``None`` or one entry per camera)
    count.  No host synchronisation beyond ``vertex_view_counts``' own."""
    from .mesh import vertex_view_counts
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"chunk must be a positive int, got {chunk!r}")
    if not isinstance(occlusion, bool):
        raise ValueError(f"occlusion must be a bool, got {occlusion!r}")
    if not (isinstance(depth_ratio, (int, float)) and 0.0 <= depth_ratio <= 1.0):
        raise ValueError(f"depth_ratio must lie in [0, 1], got {depth_ratio!r}")
    cameras = list(cameras)
    if masks is not None:
        masks = list(masks)
        if len(masks) != len(cameras):
            raise ValueError(f"{len(masks)} masks for {len(cameras)} cameras")
    if renderer is None and occlusion:
        from .renderer import render as renderer
    counts = None
    with torch.no_grad():
        for at in range(0, len(cameras), chunk):
            some = cameras[at:at + chunk]
            depths = None
            if occlusion:
                depths = [render_surface(renderer, camera, model, pipe, bg, alpha_min, depth_ratio,
                                         **({"unbiased_depth": True} if unbiased_depth else {}))[0] for camera in some]
            counts = vertex_view_counts(vertices, some, masks=None if masks is None else masks[at:at + chunk],
                                        depths=depths, near=near, depth_tol=depth_tol, counts=counts)
            del depths
        if counts is None:                  # no cameras: zeros, through the same checks
            counts = vertex_view_counts(vertices, [], near=near, depth_tol=depth_tol)
    return counts


def volume_for_points(xyz: torch.Tensor, *, voxel_size: Optional[float] = None, resolution: Optional[int] = None,
                      margin: float = 0.05, quantile: float = 0.01, sdf_trunc: Optional[float] = None,
                      with_color: bool = True, device=None) -> TSDFVolume:
    """A volume around the model's positions ``xyz [P,3]``: per axis the ``quantile`` .. ``1 - quantile`` range of the
    coordinates (outliers of a trained model would blow the box up), widened on both sides by ``margin`` times the
    longest side.  Give the ``voxel_size``, or the ``resolution``: the number of samples along the longest side
    (default 256).  ``sdf_trunc`` defaults to 4 voxels.  Plain torch; one read-back of the six bounds."""
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.shape[0] == 0:
        raise ValueError(f"xyz must be [P,3] with P > 0, got {tuple(xyz.shape)}")
    if voxel_size is not None and resolution is not None:
        raise ValueError("give voxel_size or resolution, not both")
    if not 0.0 <= quantile < 0.5 or margin < 0.0:
        raise ValueError("quantile must lie in [0, 0.5) and margin must not be negative")
    pts = xyz.detach().to(torch.float32)
    P = int(pts.shape[0])
    ordered = torch.sort(pts, dim=0).values
    lo_i = min(P - 1, int(math.floor(quantile * (P - 1))))
    lo, hi = ordered[lo_i].tolist(), ordered[P - 1 - lo_i].tolist()
    longest = max(h - l for l, h in zip(lo, hi))
    if not longest > 0.0:
        raise ValueError("the points span no volume")
    pad = margin * longest
    lo, hi = [v - pad for v in lo], [v + pad for v in hi]
    if voxel_size is None:
        resolution = 256 if resolution is None else int(resolution)
        if resolution < 2:
            raise ValueError("resolution must be at least 2")
        voxel_size = (longest + 2.0 * pad) / (resolution - 1)
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError(f"voxel_size must be positive, got {voxel_size}")
    dims = tuple(max(2, int(math.ceil((h - l) / voxel_size - 1e-9)) + 1) for l, h in zip(lo, hi))
    return TSDFVolume(lo, voxel_size, dims, 4.0 * voxel_size if sdf_trunc is None else sdf_trunc, with_color=with_color,
                      device=xyz.device if device is None else device)


__all__ = ["TSDFVolume", "ContractedTSDFVolume", "fuse_views", "volume_for_points", "contracted_volume_for_points",
           "bounding_sphere", "contract", "view_counts_for_views"]
