"""CPU-side checks of the mesh rasterizer (csrc/mesh_raster.hip; ``mesh.rasterize_mesh``, ``mesh.face_normal_map``,
``mesh.face_view_counts``, ``mesh.cull_invisible_faces``): the ABI and every refusal of the entry points
and of the Python functions -- which all come before a GPU is asked for -- the kernels' own rule built by the host compiler
(csrc/mesh_raster_math.h through tests/mesh_raster_host_check.cpp) against the numpy restatement the GPU tests compare
with (tests/mesh_raster_restate.py), the properties of the rule itself on inputs that are exact in float32, and the
condition on the general scene that makes its comparison mean something."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_raster_restate as R

ENTRY_POINTS = ("gsr_raster_view", "gsr_raster_resolve", "gsr_raster_count_faces")
PUBLIC = ("rasterize_mesh", "face_normal_map", "face_view_counts", "cull_invisible_faces")


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_abi_is_at_least_42():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib, mesh
    for name in PUBLIC:
        assert getattr(pkg, name) is getattr(mesh, name) and name in pkg.__all__ and name in mesh.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\bint " + name + r"\(", header), name
    assert hasattr(raw, "gsr_raster_queue_bytes") and "gsr_raster_queue_bytes" in _lib.SYMBOLS
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 42
    for name, value in (("GSR_RASTER_MAX_SIDE", _lib.RASTER_MAX_SIDE), ("GSR_RASTER_LANE_PIXELS", _lib.RASTER_LANE_PIXELS),
                        ("GSR_RASTER_DRAIN_WAVES", _lib.RASTER_DRAIN_WAVES)):
        assert int(re.search(r"#define " + name + r" (\d+)", header).group(1)) == value, name
    assert (R.LANE_PIXELS, R.DRAIN_WAVES) == (_lib.RASTER_LANE_PIXELS, _lib.RASTER_DRAIN_WAVES)
    for name, value in (("CLEAR", 1), ("CULL_BACKFACES", 2), ("NO_LOAD_SKIP", 4)):
        assert getattr(_lib, "RASTER_" + name) == value and re.search(r"GSR_RASTER_%s = %d\b" % (name, value), header)
    assert lib.gsr_raster_queue_bytes(0) == 256 and lib.gsr_raster_queue_bytes(100) == 256 + 1024
    assert lib.gsr_raster_queue_bytes(-1) == 0 and lib.gsr_raster_queue_bytes(2 ** 31) == 0
    makefile = open(os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "Makefile")).read()
    assert re.search(r"CONTRACT_OFF_OBJS \+= mesh_raster\.o", makefile) and "mesh_raster_math.h" in makefile
    assert re.search(r"^OBJS = .*\bmesh_raster\.o", makefile, re.M)


def test_every_entry_point_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 4096)()
    p = C.addressof(buf)
    big = 2 ** 31
    BAD, CAPACITY, ALIGN = -1, -2, -3
    nan, inf = float("nan"), float("inf")

    def view(W=8, H=6):
        row = _lib.GsrCullView()
        row.width, row.height, row.fx, row.fy = W, H, 10.0, 10.0
        row.world_to_view[:] = np.eye(4).reshape(-1).tolist()
        return C.byref(row)

    F = 4
    qbytes = lib.gsr_raster_queue_bytes(F)
    good = dict(vertices=p, V=12, faces=p, F=F, view=view(), near=0.2, flags=1, keys=p, queue=p, qbytes=qbytes, scratch=None)
    call = lambda **kw: lib.gsr_raster_view(*{**good, **kw}.values(), None)      # noqa: E731
    for name in ("vertices", "faces", "view", "keys", "queue"):
        assert call(**{name: None}) == BAD, name
    assert b"NULL" in lib.gsr_last_error()
    for kw in ({"V": -1}, {"V": big}, {"F": -1}, {"F": big}):
        assert call(**kw) == BAD, kw
    for W, H in ((0, 6), (8, 0), (-1, 6), (2 ** 14 + 1, 4), (4, 2 ** 14 + 1)):
        assert call(view=view(W, H)) == BAD, (W, H)
    for near in (0.0, -1.0, nan, inf):
        assert call(near=near) == BAD, near
    for flags in (8, -1, 16 | 1):
        assert call(flags=flags) == BAD, flags
    for name in ("vertices", "faces", "scratch"):
        assert call(**{name: p + 2}) == ALIGN, name
    for name in ("keys", "queue"):
        assert call(**{name: p + 4}) == ALIGN, name
    assert call(qbytes=qbytes - 1) == CAPACITY and call(qbytes=0) == CAPACITY
    assert b"queue" in lib.gsr_last_error()

    resolve = lib.gsr_raster_resolve
    good = [p, 6, 8, p, p]
    for n in (0, 3, 4):
        assert resolve(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    for H, W in ((0, 8), (6, 0), (-1, 8), (2 ** 14 + 1, 8), (8, 2 ** 14 + 1)):
        assert resolve(p, H, W, p, p, None) == BAD, (H, W)
    assert resolve(p + 4, 6, 8, p, p, None) == ALIGN and resolve(p, 6, 8, p + 2, p, None) == ALIGN
    assert resolve(p, 6, 8, p, p + 2, None) == ALIGN

    count = lib.gsr_raster_count_faces
    q = p + 1024
    good = [p, 6, 8, 4, 1, p, q]
    for n in (0, 5, 6):
        assert count(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    for H, W in ((0, 8), (6, 0), (2 ** 14 + 1, 8)):
        assert count(p, H, W, 4, 1, p, q, None) == BAD, (H, W)
    for F in (-1, big):
        assert count(p, 6, 8, F, 1, p, q, None) == BAD, F
    for stamp in (0, -1):
        assert count(p, 6, 8, 4, stamp, p, q, None) == BAD, stamp
    assert count(p, 6, 8, 4, 1, p, p, None) == BAD and b"stamp" in lib.gsr_last_error()
    assert count(p + 4, 6, 8, 4, 1, p, q, None) == ALIGN and count(p, 6, 8, 4, 1, p + 2, q, None) == ALIGN
    assert count(p, 6, 8, 0, 1, None, None, None) == 0                    # F = 0 launches nothing


def _cam(W=8, H=6):
    return R.camera(np.eye(4), W, H, 10.0, 10.0)


def test_python_refusals_come_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, cull_invisible_faces, face_normal_map, face_view_counts, rasterize_mesh
    vertices = torch.zeros(4, 3)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    cam, cams = _cam(), [_cam(), _cam(5, 7)]
    ids = torch.zeros(6, 8, dtype=torch.int32)
    ns = types.SimpleNamespace

    for bad in (vertices.double(), torch.zeros(4, 2), torch.zeros(12), vertices.numpy(), None):
        with pytest.raises(ValueError, match="vertices"):
            rasterize_mesh(bad, faces, cam)
        with pytest.raises(ValueError, match="vertices"):
            face_view_counts(bad, faces, cams)
        with pytest.raises(ValueError, match="vertices"):
            cull_invisible_faces(bad, faces, cameras=cams)
        with pytest.raises(ValueError, match="vertices"):
            face_normal_map(bad, faces, ids, cam)
    for bad in (faces.long(), faces.reshape(-1), faces[:, :2], None, faces.to("meta")):
        with pytest.raises(ValueError):
            rasterize_mesh(vertices, bad, cam)
        with pytest.raises(ValueError):
            face_view_counts(vertices, bad, cams)
        with pytest.raises(ValueError):
            cull_invisible_faces(vertices, bad, cameras=cams)
    with pytest.raises(ValueError, match="num_vertices is 0"):
        rasterize_mesh(vertices[:0], faces, cam)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="near"):
            rasterize_mesh(vertices, faces, cam, near=bad)
        with pytest.raises(ValueError, match="near"):
            face_view_counts(vertices, faces, cams, near=bad)
        with pytest.raises(ValueError, match="near"):
            cull_invisible_faces(vertices, faces, cameras=cams, near=bad)
    for name in ("cull_backfaces", "stats"):
        for bad in (1, 0, None, "yes"):
            with pytest.raises(ValueError, match=name):
                rasterize_mesh(vertices, faces, cam, **{name: bad})
    with pytest.raises(ValueError, match="4 x 4"):
        rasterize_mesh(vertices, faces, ns(world_view_transform=torch.eye(3), FoVx=1.0, FoVy=1.0, image_width=8, image_height=6))
    with pytest.raises(ValueError, match="empty image"):
        rasterize_mesh(vertices, faces, ns(world_view_transform=torch.eye(4), FoVx=1.0, FoVy=1.0, image_width=0, image_height=6))
    with pytest.raises(ValueError, match="2\\^14 a side"):
        face_view_counts(vertices, faces, [cam, ns(world_view_transform=torch.eye(4), FoVx=1.0, FoVy=1.0, image_width=2 ** 14 + 1,
                                                   image_height=2)])
    with pytest.raises(ValueError, match="cameras"):
        face_view_counts(vertices, faces, 5)
    with pytest.raises(TypeError):
        rasterize_mesh(vertices, faces, cam, 0.2)                          # the options are given by keyword
    with pytest.raises(TypeError):
        cull_invisible_faces(vertices, faces)                             # the cameras have no default
    ok = torch.zeros(2, dtype=torch.int32)
    for bad in ((ok, ok), ok.long(), torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)[::2], ok.to("meta"),
                ok.numpy()):
        with pytest.raises(ValueError, match="counts"):
            face_view_counts(vertices, faces, cams, counts=bad)
        with pytest.raises(ValueError, match="counts"):
            cull_invisible_faces(vertices, faces, cameras=cams, counts=bad)
    for bad in (torch.zeros(3, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, device="meta")):
        with pytest.raises(ValueError, match="colors"):
            cull_invisible_faces(vertices, faces, bad, cameras=cams)
    for bad in (-1, 1.0, True, None, "all", 2 ** 31):
        with pytest.raises(ValueError, match="min_views"):
            cull_invisible_faces(vertices, faces, cameras=cams, min_views=bad)
    with pytest.raises(ValueError, match="return_counts"):
        cull_invisible_faces(vertices, faces, cameras=cams, return_counts=1)
    for bad in (ids.long(), ids[:5], ids.T, ids.numpy(), None, ids.to("meta")):
        with pytest.raises(ValueError, match="face_id"):
            face_normal_map(vertices, faces, bad, cam)

    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        rasterize_mesh(vertices, faces, cam, near=0.5, cull_backfaces=True, stats=True)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        rasterize_mesh(vertices[:0], faces[:0], cam)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        face_view_counts(vertices, faces, cams, counts=ok)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        face_view_counts(vertices, faces, [])
    for kw in ({}, {"min_views": 0, "return_counts": True}, {"counts": ok, "min_views": 3}):
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            cull_invisible_faces(vertices, faces, torch.zeros(4, 3), cameras=cams, **kw)


def test_face_normal_map_is_plain_gathers():
    """Not hot, so plain torch: the normals of two faces seen from the identity camera, flipped towards it."""
    from mvs_gaussian_splatting_amd import face_normal_map
    vertices = torch.tensor([[0, 0, 2], [1, 0, 2], [0, 1, 2], [0, 0, 3], [0, 1, 4], [1, 0, 3]], dtype=torch.float32)
    faces = torch.tensor([[0, 1, 2], [3, 4, 5], [0, 0, 1]], dtype=torch.int32)
    ids = torch.tensor([[0, 1], [-1, 2]], dtype=torch.int32)
    n = face_normal_map(vertices, faces, ids, R.camera(np.eye(4), 2, 2, 1.0, 1.0))
    assert tuple(n.shape) == (3, 2, 2) and n.dtype == torch.float32
    assert torch.equal(n[:, 0, 0], torch.tensor([0.0, 0.0, -1.0])), "both windings face the camera"
    assert torch.allclose(n[:, 0, 1], torch.tensor([0.0, 1.0, -1.0]) / 2 ** 0.5), "(0, 1, 1) x (1, 0, 0), normalised"
    assert float((n[:, 0, 1] * vertices[3]).sum()) < 0, "towards the camera"
    assert not n[:, 1, 0].any() and not n[:, 1, 1].any(), "no face, and a face without area"


# ---- the kernels' rule on the host -------------------------------------------------------------------------------------
def _scene_bytes(s, cull):
    H, W, fx, fy = R.focal(s.cam)
    return b"".join((struct.pack("<iiiii", len(s.vertices), len(s.faces), W, H, int(cull)), struct.pack("<fff", s.near, fx, fy),
                     s.cam.world_view_transform.numpy().astype("<f4").tobytes(),
                     np.ascontiguousarray(s.vertices, dtype="<f4").tobytes(), np.ascontiguousarray(s.faces, dtype="<i4").tobytes()))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """``csrc/mesh_raster_math.h`` built by the host compiler from ``tests/mesh_raster_host_check.cpp`` into a program of
    its own, with the kernels' ``-ffp-contract=off``."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    folder = tmp_path_factory.mktemp("mesh_raster_host")
    exe = str(folder / "mesh_raster_host_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mesh_raster_host_check.cpp"), "-o", exe], check=True)

    def run(s, cull=False):
        path = str(folder / "scene.bin")
        with open(path, "wb") as f:
            f.write(_scene_bytes(s, cull))
        lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
        pieces = [tuple(l.split()[1:]) for l in lines if l.startswith("P ")]
        keys = np.array([int(l.split()[1], 16) for l in lines if l.startswith("K ")], dtype=np.uint64)
        return pieces, keys
    return run


def _restated_pieces(s, cull):
    """The lines the host program prints, from the restatement."""
    H, W, _, _ = R.focal(s.cam)
    out = []
    for f, mine in enumerate(R.pieces_of(s.vertices, s.faces, s.cam, s.near)):
        for piece in mine:
            n = None if piece is None else R.normalise(piece, cull)
            if n is None:
                out.append((str(f), "-1" if piece is None else "0") + ("0",) * 8)
                continue
            X, Y, _, _ = n
            iy, ix, z = R.cover(piece, W, H, cull)
            keys = z.view(np.uint32).astype(np.uint64) << np.uint64(32) | np.uint64(f)
            total = int(keys.astype(object).sum()) % 2 ** 64 if len(keys) else 0
            out.append((str(f), "1") + tuple(str(c) for k in range(3) for c in (X[k], Y[k])) + (str(len(iy)), "%x" % total))
    return out


SCENES = {"general": R.general_soup, "dyadic": R.dyadic_soup, "dyadic_permuted": lambda: R.dyadic_soup(permute=True, seed=4),
          "big": R.big_triangle_scene, "queued": R.queued_scene}


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("cull", [False, True])
def test_host_build_of_the_rule_gives_the_restatements_bits(host_check, name, cull):
    s = SCENES[name]()
    pieces, keys = host_check(s, cull)
    want = _restated_pieces(s, cull)
    assert len(pieces) == len(want) >= 300
    assert pieces == want, "snapped coordinates, coverage and the covered centres' depth bits, piece by piece"
    r = R.rasterize(s.vertices, s.faces, s.cam, s.near, cull)
    assert np.array_equal(keys, r.keys.reshape(-1)), "and the z-buffer"
    assert (r.face_id >= 0).sum() > 100
    if name.startswith("dyadic") or name == "general":
        assert len(s.faces) == 2000 and len(pieces) > 1000
        assert name == "general" or "0" in [p[1] for p in pieces], "pieces without area"
        assert len(pieces) > len({p[0] for p in pieces}), "faces that the near plane cuts into two pieces"


# ---- the inputs --------------------------------------------------------------------------------------------------------
def test_dyadic_inputs_are_exact_and_hold_the_cases_they_are_named_for():
    for s in (R.dyadic_soup(), R.dyadic_soup(permute=True, seed=4), R.big_triangle_scene(), R.queued_scene()):
        p32 = R.pieces_of(s.vertices, s.faces, s.cam, s.near, np.float32)
        p64 = R.pieces_of(s.vertices, s.faces, s.cam, s.near, np.float64)
        assert len(p32) == len(p64) == len(s.faces)
        for a, b in zip(p32, p64):
            assert len(a) == len(b)
            for p, q in zip(a, b):
                assert (p is None) == (q is None) and (p is None or (p[0] == q[0] and p[1] == q[1] and np.array_equal(p[2], q[2])))
        assert not R.fragile_pixels(s.vertices, s.faces, s.cam, s.near).any()
    s = R.dyadic_soup()
    H, W, _, _ = R.focal(s.cam)
    assert (W, H) == (97, 61) and W % 64 != 0 and len(s.faces) == 2000
    pieces = R.pieces_of(s.vertices, s.faces, s.cam, s.near)
    counts = [len(p) for p in pieces]
    assert counts.count(0) >= 40 and counts.count(2) >= 25 and sum(1 for k in range(s.base + 40, s.base + 100) if counts[k] == 1) >= 25
    assert np.isnan(s.vertices).sum() == 1 and pieces[-1] and all(p is None for p in pieces[-1]), "a NaN corner drops its pieces"
    flat = sum(1 for p in pieces[s.base + 100:s.base + 120] if R.normalise(p[0]) is None)
    assert flat == 20, "zero-area faces"
    r = R.rasterize(s.vertices, s.faces, s.cam, s.near)
    assert r.dropped == len(pieces[-1]) and (r.layers > 1).sum() > 500 and r.queued > 50
    dup = [(7 * k + 3, s.base + 120 + k) for k in range(39)]
    owners = set(np.unique(r.face_id))
    assert any(a in owners for a, _ in dup) and not any(b in owners for _, b in dup), "of coincident faces the smaller index wins"
    # the two scenes of the large-piece path
    b = R.big_triangle_scene()
    rb = R.rasterize(b.vertices, b.faces, b.cam, b.near)
    assert (rb.face_id >= 0).all() and (rb.face_id == b.big).sum() > 1000 and (rb.face_id != b.big).sum() > 500
    q = R.queued_scene()
    rq = R.rasterize(q.vertices, q.faces, q.cam, q.near)
    assert rq.queued > R.DRAIN_WAVES, "more queued pieces than one pass of the drain grid takes"


def test_fragile_share_of_the_general_soup_is_under_one_percent():
    """A condition on the input: were it not to hold, the exact comparison of the GPU test would cover too little."""
    s = R.general_soup()
    r = R.rasterize(s.vertices, s.faces, s.cam, s.near)
    fragile = R.fragile_pixels(s.vertices, s.faces, s.cam, s.near)
    covered = r.layers > 0
    share = fragile.sum() / covered.sum()
    print(f"[mesh_raster] general soup: {int(fragile.sum())} fragile of {int(covered.sum())} covered pixels ({100 * share:.3f} %), "
          f"{r.dropped} dropped, {r.queued} queued, up to {int(r.layers.max())} layers")
    assert covered.sum() > 0.5 * covered.size and r.layers.max() >= 3
    assert share < 0.01
    counts = [len(p) for p in R.pieces_of(s.vertices, s.faces, s.cam, s.near)]
    assert counts.count(0) >= 5 and counts.count(2) >= 5 and r.queued > 20


# ---- properties of the rule, on inputs that are exact ------------------------------------------------------------------
def _layers(tris, W=16, H=12, f=16.0, cull=False):
    cam, _ = R.dyadic_camera(W, H, f)
    vertices, faces = R.soup_mesh(tris)
    return R.rasterize(vertices, faces, cam, R.NEAR, cull)


def _px(x, y, z, W=16, H=12, f=16.0):
    """The view-space point that lands on pixel (x, y) at depth z."""
    return ((x - (W - 1) / 2) * z / f, (y - (H - 1) / 2) * z / f, z)


def test_a_shared_edge_through_pixel_centres_is_covered_exactly_once():
    for (a, b) in (((2, 2), (10, 10)), ((2, 9), (11, 0)), ((3, 1), (3, 10)), ((1, 4), (13, 4)), ((2, 2), (12, 7))):
        for z in (1.0, 2.0):
            for flip in (False, True):
                p, q = _px(*a, z), _px(*b, z)
                left, right = _px(a[0] - 3, b[1] + 2, z), _px(b[0] + 4, a[1] - 1, z)
                one, two = (p, q, left), ((q, p, right) if not flip else (p, q, right))
                r = _layers(np.array((one, two)))
                n = max(abs(b[0] - a[0]), abs(b[1] - a[1]))
                on_edge = [(a[1] + (b[1] - a[1]) * k // n, a[0] + (b[0] - a[0]) * k // n) for k in range(n + 1)
                           if (b[1] - a[1]) * k % n == 0 and (b[0] - a[0]) * k % n == 0]
                assert len(on_edge) >= 3
                inner = on_edge[1:-1]
                assert all(r.layers[y, x] == 1 for y, x in inner), (a, b, z, flip)
                assert r.layers.max() == 1 and r.layers.sum() > 10


def test_a_closed_fan_around_a_vertex_on_a_pixel_centre_covers_it_once():
    for z in (1.0, 4.0):
        hub = _px(7, 5, z)
        rim = [_px(7 + dx, 5 + dy, z) for dx, dy in ((4, 0), (3, 3), (0, 4), (-3, 2), (-4, 0), (-2, -3), (0, -4), (3, -3))]
        tris = [(hub, rim[k], rim[(k + 1) % 8]) for k in range(8)]
        tris[3] = (tris[3][0], tris[3][2], tris[3][1])                    # one of them wound the other way
        r = _layers(np.array(tris))
        assert r.layers[5, 7] == 1 and r.layers.max() == 1
        assert r.layers[3:8, 5:10].all(), "and the fan has no hole"


def test_an_edge_that_crosses_the_near_plane_is_covered_exactly_once():
    """Two faces share the edge from (-0.5, -0.25, 1) to (0.5, 0.25, -0.5); both clip it at t = 1/2 from the inside end, at
    (0, 0, near).  On a 41 x 31 image with f = 16 the clipped edge runs from pixel (12, 11) to pixel (20, 15), through the
    centres (14, 12), (16, 13), (18, 14)."""
    W, H = 41, 31
    far = np.array((-0.5, -0.25, 1.0))
    behind = np.array((0.5, 0.25, -0.5))
    cam, _ = R.dyadic_camera(W, H, 16.0)
    for left, right in ((np.array((-0.5, 0.25, 1.0)), np.array((0.25, -0.375, 1.0))),                # two corners inside each
                        (np.array((-0.5, 0.25, -0.5)), np.array((0.25, -0.375, 1.0))),               # one inside, two inside
                        (np.array((-0.75, 0.5, -0.5)), np.array((0.5, -0.5, -0.5)))):                # one inside each
        for order in (0, 1, 2):
            for flip in (False, True):
                one = np.roll(np.array((far, behind, left)), order, axis=0)
                two = np.roll(np.array((behind, far, right) if not flip else (far, behind, right)), order, axis=0)
                vertices, faces = R.soup_mesh(np.array((one, two)))
                pieces = R.pieces_of(vertices, faces, cam, R.NEAR)
                assert all(p is not None for mine in pieces for p in mine) and 2 <= sum(len(m) for m in pieces) <= 4
                ends = [{(x, y) for p in mine for x, y in zip(p[0], p[1])} for mine in pieces]
                assert {(12 * 256, 11 * 256), (20 * 256, 15 * 256)} <= ends[0] & ends[1], "the same bits on both sides"
                r = R.rasterize(vertices, faces, cam, R.NEAR)
                assert r.layers.max() == 1, "no doubly covered centre"
                assert all(r.layers[y, x] == 1 for x, y in ((14, 12), (16, 13), (18, 14))), "and none uncovered on the edge"
                assert r.layers.sum() > 8 and np.all(r.depth[r.layers > 0] >= R.NEAR)


def test_the_clamp_keeps_z_between_the_corners_depths():
    rng = np.random.default_rng(2)
    cam, _ = R.dyadic_camera(33, 21, 16.0)
    for _ in range(300):
        zs = rng.choice((1.0, 1.0 + 2.0 ** -20, 2.0, 4.0, 4.0 - 2.0 ** -19), 3)
        xy = rng.integers(-64, 65, (3, 2)) / 32.0
        piece = R.pieces_of(*R.soup_mesh(np.column_stack((xy, zs))[None]), cam, R.NEAR)[0]
        if not piece or piece[0] is None:
            continue
        _, _, z = R.cover(piece[0], 33, 21)
        assert np.all(z >= np.float32(zs.min())) and np.all(z <= np.float32(zs.max()))
    flat = np.array((_px(2, 2, 2.0, 33, 21), _px(30, 3, 2.0, 33, 21), _px(10, 19, 2.0, 33, 21)))
    r = _layers(flat[None], 33, 21)
    assert (r.depth[r.layers > 0] == 2.0).all() and r.layers.sum() > 100, "a face at one depth has that depth's bits everywhere"


def test_backfaces_are_those_whose_normal_points_away():
    front = np.array((_px(2, 2, 2.0), _px(2, 9, 2.0), _px(12, 2, 2.0)))        # (b - a) x (c - a) has z < 0: towards the camera
    back = front[[0, 2, 1]]
    n = np.cross(front[1] - front[0], front[2] - front[0])
    assert n[2] < 0
    both = _layers(np.array((front, back)))
    assert both.layers.max() == 2 and set(np.unique(both.face_id)) == {-1, 0}
    culled = _layers(np.array((back, front)), cull=True)
    assert culled.layers.max() == 1 and set(np.unique(culled.face_id)) == {-1, 1}
    assert np.array_equal(culled.depth, both.depth)
