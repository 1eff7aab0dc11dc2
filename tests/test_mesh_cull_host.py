"""CPU-side checks of the view culling (csrc/mesh_cull.hip; ``mesh.vertex_view_counts``, ``mesh.cull_mesh_by_views``,
``mesh.dilate_mask``): the ABI and every refusal of the entry points and of the Python functions -- which
all come before a GPU is asked for -- the restatement the GPU tests compare against (tests/mesh_cull_restate.py) against
scipy's dilation and against the kernel's own body built by the host compiler (csrc/mesh_cull_math.h through
tests/mesh_cull_host_check.cpp), the condition on the scene that makes those comparisons mean something, and what the
rule does to the scene."""
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
import mesh_cull_restate as R

ENTRY_POINTS = ("gsr_cull_view_counts", "gsr_cull_face_keep", "gsr_mask_dilate")


@pytest.fixture(scope="module")
def scene():
    return R.scene(9)


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_abi_is_at_least_41():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib, mesh, tsdf
    for name in ("dilate_mask", "vertex_view_counts", "cull_mesh_by_views"):
        assert getattr(pkg, name) is getattr(mesh, name) and name in pkg.__all__ and name in mesh.__all__
    assert pkg.view_counts_for_views is tsdf.view_counts_for_views
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\bint " + name + r"\(", header), name
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 41
    assert "GsrCullView" in header and C.sizeof(_lib.GsrCullView) == 96 and _lib.GsrCullView.world_to_view.offset == 32
    assert C.alignment(_lib.GsrCullView) == 8 and _lib.CULL_MAX_VIEWS == 65535 and _lib.DILATE_MAX_RADIUS == 1024
    makefile = open(os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "Makefile")).read()
    assert re.search(r"CONTRACT_OFF_OBJS \+= mesh_cull\.o", makefile) and "mesh_cull_math.h" in makefile


def test_every_entry_point_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    big = 2 ** 31
    BAD, ALIGN = -1, -3
    nan, inf = float("nan"), float("inf")

    counts = lib.gsr_cull_view_counts
    good = dict(vertices=p, V=4, views=p, S=2, near=0.2, tol=0.01, accumulate=0, in_view=p, visible=p)
    call = lambda **kw: counts(*{**good, **kw}.values(), None)      # noqa: E731
    for name in ("vertices", "views", "in_view", "visible"):
        assert call(**{name: None}) == BAD, name
    assert b"NULL" in lib.gsr_last_error()
    for V in (-1, big):
        assert call(V=V) == BAD
    for S in (-1, 65536):
        assert call(S=S) == BAD
    for near in (0.0, -1.0, nan, inf):
        assert call(near=near) == BAD, near
    for tol in (-1e-3, nan, inf, -inf):
        assert call(tol=tol) == BAD, tol
    for name in ("vertices", "in_view", "visible"):
        assert call(**{name: p + 2}) == ALIGN, name
    assert call(views=p + 4) == ALIGN
    # the successes that launch nothing: no vertices, whatever the pointers
    assert call(V=0) == 0 and call(V=0, vertices=None, in_view=None, visible=None, S=0, views=None) == 0
    assert call(V=0, tol=0.0) == 0 and call(V=0, S=65535) == 0

    fkeep = lib.gsr_cull_face_keep
    good = [p, p, 4, 8, p, p]
    for n in (0, 1, 4, 5):
        assert fkeep(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    for F, V in ((-1, 8), (big, 8), (4, -1), (4, big)):
        assert fkeep(p, p, F, V, p, p, None) == BAD, (F, V)
    assert fkeep(p + 2, p, 4, 8, p, p, None) == ALIGN and fkeep(p, p, 4, 8, p, p + 2, None) == ALIGN
    assert fkeep(p, p + 1, 0, 8, p + 1, p, None) == 0 and fkeep(None, None, 0, 0, None, p, None) == 0    # F = 0

    dilate = lib.gsr_mask_dilate
    q = p + 256
    good = [p, 4, 8, 1, q, p]
    for n in (0, 4, 5):
        assert dilate(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    for H, W in ((0, 8), (4, 0), (-1, 8), (2 ** 14 + 1, 2 ** 14)):
        assert dilate(p, H, W, 1, q, p, None) == BAD, (H, W)
    for r in (-1, 1025):
        assert dilate(p, 4, 8, r, q, p, None) == BAD, r
    assert dilate(p, 4, 8, 1, p, q, None) == BAD and dilate(p, 4, 8, 1, q, q, None) == BAD        # tmp of its own
    assert b"tmp" in lib.gsr_last_error()


def _cam(W=8, H=6, M=None):
    return R.camera(np.eye(4) if M is None else M, W, H, 10.0, 10.0)


def test_python_refusals_come_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, cull_mesh_by_views, dilate_mask, vertex_view_counts, view_counts_for_views
    vertices = torch.zeros(4, 3)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    cams = [_cam(), _cam(5, 7)]
    mask, depth = torch.ones(6, 8, dtype=torch.uint8), torch.ones(6, 8)

    for bad in (vertices.double(), torch.zeros(4, 2), torch.zeros(12), vertices.numpy(), None):
        with pytest.raises(ValueError, match="vertices"):
            vertex_view_counts(bad, cams)
        with pytest.raises(ValueError, match="vertices"):
            cull_mesh_by_views(bad, faces, cameras=cams)
    with pytest.raises(ValueError, match="cameras"):
        vertex_view_counts(vertices, 5)
    for name, maps in (("masks", [mask]), ("masks", [mask, None, None]), ("depths", [depth]), ("masks", 3)):
        with pytest.raises(ValueError, match=name):
            vertex_view_counts(vertices, cams, **{name: maps})
    for bad in (mask.float(), mask[:5], mask.T, mask.numpy(), torch.ones(2, 6, 8, dtype=torch.uint8), mask.to("meta")):
        with pytest.raises(ValueError, match=r"masks\[0\]"):
            vertex_view_counts(vertices, cams, masks=[bad, None])
    with pytest.raises(ValueError, match=r"masks\[1\]"):
        vertex_view_counts(vertices, cams, masks=[mask, mask])            # the second camera is 5 x 7
    for bad in (depth.double(), depth[:, :7], mask, depth.numpy(), depth.to("meta")):
        with pytest.raises(ValueError, match=r"depths\[0\]"):
            vertex_view_counts(vertices, cams, depths=[bad, None])
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="near"):
            vertex_view_counts(vertices, cams, near=bad)
    for bad in (-1e-3, float("nan"), float("inf"), None, "1", False):
        with pytest.raises(ValueError, match="depth_tol"):
            vertex_view_counts(vertices, cams, depth_tol=bad)
    ok = torch.zeros(4, dtype=torch.int32)
    for bad in (ok, (ok,), (ok, ok), (ok, ok.clone().long()), (ok, torch.zeros(5, dtype=torch.int32)),
                (ok, torch.zeros(8, dtype=torch.int32)[::2]), (ok, ok.clone().to("meta")), (ok, None)):
        with pytest.raises(ValueError, match="counts"):
            vertex_view_counts(vertices, cams, counts=bad)
    with pytest.raises(ValueError, match="4 x 4"):
        vertex_view_counts(vertices, [types.SimpleNamespace(world_view_transform=torch.eye(3), FoVx=1.0, FoVy=1.0,
                                                            image_width=8, image_height=6)])
    with pytest.raises(ValueError, match="empty image"):
        vertex_view_counts(vertices, [types.SimpleNamespace(world_view_transform=torch.eye(4), FoVx=1.0, FoVy=1.0,
                                                            image_width=0, image_height=6)])
    with pytest.raises(TypeError):
        vertex_view_counts(vertices, cams, [mask, None])                  # the maps are given by keyword

    for bad in (faces.long(), faces.reshape(-1), faces[:, :2], None, faces.to("meta")):
        with pytest.raises(ValueError):
            cull_mesh_by_views(vertices, bad, cameras=cams)
    for bad in (torch.zeros(3, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, device="meta")):
        with pytest.raises(ValueError, match="colors"):
            cull_mesh_by_views(vertices, faces, bad, cameras=cams)
    for bad in (-1, 1.0, True, None, "some", 2 ** 31):
        with pytest.raises(ValueError, match="min_views"):
            cull_mesh_by_views(vertices, faces, cameras=cams, min_views=bad)
    for bad in (-1, 1025, 1.0, True, None):
        with pytest.raises(ValueError, match="dilate"):
            cull_mesh_by_views(vertices, faces, cameras=cams, dilate=bad)
    with pytest.raises(ValueError, match="return_counts"):
        cull_mesh_by_views(vertices, faces, cameras=cams, return_counts=1)
    with pytest.raises(ValueError, match=r"masks\[1\]"):
        cull_mesh_by_views(vertices, faces, cameras=cams, masks=[mask, mask], dilate=2)    # before any dilation
    with pytest.raises(TypeError):
        cull_mesh_by_views(vertices, faces)                               # the cameras have no default

    for bad in (mask.float(), mask.reshape(-1), torch.ones(0, 8, dtype=torch.uint8), mask.numpy(), None):
        with pytest.raises(ValueError, match="mask"):
            dilate_mask(bad, 1)
    for bad in (-1, 1025, 1.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            dilate_mask(mask, bad)

    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="chunk"):
            view_counts_for_views(cams, None, None, None, vertices, chunk=bad)
    with pytest.raises(ValueError, match="occlusion"):
        view_counts_for_views(cams, None, None, None, vertices, occlusion=1)
    with pytest.raises(ValueError, match="masks"):
        view_counts_for_views(cams, None, None, None, vertices, masks=[mask], occlusion=False)

    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        vertex_view_counts(vertices, cams, masks=[mask, None], depths=[depth, None], counts=(ok, ok.clone()))
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        vertex_view_counts(vertices[:0], [])
    for kw in ({}, {"min_views": "all", "masks": [mask.bool(), None], "dilate": 3}, {"min_views": 0, "return_counts": True}):
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            cull_mesh_by_views(vertices, faces, torch.zeros(4, 3), cameras=cams, **kw)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        cull_mesh_by_views(vertices, faces[:0], cameras=cams)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        dilate_mask(mask, 0)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        view_counts_for_views(cams, None, None, None, vertices, occlusion=False, chunk=1)


# ---- the restatement ---------------------------------------------------------------------------------------------------
def test_restated_dilation_is_scipys():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    mask = (rng.random((37, 70)) < 0.04).astype(np.uint8) * rng.integers(1, 256, (37, 70)).astype(np.uint8)
    assert 0 < np.count_nonzero(mask) < mask.size // 10
    for r in (0, 1, 5, 71):
        want = ndimage.binary_dilation(mask != 0, structure=np.ones((2 * r + 1, 2 * r + 1)))
        got = R.dilate(mask, r)
        assert got.dtype == np.uint8 and set(np.unique(got)) <= {0, 1} and np.array_equal(got != 0, want), r
    assert np.array_equal(R.dilate(mask, 0), (mask != 0).astype(np.uint8)) and R.dilate(mask, 71).all()
    assert not R.dilate(np.zeros((1, 1), dtype=np.uint8), 64).any() and R.dilate(np.ones((1, 1), dtype=np.uint8), 64).all()


def test_scene_has_the_cases_it_is_named_for(scene):
    s = scene
    V = len(s.vertices)
    assert V == 829 and V > 3 * 256 and V % 256 not in (0, 255) and s.vertices.dtype == np.float32
    assert np.isnan(s.vertices).any(axis=1).sum() == 1
    unreferenced = np.setdiff1d(np.arange(V), s.faces.reshape(-1))
    assert len(unreferenced) == 7 and np.all(s.part[unreferenced] == "extra")
    sizes = {(c.image_width, c.image_height) for c in s.cameras}
    assert sizes == {(70, 37), (48, 40)} and len({R.focal(c)[2:] for c in s.cameras}) == 2
    kinds = [(m is not None, d is not None) for m, d in zip(s.masks, s.depths)]
    assert kinds[:5] == [(False, False), (False, False), (True, False), (False, True), (True, True)]
    for d in s.depths:
        if d is not None:
            H, W = d.shape
            assert (d[H // 2 - 3:H // 2 + 2, W // 2 + 4:W // 2 + 11] == 0).all() and d[H // 2, W // 2] > 2.9, "a hole on the sphere"
    # view 1 faces away: it sees none of the mesh, and some vertex behind the others' near plane
    a, _, _ = R.view_pairs(s.vertices, s.cameras[1], dtype=np.float64)
    assert not a[s.part != "extra"].any() and a[s.part == "extra"].any()
    n_in, _, _ = R.counts(s.vertices, [c for k, c in enumerate(s.cameras) if k != 1], dtype=np.float64)
    assert (n_in[s.part == "extra"] == 0).sum() >= 4, "behind every other camera, outside every image, or NaN"
    assert np.all(n_in[s.part != "extra"] == len(s.cameras) - 1), "the whole mesh is inside every other image"


def test_fragile_share_of_the_scenes_is_small():
    """A condition on the inputs: were it not to hold, the exact comparison of the GPU tests would cover too little."""
    for S in (1, 5, 9, 70):
        s = R.scene(S)
        _, _, fragile = R.counts(s.vertices, s.cameras, s.masks, s.depths, s.near, s.depth_tol, dtype=np.float64)
        assert fragile.sum() <= 0.01 * len(s.vertices) * S, (S, int(fragile.sum()))
    d = R.dyadic()
    got = [R.counts(d.vertices, d.cameras, d.masks, d.depths, d.near, d.depth_tol, dtype=t) for t in (np.float32, np.float64)]
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), "exact in both precisions"
    assert got[1][2].sum() > 0.1 * len(d.vertices), "and full of pairs that sit on a boundary"
    assert 0 < got[0][1].sum() < got[0][0].sum() < 3 * len(d.vertices)


def test_float32_and_float64_restatements_agree_off_the_fragile_pairs(scene):
    s = scene
    a32, b32, _ = R.counts(s.vertices, s.cameras, s.masks, s.depths, s.near, s.depth_tol, dtype=np.float32)
    a64, b64, fragile = R.counts(s.vertices, s.cameras, s.masks, s.depths, s.near, s.depth_tol, dtype=np.float64)
    assert np.all(np.abs(a32 - a64) <= fragile) and np.all(np.abs(b32 - b64) <= fragile)
    assert a64.max() == len(s.cameras) - 1 and 0 < b64.sum() < a64.sum()


# ---- the kernel's body on the host -------------------------------------------------------------------------------------
def _scene_bytes(vertices, cameras, masks, depths, near, depth_tol):
    out = [struct.pack("<iiff", len(vertices), len(cameras), near, depth_tol)]
    for cam, m, d in zip(cameras, masks, depths):
        H, W, fx, fy = R.focal(cam)
        out.append(struct.pack("<iiiiff", W, H, m is not None, d is not None, fx, fy))
        out.append(cam.world_view_transform.numpy().astype("<f4").tobytes())
        if m is not None:
            out.append(np.ascontiguousarray(m, dtype=np.uint8).tobytes())
        if d is not None:
            out.append(np.ascontiguousarray(d, dtype="<f4").tobytes())
    out.append(np.ascontiguousarray(vertices, dtype="<f4").tobytes())
    return b"".join(out)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """``csrc/mesh_cull_math.h`` -- the body of the counting kernel -- built by the host compiler from
    ``tests/mesh_cull_host_check.cpp`` into a program of its own, with the kernel's ``-ffp-contract=off``."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    folder = tmp_path_factory.mktemp("mesh_cull_host")
    exe = str(folder / "mesh_cull_host_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mesh_cull_host_check.cpp"), "-o", exe], check=True)

    def run(s):
        path = str(folder / "scene.bin")
        with open(path, "wb") as f:
            f.write(_scene_bytes(s.vertices, s.cameras, s.masks, s.depths, s.near, s.depth_tol))
        out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.split()
        got = np.array(out, dtype=np.int32).reshape(-1, 2)
        return got[:, 0], got[:, 1]
    return run


def test_host_build_of_the_kernels_body_gives_the_float32_restatements_counts(host_check, scene):
    for s in (scene, R.scene(70), R.dyadic()):
        n_in, n_vis = host_check(s)
        want_in, want_vis, _ = R.counts(s.vertices, s.cameras, s.masks, s.depths, s.near, s.depth_tol, dtype=np.float32)
        assert np.array_equal(n_in, want_in) and np.array_equal(n_vis, want_vis)
        assert n_vis.sum() > 0 and (n_vis <= n_in).all() and n_in.max() <= len(s.cameras)


# ---- what the rule does to the scene -----------------------------------------------------------------------------------
def _front(s, cameras):
    """The sphere's vertices that face one of the cameras within 37 degrees (cos > 0.8)."""
    v = s.vertices.astype(np.float64)
    front = np.zeros(len(v), dtype=bool)
    for cam in cameras:
        M = cam.world_view_transform.numpy().astype(np.float64)
        centre = -M[3, :3] @ M[:3, :3].T
        to_cam = centre - v
        to_cam /= np.linalg.norm(to_cam, axis=1, keepdims=True)
        with np.errstate(invalid="ignore"):
            front |= (v * to_cam).sum(1) > 0.8          # the sphere's normal at a vertex is the vertex
    return front & (s.part == R.SPHERE)


def test_masks_remove_the_floater_depths_remove_the_inner_shell_and_the_front_survives_both(scene):
    s = scene
    ring = [c for k, c in enumerate(s.cameras) if k != 1]
    silhouettes = [R.dilate(R.sphere_maps(c)[0], 2) for c in ring]
    surfaces = [R.sphere_maps(c)[1] for c in ring]
    front = _front(s, ring)
    assert front.sum() > 150

    n_in, n_vis, _ = R.counts(s.vertices, ring, masks=silhouettes, dtype=np.float32)
    v, f, c, kept_v, kept_f = R.cull(s.vertices, s.faces, s.colors, n_in, n_vis, "all")
    assert not (s.part[kept_v] == R.FLOATER).any(), "DTU's rule removes the floater"
    assert front[kept_v].sum() == front.sum() and (s.part[kept_v] == R.SPHERE).sum() == (s.part == R.SPHERE).sum()
    assert (s.part[kept_v] == R.INNER).sum() == (s.part == R.INNER).sum(), "masks alone keep the inner shell"
    assert np.array_equal(v.view(np.int32), s.vertices[kept_v].view(np.int32)) and np.array_equal(c, s.colors[kept_v])
    assert np.array_equal(kept_v[f], s.faces[kept_f]), "faces are re-indexed, in order"
    assert not np.isin(np.setdiff1d(np.arange(len(s.vertices)), s.faces.reshape(-1)), kept_v).any()

    n_in, n_vis, _ = R.counts(s.vertices, ring, depths=surfaces, depth_tol=s.depth_tol, dtype=np.float32)
    v, f, c, kept_v, kept_f = R.cull(s.vertices, s.faces, None, n_in, n_vis, 1)
    assert c is None and not (s.part[kept_v] == R.INNER).any(), "the occlusion test removes the inner shell"
    assert front[kept_v].sum() == front.sum(), "and keeps what faces a camera"
    assert not (s.part[kept_v] == R.FLOATER).any(), "where the depth map holds no surface nothing is visible"
    assert (n_vis[front] >= 1).all() and (n_vis[s.part == R.INNER] == 0).all()

    with pytest.raises(ValueError, match="face index"):
        R.face_keep(np.array([[0, 1, 829]]), np.ones(829))
