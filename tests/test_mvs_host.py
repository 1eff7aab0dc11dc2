"""CPU-side checks of the multi-view depth consistency filter (csrc/mvs.hip, ABI v34; mvs.py): the numpy
restatement against pixels computed by hand, ``select_source_views``, every refusal -- which all come before a GPU is asked
for -- the ABI, and what the analytic scene of tests/test_gpu_mvs.py must hold: a fragile share below 1 % and robust
pixels of every kind."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import mvs_restate as R


def test_restatement_gives_the_hand_computed_pixels_of_the_dyadic_case():
    ref, depth, cams, depths = R.exact_case()
    rows = R.source_rows(ref, cams, depths)
    fx, fy = R.focal(ref)
    assert (fx, fy, rows[0]["fx"], rows[0]["fy"]) == (64.0, 64.0, 32.0, 32.0)
    assert np.array_equal(rows[0]["A"][3], [0.78125, 0, 0, 1]) and np.array_equal(rows[0]["B"][3], [-0.78125, 0, 0, 1])
    for dtype in (np.float64, np.float32):
        n, fused, fragile, kinds = R.consistency(depth, fx, fy, rows, 1.0, 0.01, 1, dtype)
        # (35, 18): xr = 0.5 * 4 / 64 = 1/32, xs = 13/16, us = 32 * (13/16) / 4 + 23.5 = 30: an integer, ax = 0; vs = 19.5
        # back: xb' = 6.5 * 4 / 32 = 13/16, xb = 1/32, ub = 64 / 32 / 4 + 34.5 = 35: du = dv = 0, zb = 4
        assert n[18, 35] == 1 and fused[18, 35] == 4.0 and kinds[0, 18, 35] == R.KINDS.index("ok")
        # px = 69: us = 69 / 2 + 12.5 = 47 = W_s - 1 exactly: x0 + 1 = 48 > 47, refused in every row
        assert np.all(n[:, 69] == 0) and np.all(fused[:, 69] == 0) and np.all(kinds[0, :, 69] == R.KINDS.index("outside"))
        assert np.all(n[:, :69] == 1) and np.all(fused[:, :69] == 4.0)
    # one source column at 4.25: (34, 18) reads us = 29.5 between columns 29 and 30, ds = 4.125; xb' = 6 * 4.125 / 32,
    # xb = -1/128, ub = 34.5 - 0.5 / 4.125: du = 0.5 - 4/33 = 25/66, dv = 0; |zb - d| = 0.125 against 0.01 * 4 and against 0.05 * 4
    bumped = depths[0].copy()
    bumped[:, 30] = 4.25
    rows = R.source_rows(ref, cams, [bumped])
    for dtype in (np.float64, np.float32):
        n, fused, _, kinds = R.consistency(depth, fx, fy, rows, 1.0, 0.01, 0, dtype)
        assert n[18, 34] == 0 and kinds[0, 18, 34] == R.KINDS.index("depth") and fused[18, 34] == 4.0      # min_views 0: d
        n, fused, _, kinds = R.consistency(depth, fx, fy, rows, 1.0, 0.05, 1, dtype)
        assert n[18, 34] == 1 and fused[18, 34] == 4.0625
        n, _, _, kinds = R.consistency(depth, fx, fy, rows, 0.5, 0.05, 1, dtype)         # 25/66 < 1/2 still
        assert n[18, 34] == 1
        n, _, _, kinds = R.consistency(depth, fx, fy, rows, 0.25, 0.05, 1, dtype)
        assert n[18, 34] == 0 and kinds[0, 18, 34] == R.KINDS.index("pixel")


def test_identical_cameras_on_a_fronto_parallel_plane_agree_on_every_interior_pixel():
    cam = R.Cam(np.eye(3), np.zeros(3), 70, 37, 64.0, 64.0)
    depth = np.full((37, 70), 4.0, np.float32)
    S = 5
    rows = R.source_rows(cam, [cam] * S, [depth] * S)
    for dtype in (np.float64, np.float32):
        n, fused, fragile, _ = R.consistency(depth, 64.0, 64.0, rows, 1.0, 0.01, 2, dtype)
        assert np.all(n[:-1, :-1] == S) and np.all(fused[:-1, :-1] == 4.0)
        assert np.all(n[-1] == 0) and np.all(n[:, -1] == 0), "the last row and column have no 2 x 2 footprint"
    xyz = R.backproject(depth, 64.0, 64.0, R.cam_to_world32(cam))
    assert np.array_equal(xyz[18 * 70 + 35], [0.03125, 0.0, 4.0]) and xyz.shape == (37 * 70, 3)


def _ring(n=8, radius=3.0):
    target = np.array([0.5, -0.25, 1.0])
    return [R.look_at(target + radius * np.array([math.cos(a), 0.0, math.sin(a)]), target, 32, 24, 30.0, 30.0)
            for a in np.arange(n) * (2 * math.pi / n)]


def test_select_source_views_on_a_ring_of_eight_and_its_refusals():
    from mvs_gaussian_splatting_amd import select_source_views
    ring = _ring()
    got = select_source_views(ring, 4)                                     # neighbours look 45 degrees apart, the next 90
    assert [sorted(g) for g in got] == [sorted(((i - 1) % 8, (i + 1) % 8)) for i in range(8)]
    wide = select_source_views(ring, 3, max_angle_deg=100.0)
    for i, g in enumerate(wide):
        assert len(g) == 3 and set(g[:2]) == {(i - 1) % 8, (i + 1) % 8} and g[2] in ((i - 2) % 8, (i + 2) % 8)
    assert select_source_views(ring, 0) == [[]] * 8 and select_source_views([], 3) == []
    assert all(len(g) == 7 for g in select_source_views(ring, 64, max_angle_deg=180.0))
    # an uneven set against the restatement, and ties: equal distances keep the smaller index
    rng = np.random.default_rng(3)
    cams = [R.look_at(rng.normal(size=3) * 2 + np.array([0, 0, -6.0]), rng.normal(size=3) * 0.5, 20, 20, 20.0, 20.0)
            for _ in range(9)]
    for k, ang in ((2, 60.0), (4, 25.0), (9, 10.0)):
        assert select_source_views(cams, k, ang) == R.select_source_views(cams, k, ang)
    same = [R.Cam(np.eye(3), p, 8, 8, 8.0, 8.0) for p in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, 0, 2))]
    assert select_source_views(same, 2)[0] == [1, 2] and select_source_views(same, 4)[0] == [1, 2, 3, 4]
    assert select_source_views(same, 4)[4][:1] == [0]
    for bad in ({"n_sources": -1}, {"n_sources": 1.5}, {"n_sources": 2, "max_angle_deg": 0.0},
                {"n_sources": 2, "max_angle_deg": 180.5}, {"n_sources": 2, "max_angle_deg": float("nan")}):
        with pytest.raises(ValueError):
            select_source_views(ring, **bad)


def test_every_python_refusal_is_a_value_error_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import (TSDFVolume, _lib, backproject_depth, depth_consistency, fuse_depth_points,
                                            fuse_views)
    ref, depth, cams, depths = R.exact_case()
    d, sd = torch.from_numpy(depth), torch.from_numpy(depths[0])
    good = dict(depth=d, camera=ref, src_depths=[sd], src_cameras=cams)
    bad = ({"depth": d.double()}, {"depth": d.t().contiguous()}, {"depth": depth}, {"src_depths": [sd.double()]},
           {"src_depths": [d]}, {"src_depths": []}, {"src_depths": [sd] * 65, "src_cameras": cams * 65},
           {"pix_thresh": 0.0}, {"pix_thresh": float("inf")}, {"depth_thresh": -1.0}, {"depth_thresh": float("nan")},
           {"min_views": -1}, {"min_views": 1.5})
    for kw in bad:
        with pytest.raises(ValueError):
            depth_consistency(**{**good, **kw})
    with pytest.raises(ValueError):
        backproject_depth(d.double(), ref)
    with pytest.raises(ValueError):
        backproject_depth(sd, ref)
    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError):
        depth_consistency(**good)
    with pytest.raises(_lib.GsrError):
        depth_consistency(d[None], ref, [], [])
    with pytest.raises(_lib.GsrError):
        backproject_depth(d, ref)
    volume = TSDFVolume((0, 0, 0), 1.0, (2, 2, 2), 1.0, device="cpu")
    called = []
    renderer = lambda *a, **kw: called.append(kw) or {}                   # noqa: E731
    for consistency in ({"views": 2}, {"min_views": -1}, {"pix_thresh": 0.0}):
        with pytest.raises(ValueError):
            fuse_views([ref], None, None, None, volume, renderer=renderer, consistency=consistency)
    for kw in ({"min_views": -1}, {"depth_thresh": 0.0}, {"depth_ratio": 2.0}):
        with pytest.raises(ValueError):
            fuse_depth_points([ref], None, None, None, renderer=renderer, **kw)
    assert called == [], "refused before anything is rendered"


def test_library_exports_the_mvs_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    import mvs_gaussian_splatting_amd as pkg
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_mvs_consistency", "gsr_depth_backproject"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert "GsrMvsSource" in header and C.sizeof(_lib.GsrMvsSource) == 152 and _lib.GsrMvsSource.ref_to_src.offset == 24
    assert int(re.search(r"#define GSR_MVS_MAX_SOURCES (\d+)", header).group(1)) == _lib.MVS_MAX_SOURCES == 64
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 34
    for name in ("select_source_views", "depth_consistency", "backproject_depth", "fuse_depth_points"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_raw_abi_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    ptr = C.addressof(buf)
    assert ptr % 8 == 0
    good = dict(depth=ptr, H=4, W=4, fx=1.0, fy=1.0, sources=ptr, S=1, pix=1.0, dep=0.01, mv=2, count=ptr, fused=ptr)
    call = lambda **kw: lib.gsr_mvs_consistency(*{**good, **kw}.values(), None)      # noqa: E731
    inf, nan = math.inf, math.nan
    bad = [{"depth": None}, {"count": None}, {"fused": None}, {"H": 0}, {"W": 0}, {"H": -3}, {"H": 2 ** 14 + 1, "W": 2 ** 14},
           {"S": -1}, {"S": 65}, {"sources": None}, {"mv": -1}]
    bad += [{k: v} for k in ("fx", "fy", "pix", "dep") for v in (0.0, -1.0, inf, nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.gsr_last_error()
    for kw in ({"depth": ptr + 2}, {"fused": ptr + 1}, {"sources": ptr + 4}):
        assert call(**kw) == -3, kw
    c2w = (C.c_float * 16)(*np.eye(4, dtype=np.float32).reshape(-1))
    back = lambda depth=ptr, H=4, W=4, fx=1.0, fy=1.0, m=C.addressof(c2w), xyz=ptr: lib.gsr_depth_backproject(     # noqa: E731
        depth, H, W, fx, fy, m, xyz, None)
    for kw in ({"H": -1}, {"W": -1}, {"H": 2 ** 14 + 1, "W": 2 ** 14}, {"m": None}, {"depth": None}, {"xyz": None}):
        assert back(**kw) == -1, kw
    for k in ("fx", "fy"):
        for v in (0.0, -2.0, inf, nan):
            assert back(**{k: v}) == -1, (k, v)
            assert back(**{k: v, "H": 0}) == -1, "n = 0 still checks the scalars"
    for kw in ({"depth": ptr + 2}, {"xyz": ptr + 1}):
        assert back(**kw) == -3, kw
    for kw in ({"H": 0}, {"W": 0}, {"H": 0, "W": 0, "depth": None, "xyz": None}):
        assert back(**kw) == 0, "n = 0 is a successful no-op"


def test_fragile_share_of_the_scene_is_below_one_percent_and_every_kind_of_pixel_is_robustly_there():
    ref, depth, cams, depths = R.scene()
    assert depth.shape == (37, 70) and depths[0].shape == (40, 48) and len(cams) == 4
    assert R.focal(cams[0]) != R.focal(ref) and R.focal(cams[0])[0] != R.focal(cams[0])[1]
    assert (depths[1] == 0).sum() >= 100 and (depth == 0).sum() == 18
    rows = R.source_rows(ref, cams, depths)
    fx, fy = R.focal(ref)
    n, fused, fragile, kinds = R.consistency(depth, fx, fy, rows, R.PIX_THRESH, R.DEPTH_THRESH, 2)
    n32, fused32, _, _ = R.consistency(depth, fx, fy, rows, R.PIX_THRESH, R.DEPTH_THRESH, 2, np.float32)
    has = depth > 0
    share = float((fragile & has).sum()) / float(has.sum())
    ok = has & ~fragile
    by_count = [int(((n == k) & ok).sum()) for k in range(4)]
    by_kind = {k: int(((kinds == i) & ok[None]).sum()) for i, k in enumerate(R.KINDS)}
    print(f"{int(has.sum())} pixels with depth, fragile share {share:.2e}; robust pixels by count {by_count}; "
          f"(pixel, source) pairs by kind {by_kind}")
    assert share < 0.01
    assert all(c >= 100 for c in by_count) and n.max() == 3
    assert all(by_kind[k] >= 50 for k in R.KINDS), by_kind
    assert np.all(kinds[3][has] == R.KINDS.index("behind")), "the camera facing away sees no reference point"
    # the 1.02 half of source 2 fails the depth test alone; the 1.014 patch of source 0 the pixel test alone
    assert int(((kinds[2] == R.KINDS.index("depth")) & ok).sum()) >= 500
    assert int(((kinds[0] == R.KINDS.index("pixel")) & ok).sum()) >= 50
    # float32 takes every decision as float64 does on the robust pixels, and its values are close
    assert np.array_equal(n[ok], n32[ok])
    assert float((np.abs(fused32 - fused)[ok] / depth[ok]).max()) < 1e-5
    assert np.all(fused[~has] == 0) and np.all(n[~has] == 0)
    assert np.array_equal(fused > 0, has & (n >= 2))


def test_example_passes_consistency_and_writes_the_fused_points_only_when_asked(monkeypatch, tmp_path):
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("example_extract_mesh_mvs", os.path.join(ROOT, "examples", "extract_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    calls = []
    mesh = tuple(types.SimpleNamespace(shape=(n, 3), name=m) for n, m in zip((8, 12, 8), ("vertices", "faces", "colors")))

    cloud = tuple(types.SimpleNamespace(shape=(5, 3), name=m) for m in ("xyz", "rgb"))

    class Volume:
        dims, voxel_size, sdf_trunc = (4, 4, 4), 0.5, 2.0

        def extract_mesh(self, *a, **kw):
            return mesh

    class Scene:
        loaded_iter = 7

        def __init__(self, *a, **kw):
            pass

        def getTrainCameras(self):
            return ["cam"]

    monkeypatch.setattr(mod, "GaussianModel", lambda d: types.SimpleNamespace(get_xyz="xyz"))
    monkeypatch.setattr(mod, "Scene", Scene)
    monkeypatch.setattr(mod, "volume_for_points", lambda xyz, **kw: Volume())
    monkeypatch.setattr(mod, "fuse_views", lambda *a, **kw: calls.append(("fuse_views", kw)))
    monkeypatch.setattr(mod, "fuse_depth_points", lambda *a, **kw: calls.append(("fuse_depth_points", kw)) or cloud)
    monkeypatch.setattr(mod, "write_ply_mesh", lambda path, *a: calls.append(("write_ply_mesh", path)))
    monkeypatch.setattr(mod, "write_points", lambda path, xyz, rgb: calls.append(("write_points", path, xyz.name, rgb.name)))
    monkeypatch.setattr(mod, "torch", types.SimpleNamespace(no_grad=torch.no_grad, float32=torch.float32,
                                                            tensor=lambda *a, **kw: "background"))
    monkeypatch.setattr(mod, "ModelParams", lambda **kw: types.SimpleNamespace(sh_degree=3, white_background=False, **kw))
    base = ["-m", str(tmp_path), "-s", "dataset"]
    out = os.path.join(str(tmp_path), "mesh", "iteration_7")
    mod.main(base)
    assert calls == [("fuse_views", {"alpha_min": 0.5, "max_depth": None}), ("write_ply_mesh", os.path.join(out, "tsdf_mesh.ply"))]
    del calls[:]
    mod.main(base + ["--consistent", "3"])
    assert calls[0] == ("fuse_views", {"alpha_min": 0.5, "max_depth": None, "consistency": {"n_sources": 4, "min_views": 3}})
    assert len(calls) == 2
    del calls[:]
    mod.main(base + ["--consistent", "2", "--n_sources", "6", "--points", "--depth_ratio", "1"])
    assert calls[0][1]["consistency"] == {"n_sources": 6, "min_views": 2} and calls[0][1]["depth_ratio"] == 1.0
    assert calls[2] == ("fuse_depth_points", {"n_sources": 6, "min_views": 2, "alpha_min": 0.5, "depth_ratio": 1.0})
    assert calls[3] == ("write_points", os.path.join(out, "fused_points.ply"), "xyz", "rgb")
    del calls[:]
    mod.main(base + ["--points"])                                          # the cloud's own defaults; the mesh unfiltered
    assert calls[0] == ("fuse_views", {"alpha_min": 0.5, "max_depth": None})
    assert calls[2] == ("fuse_depth_points", {"n_sources": 4, "min_views": 2, "alpha_min": 0.5, "depth_ratio": 0.0})
    for flags in (["--consistent", "-1"], ["--n_sources", "0", "--consistent", "1"], ["--n_sources", "65"]):
        with pytest.raises(SystemExit):
            mod.main(base + flags)
