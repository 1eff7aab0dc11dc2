"""CPU-side checks of the multi-view geometric consistency loss (csrc/mvs_loss.hip, ABI v35; mvs.multi_view_geo_loss;
DESIGN.md §7.22): the torch restatement against central finite differences, against a dyadic case computed by hand and
against identical cameras; every refusal of the wrapper and of the entry point -- which all come before a GPU is asked
for -- the ABI, the trainer's refusals and off-switch, and what the scene of tests/test_gpu_mvs_loss.py must hold."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import mvs_restate as R
import mvs_loss_restate as L


def _scene_row():
    ref, depth, src, sdepth = L.scene()
    return depth, R.source_rows(ref, [src], [sdepth])[0], R.focal(ref)


def test_restated_float64_gradients_agree_with_central_finite_differences():
    depth, row, (fx, fy) = _scene_row()
    for depth_thresh in (None, L.DEPTH_THRESH):
        base = L.loss(depth, fx, fy, row, L.PIX_MAX, depth_thresh)
        robust = base["valid"] & ~base["fragile"]
        w0 = np.exp(-base["phi"][base["valid"]])                           # the weight is a constant of the gradient
        fixed = lambda o: float((w0 * o["phi"][base["valid"]]).sum())      # noqa: E731
        ys, xs = np.nonzero(robust)
        pick = np.linspace(0, len(ys) - 1, 6).astype(int)
        worst = 0.0
        for y, x in zip(ys[pick], xs[pick]):
            h = 1e-6 * float(depth[y, x])
            vals = []
            for sign in (1.0, -1.0):
                m = depth.astype(np.float64)
                m[y, x] += sign * h
                vals.append(fixed(L.loss(m, fx, fy, row, L.PIX_MAX, depth_thresh, round_inputs=False)))
            fd, g = (vals[0] - vals[1]) / (2 * h), float(base["grad_ref"][y, x])
            worst = max(worst, abs(fd - g) / abs(g))
            assert abs(fd - g) <= 1e-6 * abs(g), (y, x, fd, g)
        clean = (base["feeds"] >= 1) & ~base["tainted"] & (np.abs(base["grad_src"]) > 1e-3 * np.abs(base["grad_src"]).max())
        ys, xs = np.nonzero(clean)
        pick = np.linspace(0, len(ys) - 1, 6).astype(int)
        for y, x in zip(ys[pick], xs[pick]):
            h = 1e-6 * float(row["depth"][y, x])
            vals = []
            for sign in (1.0, -1.0):
                m = row["depth"].astype(np.float64)
                m[y, x] += sign * h
                vals.append(fixed(L.loss(depth, fx, fy, {**row, "depth": m}, L.PIX_MAX, depth_thresh, round_inputs=False)))
            fd, g = (vals[0] - vals[1]) / (2 * h), float(base["grad_src"][y, x])
            worst = max(worst, abs(fd - g) / abs(g))
            assert abs(fd - g) <= 1e-6 * abs(g), (y, x, fd, g)
        print(f"depth_thresh={depth_thresh}: worst relative difference from central differences {worst:.2e}")


def test_restatement_gives_the_hand_computed_dyadic_case():
    ref, depth, src, sdepth = L.exact_case()
    row = R.source_rows(ref, [src], [sdepth])[0]
    fx, fy = R.focal(ref)
    assert (fx, fy, row["fx"], row["fy"]) == (64.0, 64.0, 32.0, 32.0)
    assert np.array_equal(row["A"][3], [0.0625, 0, 0, 1]) and np.array_equal(row["B"][3], [-0.0625, 0, 0, 1])
    w = math.exp(-0.5)
    # the forward is exact; the backward's quotients and exp are not: the gradients get a few float32 roundings
    for dtype, tol, gtol in ((torch.float64, 1e-14, 1e-14), (torch.float32, 2e-7, 1e-5)):
        o = L.loss(depth, fx, fy, row, 1.0, None, dtype)
        assert o["n"] == 37 * 70 and o["valid"].all() and not o["fragile"][0::2].any()      # odd rows: vs is an integer
        assert np.all(o["phi"] == 0.5), "du = 64 t (1 / d - 1 / D) = 1/2, dv = 0: exact"
        assert abs(o["value"] - 0.5 * w) <= tol * 0.5 * w
        assert np.allclose(o["grad_ref"], -0.25 * w, rtol=gtol, atol=0)
        # texel (20, 15) is fed by px 25..28 and py 7..10: x-weights 1/4 + 3/4 + 3/4 + 1/4, y-weights 1/2 + 1 + 1/2 + 0
        assert abs(o["grad_src"][15, 20] - 0.25 * w) <= gtol * 0.25 * w and o["feeds"][15, 20] == 16
        inner = o["grad_src"][12:28, 8:40]
        assert np.allclose(inner, 0.25 * w, rtol=gtol, atol=0)
        assert abs(o["grad_src"].sum() - 37 * 70 * w / 16) <= 1e-5 * 37 * 70 * w / 16, "the bilinear weights sum to one"
        assert not o["grad_src"][:, :6].any() and not o["grad_src"][:10].any(), "no reference pixel lands there"
    # pix_max below phi: nothing is valid, the value and the gradients are zero; the depth test decides the same way
    for kw in ({"pix_max": 0.5}, {"pix_max": 1.0, "depth_thresh": 0.5}):
        o = L.loss(depth, fx, fy, row, **kw)
        assert o["n"] == 0 and o["value"] == 0.0 and not o["grad_ref"].any() and not o["grad_src"].any()
        assert np.all(o["kind"] == L.KINDS.index("pixel" if "depth_thresh" not in kw else "depth"))
    o = L.loss(depth, fx, fy, row, 1.0, 1.5)                               # |zb - d| = 4 < 1.5 * 4
    assert o["n"] == 37 * 70


def test_identical_cameras_on_a_fronto_parallel_plane_give_zero_loss_and_zero_gradients():
    cam = R.Cam(np.eye(3), np.zeros(3), 70, 37, 64.0, 64.0)
    depth = np.full((37, 70), 4.0, np.float32)
    row = R.source_rows(cam, [cam], [depth])[0]
    for dtype in (torch.float64, torch.float32):
        o = L.loss(depth, 64.0, 64.0, row, 1.0, 0.01, dtype)
        assert o["n"] == 36 * 69 and o["value"] == 0.0 and o["raw"] == 0.0, "the last row and column have no footprint"
        assert not o["grad_ref"].any() and not o["grad_src"].any() and not np.isnan(o["grad_ref"]).any()
        assert np.all(o["phi"][:-1, :-1] == 0.0)


def test_every_python_refusal_comes_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, multi_view_geo_loss
    ref, depth, src, sdepth = L.exact_case()
    d, sd = torch.from_numpy(depth), torch.from_numpy(sdepth)
    good = dict(depth=d, camera=ref, src_depth=sd, src_camera=src)
    for kw in ({"depth": d.t().contiguous()}, {"src_depth": d}, {"src_depth": sd[None, None]}, {"pix_max": 0.0},
               {"pix_max": -1.0}, {"pix_max": math.inf}, {"pix_max": math.nan}, {"depth_thresh": 0.0},
               {"depth_thresh": -0.01}, {"depth_thresh": math.nan}, {"depth_thresh": math.inf},
               {"src_depth": sd.to("meta")}):
        with pytest.raises(ValueError):
            multi_view_geo_loss(**{**good, **kw})
    tall = R.Cam(np.eye(3), np.zeros(3), 1, 2 ** 26, 1.0, 2.0 ** 26)      # 2^26 pixels, but 2^24 tiles of 256 lanes
    with pytest.raises(ValueError, match="work-items"):
        multi_view_geo_loss(torch.empty((2 ** 26, 1)), tall, sd, src)
    for kw in ({"depth": depth}, {"depth": d.double()}, {"src_depth": sd.half()}, {"src_depth": None}):
        with pytest.raises(TypeError):
            multi_view_geo_loss(**{**good, **kw})
    bad_cam = R.Cam(np.eye(3), np.zeros(3), 48, 40, 32.0, 32.0)
    bad_cam.world_view_transform = torch.zeros(3, 4)
    with pytest.raises(ValueError):
        multi_view_geo_loss(d, ref, sd, bad_cam)
    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError):
        multi_view_geo_loss(**good)
    with pytest.raises(_lib.GsrError):
        multi_view_geo_loss(d[None].requires_grad_(True), ref, sd, src, depth_thresh=0.01, return_record=True)


def test_library_exports_the_entry_points_and_the_three_abi_versions_say_35():
    from mvs_gaussian_splatting_amd import _lib
    import mvs_gaussian_splatting_amd as pkg
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_mvs_geo_loss_workspace_bytes", "gsr_mvs_geo_loss_fwd_bwd"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 35
    assert "multi_view_geo_loss" in pkg.__all__ and callable(pkg.multi_view_geo_loss)
    assert "multi_view_geo_loss" in pkg.mvs.__all__
    # one (double, uint32) pair per 64 x 4 tile; 0 for a shape the call refuses
    ws = lib.gsr_mvs_geo_loss_workspace_bytes
    assert ws(37, 70) == 2 * 10 * 12 and ws(1, 1) == 12 and ws(4, 64) == 12 and ws(5, 65) == 4 * 12
    assert ws(0, 4) == 0 and ws(4, -1) == 0 and ws(2 ** 14 + 1, 2 ** 14) == 0 and ws(2 ** 28, 1) == 0


def test_raw_abi_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    ptr = C.addressof(buf)
    assert ptr % 8 == 0
    good = dict(depth=ptr, H=4, W=4, fx=1.0, fy=1.0, source=ptr, pix=1.0, dep=0.0, record=ptr, gref=ptr, gsrc=ptr, Hs=4, Ws=4,
                ws=ptr)
    call = lambda **kw: lib.gsr_mvs_geo_loss_fwd_bwd(*{**good, **kw}.values(), None)      # noqa: E731
    inf, nan = math.inf, math.nan
    bad = [{"depth": None}, {"source": None}, {"record": None}, {"ws": None}, {"H": 0}, {"W": 0}, {"H": -3},
           {"H": 2 ** 14 + 1, "W": 2 ** 14}, {"H": 2 ** 28, "W": 1}, {"dep": nan}, {"Hs": 0}, {"Ws": -1},
           {"Hs": 2 ** 14 + 1, "Ws": 2 ** 14}]
    bad += [{k: v} for k in ("fx", "fy", "pix") for v in (0.0, -1.0, inf, nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.gsr_last_error()
    for kw in ({"depth": ptr + 2}, {"record": ptr + 1}, {"gref": ptr + 2}, {"gsrc": ptr + 2}, {"source": ptr + 4},
               {"ws": ptr + 4}):
        assert call(**kw) == -3, kw


class _Cam:
    FoVx = FoVy = 1.0
    image_width, image_height = 8, 8
    original_image = torch.zeros(3, 8, 8)


def test_optimization_params_gain_the_three_fields_and_the_trainer_refuses_up_front_and_switches_off(monkeypatch):
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    opt = OptimizationParams()
    assert (opt.lambda_multi_view_geo, opt.multi_view_from_iter, opt.multi_view_pix_max) == (0.0, 7000, 1.0)
    on = OptimizationParams(lambda_multi_view_geo=0.05, multi_view_from_iter=5, multi_view_pix_max=2.0)

    class Plain:
        def update_learning_rate(self, iteration):
            pass

    class Fork:
        _dirs_prob = torch.zeros(4, 3)

    class Dataset:
        grow_dir = True

    class Stop(Exception):
        pass

    calls = []

    def render(camera, model, pipe, bg, **kw):
        calls.append((camera, kw))
        raise Stop

    monkeypatch.setattr(trainer, "render", render)
    args = (on, None, torch.zeros(3), 10)
    with pytest.raises(ValueError, match="source_camera"):
        training_iteration(Plain(), _Cam, *args, cameras_extent=1.0)
    with pytest.raises(ValueError, match="pose_optimizer"):
        training_iteration(Plain(), _Cam, *args, cameras_extent=1.0, source_camera=_Cam, pose_optimizer=object())
    with pytest.raises(ValueError, match="grow / learned-split"):
        training_iteration(Plain(), _Cam, *args, cameras_extent=1.0, source_camera=_Cam, dataset=Dataset())
    from mvs_gaussian_splatting_amd.densify import is_fork
    if is_fork(Fork()):
        with pytest.raises(ValueError, match="grow / learned-split"):
            training_iteration(Fork(), _Cam, *args, cameras_extent=1.0, source_camera=_Cam)
    assert calls == [], "refused before anything is rendered"
    # on: the frame is rendered with its depth (and its median depth under depth_ratio)
    with pytest.raises(Stop):
        training_iteration(Plain(), _Cam, *args, cameras_extent=1.0, source_camera=_Cam)
    assert calls[-1][1].get("return_depth") is True and "return_median_depth" not in calls[-1][1]
    on.depth_ratio = 1.0
    with pytest.raises(Stop):
        training_iteration(Plain(), _Cam, *args, cameras_extent=1.0, source_camera=_Cam)
    assert calls[-1][1].get("return_depth") is True and calls[-1][1].get("return_median_depth") is True
    # off (lambda 0, or before multi_view_from_iter): source_camera is ignored and the render call is today's
    with pytest.raises(Stop):
        training_iteration(Plain(), _Cam, OptimizationParams(), None, torch.zeros(3), 10, cameras_extent=1.0)
    today = calls[-1][1]
    for off in (OptimizationParams(depth_ratio=1.0), on):
        with pytest.raises(Stop):
            training_iteration(Plain(), _Cam, off, None, torch.zeros(3), 4 if off is on else 10, cameras_extent=1.0,
                               source_camera=_Cam, pose_optimizer=object())
        assert list(calls[-1][1]) == list(today) and "return_depth" not in calls[-1][1]


def test_example_draws_a_source_only_while_the_term_is_on():
    import importlib.util
    import random
    spec = importlib.util.spec_from_file_location("example_train_mvs_loss", os.path.join(ROOT, "examples", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ring = [R.look_at(np.array([3 * math.cos(a), 0.0, 3 * math.sin(a)]), np.zeros(3), 32, 24, 30.0, 30.0)
            for a in np.arange(8) * (2 * math.pi / 8)]
    assert mod.source_views(ring, mod.OptimizationParams(), 4) is None
    sources = mod.source_views(ring, mod.OptimizationParams(lambda_multi_view_geo=0.05), 4)
    assert [sorted(s) for s in sources] == [sorted(((i - 1) % 8, (i + 1) % 8)) for i in range(8)]
    rng = random.Random(0)
    assert mod.draw_source(ring, None, 0, rng) is None and mod.draw_source(ring, [[]] * 8, 0, rng) is None
    drawn = {id(mod.draw_source(ring, sources, 3, rng)) for _ in range(40)}
    assert drawn == {id(ring[2]), id(ring[4])}


def test_scene_census_fragile_share_and_robust_pixels_of_every_kind():
    ref, depth, src, sdepth = L.scene()
    assert depth.shape == (37, 70) and sdepth.shape == (40, 48)
    assert R.focal(src) != R.focal(ref) and R.focal(src)[0] != R.focal(src)[1]
    row = R.source_rows(ref, [src], [sdepth])[0]
    fx, fy = R.focal(ref)
    has = depth > 0
    for depth_thresh in (None, L.DEPTH_THRESH):
        o = L.loss(depth, fx, fy, row, L.PIX_MAX, depth_thresh)
        o32 = L.loss(depth, fx, fy, row, L.PIX_MAX, depth_thresh, torch.float32)
        share = float((o["fragile"] & has).sum()) / float(has.sum())
        ok = has & ~o["fragile"]
        by_kind = {k: int(((o["kind"] == i) & ok).sum()) for i, k in enumerate(L.KINDS)}
        phi = o["phi"][o["valid"] & ok]
        atomic = int(((o["feeds"] >= 3) & ~o["tainted"]).sum())
        print(f"depth_thresh={depth_thresh}: {int(has.sum())} pixels with depth, fragile share {share:.2e}, robust pixels by "
              f"kind {by_kind}, phi of the robust valid pixels {phi.min():.3f} .. {phi.max():.3f}, {atomic} clean texels fed "
              f"by three or more pixels; value {o['value']:.6f}, float32 restatement off by {abs(o32['value'] - o['value']):.1e}")
        assert share <= 0.01
        assert by_kind["ok"] >= 200
        gates = ("behind", "outside", "hole", "pixel") + (("depth",) if depth_thresh is not None else ())
        assert all(by_kind[k] >= 50 for k in gates), by_kind
        assert depth_thresh is not None or by_kind["depth"] == 0
        # without the depth test (the default) phi covers (0.05, pix_max); with it the test cuts the large ones off
        assert depth_thresh is not None or (phi.min() < 0.05 and phi.max() > 0.95 * L.PIX_MAX and all(
            int(((phi >= a) & (phi < a + 0.1)).sum()) >= 10 for a in np.arange(0.0, 1.0, 0.1))), "phi covers (0.05, pix_max)"
        assert atomic >= 20
        # float32 takes every decision as float64 does on the robust pixels
        assert np.array_equal(o["valid"][ok], o32["valid"][ok])
        assert not o["grad_ref"][~o["valid"]].any() and not o["grad_src"][o["feeds"] == 0].any()
