"""CPU-side checks of the multi-view photometric (NCC) loss (csrc/mvs_ncc.hip, ABI v36; mvs.multi_view_ncc_loss;
DESIGN.md §7.23): the torch restatement against central finite differences, against identical cameras, against a rescaled
normal map and along its own gradient; every refusal of the wrapper and of the entry point -- which all come before a GPU
is asked for -- the ABI, ``gray_image``, the trainer's refusals and off-switch, and what the scene of
tests/test_gpu_mvs_ncc.py must hold."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import mvs_restate as R
import mvs_ncc_restate as N


@functools.lru_cache(maxsize=None)
def _scene():
    ref, depth, normal, gray, src, sdepth, sgray = N.scene()
    return depth, normal, gray, N.row_of(ref, src, sdepth), sgray, R.focal(ref)


@functools.lru_cache(maxsize=None)
def _base():
    depth, normal, gray, row, sgray, (fx, fy) = _scene()
    return N.loss(depth, normal, gray, fx, fy, row, sgray)


def test_restated_float64_gradients_agree_with_central_finite_differences():
    depth, normal, gray, row, sgray, (fx, fy) = _scene()
    base = _base()
    robust = base["counted"] & ~base["fragile"]
    ys, xs = np.nonzero(robust)
    pick = np.linspace(0, len(ys) - 1, 6).astype(int)
    H, W = depth.shape
    worst = 0.0
    for y, x in zip(ys[pick], xs[pick]):
        w0 = base["w"][y, x]                                               # the weight is a constant of the gradient
        inputs = [("depth", None, float(depth[y, x]))] + [("normal", c, float(np.abs(normal[:, y, x]).max())) for c in range(3)]
        for which, c, size in inputs:
            h = 1e-6 * size
            vals = []
            for sign in (1.0, -1.0):
                dm, nm = depth.astype(np.float64), normal.astype(np.float64)
                if which == "depth":
                    dm[y, x] += sign * h
                else:
                    nm[c, y, x] += sign * h
                o = N.loss(dm, nm, gray, fx, fy, row, sgray, pixels=[y * W + x], round_inputs=False)
                vals.append(w0 * o["ncc"][y, x])
            fd = (vals[0] - vals[1]) / (2 * h)
            g = float(base["grad_depth"][y, x] if which == "depth" else base["grad_normal"][c, y, x])
            scale = float(np.abs(base["grad_depth"]).max() if which == "depth" else np.abs(base["grad_normal"][:, y, x]).max())
            worst = max(worst, abs(fd - g) / scale)
            assert abs(fd - g) <= 1e-6 * scale, (y, x, which, c, fd, g)
    print(f"worst difference from central differences {worst:.2e} of the gradient's scale")
    # the kernel's forward-mode form of the gradient is the same function
    stated = N.loss(depth, normal, gray, fx, fy, row, sgray, grad="stated")
    for k in ("grad_depth", "grad_normal"):
        assert np.abs(stated[k] - base[k]).max() <= 1e-10 * np.abs(base[k]).max(), k
    assert stated["n"] == base["n"] and stated["raw"] == base["raw"]


def test_identical_cameras_warp_by_the_identity_whatever_the_depth_and_normal():
    ref, depth, normal, _, _, _, _ = N.scene()
    gray = N.contrast_image(*depth.shape)          # enough contrast in every patch for the 1e-8 of the denominator
    row = N.row_of(ref, ref, depth)
    fx, fy = R.focal(ref)
    for dtype in (torch.float64, torch.float32):
        o = N.loss(depth, normal, gray, fx, fy, row, gray, dtype=dtype)
        assert o["n"] >= 800, "most interior pixels are valid"
        worst = float(np.nanmax(o["ncc"][o["counted"]]))
        print(f"identical cameras ({dtype}): {o['n']} counted pixels, largest ncc {worst:.2e}")
        assert worst <= 1e-6
        assert not o["grad_depth"].any() and not o["grad_normal"].any(), "A[3, 0:3] = 0: the warp does not see the plane"
        assert not np.isnan(o["grad_depth"]).any() and not np.isnan(o["grad_normal"]).any()


def test_scaling_the_normal_map_by_a_positive_field_changes_neither_value_nor_depth_gradient():
    depth, normal, gray, row, sgray, (fx, fy) = _scene()
    base = _base()
    yy, xx = np.meshgrid(np.arange(depth.shape[0]), np.arange(depth.shape[1]), indexing="ij")
    field = 0.05 + 3.0 * (1.1 + np.sin(xx / 3.0) * np.cos(yy / 4.0))
    o = N.loss(depth, normal.astype(np.float64) * field[None], gray, fx, fy, row, sgray, round_inputs=False)
    assert o["n"] == base["n"] and np.array_equal(o["kind"], base["kind"])
    assert abs(o["value"] - base["value"]) <= 1e-12 * base["value"]
    assert np.abs(o["grad_depth"] - base["grad_depth"]).max() <= 1e-10 * np.abs(base["grad_depth"]).max()
    # the normal's gradient is of degree -1, and orthogonal to the normal (Euler)
    assert np.abs(o["grad_normal"] * field[None] - base["grad_normal"]).max() <= 1e-10 * np.abs(base["grad_normal"]).max()
    radial = (base["grad_normal"] * normal.astype(np.float64)).sum(0)
    assert np.abs(radial).max() <= 1e-10 * np.abs(base["grad_normal"]).max()


def test_true_geometry_scores_below_the_perturbed_map_and_a_gradient_step_lowers_the_loss():
    depth, normal, gray, row, sgray, (fx, fy) = _scene()
    base = _base()
    ref, tdepth, tnormal, tgray, src, tsdepth, tsgray = N.true_maps()
    true = N.loss(tdepth, tnormal, tgray, fx, fy, N.row_of(ref, src, tsdepth), tsgray)
    print(f"true geometry: {true['n']} counted, loss {true['value']:.3e}; perturbed: {base['n']} counted, loss {base['value']:.3e}")
    assert true["n"] >= 1000 and true["value"] < 0.1 * base["value"]
    assert float(np.nanmax(true["ncc"][true["counted"]])) < N.NCC_MAX
    step_d = 1e-3 * depth.max() / np.abs(base["grad_depth"]).max()
    step_n = 1e-3 * np.abs(normal).max() / np.abs(base["grad_normal"]).max()
    moved = N.loss(depth.astype(np.float64) - step_d * base["grad_depth"], normal.astype(np.float64) - step_n * base["grad_normal"],
                   gray, fx, fy, row, sgray, round_inputs=False)
    same = base["counted"] & moved["counted"]
    before, after = float((base["w"] * base["ncc"])[same].sum()), float((base["w"] * moved["ncc"])[same].sum())
    print(f"one step along minus the gradient: raw sum over the {int(same.sum())} pixels counted both times {before:.6f} -> "
          f"{after:.6f}; loss {base['value']:.6f} -> {moved['value']:.6f}")
    assert same.sum() >= 0.98 * base["n"]
    assert after < before and moved["value"] < base["value"]


def test_scene_census_fragile_share_and_every_kind():
    ref, depth, normal, gray, src, sdepth, sgray = N.scene()
    assert depth.shape == (37, 70) and sdepth.shape == (40, 48) and normal.shape == (3, 37, 70)
    assert R.focal(src) != R.focal(ref) and R.focal(src)[0] != R.focal(src)[1]
    base = _base()
    fx, fy = R.focal(ref)
    o32 = N.loss(depth, normal, gray, fx, fy, N.row_of(ref, src, sdepth), sgray, dtype=torch.float32)
    valid = base["kind"] >= N.KINDS.index("ncc")                           # every gate passed: the pixel has an ncc
    fragile = base["fragile"] & (depth > 0)
    by_kind = {k: int(((base["kind"] == i) & ~fragile).sum()) for i, k in enumerate(N.KINDS)}
    ncc = base["ncc"][base["counted"]]
    print(f"{int((depth > 0).sum())} pixels with depth, {int(valid.sum())} valid, {int(fragile.sum())} fragile; robust pixels by "
          f"kind {by_kind}; ncc of the counted pixels {ncc.min():.2e} .. {ncc.max():.3f}, mean {ncc.mean():.3e}; value "
          f"{base['value']:.6f}, float32 restatement off by {abs(o32['value'] - base['value']):.1e}")
    assert fragile.sum() <= 0.05 * valid.sum()
    assert all(v >= 20 for v in by_kind.values()), by_kind
    robust = (depth > 0) & ~fragile
    assert np.array_equal(base["kind"][robust], o32["kind"][robust]), "float32 takes every decision as float64 does"
    assert not base["grad_depth"][~base["counted"]].any() and not base["grad_normal"][:, ~base["counted"]].any()
    lens = np.linalg.norm(normal, axis=0)
    assert lens.min() > 0 and lens.max() > 2 * lens.min(), "the normal map is not normalised"
    assert float(np.abs(base["grad_depth"]).max()) > 0.1 and float(np.abs(base["grad_normal"]).max()) > 0.05


def test_gray_image_weights_and_caching():
    from mvs_gaussian_splatting_amd import gray_image
    from mvs_gaussian_splatting_amd.mvs import GRAY_WEIGHTS
    assert GRAY_WEIGHTS == (0.299, 0.587, 0.114)
    g = torch.Generator().manual_seed(3)
    rgb = torch.rand(3, 5, 7, generator=g)
    want = 0.299 * rgb[0].double() + 0.587 * rgb[1].double() + 0.114 * rgb[2].double()
    got = gray_image(rgb)
    assert got.shape == (5, 7) and got.dtype == torch.float32 and got.is_contiguous()
    assert float((got.double() - want).abs().max()) <= 2e-7
    for c, wgt in enumerate(GRAY_WEIGHTS):
        unit = torch.zeros(3, 2, 2)
        unit[c] = 1.0
        assert torch.equal(gray_image(unit), torch.full((2, 2), wgt, dtype=torch.float32))
    assert torch.equal(gray_image(got), got) and torch.equal(gray_image(got[None]), got)
    for bad in (rgb.double(), torch.zeros(3, 5, 7, dtype=torch.uint8)):
        with pytest.raises(TypeError):
            gray_image(bad)
    for bad in (torch.zeros(2, 5, 7), torch.zeros(1, 3, 5, 7), torch.zeros(7)):
        with pytest.raises(ValueError):
            gray_image(bad)
    with pytest.raises(TypeError):
        gray_image(object())

    class Cam:
        original_image = rgb
    cam = Cam()
    first = gray_image(cam)
    assert torch.equal(first, got) and gray_image(cam) is first, "converted once"
    cam.original_image = rgb.clone()                                       # another photograph: converted again
    assert gray_image(cam) is not first


def test_every_python_refusal_comes_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, multi_view_ncc_loss
    ref, depth, normal, gray, src, sdepth, sgray = N.scene()
    d, n, g, sd, sg = (torch.from_numpy(np.ascontiguousarray(a)) for a in (depth, normal, gray, sdepth, sgray))
    good = dict(depth=d, normal=n, image=g, camera=ref, src_depth=sd, src_image=sg, src_camera=src)
    px = torch.arange(5, dtype=torch.int32)
    for kw in ({"depth": d.t().contiguous()}, {"src_depth": d}, {"src_depth": sd[None, None]}, {"normal": n[:2]},
               {"normal": n[None]}, {"normal": n.permute(1, 2, 0).contiguous()}, {"image": sg}, {"src_image": g},
               {"image": g[None, None]}, {"image": torch.zeros(2, 37, 70)}, {"pix_max": 0.0}, {"pix_max": -1.0},
               {"pix_max": math.inf}, {"pix_max": math.nan}, {"ncc_max": 0.0}, {"ncc_max": 2.5}, {"ncc_max": math.nan},
               {"min_cos": -0.1}, {"min_cos": 1.0}, {"min_cos": math.nan}, {"patch_radius": 0}, {"patch_radius": 5},
               {"patch_radius": 2.0}, {"patch_radius": True}, {"n_samples": 0}, {"n_samples": -4}, {"n_samples": 2.5},
               {"n_samples": 10, "pixels": px}, {"pixels": px[:0]}, {"pixels": torch.zeros(37 * 70 + 1, dtype=torch.int32)},
               {"generator": torch.Generator()}, {"src_depth": sd.to("meta")}, {"normal": n.to("meta")},
               {"image": g.to("meta")}, {"pixels": px.to("meta")}):
        with pytest.raises(ValueError):
            multi_view_ncc_loss(**{**good, **kw})
    tall = R.Cam(np.eye(3), np.zeros(3), 1, 2 ** 26, 1.0, 2.0 ** 26)      # 2^26 pixels, but 2^24 tiles of 256 lanes
    with pytest.raises(ValueError, match="work-items"):
        multi_view_ncc_loss(torch.empty((2 ** 26, 1)), n, g, tall, sd, sg, src)
    for kw in ({"depth": depth}, {"depth": d.double()}, {"src_depth": sd.half()}, {"src_depth": None}, {"normal": normal},
               {"normal": n.double()}, {"image": gray}, {"image": g.double()}, {"src_image": None}, {"src_image": sg.half()},
               {"pixels": [1, 2]}, {"pixels": px.long()}, {"pixels": px[None]}):
        with pytest.raises(TypeError):
            multi_view_ncc_loss(**{**good, **kw})
    bad_cam = R.Cam(np.eye(3), np.zeros(3), 48, 40, 32.0, 32.0)
    bad_cam.world_view_transform = torch.zeros(3, 4)
    with pytest.raises(ValueError):
        multi_view_ncc_loss(d, n, g, ref, sd, sg, bad_cam)
    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError):
        multi_view_ncc_loss(**good)
    ref.original_image, src.original_image = g[None].expand(3, -1, -1), sg[None].expand(3, -1, -1)
    with pytest.raises(_lib.GsrError):
        multi_view_ncc_loss(d[None].requires_grad_(True), n, ref, ref, sd, src, src, n_samples=100, return_record=True)
    with pytest.raises(_lib.GsrError):
        multi_view_ncc_loss(**good, pixels=px, patch_radius=1)


def test_library_exports_the_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    import mvs_gaussian_splatting_amd as pkg
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_mvs_ncc_loss_workspace_bytes", "gsr_mvs_ncc_loss_fwd_bwd"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 36
    for name in ("multi_view_ncc_loss", "gray_image"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)) and name in pkg.mvs.__all__
    # one (double, uint32) pair per 64 x 4 tile, or per 256 list entries; 0 for a shape the call refuses
    ws = lib.gsr_mvs_ncc_loss_workspace_bytes
    assert ws(37, 70, 0) == 2 * 10 * 12 and ws(1, 1, 0) == 12 and ws(5, 65, 0) == 4 * 12
    assert ws(37, 70, 1) == 12 and ws(37, 70, 256) == 12 and ws(37, 70, 257) == 24 and ws(37, 70, 2590) == 11 * 12
    assert ws(0, 4, 0) == 0 and ws(4, -1, 0) == 0 and ws(2 ** 14 + 1, 2 ** 14, 0) == 0 and ws(2 ** 28, 1, 0) == 0
    assert ws(37, 70, -1) == 0 and ws(37, 70, 2591) == 0


def test_raw_abi_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    ptr = C.addressof(buf)
    assert ptr % 8 == 0
    good = dict(depth=ptr, normal=ptr, gray=ptr, H=4, W=4, fx=1.0, fy=1.0, source=ptr, sgray=ptr, pixels=ptr, n=4, radius=3,
                pix=1.0, ncc=0.9, cos=0.05, record=ptr, gd=ptr, gn=ptr, ws=ptr)
    call = lambda **kw: lib.gsr_mvs_ncc_loss_fwd_bwd(*{**good, **kw}.values(), None)      # noqa: E731
    inf, nan = math.inf, math.nan
    bad = [{"depth": None}, {"normal": None}, {"gray": None}, {"source": None}, {"sgray": None}, {"record": None},
           {"ws": None}, {"H": 0}, {"W": 0}, {"H": -3}, {"H": 2 ** 14 + 1, "W": 2 ** 14}, {"H": 2 ** 28, "W": 1, "n": 0},
           {"n": -1}, {"n": 17}, {"n": 17, "pixels": None}, {"radius": 0}, {"radius": 5}, {"radius": -1},
           {"ncc": 0.0}, {"ncc": -0.5}, {"ncc": 2.5}, {"ncc": nan}, {"ncc": inf}, {"cos": -0.01}, {"cos": 1.0}, {"cos": nan},
           {"cos": inf}]
    bad += [{k: v} for k in ("fx", "fy", "pix") for v in (0.0, -1.0, inf, nan)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.gsr_last_error()
    for kw in ({"depth": ptr + 2}, {"normal": ptr + 2}, {"gray": ptr + 1}, {"sgray": ptr + 2}, {"pixels": ptr + 2},
               {"record": ptr + 1}, {"gd": ptr + 2}, {"gn": ptr + 2}, {"source": ptr + 4}, {"ws": ptr + 4}):
        assert call(**kw) == -3, kw


class _Cam:
    FoVx = FoVy = 1.0
    image_width, image_height = 8, 8
    original_image = torch.zeros(3, 8, 8)


def test_optimization_params_gain_the_fields_and_the_trainer_refuses_up_front_and_switches_off(monkeypatch):
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    opt = OptimizationParams()
    assert (opt.lambda_multi_view_ncc, opt.multi_view_ncc_samples, opt.multi_view_patch_radius, opt.multi_view_ncc_max) == \
        (0.0, 102400, 3, 0.9)
    on = OptimizationParams(lambda_multi_view_ncc=0.15, multi_view_from_iter=5)

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
    # on: the frame is rendered with its depth and its normals (and its median depth under depth_ratio)
    with pytest.raises(Stop):
        training_iteration(Plain(), _Cam, *args, cameras_extent=1.0, source_camera=_Cam)
    kw = calls[-1][1]
    assert kw.get("return_depth") is True and kw.get("return_normals") is True and "return_median_depth" not in kw
    on.depth_ratio = 1.0
    with pytest.raises(Stop):
        training_iteration(Plain(), _Cam, *args, cameras_extent=1.0, source_camera=_Cam)
    assert calls[-1][1].get("return_normals") is True and calls[-1][1].get("return_median_depth") is True
    # the geometric term alone still renders without normals
    with pytest.raises(Stop):
        training_iteration(Plain(), _Cam, OptimizationParams(lambda_multi_view_geo=0.05, multi_view_from_iter=5), None,
                           torch.zeros(3), 10, cameras_extent=1.0, source_camera=_Cam)
    assert calls[-1][1].get("return_depth") is True and "return_normals" not in calls[-1][1]
    # off (lambda 0 whatever the other new fields say, or before multi_view_from_iter): the render call is today's
    with pytest.raises(Stop):
        training_iteration(Plain(), _Cam, OptimizationParams(), None, torch.zeros(3), 10, cameras_extent=1.0)
    today = calls[-1][1]
    others = OptimizationParams(multi_view_ncc_samples=7, multi_view_patch_radius=9, multi_view_ncc_max=-1.0, depth_ratio=1.0)
    for off in (others, on):
        with pytest.raises(Stop):
            training_iteration(Plain(), _Cam, off, None, torch.zeros(3), 4 if off is on else 10, cameras_extent=1.0,
                               source_camera=_Cam, pose_optimizer=object())
        assert list(calls[-1][1]) == list(today) and "return_depth" not in calls[-1][1]


def test_example_selects_sources_when_either_multi_view_weight_is_positive():
    import importlib.util
    spec = importlib.util.spec_from_file_location("example_train_mvs_ncc", os.path.join(ROOT, "examples", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    ring = [R.look_at(np.array([3 * math.cos(a), 0.0, 3 * math.sin(a)]), np.zeros(3), 32, 24, 30.0, 30.0)
            for a in np.arange(8) * (2 * math.pi / 8)]
    assert mod.source_views(ring, mod.OptimizationParams(), 4) is None
    assert mod.source_views(ring, mod.OptimizationParams(multi_view_ncc_samples=10), 4) is None
    for kw in ({"lambda_multi_view_ncc": 0.15}, {"lambda_multi_view_ncc": 0.15, "lambda_multi_view_geo": 0.05}):
        sources = mod.source_views(ring, mod.OptimizationParams(**kw), 4)
        assert [sorted(s) for s in sources] == [sorted(((i - 1) % 8, (i + 1) % 8)) for i in range(8)]
