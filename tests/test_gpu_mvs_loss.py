"""The multi-view geometric consistency loss on the HIP path (csrc/mvs_loss.hip, ABI v35; mvs.multi_view_geo_loss;
DESIGN.md §7.22) against the float64 restatement of tests/mvs_loss_restate.py.

Scene: ``mvs_loss_restate.scene`` -- a 70 x 37 reference (two x-tiles, ragged on both axes) and a 48 x 40 source with its
own focal lengths that stands close to the plane: pixels behind it, outside its image, over a hole, past ``pix_max`` and
(with the depth test) past ``depth_thresh``, and valid ones with phi over (0, pix_max) (tests/test_mvs_loss_host.py holds
the census).  Bars: ``n_valid`` exactly once the fragile pixels are set aside; the value within max(1e-6, 2 x the float32
restatement's own error against float64) plus what the fragile pixels can move it by; ``grad_ref`` on robust pixels and
``grad_src`` on texels only robust pixels feed, max-norm, within max(1e-6 of the map's largest gradient, 2 x the float32
restatement's error).  The observed figures are printed (-s).
"""
import functools
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import mvs_restate as R
import mvs_loss_restate as L

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _scene():
    ref, depth, src, sdepth = L.scene()
    return ref, depth, src, sdepth, R.source_rows(ref, [src], [sdepth])[0], R.focal(ref)


@functools.lru_cache(maxsize=None)
def _reference(depth_thresh):
    """float64 and float32 restatement of the scene; computed once, never modified."""
    _, depth, _, _, row, (fx, fy) = _scene()
    return (L.loss(depth, fx, fy, row, L.PIX_MAX, depth_thresh),
            L.loss(depth, fx, fy, row, L.PIX_MAX, depth_thresh, torch.float32))


def _row_on(dev, row):
    """The device copy of one restatement row -> (table tensor, the depth tensor it points into)."""
    from mvs_gaussian_splatting_amd import _lib
    sd = torch.from_numpy(np.ascontiguousarray(row["depth"], np.float32)).to(dev)
    t = _lib.GsrMvsSource()
    t.depth, t.width, t.height, t.fx, t.fy = sd.data_ptr(), row["W"], row["H"], float(row["fx"]), float(row["fy"])
    for i in range(16):
        t.ref_to_src[i], t.src_to_ref[i] = float(row["A"].reshape(-1)[i]), float(row["B"].reshape(-1)[i])
    return torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev), sd


def _raw(dev, depth, fx, fy, row, pix_max=L.PIX_MAX, depth_thresh=None, want_ref=True, want_src=True, calls=1):
    """``calls`` raw calls into outputs pre-filled with garbage -> (record, grad_ref or None, grad_src or None) on the device."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    H, W = depth.shape
    Hs, Ws = int(row["H"]), int(row["W"])
    d = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(dev)
    table, keep = _row_on(dev, row)
    record = torch.full((4,), float("nan"), device=dev)
    g_ref = torch.full((H, W), float("nan"), device=dev) if want_ref else None
    g_src = torch.full((Hs, Ws), float("nan"), device=dev) if want_src else None
    ws = torch.full((lib.gsr_mvs_geo_loss_workspace_bytes(H, W),), 0xAB, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for _ in range(calls):
            rc = lib.gsr_mvs_geo_loss_fwd_bwd(d.data_ptr(), H, W, float(fx), float(fy), table.data_ptr(), float(pix_max),
                                              0.0 if depth_thresh is None else float(depth_thresh), record.data_ptr(),
                                              None if g_ref is None else g_ref.data_ptr(),
                                              None if g_src is None else g_src.data_ptr(), Hs, Ws, ws.data_ptr(),
                                              torch.cuda.current_stream(dev).cuda_stream)
            assert rc == 0, lib.gsr_last_error()
        torch.cuda.synchronize()
    del keep
    return record, g_ref, g_src


def _n(record):
    return int(record.view(torch.int32)[1])


def _grad_bar(r32, r64, mask):
    scale = float(np.abs(r64).max())
    return max(1e-6, 2.0 * float(np.abs(r32.astype(np.float64) - r64)[mask].max()) / scale), scale


@pytest.mark.parametrize("depth_thresh", [None, L.DEPTH_THRESH])
def test_value_count_and_both_gradients_match_the_float64_restatement(gpu_device, depth_thresh):
    _, depth, _, _, row, (fx, fy) = _scene()
    r64, r32 = _reference(depth_thresh)
    record, g_ref, g_src = _raw(gpu_device, depth, fx, fy, row, depth_thresh=depth_thresh)
    rec = record.cpu().numpy()
    has = depth > 0
    fragile = r64["fragile"] & has
    robust = has & ~fragile
    # n_valid: the fragile pixels may fall either way; with them set aside (their depth removed) it is exact
    n_robust = int((r64["valid"] & robust).sum())
    assert n_robust <= _n(record) <= n_robust + int(fragile.sum())
    # ... and so is the value, at the bar without any slack, against the restatement of that same map
    aside = np.where(fragile, np.float32(0), depth)
    rec_a = _raw(gpu_device, aside, fx, fy, row, depth_thresh=depth_thresh, want_ref=False, want_src=False)[0]
    a64 = L.loss(aside, fx, fy, row, L.PIX_MAX, depth_thresh)
    a32 = L.loss(aside, fx, fy, row, L.PIX_MAX, depth_thresh, torch.float32)
    assert a64["n"] == n_robust and not (a64["fragile"] & (aside > 0)).any() and _n(rec_a) == n_robust
    err_a, bar_a = abs(float(rec_a[0]) - a64["value"]), max(1e-6, 2.0 * abs(a32["value"] - a64["value"]))
    print(f"[mvs loss] depth_thresh={depth_thresh}: fragile pixels set aside: n_valid {_n(rec_a)}, value {float(rec_a[0]):.7f} "
          f"off by {err_a:.2e} (bar {bar_a:.2e})")
    assert err_a <= bar_a, f"value without the fragile pixels: {err_a:.3e} > {bar_a:.3e}"
    # the value, over all pixels
    err_v = abs(float(rec[0]) - r64["value"])
    bar_v = max(1e-6, 2.0 * abs(r32["value"] - r64["value"])) + L.value_slack(r64)
    assert rec[3] == 0.0 and abs(float(rec[2]) - float(rec[0]) * max(_n(record), 1)) <= 1e-6 * float(rec[2]), "raw = value n"
    # grad_ref on the robust pixels; zero wherever the pixel is robustly not valid
    got_ref, got_src = g_ref.cpu().numpy().astype(np.float64), g_src.cpu().numpy().astype(np.float64)
    assert not np.isnan(got_ref).any() and not np.isnan(got_src).any(), "an output element was not written"
    bar_r, scale_r = _grad_bar(r32["grad_ref"], r64["grad_ref"], robust)
    err_r = float(np.abs(got_ref - r64["grad_ref"])[robust].max()) / scale_r
    assert not got_ref[robust & ~r64["valid"]].any() and not got_ref[~has].any()
    # grad_src on the texels that only robust pixels feed; zero where no pixel can reach
    clean = ~r64["tainted"]
    bar_s, scale_s = _grad_bar(r32["grad_src"], r64["grad_src"], clean)
    err_s = float(np.abs(got_src - r64["grad_src"])[clean].max()) / scale_s
    assert not got_src[clean & (r64["feeds"] == 0)].any()
    print(f"[mvs loss] depth_thresh={depth_thresh}: n_valid {_n(record)} (robust {n_robust}, {int(fragile.sum())} fragile); value "
          f"{rec[0]:.7f} off by {err_v:.2e} (bar {bar_v:.2e}); grad_ref max error {err_r:.2e} of {scale_r:.1f} (bar {bar_r:.2e}) "
          f"on {int(robust.sum())} pixels; grad_src {err_s:.2e} of {scale_s:.1f} (bar {bar_s:.2e}) on {int(clean.sum())} texels, "
          f"{int(((r64['feeds'] >= 3) & clean).sum())} of them fed by three or more pixels")
    assert err_v <= bar_v, f"value: {err_v:.3e} > {bar_v:.3e}"
    assert err_r <= bar_r, f"grad_ref: {err_r:.3e} > {bar_r:.3e}"
    assert err_s <= bar_s, f"grad_src: {err_s:.3e} > {bar_s:.3e}"


def test_repeat_runs_garbage_filled_outputs_and_each_gradient_alone(gpu_device):
    _, depth, _, _, row, (fx, fy) = _scene()
    r64, r32 = _reference(None)
    record, g_ref, g_src = _raw(gpu_device, depth, fx, fy, row)
    assert not torch.isnan(record).any() and not torch.isnan(g_ref).any() and not torch.isnan(g_src).any()
    clean = torch.from_numpy(~r64["tainted"]).to(gpu_device)
    bar_s, scale_s = _grad_bar(r32["grad_src"], r64["grad_src"], ~r64["tainted"])
    # twice into the same buffers: grad_src is zeroed by every call, not accumulated across calls
    rec2, ref2, src2 = _raw(gpu_device, depth, fx, fy, row, calls=2)
    assert _same_bits(rec2, record) and _same_bits(ref2, g_ref), "the value and grad_ref are the same bits from run to run"
    spread = float((src2.double() - g_src.double()).abs().max()) / scale_s
    print(f"[mvs loss] grad_src between runs: {spread:.2e} of its largest entry (atomic order; bar {bar_s:.2e})")
    assert spread <= bar_s, "grad_src is equal within the bar from run to run"
    assert float((src2.double() - g_src.double())[clean].abs().max()) / scale_s <= bar_s
    # each gradient alone: the other pointer NULL
    rec_r, only_ref, none = _raw(gpu_device, depth, fx, fy, row, want_src=False)
    assert none is None and _same_bits(rec_r, record) and _same_bits(only_ref, g_ref)
    rec_s, none, only_src = _raw(gpu_device, depth, fx, fy, row, want_ref=False)
    assert none is None and _same_bits(rec_s, record)
    assert float((only_src.double() - g_src.double()).abs().max()) / scale_s <= bar_s
    rec_0, _, _ = _raw(gpu_device, depth, fx, fy, row, want_ref=False, want_src=False)
    assert _same_bits(rec_0, record)


def test_dyadic_case_gives_the_hand_computed_value_and_gradients(gpu_device):
    ref, depth, src, sdepth = L.exact_case()
    row, (fx, fy) = R.source_rows(ref, [src], [sdepth])[0], R.focal(ref)
    record, g_ref, g_src = _raw(gpu_device, depth, fx, fy, row)
    w = math.exp(-0.5)
    assert _n(record) == 37 * 70
    assert abs(float(record[0]) - 0.5 * w) <= 2e-7 * 0.5 * w and abs(float(record[2]) - 37 * 70 * 0.5 * w) <= 2e-7 * 37 * 70 * 0.5 * w
    assert float((g_ref.double() + 0.25 * w).abs().max()) <= 1e-6 * 0.25 * w, "every reference pixel: -exp(-1/2) / 4"
    assert float((g_src[12:28, 8:40].double() - 0.25 * w).abs().max()) <= 1e-6 * 0.25 * w, "a fully fed texel: exp(-1/2) / 4"
    assert not g_src[:, :6].any() and not g_src[:10].any()
    for kw in ({"pix_max": 0.5}, {"depth_thresh": 0.5}):                   # phi = 1/2 is not < 1/2; |zb - d| = 4 is not < 2
        record, g_ref, g_src = _raw(gpu_device, depth, fx, fy, row, **kw)
        assert _n(record) == 0 and not record.any() and not g_ref.any() and not g_src.any()
    assert _n(_raw(gpu_device, depth, fx, fy, row, depth_thresh=1.5)[0]) == 37 * 70


def test_identical_cameras_and_a_source_facing_away(gpu_device):
    cam = R.Cam(np.eye(3), np.zeros(3), 70, 37, 64.0, 64.0)
    depth = np.full((37, 70), 4.0, np.float32)
    record, g_ref, g_src = _raw(gpu_device, depth, 64.0, 64.0, R.source_rows(cam, [cam], [depth])[0], depth_thresh=0.01)
    assert _n(record) == 36 * 69 and float(record[0]) == 0.0 and float(record[2]) == 0.0
    assert not g_ref.any() and not g_src.any(), "phi == 0: value 0, gradient 0, no NaN"
    ref, depth, _, _, _, (fx, fy) = _scene()
    away = R.look_at(np.array([0.5, 0.0, 0.0]), np.array([0.5, 0.0, -4.0]), 48, 40, 40.0, 40.0)
    row = R.source_rows(ref, [away], [np.full((40, 48), 3.0, np.float32)])[0]
    record, g_ref, g_src = _raw(gpu_device, depth, fx, fy, row)
    assert _n(record) == 0 and not record.any() and not g_ref.any() and not g_src.any(), "n_valid = 0: loss 0, no NaN"


@pytest.mark.parametrize("shape", [(1, 1, 48, 40), (65, 5, 48, 40), (70, 37, 2, 2)])
def test_edge_sizes_match_the_restatement(gpu_device, shape):
    W, H, Ws, Hs = shape
    ref = R.Cam(np.eye(3), np.zeros(3), W, H, 24.0, 20.0)
    src = R.look_at(np.array([0.35, -0.2, 0.0]), R.TARGET, Ws, Hs, 0.35 * Ws, 0.4 * Hs)
    depth, sdepth = R.render_depth(ref)[0], R.render_depth(src)[0]
    sdepth = (sdepth * np.float32(1.01)).astype(np.float32)
    row, (fx, fy) = R.source_rows(ref, [src], [sdepth])[0], R.focal(ref)
    r64, r32 = L.loss(depth, fx, fy, row, 2.0), L.loss(depth, fx, fy, row, 2.0, dtype=torch.float32)
    record, g_ref, g_src = _raw(gpu_device, depth, fx, fy, row, pix_max=2.0)
    robust = (depth > 0) & ~r64["fragile"]
    n_fragile = int((r64["fragile"] & (depth > 0)).sum())
    assert r64["n"] >= 1, "the case must have a valid pixel"
    assert abs(_n(record) - r64["n"]) <= n_fragile
    assert abs(float(record[0]) - r64["value"]) <= max(1e-6, 2 * abs(r32["value"] - r64["value"])) + L.value_slack(r64)
    bar_r, scale_r = _grad_bar(r32["grad_ref"], r64["grad_ref"], robust)
    assert float(np.abs(g_ref.cpu().numpy() - r64["grad_ref"])[robust].max()) / scale_r <= bar_r
    clean = ~r64["tainted"]
    if clean.any():
        bar_s, scale_s = _grad_bar(r32["grad_src"], r64["grad_src"], clean)
        assert float(np.abs(g_src.cpu().numpy() - r64["grad_src"])[clean].max()) / scale_s <= bar_s
    print(f"[mvs loss] {W} x {H} into {Ws} x {Hs}: n_valid {_n(record)}, value {float(record[0]):.6f}")


def test_wrapper_equals_the_raw_call_and_autograd_scales_by_the_upstream_factor(gpu_device):
    from mvs_gaussian_splatting_amd import multi_view_geo_loss
    ref, depth, src, sdepth, row, (fx, fy) = _scene()
    r64, r32 = _reference(None)
    bar_s, scale_s = _grad_bar(r32["grad_src"], r64["grad_src"], ~r64["tainted"])
    for depth_thresh in (None, L.DEPTH_THRESH):
        record, g_ref, g_src = _raw(gpu_device, depth, fx, fy, row, depth_thresh=depth_thresh)
        d = torch.from_numpy(depth).to(gpu_device)[None].requires_grad_(True)
        sd = torch.from_numpy(sdepth).to(gpu_device).requires_grad_(True)
        loss, rec = multi_view_geo_loss(d, ref, sd, src, pix_max=L.PIX_MAX, depth_thresh=depth_thresh, return_record=True)
        assert loss.dim() == 0 and loss.device == d.device and _same_bits(rec, record) and _same_bits(loss.detach(), record[0])
        (-2.5 * loss).backward()                                           # an upstream factor other than 1
        k = torch.tensor(-2.5, device=gpu_device) * (1.0 / torch.tensor(float(max(_n(record), 1)), device=gpu_device))
        assert d.grad.shape == d.shape and _same_bits(d.grad[0], g_ref * k), "grad_ref * (upstream / n_valid), one multiply"
        assert float((sd.grad.double() - (g_src * k).double()).abs().max()) <= bar_s * scale_s * abs(float(k))
    # each input's gradient is optional on its own; without any the call is forward only
    d = torch.from_numpy(depth).to(gpu_device).requires_grad_(True)
    sd = torch.from_numpy(sdepth).to(gpu_device)
    multi_view_geo_loss(d, ref, sd, src).backward()
    assert d.grad is not None and sd.grad is None
    sd.requires_grad_(True)
    multi_view_geo_loss(d.detach(), ref, sd, src).backward()
    assert sd.grad is not None and bool(sd.grad.any())
    plain = multi_view_geo_loss(d.detach(), ref, sd.detach(), src)
    assert not plain.requires_grad and _same_bits(plain, _raw(gpu_device, depth, fx, fy, row)[0][0])


# ---- the trainer ---------------------------------------------------------------------------------------------------------
PLANE = (0.3, -0.2, 4.0)         # view-space plane z = 4 + 0.3 x - 0.2 y (the scene of test_gpu_normal_consistency.py)


@pytest.fixture(scope="module")
def problem(gpu_device):
    """Two 64x48 views, 15 degrees apart, of 400 flat Gaussians on a tilted plane (the cloud of tests/test_gpu_joint_frame.py)."""
    import train as example
    cams, bg, _ = example.make_problem(gpu_device, P=600, W=64, H=48, n_views=24)
    g = torch.Generator().manual_seed(11)
    xy = (torch.rand(400, 2, generator=g) - 0.5) * torch.tensor([1.5, 1.2])
    view = torch.cat((xy, (PLANE[2] + PLANE[0] * xy[:, :1] + PLANE[1] * xy[:, 1:]), torch.ones(400, 1)), dim=1)
    world = (view.to(gpu_device) @ torch.linalg.inv(cams[0].world_view_transform.float()))[:, :3].contiguous()
    colors = torch.rand(400, 3, generator=g).to(gpu_device)
    return cams[:2], bg, (world, colors)


def _plane_model(problem, opt):
    import train as example
    model = example.make_model(problem, opt)
    with torch.no_grad():
        model._opacity.fill_(2.0)
        model._scaling[:, :2] = math.log(0.07)
        model._scaling[:, 2] = math.log(0.004)
    return model


def _group_grads(model):
    return {g["name"]: (None if g["params"][0].grad is None else g["params"][0].grad.detach().clone())
            for g in model.optimizer.param_groups}


def _two_frame_loss(model, cams, bg, part):
    """The trainer's two frames by hand; ``part``: "main" (the colour loss of frame 0), "mv" (the multi-view term), "both"."""
    from mvs_gaussian_splatting_amd import l1_dssim_loss, multi_view_geo_loss, render, surface_depth
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    pkgs = [render(c, model, PipelineParams(), bg, return_depth=True) for c in cams]
    main = l1_dssim_loss(pkgs[0]["render"], cams[0].original_image, 0.2)
    surf = [surface_depth(p["depth"], p["alpha"], None, 0.0) for p in pkgs]
    mv, record = multi_view_geo_loss(surf[0], cams[0], surf[1], cams[1], return_record=True)
    return {"main": main, "mv": 0.05 * mv, "both": main + 0.05 * mv}[part], record


def test_two_renders_before_one_backward_give_the_sum_of_the_separate_gradients(gpu_device, problem):
    import train as example
    from grad_util import TOL
    cams, bg, _ = problem
    opt = example.small_opt(40)
    grads = {}
    for part in ("main", "mv", "both"):
        model = _plane_model(problem, opt)
        loss, record = _two_frame_loss(model, cams, bg, part)
        loss.backward()
        grads[part] = _group_grads(model)
    n_valid = _n(record)
    print(f"[mvs loss] two frames: {n_valid} valid pixels of {64 * 48}, term {float(loss.detach()):.5f}")
    assert n_valid >= 200, "the two views must agree on enough of the plane for the test to mean anything"
    rows = []
    for k, joint in grads["both"].items():
        parts = [g[k] for g in (grads["main"], grads["mv"]) if g[k] is not None]
        assert joint is not None and parts and bool(torch.isfinite(joint).all()), k
        want = sum(p.double() for p in parts)
        if not bool(want.any()):                                          # f_rest at SH degree 0: no gradient either way
            assert not bool(joint.any()), k
            continue
        e = float((joint.double() - want).abs().max()) / float(want.abs().max())
        rows.append(f"{k} {e:.1e}")
        assert e <= TOL, f"group {k}: one backward over two frames is {e:.2e} off the sum of the separate backwards"
    assert grads["mv"]["xyz"] is not None and float(grads["mv"]["xyz"].abs().max()) > 0, "the term reaches the positions"
    print(f"[mvs loss] one backward vs the sum of two (bar {TOL:.0e}): " + ", ".join(rows))


def test_training_iteration_with_the_term_and_bit_identity_without_it(gpu_device, problem):
    import train as example
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    cams, bg, _ = problem
    pipe, extent = PipelineParams(), example.CAMERAS_EXTENT
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    snapshot = lambda m: [getattr(m, n).detach().clone() for n in names]      # noqa: E731
    for optimizer_type in ("default", "sparse_adam"):
        on = example.small_opt(40, lambda_multi_view_geo=0.05, multi_view_from_iter=0, optimizer_type=optimizer_type)
        model = _plane_model(problem, on)
        before = snapshot(model)
        loss = training_iteration(model, cams[0], on, pipe, bg, 1, cameras_extent=extent, source_camera=cams[1])
        plain = _plane_model(problem, example.small_opt(40, optimizer_type=optimizer_type))
        base = training_iteration(plain, cams[0], example.small_opt(40, optimizer_type=optimizer_type), pipe, bg, 1,
                                  cameras_extent=extent)
        print(f"[mvs loss] one iteration ({optimizer_type}) with lambda_multi_view_geo = 0.05: {float(loss):.6f}; without: "
              f"{float(base):.6f}")
        assert math.isfinite(float(loss)) and float(loss) > float(base), "the term adds to the loss"
        after = snapshot(model)
        assert all(bool(torch.isfinite(a).all()) for a in after) and not torch.equal(after[0], before[0])
        assert not torch.equal(after[0], snapshot(plain)[0]), "the term moves the positions"
        assert float(model.denom.sum()) > 0, "the densification statistics were not taken"
    with pytest.raises(ValueError, match="source_camera"):
        training_iteration(_plane_model(problem, on), cams[0], on, pipe, bg, 1, cameras_extent=extent)
    # lambda = 0, not yet switched on, and options that do not know the fields: the call made without the new arguments
    zero = example.small_opt(40)
    late = example.small_opt(40, lambda_multi_view_geo=0.05, multi_view_from_iter=7000)
    parent = types.SimpleNamespace(**{k: getattr(zero, k) for k in dir(OptimizationParams)
                                      if not k.startswith("_") and not k.startswith(("lambda_multi_view", "multi_view_"))})
    assert zero.lambda_multi_view_geo == 0.0 and not hasattr(parent, "lambda_multi_view_geo")
    results = []
    for o, kw in ((zero, {}), (zero, {"source_camera": cams[1]}), (late, {"source_camera": cams[1]}), (parent, {})):
        m = _plane_model(problem, zero)
        out = [training_iteration(m, cams[0], o, pipe, bg, it, cameras_extent=extent, **kw) for it in (1, 2)]
        results.append((out, snapshot(m)))
    for other in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0][0], other[0])), "the loss differs"
        assert all(torch.equal(x, y) for x, y in zip(results[0][1], other[1])), "a parameter differs"
