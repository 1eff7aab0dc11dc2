"""The evaluation path on the GPU: fused L1 / PSNR / SSIM per view (csrc/metrics.hip + the forward-only SSIM tile kernel),
the device-side running sums of a report, the 8-bit HWC output, and evaluate_views.

Bars, always against float64 values (the fixture's, or the reference's expressions on .double() inputs on the device),
never against the code under test: L1 and the six raw sums rel <= 1e-6, SSIM rel <= 1e-5 (the project's bars for the same
quantities, tests/test_gpu_parity.py:375,382); PSNR abs <= 1e-5 dB (a relative error e of the mse moves it by 4.3 e dB,
4.3e-6 at e = 1e-6, plus the rounding of a float32 near 16-32 dB, 1.9e-6 per ulp); sums over n views: n times the bar.
tests/test_eval_host.py shows a float32 restatement of the kernels, and the reference's own float32 results, inside them.
"""
import math
import os

import numpy as np
import pytest
import torch

from eval_restate import ABS_PSNR_DB, REL_L1, REL_SSIM, expected_f64, rel

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_metrics.npz")


def _pair(dev, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(3, H, W, generator=g)
    img = gt + 0.05 * torch.randn(3, H, W, generator=g) + 0.02
    return img.to(dev), gt.to(dev)


def _check(tag, got, want, with_ssim=False, whole=False):
    """got: image_metrics' dict; want: float64 values (dict of tensors / numpy scalars)"""
    rec = got["record"].double().cpu()
    f = lambda v: float(torch.as_tensor(v, dtype=torch.float64).reshape(-1)[0])
    errs = {"l1": rel(f(got["l1"]), f(want["l1"])), "sums": rel(rec[3:9], torch.as_tensor(want["sums"]).cpu()),
            "psnr": abs(f(got["psnr"]) - f(want["psnr1"] if whole else want["psnr"])),
            "psnr3": float((rec[9:12] - torch.as_tensor(want["psnr3"]).double().cpu().reshape(3)).abs().max())}
    if with_ssim:
        errs["ssim"] = rel(f(got["ssim"]), f(want["ssim"]))
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["l1"] <= REL_L1 and errs["sums"] <= REL_L1, (tag, errs)
    assert errs["psnr"] <= ABS_PSNR_DB and errs["psnr3"] <= ABS_PSNR_DB, (tag, errs)
    assert not with_ssim or errs["ssim"] <= REL_SSIM, (tag, errs)


@pytest.mark.parametrize("name", ["a", "b"])
def test_fixture_parity(gpu_device, name):
    """L1, both PSNR forms and SSIM against the reference's float64 results on the clamped pair; the drop-ins psnr / ssim
    on the pre-clamped pair as metrics.py calls them."""
    from mvs_gaussian_splatting_amd import image_metrics, psnr, ssim
    g = np.load(GOLDEN)
    x, gt = torch.tensor(g[f"{name}_img"], device=gpu_device), torch.tensor(g[f"{name}_gt"], device=gpu_device)
    want = {"l1": g[f"{name}_l1_f64"], "sums": g[f"{name}_sums_f64"], "psnr": g[f"{name}_psnr_mean_f64"],
            "psnr1": g[f"{name}_psnr1_f64"], "psnr3": g[f"{name}_psnr3_f64"], "ssim": g[f"{name}_ssim_f64"]}
    _check(name, image_metrics(x, gt, clamp=True, with_ssim=True), want, with_ssim=True)
    _check(name + " whole", image_metrics(x, gt, clamp=True, whole_image_psnr=True), want, whole=True)
    xc, gc = x.clamp(0.0, 1.0), gt.clamp(0.0, 1.0)
    p3, p1 = psnr(xc, gc), psnr(xc[None], gc[None])
    assert p3.shape == (3, 1) and p1.shape == (1, 1)
    assert float((p3.double().cpu() - torch.tensor(g[f"{name}_psnr3_f64"])).abs().max()) <= ABS_PSNR_DB
    assert abs(float(p1) - g[f"{name}_psnr1_f64"].item()) <= ABS_PSNR_DB
    for s in (ssim(xc, gc), ssim(xc[None], gc[None])):
        assert s.dim() == 0 and rel(float(s), g[f"{name}_ssim_f64"]) <= REL_SSIM
    p2 = psnr(torch.stack((xc, gc)), torch.stack((gc, gc)))          # a batch: one value per image, inf for the equal pair
    assert p2.shape == (2, 1) and abs(float(p2[0]) - g[f"{name}_psnr1_f64"].item()) <= ABS_PSNR_DB and math.isinf(float(p2[1]))


def test_five_view_accumulation_and_inf_case(gpu_device):
    from mvs_gaussian_splatting_amd import EvalAccumulator, image_metrics, psnr
    g = np.load(GOLDEN)
    acc = EvalAccumulator(gpu_device)
    run = g["seq_running_f64"]
    for i in range(5):
        image_metrics(torch.tensor(g["seq_img"][i], device=gpu_device), torch.tensor(g["seq_gt"][i], device=gpu_device),
                      accumulate=acc)
        s = acc.sums.cpu()                      # a read-back per view only to check the running sums of the fixture
        print("view", i, abs(float(s[0]) - run[i, 0]) / run[i, 0], abs(float(s[1]) - run[i, 1]))
        assert abs(float(s[0]) - run[i, 0]) <= (i + 1) * REL_L1 * run[i, 0]
        assert abs(float(s[1]) - run[i, 1]) <= (i + 1) * ABS_PSNR_DB and float(s[3]) == i + 1
    res = acc.result()
    assert res["n"] == 5 and res["ssim"] is None
    assert abs(res["l1"] - g["seq_mean_f64"][0]) <= REL_L1 * g["seq_mean_f64"][0]
    assert abs(res["psnr"] - g["seq_mean_f64"][1]) <= ABS_PSNR_DB
    # an identical channel: mse = 0 -> +inf for that channel and for the view's mean, finite for the whole image
    x, gt = torch.tensor(g["same_img"], device=gpu_device), torch.tensor(g["same_gt"], device=gpu_device)
    p3 = psnr(x, gt).cpu()
    assert torch.isinf(p3[1, 0]) and p3[1, 0] > 0 and torch.isfinite(p3[[0, 2]]).all()
    assert np.array_equal(np.isinf(p3.numpy()), np.isinf(g["same_psnr3_f32"]))
    assert abs(float(psnr(x[None], gt[None])) - float(g["same_psnr1_f32"].item())) <= 1e-5 + ABS_PSNR_DB
    m = image_metrics(x, gt, accumulate=acc)
    assert math.isinf(float(m["psnr"])) and rel(float(m["l1"]), g["same_l1_f64"]) <= REL_L1
    assert math.isinf(acc.result()["psnr"])


@pytest.mark.parametrize("shape", [(1080, 1920), (131, 77), (17, 13), (1, 1)])
def test_float64_expressions_on_the_device(gpu_device, shape):
    """Against the reference's expressions in float64 on the device, clamped and not, the clamp flags one by one; SSIM on
    the shapes the window fits sensibly; two calls give the same bits."""
    from mvs_gaussian_splatting_amd import image_metrics
    x, gt = _pair(gpu_device, *shape, seed=shape[0])
    with_ssim = shape[0] >= 17
    for cx, cg in ((True, True), (False, False), (True, False), (False, True)):
        want = expected_f64(x, gt, cx, cg, with_ssim=with_ssim and cx and cg)
        got = image_metrics(x, gt, clamp=cx, clamp_gt=cg, with_ssim=with_ssim and cx and cg)
        _check(f"{shape} clamp x={cx} gt={cg}", got, want, with_ssim=with_ssim and cx and cg)
        again = image_metrics(x, gt, clamp=cx, clamp_gt=cg, with_ssim=with_ssim and cx and cg)
        assert torch.equal(got["record"], again["record"])
    if with_ssim:       # SSIM of an unclamped pair (the flags reach the tile kernel too)
        want = expected_f64(x, gt, False, False, with_ssim=True)
        _check(f"{shape} unclamped ssim", image_metrics(x, gt, clamp=False, with_ssim=True), want, with_ssim=True)
        assert float(want["ssim"]) != float(expected_f64(x, gt, True, True, with_ssim=True)["ssim"])
    _check(f"{shape} whole", image_metrics(x, gt, whole_image_psnr=True), expected_f64(x, gt), whole=True)
    # a view into a larger buffer whose planes are not 16-byte aligned: the per-pixel path, same bars
    buf = torch.zeros(x.numel() + 1, device=gpu_device)
    buf[1:] = x.reshape(-1)
    _check(f"{shape} unaligned", image_metrics(buf[1:].view_as(x), gt), expected_f64(x, gt))


def _byte_inputs(dev, H, W):
    g = torch.Generator().manual_seed(H * 7 + W)
    x = torch.rand(3 * H * W, generator=g) * 1.4 - 0.2                       # below 0 and above 1 included
    k = torch.arange(256, dtype=torch.float32) / 255.0
    one = torch.tensor(1.0)
    half = (torch.arange(256, dtype=torch.float32) + 0.5) / 255.0            # rounding boundaries of "nearest"
    special = torch.cat([k, torch.nextafter(k, 2 * one), torch.nextafter(k, -one), half, torch.nextafter(half, 2 * one),
                         torch.nextafter(half, -one), torch.tensor([-1.0, 0.0, -0.0, 1.0, 2.0, 1e-8, 255.0])])
    n = min(special.numel(), x.numel())
    if x.numel() > 8:
        idx = torch.randperm(x.numel(), generator=g)[:n]
        x[idx] = special[:n]
    return x.reshape(3, H, W).to(dev)


@pytest.mark.parametrize("shape", [(1, 1), (17, 13), (131, 77), (48, 64), (1080, 1920)])
def test_uint8_output_equals_torch(gpu_device, shape):
    from mvs_gaussian_splatting_amd import image_metrics, to_uint8_hwc
    x = _byte_inputs(gpu_device, *shape)
    gt = torch.rand_like(x)
    want = {"nearest": (x.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0),        # examples/render_ply.py
            "truncate": (torch.clamp(x, min=0, max=1.0) * 255).byte().permute(1, 2, 0)}             # train.py:63
    plain = image_metrics(x, gt)["record"]
    for rounding, w in want.items():
        out = to_uint8_hwc(x, rounding)
        assert out.shape == (*shape, 3) and out.dtype == torch.uint8 and out.is_contiguous()
        assert torch.equal(out, w), (rounding, int((out != w).sum()))
        for clamp in (True, False):                       # fused with the metrics: same bytes, same metrics
            fused = torch.full((*shape, 3), 7, dtype=torch.uint8, device=gpu_device)
            rec = image_metrics(x, gt, clamp=clamp, out_u8=fused, rounding=rounding)["record"]
            assert torch.equal(fused, w), (rounding, clamp)
            assert not clamp or torch.equal(rec, plain)
    assert shape == (1, 1) or not torch.equal(want["nearest"], want["truncate"])
    assert torch.equal(to_uint8_hwc(x[None]), want["nearest"])


def _sync_mode_works(dev):
    """Does torch.cuda.set_sync_debug_mode("error") catch a read-back on this build?"""
    t = torch.ones(1, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        t.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _problem(dev, P=3000, W=200, H=120, n_views=8):
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.synthetic import SyntheticGaussianModel, PipelineParams, orbit_camera
    kw = dict(log_scale_mean=math.log(0.06), extent=(1.6, 1.0, 0.8), centre=(0, 0, 4.0))
    truth, model = SyntheticGaussianModel(P, 3, seed=1, **kw), SyntheticGaussianModel(P, 3, seed=1, **kw)
    g = torch.Generator().manual_seed(5)
    model._features_dc = model._features_dc + 0.4 * torch.randn(model._features_dc.shape, generator=g)   # over- and undershoots
    model._xyz = model._xyz + 0.01 * torch.randn(model._xyz.shape, generator=g)
    truth.to(dev), model.to(dev)
    cams = [orbit_camera(v, n_views, W, H, 220.0, 220.0, centre=(0.0, 0.0, 4.0), device=dev) for v in range(n_views)]
    bg, pipe = torch.zeros(3, device=dev), PipelineParams()
    with torch.no_grad():
        targets = [render(c, truth, pipe, bg)["render"].clone() + 0.03 for c in cams]
    return model, cams, bg, pipe, targets


@pytest.mark.parametrize("graphed", [False, True])
def test_evaluate_views_equals_the_per_view_loop(gpu_device, graphed):
    """training_report's loop over the eight orbit views: evaluate_views against render + the reference's expressions in
    float64, with the plain render and with a GraphedRenderer; SSIM too."""
    from mvs_gaussian_splatting_amd import evaluate_views, render
    from mvs_gaussian_splatting_amd.graphed import GraphedRenderer
    model, cams, bg, pipe, targets = _problem(gpu_device)
    renderer = GraphedRenderer(model, pipe, bg) if graphed else None
    l1 = psnr = ssim = 0.0
    outside = 0
    with torch.no_grad():
        for cam, t in zip(cams, targets):
            img = (renderer.render(cam) if graphed else render(cam, model, pipe, bg))["render"].clone()
            outside += int(((img < 0) | (img > 1)).sum()) + int((t > 1).sum())
            e = expected_f64(img, t, with_ssim=True)
            l1, psnr, ssim = l1 + float(e["l1"]), psnr + float(e["psnr"]), ssim + float(e["ssim"])
    assert outside > 0                                                   # the clamps are exercised
    n = len(cams)
    got = evaluate_views(cams, model, pipe, bg, gt_images=targets, with_ssim=True, renderer=renderer)
    print("graphed" if graphed else "plain", got, l1 / n, psnr / n, ssim / n)
    assert got["n"] == n
    assert abs(got["l1"] - l1 / n) <= REL_L1 * l1 / n and abs(got["psnr"] - psnr / n) <= ABS_PSNR_DB
    assert abs(got["ssim"] - ssim / n) <= REL_SSIM * ssim / n
    for cam, t in zip(cams, targets):                                    # ground truth from the cameras, as the reference
        cam.original_image = t
    if graphed:
        again = evaluate_views(cams, model, pipe, bg, renderer=lambda c: renderer.render(c)["render"])
    else:
        again = evaluate_views(cams, model, pipe, bg)
    assert again["ssim"] is None and again["l1"] == got["l1"] and again["psnr"] == got["psnr"]


def test_metric_calls_do_not_synchronise(gpu_device):
    """A whole report's metric calls run with host synchronisation forbidden; EvalAccumulator.result() is the one
    read-back.  (If this torch build's sync debug mode does not catch a read-back, the calls still run, but the test then
    shows nothing about synchronisation: it says so.)"""
    from mvs_gaussian_splatting_amd import EvalAccumulator, image_metrics, psnr, ssim, to_uint8_hwc
    works = _sync_mode_works(gpu_device)
    print("torch.cuda.set_sync_debug_mode('error') catches read-backs on this build:", works)
    pairs = [_pair(gpu_device, 131, 77, seed=s) for s in range(4)]
    u8 = torch.empty(131, 77, 3, dtype=torch.uint8, device=gpu_device)
    acc = EvalAccumulator(gpu_device)
    image_metrics(*pairs[0], with_ssim=True)                             # library load and first launches outside
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x, gt in pairs:
            out = image_metrics(x, gt, with_ssim=True, out_u8=u8, accumulate=acc)
            assert out["l1"].dim() == 0 and out["l1"].is_cuda
        psnr(*pairs[0]), ssim(*pairs[0]), to_uint8_hwc(pairs[0][0])
        if works:
            with pytest.raises(RuntimeError):
                acc.result()                                             # the read-back is here and nowhere else
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = acc.result()
    want = [expected_f64(x, gt, with_ssim=True) for x, gt in pairs]
    assert res["n"] == 4
    assert abs(res["l1"] - sum(float(w["l1"]) for w in want) / 4) <= REL_L1 * res["l1"]
    assert abs(res["psnr"] - sum(float(w["psnr"]) for w in want) / 4) <= ABS_PSNR_DB
    assert abs(res["ssim"] - sum(float(w["ssim"]) for w in want) / 4) <= REL_SSIM * res["ssim"]


def test_examples_use_the_evaluation_path(gpu_device):
    """examples/train_synthetic.py's optional report and examples/render_ply.py's PPM bytes."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_synthetic
    import render_ply
    lines = []
    _, history, _ = train_synthetic.train(gpu_device, iterations=12, log=lines.append, report_every=6)
    reports = [l for l in lines if "Evaluating" in l]
    assert len(reports) == 2 and "L1" in reports[0] and "PSNR" in reports[0], lines
    _, plain, _ = train_synthetic.train(gpu_device, iterations=12)
    assert plain == history                                               # the report does not touch the run
    import tempfile
    x = _byte_inputs(gpu_device, 17, 13)
    with tempfile.TemporaryDirectory() as d:
        render_ply.write_ppm(os.path.join(d, "a.ppm"), x)
        data = open(os.path.join(d, "a.ppm"), "rb").read()
    want = (x.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy().tobytes()
    assert data == b"P6\n13 17\n255\n" + want
