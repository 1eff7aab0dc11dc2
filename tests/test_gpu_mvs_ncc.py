"""The multi-view photometric (NCC) loss on the HIP path (csrc/mvs_ncc.hip, ABI v36; mvs.multi_view_ncc_loss; DESIGN.md
§7.23) against the float64 restatement of tests/mvs_ncc_restate.py.

Scene: ``mvs_ncc_restate.scene`` -- a textured plane seen by a 70 x 37 reference (two x-tiles, ragged on both axes) and a
48 x 40 source with its own focal lengths; pixels whose patch leaves the reference, that fail the round trip, land past
``pix_max``, have a grazing normal, lose a tap outside the source or score ``ncc >= ncc_max``, and counted ones
(tests/test_mvs_ncc_host.py holds the census).  Bars: ``n`` exactly once the fragile pixels are set aside; the value
within max(1e-6, 2 x the float32 restatement's own error against float64) plus what the fragile pixels can move it by;
``grad_depth`` and ``grad_normal`` on robust pixels, max-norm, within max(1e-6 of the map's largest gradient, 2 x the
float32 restatement's error).  The observed figures are printed (-s).
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
import mvs_ncc_restate as N

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _scene():
    ref, depth, normal, gray, src, sdepth, sgray = N.scene()
    return ref, depth, normal, gray, src, sdepth, sgray, N.row_of(ref, src, sdepth), R.focal(ref)


@functools.lru_cache(maxsize=None)
def _reference(radius=N.RADIUS):
    """float64 and float32 restatement of the scene; computed once, never modified."""
    _, depth, normal, gray, _, _, sgray, row, (fx, fy) = _scene()
    return (N.loss(depth, normal, gray, fx, fy, row, sgray, radius=radius),
            N.loss(depth, normal, gray, fx, fy, row, sgray, radius=radius, dtype=torch.float32))


def _raw(dev, depth, normal, gray, fx, fy, row, sgray, radius=N.RADIUS, pix_max=N.PIX_MAX, ncc_max=N.NCC_MAX,
         min_cos=N.MIN_COS, pixels=None, want_d=True, want_n=True, calls=1):
    """``calls`` raw calls into outputs pre-filled with garbage -> (record, grad_depth or None, grad_normal or None)."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    H, W = depth.shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)      # noqa: E731
    d, n, g, sd, sg = up(depth), up(normal), up(gray), up(row["depth"]), up(sgray)
    assert tuple(sg.shape) == (int(row["H"]), int(row["W"]))
    t = _lib.GsrMvsSource()
    t.depth, t.width, t.height, t.fx, t.fy = sd.data_ptr(), row["W"], row["H"], float(row["fx"]), float(row["fy"])
    for i in range(16):
        t.ref_to_src[i], t.src_to_ref[i] = float(row["A"].reshape(-1)[i]), float(row["B"].reshape(-1)[i])
    table = torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).to(dev)
    px = None if pixels is None else torch.as_tensor(np.asarray(pixels, np.int32)).to(dev)
    n_px = 0 if px is None else int(px.numel())
    record = torch.full((4,), float("nan"), device=dev)
    g_d = torch.full((H, W), float("nan"), device=dev) if want_d else None
    g_n = torch.full((3, H, W), float("nan"), device=dev) if want_n else None
    ws = torch.full((lib.gsr_mvs_ncc_loss_workspace_bytes(H, W, n_px),), 0xAB, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for _ in range(calls):
            rc = lib.gsr_mvs_ncc_loss_fwd_bwd(d.data_ptr(), n.data_ptr(), g.data_ptr(), H, W, float(fx), float(fy),
                                              table.data_ptr(), sg.data_ptr(), None if px is None else px.data_ptr(), n_px,
                                              int(radius), float(pix_max), float(ncc_max), float(min_cos), record.data_ptr(),
                                              None if g_d is None else g_d.data_ptr(), None if g_n is None else g_n.data_ptr(),
                                              ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            assert rc == 0, lib.gsr_last_error()
        torch.cuda.synchronize()
    return record, g_d, g_n


def _n(record):
    return int(record.view(torch.int32)[1])


def _grad_bar(r32, r64, mask):
    scale = float(np.abs(r64).max())
    return max(1e-6, 2.0 * float(np.abs(r32.astype(np.float64) - r64)[mask].max()) / scale), scale


def _compare(dev, depth, normal, gray, fx, fy, row, sgray, r64, r32, tag, **kw):
    """The bars of the module docstring for one call; prints the observed figures."""
    record, g_d, g_n = _raw(dev, depth, normal, gray, fx, fy, row, sgray, **kw)
    rec = record.cpu().numpy()
    has = r64["kind"] >= 0
    fragile = r64["fragile"] & has
    robust = has & ~fragile
    n_robust = int((r64["counted"] & robust).sum())
    assert n_robust <= _n(record) <= n_robust + int(fragile.sum())
    err_v = abs(float(rec[0]) - r64["value"])
    bar_v = max(1e-6, 2.0 * abs(r32["value"] - r64["value"])) + N.value_slack(r64)
    assert rec[3] == 0.0 and abs(float(rec[2]) - float(rec[0]) * max(_n(record), 1)) <= 1e-6 * max(float(rec[2]), 1e-30)
    got_d, got_n = g_d.cpu().numpy().astype(np.float64), g_n.cpu().numpy().astype(np.float64)
    assert not np.isnan(got_d).any() and not np.isnan(got_n).any(), "an output element was not written"
    line = f"[mvs ncc] {tag}: n {_n(record)} (robust {n_robust}, {int(fragile.sum())} fragile); value {rec[0]:.7f} off by " \
           f"{err_v:.2e} (bar {bar_v:.2e})"
    errs = {}
    if n_robust > 0:
        rob3 = np.broadcast_to(robust, got_n.shape)
        bar_d, scale_d = _grad_bar(r32["grad_depth"], r64["grad_depth"], robust)
        bar_n, scale_n = _grad_bar(r32["grad_normal"], r64["grad_normal"], rob3)
        errs = {"grad_depth": (float(np.abs(got_d - r64["grad_depth"])[robust].max()) / scale_d, bar_d),
                "grad_normal": (float(np.abs(got_n - r64["grad_normal"])[rob3].max()) / scale_n, bar_n)}
        line += f"; grad_depth max error {errs['grad_depth'][0]:.2e} of {scale_d:.3f} (bar {bar_d:.2e}); grad_normal " \
                f"{errs['grad_normal'][0]:.2e} of {scale_n:.3f} (bar {bar_n:.2e}) on {int(robust.sum())} pixels"
    print(line)
    not_counted = robust & ~r64["counted"]
    assert not got_d[not_counted].any() and not got_n[:, not_counted].any(), "zero wherever the pixel robustly does not count"
    assert err_v <= bar_v, f"value: {err_v:.3e} > {bar_v:.3e}"
    for k, (e, bar) in errs.items():
        assert e <= bar, f"{k}: {e:.3e} > {bar:.3e}"
    return record, g_d, g_n


@pytest.mark.parametrize("radius", [1, 3, 4])
def test_value_count_and_both_gradients_match_the_float64_restatement(gpu_device, radius):
    _, depth, normal, gray, _, _, sgray, row, (fx, fy) = _scene()
    r64, r32 = _reference(radius)
    _compare(gpu_device, depth, normal, gray, fx, fy, row, sgray, r64, r32, f"patch_radius {radius}", radius=radius)
    if radius != N.RADIUS:
        return
    # n exactly once the fragile pixels are set aside (their depth removed), and the value at the bar without any slack
    fragile = r64["fragile"] & (depth > 0)
    aside = np.where(fragile, np.float32(0), depth)
    rec_a = _raw(gpu_device, aside, normal, gray, fx, fy, row, sgray, want_d=False, want_n=False)[0]
    a64 = N.loss(aside, normal, gray, fx, fy, row, sgray)
    a32 = N.loss(aside, normal, gray, fx, fy, row, sgray, dtype=torch.float32)
    assert not (a64["fragile"] & (aside > 0)).any() and _n(rec_a) == a64["n"] == int((r64["counted"] & ~fragile).sum())
    err_a, bar_a = abs(float(rec_a[0]) - a64["value"]), max(1e-6, 2.0 * abs(a32["value"] - a64["value"]))
    print(f"[mvs ncc] fragile pixels set aside: n {_n(rec_a)}, value {float(rec_a[0]):.7f} off by {err_a:.2e} (bar {bar_a:.2e})")
    assert err_a <= bar_a


def test_repeat_runs_garbage_filled_outputs_and_each_gradient_alone(gpu_device):
    _, depth, normal, gray, _, _, sgray, row, (fx, fy) = _scene()
    args = (gpu_device, depth, normal, gray, fx, fy, row, sgray)
    record, g_d, g_n = _raw(*args)
    assert not torch.isnan(record).any() and not torch.isnan(g_d).any() and not torch.isnan(g_n).any()
    assert bool(g_d.any()) and bool(g_n.any())
    rec2, d2, n2 = _raw(*args, calls=2)
    assert _same_bits(rec2, record) and _same_bits(d2, g_d) and _same_bits(n2, g_n), "the same bits from run to run"
    rec_d, only_d, none = _raw(*args, want_n=False)
    assert none is None and _same_bits(rec_d, record) and _same_bits(only_d, g_d)
    rec_n, none, only_n = _raw(*args, want_d=False)
    assert none is None and _same_bits(rec_n, record) and _same_bits(only_n, g_n)
    rec_0, _, _ = _raw(*args, want_d=False, want_n=False)
    assert _same_bits(rec_0, record)


def test_pixel_list_matches_the_dense_call_on_its_pixels_and_skips_entries_outside_the_image(gpu_device):
    _, depth, normal, gray, _, _, sgray, row, (fx, fy) = _scene()
    H, W = depth.shape
    args = (gpu_device, depth, normal, gray, fx, fy, row, sgray)
    _, dense_d, dense_n = _raw(*args)
    rng = np.random.default_rng(5)
    inner = rng.choice(np.arange(1, H * W - 1), 255, replace=False)
    pixels = np.concatenate(([0], inner, [H * W - 1])).astype(np.int32)       # 257 entries: two workgroups
    rng.shuffle(pixels)
    assert len(set(pixels.tolist())) == 257
    chosen = np.zeros(H * W, bool)
    chosen[pixels] = True
    chosen_t = torch.from_numpy(chosen.reshape(H, W)).to(gpu_device)
    r64 = N.loss(depth, normal, gray, fx, fy, row, sgray, pixels=pixels)
    r32 = N.loss(depth, normal, gray, fx, fy, row, sgray, pixels=pixels, dtype=torch.float32)
    assert r64["n"] >= 50, "the list must hold counted pixels"
    record, g_d, g_n = _compare(*args, r64, r32, "257 listed pixels", pixels=pixels)
    zero = torch.zeros((), device=gpu_device)
    assert _same_bits(g_d, torch.where(chosen_t, dense_d, zero)) and _same_bits(g_n, torch.where(chosen_t[None], dense_n, zero))
    rec2, d2, n2 = _raw(*args, pixels=pixels, calls=2)
    assert _same_bits(rec2, record) and _same_bits(d2, g_d) and _same_bits(n2, g_n)
    # entries outside [0, H W) are skipped by the kernel's bounds check: the result is that of the list without them
    hostile = np.concatenate((pixels[:100], [-1, H * W, 2 ** 31 - 1, -2 ** 31], pixels[100:])).astype(np.int32)
    rec3, d3, n3 = _raw(*args, pixels=hostile)
    assert _n(rec3) == _n(record) and _same_bits(d3, g_d) and _same_bits(n3, g_n)
    assert abs(float(rec3[2]) - float(record[2])) <= 1e-6 * float(record[2]), "the lanes moved: another summation order"


def _pair(W, H, Ws, Hs):
    """A (reference, source) pair of the scene's plane at other sizes, the depth 2 % off.  The 2 x 2 source keeps a focal
    length of 30: a 7 x 7 patch of the 70 x 37 reference spans two of its pixels, more than its one bilinear cell."""
    ref = R.Cam(np.eye(3), np.zeros(3), W, H, 1.3 * W, 1.3 * W)
    src = R.Cam(N._rotation(N.SRC_AXIS, 3.0), np.array([-0.2, 0.05, 0.0]), Ws, Hs, max(0.9 * Ws, 30.0), max(0.9 * Ws, 30.0))
    depth, gray = N.render_plane(ref, ref)
    sdepth, sgray = N.render_plane(src, ref)
    normal = np.broadcast_to((1.7 * N.PLANE_N + np.array([0.05, -0.03, 0.0]))[:, None, None], (3, H, W)).astype(np.float32)
    return ref, (depth * np.float32(1.02)).astype(np.float32), normal, gray, src, sdepth, sgray


@pytest.mark.parametrize("shape", [(1, 1, 48, 40), (7, 7, 48, 40), (65, 9, 48, 40), (70, 37, 2, 2)])
def test_edge_sizes_match_the_restatement(gpu_device, shape):
    W, H, Ws, Hs = shape
    ref, depth, normal, gray, src, sdepth, sgray = _pair(W, H, Ws, Hs)
    row, (fx, fy) = N.row_of(ref, src, sdepth), R.focal(ref)
    r64 = N.loss(depth, normal, gray, fx, fy, row, sgray)
    r32 = N.loss(depth, normal, gray, fx, fy, row, sgray, dtype=torch.float32)
    candidates = int((r64["kind"] > N.KINDS.index("patch")).sum())
    assert candidates == max(W - 6, 0) * max(H - 6, 0)
    record, g_d, g_n = _compare(gpu_device, depth, normal, gray, fx, fy, row, sgray, r64, r32, f"{W} x {H} into {Ws} x {Hs}")
    if (W, H) == (1, 1) or (Ws, Hs) == (2, 2):
        assert r64["n"] == 0 and _n(record) == 0 and not record.any() and not g_d.any() and not g_n.any(), "n = 0: loss 0, no NaN"
    if (W, H) == (7, 7):
        assert candidates == 1 and r64["n"] == 1 and _n(record) == 1, "exactly one candidate pixel at R = 3, and it counts"
        assert int((g_d != 0).sum()) == 1 and bool(g_d[3, 3] != 0)
    if (W, H) == (65, 9):
        assert r64["n"] >= 100


def test_a_source_facing_away_counts_nothing(gpu_device):
    ref, depth, normal, gray, _, _, _, _, (fx, fy) = _scene()
    away = R.look_at(np.array([0.5, 0.0, 0.0]), np.array([0.5, 0.0, -4.0]), 48, 40, 40.0, 40.0)
    row = N.row_of(ref, away, np.full((40, 48), 3.0, np.float32))
    record, g_d, g_n = _raw(gpu_device, depth, normal, gray, fx, fy, row, np.full((40, 48), 0.5, np.float32))
    assert _n(record) == 0 and not record.any() and not g_d.any() and not g_n.any(), "n = 0: loss 0, no NaN"


def test_wrapper_equals_the_raw_call_autograd_scales_and_samples_are_reproducible(gpu_device):
    from mvs_gaussian_splatting_amd import multi_view_ncc_loss
    ref, depth, normal, gray, src, sdepth, sgray, row, (fx, fy) = _scene()
    dev = gpu_device
    record, g_d, g_n = _raw(dev, depth, normal, gray, fx, fy, row, sgray)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    d, n = up(depth)[None].requires_grad_(True), up(normal).requires_grad_(True)
    g, sd, sg = up(gray), up(sdepth), up(sgray)
    loss, rec = multi_view_ncc_loss(d, n, g, ref, sd, sg[None], src, return_record=True)
    assert loss.dim() == 0 and loss.device == d.device and _same_bits(rec, record) and _same_bits(loss.detach(), record[0])
    (-2.5 * loss).backward()                                               # an upstream factor other than 1
    k = torch.tensor(-2.5, device=dev) * (1.0 / torch.tensor(float(max(_n(record), 1)), device=dev))
    assert d.grad.shape == d.shape and _same_bits(d.grad[0], g_d * k), "grad_depth * (upstream / n), one multiply"
    assert n.grad.shape == n.shape and _same_bits(n.grad, g_n * k)
    # a [3,H,W] photograph is turned to grey first; a camera carries its own
    rgb = torch.stack((g, g, g))
    ref.original_image, src.original_image = rgb, torch.stack((sg, sg, sg))
    by_cam = multi_view_ncc_loss(d.detach(), n.detach(), ref, ref, sd, src, src)
    by_rgb = multi_view_ncc_loss(d.detach(), n.detach(), rgb, ref, sd, src.original_image, src)
    assert _same_bits(by_cam, by_rgb) and not by_cam.requires_grad and ref._gray_image[0] is rgb
    assert abs(float(by_cam) - float(record[0])) <= 1e-5, "0.299 + 0.587 + 0.114 = 1 up to rounding"
    # each input's gradient is optional on its own
    d1 = up(depth).requires_grad_(True)
    multi_view_ncc_loss(d1, n.detach(), g, ref, sd, sg, src).backward()
    assert _same_bits(d1.grad, g_d * (1.0 / torch.tensor(float(_n(record)), device=dev)))
    # n_samples: the same pixels from the same seed, other pixels from another; the raw call on those pixels
    gen = lambda seed: torch.Generator(device=dev).manual_seed(seed)           # noqa: E731
    outs = []
    for seed in (7, 7, 8):
        d2 = up(depth).requires_grad_(True)
        l2, r2 = multi_view_ncc_loss(d2, n.detach(), g, ref, sd, sg, src, n_samples=700, generator=gen(seed), return_record=True)
        l2.backward()
        outs.append((r2, d2.grad))
    assert _same_bits(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1])
    assert not _same_bits(outs[0][1], outs[2][1])
    pixels = torch.randperm(depth.size, device=dev, generator=gen(7))[:700].to(torch.int32)
    rec_p, gd_p, _ = _raw(dev, depth, normal, gray, fx, fy, row, sgray, pixels=pixels.cpu().numpy())
    assert _same_bits(outs[0][0], rec_p) and 0 < _n(rec_p) < _n(record)
    assert _same_bits(outs[0][1], gd_p * (1.0 / torch.tensor(float(_n(rec_p)), device=dev)))
    by_list = multi_view_ncc_loss(up(depth), n.detach(), g, ref, sd, sg, src, pixels=pixels)
    assert _same_bits(by_list, rec_p[0])
    everything = multi_view_ncc_loss(up(depth), n.detach(), g, ref, sd, sg, src, n_samples=10 ** 6)
    assert _same_bits(everything, record[0]), "n_samples >= H W: every pixel"


# ---- the trainer ---------------------------------------------------------------------------------------------------------
PLANE = (0.3, -0.2, 4.0)         # view-space plane z = 4 + 0.3 x - 0.2 y (the scene of test_gpu_mvs_loss.py)


@pytest.fixture(scope="module")
def problem(gpu_device):
    """Two 64x48 views, 15 degrees apart, of 400 flat Gaussians on a tilted plane (the cloud of tests/test_gpu_mvs_loss.py)."""
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


def test_training_iteration_with_the_term_and_bit_identity_without_it(gpu_device, problem):
    import train as example
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    cams, bg, _ = problem
    pipe, extent = PipelineParams(), example.CAMERAS_EXTENT
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    snapshot = lambda m: [getattr(m, n).detach().clone() for n in names]      # noqa: E731
    # pix_max and ncc_max are wide open: this checks the plumbing on a cloud that was never fitted to the photographs
    new = dict(lambda_multi_view_ncc=0.15, multi_view_from_iter=0, multi_view_ncc_samples=2000, multi_view_pix_max=8.0,
               multi_view_ncc_max=2.0)
    for optimizer_type in ("default", "sparse_adam"):
        plain = _plane_model(problem, example.small_opt(40, optimizer_type=optimizer_type))
        base = training_iteration(plain, cams[0], example.small_opt(40, optimizer_type=optimizer_type), pipe, bg, 1,
                                  cameras_extent=extent)
        for extra in ({}, {"lambda_multi_view_geo": 0.05}):
            on = example.small_opt(40, optimizer_type=optimizer_type, **new, **extra)
            model = _plane_model(problem, on)
            before = snapshot(model)
            loss = training_iteration(model, cams[0], on, pipe, bg, 1, cameras_extent=extent, source_camera=cams[1])
            print(f"[mvs ncc] one iteration ({optimizer_type}) with {dict(lambda_multi_view_ncc=0.15, **extra)}: {float(loss):.6f}; "
                  f"without: {float(base):.6f}")
            assert math.isfinite(float(loss)) and float(loss) > float(base), "the term adds to the loss"
            after = snapshot(model)
            assert all(bool(torch.isfinite(a).all()) for a in after) and not torch.equal(after[0], before[0])
            assert not torch.equal(after[0], snapshot(plain)[0]), "the term moves the positions"
            assert float(model.denom.sum()) > 0, "the densification statistics were not taken"
            assert getattr(cams[0], "_gray_image", None) is not None and cams[0]._gray_image[0] is cams[0].original_image
    with pytest.raises(ValueError, match="source_camera"):
        training_iteration(_plane_model(problem, on), cams[0], on, pipe, bg, 1, cameras_extent=extent)
    # lambda = 0 whatever the other new fields say, not yet switched on, and options that do not know the fields
    zero = example.small_opt(40)
    fields = example.small_opt(40, multi_view_ncc_samples=5, multi_view_patch_radius=1, multi_view_ncc_max=0.3)
    late = example.small_opt(40, lambda_multi_view_ncc=0.15, multi_view_from_iter=7000)
    parent = types.SimpleNamespace(**{k: getattr(zero, k) for k in dir(OptimizationParams)
                                      if not k.startswith("_") and "multi_view_ncc" not in k
                                      and k != "multi_view_patch_radius"})
    assert zero.lambda_multi_view_ncc == 0.0 and not hasattr(parent, "lambda_multi_view_ncc")
    results = []
    for o, kw in ((zero, {}), (fields, {"source_camera": cams[1]}), (late, {"source_camera": cams[1]}), (parent, {})):
        m = _plane_model(problem, zero)
        out = [training_iteration(m, cams[0], o, pipe, bg, it, cameras_extent=extent, **kw) for it in (1, 2)]
        results.append((out, snapshot(m)))
    for other in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0][0], other[0])), "the loss differs"
        assert all(torch.equal(x, y) for x, y in zip(results[0][1], other[1])), "a parameter differs"
