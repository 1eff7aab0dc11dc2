"""The depth-prior loss on the GPU (csrc/depth_prior.hip behind depth_prior.depth_prior_loss) against the
float64 restatement of tests/depth_prior_restate.py (fsum sums, closed-form gradients), and the term inside
``training_iteration``.

Shapes: 1x1 and 1x2 (below one wave), 13x17 (one partial workgroup), 64x65 (one pixel past a wave multiple, 17 workgroups)
and 520x520: 270 400 pixels against the 1024 x 256 = 262 144 lanes of the capped grid, so some lanes make a second trip and
the one-workgroup kernels read four trips of partials.

Bars, with n the number of valid pixels, u = 2^-53 and c the smaller of vx / (Sxx / Sw) and vy / (Syy / Sw) of the case:
  sums      |got - fsum| <= (n + 8) u sum|term|, the bound tests/test_gpu_icp.py derives for the same reduction; count exact
  loss      |got - want| <= 4 (n + 8) u / c max(1, |want|) on the record's float64, plus half a float32 ulp on the returned
            float32 (l1 has no fit: c = 1)
  gradient  l1: the restatement's float32 bits.  Fitted modes: ulp32(want) + 64 (n + 8) u / c (|a_i| + |b_i|), a_i, b_i the
            two terms of the closed form (w_i / Sw for aligned_l1): the first-order propagation of the sums' bound through
            the fit.  aligned_l1 leaves out the pixels whose residual under the restatement's fit is within that bound of 0
            (the sign is a decision there); fewer than 0.1 % may be left out.
Every test prints the figures it asserts (run with -s)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import depth_prior_restate as R

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 2), (13, 17), (64, 65), (520, 520)]
SCALE, OFFSET = 0.4, 0.1                                             # the l1 mode's affine: the one the case was built with
U = R.U


@functools.lru_cache(maxsize=None)
def reference(H, W, mode):
    """(inputs, restated result), computed once per case and left unchanged."""
    x, y, w = R.case(H, W)
    for a in (x, y, w):
        a.setflags(write=False)
    return (x, y, w), R.evaluate(x, y, w, mode, SCALE, OFFSET)


def on_gpu(dev, *arrays):
    return [None if a is None else torch.tensor(np.asarray(a), device=dev) for a in arrays]       # a copy: the case stays as it is


def run(dev, x, y, w, mode, workspace=None, want_grad=True):
    """One evaluation through the private call -> (record float64 [8], gradient float32 [H, W] or None, workspace)."""
    from mvs_gaussian_splatting_amd import depth_prior as dp
    H, W = x.shape[-2:]
    record, grad, ws = dp._call(x, y, w, H, W, mode, SCALE, OFFSET, want_grad, workspace)
    return record, grad, ws


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sums_lie_within_the_reductions_bound_of_fsum(gpu_device, shape):
    from mvs_gaussian_splatting_amd import depth_prior as dp
    (x, y, w), res = reference(*shape, "pearson")
    _, _, ws = run(gpu_device, *on_gpu(gpu_device, x, y, w), "pearson")
    count, sums = dp._sums(ws)
    sums = sums.cpu().numpy()
    bound = R.sum_bounds(res)
    err = np.abs(sums - res.sums)
    print(f"[depth prior sums] {shape}: n = {int(count)}; error / bound per sum:",
          ", ".join(f"{k} {e:.2e}/{b:.2e}" for k, e, b in zip(R.SUM_NAMES, err, bound)))
    assert int(count) == int(res.valid.sum()) == res.terms.shape[1]
    assert (err <= bound).all()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_record_and_gradient_against_the_restatement(gpu_device, shape, mode):
    from mvs_gaussian_splatting_amd import depth_prior_loss
    (x, y, w), res = reference(*shape, mode)
    tx, ty, tw = on_gpu(gpu_device, x[None], y[None], w[None])
    tx.requires_grad_(True)
    loss, record = depth_prior_loss(tx, ty, tw, mode=mode, scale=SCALE, offset=OFFSET, return_record=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.device == tx.device
    assert record.dtype == torch.float64 and tuple(record.shape) == (8,)
    loss.backward()
    got_loss32, rec, grad = float(loss.detach()), record.cpu().numpy(), tx.grad[0].cpu().numpy()
    n = int(res.valid.sum())
    assert rec[1] == n and rec[6] == res.record[6] and rec[7] == 0.0 and not np.isnan(rec).any() and not np.isnan(grad).any()
    assert np.float32(rec[0]) == np.float32(got_loss32), "the returned loss is float32(record[0])"
    degenerate = mode != "l1" and bool(res.fit.degenerate)
    if degenerate:
        print(f"[depth prior] {shape} {mode}: degenerate, as the restatement says")
        assert rec[0] == 0.0 and rec[3:7].tolist() == [1.0, 0.0, 0.0, 1.0] and not grad.any()
        return
    c = 1.0 if mode == "l1" else res.cond
    bar = 4 * (n + 8) * U / c * max(1.0, abs(res.loss))
    err = abs(rec[0] - res.loss)
    print(f"[depth prior] {shape} {mode}: loss {rec[0]:.17g} (restated {res.loss:.17g}), error {err:.2e}, bar {bar:.2e}, c = {c:.3f}")
    assert err <= bar
    assert abs(got_loss32 - res.loss) <= bar + 0.5 * float(R.ulp32(res.loss))
    assert abs(rec[2] - res.record[2]) <= (n + 8) * U * res.record[2]
    if mode == "l1":
        assert rec[3:6].tolist() == [SCALE, OFFSET, 0.0]
        assert np.array_equal(grad.view(np.uint32), res.grad.view(np.uint32)), "l1: the gradient's float32 bits"
        return
    # the fit itself: cov and vy each carry at most 6 (n + 8) u of their leading sum, 1 / c of themselves
    rel = 16 * (n + 8) * U / c
    assert abs(rec[3] - res.fit.s) <= rel * abs(res.fit.s) and abs(rec[5] - res.fit.r) <= rel
    assert abs(rec[4] - res.fit.t) <= rel * (abs(res.fit.mx) + abs(res.fit.s * res.fit.my))
    tol = 64 * (n + 8) * U / c * (np.abs(res.a) + np.abs(res.b))
    keep = np.ones(x.shape, dtype=bool)
    if mode == "aligned_l1":
        keep = ~(res.valid & (np.abs(res.residual) <= tol))
        share = 1.0 - keep.mean()
        print(f"[depth prior] {shape} aligned_l1: {int((~keep).sum())} pixels left out ({share:.2e} of the map)")
        if n == 2:
            # a line through two points leaves no residual: both signs are decisions on rounding noise, whatever the
            # inputs.  What holds there: the loss is within its bar of 0 (asserted above) and |g_i| is w_i / Sw or 0.
            assert abs(res.loss) <= bar and not keep[res.valid].any()
            assert np.isin(np.abs(grad[res.valid]), np.append(res.a[res.valid].astype(np.float32), 0.0)).all()
        else:
            assert share < 1e-3
    gap = np.abs(grad.astype(np.float64) - res.grad64)
    bound = R.ulp32(res.grad64) + tol
    worst = float((gap[keep] / np.maximum(bound[keep], 1e-300)).max()) if keep.any() else 0.0
    print(f"[depth prior] {shape} {mode}: gradient, worst error / bar {worst:.3f}")
    assert (gap[keep] <= bound[keep]).all()
    assert not grad[~res.valid].any()


@pytest.mark.parametrize("mode", R.MODES)
def test_two_runs_and_a_dirty_workspace_give_the_same_bits(gpu_device, mode):
    (x, y, w), _ = reference(520, 520, mode)
    t = on_gpu(gpu_device, x, y, w)
    r1, g1, ws = run(gpu_device, *t, mode)
    keep_ws = ws.clone()
    r2, g2, _ = run(gpu_device, *t, mode)
    dirty = torch.full_like(ws, 0xFF)
    r3, g3, ws3 = run(gpu_device, *t, mode, workspace=dirty)
    assert ws3 is dirty
    for r, g in ((r2, g2), (r3, g3)):
        assert same_bits(r, r1) and same_bits(g, g1)
    assert float(r1[0]) > 0 and bool(g1.any())
    del keep_ws


def degenerate_inputs():
    x, y, w = (a.copy() for a in R.case(13, 17))
    return {"1x1": (x[:1, :1].copy(), y[:1, :1].copy(), np.ones((1, 1), np.float32)),
            "constant render": (np.full_like(x, 0.7), y, w),
            "zero weight": (x, y, np.zeros_like(w)),
            "nan prior": (x, np.full_like(y, np.nan), w)}


@pytest.mark.parametrize("mode", ["aligned_l1", "pearson"])
@pytest.mark.parametrize("which", ["1x1", "constant render", "zero weight", "nan prior"])
def test_degenerate_input_gives_zero_loss_zero_gradient_and_the_flag(gpu_device, which, mode):
    x, y, w = degenerate_inputs()[which]
    assert R.evaluate(x, y, w, mode).fit.degenerate == 1.0
    record, grad, _ = run(gpu_device, *on_gpu(gpu_device, x, y, w), mode)
    rec = record.cpu().numpy()
    print(f"[depth prior degenerate] {which} {mode}: record {rec.tolist()}")
    assert not np.isnan(rec).any() and not torch.isnan(grad).any()
    assert rec[0] == 0.0 and rec[3:8].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0] and not bool(grad.any())
    assert rec[1] == float(R.valid_mask(x, y, w).sum())


def test_l1_on_inputs_without_a_valid_pixel_is_zero(gpu_device):
    x, y, w = degenerate_inputs()["nan prior"]
    record, grad, _ = run(gpu_device, *on_gpu(gpu_device, x, y, w), "l1")
    assert record.cpu().tolist() == [0.0, 0.0, 0.0, SCALE, OFFSET, 0.0, 0.0, 0.0] and not bool(grad.any())


@pytest.mark.parametrize("mode", R.MODES)
def test_masked_pixels_have_no_gradient_and_move_nothing(gpu_device, mode):
    (x, y, w), res = reference(64, 65, mode)
    masked = ~res.valid
    assert (w == 0).sum() > 100 and (~np.isfinite(y)).sum() >= 2
    r1, g1, _ = run(gpu_device, *on_gpu(gpu_device, x, y, w), mode)
    assert not bool(g1[torch.from_numpy(masked).to(gpu_device)].any())
    rng = np.random.default_rng(5)
    x2, y2 = x.copy(), y.copy()
    x2[masked] = rng.standard_normal(int(masked.sum())).astype(np.float32) * 50.0
    zero_w = masked & (w == 0)
    y2[zero_w] = rng.standard_normal(int(zero_w.sum())).astype(np.float32) * 50.0
    idx = np.flatnonzero(masked.reshape(-1))
    x2.reshape(-1)[idx[0::3]] = np.nan                             # a non-finite render at a masked pixel
    x2.reshape(-1)[idx[1::3]] = -np.inf
    r2, g2, _ = run(gpu_device, *on_gpu(gpu_device, x2, y2, w), mode)
    assert same_bits(r2, r1) and same_bits(g2, g1)
    assert not torch.isnan(g2).any() and not torch.isnan(r2).any()


@pytest.mark.parametrize("mode", R.MODES)
def test_call_forms_give_the_contiguous_calls_bits(gpu_device, mode):
    from mvs_gaussian_splatting_amd import depth_prior_loss
    (x, y, w), _ = reference(64, 65, mode)
    H, W = x.shape
    tx, ty, tw = on_gpu(gpu_device, x[None], y[None], w[None])
    kw = dict(mode=mode, scale=SCALE, offset=OFFSET, return_record=True)

    def call(a, b, c):
        a = a.detach().clone().requires_grad_(True) if a.is_contiguous() else a.detach().requires_grad_(True)
        loss, record = depth_prior_loss(a, b, c, **kw)
        loss.backward()
        return loss.detach(), record, a.grad.reshape(H, W)
    base = call(tx, ty, tw)

    def strided(t):                                                # every other column of a map twice as wide
        wide = torch.zeros(1, H, 2 * W, device=t.device)
        wide[:, :, ::2] = t
        view = wide[:, :, ::2]
        assert not view.is_contiguous()
        return view
    for got in (call(strided(tx), strided(ty), strided(tw)), call(tx[0], ty[0], tw[0]), call(tx, ty[0], tw)):
        assert all(same_bits(g, b) for g, b in zip(got, base))
    # weight=None is a weight of ones
    ones = call(tx, ty, torch.ones_like(tw))
    none = call(tx, ty, None)
    assert all(same_bits(g, b) for g, b in zip(none, ones)) and not same_bits(ones[0], base[0])


@pytest.mark.parametrize("mode", R.MODES)
def test_autograd_scales_the_unit_gradient_and_skips_it_when_not_wanted(gpu_device, mode, monkeypatch):
    from mvs_gaussian_splatting_amd import depth_prior as dp
    (x, y, w), _ = reference(13, 17, mode)
    tx, ty, tw = on_gpu(gpu_device, x[None], y[None], w[None])
    _, unit, _ = run(gpu_device, tx, ty, tw, mode)
    leaf = tx.clone().requires_grad_(True)
    (2.5 * dp.depth_prior_loss(leaf, ty, tw, mode=mode, scale=SCALE, offset=OFFSET)).backward()
    assert same_bits(leaf.grad, (unit * torch.tensor(2.5, device=gpu_device)).view(1, 13, 17))
    with_grad = dp.depth_prior_loss(leaf, ty, tw, mode=mode, scale=SCALE, offset=OFFSET)
    wanted, real = [], dp._call

    def spy(*args, **kw):
        out = real(*args, **kw)
        wanted.append((args[8], out[1] is None))
        return out
    monkeypatch.setattr(dp, "_call", spy)
    without = dp.depth_prior_loss(tx, ty, tw, mode=mode, scale=SCALE, offset=OFFSET)
    assert wanted == [(False, True)], "no gradient wanted: the launch gets a NULL gradient pointer"
    assert not without.requires_grad and same_bits(without, with_grad.detach())


# ---- the trainer -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem(gpu_device):
    import train as example
    return example.make_problem(gpu_device, P=300, W=64, H=48, n_views=2)


def with_prior(cam, invdepth, reliable=True):
    cam.invdepthmap = invdepth
    cam.depth_mask = torch.ones_like(invdepth) if reliable else torch.zeros_like(invdepth)
    cam.depth_reliable = reliable
    return cam


def strip_prior(cam):
    for name in ("invdepthmap", "depth_mask", "depth_reliable"):
        if hasattr(cam, name):
            delattr(cam, name)


@pytest.mark.parametrize("mode", R.MODES)
def test_training_iteration_adds_the_weighted_term(gpu_device, problem, mode, monkeypatch):
    import train as example
    from mvs_gaussian_splatting_amd import depth_prior_loss, trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cams, bg, _ = problem
    cam, pipe, it = cams[0], PipelineParams(), 3
    opt = example.small_opt(40, depth_prior_mode=mode, depth_l1_weight_init=0.5, depth_l1_weight_final=0.05)
    weight = trainer.depth_prior_weight(opt, it)
    assert 0.05 < weight < 0.5
    strip_prior(cam)
    try:
        plain = trainer.training_iteration(example.make_model(problem, opt), cam, opt, pipe, bg, it,
                                           cameras_extent=example.CAMERAS_EXTENT)
        model = example.make_model(problem, opt)
        with torch.no_grad():
            first = trainer.render(cam, model, pipe, bg, return_depth=True)
        assert float(first["alpha"].max()) > 0.01, "the scene must cover some pixels"
        g = torch.Generator().manual_seed(3)
        prior = (2.0 * first["invdepth"] + 0.05 + 0.02 * torch.randn(first["invdepth"].shape, generator=g).to(gpu_device))
        with_prior(cam, prior.contiguous())
        term = depth_prior_loss(first["invdepth"], cam.invdepthmap, cam.depth_mask, mode=mode)
        seen, real_render = [], trainer.render

        def spy(*args, **kw):
            seen.append(dict(kw))
            return real_render(*args, **kw)
        monkeypatch.setattr(trainer, "render", spy)
        groups = {gr["name"]: gr["params"][0] for gr in model.optimizer.param_groups}
        grads = {}
        for name, p in groups.items():
            p.register_hook(lambda gr, name=name: grads.__setitem__(name, gr.detach().clone()))
        before = model._xyz.detach().clone()
        loss = trainer.training_iteration(model, cam, opt, pipe, bg, it, cameras_extent=example.CAMERAS_EXTENT)
        assert len(seen) == 1 and seen[0].get("return_depth") is True
        want = plain + torch.tensor(weight, dtype=torch.float32, device=gpu_device) * term
        gap = abs(float(loss) - float(want))
        print(f"[depth prior trainer] {mode}: loss {float(plain):.7f} without, {float(loss):.7f} with; term {float(term):.6f} "
              f"x weight {weight:.4f}; gap {gap:.2e}")
        assert float(term) > 0 and gap <= 2 * float(R.ulp32(float(want)))
        assert set(grads) == set(groups) and all(bool(torch.isfinite(gr).all()) for gr in grads.values())
        assert float(model.denom.sum()) > 0 and not torch.equal(model._xyz.detach(), before)
        # an unreliable prior switches the term off: the frame and the loss of a camera without one
        with_prior(cam, prior.contiguous(), reliable=False)
        del seen[:]
        off = trainer.training_iteration(example.make_model(problem, opt), cam, opt, pipe, bg, it,
                                         cameras_extent=example.CAMERAS_EXTENT)
        assert "return_depth" not in seen[0] and same_bits(off, plain)
    finally:
        strip_prior(cam)


def test_a_camera_without_a_prior_makes_the_calls_it_made_before(gpu_device, problem, monkeypatch):
    """The frame a camera without a prior issues: ``render`` once, with the keyword arguments the trainer passed before the
    term existed and no ``return_depth``, ``depth_prior_loss`` never, and the loss bits of the same camera carrying the
    attributes of a ``Camera`` built without a map (None, None, False)."""
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cams, bg, _ = problem
    cam, pipe = cams[1], PipelineParams()
    opt = example.small_opt(40)
    assert trainer.depth_prior_weight(opt, 1) > 0, "the defaults leave the term on for cameras that carry a prior"
    strip_prior(cam)
    seen, calls, real_render = [], [], trainer.render

    def spy(*args, **kw):
        seen.append(sorted(kw))
        return real_render(*args, **kw)
    monkeypatch.setattr(trainer, "render", spy)
    monkeypatch.setattr(trainer, "depth_prior_loss", lambda *a, **k: calls.append(1))
    try:
        bare = trainer.training_iteration(example.make_model(problem, opt), cam, opt, pipe, bg, 1,
                                          cameras_extent=example.CAMERAS_EXTENT)
        cam.invdepthmap, cam.depth_mask, cam.depth_reliable = None, None, False
        none = trainer.training_iteration(example.make_model(problem, opt), cam, opt, pipe, bg, 1,
                                          cameras_extent=example.CAMERAS_EXTENT)
    finally:
        strip_prior(cam)
    before = ["cameras_extent", "continous_dir", "densify_grad_threshold", "grow_dir", "grow_distance", "iteration", "modelcg",
              "opt"]
    assert seen == [before, before] and not calls
    assert same_bits(bare, none)
