"""MCMC densification on the GPU (csrc/mcmc.hip, mcmc.py, trainer.py): the noise step, the priors, the sampler and the
relocation against tests/mcmc_restate.py, and the strategy end to end on a small model.  Error bars are counted from the
kernels' documented float32 op order (include/gsr.h), never read off the results; each test prints its measured worst."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import mcmc_restate as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

U = 2.0 ** -24                      # float32's unit roundoff
CAP_ROWS = 2048 * 256               # rows one launch of a capped streaming kernel covers without striding
SCAN_BLOCK = 1024                   # rows per scan block of the sampler


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _inputs(P, dev, seed=0, low_opacity=True):
    """Raw tensors of a P-row model.  Opacities: a third nearly transparent (o in 0.0003..0.02: the gate is open), a
    third mid-range, a third opaque (o >= 0.9: the gate is exactly 0)."""
    g = torch.Generator().manual_seed(seed + 17 * P)
    sc = 0.6 * torch.randn(P, 3, generator=g) - 2.5
    rot = torch.randn(P, 4, generator=g)
    kind = torch.arange(P) % 3
    op = torch.where(kind == 0, -8.0 + 4.1 * torch.rand(P, generator=g),
                     torch.where(kind == 1, 2.0 * torch.randn(P, generator=g).clamp(-1.5, 1.0),
                                 2.2 + 3.0 * torch.rand(P, generator=g))).reshape(P, 1)
    if not low_opacity:
        op = 1.5 * torch.randn(P, 1, generator=g)
    xyz = 3.0 * torch.randn(P, 3, generator=g)
    xyz = torch.where(xyz.abs() < 1e-3, torch.full_like(xyz, 0.5), xyz)
    nz = torch.randn(P, 3, generator=g)
    return {k: v.contiguous().to(dev) for k, v in dict(xyz=xyz, scaling=sc, rotation=rot, opacity=op, noise=nz).items()}


def _noise(t, xyz, step):
    from mvs_gaussian_splatting_amd import _lib
    P = xyz.shape[0]
    _lib.check(_lib.load().gsr_mcmc_noise(P, xyz.data_ptr(), t["scaling"].data_ptr(), t["rotation"].data_ptr(),
                                          t["opacity"].data_ptr(), t["noise"].data_ptr(), step, _stream(xyz.device)),
               "gsr_mcmc_noise")
    return xyz


# ---- noise ---------------------------------------------------------------------------------------------------------
K_V, K_ROT = 720.0, 11.0


@pytest.mark.parametrize("P", [1, 37, 257, CAP_ROWS + 1])
def test_noise_step_against_float64(gpu_device, P):
    """|delta - delta64| <= 2^-24 (K_V mag + K_ROT mag_rot) + 2 mag_floor per component, with xyz = 0 so that the kernel's
    last add is exact and the stored value is the kernel's delta.  Counted in units of u = 2^-24 from the op order of
    include/gsr.h (expf within 1 ulp = 2u, as the device library documents; /, sqrt and + - * correctly rounded):
      o = 1/(1+expf(-raw)): 2u + u + u = 4u relative, so 4u absolute; 1-o: +u; -0.995f (the constant is 0.995 (1 +- u)):
      +u, and the rounding of the difference +u: 7u absolute at most; times -100: 700u + the product's rounding
      u |c| <= 100u... the exponent c carries <= 700u absolute (|c| < 100 wherever the gate is not 0 or 1 to within u^2).
      expf(c): 700u from its argument + 2u; 1 + e, 1 / (.): 2u  -> gate 704u.  (noise * gate) * step_scale: 2u -> v 706u.
      s^2 = expf(raw)^2: 2 * 2u + u = 5u.  u_j (3 products, 2 adds): 3u.  w_j = s^2 u_j: u.  d_i: 3u.
      Sum: 706 + 5 + 3 + 1 + 3 = 718u on `mag`; K_V = 720 leaves the second-order terms (< 718u * 718u) their room.
    The entries of R are another matter: q = raw / |raw| carries 4u per component (sum of squares 4u, sqrt halves it and
    adds u, the division u), a product of two 9u, and an entry 2 (a b +- c d) or 1 - 2 (a a + b b) therefore
    10u (|a b| + |c d|) 2 -- 10u of the SUM OF ITS TERMS' MAGNITUDES (mcmc_restate.rotation64's T), not of the entry, which
    may cancel.  R enters twice, so that error scales with mag_rot = T (s^2 |R^T||v|) + |R| (s^2 T^T |v|); K_ROT = 10 + 1 for
    second order.  (For a rotation without cancellation mag_rot is 2 mag and the whole bar is 742u mag.)
    mag_floor: where the true gate is below float32's normal range the kernel's may be 0 (o >= 0.9: expf overflows);
    2^-145: a dozen roundings to subnormal numbers (2^-150 each) on the way."""
    t = _inputs(P, gpu_device)
    step = 0.37
    got = _noise(t, torch.zeros(P, 3, device=gpu_device), step).cpu().double().numpy()
    ref = rs.noise64(*(t[k].cpu().numpy() for k in ("scaling", "rotation", "opacity", "noise")), step)
    bar = U * (K_V * ref["mag"] + K_ROT * ref["mag_rot"]) + 2.0 * ref["mag_floor"] + 2.0 ** -145
    err = np.abs(got - ref["delta"])
    moved = ref["mag"] > 1e-30
    worst = float((err / bar).max())
    plain = float((err[moved] / (U * ref["mag"][moved])).max()) if moved.any() else 0.0
    print(f"[mcmc noise] P={P}: worst error / bar {worst:.3f}; worst error in units of 2^-24 mag {plain:.1f} "
          f"(bar without cancellation {K_V + 2 * K_ROT:.0f}); rows that move {int(moved.any(axis=1).sum())}")
    assert np.isfinite(got).all()
    assert P < 3 or moved.any(), "the inputs must open the gate somewhere"
    assert (err <= bar).all(), worst
    # the issue's form, K * 2^-24 * magnitude with the one magnitude |R| (s^2 |R^T| |v|): K = K_V + 2 K_ROT = 742, the
    # bar above for a rotation none of whose entries cancels
    assert plain <= K_V + 2 * K_ROT, plain


def test_noise_step_exact_properties(gpu_device):
    P = 257
    t = _inputs(P, gpu_device, seed=3)
    step = 0.37
    o = torch.sigmoid(t["opacity"].double()).reshape(-1).cpu()
    opaque = o >= 0.9
    assert 50 < int(opaque.sum()) < P - 50
    delta = _noise(t, torch.zeros(P, 3, device=gpu_device), step)
    # the stored value is float32(xyz + delta): one rounding of the exact sum
    out = _noise(t, t["xyz"].clone(), step)
    assert torch.equal(out, t["xyz"] + delta)
    # a second call with the same inputs gives the same bits
    assert torch.equal(_noise(t, t["xyz"].clone(), step).view(torch.int32), out.view(torch.int32))
    # rows with o >= 0.9 keep their bits (gate == 0 exactly), and some other row moves
    same = (out.view(torch.int32) == t["xyz"].view(torch.int32)).all(dim=1).cpu()
    assert same[opaque].all() and not same[~opaque].all()
    assert torch.equal(delta[opaque.to(gpu_device)], torch.zeros_like(delta[opaque.to(gpu_device)]))
    # rows whose noise is 0 keep their bits; their neighbours move as before
    moving = (~same).nonzero().reshape(-1)
    row = int(moving[len(moving) // 2])
    t0 = dict(t, noise=t["noise"].clone())
    t0["noise"][row] = 0.0
    out0 = _noise(t0, t["xyz"].clone(), step)
    assert torch.equal(out0[row].view(torch.int32), t["xyz"][row].view(torch.int32))
    keep = torch.ones(P, dtype=torch.bool, device=gpu_device)
    keep[row] = False
    assert torch.equal(out0[keep].view(torch.int32), out[keep].view(torch.int32))
    # only one row has noise: it moves, its neighbours are untouched
    t1 = dict(t, noise=torch.zeros_like(t["noise"]))
    t1["noise"][row] = t["noise"][row]
    out1 = _noise(t1, t["xyz"].clone(), step)
    assert torch.equal(out1[row], out[row]) and not torch.equal(out1[row], t["xyz"][row])
    assert torch.equal(out1[keep].view(torch.int32), t["xyz"][keep].view(torch.int32))
    # step_scale = 0 leaves every value equal
    assert torch.equal(_noise(t, t["xyz"].clone(), 0.0), t["xyz"])
    # P = 0: nothing to do
    from mvs_gaussian_splatting_amd import _lib
    assert _lib.load().gsr_mcmc_noise(0, None, None, None, None, None, 1.0, _stream(gpu_device)) == 0


# ---- priors --------------------------------------------------------------------------------------------------------
def _reg(t, wo, ws, g=None):
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    dev = t["opacity"].device
    P = t["opacity"].shape[0]
    record = torch.full((4,), float("nan"), device=dev)
    ws_buf = torch.empty(lib.gsr_mcmc_reg_workspace_bytes(), dtype=torch.uint8, device=dev)
    _lib.check(lib.gsr_mcmc_reg_fwd(t["opacity"].data_ptr(), t["scaling"].data_ptr(), P, wo, ws, record.data_ptr(),
                                    ws_buf.data_ptr(), ws_buf.numel(), _stream(dev)), "gsr_mcmc_reg_fwd")
    if g is None:
        return record
    go, gs = torch.empty_like(t["opacity"]), torch.empty_like(t["scaling"])
    gt = torch.tensor(g, dtype=torch.float32, device=dev)
    _lib.check(lib.gsr_mcmc_reg_bwd(t["opacity"].data_ptr(), t["scaling"].data_ptr(), P, record.data_ptr(), gt.data_ptr(),
                                    go.data_ptr(), gs.data_ptr(), _stream(dev)), "gsr_mcmc_reg_bwd")
    return record, go, gs


def _reg_bars(ref_go, ref_gs, o):
    """Opacity gradient (g f) (o (1 - o)): f = float(opacity_reg / P) u, g f u, o 4u, 1 - o: 4u o / (1 - o) + u relative,
    the two products 2u: (9 + 4 o / (1 - o)) u.  Scale gradient (g f) s: u + u + 2u (expf) + u = 5u."""
    return U * (9.0 + 4.0 * o / (1.0 - o)) * np.abs(ref_go), U * 5.0 * np.abs(ref_gs)


@pytest.mark.parametrize("P", [1, 37, 257, CAP_ROWS + 1])
def test_priors_against_float64(gpu_device, P):
    """Value within 2 * 2^-24 relative of float64 (the accumulation is in double: what is left is the float32 rounding of
    each activation, which averages, and the one at the end); gradients within the bars of _reg_bars."""
    t = _inputs(P, gpu_device, seed=5, low_opacity=False)
    wo, ws, g = 0.01, 0.02, 0.75
    record, go, gs = _reg(t, wo, ws, g)
    value, ref_go, ref_gs, o = rs.reg64(t["opacity"].cpu().numpy(), t["scaling"].cpu().numpy(), wo, ws, g)
    rec = record.cpu().double().numpy()
    rel = abs(rec[0] - value) / value
    bar_o, bar_s = _reg_bars(ref_go, ref_gs, o)
    eo, es = np.abs(go.cpu().double().numpy() - ref_go), np.abs(gs.cpu().double().numpy() - ref_gs)
    print(f"[mcmc priors] P={P}: value off by {rel / U:.2f} x 2^-24 (bar 2); gradients at {float((eo / bar_o).max()):.2f} "
          f"(opacity) and {float((es / bar_s).max()):.2f} (scale) of their bars")
    assert rel <= 2.0 * U
    assert rec[1] == float(np.float32(float(np.float32(wo)) / P)) and rec[2] == float(np.float32(float(np.float32(ws)) / (3 * P)))
    assert rec[3] == 0.0
    assert (eo <= bar_o).all() and (es <= bar_s).all()
    # the same bits on a second run
    record2, go2, gs2 = _reg(t, wo, ws, g)
    assert torch.equal(record2.view(torch.int32), record.view(torch.int32))
    assert torch.equal(go2, go) and torch.equal(gs2, gs)
    # each weight at 0 zeroes its term exactly
    only_s, only_o = _reg(t, 0.0, ws).cpu().double().numpy(), _reg(t, wo, 0.0).cpu().double().numpy()
    s64 = float(np.float32(ws)) * math.fsum(np.exp(t["scaling"].cpu().double().numpy()).ravel()) / (3 * P)
    o64 = float(np.float32(wo)) * math.fsum(o.ravel()) / P
    assert only_s[1] == 0.0 and only_o[2] == 0.0
    assert abs(only_s[0] - s64) <= 2.0 * U * s64 and abs(only_o[0] - o64) <= 2.0 * U * o64
    _, go0, _ = _reg(t, 0.0, ws, g)
    _, _, gs0 = _reg(t, wo, 0.0, g)
    assert not go0.any() and not gs0.any()


def test_mcmc_regularizer_autograd(gpu_device):
    from mvs_gaussian_splatting_amd import mcmc_regularizer
    P = 257
    t = _inputs(P, gpu_device, seed=6, low_opacity=False)
    op, sc = t["opacity"].clone().requires_grad_(True), t["scaling"].clone().requires_grad_(True)
    wo, ws, g = 0.01, 0.02, 0.75
    loss = mcmc_regularizer(op, sc, wo, ws)
    assert loss.shape == () and loss.is_cuda and loss.requires_grad
    assert torch.equal(loss.detach(), _reg(t, wo, ws)[0]), "the autograd function returns the kernel's record"
    (loss * g).backward()
    # the torch composition, in float64
    op64, sc64 = t["opacity"].double().requires_grad_(True), t["scaling"].double().requires_grad_(True)
    ref = float(np.float32(wo)) * torch.sigmoid(op64).mean() + float(np.float32(ws)) * torch.exp(sc64).mean()
    (ref * g).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 2.0 * U * float(ref.detach())
    o = torch.sigmoid(op64.detach()).cpu().numpy()
    bar_o, bar_s = _reg_bars(op64.grad.cpu().numpy(), sc64.grad.cpu().numpy(), o)
    assert op.grad.shape == (P, 1) and sc.grad.shape == (P, 3)
    assert (np.abs(op.grad.cpu().double().numpy() - op64.grad.cpu().numpy()) <= bar_o).all()
    assert (np.abs(sc.grad.cpu().double().numpy() - sc64.grad.cpu().numpy()) <= bar_s).all()
    # an empty model: a constant zero
    z = mcmc_regularizer(torch.zeros(0, 1, device=gpu_device), torch.zeros(0, 3, device=gpu_device), wo, ws)
    assert float(z) == 0.0


# ---- sampler -------------------------------------------------------------------------------------------------------
def _sample_case(dev, raw, thr, draws):
    """Runs the kernel and the restatement on the float32 activations the device forms; asserts they agree exactly."""
    from mvs_gaussian_splatting_amd.mcmc import sample_alive
    raw = raw.reshape(-1, 1).contiguous().to(dev)
    d = torch.tensor(draws, dtype=torch.int64)
    idx, count = sample_alive(raw, len(draws), thr, d.to(dev))
    o32 = torch.sigmoid(raw).cpu().numpy().ravel()           # 1 / (1 + exp(-x)) in float32 on the device
    w = rs.weights(o32, thr)
    want_idx, want_count, _ = rs.sample(w, draws)
    idx, count = idx.cpu().tolist(), count.cpu().tolist()
    assert idx == want_idx, "sampled rows differ from the integer restatement"
    assert count == want_count
    assert sum(count) == (len(draws) if sum(w) > 0 else 0)
    assert all(i == -1 or w[i] > 0 for i in idx), "a row of weight 0 was returned"
    return w, idx


def _draws(n, seed):
    g = np.random.default_rng(seed)
    return [int(x) for x in g.integers(0, 2 ** 63, size=n, dtype=np.int64)]


@pytest.mark.parametrize("P", [1, 37, 257, 2 * SCAN_BLOCK + 300])
def test_sampler_random_opacities(gpu_device, P):
    g = torch.Generator().manual_seed(P)
    raw = 3.0 * torch.randn(P, generator=g) - 3.0            # about a third of the rows are below 0.005
    raw[0] = 1.0                                             # at least one row is alive
    w, idx = _sample_case(gpu_device, raw, 0.005, _draws(500, P))
    assert P < 30 or 0 in w
    w_all, _ = _sample_case(gpu_device, raw, -1.0, _draws(500, P + 1) + rs.edge_draws(w))
    assert all(x > 0 for x in w_all)


def test_sampler_dead_runs_on_block_boundaries_and_edge_draws(gpu_device):
    P = 3 * SCAN_BLOCK + 37
    g = torch.Generator().manual_seed(11)
    raw = torch.randn(P, generator=g)
    dead = torch.zeros(P, dtype=torch.bool)
    dead[0:256] = True                                       # from the first row to a thread-block boundary
    dead[SCAN_BLOCK - 4:SCAN_BLOCK] = True                   # ends on a scan-block boundary
    dead[SCAN_BLOCK:SCAN_BLOCK + 64] = True                  # ... and starts on one
    dead[2 * SCAN_BLOCK:3 * SCAN_BLOCK] = True               # a whole scan block
    dead[P - 5:] = True                                      # the ragged tail
    dead[1500], dead[1502] = True, True                      # single dead rows around a live one
    raw[dead] = -9.0
    w = rs.weights(torch.sigmoid(raw.to(gpu_device)).cpu().numpy(), 0.005)
    assert [w[i] == 0 for i in range(P)] == dead.tolist()
    edges = rs.edge_draws(w)
    assert len(edges) > 20
    _sample_case(gpu_device, raw, 0.005, edges + _draws(300, 3) + [0, 2 ** 63 - 1])


def test_sampler_degenerate_cases(gpu_device):
    from mvs_gaussian_splatting_amd.mcmc import sample_alive
    P = SCAN_BLOCK + 257
    # all rows dead but one
    raw = torch.full((P,), -9.0)
    raw[SCAN_BLOCK + 3] = 0.5
    w, idx = _sample_case(gpu_device, raw, 0.005, _draws(64, 1) + [0, 2 ** 63 - 1])
    assert set(idx) == {SCAN_BLOCK + 3}
    # all rows dead: T == 0
    w, idx = _sample_case(gpu_device, torch.full((P,), -9.0), 0.005, _draws(64, 2))
    assert set(idx) == {-1} and sum(w) == 0
    # n == 0: the counts are still zero-filled
    idx0, count0 = sample_alive(raw.reshape(-1, 1).to(gpu_device), 0, 0.005, torch.zeros(0, dtype=torch.int64))
    assert idx0.numel() == 0 and count0.shape == (P,) and not count0.any()


def test_sampler_past_the_grid_cap(gpu_device):
    """More rows than the capped zero-fill covers in one stride and more draws than the sampling kernel does."""
    P = CAP_ROWS + 37
    g = torch.Generator().manual_seed(13)
    raw = 2.0 * torch.randn(P, generator=g) - 2.0
    _sample_case(gpu_device, raw, 0.005, _draws(CAP_ROWS + 1, 4))


# ---- relocation ----------------------------------------------------------------------------------------------------
def test_relocation_against_float64(gpu_device):
    """new_opacity_raw / new_scaling_raw within 2 ulp of the float32 rounding of the restatement.  The device's double
    log and pow are not correctly rounded (a few ulp of double, 1e-16 relative): against float32's 6e-8 that moves a
    result only when the double value sits within 1e-8 ulp of a rounding boundary, so the measured worst is 0 or 1 ulp;
    the bar of 2 leaves room for the series' cancellation at N = 51 ((1 + o')^51 / D, below 1e3 x 1e-16)."""
    from mvs_gaussian_splatting_amd.mcmc import relocation
    opac = [0.0051, 0.006, 0.5, 0.99]
    counts = [0, 1, 2, 50, 51, 200]                                     # N = 1, 2, 3, 51, 51 (clamped), 51 (clamped)
    raw_o = torch.tensor([math.log(o / (1 - o)) for o in opac], dtype=torch.float32).reshape(-1, 1)
    g = torch.Generator().manual_seed(21)
    raw_s = (0.8 * torch.randn(len(opac), 3, generator=g) - 2.0).contiguous()
    for cnt in counts:
        idx = torch.tensor([0, 1, 2, 3, 2, 0], dtype=torch.int32)       # rows 2 and 0 twice
        count = torch.full((len(opac),), cnt, dtype=torch.int32)
        new_o, new_s = relocation(idx.to(gpu_device), count.to(gpu_device), raw_o.to(gpu_device), raw_s.to(gpu_device))
        torch.cuda.synchronize()
        o32 = torch.sigmoid(raw_o.to(gpu_device)).cpu().numpy().ravel()
        s32 = torch.exp(raw_s.to(gpu_device)).cpu().numpy()
        worst = 0.0
        for j, i in enumerate(idx.tolist()):
            _, _, _, ref_o, ref_s = rs.relocation64(float(o32[i]), s32[i].astype(np.float64), cnt + 1)
            for got, ref in [(float(new_o[j, 0]), ref_o)] + list(zip(new_s[j].cpu().tolist(), ref_s.tolist())):
                r32 = np.float32(ref)
                ulps = abs(got - float(r32)) / float(np.spacing(np.abs(r32)))
                worst = max(worst, ulps)
        print(f"[mcmc relocation] count {cnt} (N = {min(cnt + 1, 51)}): worst {worst:.1f} ulp of float32")
        assert worst <= 2.0
        # two samples of the same source get identical outputs
        assert torch.equal(new_o[2], new_o[4]) and torch.equal(new_s[2], new_s[4])
        assert torch.equal(new_o[0], new_o[5]) and torch.equal(new_s[0], new_s[5])
        if cnt == 0:      # N = 1: the scales make the round trip log(exp(raw)) and the opacity logit(sigmoid(raw))
            assert (new_s.cpu() - raw_s[idx.long()]).abs().max() <= 4e-7 * raw_s.abs().max()
        if cnt >= 50:     # clamped: counts of 50, 51 and 200 agree
            ref = relocation(idx.to(gpu_device), torch.full((len(opac),), 50, dtype=torch.int32, device=gpu_device),
                             raw_o.to(gpu_device), raw_s.to(gpu_device))
            assert torch.equal(ref[0], new_o) and torch.equal(ref[1], new_s)
    # idx = -1 (the sampler found no weight): zeros
    z_o, z_s = relocation(torch.tensor([-1], dtype=torch.int32, device=gpu_device), count.to(gpu_device),
                          raw_o.to(gpu_device), raw_s.to(gpu_device))
    assert not z_o.any() and not z_s.any()


# ---- the strategy end to end -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem(gpu_device):
    import train as example
    return example.make_problem(gpu_device, P=600, W=64, H=48, n_views=1)


def _model(problem, optimizer_type="default", iterations=2, **over):
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    opt = example.small_opt(40, optimizer_type=optimizer_type, **over)
    model = example.make_model(problem, opt)
    cams, bg, _ = problem
    for it in range(1, iterations + 1):                      # moments that are not zero
        trainer.training_iteration(model, cams[0], opt, PipelineParams(), bg, it, cameras_extent=example.CAMERAS_EXTENT)
    return model, opt


def _snapshot(model):
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    snap = {a: getattr(model, a).detach().clone() for a in GROUP_ATTR.values()}
    for group in model.optimizer.param_groups:
        state = model.optimizer.state[group["params"][0]]
        snap["m:" + group["name"]], snap["v:" + group["name"]] = state["exp_avg"].clone(), state["exp_avg_sq"].clone()
    return snap


def test_relocate_gs(gpu_device, problem):
    from mvs_gaussian_splatting_amd import relocate_gs
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    from mvs_gaussian_splatting_amd.mcmc import relocation, sample_alive
    model, _ = _model(problem)
    P = model._xyz.shape[0]
    assert P == 300
    params = {a: getattr(model, a) for a in GROUP_ATTR.values()}
    keys = list(model.optimizer.state.keys())
    # a model with no dead row is untouched bit for bit
    assert float(torch.sigmoid(model._opacity.detach()).min()) > 0.005
    before = _snapshot(model)
    assert relocate_gs(model, draws=torch.tensor(_draws(8, 0))) == 0
    assert all(torch.equal(v, w) for v, w in zip(before.values(), _snapshot(model).values()))
    # 40 dead rows
    dead = torch.arange(3, P, 7, device=gpu_device)[:40]
    with torch.no_grad():
        model._opacity[dead] = -7.0
    before = _snapshot(model)
    draws = torch.tensor(_draws(64, 9))
    idx, count = sample_alive(before["_opacity"], 40, 0.005, draws)
    new_o, new_s = relocation(idx, count, before["_opacity"], before["_scaling"])
    src = idx.long()
    assert not torch.isin(src, dead).any() and int(count.sum()) == 40
    assert relocate_gs(model, draws=draws) == 40
    after = _snapshot(model)
    assert model._xyz.shape[0] == P
    assert all(getattr(model, a) is params[a] for a in params), "an nn.Parameter was replaced"
    assert list(model.optimizer.state.keys()) == keys
    for a in ("_xyz", "_features_dc", "_features_rest", "_rotation"):
        assert torch.equal(after[a][dead], before[a][src]), a                 # dead rows are copies of their sources
        assert torch.equal(after[a][src], before[a][src]), a
    for a, new in (("_opacity", new_o), ("_scaling", new_s)):
        assert torch.equal(after[a][dead], new) and torch.equal(after[a][src], new), a
    touched = torch.zeros(P, dtype=torch.bool, device=gpu_device)
    touched[dead] = True
    touched[src] = True
    is_src = torch.zeros(P, dtype=torch.bool, device=gpu_device)
    is_src[src] = True
    for a in params:
        assert torch.equal(after[a][~touched], before[a][~touched]), a
    for group in model.optimizer.param_groups:
        for k in ("m:", "v:"):
            m0, m1 = before[k + group["name"]], after[k + group["name"]]
            assert not m1[is_src].any(), "a source keeps a moment"
            assert torch.equal(m1[~is_src], m0[~is_src]), "a moment changed away from the sources"
            if group["name"] in ("xyz", "opacity"):
                assert m0[dead].any(), "the dead rows' moments must be non-zero for the check to mean something"
    # the corrected opacity is below the source's, the model trains on
    assert (torch.sigmoid(new_o) <= torch.sigmoid(before["_opacity"][src]) + 1e-7).all()


def test_add_new_gs(gpu_device, problem):
    from mvs_gaussian_splatting_amd import add_new_gs
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    from mvs_gaussian_splatting_amd.mcmc import relocation, sample_alive
    model, _ = _model(problem)
    P = model._xyz.shape[0]
    before = _snapshot(model)
    draws = torch.tensor(_draws(64, 5))
    n = int(1.05 * P) - P
    idx, count = sample_alive(before["_opacity"], n, -1.0, draws)
    new_o, new_s = relocation(idx, count, before["_opacity"], before["_scaling"])
    src = idx.long()
    assert add_new_gs(model, 10_000, draws=draws) == n == 15
    after = _snapshot(model)
    assert all(getattr(model, a).shape[0] == P + n for a in GROUP_ATTR.values())
    assert model.xyz_gradient_accum.shape == (P + n, 1) and model.denom.shape == (P + n, 1)
    assert model.max_radii2D.shape == (P + n,)
    assert not model.xyz_gradient_accum[P:].any() and not model.denom[P:].any() and not model.max_radii2D[P:].any()
    for a in ("_xyz", "_features_dc", "_features_rest", "_rotation"):
        assert torch.equal(after[a][:P], before[a]) and torch.equal(after[a][P:], before[a][src]), a
    for a, new in (("_opacity", new_o), ("_scaling", new_s)):
        assert torch.equal(after[a][P:], new) and torch.equal(after[a][src], new), a
    is_src = torch.zeros(P + n, dtype=torch.bool, device=gpu_device)
    is_src[src] = True
    is_src[P:] = True
    for group in model.optimizer.param_groups:
        assert group["params"][0] is getattr(model, GROUP_ATTR[group["name"]])
        for k in ("m:", "v:"):
            m0, m1 = before[k + group["name"]], after[k + group["name"]]
            assert m1.shape[0] == P + n and not m1[is_src].any()
            assert torch.equal(m1[:P][~is_src[:P]], m0[~is_src[:P]])
    # the cap: P follows min(cap_max, int(1.05 P)); at the cap nothing changes
    P1 = P + n
    assert add_new_gs(model, P1 + 4, draws=draws) == 4 and model._xyz.shape[0] == P1 + 4
    snap = _snapshot(model)
    params = {a: getattr(model, a) for a in GROUP_ATTR.values()}
    assert add_new_gs(model, P1 + 4, draws=draws) == 0 and add_new_gs(model, 10, draws=draws) == 0
    assert all(getattr(model, a) is params[a] for a in params)
    assert all(torch.equal(v, w) for v, w in zip(snap.values(), _snapshot(model).values()))


def test_relocation_keeps_the_picture_better_than_a_plain_copy(gpu_device):
    """One Gaussian relocated onto an isolated source (N = 2): the picture of the corrected pair is closer to the
    original's than the picture of an uncorrected copy is.  The HIP renders are also held to the float64 oracle render
    of the same parameters (the bar of smoke(): 1e-5 on robust pixels)."""
    from conftest import make_settings
    from oracle import rasterize_ref
    from grad_util import oracle_operator_inputs
    from mvs_gaussian_splatting_amd import relocate_gs, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams, SceneConfig, make_scene
    cfg = SceneConfig("reloc", 2, 0, 64, 48, 60.0, 60.0, math.log(0.25))
    model, cam, bg, _ = make_scene(cfg, seed=0)
    model._xyz = torch.tensor([[0.1, -0.05, 6.0], [4.0, 3.0, 9.0]])
    model._opacity = torch.tensor([[0.8], [-9.0]])                      # the source (o = 0.69) and a dead Gaussian
    model._features_dc = torch.tensor([[[1.2, 0.4, -0.3]], [[0.0, 0.0, 0.0]]])
    st = make_settings(cam, bg, 0)

    def oracle(m):
        _, xyz, m2, op, kw = oracle_operator_inputs(m, torch.float64)
        col, _, aux = rasterize_ref(xyz, m2, op, st, want_aux=True, want_margin=True, **kw)
        return col.detach(), aux["margin"] > 1e-4

    def hip(m):
        with torch.no_grad():
            return render(cam, m, PipelineParams(), bg.to(gpu_device))["render"].cpu().double()

    ref0, _ = oracle(model)
    model.to(gpu_device)
    cam.to(gpu_device)
    img0 = hip(model)
    assert float(img0.max()) > 0.2, "the source must be visible"
    original = {a: getattr(model, a).clone() for a in model._PARAMS}
    assert relocate_gs(model, draws=torch.tensor(_draws(4, 0))) == 1
    assert torch.equal(model._xyz[1], model._xyz[0]) and torch.equal(model._opacity[1], model._opacity[0])
    assert float(model._opacity[0]) < 0.8 and (model._scaling[0] != original["_scaling"][0]).all()
    img1 = hip(model)
    model.to("cpu")
    ref1, robust = oracle(model)
    err = ((img1 - ref1).abs() / ref1.abs().clamp(min=1.0)).max(dim=0).values
    assert float(err[robust].max()) <= 1e-5 and int((~robust).sum()) <= 0.02 * robust.numel()
    model.to(gpu_device)
    for a in model._PARAMS:                                             # the copy without the correction
        t = original[a].clone()
        t[1] = t[0]
        setattr(model, a, t)
    img2 = hip(model)
    corrected, copied = float((img1 - img0).abs().max()), float((img2 - img0).abs().max())
    print(f"[mcmc relocation] largest pixel change: corrected pair {corrected:.4f}, uncorrected copy {copied:.4f}; "
          f"oracle agrees on the original to {float((img0 - ref0).abs().max()):.1e}")
    assert corrected < copied


def _state(model):
    """Every parameter and both Adam moments of every group, cloned."""
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    out = {a: getattr(model, a).detach().clone() for a in GROUP_ATTR.values()}
    for group in model.optimizer.param_groups:
        st = model.optimizer.state.get(group["params"][0], {})
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                out[key + ":" + group["name"]] = st[key].clone()
    return out


def _run_five(problem, optimizer_type, strategy_kw, mcmc_kwargs=None):
    """-> (losses, row counts, state after the densify iteration, state at the end)."""
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    opt = example.small_opt(40, optimizer_type=optimizer_type, densify_from_iter=2, densification_interval=3, **strategy_kw)
    model = example.make_model(problem, opt)                 # seeds torch's generators: the split's draws repeat
    cams, bg, _ = problem
    losses, rows, mid = [], [], None
    for it in range(1, 6):                                   # iteration 3 densifies
        kw = {} if mcmc_kwargs is None else {"mcmc_kwargs": mcmc_kwargs}
        if it == 3 and strategy_kw.get("strategy") == "mcmc":
            with torch.no_grad():
                model._opacity[5:40:5] = -7.0                # something to relocate
        losses.append(float(trainer.training_iteration(model, cams[0], opt, PipelineParams(), bg, it,
                                                       cameras_extent=example.CAMERAS_EXTENT, **kw)))
        rows.append(int(model._xyz.shape[0]))
        if it == 3:
            mid = _state(model)
    return losses, rows, mid, _state(model)


def _assert_same_bits(s1, s2, what):
    assert list(s1) == list(s2), what
    for k in s1:
        assert s1[k].shape == s2[k].shape, (what, k)
        assert torch.equal(s1[k].view(torch.int32), s2[k].view(torch.int32)), \
            f"{what}: {k} differs in {int((s1[k] != s2[k]).sum())} values, by up to {float((s1[k] - s2[k]).abs().max()):.2e}"


@pytest.mark.parametrize("optimizer_type", ["default", "sparse_adam"])
def test_five_mcmc_iterations_are_reproducible(gpu_device, problem, optimizer_type):
    """Two identical runs across a densify iteration (7 rows relocated, 10 added) with fixed draws and noise: every
    parameter, both Adam moments of every group and every loss are the same bits, right after the densify iteration
    (so the same rows were relocated and grown) and at the end.  Nothing on this path adds in an order that can change:
    the colour path's backward sums each Gaussian's rows in slot order, Adam, the priors, the sampler, the
    relocation and the noise step are deterministic."""
    mk = {"draws": torch.tensor(_draws(64, 77)), "noise": torch.randn(400, 3, generator=torch.Generator().manual_seed(5))}
    kw = dict(strategy="mcmc", cap_max=310)
    l1, r1, mid1, end1 = _run_five(problem, optimizer_type, kw, mk)
    l2, r2, mid2, end2 = _run_five(problem, optimizer_type, kw, mk)
    assert all(math.isfinite(x) for x in l1) and all(torch.isfinite(t).all() for t in end1.values())
    assert r1 == r2 == [300, 300, 310, 310, 310], r1         # min(cap_max, int(1.05 * 300) = 315)
    assert l1 == l2, (l1, l2)
    _assert_same_bits(mid1, mid2, f"{optimizer_type}, after the densify iteration")
    _assert_same_bits(end1, end2, f"{optimizer_type}, after five iterations")
    # the dead rows were relocated: they sit on other rows' positions now
    assert float(torch.sigmoid(mid1["_opacity"]).min()) > 0.004


def test_default_strategy_is_untouched_by_the_new_keywords(gpu_device, problem):
    """Five iterations across a densification with strategy="default" spelled out, and with an ``opt`` that has none of the
    new fields and no new keyword, as a caller from before they existed: the same bits in every parameter, every Adam
    moment and every loss.  (The default path is reproducible from run to run: DESIGN.md §4.)"""
    import types
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    new = ("strategy", "cap_max", "noise_lr", "opacity_reg", "scale_reg")
    import train as example
    real_small_opt = example.small_opt

    def old_opt(*args, **kw):
        base = real_small_opt(*args, **kw)
        fields = {k: getattr(base, k) for k in dir(OptimizationParams) if not k.startswith("_") and k not in new}
        assert not any(hasattr(types.SimpleNamespace(**fields), k) for k in new)
        return types.SimpleNamespace(**fields)

    la, ra, mida, enda = _run_five(problem, "default", dict(strategy="default"))
    example.small_opt = old_opt
    try:
        lb, rb, midb, endb = _run_five(problem, "default", {})
    finally:
        example.small_opt = real_small_opt
    assert ra == rb and ra[2] != ra[1], "iteration 3 must densify, to the same row count"
    assert la == lb, (la, lb)
    _assert_same_bits(mida, midb, "default strategy, after the densify iteration")
    _assert_same_bits(enda, endb, "default strategy, after five iterations")


def test_no_frame_is_reissued_once_the_cap_is_reached(gpu_device, problem):
    """At the cap a relocation moves rows in place: P, and with it the rasterizer's capacity state, stays."""
    import train as example
    from mvs_gaussian_splatting_amd import rasterizer as rz, trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    opt = example.small_opt(40, strategy="mcmc", cap_max=300, densify_from_iter=2, densification_interval=3)
    model = example.make_model(problem, opt)
    cams, bg, _ = problem
    W, H = cams[0].image_width, cams[0].image_height
    mk = {"draws": torch.tensor(_draws(64, 3))}
    for it in (1, 2):
        trainer.training_iteration(model, cams[0], opt, PipelineParams(), bg, it, cameras_extent=example.CAMERAS_EXTENT,
                                   mcmc_kwargs=mk)
    before = rz.reissued_frames(gpu_device, 300, W, H)
    with torch.no_grad():
        model._opacity[5:40:5] = -7.0
    params = model._xyz
    for it in (3, 4, 5):                                     # iteration 3 relocates
        trainer.training_iteration(model, cams[0], opt, PipelineParams(), bg, it, cameras_extent=example.CAMERAS_EXTENT,
                                   mcmc_kwargs=mk)
    assert model._xyz is params and model._xyz.shape[0] == 300
    assert float(torch.sigmoid(model._opacity).min()) > 0.004, "the dead rows were relocated"
    assert rz.reissued_frames(gpu_device, 300, W, H) == before
