"""The masked losses on the GPU (csrc/masked_loss.hip behind masked_loss.masked_l1_dssim_loss and alpha_mask_loss;
DESIGN.md §7.32) against the float64 restatement of tests/masked_loss_restate.py.

Shapes: 3x5x7 (smaller than the window), 3x16x16 (one tile), 3x17x33 (one past a tile edge on each axis), 1x37x53 and
3x40x48.  Masks: ones, zeros, a hard edge at column 15, 16 and 17 (either side of the tile edge), and a soft one with values
from {0, 0.25, 0.5, 1}.  lambda 0, 0.2 and 1, both normalisations.  gt = x + d with |d| >= 0.02, so m |d| >= 0.005 wherever
m > 0: no pixel sits on the discontinuity of sign() and none is left out of any comparison.

The bar is the project's "2 x the float32 oracle" rule: twice the error the same restatement makes in float32 against
float64 on the same inputs, with a floor of a few float32 ulps of the compared quantity.  The oracle makes the single
roundings of x' and y' itself, so the floor only has to stand for an oracle whose own roundings happened to cancel.
  value     L = (1 - lambda) L1 + lambda Ds, and Ds is a difference: 1 - mean S in image mode, mean_m (1 - S) in mask mode,
            with S within a few per cent of 1 on these inputs (L is 0.013 to 0.13, lambda mean S 0.2 or about 1).  S is
            a float32 quotient: the products N1 N2 and D1 D2, the division and the final float32 of the loss are four
            roundings of a quantity of the size of S, not of 1 - S, and nothing makes them cancel over the pixels.  The
            compared quantity therefore has the two parts L and lambda mean S, and the floor is
            4 * 2^-24 max(|L|, lambda mean S): 4 ulps of L for lambda = 0, of the SSIM mean it is subtracted from otherwise.
            (Measured on one MI355X with the floor at 4 ulps of |L| alone: 173 of 180 cases pass; the seven that miss are
            all lambda = 1, errors 7.2e-9 to 4.0e-8 against float32-oracle errors of 2.7e-10 to 1.7e-8 on the same inputs,
            while the oracle's error on the neighbouring cases is up to 4.6e-8: one ulp of S is 6e-8.)
  gradient  per tensor, max-norm relative to max|g64|: x', y', the three stored derivative maps and the result are rounded
            once each, six half ulps; taken as 4 * 2^-24.
Every test prints the figures it asserts (run with -s)."""
import functools

import pytest
import torch

import masked_loss_restate as R

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24


def same_bits(a, b):
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


@functools.lru_cache(maxsize=None)
def reference(shape, kind, lam, normalize):
    """(x, gt, m, float64 value, float64 gradient, value bar, gradient bar, float32 oracle's errors): computed once per
    case and left unchanged."""
    x, gt = R.images(shape)
    m = R.mask(kind, shape[1], shape[2])
    v64, g64 = R.value_and_grad(R.masked_l1_dssim, x, gt, m, lam, normalize, dtype=torch.float64)
    v32, g32 = R.value_and_grad(R.masked_l1_dssim, x, gt, m, lam, normalize, dtype=torch.float32)
    S = R.ssim_map(m[None].double() * x.double(), m[None].double() * gt.double())
    if normalize == "image" or float(m.sum()) == 0.0:
        s_mean = float(S.mean())
    else:
        s_mean = float((m[None].double() * S).sum() / (shape[0] * m.double().sum()))
    e32_v = abs(v32 - v64)
    scale = float(g64.abs().max())
    e32_g = float((g32.double() - g64).abs().max()) / scale if scale > 0 else 0.0
    bar_v = max(2.0 * e32_v, 4.0 * U32 * max(abs(v64), lam * abs(s_mean)))
    bar_g = max(2.0 * e32_g, 4.0 * U32)
    return x, gt, m, v64, g64, bar_v, bar_g, (e32_v, e32_g)


def fused(dev, x, gt, m, lam, normalize):
    """(loss float32 0-dim, gradient for x, record) of the public call."""
    from mvs_gaussian_splatting_amd import masked_l1_dssim_loss
    xd = x.to(dev).requires_grad_(True)
    loss, record = masked_l1_dssim_loss(xd, gt.to(dev), m.to(dev), lam, normalize, return_record=True)
    (g,) = torch.autograd.grad(loss, xd)
    return loss.detach(), g.detach(), record


def grad_error(got, want):
    scale = float(want.abs().max())
    got = got.double().cpu()
    assert bool(torch.isfinite(got).all())
    if scale == 0.0:
        return (0.0 if not got.any() else float("inf")), scale
    return float((got - want).abs().max()) / scale, scale


@pytest.mark.parametrize("kind", R.MASKS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradient_against_the_float64_restatement(gpu_device, shape, kind):
    for normalize in R.NORMALIZE:
        for lam in R.LAMBDAS:
            x, gt, m, v64, g64, bar_v, bar_g, (e32_v, e32_g) = reference(shape, kind, lam, normalize)
            loss, g, record = fused(gpu_device, x, gt, m, lam, normalize)
            ev = abs(float(loss) - v64)
            eg, _ = grad_error(g, g64)
            print(f"[masked loss] {shape} {kind} {normalize} lambda {lam}: value {float(loss):.8f} err {ev:.2e} (float32 oracle "
                  f"{e32_v:.2e}, bar {bar_v:.2e}); gradient err {eg:.2e} (float32 oracle {e32_g:.2e}, bar {bar_g:.2e})")
            assert ev <= bar_v, (normalize, lam, ev, bar_v)
            assert eg <= bar_g, (normalize, lam, eg, bar_g)
            assert float(record[0].float()) == float(loss) and float(record[5]) == (1.0 if kind == "zeros" and normalize == "mask" else 0.0)
            assert abs(float(record[0]) - ((1.0 - lam) * float(record[1]) + lam * float(record[2]))) <= 1e-15
            if normalize == "mask":
                assert float(record[4]) == float(m.double().sum()) and float(record[3]) == shape[0] * float(m.double().sum())


@pytest.mark.parametrize("kind", R.MASKS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_image_mode_against_the_shipped_loss_of_the_premultiplied_images(gpu_device, shape, kind):
    from mvs_gaussian_splatting_amd import l1_dssim_loss
    for lam in R.LAMBDAS:
        x, gt, m, _, g64, bar_v, bar_g, _ = reference(shape, kind, lam, "image")
        loss, g, _ = fused(gpu_device, x, gt, m, lam, "image")
        xd, md = x.to(gpu_device).requires_grad_(True), m.to(gpu_device)
        comp = l1_dssim_loss(md[None] * xd, md[None] * gt.to(gpu_device), lam)
        (gc,) = torch.autograd.grad(comp, xd)
        ev = abs(float(loss) - float(comp.detach()))
        eg, _ = grad_error(g, gc.double().cpu()) if float(g64.abs().max()) > 0 else (float((g - gc).abs().max()), 0.0)
        print(f"[masked loss vs composition] {shape} {kind} lambda {lam}: fused {float(loss):.8f} composition {float(comp.detach()):.8f} "
              f"gap {ev:.2e} (bar {bar_v:.2e}); gradient gap {eg:.2e} (bar {bar_g:.2e})")
        assert ev <= bar_v and eg <= bar_g, (lam, ev, bar_v, eg, bar_g)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_an_all_ones_mask_is_the_unmasked_loss(gpu_device, shape):
    from mvs_gaussian_splatting_amd import l1_dssim_loss
    for lam in R.LAMBDAS:
        xd = R.images(shape)[0].to(gpu_device).requires_grad_(True)
        plain = l1_dssim_loss(xd, R.images(shape)[1].to(gpu_device), lam)
        (gp,) = torch.autograd.grad(plain, xd)
        for normalize in R.NORMALIZE:
            x, gt, m, _, g64, bar_v, bar_g, _ = reference(shape, "ones", lam, normalize)
            loss, g, _ = fused(gpu_device, x, gt, m, lam, normalize)
            ev = abs(float(loss) - float(plain.detach()))
            eg, _ = grad_error(g, gp.double().cpu())
            print(f"[masked loss, ones] {shape} {normalize} lambda {lam}: fused {float(loss):.8f} unmasked {float(plain.detach()):.8f} gap "
                  f"{ev:.2e} (bar {bar_v:.2e}); gradient gap {eg:.2e} (bar {bar_g:.2e})")
            assert ev <= bar_v and eg <= bar_g, (normalize, lam, ev, bar_v, eg, bar_g)


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_an_all_zeros_mask_gives_exactly_zero(gpu_device, shape):
    x, gt = R.images(shape)
    m = R.mask("zeros", shape[1], shape[2])
    for lam in R.LAMBDAS:
        for normalize in R.NORMALIZE:
            loss, g, record = fused(gpu_device, x, gt, m, lam, normalize)
            assert float(loss) == 0.0 and float(record[0]) == 0.0 and not bool(g.any()), (lam, normalize, float(record[0]))
            assert float(record[5]) == (1.0 if normalize == "mask" else 0.0)


@pytest.mark.parametrize("kind", ["edge15", "edge16", "edge17", "soft"])
@pytest.mark.parametrize("shape", R.SHAPES[2:], ids=lambda s: "x".join(map(str, s)))
def test_what_the_mask_hides_changes_no_bit(gpu_device, shape, kind):
    x, gt = R.images(shape)
    m = R.mask(kind, shape[1], shape[2])
    hidden = (m == 0)[None].expand(shape)
    assert bool(hidden.any()) and bool((~hidden).any())
    g = torch.Generator().manual_seed(5)
    other = torch.where(hidden, 1000.0 * (torch.rand(shape, generator=g) - 0.5), gt)
    other[:, 0, -1] = -3.0e38 if bool(hidden[0, 0, -1]) else other[:, 0, -1]          # finite, and as large as float32 goes
    assert not torch.equal(other, gt)
    for normalize in R.NORMALIZE:
        for lam in R.LAMBDAS:
            loss_a, grad_a, rec_a = fused(gpu_device, x, gt, m, lam, normalize)
            loss_b, grad_b, rec_b = fused(gpu_device, x, other, m, lam, normalize)
            assert same_bits(loss_a, loss_b) and same_bits(rec_a, rec_b) and same_bits(grad_a, grad_b), (normalize, lam)
            assert not bool(grad_a[hidden.to(gpu_device)].any())
            assert bool(torch.isfinite(grad_a).all()) and (lam == 1.0 or bool((grad_a[~hidden.to(gpu_device)] != 0).all()))


@pytest.mark.parametrize("shape", [(3, 40, 48), (3, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_and_a_dirty_workspace_give_the_same_bits(gpu_device, shape):
    from mvs_gaussian_splatting_amd import masked_loss as ml
    x, gt = (t.to(gpu_device) for t in R.images(shape))
    m = R.mask("soft", shape[1], shape[2]).to(gpu_device)
    for normalize in R.NORMALIZE:
        rec_a, grad_a, ws = ml._call(x, gt, m, 0.2, normalize, True)
        ws.fill_(0xA5)
        rec_b, grad_b, _ = ml._call(x, gt, m, 0.2, normalize, True, ws)
        rec_c, grad_c, _ = ml._call(x, gt, m, 0.2, normalize, True)
        assert same_bits(rec_a, rec_b) and same_bits(rec_a, rec_c) and same_bits(grad_a, grad_b) and same_bits(grad_a, grad_c)
        rec_d, none, _ = ml._call(x, gt, m, 0.2, normalize, False)
        assert none is None and same_bits(rec_a, rec_d)
        assert float(rec_a[0]) > 0 and bool(torch.isfinite(grad_a).all())


def test_autograd_scales_the_unit_gradient_and_takes_either_mask_shape(gpu_device):
    from mvs_gaussian_splatting_amd import masked_l1_dssim_loss
    shape = (3, 17, 33)
    x, gt = (t.to(gpu_device) for t in R.images(shape))
    m = R.mask("soft", 17, 33).to(gpu_device)
    xa = x.clone().requires_grad_(True)
    (2.5 * masked_l1_dssim_loss(xa, gt, m, 0.2, "mask")).backward()
    xb = x.clone().requires_grad_(True)
    masked_l1_dssim_loss(xb, gt, m[None], 0.2, "mask").backward()
    assert same_bits(xa.grad, xb.grad * 2.5)
    without = masked_l1_dssim_loss(x, gt, m, 0.2, "mask")
    assert not without.requires_grad and without.dtype == torch.float32 and without.dim() == 0
    # strided inputs are made contiguous: the contiguous call's bits
    wide = torch.zeros(3, 17, 66, device=gpu_device)
    wide[:, :, ::2] = x
    xs = wide[:, :, ::2].requires_grad_(True)
    assert not xs.is_contiguous()
    loss = masked_l1_dssim_loss(xs, gt, m, 0.2, "mask")
    (gs,) = torch.autograd.grad(loss, xs)
    assert same_bits(loss.detach(), without) and same_bits(gs, xb.grad)


# ---- the silhouette term ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def alpha_case(H, W):
    g = torch.Generator().manual_seed(H * 131 + W)
    a = (0.01 + 0.98 * torch.rand(H, W, generator=g, dtype=torch.float32)).contiguous()
    m = R.mask("soft" if H == 37 else "edge16", H, W)
    flat = a.view(-1)
    flat[0], flat[1], flat[2], flat[3] = 0.0, 1.0, 0.0, 1.0                            # clamped: the bce gradient is 0 there
    mflat = m.view(-1)
    mflat[0], mflat[1], mflat[2], mflat[3] = 1.0, 0.0, 0.0, 1.0
    return a, m


@pytest.mark.parametrize("mode", ["l1", "bce"])
@pytest.mark.parametrize("shape", [(17, 33), (37, 53)], ids=lambda s: "x".join(map(str, s)))
def test_alpha_mask_loss_against_the_float64_restatement(gpu_device, shape, mode):
    from mvs_gaussian_splatting_amd import alpha_mask_loss
    a, m = alpha_case(*shape)
    v64, g64 = R.value_and_grad(R.alpha_mask, a, m, mode, dtype=torch.float64)
    v32, g32 = R.value_and_grad(R.alpha_mask, a, m, mode, dtype=torch.float32)
    scale = float(g64.abs().max())
    e32_v, e32_g = abs(v32 - v64), float((g32.double() - g64).abs().max()) / scale
    # floor: the inputs are exact, the value and each gradient are rounded to float32 once: one ulp
    bar_v, bar_g = max(2.0 * e32_v, 2.0 * U32 * abs(v64)), max(2.0 * e32_g, 2.0 * U32)
    runs = []
    for form in ("[H,W]", "[1,H,W]"):
        ad = (a if form == "[H,W]" else a[None]).to(gpu_device).requires_grad_(True)
        loss = alpha_mask_loss(ad, m.to(gpu_device), mode=mode)
        (g,) = torch.autograd.grad(loss, ad)
        assert g.shape == ad.shape
        runs.append((loss.detach(), g.detach().reshape(shape)))
    loss, g = runs[0]
    assert same_bits(loss, runs[1][0]) and same_bits(g, runs[1][1]), "two runs, two call forms: the same bits"
    ev, (eg, _) = abs(float(loss) - v64), grad_error(g, g64)
    print(f"[alpha mask] {shape} {mode}: value {float(loss):.8f} err {ev:.2e} (float32 oracle {e32_v:.2e}, bar {bar_v:.2e}); "
          f"gradient err {eg:.2e} (float32 oracle {e32_g:.2e}, bar {bar_g:.2e})")
    assert ev <= bar_v and eg <= bar_g
    if mode == "bce":
        assert g.view(-1)[:4].tolist() == [0.0, 0.0, 0.0, 0.0] and bool((g.view(-1)[4:] != 0).all())
    without = alpha_mask_loss(a.to(gpu_device), m.to(gpu_device), mode=mode)
    assert not without.requires_grad and same_bits(without, loss)
