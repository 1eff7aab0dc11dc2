"""Torch restatement of the masked losses (mvs_gaussian_splatting_amd/masked_loss.py) from their
definitions, in whatever dtype its inputs have: float64 is the truth the GPU tests compare against, float32 the "float32
oracle" whose own error sets their bar.  Differentiable by autograd; nothing here touches a GPU or the library.

    x' = m x,  y' = m gt,  S = SSIM map of x', y' (11x11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2)
    image:  L1 = sum|x' - y'| / (C H W)      Ds = 1 - sum S / (C H W)
    mask:   Z = C sum m;  L1 = sum|x' - y'| / Z,  Ds = sum m (1 - S) / Z;   Z = 0: loss 0
    loss = (1 - lambda) L1 + lambda Ds
"""
import math

import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2
ALPHA_LO = float(torch.tensor(1e-6, dtype=torch.float32))                     # the bce clamp, float32 constants
ALPHA_HI = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-6, dtype=torch.float32))

SHAPES = [(3, 5, 7), (3, 16, 16), (3, 17, 33), (1, 37, 53), (3, 40, 48)]
MASKS = ["ones", "zeros", "edge15", "edge16", "edge17", "soft"]
LAMBDAS = [0.0, 0.2, 1.0]
NORMALIZE = ["image", "mask"]


def window(dtype, device="cpu"):
    """The 11 taps the reference builds in float32 (exp per tap, a float32 normalisation), in ``dtype``."""
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2.0 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    return (g / g.sum()).to(dtype).to(device)


def ssim_map(x, y):
    """``S [C,H,W]`` of two ``[C,H,W]`` images: the depthwise 11x11 window as the outer product of the taps."""
    Cn = x.shape[0]
    w1 = window(x.dtype, x.device)
    w2 = (w1[:, None] * w1[None, :]).expand(Cn, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t[None], w2, padding=5, groups=Cn)[0]            # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(x * x) - mu1_sq, conv(y * y) - mu2_sq, conv(x * y) - mu12
    return ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def l1_dssim(x, gt, lam):
    """The unmasked training loss ``(1 - lam) mean|x - gt| + lam (1 - mean S)``."""
    return (1.0 - lam) * (x - gt).abs().mean() + lam * (1.0 - ssim_map(x, gt).mean())


def masked_l1_dssim(x, gt, m, lam, normalize):
    """The masked loss; ``m`` is ``[H,W]``.  Returns a 0-dim tensor; with ``Z = 0`` a zero that still hangs on ``x``, so
    that autograd gives the all-zero gradient."""
    xp, yp = m[None] * x, m[None] * gt
    S = ssim_map(xp, yp)
    n = x.numel()
    if normalize == "image":
        l1 = (xp - yp).abs().sum() / n
        ds = 1.0 - S.sum() / n
    elif normalize == "mask":
        Z = x.shape[0] * m.sum()
        if float(Z) <= 0.0:
            return (xp.sum() * 0.0)
        l1 = (xp - yp).abs().sum() / Z
        ds = (m[None] * (1.0 - S)).sum() / Z
    else:
        raise ValueError(normalize)
    return (1.0 - lam) * l1 + lam * ds


def alpha_mask(a, m, mode):
    """The silhouette term of ``a [H,W]`` against ``m [H,W]``: ``mean|a - m|`` or the clamped binary cross-entropy, whose
    gradient is 0 where ``a`` was clamped (``torch.clamp``'s own rule off the closed ends)."""
    if mode == "l1":
        return (a - m).abs().mean()
    if mode == "bce":
        ah = a.clamp(ALPHA_LO, ALPHA_HI)                     # autograd: gradient 1 on [lo, hi], 0 where a was clamped
        return -(m * torch.log(ah) + (1.0 - m) * torch.log1p(-ah)).mean()
    raise ValueError(mode)


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------
def images(shape, seed=0):
    """(x, gt) float32 ``[C,H,W]``: x uniform in [0.1, 0.9] -- textured, so that the windowed variances stand well above
    the float32 rounding of the moments --, gt = x + d with 0.02 <= |d| <= 0.12 and a random sign: m |d| >= 0.005 for
    every m >= 0.25, no pixel sits on the discontinuity of sign()."""
    g = torch.Generator().manual_seed(1000 * seed + shape[0] * 100003 + shape[1] * 1009 + shape[2])
    x = 0.1 + 0.8 * torch.rand(shape, generator=g, dtype=torch.float32)
    mag = 0.02 + 0.1 * torch.rand(shape, generator=g, dtype=torch.float32)
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    gt = x + sign * mag
    assert float((gt - x).abs().min()) >= 0.02 - 1e-7
    return x.contiguous(), gt.contiguous()


def mask(kind, H, W, seed=0):
    """float32 ``[H,W]``: all ones, all zeros, a hard edge at a column (ones to its left), or values from {0, 0.25, 0.5, 1}."""
    if kind == "ones":
        return torch.ones(H, W)
    if kind == "zeros":
        return torch.zeros(H, W)
    if kind.startswith("edge"):
        col = int(kind[4:])
        m = torch.zeros(H, W)
        m[:, :col] = 1.0
        return m
    if kind == "soft":
        g = torch.Generator().manual_seed(77 + seed + 31 * H + W)
        levels = torch.tensor([0.0, 0.25, 0.5, 1.0])
        return levels[torch.randint(0, 4, (H, W), generator=g)].contiguous()
    raise ValueError(kind)


def value_and_grad(fn, x, *rest, dtype):
    """(value float, gradient for the first argument) of ``fn`` evaluated in ``dtype``."""
    xl = x.detach().to(dtype).requires_grad_(True)
    out = fn(xl, *[r.to(dtype) if isinstance(r, torch.Tensor) else r for r in rest])
    (g,) = torch.autograd.grad(out, xl, allow_unused=True)
    return float(out.detach().double()), (torch.zeros_like(xl) if g is None else g).detach()
