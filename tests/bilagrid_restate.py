"""The definitions of DESIGN.md §7.25 in torch on the CPU, at float64 and at float32: the slice as ``F.grid_sample`` on a
5-D input (``align_corners=True``, ``padding_mode="border"``) followed by the affine, with autograd for both gradients;
the total-variation term literally as defined; the inputs of tests/test_gpu_bilagrid.py and
tests/test_bilagrid_host.py; and the fragile set of an input."""
import torch
import torch.nn.functional as F

F64 = torch.float64

IMAGE_SHAPES = ((1, 1), (7, 5), (65, 9), (70, 37), (3, 130))          # H x W
GRID_SHAPES = ((2, 2, 2), (3, 5, 4), (16, 16, 8))                     # (Wg, Hg, L)
TV_CASES = ((1, (3, 5, 4)), (3, (3, 5, 4)), (65, (3, 5, 4)), (2, (16, 16, 8)))
FLOOR = 2.0 ** -22        # the rounding of the inputs' products plus the output's own rounding
FRAGILE_BAND = 1e-4       # |z - nearest integer level|
FRAGILE_CAP = 0.02


def make_image(H, W, seed=0):
    """Colours uniform in [0.05, 0.95] and a stripe of values at -0.2 and 1.3 (the clamp of the luminance)."""
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    x = 0.05 + 0.9 * torch.rand(3, H, W, generator=g)
    if W >= 5:
        x[:, :, 1] = -0.2
        x[:, :, W - 2] = 1.3
    return x.to(torch.float32)


def make_grid(shape, seed=0):
    Wg, Hg, L = shape
    g = torch.Generator().manual_seed(77 + Wg + 100 * Hg + 10000 * L + seed)
    eye = torch.eye(3, 4).reshape(12, 1, 1, 1)
    return (eye + 0.5 * torch.randn(12, L, Hg, Wg, generator=g)).to(torch.float32)


def make_upstream(H, W, seed=0):
    g = torch.Generator().manual_seed(31 * H + 7 * W + seed)
    return torch.randn(3, H, W, generator=g).to(torch.float32)


def identity_grid(shape):
    Wg, Hg, L = shape
    return torch.eye(3, 4).reshape(12, 1, 1, 1).expand(12, L, Hg, Wg).contiguous()


def gray(x):
    return (0.299 * x[0] + 0.587 * x[1]) + 0.114 * x[2]


def slice_grid(x, grid, dtype=F64):
    """``Y [3,H,W]`` of image ``x [3,H,W]`` and ``grid [12,L,Hg,Wg]`` in ``dtype``; differentiable in both."""
    x, grid = x.to(dtype), grid.to(dtype)
    H, W = x.shape[1:]
    xs = (torch.arange(W, dtype=dtype) + 0.5) / W
    ys = (torch.arange(H, dtype=dtype) + 0.5) / H
    coords = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), gray(x)], dim=-1)      # (x, y, z) in [0, 1]
    coords = (coords * 2.0 - 1.0)[None, None]                                                         # [1,1,H,W,3]
    A = F.grid_sample(grid[None], coords, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
    A = A.reshape(3, 4, H, W)
    return ((A[:, 0] * x[0] + A[:, 1] * x[1]) + A[:, 2] * x[2]) + A[:, 3]


def slice_with_grads(x, grid, up, dtype=F64):
    """(Y, dL/dx, dL/dgrid) for L = sum(Y up), all in ``dtype``."""
    xg, gg = x.to(dtype).clone().requires_grad_(True), grid.to(dtype).clone().requires_grad_(True)
    y = slice_grid(xg, gg, dtype)
    y.backward(up.to(dtype))
    return y.detach(), xg.grad, gg.grad


def tv(grids, dtype=F64):
    """``(1/N) sum_n sum_axis mean((grids[n] shifted by one along the axis - grids[n])^2)``, axes z, y, x."""
    g = grids.to(dtype)
    total = 0.0
    for n in range(g.shape[0]):
        total = total + ((g[n, :, 1:] - g[n, :, :-1]) ** 2).mean() + ((g[n, :, :, 1:] - g[n, :, :, :-1]) ** 2).mean() + \
            ((g[n, :, :, :, 1:] - g[n, :, :, :, :-1]) ** 2).mean()
    return total / g.shape[0]


def tv_with_grad(grids, dtype=F64):
    g = grids.to(dtype).clone().requires_grad_(True)
    value = tv(g, dtype)
    value.backward()
    return value.detach(), g.grad


def make_grids(N, shape, seed=0):
    return torch.stack([make_grid(shape, seed + 13 * n) for n in range(N)])


def fragile(x, L):
    """``[H,W]`` bool: the pixels whose ``z = clamp(gray, 0, 1) (L - 1)``, evaluated at float64, lies within
    ``FRAGILE_BAND`` of an integer level -- which includes a ``gray`` within ``FRAGILE_BAND / (L - 1)`` of 0 or 1 from
    inside and every clamped pixel exactly on a level.  There the slope ``dA/dz`` or the clamp decision may flip between
    two evaluations, so ``dX`` is not compared; ``Y`` and ``dG`` are continuous and are compared everywhere.  A clamped
    pixel outside the band around 0 and 1 (``gray`` well below 0 or above 1) has a firm decision and ``z`` exactly on a
    level with ``dz/dgray = 0``: its ``dX`` does not see the slope and it is not fragile."""
    gr = gray(x.to(F64))
    z = gr.clamp(0.0, 1.0) * (L - 1)
    near = (z - z.round()).abs() < FRAGILE_BAND
    firm_clamp = (gr < -FRAGILE_BAND / (L - 1)) | (gr > 1.0 + FRAGILE_BAND / (L - 1))
    return near & ~firm_clamp


def census(x, L):
    """(fragile pixels, pixels, the cap in pixels: 2 % of the input, one pixel where that would be none)."""
    n = int(fragile(x, L).sum())
    pixels = x.shape[1] * x.shape[2]
    return n, pixels, max(int(FRAGILE_CAP * pixels), 1)


def rel_err(got, ref):
    """The largest error as a share of the largest magnitude in ``ref``: the project's standing measure."""
    ref = ref.to(F64)
    if ref.numel() == 0:
        return 0.0
    return float((got.to(F64) - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def bar(own):
    """Twice the float32 restatement's own error, not less than 2^-22."""
    return max(2.0 * own, FLOOR)


def check_slice(got, x, grid, up, label, log=print):
    """The GPU test's bar: Y, dG everywhere and dX off the fragile set within twice the float32 restatement's own error
    (not less than 2^-22) of the float64 restatement, as a share of the largest magnitude in the tensor."""
    y, dx, dg = got
    L = grid.shape[1]
    r64, r32 = slice_with_grads(x, grid, up), slice_with_grads(x, grid, up, torch.float32)
    firm = ~fragile(x, L)
    n_fragile, pixels, cap = census(x, L)
    assert n_fragile <= cap, f"{label}: {n_fragile} fragile pixels of {pixels}, above the cap of {cap}"
    rows = []
    for name, g, a, b in (("Y", y, r64[0], r32[0]), ("dX", dx[:, firm], r64[1][:, firm], r32[1][:, firm]),
                          ("dG", dg, r64[2], r32[2])):
        err, own = rel_err(g, a), rel_err(b, a)
        rows.append((name, err, own))
        log(f"{label} {name}: error {err:.3e}  float32 restatement {own:.3e}  bar {bar(own):.3e}  "
            f"fragile {n_fragile}/{pixels}")
    for name, err, own in rows:
        assert err <= bar(own), f"{label} {name}: {err:.3e} above the bar {bar(own):.3e}"
