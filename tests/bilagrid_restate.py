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
# The limits of the accepted range 2..64 x 2..64 x 2..16: ((H, W), (Wg, Hg, L), lanes of the grid-gradient block = 64 L,
# whether 12 L Hg Wg floats fit the 24576 of the staged kernel's LDS, row shares of a vertex's rectangle)
LIMIT_CASES = (
    ((70, 37), (2, 2, 16), 1024, True, 8),         # L = 16: sixteen waves a block, every extent else at its minimum
    ((3, 130), (2, 2, 16), 1024, True, 1),
    ((70, 37), (5, 3, 16), 1024, True, 5),
    ((3, 130), (5, 3, 16), 1024, True, 1),
    ((70, 37), (16, 16, 16), 1024, False, 1),      # the default extents at L = 16: twice what LDS holds
    ((3, 130), (16, 16, 16), 1024, False, 1),
    ((7, 5), (64, 2, 2), 128, True, 2),            # each extent at 64: a launch grid of 64 blocks along x, along y, both
    ((70, 37), (64, 2, 2), 128, True, 8),
    ((7, 5), (2, 64, 2), 128, True, 1),
    ((70, 37), (2, 64, 2), 128, True, 1),
    ((7, 5), (64, 64, 2), 128, False, 1),
    ((70, 37), (64, 64, 2), 128, False, 1),
    ((7, 5), (64, 64, 16), 1024, False, 1),        # every extent at its maximum
    ((70, 37), (64, 64, 16), 1024, False, 1),
    ((65, 9), (33, 17, 9), 576, False, 1),         # odd, no power of two, the middle pixel exactly on a vertex
)
LARGE_IMAGE = (513, 512)                          # past the 262144 pixels at which a grid that fits is staged in LDS
LARGE_GRIDS = ((16, 16, 8), (16, 16, 16))         # fits LDS and is staged; does not fit
BLACK_IMAGE = (70, 37)
BLACK_GRIDS = ((3, 5, 4), (16, 16, 8))
# (N, (Wg, Hg, L), blocks of bilagrid_tv_kernel, passes of its grid stride): past 256 slots, past the cap of 1024 blocks
TV_LIMIT_CASES = (
    (3, (16, 16, 8), 288, 1),                     # 73728 elements: the finish kernel's second trip over the slots
    (11, (16, 16, 8), 1024, 2),                   # 270336: the cap is reached and 8192 elements take a second pass
    (1, (64, 64, 16), 1024, 3),                   # 786432: three full passes
    (2, (2, 2, 16), 6, 1),                        # each extent at its maximum beside the others at their minimum
    (1, (64, 2, 2), 12, 1),
    (1, (2, 64, 2), 12, 1),
)
TV_STRUCTURAL_CASE = (11, (16, 16, 8))            # the first size past the cap
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


def make_image_with_black(H, W, seed=0):
    """``make_image`` with exactly black pixels, the uncovered pixel of a render on a black background: a rectangle of
    6 x 5 zeros in all three channels about the middle of the image, across a cell boundary in x and in y of every grid
    of ``BLACK_GRIDS`` at ``BLACK_IMAGE``, and four single pixels, two of them in corners.  Their luminance is exactly
    0: ``z = 0`` with ``dz/dgray = 0``.  Returns the image and the ``[H,W]`` bool mask of the black pixels."""
    x = make_image(H, W, seed)
    black = torch.zeros(H, W, dtype=torch.bool)
    black[H // 2 - 20:H // 2 - 14, W // 2 - 2:W // 2 + 3] = True
    for py, px in ((0, 0), (H - 1, W - 1), (5, W - 7), (H - 20, 7)):
        black[py, px] = True
    x[:, black] = 0.0
    return x, black


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


def slice_coefficients(x, grid, dtype=F64):
    """``A [3,4,H,W]``: the affine the grid holds at each pixel of ``x``, in ``dtype``; differentiable in both."""
    x, grid = x.to(dtype), grid.to(dtype)
    H, W = x.shape[1:]
    xs = (torch.arange(W, dtype=dtype) + 0.5) / W
    ys = (torch.arange(H, dtype=dtype) + 0.5) / H
    coords = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), gray(x)], dim=-1)      # (x, y, z) in [0, 1]
    coords = (coords * 2.0 - 1.0)[None, None]                                                         # [1,1,H,W,3]
    A = F.grid_sample(grid[None], coords, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
    return A.reshape(3, 4, H, W)


def slice_grid(x, grid, dtype=F64):
    """``Y [3,H,W]`` of image ``x [3,H,W]`` and ``grid [12,L,Hg,Wg]`` in ``dtype``; differentiable in both."""
    x = x.to(dtype)
    A = slice_coefficients(x, grid, dtype)
    return ((A[:, 0] * x[0] + A[:, 1] * x[1]) + A[:, 2] * x[2]) + A[:, 3]


def slice_with_grads(x, grid, up, dtype=F64):
    """(Y, dL/dx, dL/dgrid) for L = sum(Y up), all in ``dtype``."""
    xg, gg = x.to(dtype).clone().requires_grad_(True), grid.to(dtype).clone().requires_grad_(True)
    y = slice_grid(xg, gg, dtype)
    y.backward(up.to(dtype))
    return y.detach(), xg.grad, gg.grad


def image_grad_without_the_luminance(x, grid, up, dtype=F64):
    """``A^T g``: ``dL/dx[k] = sum_c A[c,k] up[c]``, what is left of ``dL/dx`` where ``dz/dgray = 0``."""
    A, up = slice_coefficients(x, grid, dtype), up.to(dtype)
    return (A[0, :3] * up[0] + A[1, :3] * up[1]) + A[2, :3] * up[2]


def vertex_weights(x, shape):
    """``[L,Hg,Wg]`` float64: the sum over the pixels of ``x`` of the trilinear weight each puts on a vertex, which is
    ``dL/dgrid`` of a one-channel grid under an upstream gradient of ones.  Exactly 0 where no pixel reaches."""
    Wg, Hg, L = shape
    one = torch.zeros(12, L, Hg, Wg, dtype=F64, requires_grad=True)
    slice_coefficients(x, one)[0, 0].sum().backward()
    return one.grad[0]


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


def make_constant_term_grids(N, shape):
    """Grids in which each of the 12 terms of each image is one small integer, another for every term and image: every
    difference inside a term is exactly 0, every difference across a row, slab, term or image boundary is not."""
    Wg, Hg, L = shape
    values = torch.arange(N * 12, dtype=torch.float32) - 6.0 * N
    return values.reshape(N, 12, 1, 1, 1).expand(N, 12, L, Hg, Wg).contiguous()


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


def check_black(dx, x, black, grid, up, label, log=print):
    """At the exactly black pixels ``black`` (which are fragile, so ``check_slice`` leaves their ``dX`` out) ``dL/dx`` is
    ``A^T g``, the luminance path adding exactly nothing: against the float64 restatement's sliced ``A``, at the bar."""
    want = image_grad_without_the_luminance(x, grid, up)[:, black]
    own = rel_err(image_grad_without_the_luminance(x, grid, up, torch.float32)[:, black], want)
    err = rel_err(dx[:, black], want)
    log(f"{label} dX at {int(black.sum())} black pixels: error {err:.3e}  float32 restatement {own:.3e}  "
        f"bar {bar(own):.3e}")
    assert err <= bar(own), f"{label} dX at the black pixels: {err:.3e} above the bar {bar(own):.3e}"


def check_untouched(dg, x, shape, label, log=print):
    """The vertices no pixel of ``x`` puts a weight on: their ``dG`` is exact zeros, and no other element is one, so the
    zeros are as many as the restatement's weights say.  Returns the number of such vertices."""
    none = vertex_weights(x, shape) == 0
    assert bool((dg[:, none] == 0).all()), f"{label}: a vertex no pixel touches has a gradient"
    zeros, want = int((dg == 0).sum()), 12 * int(none.sum())
    log(f"{label}: {zeros} exact zeros in dG, {want} elements at vertices without a pixel, of {dg.numel()}")
    assert zeros == want, f"{label}: {zeros} exact zeros in dG, {want} elements at vertices without a pixel"
    return int(none.sum())
