"""Restatement of the depth-distortion map over the oracle's public results (float64 or float32).

For a pixel, i runs over the entries of its tile's list that the oracle's colour pass composited (the entries of
tests/depth_restate.py: the first ``n_contrib[pixel]`` entries that pass the oracle's two skip tests).  With
``w_i = alpha_i T_i``, ``z_i`` the view-space depth and ``m_i = m(z_i)``:

    dist = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2          (no background term)
    m(z) = z ("linear"),   m(z) = far / (far - near) (1 - near / z) ("ndc")

stated literally: the matrix of squared differences ``(m_i - m_j)^2`` of a tile's entries, its strict lower triangle
(j < i in list order), and per pixel the double sum of ``w_i w_j`` times it.  No prefix recurrence and no moments: the
sum is independent of the kernel's algebra, and in float32 every term is a non-negative product of differences.
Autograd reaches the operator's inputs through the oracle's own preprocess (``pre["v_depth"]``, ``v_xy``, ``v_conic``,
``v_opacity``).  Shared by tests/test_distortion_host.py and tests/test_gpu_distortion.py.
"""
import numpy as np
import torch

from depth_restate import ALPHA_MAX, ALPHA_MIN, TILE
from oracle import rasterize_ref

NEAR, FAR = 0.2, 100.0


def mapped_depth(z, mapping, near=NEAR, far=FAR):
    if mapping == "linear":
        return z
    assert mapping == "ndc"
    return far / (far - near) * (1.0 - near / z)


def tile_weights(pre, point_list, ranges, n_contrib, settings):
    """Yields, per tile with a contributor, (ty, tx, slots [n], w [n,256]): the rows of ``pre`` of the tile's first n list
    entries and their blending weights at its 256 pixels (0 where the entry is not composited), in the dtype of ``pre``."""
    dt = pre["v_xy"].dtype
    H, W = int(settings.image_height), int(settings.image_width)
    grid_x, grid_y = pre["grid"]
    slot_of = torch.full((int(pre["radii"].shape[0]),), -1, dtype=torch.int64)
    slot_of[pre["idx"]] = torch.arange(pre["idx"].shape[0])
    plist = torch.from_numpy(np.asarray(point_list).astype(np.int64))
    xy, conic, opac = pre["v_xy"], pre["v_conic"], pre["v_opacity"]
    lx = torch.arange(TILE).repeat(TILE)
    ly = torch.arange(TILE).repeat_interleave(TILE)
    a_min = torch.tensor(ALPHA_MIN, dtype=dt)
    nc = torch.zeros(grid_y * TILE, grid_x * TILE, dtype=torch.int64)
    nc[:H, :W] = n_contrib.to(torch.int64)
    for ty in range(grid_y):
        for tx in range(grid_x):
            t = ty * grid_x + tx
            last = nc[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(-1)
            n = int(last.max())
            if n == 0:
                continue
            s = int(ranges[t, 0])
            assert s + n <= int(ranges[t, 1])
            sl = slot_of[plist[s:s + n]]
            pxf = (tx * TILE + lx).to(dt)
            pyf = (ty * TILE + ly).to(dt)
            g_xy, g_con, g_o = xy[sl], conic[sl], opac[sl]
            dx = g_xy[:, 0:1] - pxf[None, :]
            dy = g_xy[:, 1:2] - pyf[None, :]
            power = -0.5 * (g_con[:, 0:1] * dx * dx + g_con[:, 2:3] * dy * dy) - g_con[:, 1:2] * dx * dy
            raw = g_o[:, None] * torch.exp(power)
            alpha = raw + (torch.clamp_max(raw, ALPHA_MAX) - raw).detach()
            pos = torch.arange(n)[:, None]
            use = (power <= 0) & (alpha >= a_min) & (pos < last[None, :])
            one_minus = torch.where(use, 1.0 - alpha, torch.ones_like(alpha))
            cp = torch.cumprod(one_minus, dim=0)
            T_excl = torch.cat([torch.ones(1, TILE * TILE, dtype=dt), cp[:-1]], dim=0)
            yield ty, tx, sl, torch.where(use, alpha * T_excl, torch.zeros_like(alpha))


def _assemble(tiles, grid, H, W, dt):
    grid_x, grid_y = grid
    zero = torch.zeros(TILE, TILE, dtype=dt)
    rows = [torch.cat([tiles.get((ty, tx), zero) for tx in range(grid_x)], dim=1) for ty in range(grid_y)]
    return torch.cat(rows, dim=0)[None, :H, :W]


def distortion_from_lists(pre, point_list, ranges, n_contrib, settings, mapping="ndc", near=NEAR, far=FAR):
    """-> dist [1,H,W] in the dtype of ``pre``: per pixel the double sum over pairs j < i of w_i w_j (m_i - m_j)^2."""
    dt = pre["v_xy"].dtype
    tiles = {}
    for ty, tx, sl, w in tile_weights(pre, point_list, ranges, n_contrib, settings):
        m = mapped_depth(pre["v_depth"][sl], mapping, near, far)
        pair = torch.tril((m[:, None] - m[None, :]) ** 2, diagonal=-1)      # [i, j] = (m_i - m_j)^2 for j < i, else 0
        tiles[(ty, tx)] = torch.einsum("ip,ij,jp->p", w, pair, w).reshape(TILE, TILE)
    return _assemble(tiles, pre["grid"], int(settings.image_height), int(settings.image_width), dt)


def moments_from_lists(pre, point_list, ranges, n_contrib, settings, mapping="ndc", near=NEAR, far=FAR):
    """-> (A, M1, M2), each [1,H,W]: sum w, sum w m, sum w m^2 -- what ``A M2 - M1^2`` is formed from (the route the kernel
    does not take; tests/test_distortion_host.py measures what it loses in float32)."""
    dt = pre["v_xy"].dtype
    A, M1, M2 = {}, {}, {}
    for ty, tx, sl, w in tile_weights(pre, point_list, ranges, n_contrib, settings):
        m = mapped_depth(pre["v_depth"][sl], mapping, near, far)
        A[(ty, tx)] = w.sum(0).reshape(TILE, TILE)
        M1[(ty, tx)] = (w * m[:, None]).sum(0).reshape(TILE, TILE)
        M2[(ty, tx)] = (w * (m * m)[:, None]).sum(0).reshape(TILE, TILE)
    H, W = int(settings.image_height), int(settings.image_width)
    return tuple(_assemble(t, pre["grid"], H, W, dt) for t in (A, M1, M2))


def distortion_ref(means3D, means2D, opacities, settings, mapping="ndc", near=NEAR, far=FAR, **kw):
    """The oracle's frame and its distortion map: -> (dist [1,H,W], color, radii, aux) with ``aux["margin"]`` etc."""
    color, radii, aux = rasterize_ref(means3D, means2D, opacities, settings, want_aux=True, want_margin=True, **kw)
    dist = distortion_from_lists(aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], settings, mapping, near,
                                 far)
    return dist, color, radii, aux


def dist_weights(H, W, seed=4717):
    """Fixed weights in (-1, 1) for the smooth loss ``sum(w * dist) / (H W)``."""
    return torch.rand((1, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2.0 - 1.0


def dist_loss(dist, weights):
    return (dist * weights.to(dist.dtype).to(dist.device)).sum() / weights.numel()


def slab_model(model, centre=5.0, half=0.005):
    """``model`` with every view depth of the identity camera moved into ``centre +- half`` (the ordering of the depths
    is kept): the thin slab a converged distortion loss produces."""
    z = model._xyz[:, 2]
    lo, hi = float(z.min()), float(z.max())
    model._xyz[:, 2] = centre + ((z - lo) / (hi - lo) * 2.0 - 1.0) * half
    return model
