"""Restatement of the per-Gaussian contribution statistics over the oracle's public results (float64 or float32).

For Gaussian g, p runs over the pixels where the oracle's colour pass composited g: the entries among the first
``n_contrib[pixel]`` of the tile's list that pass the oracle's two skip tests (``power > 0``, ``alpha < 1/255``), the rule
of tests/depth_restate.py, and ``w = alpha T`` with T the transmittance in front of the entry -- the same ``w`` matrix per
tile, scatter-added per Gaussian id instead of summed per pixel:

    sum[g] = sum_p w (unquantised),   count[g] = number of such pixels,   max[g] = max_p w

optionally under a pixel mask (pixels with a zero / False entry are left out of all three).  Shared by
tests/test_contribution_host.py and tests/test_gpu_contribution.py.
"""
import numpy as np
import torch

from depth_restate import ALPHA_MAX, ALPHA_MIN, TILE


def stats_from_lists(pre, point_list, ranges, n_contrib, settings, mask=None):
    """-> (sum [P] in the dtype of ``pre``, count [P] int64, max [P] in the dtype of ``pre``); ``mask``: None or [H,W]."""
    dt = pre["v_xy"].dtype
    H, W = int(settings.image_height), int(settings.image_width)
    grid_x, grid_y = pre["grid"]
    P = int(pre["radii"].shape[0])
    slot_of = torch.full((P,), -1, dtype=torch.int64)
    slot_of[pre["idx"]] = torch.arange(pre["idx"].shape[0])
    plist = torch.from_numpy(np.asarray(point_list).astype(np.int64))
    xy, conic, opac = pre["v_xy"].detach(), pre["v_conic"].detach(), pre["v_opacity"].detach()
    lx = torch.arange(TILE).repeat(TILE)
    ly = torch.arange(TILE).repeat_interleave(TILE)
    a_min = torch.tensor(ALPHA_MIN, dtype=dt)
    nc = torch.zeros(grid_y * TILE, grid_x * TILE, dtype=torch.int64)
    nc[:H, :W] = n_contrib.to(torch.int64)
    if mask is not None:
        nc[:H, :W] *= (torch.as_tensor(mask) != 0).to(torch.int64)      # a masked pixel walks no entry
    total = torch.zeros(P, dtype=dt)
    count = torch.zeros(P, dtype=torch.int64)
    largest = torch.zeros(P, dtype=dt)
    for ty in range(grid_y):
        for tx in range(grid_x):
            t = ty * grid_x + tx
            last = nc[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(-1)
            n = int(last.max())
            if n == 0:
                continue
            s = int(ranges[t, 0])
            assert s + n <= int(ranges[t, 1])
            ids = plist[s:s + n]
            sl = slot_of[ids]
            pxf = (tx * TILE + lx).to(dt)
            pyf = (ty * TILE + ly).to(dt)
            g_xy, g_con, g_o = xy[sl], conic[sl], opac[sl]
            dx = g_xy[:, 0:1] - pxf[None, :]
            dy = g_xy[:, 1:2] - pyf[None, :]
            power = -0.5 * (g_con[:, 0:1] * dx * dx + g_con[:, 2:3] * dy * dy) - g_con[:, 1:2] * dx * dy
            alpha = torch.clamp_max(g_o[:, None] * torch.exp(power), ALPHA_MAX)
            pos = torch.arange(n)[:, None]
            use = (power <= 0) & (alpha >= a_min) & (pos < last[None, :])
            one_minus = torch.where(use, 1.0 - alpha, torch.ones_like(alpha))
            cp = torch.cumprod(one_minus, dim=0)
            T_excl = torch.cat([torch.ones(1, TILE * TILE, dtype=dt), cp[:-1]], dim=0)
            w = torch.where(use, alpha * T_excl, torch.zeros_like(alpha))
            total.index_add_(0, ids, w.sum(dim=1))
            count.index_add_(0, ids, use.sum(dim=1))
            largest[ids] = torch.maximum(largest[ids], w.max(dim=1).values)      # a Gaussian is in a tile's list once
    return total, count, largest


def members_near(point_list, ranges, grid, where, P):
    """bool [P]: the Gaussians in the list of a tile that holds a pixel of ``where`` (bool [H,W])."""
    grid_x, grid_y = grid
    H, W = where.shape
    padded = torch.zeros(grid_y * TILE, grid_x * TILE, dtype=torch.bool)
    padded[:H, :W] = where
    tiles = padded.reshape(grid_y, TILE, grid_x, TILE).any(dim=3).any(dim=1).reshape(-1)
    plist = torch.from_numpy(np.asarray(point_list).astype(np.int64))
    out = torch.zeros(P, dtype=torch.bool)
    for t in torch.nonzero(tiles).reshape(-1).tolist():
        out[plist[int(ranges[t, 0]):int(ranges[t, 1])]] = True
    return out
