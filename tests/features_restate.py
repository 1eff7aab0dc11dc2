"""Restatement of the feature maps over the oracle's public results (float64 or float32).

For a pixel, i runs over the entries of its tile's list that the oracle's colour pass composited (the entries of
tests/depth_restate.py: the first ``n_contrib[pixel]`` entries that pass the oracle's two skip tests).  With
``w_i = alpha_i T_i`` and ``F [P,C]`` the per-Gaussian rows:

    feat[c] = sum_i w_i F[id_i, c]          (no background term, no clamp)

The geometry comes from ``pre["v_xy"]``, ``v_conic`` and ``v_opacity`` of ``oracle.rasterize_ref(..., want_aux=True)``, so
autograd reaches the operator's inputs through the oracle's own preprocess; ``F`` is a differentiable input of its own.
Shared by tests/test_features_host.py and tests/test_gpu_features.py.
"""
import numpy as np
import torch

from depth_restate import ALPHA_MAX, ALPHA_MIN, TILE
from oracle import rasterize_ref


def feature_maps_from_lists(pre, point_list, ranges, n_contrib, settings, F):
    """-> maps [C,H,W] in the dtype of ``pre``; ``point_list`` / ``ranges`` / ``n_contrib`` are the oracle's (held fixed:
    they are decisions, not differentiable quantities).  ``F``: [P,C], cast to that dtype."""
    dt = pre["v_xy"].dtype
    F = F.to(dt)
    C = int(F.shape[1])
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
    zero_tile = torch.zeros(C, TILE, TILE, dtype=dt)
    rows = []
    for ty in range(grid_y):
        row = []
        for tx in range(grid_x):
            t = ty * grid_x + tx
            last = nc[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(-1)
            n = int(last.max())
            if n == 0:
                row.append(zero_tile)
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
            raw = g_o[:, None] * torch.exp(power)
            alpha = raw + (torch.clamp_max(raw, ALPHA_MAX) - raw).detach()
            pos = torch.arange(n)[:, None]
            use = (power <= 0) & (alpha >= a_min) & (pos < last[None, :])
            one_minus = torch.where(use, 1.0 - alpha, torch.ones_like(alpha))
            cp = torch.cumprod(one_minus, dim=0)
            T_excl = torch.cat([torch.ones(1, TILE * TILE, dtype=dt), cp[:-1]], dim=0)
            w = torch.where(use, alpha * T_excl, torch.zeros_like(alpha))
            # per channel the sum of depth_restate.maps_from_lists, term for term: (w * f[:, None]).sum(0)
            row.append((w[None, :, :] * F[ids].t()[:, :, None]).sum(1).reshape(C, TILE, TILE))
        rows.append(torch.cat(row, dim=2))
    return torch.cat(rows, dim=1)[:, :H, :W]


def features_ref(means3D, means2D, opacities, settings, F, **kw):
    """The oracle's frame and its feature maps: -> (feat [C,H,W], color, radii, aux) with ``aux["margin"]`` etc."""
    color, radii, aux = rasterize_ref(means3D, means2D, opacities, settings, want_aux=True, want_margin=True, **kw)
    feat = feature_maps_from_lists(aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], settings, F)
    return feat, color, radii, aux


def feature_rows(P, C, seed=97):
    """``F = randn(P, C)`` in float32 from a fixed seed."""
    return torch.randn(P, C, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def feature_weights(C, H, W, seed=4713):
    """Fixed weights in (-1, 1) for the smooth loss ``sum(w * feat) / (C H W)``."""
    return torch.rand((C, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2.0 - 1.0
