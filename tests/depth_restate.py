"""Restatement of the depth / inverse-depth / alpha maps over the oracle's public results (float64 or float32).

For a pixel, i runs over the entries of its tile's list that the oracle's colour pass composited: the first
``n_contrib[pixel]`` entries that pass the oracle's two skip tests (``power > 0``, ``alpha < 1/255``).  With
``w_i = alpha_i T_i`` and ``z_i`` the view-space depth:

    depth = sum w z,   invdepth = sum w / z,   alpha = sum w          (no background term)

Everything differentiable comes from ``pre["v_depth"]``, ``v_xy``, ``v_conic`` and ``v_opacity`` of
``oracle.rasterize_ref(..., want_aux=True)``, so autograd reaches the operator's inputs through the oracle's own
preprocess (its upstream-convention backward pieces included).  The 0.99 clamp passes the gradient on, as the oracle's
colour pass does.  Shared by tests/test_depth_host.py and tests/test_gpu_depth.py.
"""
import numpy as np
import torch

from oracle import rasterize_ref

TILE = 16
ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX = 0.99


def maps_from_lists(pre, point_list, ranges, n_contrib, settings):
    """-> maps [3,H,W] (depth, invdepth, alpha) in the dtype of ``pre``; ``point_list`` / ``ranges`` / ``n_contrib`` are
    the oracle's (held fixed: they are decisions, not differentiable quantities)."""
    dt = pre["v_xy"].dtype
    H, W = int(settings.image_height), int(settings.image_width)
    grid_x, grid_y = pre["grid"]
    slot_of = torch.full((int(pre["radii"].shape[0]),), -1, dtype=torch.int64)
    slot_of[pre["idx"]] = torch.arange(pre["idx"].shape[0])
    plist = torch.from_numpy(np.asarray(point_list).astype(np.int64))
    xy, conic, opac, depth = pre["v_xy"], pre["v_conic"], pre["v_opacity"], pre["v_depth"]
    lx = torch.arange(TILE).repeat(TILE)
    ly = torch.arange(TILE).repeat_interleave(TILE)
    a_min = torch.tensor(ALPHA_MIN, dtype=dt)
    nc = torch.zeros(grid_y * TILE, grid_x * TILE, dtype=torch.int64)
    nc[:H, :W] = n_contrib.to(torch.int64)
    zero_tile = torch.zeros(3, TILE, TILE, dtype=dt)
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
            sl = slot_of[plist[s:s + n]]
            pxf = (tx * TILE + lx).to(dt)
            pyf = (ty * TILE + ly).to(dt)
            g_xy, g_con, g_o, g_z = xy[sl], conic[sl], opac[sl], depth[sl]
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
            m = torch.stack([(w * g_z[:, None]).sum(0), (w / g_z[:, None]).sum(0), w.sum(0)], dim=0)
            row.append(m.reshape(3, TILE, TILE))
        rows.append(torch.cat(row, dim=2))
    return torch.cat(rows, dim=1)[:, :H, :W]


def maps_ref(means3D, means2D, opacities, settings, **kw):
    """The oracle's frame and its maps: -> (maps [3,H,W], color, radii, aux) with ``aux["margin"]`` etc."""
    color, radii, aux = rasterize_ref(means3D, means2D, opacities, settings, want_aux=True, want_margin=True, **kw)
    maps = maps_from_lists(aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], settings)
    return maps, color, radii, aux


def map_weights(H, W, seed=4711):
    """Fixed weights in (-1, 1) for the smooth loss ``sum(w * maps) / (3 H W)`` that mixes the three maps."""
    return torch.rand((3, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2.0 - 1.0


def maps_loss(maps, weights):
    return (maps * weights.to(maps.dtype).to(maps.device)).sum() / weights.numel()


# ---- the scene that takes every map's round loop past two full rounds ---------------------------------------------------
STACKED = dict(P=720, sh_degree=3, width=40, height=24, focal=30.0, scale=0.25, seed=5)
ROUND = 256      # list entries a map kernel stages per round


def stacked_scene():
    """720 faint Gaussians on the ray through the middle of tile (0, 0) of a 40 x 24 image (neither a multiple of 16).
    Every eighteenth is wide (40 pixels of standard deviation, opacity 0.04: composited on every pixel of the image, well
    above the alpha threshold); the others are narrow (1.5 pixels, opacity 0.006, scattered over the tile) and pass the
    alpha test on a few pixels each, so a pixel's list positions run far ahead of its composited entries.  T stays near
    0.2 at the end of the list: n_contrib is the whole list, and T falls through one half after some 17 wide entries,
    past list position 256, in steps of 0.02 (few pixels come within the fragility bound of one half)."""
    from conftest import small_scene
    model, cam, bg, _ = small_scene(**STACKED)
    P, f = STACKED["P"], STACKED["focal"]
    g = torch.Generator().manual_seed(11)
    z = 3.0 + 6.0 * torch.rand(P, generator=g)
    wide = torch.arange(P) % 18 == 0
    centre = torch.tensor([(8.0 - 0.5 * STACKED["width"]) / f, (8.0 - 0.5 * STACKED["height"]) / f])
    jitter = (torch.rand(P, 2, generator=g) * 2 - 1) * torch.where(wide, 2.0, 8.0)[:, None] / f
    xy = centre + jitter
    model._xyz = torch.stack([xy[:, 0] * z, xy[:, 1] * z, z], dim=1).contiguous()
    sigma = torch.where(wide, 40.0, 1.5) / f
    # mildly anisotropic (a sphere has no rotation gradient to compare); one Gaussian behind the camera is culled
    model._scaling = (torch.log(z * sigma)[:, None] + 0.25 * (torch.rand(P, 3, generator=g) * 2 - 1)).contiguous()
    model._xyz[1, 2] = -4.0
    model._opacity = torch.logit(torch.where(wide, 0.04, 0.006))[:, None].contiguous()
    return model, cam, bg


def assert_rounds_covered(aux, pos=None):
    """(a) a partial last tile row and column, (b) a pixel whose composited prefix needs a full, a full and a partial
    round, (c) with ``pos`` (the median's list positions): a pixel whose chosen entry lies past the first round."""
    H, W = aux["n_contrib"].shape
    assert H % TILE != 0 and W % TILE != 0, "the image must end in partial tiles on both axes"
    n = int(aux["n_contrib"].max())
    assert n > 2 * ROUND and n % ROUND != 0, f"the longest prefix ({n}) must take two full rounds and a partial one"
    if pos is not None:
        assert int(pos.max()) >= ROUND, f"no pixel's median entry lies past the first round (largest position {int(pos.max())})"
