"""Restatement of the median-depth map and the Gaussian id map over the oracle's public results (float64 or float32).

For a pixel, i runs in list order over the entries of its tile's list that the oracle's colour pass composited (the
entries of tests/depth_restate.py: the first ``n_contrib[pixel]`` entries that pass the oracle's two skip tests).  With
``T_i`` the transmittance BEFORE entry i and ``z_i`` the view-space depth:

    k* = the last composited entry with T_i > 0.5,   median = z_{k*},   id = the Gaussian of entry k*

(2DGS: ``if (T > 0.5) { median_depth = depth; median_contributor = i; }``, before the blend).  A pixel without a
composited entry gets 0 / -1.  Stated literally: the exclusive cumulative product of ``1 - alpha`` over the composited
entries, the mask ``T > 0.5`` and the largest list position inside it; no early exit.  The median is gathered from
``pre["v_depth"]`` of ``oracle.rasterize_ref(..., want_aux=True)``, so autograd reaches means3D through the oracle's own
preprocess; the selection is a decision and carries no gradient.

The fragility of a pixel is ``min_i |T_i - 0.5|`` over its composited entries: a float32 and a float64 evaluation may pick
different entries where it is tiny.  Shared by tests/test_median_host.py and tests/test_gpu_median.py, which also share
the scenes and the per-scene reference below (computed once, never modified).
"""
import functools

import numpy as np
import torch

from conftest import make_settings, small_scene
from depth_restate import ALPHA_MAX, ALPHA_MIN, TILE, stacked_scene
from grad_util import MARGIN, oracle_operator_inputs
from oracle import rasterize_ref

FRAGILE = 1e-4          # float64 fragility below which a pixel is left out of the oracle comparisons
MAX_LEFT_OUT = 0.02     # of the covered pixels, per scene

SCENES = {
    "small": dict(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2),
    "big": dict(P=3000, sh_degree=3, width=320, height=176, focal=60.0, scale=0.5, seed=1),
}
BEHIND = (3, 17, 101)


def median_from_lists(pre, point_list, ranges, n_contrib, settings):
    """-> (median [1,H,W] in the dtype of ``pre``, id [H,W] int64 (-1: none), position in the tile's list [H,W] int64
    (-1: none), fragility [H,W] in the dtype of ``pre`` (inf: none))."""
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
    none = (torch.zeros(TILE, TILE, dtype=dt), torch.full((TILE, TILE), -1), torch.full((TILE, TILE), -1),
            torch.full((TILE, TILE), float("inf"), dtype=dt))
    rows = []
    for ty in range(grid_y):
        row = []
        for tx in range(grid_x):
            t = ty * grid_x + tx
            last = nc[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].reshape(-1)
            n = int(last.max())
            if n == 0:
                row.append(none)
                continue
            s = int(ranges[t, 0])
            assert s + n <= int(ranges[t, 1])
            ids = plist[s:s + n]
            sl = slot_of[ids]
            pxf = (tx * TILE + lx).to(dt)
            pyf = (ty * TILE + ly).to(dt)
            with torch.no_grad():       # the selection: decisions, not differentiable quantities
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
                cand = use & (T_excl > 0.5)
                k = torch.where(cand, pos.expand_as(cand), torch.full_like(cand, -1, dtype=torch.int64)).max(dim=0).values
                any_ = k >= 0
                frag = torch.where(use, (T_excl - 0.5).abs(), torch.full_like(T_excl, float("inf"))).min(dim=0).values
                kc = k.clamp_min(0)
            med = torch.where(any_, depth[sl][kc], torch.zeros(TILE * TILE, dtype=dt))      # differentiable in v_depth
            gid = torch.where(any_, ids[kc], torch.full_like(kc, -1))
            row.append((med.reshape(TILE, TILE), gid.reshape(TILE, TILE), k.reshape(TILE, TILE), frag.reshape(TILE, TILE)))
        rows.append(tuple(torch.cat([r[c] for r in row], dim=1) for c in range(4)))
    med, gid, k, frag = (torch.cat([r[c] for r in rows], dim=0)[:H, :W] for c in range(4))
    return med[None], gid, k, frag


def median_ref(means3D, means2D, opacities, settings, **kw):
    """The oracle's frame and its median: -> (median [1,H,W], id, position, fragility, radii, aux)."""
    _, radii, aux = rasterize_ref(means3D, means2D, opacities, settings, want_aux=True, want_margin=True, **kw)
    med, gid, k, frag = median_from_lists(aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], settings)
    return med, gid, k, frag, radii, aux


def median_weights(H, W, seed=4721):
    """Fixed weights in (-1, 1) for the loss ``sum(w * median) / (H W)``."""
    return torch.rand((1, H, W), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2.0 - 1.0


def median_loss(median, weights):
    return (median * weights.to(median.dtype).to(median.device)).sum() / weights.numel()


def scene(name):
    """small / big: the scenes of tests/test_gpu_depth.py; behind: its variant of small with Gaussians behind the camera and
    inside the near plane; faint: big with every raw opacity lowered by 4, so that rays stay above one half for long."""
    if name == "stacked":      # depth_restate.stacked_scene: the median entry lies past the first 256-entry round
        return stacked_scene()
    model, cam, bg, _ = small_scene(**SCENES["big" if name in ("big", "faint") else "small"])
    if name == "behind":
        model._xyz[3, 2] = -4.0          # behind the camera
        model._xyz[17, 2] = 0.1          # in front of it, inside the near plane (0.2)
        model._xyz[101] = torch.tensor([0.3, -0.2, -0.5])
    if name == "faint":
        model._opacity -= 4.0
    return model, cam, bg


@functools.lru_cache(maxsize=None)
def reference(name, use_cov=False):
    """float64 and float32 restatement of a scene: median, id, position, the kept pixels (oracle margin above
    grad_util.MARGIN and float64 fragility of at least FRAGILE), the loss weights (zero on the pixels left out) and the
    gradients of the loss for every leaf; the share left out is asserted against MAX_LEFT_OUT here, from the reference
    alone.  Computed once per scene and shared, never modified."""
    model, cam, bg = scene(name)
    st = make_settings(cam, bg, 3)
    out = {}
    for dt in (torch.float64, torch.float32):
        leaves, xyz, m2, op, kw = oracle_operator_inputs(model, dt, use_cov=use_cov)
        med, gid, k, frag, radii, aux = median_ref(xyz, m2, op, st, **kw)
        if dt == torch.float64:
            covered = aux["n_contrib"] > 0
            keep = (aux["margin"] > MARGIN) & (frag >= FRAGILE)
            weights = median_weights(*med.shape[1:]) * keep[None]
            out.update(covered=covered, keep=keep, weights=weights, radii=radii.clone(), aux=aux, frag=frag,
                       v_depth=aux["pre"]["v_depth"].detach().clone(), slots=aux["pre"]["idx"].clone())
        median_loss(med, weights).backward()
        grads = {n: (None if t.grad is None else t.grad.detach().clone()) for n, t in leaves.items()}
        out[dt] = dict(median=med.detach(), id=gid, pos=k, grads=grads)
    n_cov = int(out["covered"].sum())
    left_out = float((out["covered"] & ~out["keep"]).sum()) / max(1, n_cov)
    same = out[torch.float64]["id"] == out[torch.float32]["id"]
    print(f"[median] scene {name}: {n_cov} covered pixels, share left out of the comparison {left_out:.4f}; float32 and "
          f"float64 restatements disagree on the id of {int((~same & out['covered']).sum())} covered pixels "
          f"({int((~same & out['keep']).sum())} kept ones)")
    assert left_out <= MAX_LEFT_OUT, f"scene {name}: the reference alone leaves out {left_out:.4f} of the covered pixels"
    assert bool(same[out["keep"]].all()), f"scene {name}: the two restatements disagree on a kept pixel"
    out["left_out"] = left_out
    return out
