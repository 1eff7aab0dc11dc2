"""Restatement of the absolute view-space gradient (AbsGS; csrc/abs_grad.hip) over the oracle's public
results (float64 or float32).

Not a hand-derived formula: per tile, every (entry, pixel) pair gets ITS OWN copy of the entry's screen position
(``xy[sl][:, None, :].expand(n, 256, 2).clone().requires_grad_()``), the tile's colour -- the entries the oracle's colour
pass composited (tests/depth_restate.py: the first ``n_contrib[pixel]`` entries that pass the oracle's two skip tests),
plus ``T_final * bg`` -- is composited from those copies, and autograd backpropagates the weighted-sum loss of
tests/grad_util.py.  The per-pair gradients ``d loss / d xy_(k,p)`` follow directly:

    abs[k]    = (0.5 W, 0.5 H) * sum_p | d loss / d xy_(k,p) |      what the kernel must produce
    signed[k] = (0.5 W, 0.5 H) * sum_p   d loss / d xy_(k,p)        the oracle's own means2D gradient (the proof)

``pre["v_xy"]``, ``v_conic``, ``v_opacity``, ``v_rgb``, ``point_list``, ``ranges`` and ``n_contrib`` are those of
``oracle.rasterize_ref(..., want_aux=True, want_margin=True)``, held fixed.  Shared by tests/test_abs_grad_host.py and
tests/test_gpu_abs_grad.py.
"""
import functools

import numpy as np
import torch

from conftest import make_settings, small_scene
from depth_restate import ALPHA_MAX, ALPHA_MIN, TILE, stacked_scene
from grad_util import MARGIN, linear_weights, oracle_operator_inputs, weighted_sum
from oracle import rasterize_ref

# the scenes of tests/test_gpu_features.py, and its cap on what the oracle alone leaves out of a comparison
SCENES = {
    "small": dict(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2),
    "big": dict(P=3000, sh_degree=3, width=320, height=176, focal=60.0, scale=0.5, seed=1),
}
MAX_LEFT_OUT = 0.05
BEHIND = [3, 17, 101]
BACKGROUNDS = {"black": (0.0, 0.0, 0.0), "coloured": (1.0, 0.5, 0.25)}


def scene(name):
    if name == "stacked":
        return stacked_scene()
    model, cam, bg, _ = small_scene(**SCENES["small" if name == "behind" else name])
    if name == "behind":
        model._xyz[3, 2] = -4.0          # behind the camera
        model._xyz[17, 2] = 0.1          # in front of it, inside the near plane (0.2)
        model._xyz[101] = torch.tensor([0.3, -0.2, -0.5])
    return model, cam, bg


def abs_grad_from_lists(pre, point_list, ranges, n_contrib, settings, bg, weights):
    """-> (abs [P,3], signed [P,3]) in the dtype of ``pre`` for the loss ``weighted_sum(colour, weights)``; z = 0.
    ``weights``: [3,H,W].  ``bg``: three numbers."""
    dt = pre["v_xy"].dtype
    H, W = int(settings.image_height), int(settings.image_width)
    P = int(pre["radii"].shape[0])
    grid_x, grid_y = pre["grid"]
    slot_of = torch.full((P,), -1, dtype=torch.int64)
    slot_of[pre["idx"]] = torch.arange(pre["idx"].shape[0])
    plist = torch.from_numpy(np.asarray(point_list).astype(np.int64))
    xy, conic, opac, rgb = (pre[k].detach() for k in ("v_xy", "v_conic", "v_opacity", "v_rgb"))
    bg = torch.tensor(tuple(float(v) for v in bg), dtype=dt)
    lx = torch.arange(TILE).repeat(TILE)
    ly = torch.arange(TILE).repeat_interleave(TILE)
    a_min = torch.tensor(ALPHA_MIN, dtype=dt)
    nc = torch.zeros(grid_y * TILE, grid_x * TILE, dtype=torch.int64)
    nc[:H, :W] = n_contrib.to(torch.int64)
    wpad = torch.zeros(3, grid_y * TILE, grid_x * TILE, dtype=dt)
    wpad[:, :H, :W] = weights.to(dt)
    out_abs = torch.zeros(P, 3, dtype=dt)
    out_signed = torch.zeros(P, 3, dtype=dt)
    scale = torch.tensor([0.5 * W, 0.5 * H], dtype=dt)
    for ty in range(grid_y):
        for tx in range(grid_x):
            t = ty * grid_x + tx
            ys, xs = slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE)
            last = nc[ys, xs].reshape(-1)
            n = int(last.max())
            if n == 0:
                continue
            s = int(ranges[t, 0])
            assert s + n <= int(ranges[t, 1])
            ids = plist[s:s + n]
            sl = slot_of[ids]
            pxf = (tx * TILE + lx).to(dt)
            pyf = (ty * TILE + ly).to(dt)
            pair_xy = xy[sl][:, None, :].expand(n, TILE * TILE, 2).clone().requires_grad_()
            g_con, g_o, g_rgb = conic[sl], opac[sl], rgb[sl]
            dx = pair_xy[:, :, 0] - pxf[None, :]
            dy = pair_xy[:, :, 1] - pyf[None, :]
            power = -0.5 * (g_con[:, 0:1] * dx * dx + g_con[:, 2:3] * dy * dy) - g_con[:, 1:2] * dx * dy
            raw = g_o[:, None] * torch.exp(power)
            alpha = raw + (torch.clamp_max(raw, ALPHA_MAX) - raw).detach()      # the clamp passes the gradient on
            pos = torch.arange(n)[:, None]
            use = (power <= 0) & (alpha >= a_min) & (pos < last[None, :])
            one_minus = torch.where(use, 1.0 - alpha, torch.ones_like(alpha))
            cp = torch.cumprod(one_minus, dim=0)
            T_excl = torch.cat([torch.ones(1, TILE * TILE, dtype=dt), cp[:-1]], dim=0)
            w = torch.where(use, alpha * T_excl, torch.zeros_like(alpha))
            colour = torch.einsum("np,nc->cp", w, g_rgb) + cp[-1][None, :] * bg[:, None]
            loss = weighted_sum(colour, wpad[:, ys, xs].reshape(3, -1)) * (TILE * TILE) / (H * W)   # / (3 H W) in all
            (g,) = torch.autograd.grad(loss, pair_xy)
            out_abs[:, :2].index_add_(0, ids, g.abs().sum(dim=1) * scale)
            out_signed[:, :2].index_add_(0, ids, g.sum(dim=1) * scale)
    return out_abs, out_signed


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """The oracle's frame of a scene in float64 and float32 (autograd graph kept), the robust / covered pixel sets of the
    float64 run and the share of covered pixels left out; computed once, never modified.  The lists, the margins and
    radii do not depend on the background: every background shares the frame."""
    model, cam, bg = scene(name)
    st = make_settings(cam, bg, 3)
    out = {"settings": st, "model": model, "cam": cam}
    for dt in (torch.float64, torch.float32):
        leaves, xyz, m2, op, kw = oracle_operator_inputs(model, dt)
        color, radii, aux = rasterize_ref(xyz, m2, op, st, want_aux=True, want_margin=True, **kw)
        out[dt] = (leaves, aux, color)
        if dt == torch.float64:
            out.update(robust=aux["margin"] > MARGIN, covered=aux["n_contrib"] > 0, radii=radii.clone(), aux=aux)
    out["left_out"] = float((out["covered"] & ~out["robust"]).sum()) / max(1, int(out["covered"].sum()))
    H, W = out["robust"].shape
    out["weights"] = linear_weights((3, H, W)) * out["robust"][None]      # zero on the threshold-fragile pixels
    return out


@functools.lru_cache(maxsize=None)
def reference(name, bg_name):
    """{dtype: (abs [P,3], signed [P,3])} of the restatement for the frame's weights and one of BACKGROUNDS."""
    fr = oracle_frame(name)
    out = {}
    for dt in (torch.float64, torch.float32):
        aux = fr[dt][1]
        out[dt] = abs_grad_from_lists(aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], fr["settings"],
                                      BACKGROUNDS[bg_name], fr["weights"])
    return out


def oracle_means2D_grad(name):
    """The float64 oracle's own autograd gradient of means2D for the frame's weights (its own background: black)."""
    fr = oracle_frame(name)
    leaves, _, color = fr[torch.float64]
    (g,) = torch.autograd.grad(weighted_sum(color, fr["weights"]), [leaves["means2D"]], retain_graph=True)
    return g.detach()
