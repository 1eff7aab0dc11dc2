"""Plain-torch restatement of the depth-normal consistency loss, written from the definition and not
from the kernel: whole-array arithmetic, ``torch.cross``, and autograd for the three gradients -- no stencil loop, no
hand-derived backward.  ``dtype=torch.float64`` is the truth the GPU tests compare against; the same code in
``torch.float32`` gives them their bar (twice its own error against float64).  Also the inputs the host and GPU tests
share, and the fragility masks.
"""
import math

import numpy as np
import torch

MARGIN = 1e-4            # a decision within this relative distance of flipping is fragile
S_MIN = 1e-20
SHAPES = ((2, 5), (5, 2), (3, 3), (5, 7), (17, 33), (67, 131))
KINDS = ("plane", "sphere", "random")
TANFOV = (0.7, 0.45)     # tanfovx, tanfovy of every shared case


def focal(H, W, tanfovx, tanfovy):
    """fx, fy as the library forms them: from the float32 tangents, each rounded once to float32."""
    tx, ty = float(np.float32(tanfovx)), float(np.float32(tanfovy))
    return float(np.float32(W / (2.0 * tx))), float(np.float32(H / (2.0 * ty)))


def restate(depth, alpha, normal, tanfovx, tanfovy, alpha_min=0.5, dtype=torch.float64):
    """depth, alpha [1,H,W] (or [H,W]), normal [3,H,W] -> dict: loss (0-dim), n_valid (int), valid [H,W] bool,
    depth_normal [3,H,W], d_depth [H,W], d_alpha [H,W], d_normal [3,H,W], and the per-pixel margins of the two decisions,
    always float64: margin_alpha = alpha / alpha_min - 1 [H,W], margin_s = s / 1e-20 - 1 [H,W] (+inf where the pixel is
    not interior or a pixel of its stencil is not covered: s is not consulted there)."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    dep = depth.detach().reshape(H, W).to(dtype).clone().requires_grad_(True)
    alp = alpha.detach().reshape(H, W).to(dtype).clone().requires_grad_(True)
    nrm = normal.detach().reshape(3, H, W).to(dtype).clone().requires_grad_(True)
    fx, fy = focal(H, W, tanfovx, tanfovy)
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    a_min = torch.tensor(float(np.float32(alpha_min)), dtype=dtype)
    covered = alp.detach() >= a_min
    margin_alpha = alp.detach().double() / float(np.float32(alpha_min)) - 1.0
    margin_s = torch.full((H, W), math.inf, dtype=torch.float64)
    valid = torch.zeros(H, W, dtype=torch.bool)
    depth_normal = torch.zeros(3, H, W, dtype=dtype)
    loss = (dep.sum() + alp.sum() + nrm.sum()) * 0.0
    if H >= 3 and W >= 3:
        d = torch.where(covered, dep / torch.where(covered, alp, torch.ones_like(alp)), torch.zeros_like(dep))
        xs = torch.arange(W, dtype=dtype).view(1, W).expand(H, W)
        ys = torch.arange(H, dtype=dtype).view(H, 1).expand(H, W)
        P = torch.stack((d * (xs - cx) / fx, d * (ys - cy) / fy, d))                  # [3,H,W]
        tx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
        ty = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
        c = torch.cross(ty, tx, dim=0)
        s = (c * c).sum(dim=0)
        five = covered[1:-1, 1:-1] & covered[1:-1, 2:] & covered[1:-1, :-2] & covered[2:, 1:-1] & covered[:-2, 1:-1]
        ok = five & torch.isfinite(s.detach()) & (s.detach() > S_MIN)
        margin_s[1:-1, 1:-1] = torch.where(five, s.detach().double() / S_MIN - 1.0,
                                           torch.full_like(s.detach().double(), math.inf))
        n_d = c / torch.sqrt(torch.where(ok, s, torch.ones_like(s)))
        n_d = torch.where(ok.unsqueeze(0), n_d, torch.zeros_like(n_d))
        e = alp[1:-1, 1:-1] - (nrm[:, 1:-1, 1:-1] * n_d).sum(dim=0)
        loss = torch.where(ok, e, torch.zeros_like(e)).sum() / (H * W) + loss
        valid[1:-1, 1:-1] = ok
        depth_normal[:, 1:-1, 1:-1] = n_d.detach()
    loss.backward()
    return {"loss": loss.detach(), "n_valid": int(valid.sum()), "valid": valid, "depth_normal": depth_normal,
            "d_depth": dep.grad, "d_alpha": alp.grad, "d_normal": nrm.grad, "margin_alpha": margin_alpha,
            "margin_s": margin_s}


def fragile_mask(ref):
    """bool [H,W]: the pixels an output of which depends on a decision within MARGIN of flipping.  A pixel's coverage
    enters the validity of its four neighbours, and a pixel's validity the gradients of its four neighbours: the mask is
    the fragile decisions spread over the diamond of radius 2."""
    seed = (ref["margin_alpha"].abs() < MARGIN) | (ref["margin_s"].abs() < MARGIN)
    out = seed.clone()
    for _ in range(2):
        grown = out.clone()
        grown[1:, :] |= out[:-1, :]
        grown[:-1, :] |= out[1:, :]
        grown[:, 1:] |= out[:, :-1]
        grown[:, :-1] |= out[:, 1:]
        out = grown
    return out


# ---- shared inputs -----------------------------------------------------------------------------------------------------
PLANE_N = (0.35, -0.25)          # the plane z = z0 + a x + b y in view space: (a, b)
PLANE_Z0 = 4.0


def plane_normal():
    """The camera-facing unit normal of the plane z = z0 + a x + b y (view space, +z forward): (a, b, -1) normalised."""
    a, b = PLANE_N
    n = np.array([a, b, -1.0])
    return n / np.linalg.norm(n)


def plane_depth(H, W, tanfovx, tanfovy):
    """float64 [H,W]: the view depth of the plane along the ray of every pixel centre.  The ray of pixel (x, y) is
    ((x - cx) / fx, (y - cy) / fy, 1) t; on the plane t = z0 / (1 - a rx - b ry)."""
    fx, fy = focal(H, W, tanfovx, tanfovy)
    xs = (torch.arange(W, dtype=torch.float64).view(1, W) - (W - 1) / 2.0) / fx
    ys = (torch.arange(H, dtype=torch.float64).view(H, 1) - (H - 1) / 2.0) / fy
    a, b = PLANE_N
    return PLANE_Z0 / (1.0 - a * xs - b * ys)


def _unit(v):
    return v / v.norm(dim=0, keepdim=True)


def make_case(kind, H, W, seed=0):
    """(depth [1,H,W], alpha [1,H,W], normal [3,H,W]) float32 on the CPU, deterministic in (kind, H, W, seed).
    plane : the tilted plane under full coverage (alpha varies in [0.7, 1]); normal = alpha * a unit vector 0.3 rad or so
            off the plane's normal, so the loss is not a difference of near-equal numbers.
    sphere: a sphere over empty background: alpha exactly 0 outside, >= 0.6 inside: the covered test is never fragile and
            the valid mask has a ragged edge; normal = alpha * the sphere's camera-facing normal, perturbed.
    random: a smooth random depth field, alpha in [0.6, 1], normal = 0.8 alpha * a random unit vector per pixel, so
            every e is positive and the loss is no cancellation either."""
    g = torch.Generator().manual_seed(1000 * H + W + 7919 * seed + {"plane": 1, "sphere": 2, "random": 3}[kind])
    tanx, tany = TANFOV
    fx, fy = focal(H, W, tanx, tany)
    xs = (torch.arange(W, dtype=torch.float64).view(1, W).expand(H, W) - (W - 1) / 2.0) / fx
    ys = (torch.arange(H, dtype=torch.float64).view(H, 1).expand(H, W) - (H - 1) / 2.0) / fy
    u = torch.linspace(0, 1, W, dtype=torch.float64).view(1, W).expand(H, W)
    v = torch.linspace(0, 1, H, dtype=torch.float64).view(H, 1).expand(H, W)
    if kind == "plane":
        z = plane_depth(H, W, tanx, tany)
        alpha = 0.85 + 0.15 * torch.cos(3.0 * u + 2.0 * v)
        n = torch.tensor(plane_normal()).view(3, 1, 1).expand(3, H, W)
        n = _unit(n + 0.3 * torch.stack((torch.sin(5 * u), torch.cos(4 * v), 0.2 * u * v)))
        normal = alpha * n
    elif kind == "sphere":
        # centre (0.1, -0.05, 5) R: the ray r t hits at t = (r.c - sqrt((r.c)^2 - |r|^2 (|c|^2 - R^2))) / |r|^2
        c = torch.tensor([0.1, -0.05, 5.0], dtype=torch.float64).view(3, 1, 1)
        R = 5.0 * min(tanx, tany) * 0.75
        r = torch.stack((xs, ys, torch.ones_like(xs)))
        rc, rr = (r * c).sum(0), (r * r).sum(0)
        disc = rc * rc - rr * (float((c * c).sum()) - R * R)
        inside = disc > 0
        t = (rc - torch.sqrt(disc.clamp(min=0))) / rr
        z = torch.where(inside, t, torch.zeros_like(t))
        alpha = torch.where(inside, 0.8 + 0.2 * torch.cos(4.0 * u - 3.0 * v), torch.zeros_like(u))
        hit = r * t
        n = torch.where(inside, _unit(hit - c), torch.zeros_like(hit))
        n = torch.where(inside, _unit(n + 0.2 * torch.stack((torch.cos(6 * v), torch.sin(5 * u), 0.3 * u))),
                        torch.zeros_like(n))
        normal = alpha * n
    elif kind == "random":
        # a few low-frequency waves: smooth, no flat spot that would put s near its threshold
        z = 4.0 + 0.6 * xs - 0.4 * ys
        for _ in range(4):
            k = torch.rand(2, generator=g, dtype=torch.float64) * 6.0 + 1.0
            ph = torch.rand(1, generator=g, dtype=torch.float64) * 6.28
            z = z + 0.08 * torch.sin(k[0] * u + k[1] * v + ph)
        alpha = 0.8 + 0.2 * torch.sin(5.0 * u + float(torch.rand(1, generator=g)) * 6.28) * torch.cos(4.0 * v)
        n = _unit(torch.randn(3, H, W, generator=g, dtype=torch.float64))
        normal = 0.8 * alpha * n
    else:
        raise ValueError(kind)
    depth = (z * alpha).to(torch.float32).view(1, H, W)                  # the rendered map is sum w z = alpha * expected depth
    return depth, alpha.to(torch.float32).view(1, H, W), normal.to(torch.float32).contiguous()
