"""torch restatement of the multi-view geometric consistency loss (csrc/mvs_loss.hip; mvs.multi_view_geo_loss; DESIGN.md
§7.22), written from the definition on the CPU.  The round trip is that of ``mvs_restate.consistency``; the bilinear
value is formed over four explicitly indexed taps, so autograd gives the gradient to the reference depth and, as a
scatter-add over the taps, to the source depth.  ``dtype=torch.float64`` is the truth the GPU tests compare against;
``dtype=torch.float32`` runs the same operations in the stated order rounded one by one and gives the tests their bar
(twice its own error against float64).  Both start from the same float32 inputs.  Also the scene the host and GPU tests
share.
"""
import math

import numpy as np
import torch

import mvs_restate as R

MARGIN = R.MARGIN
PHI_MIN = 1e-3         # below this the direction (du, dv) / phi has no float32 digits left: fragile
KINDS = ("behind", "outside", "hole", "back_behind", "pixel", "depth", "ok")
E_MAX = math.exp(-1.0)                 # max of phi exp(-phi): what one pixel can add to the raw sum


def _through(M, x, y, z):
    col = lambda c: ((x * M[0, c] + y * M[1, c]) + z * M[2, c]) + M[3, c]      # noqa: E731
    return col(0), col(1), col(2)


def loss(depth, fx, fy, row, pix_max=1.0, depth_thresh=None, dtype=torch.float64, round_inputs=True):
    """One (reference, source) pair; ``row`` is a row of ``mvs_restate.source_rows``.  -> dict with
    ``value`` (raw / max(n, 1)), ``raw``, ``n`` (valid pixels), ``grad_ref [H,W]`` and ``grad_src [Hs,Ws]`` (unit
    gradients of raw, numpy, of ``dtype``), ``valid`` bool [H,W], ``phi`` [H,W] (NaN where the trip did not get there),
    ``kind`` int8 [H,W] indexing KINDS (-1 without depth), ``fragile`` bool [H,W] (meaningful at float64), ``tainted``
    bool [Hs,Ws]: source texels a fragile pixel may feed, ``feeds`` int [Hs,Ws]: valid pixels feeding each texel.
    ``round_inputs=False`` takes the two depth maps as float64 (finite differences step them below float32's spacing)."""
    t = lambda v: torch.tensor(float(np.float32(v)), dtype=dtype)              # noqa: E731
    as_input = (lambda m: np.asarray(m, np.float32)) if round_inputs else (lambda m: np.asarray(m, np.float64))
    d_map = torch.tensor(as_input(depth), dtype=dtype, requires_grad=True)
    s_map = torch.tensor(as_input(row["depth"]), dtype=dtype, requires_grad=True)
    A, B = (torch.tensor(np.asarray(row[k], np.float32), dtype=dtype) for k in ("A", "B"))
    H, W = d_map.shape
    Hs, Ws = int(row["H"]), int(row["W"])
    fx, fy, fxs, fys, pix_max = t(fx), t(fy), t(row["fx"]), t(row["fy"]), t(pix_max)
    one, half = torch.tensor(1.0, dtype=dtype), torch.tensor(0.5, dtype=dtype)
    cx, cy = (torch.tensor(float(W), dtype=dtype) - one) * half, (torch.tensor(float(H), dtype=dtype) - one) * half
    cxs, cys = (torch.tensor(float(Ws), dtype=dtype) - one) * half, (torch.tensor(float(Hs), dtype=dtype) - one) * half

    kind = np.full((H, W), -1, np.int8)
    fragile = np.zeros((H, W), bool)
    phi_map = np.full((H, W), np.nan)
    tainted = np.zeros((Hs, Ws), bool)
    feeds = np.zeros((Hs, Ws), np.int64)

    iy, ix = torch.nonzero(d_map.detach() > 0, as_tuple=True)                  # the live pixels, compacted gate by gate
    live = {"iy": iy, "ix": ix}

    def gate(ok, name, **arrays):
        """Pixels failing ``ok`` get ``name``; every array (and the live indices) keeps the passing ones."""
        bad = ~ok
        kind[live["iy"][bad].numpy(), live["ix"][bad].numpy()] = KINDS.index(name)
        live["iy"], live["ix"] = live["iy"][ok], live["ix"][ok]
        return [a[ok] for a in arrays.values()]

    def mark(mask):
        fragile[live["iy"][mask].numpy(), live["ix"][mask].numpy()] = True

    px, py = ix.to(dtype), iy.to(dtype)
    d = d_map[iy, ix]
    xr, yr = ((px - cx) * d) / fx, ((py - cy) * d) / fy
    xs, ys, zs = _through(A, xr, yr, d)
    mark((zs.detach() - 0.2).abs() < MARGIN)
    px, py, d, xs, ys, zs = gate(zs.detach() > 0.2, "behind", px=px, py=py, d=d, xs=xs, ys=ys, zs=zs)
    us, vs = (fxs * xs) / zs + cxs, (fys * ys) / zs + cys
    x0, y0 = torch.floor(us.detach()), torch.floor(vs.detach())
    ax, ay = us - x0, vs - y0
    # a cell border: the footprint or a tap may flip there, and the bilinear slope jumps (the value does not)
    near = lambda a: (a.detach() < MARGIN) | (1 - a.detach() < MARGIN)         # noqa: E731
    edge = near(ax) | near(ay)
    mark(edge)
    for dy in range(-1, 3):                                                    # what such a pixel may feed
        for dx in range(-1, 3):
            ty, tx = (y0[edge] + dy).long(), (x0[edge] + dx).long()
            ok = (ty >= 0) & (ty < Hs) & (tx >= 0) & (tx < Ws)
            tainted[ty[ok].numpy(), tx[ok].numpy()] = True
    inside = (x0 >= 0) & (x0 + 1 <= Ws - 1) & (y0 >= 0) & (y0 + 1 <= Hs - 1)
    px, py, d, us, vs, x0, y0, ax, ay = gate(inside, "outside", px=px, py=py, d=d, us=us, vs=vs, x0=x0, y0=y0, ax=ax, ay=ay)
    xi, yi = x0.long(), y0.long()
    d00, d10, d01, d11 = s_map[yi, xi], s_map[yi, xi + 1], s_map[yi + 1, xi], s_map[yi + 1, xi + 1]
    taps = torch.stack((d00, d10, d01, d11)).detach()
    mark(((taps > 0) & (taps < MARGIN)).any(dim=0))
    px, py, d, us, vs, xi, yi, ax, ay, d00, d10, d01, d11 = gate(
        (taps > 0).all(dim=0), "hole", px=px, py=py, d=d, us=us, vs=vs, xi=xi, yi=yi, ax=ax, ay=ay, d00=d00, d10=d10,
        d01=d01, d11=d11)
    ds = (d00 * (1 - ax) + d10 * ax) * (1 - ay) + (d01 * (1 - ax) + d11 * ax) * ay
    xb0, yb0 = ((us - cxs) * ds) / fxs, ((vs - cys) * ds) / fys
    xb, yb, zb = _through(B, xb0, yb0, ds)
    mark((zb.detach() - 0.2).abs() < MARGIN)
    px, py, d, xi, yi, xb, yb, zb = gate(zb.detach() > 0.2, "back_behind", px=px, py=py, d=d, xi=xi, yi=yi, xb=xb, yb=yb,
                                         zb=zb)
    ub, vb = (fx * xb) / zb + cx, (fy * yb) / zb + cy
    du, dv = ub - px, vb - py
    e2 = du * du + dv * dv
    phi_d = torch.sqrt(e2.detach())
    phi_map[live["iy"].numpy(), live["ix"].numpy()] = phi_d.double().numpy()
    mark(((phi_d - pix_max).abs() < MARGIN) | (phi_d < PHI_MIN))
    gap = (zb - d).abs().detach()
    pix_ok = phi_d < pix_max
    depth_ok = torch.ones_like(pix_ok)
    if depth_thresh is not None:
        dt = t(depth_thresh)
        mark(pix_ok & ((gap / d.detach() - dt).abs() < MARGIN))      # past pix_max the depth test decides nothing
        depth_ok = gap < dt * d.detach()
    here_y, here_x = live["iy"], live["ix"]
    touch = fragile[here_y.numpy(), here_x.numpy()]                            # fragile pixels that got this far
    for dy in range(-1, 3):
        for dx in range(-1, 3):
            ty, tx = (yi[touch] + dy), (xi[touch] + dx)
            ok = (ty >= 0) & (ty < Hs) & (tx >= 0) & (tx < Ws)
            tainted[ty[ok].numpy(), tx[ok].numpy()] = True
    kind[here_y[~pix_ok].numpy(), here_x[~pix_ok].numpy()] = KINDS.index("pixel")
    only_depth = pix_ok & ~depth_ok
    kind[here_y[only_depth].numpy(), here_x[only_depth].numpy()] = KINDS.index("depth")
    ok = pix_ok & depth_ok
    kind[here_y[ok].numpy(), here_x[ok].numpy()] = KINDS.index("ok")
    valid = np.zeros((H, W), bool)
    valid[here_y[ok].numpy(), here_x[ok].numpy()] = True
    for dy in (0, 1):
        for dx in (0, 1):
            np.add.at(feeds, ((yi[ok] + dy).numpy(), (xi[ok] + dx).numpy()), 1)
    sel = ok & (e2.detach() > 0)                                               # phi == 0: value 0, gradient 0
    phi = torch.sqrt(e2[sel])
    w = torch.exp(-phi).detach()
    raw = (w * phi).sum()
    n = int(ok.sum())
    if sel.any():
        raw.backward()
    zeros = lambda m: torch.zeros_like(m).numpy()                              # noqa: E731
    return {"value": float(raw.detach().double()) / max(n, 1) if dtype == torch.float64
            else float((raw.detach() / torch.tensor(float(max(n, 1)), dtype=dtype)).double()),
            "raw": float(raw.detach().double()), "n": n,
            "grad_ref": zeros(d_map) if d_map.grad is None else d_map.grad.numpy(),
            "grad_src": zeros(s_map) if s_map.grad is None else s_map.grad.numpy(),
            "valid": valid, "phi": phi_map, "kind": kind, "fragile": fragile, "tainted": tainted, "feeds": feeds}


def value_slack(ref64):
    """What the fragile pixels may move the value by: each adds at most E_MAX to the raw sum and one to the count, so
    ``|raw' / n' - raw / n| <= F (E_MAX + value) / (n - F)``."""
    F = int((ref64["fragile"] & (ref64["kind"] >= 0)).sum())
    return F * (E_MAX + ref64["value"]) / max(ref64["n"] - F, 1)


# ---- the scene ---------------------------------------------------------------------------------------------------------
PIX_MAX, DEPTH_THRESH = 1.0, 0.004
REF_FX, REF_FY = 44.0, 40.0
SRC_W, SRC_H, SRC_FX, SRC_FY = 48, 40, 38.0, 42.0
SRC_POS, SRC_TARGET = np.array([0.8, -0.5, 3.4]), np.array([-0.6, 0.0, 4.0])


def scene():
    """-> (reference camera, its depth [37,70], source camera, its depth [40,48]).  The plane and sphere of
    ``mvs_restate``; the reference is its 70 x 37 camera at the origin (two x-tiles, ragged on both axes).  The source, 48
    x 40 with its own focal lengths, stands close to the plane and looks along it, so that the plane's right-hand end lies
    behind it and much of the reference lies outside its image.  Its depth is scaled by a smooth field 1 + 0.07 sin sin,
    which spreads phi over (0, pix_max) and beyond; a rectangle of it is zeroed (holes)."""
    ref = R.Cam(np.eye(3), np.zeros(3), R.REF_W, R.REF_H, REF_FX, REF_FY)
    src = R.look_at(SRC_POS, SRC_TARGET, SRC_W, SRC_H, SRC_FX, SRC_FY)
    depth, _ = R.render_depth(ref)
    sdepth, _ = R.render_depth(src)
    yy, xx = np.meshgrid(np.arange(SRC_H), np.arange(SRC_W), indexing="ij")
    sdepth = (sdepth.astype(np.float64) * (1.0 + 0.07 * np.sin(xx / 5.0) * np.sin(yy / 4.0 + 0.5))).astype(np.float32)
    sdepth[19:27, 18:26] = 0.0
    depth[3:6, 60:66] = 0.0                                                # reference pixels without depth
    return ref, depth, src, sdepth


def exact_case():
    """Dyadic cameras and fronto-parallel maps that disagree: every operation of the round trip is exact in float32.
    Reference 70 x 37, f = 64, at the origin, depth d = 4; source 48 x 40, f = 32, p_src = p_ref + (t, 0, 0) with t = 1/16,
    depth D = 8 everywhere.  With k = px - 34.5: us = k / 2 + 32 t / d + 23.5 = px / 2 + 6.75 (ax = 3/4 at even px, 1/4 at odd),
    vs = py / 2 + 10.5 (ay = 1/2 at even py, 0 at odd); every footprint lies inside the source, so all 2590 pixels are
    valid; ub = k + 64 t / d - 64 t / D + 34.5, so du = 64 t (1 / d - 1 / D) = 1/2, dv = 0, phi = 1/2 everywhere.
    d du / d d = -64 t / d^2 = -1/4 and d du / d D = 64 t / D^2 = 1/16: the unit gradient to every reference pixel is
    -exp(-1/2) / 4, and a source texel whose feeding pixels all exist collects bilinear weights 2 x 2 = 4: exp(-1/2) / 4.
    -> (ref camera, depth, source camera, source depth)."""
    ref = R.Cam(np.eye(3), np.zeros(3), 70, 37, 64.0, 64.0)
    src = R.Cam(np.eye(3), np.array([-0.0625, 0.0, 0.0]), 48, 40, 32.0, 32.0)
    return ref, np.full((37, 70), 4.0, np.float32), src, np.full((40, 48), 8.0, np.float32)
