"""torch restatement of the multi-view photometric (NCC) loss (csrc/mvs_ncc.hip; mvs.multi_view_ncc_loss; DESIGN.md
§7.23), written from the definition on the CPU, with the bilinear reads over explicitly indexed taps.
``dtype=torch.float64`` with autograd is the truth the GPU tests compare against; ``dtype=torch.float32`` runs the
operations of the kernel's header comment in its order, rounded one by one, the gradient in its forward-mode form
(``grad="stated"``), and gives the tests their bars (twice its own error against float64).  Both start from the same
float32 inputs.  Also the analytic scene the host and GPU tests share.
"""
import math

import numpy as np
import torch

import mvs_restate as R

MARGIN = R.MARGIN
KINDS = ("patch", "trip", "pix_max", "grazing", "tap", "ncc", "counted")


def _through(M, x, y, z):
    col = lambda c: ((x * M[0, c] + y * M[1, c]) + z * M[2, c]) + M[3, c]      # noqa: E731
    return col(0), col(1), col(2)


def _tap(A, fxs, fys, cxs, cys, Ws, Hs, sg, mx, my, mz, qx, qy):
    """One tap of the definition for vectors of pixels -> (ok, fragile, S, g): ``ok`` every gate passes, ``fragile`` a
    decision of this tap (k, Y_z, a cell border) lies within MARGIN of flipping, S the bilinear value of ``sg`` and g with
    d S / d m = g (qx, qy, 1).  S and g are meaningful (and finite) where ok; elsewhere the indices are clamped."""
    k = (mx * qx + my * qy) + mz
    Yx = ((qx * A[0, 0] + qy * A[1, 0]) + A[2, 0]) + k * A[3, 0]
    Yy = ((qx * A[0, 1] + qy * A[1, 1]) + A[2, 1]) + k * A[3, 1]
    Yz = ((qx * A[0, 2] + qy * A[1, 2]) + A[2, 2]) + k * A[3, 2]
    front = (k.detach() > 0) & (Yz.detach() > 0)
    fragile = (k.detach().abs() < MARGIN) | (Yz.detach().abs() < MARGIN)
    Yz_safe = torch.where(front, Yz, torch.ones_like(Yz))
    ix, iy = Yx / Yz_safe, Yy / Yz_safe
    u, v = fxs * ix + cxs, fys * iy + cys
    x0, y0 = torch.floor(u.detach()), torch.floor(v.detach())
    inside = (x0 >= 0) & (x0 + 1 <= Ws - 1) & (y0 >= 0) & (y0 + 1 <= Hs - 1)
    ax, ay = u - x0, v - y0
    near = lambda a: (a.detach() < MARGIN) | (1 - a.detach() < MARGIN)         # noqa: E731
    # a cell border: the footprint may flip there (the image border is one), and the bilinear slope jumps
    reach = (x0 >= -1) & (x0 <= Ws - 1) & (y0 >= -1) & (y0 <= Hs - 1)
    fragile = fragile | (front & reach & (near(ax) | near(ay)))
    ok = front & inside
    xi = torch.where(ok, x0, torch.zeros_like(x0)).long()
    yi = torch.where(ok, y0, torch.zeros_like(y0)).long()
    s00, s10, s01, s11 = sg[yi, xi], sg[yi, xi + 1], sg[yi + 1, xi], sg[yi + 1, xi + 1]
    bx, by = 1 - ax, 1 - ay
    top, bot = s00 * bx + s10 * ax, s01 * bx + s11 * ax
    S = top * by + bot * ay
    Sx, Sy = (s10 - s00) * by + (s11 - s01) * ay, bot - top
    hu = (fxs * (A[3, 0] - ix * A[3, 2])) / Yz_safe
    hv = (fys * (A[3, 1] - iy * A[3, 2])) / Yz_safe
    return ok, fragile, S, Sx * hu + Sy * hv


def loss(depth, normal, gray, fx, fy, row, src_gray, radius=3, pix_max=1.0, ncc_max=0.9, min_cos=0.05,
         dtype=torch.float64, pixels=None, round_inputs=True, grad=None):
    """One (reference, source) pair; ``row`` is a row of ``mvs_restate.source_rows`` (its depth: the source's).
    ``pixels``: flat indices to evaluate (None: all).  ``grad``: "autograd" (the default at float64) or "stated" (the
    default at float32: the kernel's forward-mode accumulators and chain, in its association).  -> dict with ``value``
    (raw / max(n, 1)), ``raw``, ``n``, ``grad_depth [H,W]`` and ``grad_normal [3,H,W]`` (unit gradients of raw, numpy, of
    ``dtype``), ``counted`` bool [H,W], ``ncc`` and ``w`` [H,W] (NaN where the pixel did not get there), ``kind`` int8
    [H,W] indexing KINDS (-1: no depth, or not evaluated), ``fragile`` bool [H,W] (meaningful at float64).
    ``round_inputs=False`` takes depth and normal as float64 (finite differences step below float32's spacing)."""
    if grad is None:
        grad = "autograd" if dtype == torch.float64 else "stated"
    t = lambda v: torch.tensor(float(np.float32(v)), dtype=dtype)              # noqa: E731
    as_input = (lambda m: np.asarray(m, np.float32)) if round_inputs else (lambda m: np.asarray(m, np.float64))
    d_map = torch.tensor(as_input(depth), dtype=dtype, requires_grad=grad == "autograd")
    n_map = torch.tensor(as_input(normal), dtype=dtype, requires_grad=grad == "autograd")
    g_map = torch.tensor(np.asarray(gray, np.float32), dtype=dtype)
    sg = torch.tensor(np.asarray(src_gray, np.float32), dtype=dtype)
    s_map = torch.tensor(np.asarray(row["depth"], np.float32), dtype=dtype)
    A, B = (torch.tensor(np.asarray(row[k], np.float32), dtype=dtype) for k in ("A", "B"))
    H, W = d_map.shape
    Hs, Ws = int(row["H"]), int(row["W"])
    assert tuple(sg.shape) == (Hs, Ws) and tuple(n_map.shape) == (3, H, W) and tuple(g_map.shape) == (H, W)
    fx, fy, fxs, fys = t(fx), t(fy), t(row["fx"]), t(row["fy"])
    pix_max, ncc_max, min_cos = t(pix_max), t(ncc_max), t(min_cos)
    one, half = torch.tensor(1.0, dtype=dtype), torch.tensor(0.5, dtype=dtype)
    cx, cy = (torch.tensor(float(W), dtype=dtype) - one) * half, (torch.tensor(float(H), dtype=dtype) - one) * half
    cxs, cys = (torch.tensor(float(Ws), dtype=dtype) - one) * half, (torch.tensor(float(Hs), dtype=dtype) - one) * half
    Rr = int(radius)

    kind = np.full((H, W), -1, np.int8)
    fragile = np.zeros((H, W), bool)
    ncc_map, w_map = np.full((H, W), np.nan), np.full((H, W), np.nan)
    counted = np.zeros((H, W), bool)

    has = d_map.detach() > 0
    if pixels is not None:
        chosen = torch.zeros(H * W, dtype=torch.bool)
        idx = torch.as_tensor(np.asarray(pixels, np.int64))
        chosen[idx[(idx >= 0) & (idx < H * W)]] = True
        has = has & chosen.view(H, W)
    iy, ix = torch.nonzero(has, as_tuple=True)
    live = {"iy": iy, "ix": ix}

    def gate(ok, name, *arrays):
        bad = ~ok
        kind[live["iy"][bad].numpy(), live["ix"][bad].numpy()] = KINDS.index(name)
        live["iy"], live["ix"] = live["iy"][ok], live["ix"][ok]
        return [a[ok] for a in arrays]

    def mark(mask):
        fragile[live["iy"][mask].numpy(), live["ix"][mask].numpy()] = True

    # the patch lies inside the reference image (integers: never fragile)
    gate((ix - Rr >= 0) & (ix + Rr <= W - 1) & (iy - Rr >= 0) & (iy + Rr <= H - 1), "patch")
    iy, ix = live["iy"], live["ix"]
    px, py = ix.to(dtype), iy.to(dtype)

    # ---- the geometric gate and the weight: the round trip of mvs_loss_restate, without gradient -----------------------
    with torch.no_grad():
        d = d_map[iy, ix]
        xr, yr = ((px - cx) * d) / fx, ((py - cy) * d) / fy
        xs, ys, zs = _through(A, xr, yr, d)
        mark((zs - 0.2).abs() < MARGIN)
        px, py, xs, ys, zs = gate(zs > 0.2, "trip", px, py, xs, ys, zs)
        us, vs = (fxs * xs) / zs + cxs, (fys * ys) / zs + cys
        x0, y0 = torch.floor(us), torch.floor(vs)
        ax, ay = us - x0, vs - y0
        near = lambda a: (a < MARGIN) | (1 - a < MARGIN)                       # noqa: E731
        mark(near(ax) | near(ay))
        inside = (x0 >= 0) & (x0 + 1 <= Ws - 1) & (y0 >= 0) & (y0 + 1 <= Hs - 1)
        px, py, us, vs, x0, y0, ax, ay = gate(inside, "trip", px, py, us, vs, x0, y0, ax, ay)
        xi, yi = x0.long(), y0.long()
        d00, d10, d01, d11 = s_map[yi, xi], s_map[yi, xi + 1], s_map[yi + 1, xi], s_map[yi + 1, xi + 1]
        four = torch.stack((d00, d10, d01, d11))
        mark(((four > 0) & (four < MARGIN)).any(dim=0))
        px, py, us, vs, ax, ay, d00, d10, d01, d11 = gate((four > 0).all(dim=0), "trip", px, py, us, vs, ax, ay, d00, d10,
                                                          d01, d11)
        dsrc = (d00 * (1 - ax) + d10 * ax) * (1 - ay) + (d01 * (1 - ax) + d11 * ax) * ay
        xb0, yb0 = ((us - cxs) * dsrc) / fxs, ((vs - cys) * dsrc) / fys
        xb, yb, zb = _through(B, xb0, yb0, dsrc)
        mark((zb - 0.2).abs() < MARGIN)
        px, py, xb, yb, zb = gate(zb > 0.2, "trip", px, py, xb, yb, zb)
        ub, vb = (fx * xb) / zb + cx, (fy * yb) / zb + cy
        du, dv = ub - px, vb - py
        phi = torch.sqrt(du * du + dv * dv)
        mark((phi - pix_max).abs() < MARGIN)
        px, py, phi = gate(phi < pix_max, "pix_max", px, py, phi)
        w = torch.exp(-phi)

    # ---- the plane --------------------------------------------------------------------------------------------------------
    def plane(iy, ix, px, py):
        d = d_map[iy, ix]
        Nx, Ny, Nz = n_map[0, iy, ix], n_map[1, iy, ix], n_map[2, iy, ix]
        rx, ry = (px - cx) / fx, (py - cy) / fy
        nn = (Nx * Nx + Ny * Ny) + Nz * Nz
        s = (Nx * rx + Ny * ry) + Nz
        rr = (rx * rx + ry * ry) + 1
        return d, (Nx, Ny, Nz), rx, ry, nn, s, rr

    with torch.no_grad():
        d, N, rx, ry, nn, s, rr = plane(live["iy"], live["ix"], px, py)
        norm = torch.sqrt(nn * rr)
        mark(((s.abs() - min_cos * norm).abs() < MARGIN * norm) | ((nn - 1e-12).abs() < 1e-13))
        px, py, w = gate((nn > 1e-12) & (s.abs() >= min_cos * norm), "grazing", px, py, w)

    offsets = [(i, j) for j in range(-Rr, Rr + 1) for i in range(-Rr, Rr + 1)]       # j outer, i inner: the kernel's order
    tap_args = (A, fxs, fys, cxs, cys, Ws, Hs, sg)

    # pass 1, without gradient: which pixels keep every tap, and how surely
    with torch.no_grad():
        d, N, rx, ry, nn, s, rr = plane(live["iy"], live["ix"], px, py)
        dsr = d * s
        mx, my, mz = N[0] / dsr, N[1] / dsr, N[2] / dsr
        all_ok = torch.ones_like(px, dtype=torch.bool)
        any_fragile = torch.zeros_like(all_ok)
        sure_fail = torch.zeros_like(all_ok)
        for i, j in [(0, 0)] + offsets:
            ok, fr, _, _ = _tap(*tap_args, mx, my, mz, ((px + i) - cx) / fx, ((py + j) - cy) / fy)
            all_ok &= ok
            any_fragile |= fr
            sure_fail |= ~ok & ~fr
        mark((all_ok & any_fragile) | (~all_ok & ~sure_fail))
        px, py, w = gate(all_ok, "tap", px, py, w)

    # pass 2, on the pixels that keep every tap: the sums
    iy, ix = live["iy"], live["ix"]
    d, N, rx, ry, nn, s, rr = plane(iy, ix, px, py)
    dsr = d * s
    mx, my, mz = N[0] / dsr, N[1] / dsr, N[2] / dsr
    _, _, Sc, _ = _tap(*tap_args, mx, my, mz, rx, ry)
    Sc = Sc.detach()
    Rp = g_map[iy, ix]
    z = torch.zeros_like(px)
    sR, sS, sRR, sSS, sRS = z, z, z, z, z
    D, SD, RD = [z, z, z], [z, z, z], [z, z, z]
    for i, j in offsets:
        qx, qy = ((px + i) - cx) / fx, ((py + j) - cy) / fy
        _, _, S, g = _tap(*tap_args, mx, my, mz, qx, qy)
        a, b = g_map[iy + j, ix + i] - Rp, S - Sc
        sR, sS, sRR, sSS, sRS = sR + a, sS + b, sRR + a * a, sSS + b * b, sRS + a * b
        if grad == "stated":
            gc = (g * qx, g * qy, g)
            for c in range(3):
                D[c], SD[c], RD[c] = D[c] + gc[c], SD[c] + b * gc[c], RD[c] + a * gc[c]
    T = torch.tensor(float(len(offsets)), dtype=dtype)
    cross, vr, vs_ = sRS - (sR * sS) / T, sRR - (sR * sR) / T, sSS - (sS * sS) / T
    den = vr * vs_ + torch.tensor(float(np.float32(1e-8)), dtype=dtype)
    cc = (cross * cross) / den
    tt = 1 - cc
    ncc = torch.clamp(tt, 0.0, 2.0)
    nd, td = ncc.detach(), tt.detach()
    mark(((nd - ncc_max).abs() < MARGIN) | (td.abs() < MARGIN) | ((td - 2).abs() < MARGIN))
    ok = nd < ncc_max
    ncc_map[iy.numpy(), ix.numpy()] = nd.double().numpy()
    w_map[iy.numpy(), ix.numpy()] = w.double().numpy()
    kind[iy[~ok].numpy(), ix[~ok].numpy()] = KINDS.index("ncc")
    kind[iy[ok].numpy(), ix[ok].numpy()] = KINDS.index("counted")
    counted[iy[ok].numpy(), ix[ok].numpy()] = True
    n = int(ok.sum())
    raw = (w * ncc)[ok].sum()
    g_depth, g_normal = np.zeros((H, W), d_map.detach().numpy().dtype), np.zeros((3, H, W), d_map.detach().numpy().dtype)
    if grad == "autograd":
        if n > 0:
            raw.backward()
            g_depth, g_normal = d_map.grad.numpy(), n_map.grad.numpy()
    else:
        inner = ok & (td > 0) & (td < 2)
        c2, q2, den2 = 2 * cross, (cross * cross) * vr, den * den
        G = [-(w * ((c2 * (RD[c] - (sR * D[c]) / T)) / den - (q2 * (2 * (SD[c] - (sS * D[c]) / T))) / den2)) for c in range(3)]
        gm = (G[0] * mx + G[1] * my) + G[2] * mz
        parts = (-(gm / d), G[0] / dsr - (gm * rx) / s, G[1] / dsr - (gm * ry) / s, G[2] / dsr - gm / s)
        yy, xx = iy[inner].numpy(), ix[inner].numpy()
        g_depth[yy, xx] = parts[0][inner].numpy()
        for c in range(3):
            g_normal[c, yy, xx] = parts[1 + c][inner].numpy()
    rawf = float(raw.detach().double())
    value = rawf / max(n, 1) if dtype == torch.float64 else float((raw.detach() / torch.tensor(float(max(n, 1)), dtype=dtype)).double())
    return {"value": value, "raw": rawf, "n": n, "grad_depth": g_depth, "grad_normal": g_normal, "counted": counted,
            "ncc": ncc_map, "w": w_map, "kind": kind, "fragile": fragile}


def value_slack(ref64):
    """What the fragile pixels may move the value by: each adds at most 2 w <= 2 to the raw sum and one to the count, so
    ``|raw' / n' - raw / n| <= F (2 + value) / (n - F)``."""
    F = int((ref64["fragile"] & (ref64["kind"] >= 0)).sum())
    return F * (2.0 + ref64["value"]) / max(ref64["n"] - F, 1)


# ---- the scene ---------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.25, -0.15, -1.0]) / np.linalg.norm([0.25, -0.15, -1.0])
PLANE_C = float(PLANE_N @ np.array([0.0, 0.0, 4.0]))                      # n . X = c, through (0, 0, 4)
REF_W, REF_H, REF_FX, REF_FY = 70, 37, 44.0, 40.0
SRC_W, SRC_H, SRC_FX, SRC_FY = 48, 40, 38.0, 42.0
SRC_AXIS, SRC_DEG, SRC_POS = np.array([0.2, 1.0, 0.1]), 7.0, np.array([-0.45, 0.12, 0.05])
RADIUS, PIX_MAX, NCC_MAX, MIN_COS = 3, 1.0, 0.9, 0.05
GRAZING_COLUMN = 12


def texture(X):
    """The plane's texture at reference-frame points ``X [...,3]``."""
    x, y = X[..., 0], X[..., 1]
    return 0.5 + 0.2 * np.sin(3.1 * x + 0.4) + 0.15 * np.sin(2.3 * y - 1.0) + 0.1 * np.sin(5.0 * (x + y))


def _rotation(axis, deg):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = math.radians(deg)
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def cameras():
    ref = R.Cam(np.eye(3), np.zeros(3), REF_W, REF_H, REF_FX, REF_FY)
    src = R.Cam(_rotation(SRC_AXIS, SRC_DEG), SRC_POS, SRC_W, SRC_H, SRC_FX, SRC_FY)
    return ref, src


def render_plane(cam, ref):
    """Ray-plane intersection in ``cam`` -> (depth float32 [H,W], grey image float32 [H,W]); the plane and its texture
    live in the frame of ``ref``."""
    W, H = cam.image_width, cam.image_height
    fx, fy = (np.float64(v) for v in R.focal(cam))
    to_ref = np.linalg.inv(R.view64(cam)) @ R.view64(ref)                  # cam frame -> world -> ref frame, row vectors
    py, px = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ray = np.stack(((px - (W - 1) / 2) / fx, (py - (H - 1) / 2) / fy, np.ones_like(px)), axis=-1)
    ray_ref, o_ref = ray @ to_ref[:3, :3], to_ref[3, :3]
    tt = (PLANE_C - PLANE_N @ o_ref) / (ray_ref @ PLANE_N)
    X = o_ref + ray_ref * tt[..., None]
    return np.where(tt > 0, tt, 0.0).astype(np.float32), texture(X).astype(np.float32)


def true_maps():
    """-> (ref camera, depth [37,70], normal [3,37,70], gray, source camera, its depth [40,48], its gray): the true
    geometry.  The normal map is the plane's normal times a smooth positive field."""
    ref, src = cameras()
    depth, gray = render_plane(ref, ref)
    sdepth, sgray = render_plane(src, ref)
    yy, xx = np.meshgrid(np.arange(REF_H), np.arange(REF_W), indexing="ij")
    scale = 0.6 + 0.3 * np.sin(xx / 6.0 + 0.3) * np.cos(yy / 5.0)
    normal = (PLANE_N[:, None, None] * scale[None]).astype(np.float32)
    return ref, depth, normal, gray, src, sdepth, sgray


def scene():
    """The map the tests use -> (ref camera, depth, normal, gray, source camera, source depth, source gray).  The
    reference depth is the true one times a smooth field 1.03 .. 1.06 and the normals are tilted by a smooth field up to
    0.1, so the gradients are not near zero.  A rectangle of the source image holds an unrelated pattern (``ncc >=
    ncc_max``), a rectangle of the source depth is zero (a hole: the round trip fails) and another is scaled by 1.5 (the
    round trip lands past ``pix_max``), one column of the normal map is grazing, and a block of the reference has no
    depth."""
    ref, depth, normal, gray, src, sdepth, sgray = true_maps()
    yy, xx = np.meshgrid(np.arange(REF_H, dtype=np.float64), np.arange(REF_W, dtype=np.float64), indexing="ij")
    depth = (depth.astype(np.float64) * (1.045 + 0.015 * np.sin(xx / 9.0) * np.cos(yy / 7.0))).astype(np.float32)
    tilt = np.stack((-0.1 * np.sin(xx / 11.0 + 0.2), 0.1 * np.cos(yy / 8.0 - 0.4), np.zeros_like(xx)))
    length = np.linalg.norm(normal.astype(np.float64), axis=0)
    normal = (normal.astype(np.float64) + tilt * length[None]).astype(np.float32)
    ray = np.array([(GRAZING_COLUMN - (REF_W - 1) / 2) / REF_FX, 0.0, 1.0])
    normal[:, :, GRAZING_COLUMN] = np.array([1.0, 0.0, -ray[0] + 0.01], np.float32)[:, None]       # nearly in the plane of the rays
    depth[3:6, 60:66] = 0.0
    sy, sx = np.meshgrid(np.arange(SRC_H, dtype=np.float64), np.arange(SRC_W, dtype=np.float64), indexing="ij")
    pattern = (0.5 + 0.3 * np.sin(1.9 * sx) * np.cos(1.3 * sy + 0.7)).astype(np.float32)
    sgray = sgray.copy()
    sgray[4:16, 6:18] = pattern[4:16, 6:18]
    sdepth = sdepth.copy()
    sdepth[24:31, 8:16] = 0.0
    sdepth[24:32, 26:36] *= np.float32(1.5)
    return ref, depth, normal, gray, src, sdepth, sgray


def contrast_image(H, W):
    """A grey image whose every 3 x 3 (and larger) patch has a sum of squared deviations above 0.1: under the identity
    warp ``ncc`` is exactly ``1e-8 / (var^2 + 1e-8)``, which is below 1e-6 only from ``var >= 0.1`` on."""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    return (0.5 + 0.45 * np.sin(1.3 * xx + 0.2) * np.cos(1.1 * yy - 0.3)).astype(np.float32)


def row_of(ref, src, sdepth):
    return R.source_rows(ref, [src], [sdepth])[0]
