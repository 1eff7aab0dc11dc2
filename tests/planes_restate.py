"""Torch restatement of ``csrc/planes.hip`` and ``csrc/plane_depth.hip`` (include/gsr.h, ABI v37) at a
chosen dtype -- float64 is the truth, float32 the yardstick for the bar -- with the "fragile" sets: the rows and pixels
whose decisions sit within ``MARGIN`` of flipping, where two correct implementations may disagree.  Also the inputs the
GPU test runs on, so that the host test can take their census at float64."""
import math

import torch

MARGIN = 1e-4
FLT_MAX = 3.4028234663852886e38


def rotation_matrices(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = (1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
            2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
            2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y))
    return torch.stack(rows, dim=1).reshape(-1, 3, 3)


def planes(scales, rotations, means3D, viewmatrix, campos, dtype=torch.float64):
    """-> dict(planes [P,4], axis [P], sign [P], fragile [P] bool, tie [P] bool, facing0 [P] bool).  ``rotations`` and
    ``means3D`` may require a gradient (at ``dtype``, or float32 tensors that are cast here)."""
    s, rot, mean = scales.detach().to(dtype), rotations.to(dtype), means3D.to(dtype)
    V, cam = viewmatrix.detach().to(dtype)[:3, :3], campos.detach().to(dtype).view(1, 3)
    q = torch.nn.functional.normalize(rot, dim=1)                      # rot / max(|rot|, 1e-12)
    R = rotation_matrices(q)
    axis = torch.argmin(s, dim=1)                                      # the smallest index among equals
    col = torch.gather(R, 2, axis.view(-1, 1, 1).expand(-1, 3, 1)).squeeze(2)
    to_cam = cam - mean
    facing = (col.detach() * to_cam.detach()).sum(dim=1)
    sign = torch.where(facing < 0, -1.0, 1.0).to(dtype)                # exactly 0 keeps +1
    n_w = col * sign.unsqueeze(1)
    out = torch.cat([n_w @ V, (n_w * to_cam).sum(dim=1, keepdim=True)], dim=1)
    s2 = torch.sort(s, dim=1).values
    tie = s2[:, 0] == s2[:, 1]
    near_tie = ((s2[:, 1] - s2[:, 0]) <= MARGIN * s2[:, 1].abs()) & ~tie
    dist = to_cam.detach().norm(dim=1)
    facing0 = facing == 0
    near_facing = (facing.abs() <= MARGIN * dist) & ~facing0
    return {"planes": out, "axis": axis, "sign": sign, "fragile": near_tie | near_facing, "tie": tie, "facing0": facing0}


def focal(H, W, tanfovx, tanfovy):
    """(fx, fy, cx, cy) as the entry point builds them: the tangents arrive as float32, each focal length is one double
    division rounded to float32."""
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))      # noqa: E731
    fx, fy = f32(W / (2.0 * f32(tanfovx))), f32(H / (2.0 * f32(tanfovy)))
    return fx, fy, (W - 1) * 0.5, (H - 1) * 0.5


def rays(H, W, tanfovx, tanfovy, dtype):
    fx, fy, cx, cy = focal(H, W, tanfovx, tanfovy)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    return (xs - cx) / torch.tensor(fx, dtype=dtype), (ys - cy) / torch.tensor(fy, dtype=dtype)


def plane_depth(normal, distance, alpha, tanfovx, tanfovy, alpha_min=0.5, min_cos=0.05, dtype=torch.float64):
    """-> dict(z [H,W], valid [H,W] bool, fragile [H,W] bool, dz_dD [H,W], dz_dN [3,H,W]); ``normal [3,H,W]`` and
    ``distance [H,W]`` may require a gradient (``z`` is differentiable; the unit gradients are the closed forms)."""
    N, D, A = normal.to(dtype), distance.to(dtype).reshape(normal.shape[1:]), alpha.detach().to(dtype).reshape(normal.shape[1:])
    H, W = D.shape
    rx, ry = rays(H, W, tanfovx, tanfovy, dtype)
    am, mc = float(torch.tensor(alpha_min, dtype=torch.float32)), float(torch.tensor(min_cos, dtype=torch.float32))
    c = -((N[0] * rx + N[1] * ry) + N[2])
    Nd, Dd, cd = N.detach(), D.detach(), c.detach()
    nr = torch.sqrt(((Nd[0] * Nd[0] + Nd[1] * Nd[1]) + Nd[2] * Nd[2]) * ((rx * rx + ry * ry) + 1.0))
    finite = (Nd.abs() <= FLT_MAX).all(dim=0) & (Dd.abs() <= FLT_MAX) & (A.abs() <= FLT_MAX)
    valid = finite & (A >= am) & (Dd > 0) & (cd > 0) & (cd >= mc * nr)
    inv = 1.0 / torch.where(valid, c, torch.ones_like(c))
    zz = D * inv
    k = zz.detach() * inv.detach()
    rmax = torch.maximum(torch.ones_like(rx), torch.maximum(rx.abs(), ry.abs()))
    valid = valid & (zz.detach() <= FLT_MAX) & (inv.detach() <= FLT_MAX) & (k * rmax <= FLT_MAX)
    zero = torch.zeros_like(zz)
    z = torch.where(valid, zz, zero)
    dz_dD = torch.where(valid, inv.detach(), zero)
    dz_dN = torch.stack([torch.where(valid, k * rx, zero), torch.where(valid, k * ry, zero), torch.where(valid, k, zero)])
    fragile = finite & (((A - am).abs() <= MARGIN) | ((Dd != 0) & (Dd.abs() <= MARGIN)) |
                        ((cd - mc * nr).abs() <= MARGIN * nr))
    return {"z": z, "valid": valid, "fragile": fragile, "dz_dD": dz_dD, "dz_dN": dz_dN}


# ---- the inputs of tests/test_gpu_planes.py ---------------------------------------------------------------------------

ROW_SIZES = (1, 63, 64, 65, 257, 4099)
MAP_SHAPES = ((1, 1), (7, 7), (65, 9), (70, 37), (3, 130))            # (W, H): 70 x 37 is the NCC test's reference size
TANFOV = (0.62, 0.41)


def row_camera():
    """(viewmatrix [4,4], campos [3]) float32: some rigid camera, row-vector convention."""
    q = torch.tensor([[0.9, 0.1, -0.3, 0.2]], dtype=torch.float64)
    Rw2c = rotation_matrices(torch.nn.functional.normalize(q, dim=1))[0]
    campos = torch.tensor([0.3, -0.2, -1.0], dtype=torch.float64)
    vm = torch.eye(4, dtype=torch.float64)
    vm[:3, :3] = Rw2c.t()
    vm[3, :3] = -(Rw2c @ campos)
    return vm.to(torch.float32), campos.to(torch.float32)


def make_rows(P, seed=0):
    """(scales [P,3], rotations [P,4], means3D [P,3]) float32: ordinary rows -- log-normal scales, unnormalised
    quaternions over three decades of length -- and, by row index modulo 16 (from row 1 on, as far as P reaches): 1 a
    two-way scale tie at the minimum (indices 0 and 1), 2 a two-way tie (1 and 2), 3 a three-way tie, 4 and 5 a facing dot
    product of exactly 0 (a rotation about z, z the flattest axis, the mean at campos + t (a, b, 0)); once each: row 6 an
    all-zero quaternion, row 7 very flat, row 8 nearly isotropic."""
    g = torch.Generator().manual_seed(1000 + seed)
    scales = torch.exp(torch.randn(P, 3, generator=g) * 0.7 - 3.0)
    rot = torch.randn(P, 4, generator=g) * torch.exp(torch.randn(P, 1, generator=g) * 1.5)
    means = torch.randn(P, 3, generator=g) * 2.0 + torch.tensor([0.0, 0.0, 5.0])
    _, campos = row_camera()
    for i in range(1, P):
        k = i % 16
        a = float(scales[i, 0])
        if k == 1:
            scales[i] = torch.tensor([a, a, 2.5 * a])
        elif k == 2:
            scales[i] = torch.tensor([3.0 * a, a, a])
        elif k == 3:
            scales[i] = torch.tensor([a, a, a])
        elif k in (4, 5):
            ang = float(torch.rand((), generator=g)) * 6.0
            rot[i] = torch.tensor([math.cos(ang), 0.0, 0.0, math.sin(ang)]) * (0.5 + k)
            scales[i] = torch.tensor([2.0 * a, 3.0 * a, a])
            t = torch.randn(2, generator=g) * 3.0
            means[i] = torch.stack([campos[0] + t[0], campos[1] + t[1], campos[2]])
    if P > 6:
        rot[6] = 0.0
    if P > 7:
        scales[7] = torch.tensor([1.0, 1.5, 1e-6])
    if P > 8:
        scales[8] = torch.tensor([1.0, 1.001, 0.999])
    return scales, rot, means


def make_maps(W, H, seed=0):
    """(normal [3,H,W], distance [H,W], alpha [H,W]) float32: a plane tilted against the view axis with a smooth
    perturbation of its normal and distance under a smooth coverage in [0.65, 0.95], and -- on images of 16 pixels or more
    -- a rectangle of alpha = 0.3 < alpha_min, a rectangle of D = 0, the last column grazing (c about 0.01 |N| |r|, below
    min_cos) and one pixel with a NaN normal."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    u, v = xs / max(W - 1, 1), ys / max(H - 1, 1)
    n = torch.stack([0.45 + 0.05 * torch.sin(3.0 * u + seed), 0.2 + 0.05 * torch.cos(2.0 * v), -torch.ones_like(u)])
    n = n / n.norm(dim=0, keepdim=True)
    alpha = 0.8 + 0.15 * torch.sin(2.0 * u + 3.0 * v + 0.5 * seed)
    d = 3.0 + 0.1 * torch.sin(4.0 * u) * torch.cos(3.0 * v)
    N, D = n * alpha, d * alpha
    if H * W >= 16:
        alpha[H // 4:max(H // 2, H // 4 + 1), W // 4:max(W // 2, W // 4 + 1)] = 0.3
        D[H // 2:max(3 * H // 4, H // 2 + 1), W // 2:max(3 * W // 4, W // 2 + 1)] = 0.0
        rx, ry = rays(H, W, TANFOV[0], TANFOV[1], torch.float64)
        r = torch.stack([rx, ry, torch.ones_like(rx)])[:, :, W - 1]
        r = r / r.norm(dim=0, keepdim=True)
        side = torch.linalg.cross(r, torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).view(3, 1).expand_as(r), dim=0)
        side = side / side.norm(dim=0, keepdim=True)
        N[:, :, W - 1] = (side - 0.01 * r) * alpha[:, W - 1]
        N[:, H - 1, 0] = float("nan")
    return N.to(torch.float32), D.to(torch.float32), alpha.to(torch.float32)


def rel_err(got, ref):
    """The largest error as a share of the largest magnitude in ``ref``: the project's standing measure."""
    ref = ref.to(torch.float64)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    if ref.numel() == 0:
        return 0.0
    return float((got.to(torch.float64) - ref).abs().max()) / max(scale, 1e-300)
