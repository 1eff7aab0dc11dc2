"""The numpy restatement of Mip-Splatting's 3D smoothing filter (csrc/filter3d_math.h; filter3d.py).

The sampling rule in float32, every operation rounded on its own and in the header's order, so that the host build of the
header and the kernel can be compared with it bit for bit; the application and its gradients in float64 (the gradient from
torch float64 autograd on the closed form), rounded to float32 once.  Not a test module: tests/test_filter3d_host.py and
tests/test_gpu_filter3d.py import it."""
import math
from types import SimpleNamespace

import numpy as np
import torch

F = np.float32
RULES = {"mip_splatting": 0, "paper": 1}


class Cam(SimpleNamespace):
    """What ``compute_3d_filter`` reads of a camera."""


def camera(W, H, fx, fy, M=None):
    M = np.eye(4, dtype=np.float32) if M is None else np.asarray(M, dtype=np.float32)
    return Cam(image_width=int(W), image_height=int(H), FoVx=2.0 * math.atan(W / (2.0 * fx)),
               FoVy=2.0 * math.atan(H / (2.0 * fy)), world_view_transform=torch.from_numpy(M.copy()))


def focal(cam):
    """(H, W, fx, fy) with the focal lengths as the float32 the table row holds (``mvs._focal`` in Python floats)."""
    H, W = int(cam.image_height), int(cam.image_width)
    return H, W, F(W / (2.0 * math.tan(float(cam.FoVx) * 0.5))), F(H / (2.0 * math.tan(float(cam.FoVy) * 0.5)))


def look_from(angle, radius, centre=(0.0, 0.0, 0.0), tilt=0.0):
    """A world-to-view matrix (row-vector convention, float32) of a camera on a circle of ``radius`` about ``centre``,
    looking at it."""
    c, s = math.cos(angle), math.sin(angle)
    R = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]], dtype=np.float64)          # world -> camera rotation (column form)
    ct, st = math.cos(tilt), math.sin(tilt)
    R = np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]], dtype=np.float64) @ R
    t = -R @ np.asarray(centre, dtype=np.float64) + np.array([0.0, 0.0, radius])
    M = np.eye(4, dtype=np.float64)
    M[:3, :3] = R.T
    M[3, :3] = t
    return M.astype(np.float32)


def sample(xyz, cameras, near=0.2, margin=0.15):
    """-> (min_depth float32 [P], max_rate float32 [P], seen bool [P]) in csrc/filter3d_math.h's operation order."""
    xyz = np.asarray(xyz, dtype=F)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    P = len(xyz)
    near, margin = F(near), F(margin)
    min_depth, max_rate, seen = np.full(P, np.inf, dtype=F), np.zeros(P, dtype=F), np.zeros(P, dtype=bool)
    with np.errstate(all="ignore"):
        for cam in cameras:
            H, W, fx, fy = focal(cam)
            M = cam.world_view_transform.detach().cpu().numpy().astype(F).reshape(-1)
            xv = ((x * M[0] + y * M[4]) + z * M[8]) + M[12]
            yv = ((x * M[1] + y * M[5]) + z * M[9]) + M[13]
            zv = ((x * M[2] + y * M[6]) + z * M[10]) + M[14]
            Wf, Hf = F(W), F(H)
            u = (xv / zv) * fx + Wf * F(0.5)
            w = (yv / zv) * fy + Hf * F(0.5)
            hi = F(1.0) + margin
            ok = (zv > near) & (u >= -margin * Wf) & (u <= hi * Wf) & (w >= -margin * Hf) & (w <= hi * Hf)
            min_depth = np.where(ok, np.minimum(min_depth, zv), min_depth).astype(F)
            max_rate = np.where(ok, np.maximum(max_rate, fx / zv), max_rate).astype(F)
            seen |= ok
    assert min_depth.dtype == F and max_rate.dtype == F
    return min_depth, max_rate, seen


def width(min_depth, max_rate, seen, cameras, variance=0.2, rule="mip_splatting"):
    """-> (filter float32 [P], none_seen 0 / 1)."""
    P = len(seen)
    if not seen.any():
        return np.zeros(P, dtype=F), 1
    sd = np.sqrt(F(variance))
    assert sd.dtype == F
    if rule == "paper":
        v = np.where(seen, max_rate, max_rate[seen].min()).astype(F)
        out = sd / v
    else:
        focal_max = max(focal(c)[2] for c in cameras)
        v = np.where(seen, min_depth, min_depth[seen].max()).astype(F)
        out = (v / F(focal_max)) * sd
    assert out.dtype == F
    return out, 0


def compute(xyz, cameras, near=0.2, margin=0.15, variance=0.2, rule="mip_splatting"):
    return width(*sample(xyz, cameras, near, margin), cameras, variance, rule)


# ---- the application: float64 closed forms ---------------------------------------------------------------------------------
def apply_torch(s, o, f):
    """The effective raw parameters in torch float64, differentiable: ``s [P,3]``, ``o [P]``, ``f [P]`` (float64 tensors)
    -> ``(s' [P,3], o' [P])``, the closed form of csrc/filter3d_math.h."""
    t = (f * f)[:, None] * torch.exp(-2.0 * s)
    l = 0.5 * torch.log1p(t)
    L = (l[:, 0] + l[:, 1]) + l[:, 2]
    omc = -torch.expm1(-L)
    neg = (o - L) - torch.log1p(omc * torch.exp(torch.clamp(o, max=0.0)))
    pos = -L - torch.log(omc + torch.exp(-torch.clamp(o, min=0.0)))
    return s + l, torch.where(o <= 0, neg, pos)


def apply(s, o, f):
    """float32 arrays -> ``(s' [P,3], o' [P])`` float32: the float64 results rounded once."""
    sd, od, fd = (torch.from_numpy(np.asarray(a, dtype=np.float64)) for a in (s, o, f))
    so, oo = apply_torch(sd, od.reshape(-1), fd)
    return so.numpy().astype(F), oo.numpy().astype(F).reshape(np.shape(o))


def apply_direct(s, o, f):
    """The definition itself in float64 -> the ACTIVATED filtered values ``(sqrt(a + f^2) [P,3], sigmoid(o) c [P])``."""
    s, o, f = (np.asarray(a, dtype=np.float64) for a in (s, o, f))
    a = np.exp(2.0 * s)
    af = a + (f * f)[:, None]
    c = np.sqrt(np.prod(a / af, axis=1))
    return np.sqrt(af), c / (1.0 + np.exp(-o.reshape(-1)))


def apply_bwd(s, o, f, g_s, g_o):
    """float64 autograd on the closed form -> ``(dL/ds [P,3], dL/do [P])`` as float64 arrays, and the conditioning of
    dL/ds: the sum of the magnitudes of its two terms (what a rounding error of the float64 evaluation scales with)."""
    sd = torch.from_numpy(np.asarray(s, dtype=np.float64)).requires_grad_(True)
    od = torch.from_numpy(np.asarray(o, dtype=np.float64).reshape(-1)).requires_grad_(True)
    fd = torch.from_numpy(np.asarray(f, dtype=np.float64))
    gs = torch.from_numpy(np.asarray(g_s, dtype=np.float64))
    go = torch.from_numpy(np.asarray(g_o, dtype=np.float64).reshape(-1))
    so, oo = apply_torch(sd, od, fd)
    d_s, d_o = torch.autograd.grad([so, oo], [sd, od], [gs, go])
    only_s, = torch.autograd.grad(apply_torch(sd, od, fd)[0], sd, gs)
    cond = only_s.abs() + (d_s - only_s).abs()
    return d_s.numpy(), d_o.numpy(), cond.numpy()


def ulps(got, want64):
    """|got - want| in units of the float32 spacing at ``want`` (``got`` float32, ``want64`` float64, compared against its
    float32 rounding)."""
    want = np.asarray(want64, dtype=np.float64).astype(F)
    got = np.asarray(got, dtype=F)
    spacing = np.spacing(np.abs(want)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / spacing


# ---- test scenes -------------------------------------------------------------------------------------------------------------
def gate_scene(P, V, seed=0):
    """P points and V cameras that put points on both sides of every gate: behind and in front of the near plane, left
    and right, above and below the margins, and some that no camera sees."""
    rng = np.random.default_rng(1000 * V + P + seed)
    xyz = (rng.standard_normal((P, 3)) * np.array([3.0, 2.0, 3.0])).astype(F)
    cams = []
    for v in range(V):
        W, H = (64, 48) if v % 2 == 0 else (96, 40)
        fx = 60.0 + 25.0 * (v % 5)
        cams.append(camera(W, H, fx, fx * 1.1, look_from(2.0 * math.pi * v / max(V, 1) + 0.3, 2.5 + 0.5 * (v % 3),
                                                         tilt=0.1 * (v % 4))))
    return xyz, cams
