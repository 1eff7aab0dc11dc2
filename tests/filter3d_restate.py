"""The numpy restatement of Mip-Splatting's 3D smoothing filter (csrc/filter3d_math.h; filter3d.py).

The sampling rule in float32, every operation rounded on its own and in the header's order, so that the host build of the
header and the kernel can be compared with it bit for bit; the application and its gradients in float64 (the gradient from
torch float64 autograd on the closed form), rounded to float32 once; the definition of the application in 80-digit decimal
arithmetic (``apply_exact``); and the planted per-row states for the global reduction.  Not a test module: tests/test_filter3d_host.py and
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


# ---- planted per-row states for the global reduction (csrc/filter3d.hip: filter3d_reduce_kernel) ---------------------------------
WAVE = 64
PLANT_SIZES = (4097, 65536, 65537, 131073)
PLANT_PAIRS = (0, 15, 16, 63, 64, 1023, 1024, 1087, 2047, 2048)


def plant_pairs(P):
    """The pairs (one per 64 rows) a planted row is put in at ``P`` rows: those of ``PLANT_PAIRS`` that exist and the last."""
    n = (P + WAVE - 1) // WAVE
    return sorted({k for k in PLANT_PAIRS if k < n} | {n - 1})


def plant_row(P, k):
    """The row planted in pair ``k``: a lane that differs from pair to pair, clipped to the live rows."""
    return min(WAVE * k + k % WAVE, P - 1)


def _unseen(P):
    """What the sampling pass leaves of a row no view saw: exactly the values that would win the maximum and the minimum
    if the reduction dropped its ``seen`` gate."""
    return np.full(P, np.inf, dtype=F), np.zeros(P, dtype=F), np.zeros(P, dtype=np.uint8)


def planted_cases(P):
    """-> a list of ``(name, min_depth, max_rate, seen uint8)`` at ``P`` rows; every value a float32 the caller plants."""
    cases, ks = [], plant_pairs(P)
    for k in ks:                                                    # one seen row only
        d, r, hit = _unseen(P)
        i = plant_row(P, k)
        d[i], r[i], hit[i] = 3.0, 7.0, 1
        cases.append((f"one seen row, pair {k}", d, r, hit))
    rng = np.random.default_rng(P)
    base_d, base_r = rng.uniform(1.0, 2.0, size=P).astype(F), rng.uniform(10.0, 20.0, size=P).astype(F)
    base_hit = (np.arange(P) % 7 != 3).astype(np.uint8)
    blank_d, blank_r, _ = _unseen(P)
    for shift in (1, len(ks) - 1):                                  # D and R from neighbours in the list, both ways round
        for n, kd in enumerate(ks):
            kr = ks[(n + shift) % len(ks)]
            hit = base_hit.copy()
            i, j = plant_row(P, kd), plant_row(P, kr)
            hit[i] = hit[j] = 1
            d, r = np.where(hit, base_d, blank_d), np.where(hit, base_r, blank_r)
            d[i], r[j] = 9.0, 0.5
            cases.append((f"D in pair {kd}, R in pair {kr}", d, r, hit))
    hit = base_hit.copy()                                           # wholly unseen waves between seen ones
    hit[WAVE:63 * WAVE] = 0
    hit[WAVE * ((P - 1) // WAVE):] = 0                              # the last wave: its one live lane where it is partial
    cases.append(("pairs 1 to 62 and the last unseen", np.where(hit, base_d, blank_d), np.where(hit, base_r, blank_r), hit))
    return cases


def wave_pairs(min_depth, max_rate, seen):
    """-> float32 ``[ceil(P / 64), 2]``: per 64 rows (max of min_depth, min of max_rate) over the seen rows, the neutral
    (-inf, +inf) where none is seen -- what ``gsr_filter3d_sample`` leaves in the workspace."""
    P = len(seen)
    n = (P + WAVE - 1) // WAVE
    d, r = np.full(n * WAVE, -np.inf, dtype=F), np.full(n * WAVE, np.inf, dtype=F)
    hit = np.asarray(seen).astype(bool)
    d[:P][hit], r[:P][hit] = min_depth[hit], max_rate[hit]
    return np.stack([d.reshape(n, WAVE).max(axis=1), r.reshape(n, WAVE).min(axis=1)], axis=1)


def reduce_model(pairs, block=1024, first_wave=1, step=None):
    """A host model of ``filter3d_reduce_kernel``'s data flow over ``pairs [n,2]``: lane ``t`` of ``block`` folds pairs
    ``t, t + step, ...``; each wave of 64 lanes folds its lanes; lane 0 holds wave 0's result and folds in waves
    ``first_wave ..``.  The kernel has ``first_wave = 1`` and ``step = block``; other values model a broken combine or
    stride.  -> ``(D, R, none_seen)``."""
    step = block if step is None else step
    n = len(pairs)
    lane_d, lane_r = np.full(block, -np.inf, dtype=F), np.full(block, np.inf, dtype=F)
    for t in range(min(block, n)):
        lane_d[t], lane_r[t] = pairs[t:n:step, 0].max(), pairs[t:n:step, 1].min()
    wd, wr = lane_d.reshape(-1, WAVE).max(axis=1), lane_r.reshape(-1, WAVE).min(axis=1)
    D, R_ = max([wd[0]] + list(wd[first_wave:])), min([wr[0]] + list(wr[first_wave:]))
    return F(D), F(R_), int(not D > -np.inf)


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


# ---- the application: the definition itself, exactly ---------------------------------------------------------------------------
EXACT_DIGITS = 80
GRID_S0 = (-87.0, -60.0, -40.0, -20.0, -10.0, -3.0, 0.0, 5.0, 10.0, 40.0, 87.0)
GRID_O = (-88.0, -40.0, -17.0, -1.0, -1e-3, 0.0, 1e-3, 1.0, 17.0, 40.0, 88.0)
GRID_RATIO = (1e-12, 1e-8, 1e-4, 1e-2, 1.0, 1e2, 1e4, 1e8, 1e12)


def _filtered(dec, s, o, f2):
    """One row of the definition in ``decimal``: ``s`` three Decimals, ``o`` and ``f2 = f^2`` Decimals ->
    ``(a_i + f^2, p, c, 1 - p c)``."""
    af = [(2 * x).exp() + f2 for x in s]
    c = dec.Decimal(1)
    for x, y in zip(s, af):
        c *= (2 * x).exp() / y
    c = c.sqrt()
    p = 1 / (1 + (-o).exp())
    return af, p, c, 1 - p * c


def apply_exact(s, o, f):
    """The DEFINITION of the application, not its closed form, in the standard library's ``decimal`` at 80 digits:

        a_i = exp(2 s_i)      s'_i = ln(a_i + f^2) / 2      c = sqrt(prod a_i / (a_i + f^2))      p = 1 / (1 + exp(-o))
        o' = ln(p c / (1 - p c))                      (o itself where f = 0)
        ds'_i/ds_i = a_i / (a_i + f^2)     do'/do = (1 - p) / (1 - p c)     do'/ds_i = (f^2 / (a_i + f^2)) / (1 - p c)

    (``do'/ds_i`` is positive: a larger Gaussian is attenuated less.)  No ``log1p``, no ``expm1``, no factored exponential:
    at 80 digits ``1 - p c`` keeps 40 of them where it is smallest on float32 inputs (``1 - p`` at ``o = 88`` is 6e-39).
    The inputs are the float32 values themselves (a float32 has up to 112 decimal digits; the first operation rounds it to
    80).  -> a namespace of float64 arrays ``s [P,3]``, ``o [P]``, ``ds_ds [P,3]``, ``do_do [P]``, ``do_ds [P,3]``, each
    the exact value rounded once."""
    import decimal as dec
    s, o, f = np.asarray(s, dtype=F).reshape(-1, 3), np.asarray(o, dtype=F).reshape(-1), np.asarray(f, dtype=F).reshape(-1)
    P = len(o)
    assert len(s) == P and len(f) == P
    out = SimpleNamespace(s=np.empty((P, 3)), o=np.empty(P), ds_ds=np.empty((P, 3)), do_do=np.empty(P), do_ds=np.empty((P, 3)))
    with dec.localcontext() as ctx:
        ctx.prec = EXACT_DIGITS
        for i in range(P):
            sd, od, fd = [dec.Decimal(float(v)) for v in s[i]], dec.Decimal(float(o[i])), dec.Decimal(float(f[i]))
            f2 = fd * fd
            af, p, c, omx = _filtered(dec, sd, od, f2)
            out.s[i] = [float(y.ln() / 2) for y in af]
            out.o[i] = float(o[i]) if f[i] == 0 else float((p * c / omx).ln())
            out.ds_ds[i] = [float(1 - f2 / y) for y in af]
            out.do_do[i] = float((1 - p) / omx)
            out.do_ds[i] = [float(f2 / y / omx) for y in af]
    return out


def exact_bwd(ex, g_s, g_o):
    """The chain rule over ``apply_exact``'s factors, in float64 (three roundings of the terms' size: what the backward
    bar's ``1e-14 x`` allowance covers 30 times over) -> ``(dL/ds [P,3], dL/do [P], cond [P,3])`` with ``cond`` the sum of
    the magnitudes of the two terms of ``dL/ds``."""
    g_s, g_o = np.asarray(g_s, dtype=np.float64).reshape(-1, 3), np.asarray(g_o, dtype=np.float64).reshape(-1)
    own, cross = g_s * ex.ds_ds, g_o[:, None] * ex.do_ds
    return own + cross, g_o * ex.do_do, np.abs(own) + np.abs(cross)


def exact_grid():
    """The 11 x 11 x 9 grid of the range float32 parameters can hold (``|s| <= 87``: ``exp(s)`` a normal float32):
    ``s = (s0, s0 + 0.7, s0 - 1.3)``, ``f = float32(e^s0 * ratio)``; a row whose ``f`` is not a finite positive float32 is
    dropped and nothing else is -> ``(s float32 [n,3], o float32 [n], f float32 [n], dropped)``, ``dropped`` the set of
    ``(s0, ratio)`` pairs that went (with all eleven ``o`` each)."""
    rows, dropped = [], set()
    with np.errstate(over="ignore", under="ignore"):
        for s0 in GRID_S0:
            for ratio in GRID_RATIO:
                f = F(math.exp(s0) * ratio)
                if not (np.isfinite(f) and f > 0):
                    dropped.add((s0, ratio))
                    continue
                rows += [(s0, s0 + 0.7, s0 - 1.3, o, f) for o in GRID_O]
    rows = np.array(rows, dtype=np.float64).astype(F)
    return rows[:, :3].copy(), rows[:, 3].copy(), rows[:, 4].copy(), dropped


def exact_case(random_rows):
    """The rows every comparison with ``apply_exact`` runs on: the grid, ``random_rows = (s, o, f)`` of the narrow box the
    first tests used (the caller's ``_apply_case``), and ``f = 0`` at ``o`` in {-88, -0.0, 88} -> ``(s, o, f, g_s, g_o,
    n_grid)``, the gradients from a seeded normal."""
    s, o, f, _ = exact_grid()
    n_grid = len(o)
    rng = np.random.default_rng(734)
    rs, ro, rf = (np.asarray(a, dtype=F) for a in random_rows)
    ro = ro.reshape(-1)
    zs = np.array([[-87.0, 0.7, 87.0], [0.0, -3.0, 5.0], [87.0, 86.0, -87.0]], dtype=F)
    zo = np.array([-88.0, -0.0, 88.0], dtype=F)
    s, o, f = np.concatenate([s, rs, zs]), np.concatenate([o, ro, zo]), np.concatenate([f, rf, np.zeros(3, dtype=F)])
    return s, o, f, rng.standard_normal((len(o), 3)).astype(F), rng.standard_normal(len(o)).astype(F), n_grid


def worst_places(got, want64, groups):
    """For a printed report: per named boolean row mask, the largest ``ulps`` and the row it occurs at."""
    u = ulps(got, want64)
    u = u.reshape(len(u), -1).max(axis=1)
    return {name: (float(u[m].max()), int(np.flatnonzero(m)[u[m].argmax()])) if m.any() else (0.0, -1)
            for name, m in groups.items()}


def assert_exact_bars(got_s, got_o, got_ds, got_do, case, what):
    """The bars tests/test_filter3d_host.py and tests/test_gpu_filter3d.py hold an evaluation of the application to,
    against ``apply_exact``: ``case`` has ``s, o, f, g_s, g_o`` (float32) and ``ex = apply_exact(s, o, f)``.  Forward: at
    most one float32 place from the exact value rounded once.  Backward: one float32 spacing plus 1e-14 x the sum of the
    magnitudes of the two terms of ``dL/ds``, or 1e-14 |dL/do|.  ``f = 0`` rows: bit copies in both directions.  Prints
    the worst place counts per branch and their rows before it asserts."""
    def same(a, b):
        return np.array_equal(np.asarray(a, dtype=F).view(np.uint32), np.asarray(b, dtype=F).view(np.uint32))
    ex, zero = case.ex, case.f == 0
    got_s, got_o = np.asarray(got_s, dtype=F).reshape(-1, 3), np.asarray(got_o, dtype=F).reshape(-1)
    got_ds, got_do = np.asarray(got_ds).reshape(-1, 3), np.asarray(got_do).reshape(-1)
    groups = {"o <= 0": ~zero & (case.o <= 0), "o > 0": ~zero & (case.o > 0), "f = 0": zero}
    fwd_s, fwd_o = worst_places(got_s, ex.s, groups), worst_places(got_o, ex.o, groups)
    w_ds, w_do, cond = exact_bwd(ex, case.g_s, case.g_o)
    err_s = (np.abs(got_ds.astype(np.float64) - w_ds) - 1e-14 * cond) / np.spacing(np.abs(w_ds).astype(F))
    err_o = (np.abs(got_do.astype(np.float64) - w_do) - 1e-14 * np.abs(w_do)) / np.spacing(np.abs(w_do).astype(F))
    for name, m in groups.items():
        rs, ro = int(np.flatnonzero(m)[err_s[m].max(axis=1).argmax()]), int(np.flatnonzero(m)[err_o[m].argmax()])
        print(f"[filter3d exact] {what}, {name} ({int(m.sum())} rows): forward worst {fwd_s[name][0]:.0f} places (s', row "
              f"{fwd_s[name][1]}) / {fwd_o[name][0]:.0f} (o', row {fwd_o[name][1]}); backward worst "
              f"{max(err_s[rs].max(), 0.0):.2f} (dL/ds, row {rs}) / {max(err_o[ro], 0.0):.2f} (dL/do, row {ro})")
    assert all(v[0] <= 1 for v in fwd_s.values()), fwd_s
    assert all(v[0] <= 1 for v in fwd_o.values()), fwd_o
    assert (err_s <= 1).all() and (err_o <= 1).all()
    assert zero.sum() >= 3 and same(got_s[zero], case.s[zero]) and same(got_o[zero], case.o[zero])
    assert same(got_ds[zero], case.g_s[zero]) and same(got_do[zero], case.g_o[zero])


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
