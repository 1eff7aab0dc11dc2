"""Float64 / Python-integer restatement of the MCMC strategy's arithmetic (include/gsr.h, ABI v25),
written from the formulas and using nothing of the package.  Inputs are the model's RAW float32 tensors as numpy arrays;
they are converted to float64 once and everything after that is float64 (or Python ints for the sampler)."""
import bisect
import itertools
import math

import numpy as np

FX_ONE = 1 << 30
NMAX = 51


def f64(a):
    return np.asarray(a, dtype=np.float64)


def sigmoid64(raw):
    return 1.0 / (1.0 + np.exp(-f64(raw)))


def rotation64(rotation_raw):
    """(R [P,3,3], T [P,3,3]) of q = raw / max(|raw|, 1e-12): the rotation and, per entry, the sum of the absolute values
    of the terms it is formed from (2 (|a b| + |c d|) off the diagonal, |R_ii| + 2 (a^2 + b^2) on it): what the rounding
    error of an entry scales with -- an entry 2 (x y - r z) can cancel, its error cannot."""
    q = f64(rotation_raw)
    q = q / np.maximum(np.sqrt((q * q).sum(axis=1, keepdims=True)), 1e-12)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(-1, 3, 3)
    a = np.abs
    T = np.stack([a(R[:, 0, 0]) + 2 * (y * y + z * z), 2 * (a(x * y) + a(r * z)), 2 * (a(x * z) + a(r * y)),
                  2 * (a(x * y) + a(r * z)), a(R[:, 1, 1]) + 2 * (x * x + z * z), 2 * (a(y * z) + a(r * x)),
                  2 * (a(x * z) + a(r * y)), 2 * (a(y * z) + a(r * x)), a(R[:, 2, 2]) + 2 * (x * x + y * y)],
                 axis=1).reshape(-1, 3, 3)
    return R, T


def _sandwich(A, s2, B, v):
    """A (s2 * (B^T v)) per row."""
    return np.einsum("pij,pj->pi", A, s2 * np.einsum("pkj,pk->pj", B, v))


def noise64(scaling_raw, rotation_raw, opacity_raw, noise, step_scale):
    """The noise step: delta = R (s^2 * (R^T v)), v = noise * gate * step_scale, gate = 1 / (1 + exp(-100 ((1 - o) -
    0.995))).  step_scale is rounded to float32 first (the C ABI takes a float).  Returns a dict:
      delta     [P,3]  the change of xyz
      mag       [P,3]  |R| (s^2 * (|R^T| |v|)): what the roundings of v, s^2 and the two products scale with
      mag_rot   [P,3]  T (s^2 * (|R^T| |v|)) + |R| (s^2 * (T^T |v|)): what the roundings of R's entries scale with
      mag_floor [P,3]  mag with |v| = 2^-126 |noise| step_scale: a gate below float32's normal range may come out as 0"""
    step = float(np.float32(step_scale))
    o = sigmoid64(opacity_raw).reshape(-1, 1)
    gate = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - o) - 0.995)))
    v = f64(noise) * gate * step
    s2 = np.exp(f64(scaling_raw)) ** 2
    R, T = rotation64(rotation_raw)
    aR, av = np.abs(R), np.abs(v)
    vf = 2.0 ** -126 * np.abs(f64(noise)) * abs(step)
    return {"delta": _sandwich(R, s2, R, v), "mag": _sandwich(aR, s2, aR, av),
            "mag_rot": _sandwich(T, s2, aR, av) + _sandwich(aR, s2, T, av), "mag_floor": _sandwich(aR, s2, aR, vf),
            "gate": gate}


def reg64(opacity_raw, scaling_raw, opacity_reg, scale_reg, g=1.0):
    """(value, d value / d opacity_raw [P,1], d value / d scaling_raw [P,3], o [P,1]) of
    opacity_reg * mean(o) + scale_reg * mean(s); the weights are rounded to float32 first (the C ABI takes floats)."""
    wo, ws = float(np.float32(opacity_reg)), float(np.float32(scale_reg))
    o, s = sigmoid64(opacity_raw).reshape(-1, 1), np.exp(f64(scaling_raw))
    P = o.shape[0]
    value = wo * math.fsum(o.ravel()) / P + ws * math.fsum(s.ravel()) / (3 * P)
    return value, g * wo / P * o * (1 - o), g * ws / (3 * P) * s, o


def weights(o32, alive_threshold):
    """w_i = round-to-nearest(o_i 2^30) as Python ints where o_i > alive_threshold (< 0: every row), else 0.  o32: the
    float32 activations.  o 2^30 is exact in double; Python's round is to nearest, ties to even."""
    thr = np.float32(alive_threshold)
    out = []
    for o in np.asarray(o32, dtype=np.float32).ravel():
        alive = True if thr < 0 else bool(o > thr)
        out.append(int(round(float(o) * FX_ONE)) if alive else 0)
    return out


def sample(w, draws):
    """(idx, count, C): for draw r in [0, 2^63), t = (r T) >> 63 and the sample is the smallest i with C_i > t; T == 0
    gives -1 everywhere."""
    C = list(itertools.accumulate(w))
    T = C[-1] if C else 0
    idx, count = [], [0] * len(w)
    for r in draws:
        r = int(r)
        if T == 0:
            idx.append(-1)
            continue
        t = (r * T) >> 63
        i = bisect.bisect_right(C, t)
        idx.append(i)
        count[i] += 1
    return idx, count, C


def draw_for(t, T):
    """The smallest draw r with (r T) >> 63 == t (0 <= t < T)."""
    r = -((-t << 63) // T)
    assert 0 <= r < 1 << 63 and (r * T) >> 63 == t
    return r


def edge_draws(w):
    """Draws whose t is C_i - 1 (the last unit of row i) and C_i (the first unit of the next row with weight) for every
    row with weight that has a zero-weight neighbour, plus t = 0 and t = T - 1."""
    C = list(itertools.accumulate(w))
    T = C[-1]
    ts = {0, T - 1}
    for i, wi in enumerate(w):
        if wi > 0 and ((i > 0 and w[i - 1] == 0) or (i + 1 < len(w) and w[i + 1] == 0)):
            ts.update(t for t in (C[i] - wi - 1, C[i] - wi, C[i] - 1, C[i]) if 0 <= t < T)
    return [draw_for(t, T) for t in sorted(ts)]


def relocation64(o, s, N):
    """The correction of a Gaussian of opacity o and scales s (floats / array) that stands for N copies:
    (o', D, s', new_opacity_raw, new_scaling_raw)."""
    N = min(int(N), NMAX)
    o = float(o)
    op = 1.0 - (1.0 - o) ** (1.0 / N)
    D = 0.0
    for m in range(1, N + 1):
        for k in range(m):
            D += math.comb(m - 1, k) * ((-1.0) ** k / math.sqrt(k + 1)) * op ** (k + 1)
    sp = (o / D) * f64(s)
    oc = min(max(op, 0.005), 1.0 - 2.0 ** -23)
    return op, D, sp, math.log(oc / (1.0 - oc)), np.log(sp)


def coverage_quadrature(amp, sigma, N, intervals=8000, reach=12.0):
    """integral over x of 1 - (1 - amp exp(-x^2 / (2 sigma^2)))^N by the trapezoid rule on [-reach sigma, reach sigma]:
    the integrand is entire and decays like a Gaussian, so the rule converges geometrically -- an evaluation that shares
    nothing with the binomial series."""
    x = np.linspace(-reach * sigma, reach * sigma, intervals + 1)
    a = amp * np.exp(-x * x / (2.0 * sigma * sigma))
    f = -np.expm1(N * np.log1p(-a))
    h = 2.0 * reach * sigma / intervals
    return h * (math.fsum(f) - 0.5 * (f[0] + f[-1]))
