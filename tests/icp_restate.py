"""Restatement of the registration layer of ``mvs_gaussian_splatting_amd/geometry_eval.py`` (``csrc/icp.hip``,
``csrc/icp_math.h``) in numpy float64, and the clouds both test files run.

``transform``           ``float32(((m0 x + m1 y) + m2 z) + m3)`` per axis: numpy fuses nothing, one rounding at the end.
``step``                the transformed source, its correspondences from ``nearest_restate.nearest_f32_brute`` (float32:
                        indices and dist2 are the bits of the device query), the 17 terms of every accepted pair in the
                        op order of icp_math.h, and their sums with ``math.fsum`` (exactly rounded), next to the sums of
                        the terms' absolute values that the bound needs.
``BOUND``               a device sum may differ from the fsum value by ``(n + 8) 2^-53 sum |term|``, n = accepted pairs.
                        Both sides add the SAME float64 terms (tests/icp_host_check.cpp shows the kernel's body gives the
                        restatement's term bits), so only the order of the additions differs: any order of n - 1 float64
                        additions is within ``(n - 1) u sum |term|`` of the exact sum to first order (Higham, Accuracy
                        and Stability, eq. 4.4), u = 2^-53; fsum's own rounding adds ``u |sum|``; the remaining 8 u is
                        second-order room.  Derived, not measured.
``registration``        Open3D's loop on top of ``step`` with the package's ``estimate_similarity`` (host float64 code).
``voxel_down_sample``   cells by float64 floor, keys ``ix << 42 | iy << 21 | iz``, rows in ascending key, each the float64
                        sum of its points in ascending index divided by their number and rounded once.
``voxel_cells``         a dictionary-of-cells reference for it, written the other way round.

Shared by tests/test_icp_host.py (no GPU) and tests/test_gpu_icp.py.
"""
import functools
import math

import numpy as np

import nearest_restate as NR

U53 = 2.0 ** -53
TERMS = 17


def transform(points, T):
    p = np.ascontiguousarray(np.asarray(points), dtype=np.float32).astype(np.float64)
    M = np.asarray(T, dtype=np.float64)
    out = np.empty(p.shape, dtype=np.float32)
    for a in range(3):
        v = M[a, 0] * p[:, 0]
        v = v + M[a, 1] * p[:, 1]
        v = v + M[a, 2] * p[:, 2]
        v = v + M[a, 3]
        out[:, a] = v.astype(np.float32)
    return out


def thr2(max_dist):
    with np.errstate(over="ignore"):
        return np.float32(float(max_dist) * float(max_dist))


def pair_terms(q, r, dist2, cq, cr):
    """-> [n, 17] float64: the terms of icp_math.h's icp_pair_terms for the pairs (q[i], r[i])."""
    a = np.asarray(q, dtype=np.float32).astype(np.float64) - np.asarray(cq, dtype=np.float64)
    b = np.asarray(r, dtype=np.float32).astype(np.float64) - np.asarray(cr, dtype=np.float64)
    t = np.empty((a.shape[0], TERMS))
    t[:, 0:3], t[:, 3:6] = a, b
    for i in range(3):
        for j in range(3):
            t[:, 6 + 3 * i + j] = a[:, i] * b[:, j]
    t[:, 15] = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    t[:, 16] = np.asarray(dist2, dtype=np.float32).astype(np.float64)
    return t


class Step:
    """One evaluation: count, the fsum of each of the 17 terms, the fsum of their absolute values, and what led there."""

    def __init__(self, q, dist2, nearest, accepted, terms, cq, cr):
        self.q, self.dist2, self.nearest, self.accepted = q, dist2, nearest, accepted
        self.count = int(accepted.sum())
        self.sums = np.array([math.fsum(terms[:, k]) for k in range(TERMS)])
        self.abs_sums = np.array([math.fsum(np.abs(terms[:, k])) for k in range(TERMS)])
        self.cq, self.cr = np.asarray(cq, dtype=np.float64), np.asarray(cr, dtype=np.float64)
        self.num_source = int(q.shape[0])

    @property
    def bound(self):
        return (self.count + 8) * U53 * self.abs_sums

    def icp_sums(self):
        from mvs_gaussian_splatting_amd.geometry_eval import IcpSums
        s = self.sums
        return IcpSums(self.count, s[0:3].copy(), s[3:6].copy(), s[6:15].reshape(3, 3).copy(), float(s[15]), float(s[16]),
                       self.cq.copy(), self.cr.copy(), self.num_source)


def accumulate(q, dist2, nearest, target, t2, cq=(0, 0, 0), cr=(0, 0, 0)):
    target = np.asarray(target, dtype=np.float32).reshape(-1, 3)
    nearest = np.asarray(nearest, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        accepted = (np.asarray(dist2, dtype=np.float32) <= np.float32(t2)) & (nearest >= 0) & (nearest < target.shape[0])
    terms = pair_terms(q[accepted], target[nearest[accepted]], dist2[accepted], cq, cr)
    return Step(q, dist2, nearest, accepted, terms, cq, cr)


def step(source, target, T, max_dist, pivots=None):
    cq, cr = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) if pivots is None else pivots
    q = transform(source, T)
    dist2, nearest, _ = NR.nearest_f32_brute(q, target)
    return accumulate(q, dist2, nearest, target, thr2(max_dist), cq, cr)


def centred_moments(st):
    """H = sum a b^T - (sum a)(sum b)^T / n of a Step: what estimate_similarity decomposes, whatever the pivots."""
    s = st.sums
    return s[6:15].reshape(3, 3) - np.outer(s[0:3], s[3:6]) / st.count


class Result:
    def __init__(self, T, fitness, rmse, iterations, converged):
        self.transformation, self.fitness, self.inlier_rmse = T, fitness, rmse
        self.iterations, self.converged = iterations, converged


def registration(source, target, max_dist, init=None, with_scaling=False, max_iterations=30, relative_fitness=1e-6,
                 relative_rmse=1e-6):
    from mvs_gaussian_splatting_amd.geometry_eval import estimate_similarity
    source = np.ascontiguousarray(source, dtype=np.float32)
    target = np.ascontiguousarray(target, dtype=np.float32)
    M = np.eye(4) if init is None else np.array(init, dtype=np.float64)
    s64, t64 = source.astype(np.float64), target.astype(np.float64)
    c_src, c_tgt = 0.5 * (s64.min(axis=0) + s64.max(axis=0)), 0.5 * (t64.min(axis=0) + t64.max(axis=0))
    st = step(source, target, M, max_dist, (M[:3, :3] @ c_src + M[:3, 3], c_tgt))
    fit = lambda s: s.count / s.num_source                                          # noqa: E731
    rmse = lambda s: math.sqrt(s.sums[16] / s.count) if s.count else 0.0           # noqa: E731
    iterations, converged = 0, False
    for _ in range(max_iterations):
        if st.count < 3:
            break
        update = estimate_similarity(st.icp_sums(), with_scaling=with_scaling)
        M = update @ M
        iterations += 1
        mean_q, mean_r = st.cq + st.sums[0:3] / st.count, st.cr + st.sums[3:6] / st.count
        before = st
        st = step(source, target, M, max_dist, (update[:3, :3] @ mean_q + update[:3, 3], mean_r))
        if abs(fit(before) - fit(st)) < relative_fitness and abs(rmse(before) - rmse(st)) < relative_rmse:
            converged = True
            break
    return Result(M, fit(st), rmse(st), iterations, converged)


# ---- voxel down-sampling ---------------------------------------------------------------------------------------------------
def default_origin(points, h):
    p = np.asarray(points, dtype=np.float32)
    return p.min(axis=0).astype(np.float64) - float(h) / 2.0


def cell_index(points, h, origin):
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    idx = np.floor((p - np.asarray(origin, dtype=np.float64)) / float(h))
    assert (idx >= 0).all() and (idx < 2 ** 21).all()
    return idx.astype(np.int64)


def voxel_down_sample(points, h, origin=None):
    """-> (rows float32 [K,3] in ascending cell key, keys int64 [K])."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    if p.shape[0] == 0:
        return np.empty((0, 3), dtype=np.float32), np.empty(0, dtype=np.int64)
    origin = default_origin(p, h) if origin is None else origin
    i = cell_index(p, h, origin)
    key = (i[:, 0] << 42) | (i[:, 1] << 21) | i[:, 2]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    heads = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    ends = np.concatenate([heads[1:], [ks.size]])
    out = np.empty((heads.size, 3), dtype=np.float32)
    for c, (lo, hi) in enumerate(zip(heads, ends)):
        acc = p[order[lo]].astype(np.float64)
        for m in order[lo + 1:hi]:
            acc = acc + p[m].astype(np.float64)
        out[c] = (acc / float(hi - lo)).astype(np.float32) if hi - lo > 1 else p[order[lo]]
    return out, ks[heads]


def voxel_cells(points, h, origin=None):
    """The reference written the other way round: a dictionary from the cell's index triple to its member indices (in the
    order they come), read out in the order of the triples -> (means float64 [K,3], triples)."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    origin = default_origin(p, h) if origin is None else origin
    cells = {}
    for n, row in enumerate(p):
        triple = tuple(int(math.floor((float(x) - float(o)) / float(h))) for x, o in zip(row, origin))
        cells.setdefault(triple, []).append(n)
    triples = sorted(cells)
    means = np.array([[math.fsum(float(p[m, a]) for m in cells[t]) / len(cells[t]) for a in range(3)] for t in triples])
    return means, triples


# ---- the clouds --------------------------------------------------------------------------------------------------------------
def similarity(rotvec_deg, shift, scale):
    """4x4 float64 of a rotation (axis * angle in degrees, Rodrigues), a scale and a shift."""
    r = np.radians(np.asarray(rotvec_deg, dtype=np.float64))
    angle = float(np.linalg.norm(r))
    T = np.eye(4)
    if angle > 0:
        k = r / angle
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    T[:3, :3] *= float(scale)
    T[:3, 3] = shift
    return T


def about(T, centre):
    """The similarity that does to the points around `centre` what T does to those around the origin."""
    c = np.asarray(centre, dtype=np.float64)
    out = np.array(T, dtype=np.float64)
    out[:3, 3] = c - out[:3, :3] @ c + out[:3, 3]
    return out


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def asymmetric_cloud(n=2000, seed=7, offset=0.0):
    """n points with no symmetry: a 4 x 2 x 1 box filled uniformly, a denser lump in one corner and a tilted sheet."""
    rng = np.random.default_rng([2026, seed])
    k = n // 4
    box = rng.random((n - 2 * k, 3)) * [4.0, 2.0, 1.0]
    lump = rng.normal(0.0, 0.15, size=(k, 3)) + [3.3, 0.4, 0.8]
    uv = rng.random((k, 2))
    sheet = np.stack([uv[:, 0] * 2.0, uv[:, 1] * 1.5 + 0.5, 1.2 + 0.4 * uv[:, 0] + 0.2 * uv[:, 1] ** 2], axis=1)
    p = rng.permutation(np.concatenate([box, lump, sheet])) + float(offset)
    return _frozen(p.astype(np.float32))


def extent(points):
    p = np.asarray(points, dtype=np.float64)
    return float(np.linalg.norm(p.max(axis=0) - p.min(axis=0)))


@functools.lru_cache(maxsize=None)
def registration_case(with_scaling=True, n=2000):
    """(source, target, T_true, max_dist): target = float32(T_true source); rotation 3 degrees about a skew axis, a shift
    of 2 % of the extent, scale 1.02 (1 when not with_scaling).  T_true turns about the cloud's centre."""
    src = asymmetric_cloud(n)
    ext = extent(src)
    axis = np.array([0.3, -0.5, 0.81])
    R = similarity(3.0 * axis / np.linalg.norm(axis), (0, 0, 0), 1.02 if with_scaling else 1.0)
    c = src.astype(np.float64).mean(axis=0)
    shift = 0.02 * ext * np.array([0.6, 0.64, -0.48])
    T = R.copy()
    T[:3, 3] = c - R[:3, :3] @ c + shift
    return src, _frozen(transform(src, T)), _frozen(T), 0.1 * ext


@functools.lru_cache(maxsize=None)
def registration_restated(with_scaling=True):
    src, tgt, T, max_dist = registration_case(with_scaling)
    return registration(src, tgt, max_dist, with_scaling=with_scaling)


def max_point_error(T_est, T_true, points):
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    d = (p @ (np.asarray(T_est)[:3, :3] - np.asarray(T_true)[:3, :3]).T) + (np.asarray(T_est)[:3, 3] - np.asarray(T_true)[:3, 3])
    return float(np.linalg.norm(d, axis=1).max())
