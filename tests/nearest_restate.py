"""Restatement of the cross-set nearest point (``mvs_gaussian_splatting_amd/geometry_eval.py``, ``csrc/nearest.hip``), twice
over, and the table of (reference, query) clouds both test files run.

``nearest_f32_brute``   the definition: for every query the minimum over the reference of
                        d2 = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)), dx = fl(q.x - r.x), in float32 numpy (which fuses
                        nothing), and the smallest reference index that attains it (``argmin`` returns the first).  The
                        kernel must give these bits and this index.
``nearest_f64``         the truth: float64 arithmetic on the float32 coordinates, the neighbour from scipy's cKDTree.

BOUND: dx carries one rounding, its square two from it and one of its own, the two sums one each: about 5 roundings to
first order, 8 leaves the second-order room (the derivation of ``knn_restate.BOUND``, without the mean of three).

Shared by tests/test_nearest_host.py (no GPU) and tests/test_gpu_nearest.py.
"""
import functools
import math

import numpy as np

import tsdf_restate as T

U = 2.0 ** -24
BOUND = 8 * U
BOX, SUPER = 128, 64          # knn_index.h


def _as_f32(points):
    p = np.ascontiguousarray(np.asarray(points), dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {p.shape}")
    return p


def nearest_f32_brute(query, ref, block_elems=1 << 20):
    """-> (dist2 float32 [Q], nearest int32 [Q], ties int64 [Q]: how many reference points attain the minimum)."""
    q, r = _as_f32(query), _as_f32(ref)
    nq, nr = q.shape[0], r.shape[0]
    d2 = np.full(nq, np.inf, dtype=np.float32)
    idx = np.full(nq, -1, dtype=np.int32)
    ties = np.zeros(nq, dtype=np.int64)
    if nr == 0 or nq == 0:
        return d2, idx, ties
    x, y, z = (np.ascontiguousarray(r[:, a]) for a in range(3))
    rows = max(1, block_elems // nr)
    with np.errstate(over="ignore"):
        for r0 in range(0, nq, rows):
            r1 = min(nq, r0 + rows)
            t = q[r0:r1, 0, None] - x[None, :]
            d = t * t
            t = q[r0:r1, 1, None] - y[None, :]
            d = d + t * t
            t = q[r0:r1, 2, None] - z[None, :]
            d = d + t * t
            assert d.dtype == np.float32
            j = d.argmin(axis=1)
            m = d[np.arange(r1 - r0), j]
            d2[r0:r1], idx[r0:r1] = m, j
            ties[r0:r1] = (d == m[:, None]).sum(axis=1)
    return d2, idx, ties


def dist2_f64(query, ref, idx):
    """The float64 squared distance of every query to reference point idx[.]."""
    q, r = _as_f32(query).astype(np.float64), _as_f32(ref).astype(np.float64)
    return ((q - r[np.asarray(idx, dtype=np.int64)]) ** 2).sum(axis=1)


def nearest_f64(query, ref):
    """-> (dist2 float64 [Q], an index that attains it).  The tree only names the neighbour; the squared distance is
    recomputed from the coordinates."""
    from scipy.spatial import cKDTree
    q, r = _as_f32(query).astype(np.float64), _as_f32(ref).astype(np.float64)
    _, idx = cKDTree(r).query(q, k=1)
    return dist2_f64(query, ref, idx), idx


# ---- the case table: name -> (ref [R,3], query [Q,3]) -------------------------------------------------------------------
def _uniform(rng, n, scale=(4.0, 2.0, 1.0), shift=-1.0):
    return rng.random((n, 3), dtype=np.float32) * np.asarray(scale, dtype=np.float32) + np.float32(shift)


def _sizes(nr, nq):
    return lambda rng: (_uniform(rng, nr), _uniform(rng, nq))


def _self(rng):
    ref = _uniform(rng, 3000)
    return ref, ref.copy()


def _duplicated(rng):
    """Every reference point twice, shuffled: each query (the points themselves and points nearby) has a two-way tie."""
    pts = _uniform(rng, 1500)
    ref = rng.permutation(np.concatenate([pts, pts]))
    return ref, np.concatenate([pts[:700], _uniform(rng, 700)])


def _coincident(rng):
    ref = np.tile(np.array([[0.3, -1.7, 2.5]], dtype=np.float32), (500, 1))
    return ref, np.concatenate([ref[:3], _uniform(rng, 400, scale=(6.0, 6.0, 6.0), shift=-3.0)])


def _collinear(rng):
    ref = np.zeros((1500, 3), dtype=np.float32)
    ref[:, 0] = rng.uniform(-3.0, 3.0, size=1500)
    return ref, _uniform(rng, 600, scale=(8.0, 2.0, 2.0), shift=-1.0) - np.float32([3.0, 0.0, 0.0])


def _lattice(rng):
    """12^3 points of spacing 1/4, shuffled, queried at the 11^3 cell centres: every coordinate and distance is exact in
    float32 and eight corners tie."""
    a = (np.arange(12, dtype=np.float32) - 6) * np.float32(0.25)
    ref = rng.permutation(np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3))
    c = a[:-1] + np.float32(0.125)
    return ref, rng.permutation(np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3))


def _two_sheets(rng):
    """8192 + 300 points on the planes z = -+5e-4 (a jittered grid of spacing 0.05 each), queries on z = 0 and just off it:
    the nearest point lies on either sheet, whose quantised z is 0 against 1023 -- the other half of the sorted order."""
    n = BOX * SUPER + 300
    m = n // 2
    side = int(np.ceil(np.sqrt(m)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)
    ref = np.empty((n, 3))
    ref[:m, :2] = g[:m] * 0.05 + rng.uniform(-0.01, 0.01, size=(m, 2))
    ref[m:, :2] = g[:n - m] * 0.05 + rng.uniform(-0.01, 0.01, size=(n - m, 2))
    ref[:m, 2], ref[m:, 2] = -5e-4, 5e-4
    q = np.empty((700, 3))
    q[:, :2] = rng.uniform(0.0, 0.05 * side, size=(700, 2))
    q[:, 2] = np.where(rng.random(700) < 0.5, 0.0, rng.uniform(-2e-4, 2e-4, size=700))
    return rng.permutation(ref.astype(np.float32)), q.astype(np.float32)


def _cluster_and_outliers(rng):
    """4000 points within 1e-3 of a centre and 100 outliers at scale 100: the cluster shares a handful of Morton cells."""
    centre = np.array([0.4, -0.2, 0.1])
    cluster = centre + rng.uniform(-1e-3, 1e-3, size=(4000, 3))
    far = rng.standard_normal((100, 3)) * 100.0
    ref = rng.permutation(np.concatenate([cluster, far]).astype(np.float32))
    q = np.concatenate([centre + rng.uniform(-2e-3, 2e-3, size=(300, 3)), far[:60] + rng.uniform(-1.0, 1.0, size=(60, 3)),
                        rng.standard_normal((140, 3)) * 100.0])
    return ref, q.astype(np.float32)


def _far_queries(rng):
    """Queries 1000 box sizes (of a 2000-point cloud in a unit cube: boxes of ~0.4) and more outside the bounding box, on
    every side: all of them clamp to face cells of the Morton frame."""
    ref = _uniform(rng, 2000, scale=(1.0, 1.0, 1.0), shift=0.0)
    d = rng.standard_normal((300, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    q = 0.5 + d * rng.uniform(800.0, 4000.0, size=(300, 1))
    q[:6] = 0.5 + np.array([[1e3, 0, 0], [-1e3, 0, 0], [0, 1e3, 0], [0, -1e3, 0], [0, 0, 1e3], [0, 0, -1e3]])
    return ref, q.astype(np.float32)


CASES = {
    "R1": _sizes(1, 5),
    "R127": _sizes(BOX - 1, 300), "R128": _sizes(BOX, 300), "R129": _sizes(BOX + 1, 300),
    "R8192": _sizes(BOX * SUPER, 300), "R8193": _sizes(BOX * SUPER + 1, 300),
    "Q1": _sizes(1000, 1), "Q255": _sizes(1000, 255), "Q257": _sizes(1000, 257),
    "Q0": _sizes(1000, 0), "R0": _sizes(0, 10),
    "self": _self,
    "duplicated": _duplicated,
    "coincident": _coincident,
    "collinear": _collinear,
    "lattice_centres": _lattice,
    "two_sheets": _two_sheets,
    "cluster_and_outliers": _cluster_and_outliers,
    "far_queries": _far_queries,
    "uniform_20000x10000": _sizes(10000, 20000),
}
CASE_NAMES = list(CASES)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    """(ref float32 [R,3], query float32 [Q,3]) of a case: seeded by its position in the table, computed once, read-only."""
    rng = np.random.default_rng([2025, CASE_NAMES.index(name)])
    ref, query = CASES[name](rng)
    return _frozen(_as_f32(ref)), _frozen(_as_f32(query))


@functools.lru_cache(maxsize=None)
def case_brute(name):
    """nearest_f32_brute of a case: computed once, read-only."""
    ref, query = case(name)
    return tuple(_frozen(a) for a in nearest_f32_brute(query, ref))


def has_ties(name):
    return bool((case_brute(name)[2] > 1).any())


# ---- the clouds of the evaluate_points check -----------------------------------------------------------------------------
EVAL_SAMPLES, EVAL_GT = 6000, 5000
EVAL_SHIFT = (1.0 / 3.0, 0.0, 0.0)           # a third of the sphere volume's voxel
EVAL_THRESHOLDS = (0.15, 0.3, 0.45)
EVAL_MARGIN = 1e-5


def sphere_gt_points(n=EVAL_GT):
    """n points of the analytic sphere of tsdf_restate.sphere_field (a Fibonacci spiral), float32."""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * math.pi * (3.0 - math.sqrt(5.0))
    rho = np.sqrt(1.0 - z * z)
    p = np.stack((rho * np.cos(phi), rho * np.sin(phi), z), axis=1) * T.SPHERE_R + np.asarray(T.SPHERE_C)
    return p.astype(np.float32)


def evaluate_f64(pred, gt, thresholds=(), max_dist=None):
    """evaluate_points in float64 with cKDTree: the truth.  -> (result dict, all distances pred->gt and gt->pred)."""
    d_p = np.sqrt(nearest_f64(pred, gt)[0])
    d_g = np.sqrt(nearest_f64(gt, pred)[0])
    out = {}
    for key, d in (("accuracy", d_p), ("completeness", d_g)):
        kept = d[d <= max_dist] if max_dist is not None else d
        out[key] = float(kept.mean())
        out["dropped_" + ("pred" if key == "accuracy" else "gt")] = 1.0 - kept.size / d.size
    out["chamfer"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["thresholds"] = []
    for tau in thresholds:
        p, r = float((d_p <= tau).sum()) / d_p.size, float((d_g <= tau).sum()) / d_g.size
        out["thresholds"].append({"tau": tau, "precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r else 0.0})
    return out, np.concatenate([d_p, d_g])


def assert_thresholds_are_clear(dists, thresholds, what):
    """No distance within EVAL_MARGIN relative of a threshold: a float32 distance 3e-7 off the truth falls on the same
    side of every threshold, so the counts must be exactly the truth's."""
    for tau in thresholds:
        gap = float(np.abs(dists / tau - 1.0).min())
        print(f"{what}: closest distance to tau = {tau} is {gap:.2e} relative away (needs > {EVAL_MARGIN})")
        assert gap > EVAL_MARGIN, (what, tau, gap)
