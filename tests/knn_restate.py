"""Restatement of ``distCUDA2`` (``mvs_gaussian_splatting_amd/knn.py``, ``csrc/knn.hip``): the mean squared distance of
every point to its three nearest OTHER points, twice over, and the table of point clouds both test files run.

``dist2_knn3_f64``        the truth: float64 arithmetic on the float32 coordinates, neighbours from scipy's cKDTree.
``dist2_knn3_f32_brute``  the same operation in float32 by brute force, no tree: what a float32 kernel can be expected to
                          give, and the definition of the result for fewer than four points.

The contract for N < 4 (the kernel's ``best[]`` starts at FLT_MAX and a missing neighbour leaves it there):
    N = 1, 2    +inf            (FLT_MAX + FLT_MAX overflows)
    N = 3       (d1 + d2 + FLT_MAX) / 3 in float32: a huge finite number
Upstream ``simple_knn`` initialises its three best distances to FLT_MAX in the same way to our knowledge; upstream is not
available to this project, so that is UNPINNED.

Shared by tests/test_knn_host.py (no GPU) and tests/test_gpu_knn.py; tests/test_gpu_parity.py imports BOUND.
"""
import functools

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
U = 2.0 ** -24            # unit roundoff of float32

# The bar on |float32 result - float64 truth| / truth.  Derived, not tuned; every step is a relative error in units of U
# ("ulp" below), first order, and every quantity from the squares on is non-negative, so no step cancels:
#   dx = q.x - p.x                    1 ulp   (one rounded subtraction of two float32 values)
#   dx * dx                           3 ulp   (the square of a value 1 ulp off is 2 ulp off, rounding it adds 1)
#   dx*dx + dy*dy + dz*dz             5 ulp   (two additions of non-negative terms: each keeps the worst relative
#                                              error of its operands and adds 1)
#   (b0 + b1) + b2                    7 ulp   (two more such additions)
#   / 3                               8 ulp   (one correctly rounded division)
# Choosing the three neighbours by float32 rank and not by float64 rank can only exchange values that agree within the
# 5 ulp of one distance, so the bound on the mean stands.  A fused multiply-add rounds once where the product and the sum
# round twice: contraction only lowers the error.  The bound presumes no subnormal squared distance (CASES keeps every
# non-zero one above 1e-30) and finite coordinates.
BOUND = 8 * U

BOX = 128                 # knn.hip KNN_BOX: sorted points per box
SUPER = 64                # knn.hip KNN_SUPER: boxes per super-box
QUERY_BLOCK = 256         # lanes per block of knn_query_kernel


def _as_f32(points):
    p = np.ascontiguousarray(np.asarray(points), dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {p.shape}")
    return p


def neighbour_dist2_f64(points_f32):
    """-> [N, min(3, N - 1)] float64: the squared distances to the nearest other points, ascending.  The tree only names
    the neighbours; each squared distance is recomputed from the coordinates (no square root in between).  A point that
    coincides with others may not find ITSELF in the first column, but that column holds a zero either way."""
    from scipy.spatial import cKDTree
    p = _as_f32(points_f32).astype(np.float64)
    n = p.shape[0]
    k = min(4, n)
    if n < 2:
        return np.zeros((n, 0))
    _, idx = cKDTree(p).query(p, k=k)
    d2 = ((p[idx] - p[:, None, :]) ** 2).sum(axis=2)
    return np.sort(d2, axis=1)[:, 1:]


def dist2_knn3_f64(points_f32):
    """The float64 truth for N >= 4: the mean of the three smallest squared distances to other points.  With fewer than
    four points there is no third neighbour and no truth: dist2_knn3_f32_brute defines that result."""
    d2 = neighbour_dist2_f64(points_f32)
    if d2.shape[0] < 4:
        raise ValueError("dist2_knn3_f64 needs N >= 4 (the N < 4 contract is dist2_knn3_f32_brute's)")
    return d2.sum(axis=1) / 3.0


def dist2_knn3_f32_brute(points_f32, block_elems=1 << 17):
    """``distCUDA2`` in float32 without a tree, a block of rows against all points at a time: dx*dx + dy*dy + dz*dz with
    every operation rounded to float32 (numpy fuses nothing), the three smallest of a row with the point's own INDEX left
    out (a coincident point counts, at distance 0), missing neighbours FLT_MAX (see the module docstring: unpinned
    against upstream), then (b0 + b1 + b2) / 3 in float32.  -> [N] float32."""
    p = _as_f32(points_f32)
    n = p.shape[0]
    out = np.empty(n, dtype=np.float32)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    rows = max(1, block_elems // max(n, 1))
    t_buf, d_buf = np.empty((rows, n), dtype=np.float32), np.empty((rows, n), dtype=np.float32)
    best = np.empty((3, rows), dtype=np.float32)
    three = np.float32(3.0)
    with np.errstate(over="ignore"):
        for r0 in range(0, n, rows):
            r1 = min(n, r0 + rows)
            m = r1 - r0
            t, d, row = t_buf[:m], d_buf[:m], np.arange(m)
            np.subtract(x[None, :], x[r0:r1, None], out=t)
            np.multiply(t, t, out=d)
            for c in (y, z):
                np.subtract(c[None, :], c[r0:r1, None], out=t)
                np.multiply(t, t, out=t)
                d += t
            d[row, np.arange(r0, r1)] = np.inf                          # the point itself, by index
            for k in range(3):                                          # the smallest, struck out by index, three times
                j = d.argmin(axis=1)
                best[k, :m] = np.minimum(d[row, j], FLT_MAX)            # nothing left: the kernel's initial FLT_MAX
                d[row, j] = np.inf
            out[r0:r1] = ((best[0, :m] + best[1, :m]) + best[2, :m]) / three
    return out


# ---- the case table -----------------------------------------------------------------------------------------------------
def _uniform(rng, n, scale=(4.0, 2.0, 1.0), shift=-1.0):
    return rng.random((n, 3), dtype=np.float32) * np.asarray(scale, dtype=np.float32) + np.float32(shift)


def _size(n):
    """The anisotropic uniform cloud of test_distCUDA2_matches_kdtree at a structural size."""
    return lambda rng: _uniform(rng, n)


def _two_sheets(axis):
    """3 * 8192 + 77 points on two planes 1e-3 apart, symmetric about the middle of the cloud along `axis`; the in-plane
    positions are a jittered grid of spacing 0.05 (points at least 0.03 apart) that both sheets share up to a jitter of
    1e-4.  The nearest neighbour of every point (but the one without a partner) is its partner on the other sheet, whose
    quantised `axis` coordinate is 1023 against 0: every Morton bit of that axis differs, and with axis = 2 that is the
    top bit of the code, so the partner lies in the other half of the sorted order."""
    def make(rng):
        n = 3 * BOX * SUPER + 77
        m = (n + 1) // 2
        side = int(np.ceil(np.sqrt(m)))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), axis=-1).reshape(-1, 2)[:m]
        plane = g * 0.05 + rng.uniform(-0.01, 0.01, size=(m, 2))
        both = np.concatenate([plane, plane[: n - m] + rng.uniform(-1e-4, 1e-4, size=(n - m, 2))])
        pts = np.empty((n, 3))
        pts[:, [a for a in range(3) if a != axis]] = both - 0.05 * side / 2
        pts[:m, axis] = -5e-4
        pts[m:, axis] = 5e-4
        return rng.permutation(pts.astype(np.float32))
    return make


def _lattice(rng):
    """29^3 points on a grid of spacing 1/8 (every coordinate and every squared distance exact in float32): six nearest
    neighbours tie exactly, boxes sit at exactly the third-best distance."""
    a = (np.arange(29, dtype=np.float32) - 14) * np.float32(0.125)
    return rng.permutation(np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3))


def _jittered_lattice(rng):
    """21^3 points of the same grid, each coordinate moved by up to 2e-6: the six nearest neighbours now differ by a few
    1e-5 relative, and so do the faces of the boxes, which lie on the grid's planes.  Whether a box across a face holds
    the third neighbour is decided inside that margin, and opening the wrong one costs a few 1e-6 relative, several
    times the bound: a pruning test or a bounding box that is off by 1e-5 shows on thousands of points."""
    a = (np.arange(21, dtype=np.float64) - 10) * 0.125
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    return rng.permutation((g + rng.uniform(-2e-6, 2e-6, size=g.shape)).astype(np.float32))


def _coincident_block(rng):
    """300 copies of one point of a uniform cloud of 2000: more than two boxes of points at distance 0 from each other."""
    pts = _uniform(rng, 2000)
    return rng.permutation(np.concatenate([pts, np.repeat(pts[777:778], 300, axis=0)]))


def _every_point_twice(rng):
    pts = _uniform(rng, 1500)
    return rng.permutation(np.concatenate([pts, pts]))


def _all_identical(rng):
    return np.tile(np.array([[0.3, -1.7, 2.5]], dtype=np.float32), (500, 1))


def _collapsed_cluster(rng):
    """10 000 points within 1e-4 of the origin (coordinates k * 2^-34, |k| <= 2^19: distinct values 5.8e-11 apart) and 200
    outliers at scale 1e3: the 10-bit quantisation of an extent of several thousand gives the cluster one Morton code."""
    k = rng.integers(-(1 << 19), (1 << 19) + 1, size=(10_000, 3))
    cluster = (k * 2.0 ** -34).astype(np.float32)
    far = (rng.standard_normal((200, 3)) * 1e3).astype(np.float32)
    return rng.permutation(np.concatenate([cluster, far]))


def _collinear(rng):
    pts = np.empty((1500, 3), dtype=np.float32)
    pts[:, 0], pts[:, 2] = 0.25, -1.5
    pts[:, 1] = rng.uniform(-3.0, 3.0, size=1500)
    return pts


def _planar(rng):
    pts = _uniform(rng, 3000)
    pts[:, 2] = 0.5
    return pts


def _offset(rng):
    """Geo-referenced SfM: a jittered 16^3 grid of spacing 1e-2 around (5000, -3000, 800), where one float32 step is up
    to 4.9e-4."""
    a = np.arange(16) - 7.5
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3) * 1e-2
    g = g + rng.uniform(-3e-3, 3e-3, size=g.shape) + np.array([5000.0, -3000.0, 800.0])
    return rng.permutation(g.astype(np.float32))


def _negative_octant(rng):
    """Every coordinate negative: x in (-4.1, -0.1], y in (-2.6, -0.1], z in (-2.0, -0.1]."""
    return -_uniform(rng, 2000, scale=(4.0, 2.5, 1.9), shift=0.1)


def _signed_zeros(rng):
    """Coordinates in [-1, 1] of which three in ten are a zero, +0.0 or -0.0 at random: about 50 points are the origin
    under mixed signs and must count as coincident."""
    pts = _uniform(rng, 2000, scale=(2.0, 2.0, 2.0), shift=-1.0)
    zero = rng.random(pts.shape) < 0.3
    pts[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return pts


SIZES = [1, 2, 3, 4, 5, BOX - 1, BOX, BOX + 1, QUERY_BLOCK - 1, QUERY_BLOCK, QUERY_BLOCK + 1, BOX * SUPER - 1, BOX * SUPER,
         BOX * SUPER + 1, BOX * SUPER + BOX, 2 * BOX * SUPER, 2 * BOX * SUPER + 1]

CASES = {f"uniform_{n}": _size(n) for n in SIZES}
CASES.update({
    "two_sheets_x": _two_sheets(0),
    "two_sheets_z": _two_sheets(2),
    "lattice": _lattice,
    "jittered_lattice": _jittered_lattice,
    "coincident_block": _coincident_block,
    "every_point_twice": _every_point_twice,
    "all_identical": _all_identical,
    "collapsed_cluster": _collapsed_cluster,
    "collinear": _collinear,
    "planar": _planar,
    "offset": _offset,
    "negative_octant": _negative_octant,
    "signed_zeros": _signed_zeros,
})
CASE_NAMES = list(CASES)
SMALL_CASES = [c for c in CASE_NAMES if c in ("uniform_1", "uniform_2", "uniform_3")]
FULL_CASES = [c for c in CASE_NAMES if c not in SMALL_CASES]


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case_points(name):
    """The float32 [N, 3] cloud of a case: seeded by the case's position in the table, computed once, read-only."""
    rng = np.random.default_rng([2024, CASE_NAMES.index(name)])
    return _frozen(_as_f32(CASES[name](rng)))


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """dist2_knn3_f64 of a case with N >= 4: computed once, read-only."""
    return _frozen(dist2_knn3_f64(case_points(name)))


def assert_within_bound(got, truth, what):
    """|got - truth| <= BOUND * truth elementwise, exactly 0 where the truth is 0.  -> the worst error in units of U."""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite result"
    zero = truth == 0
    assert (got[zero] == 0).all(), f"{what}: {int((got[zero] != 0).sum())} results are not exactly 0 where the truth is"
    err = np.abs(got[~zero] - truth[~zero]) / truth[~zero]
    worst = float(err.max() / U) if err.size else 0.0
    print(f"{what}: N = {truth.shape[0]}, {int(zero.sum())} exact zeros, worst error {worst:.2f} ulp (bound {BOUND / U:.0f})")
    if err.size and err.max() > BOUND:
        i = np.flatnonzero(~zero)[int(err.argmax())]
        raise AssertionError(f"{what}: {int((err > BOUND).sum())} results beyond {BOUND / U:.0f} ulp, worst {worst:.1f} ulp "
                             f"at point {i}: got {got[i]!r}, truth {truth[i]!r}")
    return worst
