"""distCUDA2, the part that runs without a GPU: the two restatements of tests/knn_restate.py against each other on every
case of the table, which proves the reference and the bound the GPU test (tests/test_gpu_knn.py) holds the kernel to.

  - float32 brute force against the float64 truth: |f32 - f64| <= 8 * 2^-24 * f64 on every point of every case with
    N >= 4, exactly 0 where the truth is 0 (the derivation stands next to knn_restate.BOUND).  A case that misses the
    bound here is ill-posed (subnormal distances, say): the case changes, never the bound;
  - the contract for N < 4;
  - the brute force is permutation-equivariant bit for bit, as the kernel is required to be;
  - every case is what its name says: finite float32, no non-zero squared distance below 1e-30, sizes on the kernel's
    structural boundaries, partners across the sheets, one Morton code for the collapsed cluster, exact ties on the lattice,
    near ties on the jittered one.
"""
import functools
import os
import re

import numpy as np
import pytest

import knn_restate as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN_HIP = os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "knn.hip")


@functools.lru_cache(maxsize=None)
def _brute(name):
    b = K.dist2_knn3_f32_brute(K.case_points(name))
    b.setflags(write=False)
    return b


def _morton_codes(p):
    """knn_morton_kernel restated: 10 bits per axis over the cloud's extent, x in the lowest bit of every triple."""
    lo, hi = p.min(axis=0), p.max(axis=0)
    t = (p - lo) / np.maximum(hi - lo, np.float32(1e-30))
    q = np.clip(t * np.float32(1023.0), 0, 1023).astype(np.uint32)
    code = np.zeros(p.shape[0], dtype=np.uint32)
    for bit in range(10):
        for a in range(3):
            code |= ((q[:, a] >> bit) & 1) << np.uint32(3 * bit + a)
    return code


def test_the_table_sits_on_the_kernels_structural_sizes():
    src = open(KNN_HIP).read()
    assert int(re.search(r"constexpr int KNN_BOX = (\d+);", src).group(1)) == K.BOX
    assert int(re.search(r"constexpr int KNN_SUPER = (\d+);", src).group(1)) == K.SUPER
    assert re.search(r"__launch_bounds__\((\d+)\) void knn_query_kernel", src).group(1) == str(K.QUERY_BLOCK)
    assert K.SIZES == [1, 2, 3, 4, 5, 127, 128, 129, 255, 256, 257, 8191, 8192, 8193, 8192 + 128, 16384, 16385]
    for n in K.SIZES:
        assert K.case_points(f"uniform_{n}").shape == (n, 3)
    assert K.case_points("two_sheets_z").shape[0] == 3 * 8192 + 77 and K.case_points("lattice").shape[0] == 29 ** 3
    assert max(K.case_points(c).shape[0] for c in K.CASE_NAMES) <= 25_000


@pytest.mark.parametrize("case", K.CASE_NAMES)
def test_case_is_well_posed(case):
    """Finite float32 input, read-only, reproducible; distinct points are more than 1e-15 apart, so no squared distance
    is subnormal (and none overflows: coordinates stay far below 1e18)."""
    from scipy.spatial import cKDTree
    p = K.case_points(case)
    assert p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 3 and not p.flags.writeable
    assert np.isfinite(p).all() and np.abs(p).max() < 1e6
    rng = np.random.default_rng([2024, K.CASE_NAMES.index(case)])
    assert np.array_equal(K.CASES[case](rng), p)
    u = np.unique(p.astype(np.float64) + 0.0, axis=0)                  # + 0.0: -0.0 and +0.0 are one point
    if u.shape[0] > 1:
        d, _ = cKDTree(u).query(u, k=2)
        assert (d[:, 1] ** 2).min() > 1e-30, (d[:, 1] ** 2).min()


@pytest.mark.parametrize("case", K.FULL_CASES)
def test_float32_restatement_is_within_the_bound_of_float64(case):
    worst = K.assert_within_bound(_brute(case), K.case_truth(case), f"f32 brute force, {case}")
    assert worst <= K.BOUND / K.U


def test_fewer_than_four_points_follow_the_contract():
    """N = 1, 2: +inf.  N = 3: (d1 + d2 + FLT_MAX) / 3 in float32, finite, and since d1 + d2 is far below half a float32
    step of FLT_MAX (2^103) it is FLT_MAX / 3 bit for bit.  N = 0: an empty result."""
    assert K.dist2_knn3_f32_brute(np.zeros((0, 3), np.float32)).shape == (0,)
    for name, n in (("uniform_1", 1), ("uniform_2", 2)):
        b = _brute(name)
        assert b.shape == (n,) and b.dtype == np.float32 and np.isposinf(b).all()
    b = _brute("uniform_3")
    d = K.neighbour_dist2_f64(K.case_points("uniform_3")).astype(np.float32)
    assert d.shape == (3, 2) and (d > 0).all()
    with np.errstate(over="ignore"):
        want = ((d[:, 0] + d[:, 1]) + K.FLT_MAX) / np.float32(3.0)
    assert b.dtype == np.float32 and np.isfinite(b).all()
    assert np.array_equal(b.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(b.view(np.uint32), np.full(3, K.FLT_MAX / np.float32(3.0)).view(np.uint32))
    # three coincident points: 0 + 0 + FLT_MAX
    assert np.array_equal(K.dist2_knn3_f32_brute(np.ones((3, 3), np.float32)), np.full(3, K.FLT_MAX / np.float32(3.0)))
    with pytest.raises(ValueError):
        K.dist2_knn3_f64(K.case_points("uniform_3"))


@pytest.mark.parametrize("case", ["uniform_257", "coincident_block", "every_point_twice", "signed_zeros", "collapsed_cluster"])
def test_float32_restatement_is_permutation_equivariant(case):
    p, b = K.case_points(case), _brute(case)
    n = p.shape[0]
    for perm in (np.random.default_rng(n).permutation(n), np.arange(n)[::-1]):
        assert np.array_equal(K.dist2_knn3_f32_brute(p[perm]).view(np.uint32), b[perm].view(np.uint32))


def test_row_blocking_does_not_change_the_restatement():
    p = K.case_points("coincident_block")
    assert np.array_equal(K.dist2_knn3_f32_brute(p, block_elems=1), _brute("coincident_block"))
    assert np.array_equal(K.dist2_knn3_f32_brute(p, block_elems=1 << 24), _brute("coincident_block"))


@pytest.mark.parametrize("axis", [0, 2])
def test_two_sheets_pair_every_point_across_the_gap(axis):
    """The nearest neighbour is the partner on the other sheet (about 1e-3 away, the next one at least 0.03), the sheets
    quantise to 0 and 1023 along their axis, and for axis 2 that puts the partners in different halves of the code range."""
    from scipy.spatial import cKDTree
    p = K.case_points(f"two_sheets_{'xyz'[axis]}")
    p64 = p.astype(np.float64)
    d, idx = cKDTree(p64).query(p64, k=3)
    paired = d[:, 1] < 1.2e-3
    assert paired.sum() >= p.shape[0] - 1 and (d[paired, 2] > 0.029).all()
    assert (np.sign(p[idx[paired, 1], axis]) == -np.sign(p[paired, axis])).all()
    assert sorted(np.unique(p[:, axis]).tolist()) == [np.float32(-5e-4), np.float32(5e-4)]
    code = _morton_codes(p)
    top = (code >> np.uint32(27 + axis)) & 1
    assert (top[idx[paired, 1]] != top[paired]).all()
    if axis == 2:                                   # the top bit of the code: partners are half the sorted order apart
        rank = np.empty(p.shape[0], dtype=np.int64)
        rank[np.argsort(code, kind="stable")] = np.arange(p.shape[0])
        assert (np.abs(rank[idx[paired, 1]] - rank[paired]) > K.BOX).all()
        assert np.mean(rank[idx[paired, 1]] // (K.BOX * K.SUPER) != rank[paired] // (K.BOX * K.SUPER)) > 0.6


def test_structured_cases_have_the_structure_they_claim():
    # lattice: the six nearest neighbours tie exactly, in float64 and in float32
    t = K.case_truth("lattice")
    assert (t == 0.125 ** 2).all() and (_brute("lattice") == np.float32(0.125 ** 2)).all()
    # jittered lattice: ranks 3 and 4 apart by more than the bound allows to confuse, and by far less than 1e-4
    p = K.case_points("jittered_lattice").astype(np.float64)
    from scipy.spatial import cKDTree
    d, _ = cKDTree(p).query(p, k=5)
    gap = (d[:, 4] ** 2 - d[:, 3] ** 2) / (3 * K.case_truth("jittered_lattice"))
    assert np.mean((gap > 2 * K.BOUND) & (gap < 3e-5)) > 0.8
    # collapsed cluster: one Morton code for the 10 000, so its boxes are runs of the stable sort
    p = K.case_points("collapsed_cluster")
    near = np.abs(p).max(axis=1) < 1e-4
    assert near.sum() == 10_000 and np.linalg.norm(p[near].astype(np.float64), axis=1).max() < 1e-4
    assert np.unique(_morton_codes(p)[near]).size == 1
    # coincident points: a block of 301, every point twice, all 500 identical
    p = K.case_points("coincident_block")
    assert (p == p[np.flatnonzero(K.case_truth("coincident_block") == 0)[0]]).all(axis=1).sum() == 301 > 2 * K.BOX
    assert (K.neighbour_dist2_f64(K.case_points("every_point_twice"))[:, 0] == 0).all()
    assert (K.neighbour_dist2_f64(K.case_points("every_point_twice"))[:, 1] > 0).all()
    assert (K.case_truth("all_identical") == 0).all() and np.ptp(K.case_points("all_identical"), axis=0).max() == 0
    # degenerate extents
    assert np.ptp(K.case_points("collinear")[:, [0, 2]], axis=0).max() == 0 and np.ptp(K.case_points("planar")[:, 2]) == 0
    # offset, negative octant, signed zeros
    p = K.case_points("offset")
    assert np.abs(p.mean(axis=0) - [5000, -3000, 800]).max() < 0.01 and 5e-5 < np.median(K.case_truth("offset")) < 2e-4
    assert (K.case_points("negative_octant") < 0).all()
    p = K.case_points("signed_zeros")
    zeros = p == 0
    assert (zeros & np.signbit(p)).sum() > 100 and (zeros & ~np.signbit(p)).sum() > 100
    assert zeros.all(axis=1).sum() >= 4 and (K.case_truth("signed_zeros")[zeros.all(axis=1)] == 0).all()
