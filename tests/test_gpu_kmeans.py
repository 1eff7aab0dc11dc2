"""GPU checks of the k-means layer (csrc/kmeans.hip; compress.kmeans_assign / kmeans_update / kmeans)
against the numpy restatement (tests/kmeans_restate.py): the assignment bit for bit and within the derived float64 gap,
padding, ties, repeatability, the two paths against each other, the centre update bit for bit, and Lloyd's iteration
as a whole (its init and every codebook of its trajectory bit for bit, monotone up to the stated slack, lossless on few
distinct rows).

The codebook stage of the kernel is 128 codes, its tile 32: K = 4097 is 32 full stages and a last stage of one code,
K = 33 and K = 100 end inside a tile, K = 1 and 2 inside the first, K = 128 and 256 fill their last stage, K = 65536 is
the limit.  The first ten CASES leave D = 17..32 (one of the five instantiations of the kernel), the other edges of the
dispatch on D, and every N that ends past wave 0 of its workgroup unvisited: ``R.ASSIGN_EDGE_CASES`` names those, and
tests/test_kmeans_host.py checks which instantiation each reaches."""
import functools

import numpy as np
import pytest
import torch

import kmeans_restate as R
from mvs_gaussian_splatting_amd.compress import _distinct_rows, kmeans, kmeans_assign, kmeans_update

pytestmark = pytest.mark.gpu

#          N    K     D
CASES = [(1, 1, 1), (31, 2, 3), (33, 33, 9), (257, 100, 45), (33, 4097, 63), (257, 4097, 4), (31, 100, 48),
         (257, 33, 64), (33, 4097, 1), (257, 2, 45)] + [c[:3] for c in R.ASSIGN_EDGE_CASES]
RANGES = ("unit", "wide")


@functools.lru_cache(maxsize=None)
def case(N, K, D, spread):
    """x, codebook and the restatement's (index, dist2), computed once.  Half of the codes are perturbed rows of x, so the
    nearest code is often a close call; "wide" scales every row of both by 10^u, u uniform in [-2, 2]."""
    rng = np.random.default_rng(1000 * N + 10 * K + D)
    x = rng.standard_normal((N, D)).astype(np.float32)
    cb = rng.standard_normal((K, D)).astype(np.float32)
    near = rng.integers(0, N, size=K)
    cb[::2] = (x[near] + 1e-3 * rng.standard_normal((K, D)).astype(np.float32))[::2]
    if spread == "wide":
        x *= (10.0 ** rng.uniform(-2, 2, size=(N, 1))).astype(np.float32)
        cb *= (10.0 ** rng.uniform(-2, 2, size=(K, 1))).astype(np.float32)
    index, dist2 = R.assign(x, cb)
    return x, cb, index, dist2


def run(x, cb, dev, path=None):
    index, dist2 = kmeans_assign(torch.from_numpy(np.ascontiguousarray(x)).to(dev),
                                 torch.from_numpy(np.ascontiguousarray(cb)).to(dev), path=path)
    assert index.dtype == torch.int32 and dist2.dtype == torch.float32 and index.shape == dist2.shape == (len(x),)
    return index.cpu().numpy(), dist2.cpu().numpy()


@pytest.mark.parametrize("spread", RANGES)
@pytest.mark.parametrize("N,K,D", CASES)
def test_assignment_is_the_restatements_bit_for_bit(gpu_device, N, K, D, spread):
    x, cb, want_index, want_dist2 = case(N, K, D, spread)
    index, dist2 = run(x, cb, gpu_device)
    assert index.min() >= 0 and index.max() < K
    assert np.array_equal(index, want_index), f"{int((index != want_index).sum())} of {N} indices differ from the fmaf chain"
    assert np.array_equal(dist2.view(np.uint32), want_dist2.view(np.uint32)), "dist2 differs in its float32 bits"


@pytest.mark.parametrize("spread", RANGES)
@pytest.mark.parametrize("N,K,D", CASES)
def test_chosen_code_is_within_the_derived_gap_of_the_true_nearest(gpu_device, N, K, D, spread):
    x, cb, _, _ = case(N, K, D, spread)
    index, _ = run(x, cb, gpu_device)
    nearest, d = R.brute(x, cb)
    rows = np.arange(N)
    gap = d[rows, index] - d[rows, nearest]
    bound = R.gap_bound(x, cb, index, nearest)
    print(f"N={N} K={K} D={D} {spread}: largest gap / bound = {float((gap / np.maximum(bound, 1e-300)).max()):.3g}, "
          f"{int((index != nearest).sum())} points not at the float64 nearest")
    assert (gap >= 0).all() and (gap <= bound).all()


def test_padded_codes_never_win_a_codebook_far_from_the_origin(gpu_device):
    rng = np.random.default_rng(7)
    K, D, N = 33, 9, 257
    cb = rng.standard_normal((K, D))
    cb = (cb / np.linalg.norm(cb, axis=1, keepdims=True) * rng.uniform(100, 200, size=(K, 1))).astype(np.float32)
    assert (np.linalg.norm(cb.astype(np.float64), axis=1) >= 100).all()
    owner = rng.integers(0, K, size=N)
    x = (cb[owner] + 0.01 * rng.standard_normal((N, D))).astype(np.float32)
    index, _ = run(x, cb, gpu_device)
    assert index.min() >= 0 and index.max() < K
    assert np.array_equal(index, R.brute(x, cb)[0]) and np.array_equal(index, owner)


@pytest.mark.parametrize("half,D", [(40, 4), (40, 9), (2100, 4)])
def test_of_equal_scores_the_smallest_index_wins(gpu_device, half, D):
    rng = np.random.default_rng(half + D)
    cb = rng.standard_normal((half, D)).astype(np.float32)
    both = np.concatenate((cb, cb))                      # every row again at index + half: other lane half, tile, stage
    x = np.concatenate((rng.standard_normal((200, D)).astype(np.float32), cb[:40]))
    index, dist2 = run(x, both, gpu_device)
    assert index.max() < half, "a duplicate at the higher index was chosen"
    assert np.array_equal(index, run(x, cb, gpu_device)[0])
    assert np.array_equal(index[200:], np.arange(40)) and (dist2[200:] == 0).all(), "a point equal to a code"


def test_same_bits_twice_and_under_a_permutation_of_the_rows(gpu_device):
    x, cb, _, _ = case(257, 4097, 4, "unit")
    a, b = run(x, cb, gpu_device), run(x, cb, gpu_device)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    perm = np.random.default_rng(3).permutation(len(x))
    c = run(x[perm], cb, gpu_device)
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(c[1].view(np.uint32), a[1][perm].view(np.uint32))


def test_the_last_code_of_the_largest_codebook_can_win(gpu_device):
    x, cb, rows, codes = R.largest_codebook_case()
    index, dist2 = run(x, cb, gpu_device)
    assert np.array_equal(index, R.assign(x, cb)[0])
    assert np.array_equal(index[rows], codes) and (dist2[rows] == 0).all(), "a point equal to a code"
    assert index.max() == 65535


# every D of the vector-ALU kernel is an instantiation of its own; its stage is 1024 codes, so K = 1024 fills one and
# K = 1025 leaves one code to a second.  (D = 3 and 4 at K = 4097 keep the ids they had before the other cases came.)
VALU_CASES = [pytest.param(D, K, id=str(D) if D >= 3 and K == 4097 else f"{D}-{K}")
              for D in (1, 2, 3, 4) for K in (1024, 1025, 4097)]


@pytest.mark.parametrize("D,K", VALU_CASES)
def test_vector_alu_path_agrees_with_the_matrix_core_path_bit_for_bit(gpu_device, D, K):
    rng = np.random.default_rng(D)
    x = rng.standard_normal((257, D)).astype(np.float32)
    cb = rng.standard_normal((K, D)).astype(np.float32)
    a, b = run(x, cb, gpu_device), run(x, cb, gpu_device, path="valu")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- update ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_update_is_the_float64_mean_rounded_once(gpu_device, weighted):
    rng = np.random.default_rng(11)
    N, K, D = 700, 7, 5
    x = (rng.standard_normal((N, D)) * 10.0 ** rng.uniform(-2, 2, size=(N, 1))).astype(np.float32)
    index = rng.choice([0, 1, 2, 4, 5, 6], size=N).astype(np.int32)          # code 3 has no row
    cb = rng.standard_normal((K, D)).astype(np.float32)
    w = None
    if weighted:
        w = rng.uniform(0, 3, size=N).astype(np.float32)
        w[index == 5] = 0                                                     # every row of code 5 weighs nothing
    want, want_empty = R.update(x, index, cb, w)
    assert want_empty == (2 if weighted else 1)
    t = lambda a: None if a is None else torch.from_numpy(a).to(gpu_device)                      # noqa: E731
    got, empty = kmeans_update(t(x), t(index), t(cb), t(w))
    got = got.cpu().numpy()
    assert empty == want_empty
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[3], cb[3]) and (not weighted or np.array_equal(got[5], cb[5])), "an empty code keeps its centre"


def test_update_with_one_code_owning_every_row(gpu_device):
    rng = np.random.default_rng(12)
    x = rng.standard_normal((3001, 64)).astype(np.float32)
    cb = rng.standard_normal((3, 64)).astype(np.float32)
    index = np.full(3001, 1, dtype=np.int32)
    want, _ = R.update(x, index, cb)
    got, empty = kmeans_update(torch.from_numpy(x).to(gpu_device), torch.from_numpy(index).to(gpu_device),
                               torch.from_numpy(cb).to(gpu_device))
    assert empty == 2 and np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("weighted", [False, True])
def test_update_with_runs_that_end_where_a_workgroup_ends(gpu_device, weighted):
    x, index, cb, w = R.workgroup_edge_update_input()
    w = w if weighted else None
    want, want_empty = R.update(x, index, cb, w)
    t = lambda a: None if a is None else torch.from_numpy(a).to(gpu_device)                      # noqa: E731
    got, empty = kmeans_update(t(x), t(index), t(cb), t(w))
    got = got.cpu().numpy()
    assert empty == want_empty == 2
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[2], cb[2]) and np.array_equal(got[4], cb[4]), "an empty code keeps its centre"


# ---- Lloyd's iteration -----------------------------------------------------------------------------------------------------
def host_permutation(N, seed):
    """The permutation ``kmeans`` walks for its init."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    return torch.randperm(N, generator=gen)


@pytest.mark.parametrize("weighted", [False, True])
def test_lloyds_trajectory_is_the_restatements_bit_for_bit(gpu_device, weighted):
    x, w, K, iters, seed = R.trajectory_input()
    w = w if weighted else None
    first = R.first_distinct(x, host_permutation(len(x), seed).numpy(), K)
    books, want_index, want_empty, dist2s = R.lloyd(x, first, iters, w)
    codebook, index, info = kmeans(torch.from_numpy(x).to(gpu_device), K, iters=iters, seed=seed, history=True,
                                   weights=None if w is None else torch.from_numpy(w).to(gpu_device))
    assert len(info["codebooks"]) == len(books) == iters + 1 and not info["shortcut"]
    for t, (got, want) in enumerate(zip(info["codebooks"], books)):
        assert got.shape == want.shape == (K, x.shape[1]), t
        differ = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
        assert not differ.any(), f"codebook {t}: codes {np.flatnonzero(differ)[:8]} differ in their bits"
    assert np.array_equal(codebook.cpu().numpy().view(np.uint32), books[-1].view(np.uint32))
    assert np.array_equal(index.cpu().numpy(), want_index)
    assert info["empty"] == want_empty
    assert len(info["objective"]) == iters + 1
    for t, d in enumerate(dist2s):         # the float64 sum of the same float32 values: only the order of the sum differs
        want = float(d.astype(np.float64).sum())
        print(f"step {t}: objective {info['objective'][t]!r} against {want!r}")
        assert abs(info["objective"][t] - want) <= 1e-6 * want, t


def test_init_takes_the_first_k_distinct_rows_in_permutation_order(gpu_device):
    x, seed = R.init_input()
    perm = host_permutation(len(x), seed)
    assert len(np.unique(x[perm.numpy()[:64]], axis=0)) < 64, "the first chunk has to leave the init short of K = 64"
    xd = torch.from_numpy(x).to(gpu_device)
    for K, rows in ((64, 64), (128, 90)):
        want = R.first_distinct(x, perm.numpy(), K)
        got = _distinct_rows(xd, perm.to(gpu_device), K).cpu().numpy()
        assert len(want) == rows and np.array_equal(got, want), K
    codebook, index, info = kmeans(xd, 128, iters=2, seed=seed)
    assert codebook.shape == (90, x.shape[1]) and not info["shortcut"]
    assert np.array_equal(codebook.cpu().numpy().view(np.uint32), x[R.first_distinct(x, perm.numpy(), 128)].view(np.uint32))
    rebuilt = codebook.index_select(0, index.long()).cpu().numpy()
    assert np.array_equal(rebuilt.view(np.uint32), x.view(np.uint32))


def test_objective_does_not_rise_by_more_than_the_rounding_of_the_centres(gpu_device):
    rng = np.random.default_rng(21)
    centres = 4.0 * rng.standard_normal((12, 6))
    x = (centres[rng.integers(0, 12, size=2000)] + rng.standard_normal((2000, 6))).astype(np.float32)
    codebook, index, info = kmeans(torch.from_numpy(x).to(gpu_device), 16, iters=6, seed=3, history=True)
    books = info["codebooks"]
    assert len(books) == 7 and len(info["objective"]) == 7 and len(info["empty"]) == 6
    assert np.array_equal(books[-1], codebook.cpu().numpy())
    assert np.array_equal(index.cpu().numpy(), R.assign(x, books[-1])[0])
    J = [R.objective(x, b) for b in books]
    print("J* per iteration:", J, "device sums of dist2:", info["objective"])
    for t in range(6):
        assert J[t + 1] <= J[t] + R.monotone_slack(x, books[t], books[t + 1], J[t]), t
    assert J[-1] < J[0], "six iterations from a random init lower the objective"
    assert abs(info["objective"][-1] - J[-1]) <= 1e-4 * J[-1]


def test_few_distinct_rows_are_reproduced_bit_for_bit(gpu_device):
    rng = np.random.default_rng(22)
    distinct = rng.standard_normal((50, 12)).astype(np.float32)
    x = distinct[rng.permutation(np.repeat(np.arange(50), 10))]
    codebook, index, info = kmeans(torch.from_numpy(x).to(gpu_device), 64, iters=4, seed=0)
    assert codebook.shape[0] <= 64 and not info["shortcut"]
    rebuilt = codebook.index_select(0, index.long()).cpu().numpy()
    assert np.array_equal(rebuilt.view(np.uint32), x.view(np.uint32))
