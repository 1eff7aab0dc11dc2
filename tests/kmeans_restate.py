"""Restatement of the k-means assignment rule and centre update (``mvs_gaussian_splatting_amd/compress.py``,
``csrc/kmeans.hip``, ``csrc/kmeans_math.h``) in numpy, the float64 brute force, and the two derived bounds.

``fma32``          one float32 fused multiply-add on arrays: the product of two float32 values is exact in float64 (48
                   significant bits), the sum with the float32 addend is rounded to float64 TO ODD (TwoSum gives the exact
                   error of the float64 addition; an inexact result whose last mantissa bit is even moves to its odd
                   neighbour on the side of the error), and a value rounded to odd at 53 bits rounds to float32 exactly as
                   the unrounded value does (53 >= 24 + 2), so there is no double rounding.  Presumes no float64
                   overflow: float32 products and sums of the test data stay far below it.
``chain``          fmaf(a[n-1], b[n-1], ... fmaf(a[0], b[0], 0.0f))
``assign``         the rule: score = fma32(-2, chain(x, c), chain(c, c)), the smallest score, the smallest index among
                   equal scores (``numpy.argmin`` returns the first), dist2 = max(0, float32(chain(x, x) + score)).
``brute``          float64 squared distances on the float32 values and their argmin: the truth.
``update``         the float64 mean per code in ascending row order (``numpy.cumsum`` adds sequentially, from the first
                   member on), ``sum w x / sum w`` with weights, rounded to float32 once; a code with no row or with
                   sum w = 0 keeps its centre.
``first_distinct`` the init of ``compress.kmeans`` as a loop over the permutation.
``lloyd``          ``compress.kmeans`` as ``assign`` and ``update`` in turn: no arithmetic of its own.

The float64-gap bound (``gap_bound``).  Let u = 2^-24, gamma_n = n u / (1 - n u), s(c) = |c|^2 - 2 x.c in exact
arithmetic (so |x - c|^2 = |x|^2 + s(c)) and s^(c) the computed score.  The two chains are D fused multiply-adds each:
|dot^ - x.c| <= gamma_D sum_k |x_k c_k| and |cnorm^ - |c|^2| <= gamma_D |c|^2 (Higham, Accuracy and Stability, §3.1; an fma
chain has one rounding per term).  The last fmaf rounds cnorm^ - 2 dot^ once more, so
    |s^(c) - s(c)| <= gamma_{D+1} (2 sum_k |x_k c_k| + |c|^2) <= gamma_{D+2} B(x, c),   B = 2 sum_k |x_k c_k| + |c|^2
(gamma_{D+2}: one step of slack for the padded step of an odd D, which is exact, and the products of the gammas).  The rule
picks i with s^(c_i) <= s^(c_j) for every j, in particular for the true nearest j, hence
    |x - c_i|^2 - |x - c_j|^2 = s(c_i) - s(c_j) <= (s(c_i) - s^(c_i)) + (s^(c_j) - s(c_j)) <= 2 gamma_{D+2} max(B_i, B_j).
Presumes no underflow in the products (the test data keeps |x_k c_k| above 1e-30 or exactly 0).

The monotonicity slack (``monotone_slack``).  J*(C) = sum_i min_c |x_i - c|^2 in float64.  One iteration takes the rule's
assignment a under C, which costs at most J*(C) + sum_i gap_i; the exact means minimise the cost of a, and a centre rounded
to float32, m^ = m (1 + delta) with |delta| <= u per component, adds n_c |m^ - m|^2 <= n_c u^2 |m|^2 for its n_c rows (the
float64 accumulation error is of order 2^-53 n_c and is covered by the factor below); J*(C') is at most the cost of a under
C'.  With |x.c| <= |x| |c|:
    J*(C') - J*(C) <= N (u^2 Cmax^2 + 2 gamma_{D+2} (2 Xmax Cmax + Cmax^2)) (1 + 1e-3) + 1e-12 J*(C)
Xmax, Cmax the largest row norms of x and of both codebooks; the last term is the float64 evaluation of J* itself.

Shared by tests/test_kmeans_host.py (no GPU), tests/test_gpu_kmeans.py and tests/test_gpu_compress.py.  The inputs at
the end of the file are shared in the same way: the host tests check the premises of each (that the weighted trajectory
has an empty code, that the init has to go round its loop again, which kernel instantiation a shape reaches) on the
restatement, the GPU tests run them.
"""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def fma32(a, b, c):
    """float32(a * b + c) with one rounding, elementwise on float32 arrays (broadcast)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                                   # exact
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)                 # TwoSum: p + c = s + e exactly
    s, e = np.broadcast_arrays(s, e)
    s = s.copy()
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s[fix] = np.nextafter(s[fix], np.where(e[fix] > 0, np.inf, -np.inf))
    return s.astype(np.float32)


def chain(a, b):
    """The fmaf chain over the last axis of two broadcastable float32 arrays."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    shape = np.broadcast_shapes(a.shape[:-1], b.shape[:-1])
    acc = np.zeros(shape, dtype=np.float32)
    for k in range(a.shape[-1]):
        acc = fma32(a[..., k], b[..., k], acc)
    return acc


def scores(x, codebook):
    """float32 [N,K]: the score of every (point, code)."""
    x, codebook = np.asarray(x, dtype=np.float32), np.asarray(codebook, dtype=np.float32)
    dot = chain(x[:, None, :], codebook[None, :, :])
    cnorm = chain(codebook, codebook)
    return fma32(np.float32(-2.0), dot, cnorm[None, :])


def assign(x, codebook):
    """-> (index int32 [N], dist2 float32 [N])."""
    sc = scores(x, codebook)
    index = np.argmin(sc, axis=1).astype(np.int32)
    best = sc[np.arange(len(index)), index]
    xnorm = chain(x, x)
    with np.errstate(invalid="ignore"):
        d = (xnorm + best).astype(np.float32)
    return index, np.where(d > 0, d, np.float32(0)).astype(np.float32)


def dist2_f64(x, codebook):
    x, c = np.asarray(x, dtype=np.float64), np.asarray(codebook, dtype=np.float64)
    return ((x[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)


def brute(x, codebook):
    """-> (index of the true nearest code, the float64 [N,K] squared distances)."""
    d = dist2_f64(x, codebook)
    return np.argmin(d, axis=1).astype(np.int32), d


def gap_bound(x, codebook, i, j):
    """Per point: 2 gamma_{D+2} max(B(x, c_i), B(x, c_j))."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(codebook, dtype=np.float64)
    B = lambda idx: 2.0 * np.abs(x * c[idx]).sum(axis=1) + (c[idx] ** 2).sum(axis=1)       # noqa: E731
    return 2.0 * gamma(x.shape[1] + 2) * np.maximum(B(i), B(j))


def objective(x, codebook):
    """J*(C): the float64 sum of the squared distances to the true nearest code."""
    return float(dist2_f64(x, codebook).min(axis=1).sum())


def monotone_slack(x, before, after, j_before):
    x = np.asarray(x, dtype=np.float64)
    xmax = np.sqrt((x ** 2).sum(axis=1).max())
    cmax = max(np.sqrt((np.asarray(c, dtype=np.float64) ** 2).sum(axis=1).max()) for c in (before, after))
    D = x.shape[1]
    return len(x) * (U * U * cmax * cmax + 2.0 * gamma(D + 2) * (2.0 * xmax * cmax + cmax * cmax)) * (1.0 + 1e-3) \
        + 1e-12 * j_before


def update(x, index, codebook, weights=None):
    """-> (new codebook float32 [K,D], the number of codes that kept their centre)."""
    x, codebook = np.asarray(x, dtype=np.float32), np.asarray(codebook, dtype=np.float32)
    out, empty = codebook.copy(), 0
    for c in range(codebook.shape[0]):
        rows = np.flatnonzero(np.asarray(index) == c)                # ascending row index
        if rows.size == 0:
            empty += 1
            continue
        w = np.ones(rows.size) if weights is None else np.asarray(weights, dtype=np.float32)[rows].astype(np.float64)
        wsum = np.cumsum(w)[-1]
        if not wsum > 0:
            empty += 1
            continue
        total = np.cumsum(w[:, None] * x[rows].astype(np.float64), axis=0)[-1]       # products exact, sums sequential
        out[c] = (total / wsum).astype(np.float32)
    return out, empty


def canonical_rotation(q):
    """float32: q / max(|q|, 1e-12) with the sign fixed so that w >= 0 (torch's float32 op order is restated by the
    callers through torch itself; this is the float64 check of unit length and sign)."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.maximum(np.sqrt((q ** 2).sum(axis=1, keepdims=True)), 1e-12)
    return np.where(q[:, :1] < 0, -q, q)


# ---- Lloyd's iteration, sequentially ---------------------------------------------------------------------------------------
def first_distinct(x, perm, K):
    """The init of ``compress.kmeans``: walking ``perm``, the entries whose row of ``x`` differs in its float32 bits from
    every row kept before, until there are ``K`` (fewer if ``x`` runs out of distinct rows) -> int64 [K']."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    kept, rows = [], set()
    for p in perm:
        if len(kept) == K:
            break
        bits = x[int(p)].tobytes()
        if bits not in rows:
            kept.append(int(p))
            rows.add(bits)
    return np.array(kept, dtype=np.int64)


def lloyd(x, first, iters, weights=None):
    """``compress.kmeans`` from the initial codebook ``x[first]``: ``iters`` times ``assign`` then ``update``, and a last
    ``assign`` -> (the ``iters + 1`` codebooks, each the one its assign ran against; the final index; per iteration the
    number of codes that kept their centre; the ``iters + 1`` dist2 arrays of the assigns)."""
    x = np.asarray(x, dtype=np.float32)
    codebook = x[np.asarray(first)].copy()
    books, empties, dist2s = [], [], []
    for _ in range(iters):
        books.append(codebook)
        index, dist2 = assign(x, codebook)
        dist2s.append(dist2)
        codebook, empty = update(x, index, codebook, weights)
        empties.append(empty)
    books.append(codebook)
    index, dist2 = assign(x, codebook)
    dist2s.append(dist2)
    return books, index, empties, dist2s


# ---- inputs shared by the host tests (which check their premises) and the GPU tests (which run them) -------------------------
# Assignment shapes beyond the first ten of tests/test_gpu_kmeans.py: (N, K, D, the STEPS instantiation of
# kmeans_assign_mfma_kernel that D dispatches to, the edge the case is there for).  A workgroup is 256 points = 4 waves of
# two 32-point tiles; a codebook stage is 128 codes = 4 tiles of 32.
ASSIGN_EDGE_CASES = [
    (33, 100, 5, 8, "D = 5, the first D of STEPS = 8"),
    (97, 33, 16, 8, "D = 16, the last D of STEPS = 8; N ends on the first point of wave 1's tile 1"),
    (353, 129, 17, 16, "D = 17, the first D of STEPS = 16; N ends in tile 1 of wave 1 of the second workgroup"),
    (353, 4097, 24, 16, "D = 24 (f_rest at SH degree 2) over 33 stages"),
    (97, 128, 32, 16, "D = 32, the last D of STEPS = 16; the only stage exactly full"),
    (353, 256, 33, 24, "D = 33, the first D of STEPS = 24; the last of two stages exactly full"),
    (97, 100, 49, 32, "D = 49, the first D of STEPS = 32"),
    (256 + 3 * 64 + 1, 33, 9, 8, "N ends on the first point of wave 3"),
    (256 + 2 * 64 + 33, 2, 3, 2, "N ends on the first point of wave 2's tile 1"),
    (32, 2, 3, 2, "N fills tile 0 of wave 0 and nothing else"),
    (64, 33, 9, 8, "N fills wave 0 and nothing else"),
    (256, 100, 4, 2, "N fills one workgroup and nothing else"),
    (97, 128, 9, 8, "K = 128 at an odd D"),
    (97, 256, 4, 2, "K = 256 on the STEPS = 2 instantiation"),
    (97, 129, 45, 24, "K = 129: one code past a full stage, at an odd D"),
]


def largest_codebook_case():
    """-> (x [97,3], codebook [65536,3], rows, codes): K at its limit, the last index a uint16 holds.  x[rows[i]] is a
    bit copy of codebook[codes[i]]: the last two codes, the first code of the last stage (65408) and the one before it,
    the middle, both sides of the first stage boundary, and code 0."""
    rng = np.random.default_rng(65536)
    cb = rng.standard_normal((65536, 3)).astype(np.float32)
    x = rng.standard_normal((97, 3)).astype(np.float32)
    codes = np.array([65535, 65534, 65408, 65407, 32768, 127, 128, 0], dtype=np.int32)
    rows = np.array([96, 0, 31, 32, 63, 64, 65, 95])          # both tiles of wave 0, and wave 1 up to the last point
    x[rows] = cb[codes]
    return x, cb, rows, codes


def trajectory_input():
    """-> (x [1500,6], weights [1500], K, iters, seed) for Lloyd's trajectory: 12 clusters of unequal size, 300 rows that
    are bit copies of other rows (the init has to skip duplicates), weights uniform in [0, 3] with about a tenth exactly
    0 -- the whole of the smallest cluster, so that a code the init takes from it never gathers any weight, and rows
    scattered over the others."""
    rng = np.random.default_rng(33)
    N, D = 1500, 6
    centres = 4.0 * rng.standard_normal((12, D))
    owner = rng.choice(12, size=N, p=np.array([6.0] + [8.5] * 10 + [9.0]) / 100.0)
    x = (centres[owner] + rng.standard_normal((N, D))).astype(np.float32)
    copy = rng.permutation(N)
    source = copy[300 + rng.integers(0, 30, size=300)]      # of 30 rows only, so that copies meet early in a permutation
    x[copy[:300]], owner[copy[:300]] = x[source], owner[source]
    w = rng.uniform(0, 3, size=N).astype(np.float32)
    w[owner == 0] = 0
    w[rng.random(N) < 0.05] = 0
    return x, w, 40, 5, 6


def init_input():
    """-> (x [5000,8], seed): 5000 rows drawn from 90 distinct ones."""
    rng = np.random.default_rng(90)
    distinct = rng.standard_normal((90, 8)).astype(np.float32)
    return distinct[rng.integers(0, 90, size=5000)], 4


def workgroup_edge_update_input():
    """-> (x [768,7], index, codebook [5,7], weights): the runs of codes 0, 1 and 3 are 256 rows each, so every run ends
    where a 256-lane workgroup of the run search ends; codes 2 and 4 have no row."""
    rng = np.random.default_rng(768)
    x = (rng.standard_normal((768, 7)) * 10.0 ** rng.uniform(-2, 2, size=(768, 1))).astype(np.float32)
    index = np.repeat(np.array([0, 1, 3], dtype=np.int32), 256)
    cb = rng.standard_normal((5, 7)).astype(np.float32)
    return x, index, cb, rng.uniform(0, 3, size=768).astype(np.float32)


def model_arrays(P, degree, seed=0):
    """The tensors of a model of ``P`` Gaussians at SH ``degree`` as float32 arrays, by the names of ``ply_io.load_ply``,
    and dense weights in [0, 3)."""
    rng = np.random.default_rng(1000 * degree + seed)
    k = (degree + 1) ** 2 - 1
    r = lambda *s: rng.standard_normal(s).astype(np.float32)                                      # noqa: E731
    model = {"_xyz": r(P, 3), "_features_dc": r(P, 1, 3), "_features_rest": r(P, k, 3), "_opacity": r(P, 1),
             "_scaling": r(P, 3), "_rotation": r(P, 4)}
    return model, rng.uniform(0, 3, size=P).astype(np.float32)
