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

Shared by tests/test_kmeans_host.py (no GPU), tests/test_gpu_kmeans.py and tests/test_gpu_compress.py.
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
