"""Designed inputs and a float64 reference for the three densification plans (``gsr_densify_plan``,
``gsr_densify_fork_plan``, ``gsr_grow_plan``) and the row order their gathers produce.

A case fixes ``P`` and, for every row, a class: which side of each threshold the row lies on.  The raw inputs
(``accum``, ``denom``, ``scaling[P,3]``, ``opacity[P]``, ``split_scale[P]``) are derived from the class, so the expected
flags are known by construction (``designed_flags``); ``rule_flags`` evaluates the rule of csrc/densify.hip's header in
float64 from the raw inputs alone and must give the same flags (tests/test_densify_plan_host.py).

Ordinary rows keep every tested quantity a factor 2 from its threshold, so float32 ``expf`` on the device and float64
here cannot disagree.  Only the edge rows (``EDGES``, at most 64 per case) sit on or near a threshold, with values that
are exact in float32: ``scaling = 0`` (scale 1 = ``PDE``), ``accum = 2 THR, denom = 2`` (gradient = ``THR``),
``accum = +-1, denom = 0`` (+-inf) and ``0 / 0`` (NaN -> 0).

The class pattern is laid out in 256-row blocks (the plan kernels' block) to exercise the scan of the block counters:
runs of blocks without a member of a class, runs with all 256, a partial last block, and one class (``last_only``:
clones or kept children, alternating over the cases) whose counter is non-zero in the last block only.
"""
import numpy as np

BLOCK = 256
THR = float(2.0 ** -12)          # gradient threshold: a power of two, so 2 THR / 2 == THR exactly
PDE = 1.0                        # percent_dense * extent: exp(0) sits exactly on it
WS = 10.0                        # 0.1 * extent, the world-size prune limit
MIN_OPACITY = 0.005

KEEP, CLONE, CHILD, SPLIT_SEL, SEL = 1, 2, 4, 8, 16          # flag bits: densify.hip's four, densify_fork.hip's fifth
G_LO, G_HI, G_NAN, G_NEG = 0, 1, 2, 3                        # gradient: THR / 4, 4 THR, 0 / 0, -4 THR
S_SMALL, S_MID, S_BIG = 0, 1, 2                              # largest scale: 0.25, 3, 80
O_OK, O_LOW = 0, 1                                           # raw opacity >= 1, or -8 (sigmoid 3.4e-4)

# case -> (P, class that only the last block holds)
CASES = {
    "aligned": (256 * 79, "clone"),                  # stride 80 words: 16-byte aligned by accident (the control)
    "line32": (256 * 32, "child"),                   # nb = 32: only lane 0 owns a whole line
    "odd1": (256 * 32 + 1, "clone"),                 # nb = 33, nb + 1 = 34: 8-byte aligned before the padding
    "odd2": (256 * 33 + 1, "child"),                 # nb = 34, nb + 1 = 35: 4-byte aligned
    "odd3": (256 * 36 + 255, "clone"),               # nb = 37, partial last block
    "tail": (256 * 63 + 7, "child"),                 # nb = 64: two whole lines
    "two_rounds": (256 * 32768 + 256 * 33 + 5, "clone"),      # nb = 32802: a second round of 32768 with carry
}
SMALL_CASES = [c for c in CASES if c != "two_rounds"]
# expected (nb, (nb + 1) % 4) of every case
TABLE = {"aligned": (79, 0), "line32": (32, 1), "odd1": (33, 2), "odd2": (34, 3), "odd3": (37, 2), "tail": (64, 1),
         "two_rounds": (32802, 3)}

# block kinds, period 12: M = mixed rows; the others hold one class in all 256 rows
K_MIX, K_KEEP, K_CLONE, K_SPLIT, K_NONE = 0, 1, 2, 3, 4
SCHEDULE = np.array([K_MIX, K_MIX, K_KEEP, K_KEEP, K_MIX, K_SPLIT, K_SPLIT, K_NONE, K_NONE, K_MIX, K_CLONE, K_CLONE],
                    dtype=np.uint8)
KIND_CODE = {K_KEEP: (G_LO, S_SMALL, O_OK), K_CLONE: (G_HI, S_SMALL, O_OK), K_SPLIT: (G_HI, S_MID, O_OK),
             K_NONE: (G_LO, S_MID, O_LOW)}

_G_COEF = np.array([THR / 4, 4 * THR, 0.0, -4 * THR], dtype=np.float32)
_S_MAX = np.array([0.25, 3.0, 80.0])
_S_TAB = np.log(_S_MAX[:, None] * np.array([1.0, 0.5, 0.25])[None, :]).astype(np.float32)       # [class, component]
_M12 = np.log(np.array([12.0, 6.0, 3.0])).astype(np.float32)        # above WS; its children at / 1.6 are below

# Edge rows: name, kind ("any" / "clone" / "child": which last_only class they would break outside the last block),
# accum, denom, scaling, opacity, split_scale, then the designed booleans
#   sel (g >= THR), gsel (|g| >= THR), big, low, over (parent > WS), over_c (child > WS at 1.6), over_cl (learned k)
_Z, _MID = np.zeros(3, np.float32), _S_TAB[S_MID]
EDGES = [
    ("inf_split_low", "any", 1.0, 0.0, _MID, -8.0, 0.0, 1, 1, 1, 1, 0, 0, 0),       # accum > 0, denom = 0: +inf, selected
    ("thr_split_low", "any", 2 * THR, 2.0, _MID, -8.0, 0.0, 1, 1, 1, 1, 0, 0, 0),   # g == THR: selected (>=)
    ("nan_keep", "any", 0.0, 0.0, _Z, 1.0, 0.0, 0, 0, 0, 0, 0, 0, 0),               # 0 / 0 -> 0: not selected
    ("pde_low", "any", 4 * THR, 1.0, _Z, -8.0, 0.0, 1, 1, 0, 1, 0, 0, 0),           # scale == PDE: not big (>), so no split
    ("neginf_keep", "any", -1.0, 0.0, _Z, 1.0, 0.0, 0, 1, 0, 0, 0, 0, 0),           # -inf: only |g| selects it
    ("over_lo", "any", THR / 4, 1.0, _M12, 1.0, 0.0, 0, 0, 1, 0, 1, 0, 0),          # pruned by size only with a limit
    ("inf_clone", "clone", 1.0, 0.0, _Z, 1.0, 0.0, 1, 1, 0, 0, 0, 0, 0),
    ("thr_clone", "clone", 2 * THR, 2.0, _Z, 1.0, 0.0, 1, 1, 0, 0, 0, 0, 0),
    ("pde_clone", "clone", 4 * THR, 1.0, _Z, 1.0, 0.0, 1, 1, 0, 0, 0, 0, 0),        # scale == PDE clones
    ("thr_child", "child", 2 * THR, 2.0, _MID, 1.0, 0.0, 1, 1, 1, 0, 0, 0, 0),
    ("inf_child", "child", 1.0, 0.0, _MID, 1.0, 0.0, 1, 1, 1, 0, 0, 0, 0),
    ("child_under", "child", 4 * THR, 1.0, _M12, 1.0, 4.0, 1, 1, 1, 0, 1, 0, 0),    # parent 12 > WS, children 7.5 / 5.5
    ("child_over_k", "child", 4 * THR, 1.0, _M12, 1.0, -4.0, 1, 1, 1, 0, 1, 0, 1),  # k = 1.02: children 11.7 > WS
]
_BOOLS = ("sel", "gsel", "big", "low", "over", "over_c", "over_cl")
EDGE_AT = 250          # the common edge rows straddle the boundary of blocks 0 and 1 (both mixed)
EDGE_LAST = 8          # the last_only kind's edge rows start here in the last block, when it has 32 rows or more


class Case:
    """name, P, nb, last_only, the raw float32 inputs, ``edge`` (bool [P]) and the designed booleans ``d[...]``."""


def block_count(P):
    return max((P + BLOCK - 1) // BLOCK, 1)


def build(name):
    P, last_only = CASES[name]
    nb = block_count(P)
    c = Case()
    c.name, c.P, c.nb, c.last_only = name, P, nb, last_only
    rng = np.random.default_rng(1000 + sorted(CASES).index(name))
    i = np.arange(P, dtype=np.int64)
    blk = i >> 8
    kinds = SCHEDULE[np.arange(nb) % len(SCHEDULE)].copy()
    kinds[nb - 1] = K_MIX
    kind = kinds[blk]
    g = np.array([G_LO] * 3 + [G_HI] * 3 + [G_NAN, G_NEG], dtype=np.uint8)[rng.integers(0, 8, P, dtype=np.uint8)]
    s = np.array([S_SMALL] * 3 + [S_MID] * 3 + [S_BIG] * 2, dtype=np.uint8)[rng.integers(0, 8, P, dtype=np.uint8)]
    o = (rng.integers(0, 5, P, dtype=np.uint8) == 0).astype(np.uint8)
    for k, (kg, ks, ko) in KIND_CODE.items():
        m = kind == k
        g[m], s[m], o[m] = kg, ks, ko
    # the last_only class: no member before the last block (those rows become low-opacity: still selected, but pruned),
    # and the first row of the last block is one
    first_last = (nb - 1) * BLOCK
    before = blk < nb - 1
    if last_only == "clone":
        o[before & (g == G_HI) & (s == S_SMALL)] = O_LOW
        g[first_last], s[first_last], o[first_last] = G_HI, S_SMALL, O_OK
    else:
        o[before & (g == G_HI) & (s >= S_MID)] = O_LOW
        g[first_last], s[first_last], o[first_last] = G_HI, S_MID, O_OK
    r3 = (i % 3).astype(np.int64)
    c.denom = np.where(g == G_NAN, 0, 1 + r3).astype(np.float32)
    c.accum = (_G_COEF[g] * c.denom).astype(np.float32)
    comp = (np.arange(3)[None, :] - r3[:, None]) % 3               # the largest scale moves over the three components
    c.scaling = _S_TAB[s[:, None], comp]
    c.opacity = np.where(o == O_LOW, -8.0, 1.0 + 0.5 * (i % 5)).astype(np.float32)
    c.split_scale = (((i % 7) - 3) * 1.5).astype(np.float32)
    d = {"sel": g == G_HI, "gsel": (g == G_HI) | (g == G_NEG), "big": s >= S_MID, "low": o == O_LOW, "over": s == S_BIG}
    d["over_c"] = d["over"].copy()
    d["over_cl"] = d["over"].copy()
    c.edge = np.zeros(P, dtype=bool)
    c.edge_names = {}
    room_last = P - first_last >= 32
    common = [e for e in EDGES if e[1] != last_only]
    at = [(EDGE_AT + j, e) for j, e in enumerate(common)]
    if room_last:
        at += [(first_last + EDGE_LAST + j, e) for j, e in enumerate(e for e in EDGES if e[1] == last_only)]
    for row, e in at:
        c.accum[row], c.denom[row], c.scaling[row], c.opacity[row], c.split_scale[row] = e[2], e[3], e[4], e[5], e[6]
        for k, v in zip(_BOOLS, e[7:]):
            d[k][row] = bool(v)
        c.edge[row] = True
        c.edge_names[row] = e[0]
    c.d = d
    return c


def _flags(sel, big, low, over, over_c, use_ws, fork):
    prune_o = low | (over & use_ws)
    prune_c = low | (over_c & use_ws)
    split = sel & big
    f = np.zeros(sel.shape[0], dtype=np.uint8)
    f[~split & ~prune_o] |= KEEP
    f[sel & ~big & ~prune_o] |= CLONE
    f[split & ~prune_c] |= CHILD
    f[split] |= SPLIT_SEL
    if fork:
        f[sel] |= SEL
    return f


def designed_flags(c, use_ws, learned=False, fork=False):
    d = c.d
    return _flags(d["sel"], d["big"], d["low"], d["over"], d["over_cl"] if learned else d["over_c"], bool(use_ws), fork)


def _raw64(c):
    """Gradient (NaN -> 0), largest scale and sigmoid(opacity) in float64 from the raw inputs; computed once per case."""
    if getattr(c, "_raw", None) is None:
        with np.errstate(divide="ignore", invalid="ignore"):
            g = c.accum.astype(np.float64) / c.denom.astype(np.float64)
        g[np.isnan(g)] = 0.0
        mx = np.exp(c.scaling.astype(np.float64)).max(axis=1)
        op = 1.0 / (1.0 + np.exp(-c.opacity.astype(np.float64)))
        c._raw = (g, mx, op)
    return c._raw


def child_divisor(c, learned):
    """2 (0.6 sigmoid(split_scale) + 0.5) with learn_split_scale, else 0.8 * 2."""
    if not learned:
        return np.full(c.P, 1.6)
    return 2.0 * (0.6 / (1.0 + np.exp(-c.split_scale.astype(np.float64))) + 0.5)


def rule_flags(c, use_ws, learned=False, fork=False):
    """csrc/densify.hip's header (densify_fork.hip's with ``fork``) in float64 from the raw inputs."""
    g, mx, op = _raw64(c)
    sel, big, low = g >= THR, mx > PDE, op < MIN_OPACITY
    k = child_divisor(c, learned)
    return _flags(sel, big, low, mx > WS, mx / k > WS, bool(use_ws), fork)


def block_counters(flags, bit, nb):
    return np.bincount(np.flatnonzero(flags & bit) >> 8, minlength=nb)


def densify_expected(flags):
    """counts {kept, clones, children per copy, split-selected} and the source row of every output row."""
    keep, clone, child = (np.flatnonzero(flags & b) for b in (KEEP, CLONE, CHILD))
    counts = [keep.size, clone.size, child.size, int(np.count_nonzero(flags & SPLIT_SEL))]
    return counts, np.concatenate((keep, clone, child, child))


def fork_expected(flags, grow):
    """Five counts and the c = 2 (clone + split) or c = 4 (grow branch) row order of include/gsr.h."""
    keep, clone, child = (np.flatnonzero(flags & b) for b in (KEEP, CLONE, CHILD))
    counts = [keep.size, clone.size, child.size, int(np.count_nonzero(flags & SPLIT_SEL)),
              int(np.count_nonzero(flags & SEL))]
    return counts, np.concatenate([keep, clone] + [child] * (4 if grow else 2))


def split_ranks(flags):
    """Rank of every row among the split-selected (the row of its first noise sample), -1 elsewhere."""
    m = (flags & SPLIT_SEL) != 0
    return np.where(m, np.cumsum(m) - 1, -1)


def _grow(sel, big):
    vidx = np.where(sel, np.cumsum(sel) - 1, -1).astype(np.int32)
    src = np.flatnonzero(sel).astype(np.int32)
    return vidx, src, sel.astype(np.uint8), [int(src.size), int(np.count_nonzero(sel & big))]


def grow_designed(c, split_mode):
    sel = c.d["gsel"] & c.d["big"] if split_mode else c.d["gsel"]
    return _grow(sel, c.d["big"])


def grow_rule(c, split_mode):
    """csrc/grow.hip's header in float64: |g| >= thr, in split mode also max scale > percent_dense * extent."""
    g, mx, _ = _raw64(c)
    big = mx > PDE
    sel = np.abs(g) >= THR
    return _grow(sel & big if split_mode else sel, big)
