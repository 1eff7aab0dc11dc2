"""The designed densification-plan cases (tests/densify_plan_restate.py) are what they claim to be: the sizes reach the
scan paths they are named after, the float64 rule reproduces the designed classes, ordinary rows keep a factor 2 from
every threshold, every class has members, and the block pattern has the empty runs, the full runs and the
last-block-only class that the scan of the block counters is to be tested on.  No GPU."""
import numpy as np
import pytest

import densify_plan_restate as R

MODES = [(ws, learned) for ws in (True, False) for learned in (False, True)]


@pytest.fixture(scope="module")
def cases():
    return {name: R.build(name) for name in R.CASES}


@pytest.mark.parametrize("name", list(R.CASES))
def test_sizes_reach_the_tabulated_scan_path(cases, name):
    c = cases[name]
    nb, rem = R.TABLE[name]
    assert c.nb == nb == (c.P + 255) // 256 and (nb + 1) % 4 == rem
    assert nb >= 32                                  # at least one lane owns a whole 32-entry line: the 16-byte path
    assert (nb > 32768) == (name == "two_rounds")    # a second round of 1024 lanes x 32 entries
    if name == "two_rounds":
        assert (nb - 32768) // 32 >= 1 and (nb - 32768) % 32 != 0    # round two: a whole line and a scalar tail
    if name in ("odd1", "odd2", "odd3", "tail", "two_rounds"):
        assert c.P % 256 != 0                        # partial last block
    assert c.P < 2 ** 24                             # row numbers are exact in float32


@pytest.mark.parametrize("name", list(R.CASES))
def test_float64_rule_reproduces_the_designed_classes(cases, name):
    c = cases[name]
    for ws, learned in MODES:
        for fork in (False, True):
            assert np.array_equal(R.rule_flags(c, ws, learned, fork), R.designed_flags(c, ws, learned, fork)), \
                (name, ws, learned, fork)
    for split_mode in (False, True):
        for got, want in zip(R.grow_rule(c, split_mode), R.grow_designed(c, split_mode)):
            assert np.array_equal(got, want), (name, split_mode)


@pytest.mark.parametrize("name", list(R.CASES))
def test_ordinary_rows_keep_a_factor_two_from_every_threshold(cases, name):
    c = cases[name]
    n_edge = int(c.edge.sum())
    assert 0 < n_edge <= 64 and len(c.edge_names) == n_edge
    m = ~c.edge
    g, mx, op = R._raw64(c)
    g, mx, op = g[m], mx[m], op[m]
    assert np.all(np.isfinite(g))
    assert np.all((np.abs(g) >= 2 * R.THR) | (np.abs(g) <= R.THR / 2))
    assert np.all((mx >= 2 * R.PDE) | (mx <= R.PDE / 2))
    assert np.all((mx >= 2 * R.WS) | (mx <= R.WS / 2))
    for learned in (False, True):
        child = mx / R.child_divisor(c, learned)[m]
        assert np.all((child >= 2 * R.WS) | (child <= R.WS / 2))
    assert np.all((op >= 2 * R.MIN_OPACITY) | (op <= R.MIN_OPACITY / 2))
    # the values the edge rows rest on are exact in float32
    assert np.float32(2 * R.THR) / np.float32(2.0) == np.float32(R.THR) and float(np.float32(R.THR)) == R.THR
    assert np.exp(np.float32(0.0)) == np.float32(R.PDE)
    # every edge kind is present in some case, and every case holds the ones that fit it
    names = set(c.edge_names.values())
    assert {e[0] for e in R.EDGES if e[1] != c.last_only} <= names


def test_every_edge_row_occurs_in_a_small_case(cases):
    seen = set()
    for name in R.SMALL_CASES:
        seen |= set(cases[name].edge_names.values())
    assert seen == {e[0] for e in R.EDGES}


@pytest.mark.parametrize("name", list(R.CASES))
def test_every_class_has_a_distinct_non_zero_count(cases, name):
    c = cases[name]
    for ws, learned in MODES:
        counts, order = R.densify_expected(R.designed_flags(c, ws, learned))
        assert min(counts) > 0 and len(set(counts)) == 4, (name, ws, learned, counts)
        assert order.size == counts[0] + counts[1] + 2 * counts[2]
        counts, _ = R.fork_expected(R.designed_flags(c, ws, learned, fork=True), grow=True)
        assert min(counts) > 0 and len(set(counts)) == 5, (name, ws, learned, counts)
    vidx, src, selected, counts = R.grow_designed(c, False)
    assert 0 < counts[1] < counts[0] < c.P
    vidx, src, selected, counts = R.grow_designed(c, True)
    assert 0 < counts[0] == counts[1] < c.P          # split mode selects only big rows
    # the child-prune edge separates the two divisors and the two prune modes (plain cases that hold it)
    rows = [r for r, n in c.edge_names.items() if n == "child_over_k"]
    for r in rows:
        assert R.designed_flags(c, True, False)[r] & R.CHILD and not R.designed_flags(c, True, True)[r] & R.CHILD
        assert R.designed_flags(c, False, True)[r] & R.CHILD


@pytest.mark.parametrize("name", list(R.CASES))
def test_workspaces_hold_counter_arrays_a_multiple_of_64_words_apart(cases, name):
    """The scan moves whole lines as 16-byte words, so each of a plan's n counter arrays (and n offset arrays) starts
    (nb + 1 rounded up to 64) words after the one before: row_plan.h's layout, the head of the workspaces of densify.hip, densify_fork.hip and grow.hip."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    c = cases[name]

    def a256(v):
        return (v + 255) // 256 * 256

    stride = (c.nb + 1 + 63) // 64 * 64
    assert stride % 64 == 0 and stride >= c.nb + 1
    head = lambda n: a256(c.P) + 2 * a256(4 * n * stride) + 256           # flags, counters, offsets, totals
    assert lib.gsr_densify_workspace_bytes(c.P) == head(4) + a256(16 * c.P)
    assert lib.gsr_densify_fork_workspace_bytes(c.P) == head(5) + a256(20 * c.P) + a256(4 * c.P)
    assert lib.gsr_grow_workspace_bytes(c.P) == head(2)


def _has_run(mask, n=2):
    """True when `mask` holds n consecutive True values."""
    return bool(np.any(np.convolve(mask.astype(np.int64), np.ones(n, dtype=np.int64), "valid") == n))


@pytest.mark.parametrize("name", list(R.CASES))
def test_block_pattern_has_empty_runs_full_runs_and_a_last_block_only_class(cases, name):
    c = cases[name]
    for ws in (True, False):
        f = R.designed_flags(c, ws, fork=True)
        for bit in (R.KEEP, R.SPLIT_SEL, R.SEL):
            k = R.block_counters(f, bit, c.nb)
            assert _has_run(k == 0) and _has_run(k == 256), (name, ws, bit)
            assert len(set(k.tolist())) > 4          # and mixed blocks in between
        last = R.block_counters(f, R.CLONE if c.last_only == "clone" else R.CHILD, c.nb)
        assert last[-1] > 0 and not last[:-1].any(), (name, ws)
        other = R.block_counters(f, R.CHILD if c.last_only == "clone" else R.CLONE, c.nb)
        assert np.count_nonzero(other) > c.nb // 4
    if name == "two_rounds":                         # round two starts with a carry that no single round could hold
        f = R.designed_flags(c, True)
        for bit in (R.KEEP, R.CHILD, R.SPLIT_SEL):
            k = R.block_counters(f, bit, c.nb)
            assert k[:32768].sum() > 0 and k[32768:-1].sum() > 0
