"""The 32-bit radix sort paths of the two-level binning and the tile ranges derived from the sort, called on their own
(run on the GPU box: pytest -m gpu).

What runs: `sort_pairs_impl<uint32, uint32>` and `<uint32, uint2>` with a host-side or a device-side count, the depth
sort's top-digit pass, the segmented last pass of a two-pass sort (seg_block, the seg_totals branches of the hist /
rowscan / scatter kernels, the runs_rel write-back) and ranges_and_order_from_sort_kernel -- through gsr_sort_pairs_u32,
gsr_sort_extra_pass_u32 and gsr_sort_tile_runs_u32 (include/gsr.h).

The reference is numpy: np.argsort(keys & mask, kind="stable").  Every result is an integer and every comparison is exact
equality.  The one exception is `order`, whose entries may swap inside a length bucket: it is checked as a permutation per
chunk along which the bucket never increases.

Conventions of every case: keys carry random bits above end_bit (a missing mask shows); values carry the original index
(stability shows), two-word values are (i, ~i); buffers and scratch come from torch.empty, outputs and scratch are
pre-filled with 0xA5 bytes; with a device-side count below the capacity, everything at index >= count must still hold
its input value (first buffer) or the sentinel (second buffer).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc")


def _source_int(pattern, fn="gsr_common.h"):
    return int(re.search(pattern, open(os.path.join(CSRC, fn)).read()).group(1))


# keys per sort block (gsr_common.h: SORT_TILE = SORT_THREADS * SORT_ITEMS) and the widest digit
SORT_TILE = _source_int(r"constexpr int SORT_THREADS = (\d+);") * _source_int(r"#define GSR_SORT_ITEMS (\d+)")
RADIX_BITS = _source_int(r"constexpr int RADIX_BITS = (\d+);")
# keys ordered per pass of ranges_and_order_from_sort_kernel (binning.hip: CHUNK = 8 * 1024)
ORDER_CHUNK = 8 * _source_int(r"ranges_and_order_from_sort_kernel[^{]*\{\s*constexpr int CHUNK = 8 \* (\d+);", "binning.hip")
SENTINEL_BYTE = 0xA5
SENTINEL = np.uint32(0xA5A5A5A5)


# ---- the host-side rules of the sort, restated ------------------------------------------------------------------------
def sort_passes(end_bit):
    """gsr_launch.h sort_passes: the fewest passes the 9-bit kernels allow."""
    return (end_bit + RADIX_BITS - 1) // RADIX_BITS


def sort_pass_plan(end_bit):
    """binning.hip sort_pass_plan: the bits spread evenly over the passes, the wider digits last."""
    passes = sort_passes(end_bit)
    lo, extra = divmod(end_bit, passes)
    return [lo + (1 if p >= passes - extra else 0) for p in range(passes)]


def tile_sort_bits(n_keys):
    """gsr_common.h tile_sort_bits, the end_bit of the tile sort in enqueue_stage2 (gsr_api.hip): ceil(log2 n_keys), at
    least one bit so that a pass always runs."""
    b = 0
    while (1 << b) < n_keys:
        b += 1
    return max(b, 1)


def len_bucket(length):
    """binning.hip len_bucket on an int64 array: the length itself below 16, then eight steps per power of two."""
    length = np.asarray(length, dtype=np.int64)
    e = np.zeros_like(length)
    big = length >= 16
    e[big] = np.floor(np.log2(length[big])).astype(np.int64)      # exact: lengths are far below 2^53
    e[big & ((np.int64(1) << e) > length)] -= 1
    b = 16 + (e - 4) * 8 + ((length >> np.maximum(e - 3, 0)) & 7)
    return np.where(big, np.minimum(b, 255), length)


def test_restated_rules_agree_with_their_documented_examples():
    """The examples the source comments give for sort_pass_plan, and the shape of len_bucket."""
    assert SORT_TILE == 4096 and RADIX_BITS == 9 and ORDER_CHUNK == 8192
    assert sort_pass_plan(32) == [8, 8, 8, 8] and sort_pass_plan(13) == [6, 7] and sort_pass_plan(45) == [9] * 5
    assert [tile_sort_bits(t) for t in (1, 2, 3, 512, 513, 8160)] == [1, 1, 2, 9, 10, 13]
    assert list(len_bucket([0, 1, 15, 16, 17, 18, 31, 32, 36, 2 ** 31])) == [0, 1, 15, 16, 16, 17, 23, 24, 25, 232]
    lens = np.arange(0, 70000)
    assert (np.diff(len_bucket(lens)) >= 0).all()


# ---- plumbing ---------------------------------------------------------------------------------------------------------
def _mask(end_bit):
    return np.uint32((1 << end_bit) - 1)


def _stable_order(keys, end_bit):
    masked = keys & _mask(end_bit)
    if end_bit <= 16:
        masked = masked.astype(np.uint16)       # same order; numpy's stable sort of 16-bit integers is a radix sort
    return np.argsort(masked, kind="stable")


def _high_bits(rng, n, end_bit):
    """Random bits above end_bit: a sort that forgets its mask orders by them."""
    if end_bit >= 32:
        return np.zeros(n, dtype=np.uint32)
    return (rng.integers(0, 1 << (32 - end_bit), size=n, dtype=np.uint64) << np.uint64(end_bit)).astype(np.uint32)


def _values(n, val_words):
    i = np.arange(n, dtype=np.uint32)
    return i if val_words == 1 else np.stack([i, ~i], axis=1)


def _dev(arr, dev):
    t = torch.empty(arr.shape, dtype=torch.int32, device=dev)
    t.copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)))
    return t


def _sentinel(shape, dev):
    return torch.empty(shape, dtype=torch.int32, device=dev).view(torch.uint8).fill_(SENTINEL_BYTE).view(torch.int32)


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def _count_tensor(n_dev, dev):
    return None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=dev)


def _scratch(lib, capacity, dev):
    return torch.empty(lib.gsr_sort_scratch_bytes(capacity), dtype=torch.uint8, device=dev).fill_(SENTINEL_BYTE)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sort(dev, keys, vals, end_bit, n_dev=None):
    """gsr_sort_pairs_u32 on fresh buffers -> (first keys, first vals, second keys, second vals, result_in_tmp), host."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    cap = keys.shape[0]
    k, v = _dev(keys, dev), _dev(vals, dev)
    kt, vt = _sentinel(k.shape, dev), _sentinel(v.shape, dev)
    scratch, nd = _scratch(lib, cap, dev), _count_tensor(n_dev, dev)
    in_tmp = C.c_int32(-1)
    with torch.cuda.device(dev):
        _lib.check(lib.gsr_sort_pairs_u32(k.data_ptr(), v.data_ptr(), kt.data_ptr(), vt.data_ptr(), cap, _ptr(nd), end_bit,
                                          1 if vals.ndim == 1 else 2, scratch.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream, C.byref(in_tmp)), "gsr_sort_pairs_u32")
        torch.cuda.synchronize()
    return _host(k), _host(v), _host(kt), _host(vt), in_tmp.value


def _assert_sorted(res, keys, vals, end_bit, n, what):
    """The first n entries of the result buffer are the stable sort of the first n inputs; nothing at index >= n was
    written in either buffer; the flag names the buffer the pass count implies."""
    k, v, kt, vt, in_tmp = res
    assert in_tmp == sort_passes(end_bit) % 2, f"{what}: result_in_tmp {in_tmp} with {sort_passes(end_bit)} passes"
    ko, vo = (kt, vt) if in_tmp else (k, v)
    ref = _stable_order(keys[:n], end_bit)
    assert np.array_equal(vo[:n], vals[:n][ref]), f"{what}: values"
    assert np.array_equal(ko[:n], keys[:n][ref]), f"{what}: keys"
    assert np.array_equal(k[n:], keys[n:]) and np.array_equal(v[n:], vals[n:]), f"{what}: first buffer written past {n}"
    assert (kt[n:] == SENTINEL).all() and (vt[n:] == SENTINEL).all(), f"{what}: second buffer written past {n}"


# ---- (a) plain sort, both payload widths --------------------------------------------------------------------------------
END_BITS = [1, 5, 6, 7, 9, 10, 13, 18, 19, 24, 30, 32]
DISTS = ["uniform", "equal", "two_values", "sorted", "reversed", "quarter_run"]
SMALL_N = [1, 63, 64, 65]
LARGE_N = [SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 3 * SORT_TILE, 100_003]


def _plain_keys(dist, n, end_bit, rng):
    top = 1 << end_bit
    low = rng.integers(0, top, size=n, dtype=np.uint64)
    if dist == "equal":
        low[:] = low[0]
    elif dist == "two_values":
        a = int(low[0])
        low = np.where(rng.integers(0, 2, size=n) == 1, a, (a + 1 + int(rng.integers(0, top - 1))) % top).astype(np.uint64)
    elif dist == "sorted":
        low = np.sort(low)
    elif dist == "reversed":
        low = np.sort(low)[::-1]
    elif dist == "quarter_run":
        low[: n // 4] = low[0]
    return low.astype(np.uint32) | _high_bits(rng, n, end_bit)


# the four smallest sizes: the full cross product; the larger ones: every size sees every end_bit once, the payload width
# and the distribution rotating with (size, end_bit) so that each end_bit meets both widths and several distributions
PLAIN_CASES = [(w, e, n, d) for w in (1, 2) for e in END_BITS for n in SMALL_N for d in DISTS]
PLAIN_CASES += [(1 + (i + j) % 2, e, n, DISTS[(i + 2 * j) % len(DISTS)])
                for j, n in enumerate(LARGE_N) for i, e in enumerate(END_BITS)]


@pytest.mark.parametrize("val_words,end_bit,n,dist", PLAIN_CASES)
def test_sort_pairs_u32_matches_numpy_stable_argsort(gpu_device, val_words, end_bit, n, dist):
    rng = np.random.default_rng([val_words, end_bit, n, DISTS.index(dist)])
    keys, vals = _plain_keys(dist, n, end_bit, rng), _values(n, val_words)
    _assert_sorted(_sort(gpu_device, keys, vals, end_bit), keys, vals, end_bit, n, f"{dist} n={n} end_bit={end_bit}")


# ---- (b) device-side count ----------------------------------------------------------------------------------------------
CAPACITY = 5 * SORT_TILE + 17


@pytest.mark.parametrize("end_bit", [13, 32])
@pytest.mark.parametrize("val_words", [1, 2])
@pytest.mark.parametrize("n_dev", [0, 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE, CAPACITY - 1, CAPACITY])
def test_sort_pairs_u32_device_count(gpu_device, n_dev, val_words, end_bit):
    """The grid is sized for the capacity, the count is read on the device: the first n_dev outputs are the sort of the
    first n_dev inputs and the rest of every buffer is untouched (n_dev = 0: nothing is written anywhere)."""
    rng = np.random.default_rng([n_dev, val_words, end_bit])
    keys, vals = _plain_keys("quarter_run", CAPACITY, end_bit, rng), _values(CAPACITY, val_words)
    _assert_sorted(_sort(gpu_device, keys, vals, end_bit, n_dev=n_dev), keys, vals, end_bit, n_dev,
                   f"n_dev={n_dev} of {CAPACITY}")


# ---- (c) the extra pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_dev", [None, 2 * SORT_TILE + 1, 0], ids=["host_count", "device_count", "device_count_0"])
@pytest.mark.parametrize("nbits", [1, 3, 8])
def test_sort_extra_pass_u32_completes_a_24_bit_sort(gpu_device, nbits, n_dev):
    """Three passes on the low 24 bits, then the top-digit pass on bits [24, 24 + nbits): together a stable sort on
    24 + nbits bits.  With a device-side count of 0 the pass does not run and its outputs keep the sentinel."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    dev, cap = gpu_device, 3 * SORT_TILE + 17
    rng = np.random.default_rng([nbits, 1 << 20 if n_dev is None else n_dev])
    keys = rng.integers(0, 1 << 32, size=cap, dtype=np.uint64).astype(np.uint32)
    keys[: cap // 4] = (keys[: cap // 4] & np.uint32(0xFF000000)) | (keys[0] & np.uint32(0x00FFFFFF))
    vals = _values(cap, 2)
    n = cap if n_dev is None else n_dev
    k, v = _dev(keys, dev), _dev(vals, dev)
    kt, vt = _sentinel(k.shape, dev), _sentinel(v.shape, dev)
    ko, vo = _sentinel(k.shape, dev), _sentinel(v.shape, dev)
    scratch, nd = _scratch(lib, cap, dev), _count_tensor(n_dev, dev)
    in_tmp = C.c_int32(-1)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_sort_pairs_u32(k.data_ptr(), v.data_ptr(), kt.data_ptr(), vt.data_ptr(), cap, _ptr(nd), 24, 2,
                                          scratch.data_ptr(), s, C.byref(in_tmp)), "gsr_sort_pairs_u32")
        assert in_tmp.value == 1                    # three passes
        _lib.check(lib.gsr_sort_extra_pass_u32(kt.data_ptr(), vt.data_ptr(), ko.data_ptr(), vo.data_ptr(), cap, _ptr(nd),
                                               24, nbits, scratch.data_ptr(), s), "gsr_sort_extra_pass_u32")
        torch.cuda.synchronize()
    ko, vo, k24 = _host(ko), _host(vo), _host(kt)
    assert np.array_equal(k24[:n], keys[:n][_stable_order(keys[:n], 24)])
    ref = _stable_order(keys[:n], 24 + nbits)
    assert np.array_equal(vo[:n], vals[:n][ref])
    assert np.array_equal(ko[:n], keys[:n][ref])
    assert (ko[n:] == SENTINEL).all() and (vo[n:] == SENTINEL).all()


# ---- (d) tile runs from the sort ----------------------------------------------------------------------------------------
N_KEYS = [1, 2, 63, 64, 65, 510, 512, 513, 8160, 8192, 8193, 40_000]
TILE_DISTS = ["uniform", "one_key", "last_key", "even_keys", "one_each", "segment_edges", "heavy_tail"]
TILE_N = [257, SORT_TILE, SORT_TILE + 1, 20_011, 70_001, 300_000]
SEGMENT_LENGTHS = [0, 1, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE]


def _segment_edge_keys(n_keys, rng):
    """Segments (the items that share the first-pass digit) of SEGMENT_LENGTHS items side by side, the other segments
    0..2 items long.  The first-pass digit is the low widths[0] bits of the key (the whole key in a one-pass sort)."""
    lo_bits = sort_pass_plan(tile_sort_bits(n_keys))[0]
    digits = min(1 << lo_bits, n_keys)
    if digits >= len(SEGMENT_LENGTHS):
        counts = rng.integers(0, 3, size=digits)
        d0 = (digits - len(SEGMENT_LENGTHS)) // 2
        counts[d0:d0 + len(SEGMENT_LENGTHS)] = SEGMENT_LENGTHS
    else:
        counts = np.array(SEGMENT_LENGTHS[-digits:])
    parts = []
    for d, c in enumerate(counts):
        hi_max = (n_keys - 1 - d) >> lo_bits                  # d | hi << lo_bits stays below n_keys
        parts.append(d + (rng.integers(0, hi_max + 1, size=int(c)) << lo_bits))
    return rng.permutation(np.concatenate(parts))


def _tile_keys(dist, n_keys, n, rng):
    """Keys in [0, n_keys) (int64); `one_each` and `segment_edges` choose their own count."""
    if dist == "uniform":
        return rng.integers(0, n_keys, size=n)
    if dist == "one_key":
        return np.full(n, n_keys // 3)
    if dist == "last_key":
        return np.full(n, n_keys - 1)
    if dist == "even_keys":
        return 2 * rng.integers(0, (n_keys + 1) // 2, size=n)
    if dist == "one_each":
        return rng.permutation(n_keys)
    if dist == "segment_edges":
        return _segment_edge_keys(n_keys, rng)
    assert dist == "heavy_tail"
    heavy = np.array([0, n_keys // 2, n_keys - 1])
    return rng.permutation(np.concatenate([heavy[rng.integers(0, 3, size=n // 2)], rng.integers(0, n_keys, size=n - n // 2)]))


def _make_tile_case(dist, n_keys, n, seed, slack=0):
    """-> (keys [n + slack] with random bits above end_bit, n): `slack` entries of arbitrary keys past the count."""
    rng = np.random.default_rng(seed)
    low = _tile_keys(dist, n_keys, n, rng)
    n = low.shape[0]
    low = np.concatenate([low, rng.integers(0, 1 << 32, size=slack)])
    return low.astype(np.uint32) | _high_bits(rng, n + slack, tile_sort_bits(n_keys)), n


class _TileRunBuffers:
    """ranges / order / scratch of a tile-run sort; kept by the one test that reuses them."""

    def __init__(self, lib, dev, capacity, n_keys):
        self.ranges = _sentinel((n_keys, 2), dev)
        self.order = _sentinel((n_keys,), dev)
        self.scratch = _scratch(lib, capacity, dev)


def _tile_runs(dev, keys, n_keys, n_dev=None, bufs=None):
    """gsr_sort_tile_runs_u32 -> (sort result as _sort gives it, ranges [n_keys, 2], order [n_keys], runs_valid)."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    cap = keys.shape[0]
    vals = _values(cap, 1)
    k, v = _dev(keys, dev), _dev(vals, dev)
    kt, vt = _sentinel(k.shape, dev), _sentinel(v.shape, dev)
    bufs = bufs or _TileRunBuffers(lib, dev, cap, n_keys)
    nd = _count_tensor(n_dev, dev)
    in_tmp, valid = C.c_int32(-1), C.c_int32(-1)
    assert bufs.ranges.data_ptr() % 16 == 0
    with torch.cuda.device(dev):
        _lib.check(lib.gsr_sort_tile_runs_u32(k.data_ptr(), v.data_ptr(), kt.data_ptr(), vt.data_ptr(), cap, _ptr(nd),
                                              tile_sort_bits(n_keys), n_keys, bufs.ranges.data_ptr(), bufs.order.data_ptr(),
                                              bufs.scratch.data_ptr(), torch.cuda.current_stream(dev).cuda_stream,
                                              C.byref(in_tmp), C.byref(valid)), "gsr_sort_tile_runs_u32")
        torch.cuda.synchronize()
    return (_host(k), _host(v), _host(kt), _host(vt), in_tmp.value), _host(bufs.ranges), _host(bufs.order), valid.value


def _assert_tile_runs(out, keys, n_keys, n, what):
    res, ranges, order, valid = out
    end_bit = tile_sort_bits(n_keys)
    assert valid == (1 if sort_passes(end_bit) <= 2 else 0), f"{what}: runs_valid {valid}"
    _assert_sorted(res, keys, _values(keys.shape[0], 1), end_bit, n, what)
    if not valid:
        assert (ranges == SENTINEL).all() and (order == SENTINEL).all(), f"{what}: ranges / order written without runs"
        return
    sorted_keys = np.sort((keys[:n] & _mask(end_bit)).astype(np.int64))
    t = np.arange(n_keys)
    first, last = np.searchsorted(sorted_keys, t, "left"), np.searchsorted(sorted_keys, t, "right")
    expect = np.stack([first, last], axis=1)
    expect[first == last] = 0                                          # an empty key is exactly (0, 0)
    bad = np.nonzero((ranges.astype(np.int64) != expect).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} ranges differ, first key {bad[0]}: got {ranges[bad[0]]}, expect {expect[bad[0]]}"
    bucket = len_bucket(last - first)
    for c0 in range(0, n_keys, ORDER_CHUNK):
        c1 = min(c0 + ORDER_CHUNK, n_keys)
        o = order[c0:c1].astype(np.int64)
        assert np.array_equal(np.sort(o), np.arange(c0, c1)), f"{what}: order of chunk {c0} is no permutation"
        assert (np.diff(bucket[o]) <= 0).all(), f"{what}: length bucket increases along the order of chunk {c0}"


TILE_CASES = [(k, d, TILE_N[(i + j) % len(TILE_N)]) for i, k in enumerate(N_KEYS) for j, d in enumerate(TILE_DISTS)]


@pytest.mark.parametrize("n_keys,dist,n", TILE_CASES)
def test_tile_runs_match_searchsorted(gpu_device, n_keys, dist, n):
    keys, n = _make_tile_case(dist, n_keys, n, [n_keys, TILE_DISTS.index(dist), n])
    _assert_tile_runs(_tile_runs(gpu_device, keys, n_keys), keys, n_keys, n, f"{dist} n_keys={n_keys} n={n}")


@pytest.mark.parametrize("n_keys,dist,n", [(8160, "uniform", 70_001), (513, "segment_edges", 0), (64, "heavy_tail", 20_011)])
def test_tile_runs_device_count_below_capacity(gpu_device, n_keys, dist, n):
    keys, n = _make_tile_case(dist, n_keys, n, [n_keys, TILE_DISTS.index(dist), n, 1], slack=SORT_TILE + 3)
    assert keys.shape[0] > n
    _assert_tile_runs(_tile_runs(gpu_device, keys, n_keys, n_dev=n), keys, n_keys, n,
                      f"{dist} n_keys={n_keys} n_dev={n} of {keys.shape[0]}")


def test_tile_runs_are_not_derived_from_a_three_pass_sort(gpu_device):
    """More than 2^18 keys sort in three passes: the sort is still right, runs_valid is 0, ranges and order are untouched."""
    n_keys = (1 << 18) + 1
    assert sort_passes(tile_sort_bits(n_keys)) == 3
    keys, n = _make_tile_case("uniform", n_keys, 20_011, [n_keys])
    _assert_tile_runs(_tile_runs(gpu_device, keys, n_keys), keys, n_keys, n, "three passes")


# ---- (e) row scan beyond one round of 2048 columns ------------------------------------------------------------------------
ROWSCAN_N = 2048 * SORT_TILE + SORT_TILE + 5


def test_sort_pairs_u32_histogram_rows_longer_than_one_scan_round(gpu_device):
    """2050 blocks: the row scan's loop takes a second trip, whose group of columns is partial."""
    rng = np.random.default_rng(2050)
    keys, vals = _plain_keys("quarter_run", ROWSCAN_N, 13, rng), _values(ROWSCAN_N, 2)
    _assert_sorted(_sort(gpu_device, keys, vals, 13), keys, vals, 13, ROWSCAN_N, "2050 blocks")


def test_tile_runs_histogram_rows_longer_than_one_scan_round(gpu_device):
    """64 segments of about 131 000 items: the segmented pass uses 2050 to 2113 columns, and the runs are read back from
    row prefixes of the second trip."""
    keys, n = _make_tile_case("uniform", 8160, ROWSCAN_N, [8160, 2050])
    _assert_tile_runs(_tile_runs(gpu_device, keys, 8160), keys, 8160, n, "2050+ blocks")


# ---- (f) an empty frame after a full one ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [510, 8160], ids=["one_pass", "two_passes"])
def test_empty_frame_does_not_inherit_the_previous_frames_runs(gpu_device, n_keys):
    """A sort of a few thousand items, then a device-side count of 0 into the SAME scratch and ranges: the digit totals the
    ranges are derived from must be published as zeros, or the previous frame's runs come back."""
    from mvs_gaussian_splatting_amd import _lib
    keys, n = _make_tile_case("uniform", n_keys, 5000, [n_keys, 5000])
    bufs = _TileRunBuffers(_lib.load(), gpu_device, n, n_keys)
    _assert_tile_runs(_tile_runs(gpu_device, keys, n_keys, n_dev=n, bufs=bufs), keys, n_keys, n, "full frame")
    bufs.order = _sentinel((n_keys,), gpu_device)              # scratch and ranges stay as the full frame left them
    out = _tile_runs(gpu_device, keys, n_keys, n_dev=0, bufs=bufs)
    assert (out[1] == 0).all(), "empty frame: a range is not (0, 0)"
    _assert_tile_runs(out, keys, n_keys, 0, "empty frame")


# ---- (g) determinism ----------------------------------------------------------------------------------------------------------
def test_tile_runs_are_deterministic(gpu_device):
    keys, n = _make_tile_case("heavy_tail", 8160, 70_001, [8160, 7])
    a, b = _tile_runs(gpu_device, keys, 8160), _tile_runs(gpu_device, keys, 8160)
    _assert_tile_runs(a, keys, 8160, n, "first run")
    _assert_tile_runs(b, keys, 8160, n, "second run")       # order: compared through its properties only
    for x, y in zip(a[0][:4], b[0][:4]):
        assert np.array_equal(x, y)
    assert a[0][4] == b[0][4] and np.array_equal(a[1], b[1])
