"""The three densification plans at the C ABI (``gsr_densify_plan``, ``gsr_densify_fork_plan``, ``gsr_grow_plan``) with
their gathers, on the designed cases of tests/densify_plan_restate.py: sizes past one 32-entry line of the block-counter
scan, counter arrays at every residue of ``nb + 1`` modulo 4, a model past one round of 32768 blocks, and rows that sit
exactly on each decision threshold.

Everything compared is an integer or a bit copy: the counts, the source row of every output row (gathered from
``arange(P)``, exact in float32 below 2^24), ``vidx`` / ``src`` / ``selected``.  The only arithmetic read back is the split
children's ``xyz``, built to be exact (identity rotation, unit scale, integer noise).  Every workspace is followed by a
guard band that must come back untouched, and every plan runs twice with identical bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import densify_plan_restate as R

pytestmark = pytest.mark.gpu
GUARD = 4096
SENTINEL = -7.0


@pytest.fixture(scope="module")
def lib():
    from mvs_gaussian_splatting_amd import _lib
    return _lib.load()


_built = {}


def _case(name, dev):
    """The case and its inputs on the device; the small cases are built once and shared, never modified."""
    if name in _built:
        return _built[name]
    c = R.build(name)
    t = {k: torch.from_numpy(getattr(c, k)).to(dev) for k in ("accum", "denom", "scaling", "opacity", "split_scale")}
    t["rows"] = torch.arange(c.P, dtype=torch.float32, device=dev)
    if name != "two_rounds":
        _built[name] = (c, t)
    return c, t


def _workspace(nbytes, dev):
    ws = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    return ws


def _guard_intact(ws, nbytes):
    return bool((ws[nbytes:] == 0xA5).all())


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _check(rc, what):
    from mvs_gaussian_splatting_amd import _lib
    _lib.check(rc, what)


def _plain_plan(lib, c, t, use_ws, dev):
    nbytes = lib.gsr_densify_workspace_bytes(c.P)
    ws = _workspace(nbytes, dev)
    counts = (C.c_uint32 * 4)()
    _check(lib.gsr_densify_plan(c.P, t["accum"].data_ptr(), t["denom"].data_ptr(), t["scaling"].data_ptr(),
                                t["opacity"].data_ptr(), R.THR, R.PDE, R.MIN_OPACITY, R.WS if use_ws else -1.0,
                                ws.data_ptr(), nbytes, counts, _stream(dev)), "gsr_densify_plan")
    assert _guard_intact(ws, nbytes), "gsr_densify_plan wrote past its workspace"
    return ws, counts


def _plain_gather(lib, c, src, ws, counts, zero_new, n_out, dev):
    w = src.numel() // c.P
    dst = torch.full((n_out, w), SENTINEL, dtype=torch.float32, device=dev)
    _check(lib.gsr_densify_gather_rows(c.P, w, src.data_ptr(), ws.data_ptr(), counts, zero_new, dst.data_ptr(),
                                       _stream(dev)), "gsr_densify_gather_rows")
    return dst


def _plain_order_twice(lib, c, t, use_ws, dev):
    """Counts and gathered row numbers of two runs of the plain plan; asserts the counts before anything is sized by them."""
    want_counts, want_order = R.densify_expected(R.designed_flags(c, use_ws))
    outs = []
    for _ in range(2):
        ws, counts = _plain_plan(lib, c, t, use_ws, dev)
        assert list(counts) == want_counts, (c.name, use_ws, list(counts), want_counts)
        outs.append(_plain_gather(lib, c, t["rows"], ws, counts, 0, want_order.size, dev))
    assert torch.equal(outs[0], outs[1]), "two runs of the plan differ"
    got = outs[0].cpu().numpy().reshape(-1)
    assert np.array_equal(got.astype(np.int64), want_order), _first_difference(got, want_order)
    return ws, counts


def _first_difference(got, want):
    bad = np.flatnonzero(np.asarray(got).astype(np.int64) != np.asarray(want).astype(np.int64))
    k = int(bad[0])
    return f"{bad.size} of {len(want)} rows differ, first at output row {k}: got {got[k]}, want {want[k]}"


@pytest.mark.parametrize("use_ws", [True, False], ids=["world_limit", "no_world_limit"])
@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_plain_plan_counts_and_row_order(gpu_device, lib, name, use_ws):
    c, t = _case(name, gpu_device)
    _plain_order_twice(lib, c, t, use_ws, gpu_device)


def test_plain_gather_three_floats_zero_new(gpu_device, lib):
    """Kept rows are bit copies (any bit pattern, NaNs included), appended rows are +0."""
    c, t = _case("odd2", gpu_device)
    want_counts, want_order = R.densify_expected(R.designed_flags(c, True))
    bits = torch.from_numpy(np.random.default_rng(5).integers(-2 ** 31, 2 ** 31, (c.P, 3), dtype=np.int64)
                            .astype(np.int32))
    src = bits.view(torch.float32).to(gpu_device)
    outs = []
    for _ in range(2):
        ws, counts = _plain_plan(lib, c, t, True, gpu_device)
        assert list(counts) == want_counts
        outs.append(_plain_gather(lib, c, src, ws, counts, 1, want_order.size, gpu_device).view(torch.int32).cpu())
    assert torch.equal(outs[0], outs[1])
    n_keep = want_counts[0]
    assert torch.equal(outs[0][:n_keep], bits[torch.from_numpy(want_order[:n_keep])])
    assert n_keep < want_order.size and not outs[0][n_keep:].any()


def test_split_children_read_the_noise_row_of_their_split_rank(gpu_device, lib):
    """odd1, with the world limit: some split-selected parents lose their children, so the rank among the kept children
    and the rank among the split-selected differ.  Identity rotation, scaling 0 and noise (j, 0, 0) in row j make
    xyz_child - xyz_parent the noise row exactly."""
    dev = gpu_device
    c, t = _case("odd1", dev)
    flags = R.designed_flags(c, True)
    (n_keep, n_clone, n_child, n_sel), order = R.densify_expected(flags)
    assert n_sel > n_child > 0
    ws, counts = _plain_order_twice(lib, c, t, True, dev)
    i = torch.arange(c.P, dtype=torch.float32)
    xyz = torch.stack((i, 2 * i, 3 * i), dim=1).contiguous()
    rotation = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(c.P, 1).contiguous()
    noise = torch.zeros(2 * n_sel, 3)
    noise[:, 0] = torch.arange(2 * n_sel, dtype=torch.float32)
    zeros = torch.zeros(c.P, 3, device=dev)
    d_xyz, d_rotation, d_noise = xyz.to(dev), rotation.to(dev), noise.to(dev)
    outs = []
    for _ in range(2):
        dst_xyz = torch.full((order.size, 3), SENTINEL, device=dev)
        dst_scaling = torch.full((order.size, 3), SENTINEL, device=dev)
        _check(lib.gsr_densify_split_children(c.P, d_xyz.data_ptr(), zeros.data_ptr(), d_rotation.data_ptr(),
                                              d_noise.data_ptr(), ws.data_ptr(), counts, dst_xyz.data_ptr(),
                                              dst_scaling.data_ptr(), _stream(dev)), "gsr_densify_split_children")
        outs.append((dst_xyz.cpu(), dst_scaling.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    got_xyz, got_scaling = outs[0]
    first = n_keep + n_clone
    assert bool((got_xyz[:first] == SENTINEL).all()) and bool((got_scaling[:first] == SENTINEL).all())
    parents = torch.from_numpy(np.flatnonzero(flags & R.CHILD))
    rank = torch.from_numpy(R.split_ranks(flags))[parents].float()
    for k in range(2):
        rows = got_xyz[first + k * n_child: first + (k + 1) * n_child]
        want = torch.stack((rank + k * n_sel, torch.zeros(n_child), torch.zeros(n_child)), dim=1)
        assert torch.equal(rows - xyz[parents], want), f"children #{k + 1} read another noise row"
    child_scaling = got_scaling[first:]
    assert bool((child_scaling == child_scaling[0, 0]).all()) and float(child_scaling[0, 0]) < 0.0     # log(1 / 1.6)


def _fork_plan(lib, c, t, use_ws, learned, dev):
    nbytes = lib.gsr_densify_fork_workspace_bytes(c.P)
    ws = _workspace(nbytes, dev)
    counts = (C.c_uint32 * 5)()
    _check(lib.gsr_densify_fork_plan(c.P, t["accum"].data_ptr(), t["denom"].data_ptr(), t["scaling"].data_ptr(),
                                     t["opacity"].data_ptr(), t["split_scale"].data_ptr() if learned else None, R.THR,
                                     R.PDE, R.MIN_OPACITY, R.WS if use_ws else -1.0, ws.data_ptr(), nbytes, counts,
                                     _stream(dev)), "gsr_densify_fork_plan")
    assert _guard_intact(ws, nbytes), "gsr_densify_fork_plan wrote past its workspace"
    return ws, counts


@pytest.mark.parametrize("use_ws", [True, False], ids=["world_limit", "no_world_limit"])
@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_fork_plan_counts_and_row_order(gpu_device, lib, name, use_ws):
    """With and without split_scale_raw, in the clone + split (c = 2) and the grow (c = 4) order; every role copies.
    Rows of one float take the scalar gather, rows of four the 16-byte one."""
    from mvs_gaussian_splatting_amd import _lib
    dev = gpu_device
    c, t = _case(name, dev)
    policy = _lib.ROW_POLICY(_lib.ROW_COPY, _lib.ROW_COPY, _lib.ROW_COPY)
    rows4 = t["rows"][:, None].repeat(1, 4).contiguous()
    for learned in (False, True):
        flags = R.designed_flags(c, use_ws, learned, fork=True)
        for grow in (False, True):
            want_counts, want_order = R.fork_expected(flags, grow)
            src = rows4 if grow else t["rows"]
            w = 4 if grow else 1
            outs = []
            for _ in range(2):
                ws, counts = _fork_plan(lib, c, t, use_ws, learned, dev)
                assert list(counts) == want_counts, (name, use_ws, learned, list(counts), want_counts)
                dst = torch.full((want_order.size, w), SENTINEL, device=dev)
                _check(lib.gsr_densify_fork_gather_rows(c.P, w, src.data_ptr(), ws.data_ptr(), counts, 1 if grow else 0,
                                                        policy, 0.0, dst.data_ptr(), _stream(dev)),
                       "gsr_densify_fork_gather_rows")
                outs.append(dst)
            assert torch.equal(outs[0], outs[1])
            got = outs[0].cpu().numpy()
            assert (got == got[:, :1]).all()
            assert np.array_equal(got[:, 0].astype(np.int64), want_order), \
                (name, learned, grow, _first_difference(got[:, 0], want_order))


def _grow_plan_check(lib, c, t, split_mode, dev):
    from mvs_gaussian_splatting_amd import _lib
    want_vidx, want_src, want_selected, want_counts = R.grow_designed(c, split_mode)
    mode = _lib.SPLIT_DISTANCE if split_mode else _lib.GROW_DIR
    nbytes = lib.gsr_grow_workspace_bytes(c.P)
    outs = []
    for _ in range(2):
        ws = _workspace(nbytes, dev)
        vidx = torch.full((c.P,), -5, dtype=torch.int32, device=dev)
        src = torch.full((c.P,), -5, dtype=torch.int32, device=dev)
        selected = torch.full((c.P,), 7, dtype=torch.uint8, device=dev)
        counts = (C.c_uint32 * 2)()
        _check(lib.gsr_grow_plan(c.P, t["accum"].data_ptr(), t["denom"].data_ptr(), t["scaling"].data_ptr(), R.THR, R.PDE,
                                 mode, ws.data_ptr(), nbytes, vidx.data_ptr(), src.data_ptr(), selected.data_ptr(),
                                 counts, _stream(dev)), "gsr_grow_plan")
        assert _guard_intact(ws, nbytes), "gsr_grow_plan wrote past its workspace"
        assert list(counts) == want_counts, (c.name, split_mode, list(counts), want_counts)
        outs.append((vidx.cpu().numpy(), src.cpu().numpy(), selected.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b), "two runs of the plan differ"
    vidx, src, selected = outs[0]
    G = want_counts[0]
    assert np.array_equal(selected, want_selected)
    assert np.array_equal(vidx, want_vidx), _first_difference(vidx, want_vidx)
    assert np.array_equal(src[:G], want_src), _first_difference(src[:G], want_src)
    assert (src[G:] == -5).all()


@pytest.mark.parametrize("split_mode", [False, True], ids=["grow", "split"])
@pytest.mark.parametrize("name", R.SMALL_CASES)
def test_grow_plan_rows_and_counts(gpu_device, lib, name, split_mode):
    c, t = _case(name, gpu_device)
    _grow_plan_check(lib, c, t, split_mode, gpu_device)


def test_two_rounds_of_the_block_scan(gpu_device, lib):
    """nb = 32802 > 32768: the scan's second round with its carry, a whole line and a scalar tail inside round two, and
    counter arrays 32803 words apart before the padding.  The plain plan in both prune modes and the grow plan in both
    modes; about 200 MB of inputs and 150 MB of workspace, freed at the end."""
    dev = gpu_device
    c, t = _case("two_rounds", dev)
    assert c.nb > 32768
    try:
        _plain_order_twice(lib, c, t, True, dev)
        _plain_order_twice(lib, c, t, False, dev)
        _grow_plan_check(lib, c, t, False, dev)
        _grow_plan_check(lib, c, t, True, dev)
    finally:
        del t, c
        torch.cuda.empty_cache()
