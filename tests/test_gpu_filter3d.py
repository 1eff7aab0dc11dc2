"""The 3D smoothing filter on the device (csrc/filter3d.hip; filter3d.py): the sampling pass and the width
against the float32 restatement (tests/filter3d_restate.py) bit for bit, the fused application and its gradient against
the float64 restatement rounded once and against the exact definition at range, planted per-row states through the global
reduction past one wave and one trip, ``accumulate`` and V = 0 at the entry points, ``render`` with a filter on both
paths, three training iterations across a densification, and the trainer's periodic and MCMC recomputes."""
import numpy as np
import pytest
import torch
from torch import nn

from conftest import small_scene
import filter3d_restate as R

pytestmark = pytest.mark.gpu
F = np.float32


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- sampling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 1000])
def test_sampling_is_the_restatements_bits(gpu_device, P, monkeypatch):
    """V in {1, 2, 3} in one launch, and V = 5 fed in chunks of two views that accumulate; both rules; twice."""
    from mvs_gaussian_splatting_amd import compute_3d_filter, filter3d
    for V, chunk in ((1, None), (2, None), (3, None), (5, 2)):
        xyz, cams = R.gate_scene(P, V)
        dev_xyz = torch.from_numpy(xyz).to(gpu_device)
        monkeypatch.setattr(filter3d, "VIEW_CHUNK", chunk or filter3d.MAX_VIEWS)
        min_depth, max_rate, seen = R.sample(xyz, cams)
        if P >= 257:
            assert 0 < seen.sum() < P, "points on both sides of the gates"
        for rule in ("mip_splatting", "paper"):
            want, want_flag = R.width(min_depth, max_rate, seen, cams, rule=rule)
            out = torch.full((P,), float("nan"), device=gpu_device)
            got, flag = compute_3d_filter(dev_xyz, cams, rule=rule, out=out)
            again, flag2 = compute_3d_filter(dev_xyz, cams, rule=rule)
            assert got is out and got.dtype == torch.float32 and flag.dtype == torch.int32 and tuple(flag.shape) == (1,)
            assert np.array_equal(bits(got), want.view(np.uint32)), (V, rule)
            assert np.array_equal(bits(again), bits(got)) and int(flag) == int(flag2) == want_flag, (V, rule)


def test_sampling_arrays_boundaries_and_the_unseen(gpu_device):
    """Through the entry points themselves, into arrays full of garbage: the three per-Gaussian values, the dyadic
    boundary case (z == near out; u == -m W and u == (1 + m) W in), a table that sees nothing, and P = 0."""
    from mvs_gaussian_splatting_amd import _lib, compute_3d_filter, filter3d
    lib, dev = _lib.load(), gpu_device
    cam = R.camera(64, 32, 32.0, 32.0)
    xyz = np.array([[0.0, 0.0, 0.25], [0.0, 0.0, 0.2500001], [-1.5, 0.0, 1.0], [1.5, 0.0, 1.0], [-1.5000001, 0.0, 1.0],
                    [1.500001, 0.0, 1.0], [0.0, -0.75, 1.0], [0.0, 0.75, 1.0], [0.0, 0.7500001, 1.0], [0.0, 0.0, -3.0],
                    [np.nan, 0.0, 1.0], [0.0, 0.0, 8.0]], dtype=F)
    want_seen = np.array([0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1], dtype=bool)
    P = len(xyz)
    rows, focal_max = filter3d.view_table([cam])
    table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
    dev_xyz = torch.from_numpy(xyz).to(dev)
    min_depth, max_rate = torch.full((P,), -7.0, device=dev), torch.full((P,), 1e9, device=dev)
    seen = torch.full((P,), 9, dtype=torch.uint8, device=dev)
    ws_bytes = lib.gsr_filter3d_workspace_bytes(P)
    ws = torch.full((ws_bytes,), 0xAB, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.gsr_filter3d_sample(dev_xyz.data_ptr(), P, table.data_ptr(), 1, 0.25, 0.25, 0, min_depth.data_ptr(),
                                       max_rate.data_ptr(), seen.data_ptr(), ws.data_ptr(), ws_bytes, stream), "sample")
    w_depth, w_rate, w_seen = R.sample(xyz, [cam], near=0.25, margin=0.25)
    assert np.array_equal(w_seen, want_seen) and np.array_equal(seen.cpu().numpy().astype(bool), want_seen)
    assert np.array_equal(bits(min_depth), w_depth.view(np.uint32)) and np.array_equal(bits(max_rate), w_rate.view(np.uint32))
    for rule in ("mip_splatting", "paper"):
        got, flag = compute_3d_filter(dev_xyz, [cam], near=0.25, margin=0.25, rule=rule)
        want, _ = R.compute(xyz, [cam], near=0.25, margin=0.25, rule=rule)
        assert int(flag) == 0 and np.array_equal(bits(got), want.view(np.uint32))
        assert (got[torch.from_numpy(~want_seen).to(dev)] == got[11]).all(), "the unseen take the farthest seen one's"
    behind = np.eye(4, dtype=F)
    behind[3, 2] = -100.0
    got, flag = compute_3d_filter(dev_xyz, [R.camera(64, 32, 32.0, 32.0, behind)] * 2, near=0.25, margin=0.25)
    assert int(flag) == 1 and not bits(got).any(), "no Gaussian seen: filter 0 everywhere and the flag"
    got, flag = compute_3d_filter(dev_xyz[:0], [cam])
    assert tuple(got.shape) == (0,) and int(flag) == 1


# ---- the entry points themselves: planted per-row states, accumulate, V = 0 ---------------------------------------------------------
class _Pass:
    """The two calls of a sampling pass through the C ABI, over arrays the test owns: ``P`` rows, the workspace filled with
    0xAB bytes, ``min_depth`` / ``max_rate`` / ``seen`` set by ``plant``."""

    def __init__(self, dev, P, xyz=None):
        from mvs_gaussian_splatting_amd import _lib
        self._lib, self.lib, self.dev, self.P = _lib, _lib.load(), dev, P
        self.xyz = torch.zeros(P, 3, device=dev) if xyz is None else torch.from_numpy(np.ascontiguousarray(xyz, dtype=F)).to(dev)
        self.min_depth, self.max_rate = torch.empty(P, device=dev), torch.empty(P, device=dev)
        self.seen = torch.empty(P, dtype=torch.uint8, device=dev)
        self.ws_bytes = int(self.lib.gsr_filter3d_workspace_bytes(P))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.filter, self.flag = torch.empty(P, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream(dev).cuda_stream

    def plant(self, min_depth, max_rate, seen):
        for dst, src in ((self.min_depth, min_depth), (self.max_rate, max_rate), (self.seen, seen)):
            dst.copy_(torch.from_numpy(np.ascontiguousarray(src)) if isinstance(src, np.ndarray) else torch.full_like(dst, src))
        self.ws.fill_(0xAB)

    def sample(self, cams, accumulate, near=0.2, margin=0.15):
        from mvs_gaussian_splatting_amd import filter3d
        table = None
        if cams:
            table = torch.frombuffer(bytearray(bytes(filter3d.view_table(cams)[0])), dtype=torch.uint8).to(self.dev)
        self._lib.check(self.lib.gsr_filter3d_sample(self.xyz.data_ptr(), self.P, table.data_ptr() if cams else None, len(cams),
                                                     near, margin, accumulate, self.min_depth.data_ptr(),
                                                     self.max_rate.data_ptr(), self.seen.data_ptr(), self.ws.data_ptr(),
                                                     self.ws_bytes, self.stream), "gsr_filter3d_sample")
        torch.cuda.synchronize(self.dev)                             # the table lives until the launch has read it

    def finish(self, rule, focal_max, variance=0.2):
        self.filter.fill_(float("nan"))
        self.flag.fill_(-1)
        self._lib.check(self.lib.gsr_filter3d_finish(self.P, self.min_depth.data_ptr(), self.max_rate.data_ptr(),
                                                     self.seen.data_ptr(), R.RULES[rule], focal_max, variance,
                                                     self.ws.data_ptr(), self.ws_bytes, self.filter.data_ptr(),
                                                     self.flag.data_ptr(), self.stream), "gsr_filter3d_finish")
        return bits(self.filter), int(self.flag)

    def arrays(self):
        return bits(self.min_depth), bits(self.max_rate), self.seen.cpu().numpy()

    def pairs(self):
        """The per-64-row (max, min) pairs the sampling call left at the head of the workspace."""
        n = (self.P + R.WAVE - 1) // R.WAVE
        return self.ws[:8 * n].cpu().numpy().view(F).reshape(n, 2)


@pytest.mark.parametrize("P", R.PLANT_SIZES)
def test_planted_states_through_the_reduction_past_one_wave_and_one_trip(gpu_device, P):
    """``gsr_filter3d_sample(V = 0, views = NULL, accumulate = 1)`` loads the caller's per-row state, runs an empty view
    loop, writes the state back unchanged and the per-wave pairs from it; ``gsr_filter3d_finish`` follows.  So D, R and
    the none-seen flag come from rows the test chose: a single seen row in each of the pairs ``R.plant_pairs(P)``; D and R
    planted in different pairs, reduce waves and trips of the strided loop, every 7th row unseen; pairs 1 to 62 and the
    partial last wave wholly unseen.  (tests/test_filter3d_host.py pins the reduce lane, wave and trip each pair reaches:
    4097 rows put data in reduce wave 1, 65536 give every lane one pair, 65537 give lane 0 a second trip, 131073 a third.)
    A maximum and a minimum do not depend on the order: the filter is ``R.width`` of the planted arrays bit for bit under
    both rules, the flag exactly, the pairs exactly, and a second run gives the same bits.
    Measured on an MI355X: 16, 19, 22 and 31 planted states at the four sizes, each under both rules, all bit-equal to the
    restatement, and the second run equal to the first in every bit."""
    run = _Pass(gpu_device, P)
    cam = R.camera(64, 48, 64.0, 64.0)                              # read for its focal length alone
    focal_max = float(R.focal(cam)[2])
    cases = R.planted_cases(P)
    for name, d, r, hit in cases:
        seen = hit.astype(bool)
        run.plant(d, r, hit)
        run.sample([], 1)
        got_d, got_r, got_hit = run.arrays()
        assert np.array_equal(got_d, d.view(np.uint32)) and np.array_equal(got_r, r.view(np.uint32)) and \
            np.array_equal(got_hit, hit), (name, "V = 0 with accumulate = 1 writes the arrays back unchanged")
        assert np.array_equal(run.pairs().view(np.uint32), R.wave_pairs(d, r, hit).view(np.uint32)), (name, "per-wave pairs")
        for rule in ("mip_splatting", "paper"):
            want, want_flag = R.width(d, r, seen, [cam], rule=rule)
            got, flag = run.finish(rule, focal_max)
            assert flag == want_flag == 0, (name, rule, "none_seen")
            assert np.array_equal(got, want.view(np.uint32)), (name, rule, int((got != want.view(np.uint32)).sum()))
            again, flag2 = run.finish(rule, focal_max)
            assert flag2 == 0 and np.array_equal(again, got), (name, rule, "the same bits from run to run")
            if name.startswith("D in"):                              # the unseen take exactly the planted value's width
                own = R.width(np.array([9.0], dtype=F), np.array([0.5], dtype=F), np.array([True]), [cam], rule=rule)[0][0]
                assert (want[~seen] == own).all() and (~seen).sum() > P // 8
            elif name.startswith("one seen"):
                assert (want == want[seen][0]).all() and want[0] > 0
    neutral = run.pairs()                                            # of the last case: the wholly unseen waves
    assert cases[-1][0].startswith("pairs 1 to 62") and np.isneginf(neutral[1:63, 0]).all() and np.isposinf(neutral[1:63, 1]).all()
    assert np.isneginf(neutral[-1, 0]) and np.isposinf(neutral[-1, 1]) and np.isfinite(neutral[[0, 63]]).all()
    print(f"[filter3d] P={P}: {len(cases)} planted states x 2 rules bit-equal to the restatement, twice")
    if P == 65537:
        d, r, hit = R._unseen(P)
        run.plant(d, r, hit)
        run.sample([], 1)
        for rule in ("mip_splatting", "paper"):
            got, flag = run.finish(rule, focal_max)
            assert flag == 1 and not got.any(), "nothing seen: the flag, and a filter whose bits are all zero"


@pytest.mark.parametrize("P,late", [(4097, 64), (65537, 1024)])
def test_the_public_pass_takes_its_maximum_from_a_late_pair(gpu_device, P, late):
    """``compute_3d_filter`` on a constructed scene: the identity camera, points on the optical axis at distinct dyadic
    depths 1 + i 2^-17 (every float32 operation exact), rows from 64 on behind the camera except one row of pair ``late``
    at depth 4, the farthest seen.  D and R come from that pair alone -- reduce wave 1 at 4097 rows, lane 0's second trip
    at 65537 --, and about every row past 63 is unseen and takes them.  Bit for bit ``R.compute``, both rules."""
    from mvs_gaussian_splatting_amd import compute_3d_filter
    cam = R.camera(64, 32, 32.0, 32.0)
    xyz = np.zeros((P, 3), dtype=F)
    xyz[:, 2] = 1.0 + np.arange(P) * 2.0 ** -17
    xyz[64:, 2] *= -1.0
    far = R.plant_row(P, late)
    xyz[far, 2] = 4.0
    min_depth, max_rate, seen = R.sample(xyz, [cam])
    assert seen.sum() == 65 and seen[far] and far // 64 == late and len(np.unique(min_depth[seen])) == 65
    assert min_depth[seen].max() == min_depth[far] == 4.0 and max_rate[seen].min() == max_rate[far] == 8.0
    dev_xyz = torch.from_numpy(xyz).to(gpu_device)
    for rule in ("mip_splatting", "paper"):
        want, _ = R.width(min_depth, max_rate, seen, [cam], rule=rule)
        got, flag = compute_3d_filter(dev_xyz, [cam], rule=rule)
        assert int(flag) == 0 and np.array_equal(bits(got), want.view(np.uint32)), rule
        assert (want[~seen] == want[far]).all() and want[far] > want[:64].max()


def test_accumulate_and_an_empty_table_at_the_entry_points(gpu_device):
    """The promises of include/gsr.h, on 130 rows (two full waves and two rows) into arrays full of garbage:
    ``accumulate = 0`` ignores what the arrays hold, also with V = 0 (the start values); ``accumulate = 1`` carries all
    three arrays forward, across a launch that sees nothing and across V = 0 with a NULL table; two chunks give the bits of
    one table."""
    P = 130
    xyz, (cam_a, cam_b) = R.gate_scene(P, 2)
    behind = np.eye(4, dtype=F)
    behind[3, 2] = -100.0
    blind = R.camera(64, 48, 60.0, 66.0, behind)
    w_a, w_ab = R.sample(xyz, [cam_a]), R.sample(xyz, [cam_a, cam_b])
    only_a = w_a[2] & ~R.sample(xyz, [cam_b])[2]
    assert only_a.any() and (w_ab[2] & ~w_a[2]).any() and not w_ab[2].all() and not R.sample(xyz, [blind])[2].any()
    run = _Pass(gpu_device, P, xyz)

    def same(want):
        d, r, hit = run.arrays()
        pairs = R.wave_pairs(want[0], want[1], want[2])
        return np.array_equal(d, want[0].view(np.uint32)) and np.array_equal(r, want[1].view(np.uint32)) and \
            np.array_equal(hit, want[2].astype(np.uint8)) and np.array_equal(run.pairs().view(np.uint32), pairs.view(np.uint32))

    run.plant(-7.0, 1e9, 9)
    run.sample([], 0)
    assert same((np.full(P, np.inf, dtype=F), np.zeros(P, dtype=F), np.zeros(P, dtype=bool))), "V = 0: the start values"
    run.plant(-7.0, 1e9, 9)
    run.sample([cam_a], 0)
    assert same(w_a), "accumulate = 0 ignores the garbage"
    run.sample([cam_b], 1)
    assert same(w_ab), "two chunks are one table"
    run.plant(-7.0, 1e9, 9)
    run.sample([cam_a], 0)
    run.sample([blind], 1)
    assert same(w_a), "a launch that sees nothing changes nothing"
    run.sample([cam_b], 1)
    assert same(w_ab), "a row seen only by the first chunk stays seen, with its values"
    d, r, hit = run.arrays()
    assert hit[only_a].all() and np.array_equal(d[only_a], w_a[0][only_a].view(np.uint32))
    run.ws.fill_(0xAB)
    run.sample([], 1)
    assert same(w_ab), "accumulate = 1 with V = 0 and a NULL table changes nothing (and writes the pairs again)"
    for rule in ("mip_splatting", "paper"):
        want, want_flag = R.width(*w_ab, [cam_a, cam_b], rule=rule)
        got, flag = run.finish(rule, focal_max=float(max(R.focal(c)[2] for c in (cam_a, cam_b))))
        assert flag == want_flag == 0 and np.array_equal(got, want.view(np.uint32)), rule


# ---- application ----------------------------------------------------------------------------------------------------------------
def _apply_case(n, seed=0):
    """Raw scales in [-12, 4], raw opacities in [-12, 12], filters from 0 to 10 times the scale, and rows with f = 0."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-12.0, 4.0, size=(n, 3)).astype(F)
    o = rng.uniform(-12.0, 12.0, size=(n, 1)).astype(F)
    f = (np.exp(s.astype(np.float64).mean(axis=1)) * rng.uniform(0.0, 10.0, size=n)).astype(F)
    f[::7] = 0.0
    return s, o, f, rng.standard_normal((n, 3)).astype(F), rng.standard_normal((n, 1)).astype(F)


@pytest.mark.parametrize("n", [1, 65, 257, 20000])
def test_application_and_its_gradient_against_float64(gpu_device, n):
    """Forward: at most one float32 place from the float64 restatement rounded once (two correctly rounded float64
    evaluations differ by no more: host and device exp / log1p disagree only in the last place of a double).  Backward:
    the same one-place bar on every component -- it applied to all of them: the kernel evaluates the gradient in float64
    and rounds once, so a component that is a difference of two terms loses double places, not float32 ones; the
    allowance for that is 1e-14 of the terms' magnitudes (64 double roundings), far below one float32 place."""
    from mvs_gaussian_splatting_amd import apply_3d_filter, filtered_scaling_opacity
    s, o, f, g_s, g_o = _apply_case(n, seed=n)
    dev = gpu_device
    ds, do, df = (torch.from_numpy(a).to(dev) for a in (s, o, f))
    ds.requires_grad_(True)
    do.requires_grad_(True)
    se, oe = apply_3d_filter(ds, do, df)
    assert se.shape == ds.shape and oe.shape == do.shape and se.dtype == oe.dtype == torch.float32
    want_s, want_o = R.apply(s, o, f)
    got_s, got_o = se.detach().cpu().numpy(), oe.detach().cpu().numpy()
    eq_s, eq_o = np.mean(got_s.view(np.uint32) == want_s.view(np.uint32)), np.mean(got_o.view(np.uint32) == want_o.view(np.uint32))
    print(f"[filter3d] n={n}: forward bit-equal share: scaling {eq_s:.5f}, opacity {eq_o:.5f}; "
          f"worst {R.ulps(got_s, want_s.astype(np.float64)).max():.0f} / {R.ulps(got_o, want_o.astype(np.float64)).max():.0f} places")
    assert R.ulps(got_s, want_s.astype(np.float64)).max() <= 1 and R.ulps(got_o, want_o.astype(np.float64)).max() <= 1
    zero = f == 0
    assert np.array_equal(got_s[zero].view(np.uint32), s[zero].view(np.uint32)), "f = 0 rows exactly unchanged"
    assert np.array_equal(got_o[zero].view(np.uint32), o[zero].view(np.uint32))
    torch.autograd.backward([se, oe], [torch.from_numpy(g_s).to(dev), torch.from_numpy(g_o).to(dev)])
    w_ds, w_do, cond = R.apply_bwd(s, o, f, g_s, g_o)
    got_ds, got_do = ds.grad.cpu().numpy(), do.grad.cpu().numpy().reshape(-1)
    err_s = np.abs(got_ds.astype(np.float64) - w_ds) - 1e-14 * cond
    err_o = np.abs(got_do.astype(np.float64) - w_do) - 1e-14 * np.abs(w_do)
    print(f"[filter3d] n={n}: backward worst {np.max(err_s / np.spacing(np.abs(w_ds).astype(F))):.2f} / "
          f"{np.max(err_o / np.spacing(np.abs(w_do).astype(F))):.2f} places; bit-equal share "
          f"{np.mean(got_ds == w_ds.astype(F)):.5f} / {np.mean(got_do == w_do.astype(F)):.5f}")
    assert (err_s <= np.spacing(np.abs(w_ds).astype(F))).all() and (err_o <= np.spacing(np.abs(w_do).astype(F))).all()
    assert np.array_equal(got_ds[zero].view(np.uint32), g_s[zero].view(np.uint32))
    assert np.array_equal(got_do[zero].view(np.uint32), g_o.reshape(-1)[zero].view(np.uint32))
    # the getter path's activated values are the activations of the same tensors, and the definition's to float32
    with torch.no_grad():
        scale, opacity = filtered_scaling_opacity(ds, do, df)
    assert torch.equal(scale, torch.exp(se.detach())) and torch.equal(opacity, torch.sigmoid(oe.detach()))
    d_scale, d_opacity = R.apply_direct(s, o, f)
    assert np.allclose(scale.cpu().numpy(), d_scale, rtol=2e-6, atol=0)
    assert np.allclose(opacity.cpu().numpy().reshape(-1), d_opacity, rtol=2e-5, atol=1e-30)


def test_application_and_its_gradient_against_the_exact_definition_at_range(gpu_device):
    """``apply_3d_filter`` forward and backward against ``R.apply_exact`` -- the definition in 80-digit decimal arithmetic,
    none of the kernel's algebra -- on the 1023-row grid |s| <= 87, |o| <= 88, f from 1e-12 to 1e12 times the scale
    (tests/test_filter3d_host.py asserts the grid row for row), 300 rows of the narrow box and f = 0 at o in {-88, -0.0,
    88}.  The bars of the test above, now against the definition: forward at most one float32 place; backward one float32
    spacing plus 1e-14 x the magnitudes of the terms; f = 0 rows bit copies in both directions.
    Measured on an MI355X, worst per branch: o <= 0 (678 rows) forward 0 places (s') / 0 (o'), backward 0.50 of a spacing
    (dL/ds, row 617) / 0.50 (dL/do, row 1035); o > 0 (602 rows) forward 0 / 0, backward 0.50 (row 611) / 0.50 (row 922);
    f = 0 (46 rows) 0 / 0 and 0.00 / 0.00.  Every forward value is the exact value's float32; the half spacing of the
    backward is the one rounding to float32.  The host build of the header gives the same figures at the same rows."""
    from mvs_gaussian_splatting_amd import apply_3d_filter
    import types
    s, o, f, _, _ = _apply_case(300, seed=2)
    s, o, f, g_s, g_o, n_grid = R.exact_case((s, o, f))
    assert n_grid == 1023 and len(o) == 1326
    case = types.SimpleNamespace(s=s, o=o, f=f, g_s=g_s, g_o=g_o, ex=R.apply_exact(s, o, f))
    ds, do, df = (torch.from_numpy(a).to(gpu_device) for a in (s, o, f))
    ds.requires_grad_(True)
    do.requires_grad_(True)
    se, oe = apply_3d_filter(ds, do, df)
    torch.autograd.backward([se, oe], [torch.from_numpy(g_s).to(gpu_device), torch.from_numpy(g_o).to(gpu_device)])
    R.assert_exact_bars(se.detach().cpu().numpy(), oe.detach().cpu().numpy(), ds.grad.cpu().numpy(), do.grad.cpu().numpy(),
                        case, "device")


# ---- render ---------------------------------------------------------------------------------------------------------------------
def _scene(dev, P=300):
    model, cam, bg, target = small_scene(P=P, sh_degree=3, width=64, height=48, focal=60.0, scale=0.08)
    model.to(dev)
    cam.to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    return model, cam, bg.to(dev), target.to(dev)


def _frame(model, cam, bg, target, fused):
    from mvs_gaussian_splatting_amd import l1_loss, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    for p in model.parameters():
        p.grad = None
    pipe = PipelineParams()
    pipe.fuse_activations = fused
    pkg = render(cam, model, pipe, bg)
    l1_loss(pkg["render"], target).backward()
    return pkg["render"].detach().clone(), pkg["radii"].clone(), model._scaling.grad.clone(), model._opacity.grad.clone()


def test_render_with_a_filter_on_both_paths(gpu_device):
    from mvs_gaussian_splatting_amd import compute_3d_filter
    from mvs_gaussian_splatting_amd.synthetic import orbit_camera
    model, cam, bg, target = _scene(gpu_device)
    plain = {fused: _frame(model, cam, bg, target, fused) for fused in (True, False)}
    cams = [cam] + [orbit_camera(v, 8, 64, 48, 60.0, 60.0) for v in (1, 7)]
    model.filter_3D, flag = compute_3d_filter(model._xyz.detach(), cams)
    assert int(flag) == 0 and float(model.filter_3D.min()) > 0.0
    filtered = {fused: _frame(model, cam, bg, target, fused) for fused in (True, False)}
    # the two paths agree within the bar test_gpu_parity.py holds them to without a filter
    assert int((filtered[True][1] != filtered[False][1]).sum()) <= 2
    assert float((filtered[True][0] - filtered[False][0]).abs().max()) <= 2.0 / 255.0
    for fused in (True, False):
        img, radii, g_s, g_o = filtered[fused]
        assert float((img - plain[fused][0]).abs().max()) > 1e-3, "the filtered frame differs from the unfiltered one"
        assert bool(torch.isfinite(g_s).all()) and bool(torch.isfinite(g_o).all())
        assert float(g_s.abs().max()) > 0.0 and float(g_o.abs().max()) > 0.0, "gradients reach _scaling and _opacity"
    # a filter of zeros is the unfiltered frame, bit for bit, on the fused path -- gradients included
    model.filter_3D = torch.zeros_like(model.filter_3D)
    zero = _frame(model, cam, bg, target, True)
    for a, b in zip(zero, plain[True]):
        assert torch.equal(a, b)
    # the maps' glue runs with a filter too, and the planes keep their normals (the unfiltered scales decide them)
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model.filter_3D, _ = compute_3d_filter(model._xyz.detach(), cams)
    with torch.no_grad():
        pkg = render(cam, model, PipelineParams(), bg, return_depth=True, return_normals=True)
    assert bool(torch.isfinite(pkg["normal"]).all()) and float(pkg["alpha"].max()) > 0.0
    model._filter_3D_stale = True
    with pytest.raises(ValueError, match="compute_3D_filter"):
        render(cam, model, PipelineParams(), bg)


# ---- the model and the training loop ----------------------------------------------------------------------------------------------
def _trainable(dev, opt, P=300):
    from mvs_gaussian_splatting_amd import GaussianModel
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    src = small_scene(P=P, sh_degree=3, width=64, height=48, focal=60.0, scale=0.08)[0]
    m = GaussianModel(3)
    torch.manual_seed(0)
    m.create_from_pcd(src._xyz.to(dev), torch.rand(P, 3).to(dev), 1.0)
    for a in GROUP_ATTR.values():
        setattr(m, a, nn.Parameter(getattr(src, a).detach().clone().to(dev).requires_grad_(True)))
    m.active_sh_degree = 3
    m.training_setup(opt)
    return m


def test_model_filter_fuse_and_files(gpu_device, tmp_path):
    from mvs_gaussian_splatting_amd import GaussianModel, compress_model, layout, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    _, cam, bg, _ = _scene(gpu_device)
    m = _trainable(gpu_device, OptimizationParams())
    assert m.filter_3D is None
    f = m.compute_3D_filter([cam], rule="paper")
    assert f is m.filter_3D and tuple(f.shape) == (300,) and int(m.filter_3D_none_seen) == 0
    with torch.no_grad():
        want = render(cam, m, PipelineParams(), bg)["render"]
        scale, opacity = m.get_scaling_with_3D_filter, m.get_opacity_with_3D_filter
    assert tuple(scale.shape) == (300, 3) and tuple(opacity.shape) == (300, 1)
    assert (scale > m.get_scaling).all() and (opacity < m.get_opacity).all()
    # the filtered PLY round trip, and the fused PLY: a standard file that renders the same frame without a filter
    a, b = str(tmp_path / "filtered.ply"), str(tmp_path / "fused.ply")
    m.save_ply(a)
    m.save_ply(b, fuse_filter=True)
    back = GaussianModel(3)
    back.load_ply(a)
    assert torch.equal(back.filter_3D, m.filter_3D) and torch.equal(back._scaling, m._scaling)
    fused = GaussianModel(3)
    fused.load_ply(b)
    assert fused.filter_3D is None and not torch.equal(fused._scaling, m._scaling)
    with torch.no_grad():
        assert torch.equal(render(cam, back, PipelineParams(), bg)["render"], want)
        assert torch.equal(render(cam, fused, PipelineParams(), bg)["render"], want)
    with pytest.raises(ValueError, match="fuse_filter_3D_"):
        compress_model(m)
    # pruning marks it stale; recomputing clears that; fusing bakes it in place and drops it
    keep = torch.ones(300, dtype=torch.bool, device=gpu_device)
    keep[::3] = False
    layout.prune_points_(m, keep)
    with pytest.raises(ValueError, match="compute_3D_filter"):
        render(cam, m, PipelineParams(), bg)
    m.compute_3D_filter([cam], rule="paper")
    assert tuple(m.filter_3D.shape) == (200,) and not m._filter_3D_stale and bool(torch.isfinite(m.filter_3D).all())
    scaling_param = m._scaling
    with torch.no_grad():
        want = render(cam, m, PipelineParams(), bg)["render"]
    assert m.fuse_filter_3D_() is m and m.filter_3D is None and m._scaling is scaling_param
    with torch.no_grad():
        assert torch.equal(render(cam, m, PipelineParams(), bg)["render"], want)
    assert compress_model(m, codebook_size=256).num_points == 200


def test_training_iterations_across_a_densification(gpu_device):
    from mvs_gaussian_splatting_amd.rasterizer import rasterize_gaussians_fused
    from mvs_gaussian_splatting_amd.renderer import _settings, _zero_leaf, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams, orbit_camera
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    _, cam, bg, target = _scene(gpu_device)
    cams = [cam, orbit_camera(1, 8, 64, 48, 60.0, 60.0)]
    over = dict(iterations=30, position_lr_max_steps=30, densify_from_iter=1, densification_interval=2,
                densify_until_iter=10, densify_grad_threshold=1e-9)
    opt = OptimizationParams(filter_3d=True, **over)
    m = _trainable(gpu_device, opt)
    sizes, filters = [], []
    for it in (1, 2, 3):
        torch.manual_seed(it)
        loss = training_iteration(m, cam, opt, PipelineParams(), bg, it, cameras_extent=1.0, gt_image=target,
                                  filter_cameras=cams)
        assert bool(torch.isfinite(loss)) and not m._filter_3D_stale
        sizes.append(int(m._xyz.shape[0]))
        filters.append(m.filter_3D)
        assert tuple(m.filter_3D.shape) == (sizes[-1],) and float(m.filter_3D.min()) > 0.0
    print(f"[filter3d] Gaussians over three iterations: {sizes}")
    assert sizes[1] > sizes[0] and sizes[2] == sizes[1], "iteration 2 densifies"
    assert filters[1] is not filters[0] and filters[2] is filters[1], "recomputed after the densification, then kept"
    want, _ = R.compute(m._xyz.detach().cpu().numpy(), cams)
    # the optimizer steps since moved the points a little: nearly every row is close to, not equal to, a fresh filter
    assert np.mean(np.isclose(filters[2].cpu().numpy(), want, rtol=0.05)) > 0.9
    # filter_3d = False: the calls made before -- with or without cameras the same bits, and the frame the operator
    # gives for the model's own tensors
    off = OptimizationParams(**over)
    a, b = _trainable(gpu_device, off), _trainable(gpu_device, off)
    for it in (1, 2, 3):
        for model, kw in ((a, {"filter_cameras": cams}), (b, {})):
            torch.manual_seed(it)
            training_iteration(model, cam, off, PipelineParams(), bg, it, cameras_extent=1.0, gt_image=target, **kw)
    assert a.filter_3D is None and b.filter_3D is None and len(a.capture()) == 12
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    with torch.no_grad():
        pipe = PipelineParams()
        frame = render(cam, a, pipe, bg)["render"]
        visible = torch.empty(a._xyz.shape[0], dtype=torch.bool, device=gpu_device)
        parent, _ = rasterize_gaussians_fused(a._xyz, _zero_leaf(a._xyz), a._features_dc, a._features_rest, a._opacity,
                                              a._scaling, a._rotation, _settings(cam, a, pipe, bg, 1.0), visible=visible)
    assert torch.equal(frame, parent)


def _recorded(m, monkeypatch, now):
    """Wraps ``m.compute_3D_filter``: every call appends (the iteration in ``now[0]``, a clone of ``_xyz``, the filter it
    made) to the returned list."""
    calls, real = [], m.compute_3D_filter

    def compute(cameras, **kw):
        xyz = m._xyz.detach().clone()
        out = real(cameras, **kw)
        calls.append((now[0], xyz, m.filter_3D))
        return out

    monkeypatch.setattr(m, "compute_3D_filter", compute)
    return calls


def _assert_recorded_filters(calls, cams, rule="mip_splatting"):
    for it, xyz, filt in calls:
        want, flag = R.compute(xyz.cpu().numpy(), cams, rule=rule)
        assert flag == 0 and tuple(filt.shape) == (len(xyz),) and np.array_equal(bits(filt), want.view(np.uint32)), it


def test_trainer_recomputes_every_interval_once_densification_has_ended(gpu_device, monkeypatch):
    """``densify_until_iter = 2, filter_3d_interval = 2, iterations = 10``: the filter is computed at iteration 1 before
    the frame and again after that iteration's densification, then exactly at iterations 4 and 6 -- not at 2 (not yet past
    ``densify_until_iter``), not at 8 (``iteration < iterations - interval`` fails) or later.  ``filter_3D`` is a new tensor
    at exactly those iterations and the same object in between, and every computed filter is ``R.compute`` of the ``_xyz``
    of that moment, bit for bit."""
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams, orbit_camera
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    _, cam, bg, target = _scene(gpu_device)
    cams = [cam, orbit_camera(1, 8, 64, 48, 60.0, 60.0)]
    opt = OptimizationParams(filter_3d=True, filter_3d_interval=2, iterations=10, position_lr_max_steps=10,
                             densify_from_iter=0, densification_interval=1, densify_until_iter=2, densify_grad_threshold=1e-9)
    m = _trainable(gpu_device, opt)
    now = [0]
    calls = _recorded(m, monkeypatch, now)
    held, sizes = [], []
    for it in range(1, 11):
        now[0] = it
        torch.manual_seed(it)
        loss = training_iteration(m, cam, opt, PipelineParams(), bg, it, cameras_extent=1.0, gt_image=target,
                                  filter_cameras=cams)
        assert bool(torch.isfinite(loss)) and not m._filter_3D_stale
        held.append(m.filter_3D)
        sizes.append(int(m._xyz.shape[0]))
    assert [c[0] for c in calls] == [1, 1, 4, 6], [c[0] for c in calls]
    assert sizes[0] > 300 and len(set(sizes)) == 1, "iteration 1 densifies, nothing does after it"
    assert calls[0][1].shape[0] == 300 and calls[1][1].shape[0] == sizes[0] and held[0] is calls[1][2]
    changed = [it for it in range(2, 11) if held[it - 1] is not held[it - 2]]
    assert changed == [4, 6] and held[3] is calls[2][2] and held[5] is calls[3][2] and held[9] is calls[3][2]
    assert not torch.equal(calls[2][1], calls[1][1]) and not torch.equal(calls[3][1], calls[2][1]), "the points had moved"
    _assert_recorded_filters(calls, cams)


def test_trainer_recomputes_after_an_mcmc_relocation_and_growth(gpu_device, monkeypatch):
    """``strategy = "mcmc"`` with a cap of 310 on 300 rows, densifying at iterations 2 and 4.  Iteration 2 relocates 7 dead
    rows in place and appends 10: the trainer recomputes the filter right after the two steps, so it has 310 rows, is not
    stale, and iteration 3 -- whose ``render`` would refuse a stale or short filter -- draws with that very tensor.
    Iteration 4 is at the cap: relocation alone, P stays, the filter is recomputed all the same.  Every computed filter is
    ``R.compute`` of the ``_xyz`` of that moment, bit for bit."""
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams, orbit_camera
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    _, cam, bg, target = _scene(gpu_device)
    cams = [cam, orbit_camera(1, 8, 64, 48, 60.0, 60.0)]
    opt = OptimizationParams(filter_3d=True, filter_3d_rule="paper", strategy="mcmc", cap_max=310, iterations=30,
                             position_lr_max_steps=30, densify_from_iter=1, densification_interval=2, densify_until_iter=10)
    m = _trainable(gpu_device, opt)
    now = [0]
    calls = _recorded(m, monkeypatch, now)
    draws = torch.from_numpy(np.random.default_rng(5).integers(0, 2 ** 63, size=64, dtype=np.int64))
    held, sizes = [], []
    for it in range(1, 6):
        now[0] = it
        if it in (2, 4):
            with torch.no_grad():
                m._opacity[5:40:5] = -7.0                              # seven dead rows: something to relocate
        torch.manual_seed(it)
        loss = training_iteration(m, cam, opt, PipelineParams(), bg, it, cameras_extent=1.0, gt_image=target,
                                  filter_cameras=cams, mcmc_kwargs={"draws": draws})
        assert bool(torch.isfinite(loss)) and not m._filter_3D_stale
        held.append(m.filter_3D)
        sizes.append(int(m._xyz.shape[0]))
        assert tuple(m.filter_3D.shape) == (sizes[-1],)
    assert sizes == [300, 310, 310, 310, 310] and [c[0] for c in calls] == [1, 2, 4], [c[0] for c in calls]
    assert [int(c[1].shape[0]) for c in calls] == [300, 310, 310]
    assert held[1] is calls[1][2] and held[2] is held[1] and held[3] is calls[2][2] and held[3] is not held[2] and held[4] is held[3]
    for xyz, rows in ((calls[1][1], list(range(5, 40, 5)) + list(range(300, 310))), (calls[2][1], range(5, 40, 5))):
        twins = [int((xyz == xyz[i]).all(dim=1).sum()) for i in rows]
        assert min(twins) >= 2, "the filter was computed with the relocated and the new rows on their sources' positions"
    _assert_recorded_filters(calls, cams, rule="paper")
