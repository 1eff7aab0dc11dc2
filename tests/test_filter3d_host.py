"""CPU-side checks of the 3D smoothing filter (csrc/filter3d.hip, csrc/filter3d_math.h; filter3d.py): the
ABI and the refusals of the entry points and of the Python functions -- all before a GPU is asked for --, the header built
by the host compiler (tests/filter3d_host_check.cpp) against the numpy restatement (tests/filter3d_restate.py), the
boundary cases of the sampling rule, the closed forms against the definition (in float64 on a narrow box, and against the
definition in 80-digit decimal arithmetic over the range float32 parameters hold), the premises of the planted reduction
cases of tests/test_gpu_filter3d.py, and the model's side: checkpoints, PLY files, staleness, the refusals of ``render``
and ``compress_model``."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
import torch
from torch import nn

from conftest import ROOT
import filter3d_restate as R
from mvs_gaussian_splatting_amd import filter3d
from mvs_gaussian_splatting_amd.densify import GROUP_ATTR

ENTRY_POINTS = ("gsr_filter3d_workspace_bytes", "gsr_filter3d_sample", "gsr_filter3d_finish", "gsr_filter3d_apply",
                "gsr_filter3d_apply_bwd")
BAD, CAPACITY, ALIGN = -1, -2, -3
F = np.float32


# ---- ABI and refusals ----------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_abi_versions_agree():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib
    for name in ("compute_3d_filter", "apply_3d_filter", "filtered_scaling_opacity"):
        assert getattr(pkg, name) is getattr(filter3d, name) and name in pkg.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\b(int|size_t) " + name + r"\(", header), name
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("gsr_filter3d_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 47
    assert int(re.search(r"#define GSR_FILTER3D_MAX_VIEWS (\d+)", header).group(1)) == _lib.FILTER3D_MAX_VIEWS == 65535
    assert filter3d.MAX_VIEWS == filter3d.VIEW_CHUNK == 65535
    assert "GsrFilterView" in header and C.sizeof(_lib.GsrFilterView) == 80 and _lib.GsrFilterView.fx.offset == 64
    assert (_lib.FILTER3D_MIP_SPLATTING, _lib.FILTER3D_PAPER) == (0, 1) == (filter3d.RULES["mip_splatting"], filter3d.RULES["paper"])
    # one (max, min) pair per 64 rows, padded to 16 bytes, and the 16-byte result; 0 for a refused P
    ws = lib.gsr_filter3d_workspace_bytes
    assert (ws(0), ws(1), ws(64), ws(65), ws(129), ws(-1), ws(2 ** 31)) == (16, 32, 32, 32, 48, 0, 0)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    q = p + 1024
    # sample(xyz, P, views, V, near, margin, accumulate, min_depth, max_rate, seen, ws, ws_bytes, stream)
    good = [p, 10, p, 2, 0.2, 0.15, 0, q, q + 256, q + 512, q + 1024, 4096]
    nan, inf = float("nan"), float("inf")
    for n, value, code in ((0, None, BAD), (2, None, BAD), (7, None, BAD), (8, None, BAD), (9, None, BAD), (10, None, BAD),
                           (1, -1, BAD), (1, 2 ** 31, BAD), (3, -1, BAD), (3, 65536, BAD), (4, 0.0, BAD), (4, nan, BAD),
                           (4, inf, BAD), (5, -0.1, BAD), (5, nan, BAD), (5, inf, BAD), (0, p + 2, ALIGN), (7, q + 1, ALIGN),
                           (8, q + 258, ALIGN), (2, p + 4, ALIGN), (10, q + 1032, ALIGN), (11, 31, CAPACITY)):
        args = list(good)
        args[n] = value
        assert lib.gsr_filter3d_sample(*args, None) == code, (n, value)
    assert lib.gsr_filter3d_sample(None, 0, None, 0, 0.2, 0.15, 0, None, None, None, None, 0, None) == 0      # P = 0
    # finish(P, min_depth, max_rate, seen, rule, focal_max, variance, ws, ws_bytes, filter, none_seen, stream)
    good = [10, q, q + 256, q + 512, 0, 100.0, 0.2, q + 1024, 4096, p, p + 512]
    for n, value, code in ((1, None, BAD), (2, None, BAD), (3, None, BAD), (7, None, BAD), (9, None, BAD), (10, None, BAD),
                           (0, -1, BAD), (0, 2 ** 31, BAD), (4, 2, BAD), (4, -1, BAD), (5, 0.0, BAD), (5, nan, BAD),
                           (5, inf, BAD), (6, 0.0, BAD), (6, -1.0, BAD), (6, nan, BAD), (1, q + 2, ALIGN), (9, p + 1, ALIGN),
                           (10, p + 514, ALIGN), (7, q + 1028, ALIGN), (8, 16, CAPACITY)):
        args = list(good)
        args[n] = value
        assert lib.gsr_filter3d_finish(*args, None) == code, (n, value)
    assert b"rule" in (lib.gsr_filter3d_finish(*(good[:4] + [7] + good[5:]), None), lib.gsr_last_error())[1]
    # apply(scaling, opacity, filter, P, scaling_out, opacity_out, stream)
    good = [p, p + 256, p + 512, 10, q, q + 256]
    for n, value, code in ((0, None, BAD), (1, None, BAD), (2, None, BAD), (4, None, BAD), (5, None, BAD), (3, -1, BAD),
                           (3, 2 ** 31, BAD), (4, p, BAD), (5, p + 256, BAD), (0, p + 1, ALIGN), (5, q + 258, ALIGN)):
        args = list(good)
        args[n] = value
        assert lib.gsr_filter3d_apply(*args, None) == code, (n, value)
    assert lib.gsr_filter3d_apply(None, None, None, 0, None, None, None) == 0
    # apply_bwd(scaling, opacity, filter, P, g_scaling, g_opacity, d_scaling, d_opacity, stream)
    good = [p, p + 256, p + 512, 10, p + 768, p + 1024, q, q + 256]
    for n in (0, 1, 2, 4, 5, 6, 7):
        args = list(good)
        args[n] = None
        assert lib.gsr_filter3d_apply_bwd(*args, None) == BAD, n
        args[n] = good[n] + 2
        assert lib.gsr_filter3d_apply_bwd(*args, None) == ALIGN, n
    assert lib.gsr_filter3d_apply_bwd(*(good[:3] + [-1] + good[4:]), None) == BAD
    assert lib.gsr_filter3d_apply_bwd(None, None, None, 0, None, None, None, None, None) == 0


def test_python_functions_refuse_bad_arguments_and_cpu_tensors():
    from mvs_gaussian_splatting_amd import _lib, apply_3d_filter, compute_3d_filter, filtered_scaling_opacity
    xyz, cams = torch.zeros(10, 3), [R.camera(64, 48, 60.0, 60.0)]
    for bad in (xyz.double(), xyz[:, :2], xyz[0], xyz.numpy()):
        with pytest.raises(ValueError):
            compute_3d_filter(bad, cams)
    for kw in (dict(near=0.0), dict(near=float("nan")), dict(margin=-0.1), dict(variance=0.0), dict(variance=float("inf")),
               dict(rule="mip"), dict(near=True), dict(out=torch.zeros(9)), dict(out=torch.zeros(10).double())):
        with pytest.raises(ValueError):
            compute_3d_filter(xyz, cams, **kw)
    with pytest.raises(ValueError, match="at least one camera"):
        compute_3d_filter(xyz, [])
    with pytest.raises(ValueError):
        compute_3d_filter(xyz, 7)
    broken = R.camera(64, 48, 60.0, 60.0)
    broken.world_view_transform[1, 2] = float("nan")
    with pytest.raises(ValueError, match="camera 1"):
        compute_3d_filter(xyz, cams + [broken])
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        compute_3d_filter(xyz, cams)
    s, o, f = torch.zeros(10, 3), torch.zeros(10, 1), torch.zeros(10)
    for a, b, c in ((s.double(), o, f), (s[:, :2], o, f), (s, o[:9], f), (s, o, f[:9]), (s, o, torch.zeros(10, 3)),
                    (s, o, f.clone().requires_grad_(True)), (s.numpy(), o, f)):
        with pytest.raises(ValueError):
            apply_3d_filter(a, b, c)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        apply_3d_filter(s, o, f)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        filtered_scaling_opacity(s, o, f)


# ---- the rule: host build against the restatement -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """``csrc/filter3d_math.h`` built by the host compiler from ``tests/filter3d_host_check.cpp`` into a program of its
    own, with the kernel's ``-ffp-contract=off``."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    folder = tmp_path_factory.mktemp("filter3d_host")
    exe = str(folder / "filter3d_host_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "filter3d_host_check.cpp"), "-o", exe], check=True)

    def run(xyz, cams, near=0.2, margin=0.15, variance=0.2, rule="mip_splatting", rows=None):
        """-> (none_seen, dict of per-Gaussian columns)."""
        P = len(xyz)
        if rows is None:
            rows = np.zeros((P, 9), dtype=F)
            rows[:, 4] = -1.0
        focal_max = max([R.focal(c)[2] for c in cams] + [F(1.0)]) if cams else F(1.0)
        blob = struct.pack("<iiiffff", P, len(cams), R.RULES[rule], near, margin, variance, float(focal_max))
        for cam in cams:
            H, W, fx, fy = R.focal(cam)
            blob += struct.pack("<iiff", W, H, float(fx), float(fy)) + cam.world_view_transform.numpy().astype("<f4").tobytes()
        blob += np.ascontiguousarray(xyz, dtype="<f4").tobytes() + np.ascontiguousarray(rows, dtype="<f4").tobytes()
        path = str(folder / "case.bin")
        with open(path, "wb") as f:
            f.write(blob)
        lines = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
        words = np.array([[int(v, 16) for v in ln.split()] for ln in lines[1:]], dtype=np.uint32).reshape(-1, 12)
        fl = words.view(F)
        return int(lines[0]), {"min_depth": fl[:, 0], "max_rate": fl[:, 1], "seen": words[:, 2].astype(bool),
                               "filter": fl[:, 3], "s": fl[:, 4:7], "o": fl[:, 7], "ds": fl[:, 8:11], "do": fl[:, 11]}
    return run


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=F).view(np.uint32), np.asarray(b, dtype=F).view(np.uint32))


@pytest.mark.parametrize("rule", ["mip_splatting", "paper"])
@pytest.mark.parametrize("P,V", [(1, 1), (65, 2), (257, 3), (1000, 7)])
def test_host_build_of_the_sampling_rule_gives_the_restatements_bits(host_check, P, V, rule):
    xyz, cams = R.gate_scene(P, V)
    flag, got = host_check(xyz, cams, rule=rule)
    min_depth, max_rate, seen = R.sample(xyz, cams)
    want, want_flag = R.width(min_depth, max_rate, seen, cams, rule=rule)
    assert same_bits(got["min_depth"], min_depth) and same_bits(got["max_rate"], max_rate)
    assert np.array_equal(got["seen"], seen) and flag == want_flag
    assert same_bits(got["filter"], want)
    if P >= 257:
        assert 0 < seen.sum() < P, "the scene must hold seen and unseen Gaussians"
        assert np.isfinite(want).all() and (want > 0).all()
        # an unseen Gaussian takes the filter of the farthest (most coarsely sampled) seen one
        assert (want[~seen] == want[seen].max()).all()


def test_boundaries_of_the_sampling_rule(host_check):
    """Dyadic numbers, so float32 decides every gate exactly: W = 64, H = 32, fx = fy = 32, margin = 1/4, near = 1/4;
    the identity camera.  u = 32 x / z + 32 must lie in [-16, 80], w = 32 y / z + 16 in [-8, 40]."""
    cam = R.camera(64, 32, 32.0, 32.0)
    assert R.focal(cam)[2:] == (F(32.0), F(32.0))
    xyz = np.array([[0.0, 0.0, 0.25],        # z == near: does not count
                    [0.0, 0.0, 0.2500001],   # just past it: counts
                    [-1.5, 0.0, 1.0],        # u == -m W = -16: counts
                    [1.5, 0.0, 1.0],         # u == (1 + m) W = 80: counts
                    [-1.5000001, 0.0, 1.0],  # one place outside on the left
                    [1.500001, 0.0, 1.0],    # ... and on the right (80 has a coarser grid than 16)
                    [0.0, -0.75, 1.0],       # w == -m H = -8: counts
                    [0.0, 0.75, 1.0],        # w == (1 + m) H = 40: counts
                    [0.0, 0.7500001, 1.0],   # one place outside below
                    [0.0, 0.0, -3.0],        # behind the camera
                    [np.nan, 0.0, 1.0],      # a NaN counts nowhere
                    [0.0, 0.0, 8.0]], dtype=F)
    want_seen = np.array([0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1], dtype=bool)
    for rule in ("mip_splatting", "paper"):
        flag, got = host_check(xyz, [cam], near=0.25, margin=0.25, rule=rule)
        min_depth, max_rate, seen = R.sample(xyz, [cam], near=0.25, margin=0.25)
        assert np.array_equal(seen, want_seen) and np.array_equal(got["seen"], want_seen) and flag == 0
        assert same_bits(got["min_depth"], min_depth) and same_bits(got["max_rate"], max_rate)
        assert np.isinf(min_depth[~want_seen]).all() and (max_rate[~want_seen] == 0).all()
        assert min_depth[2] == 1.0 and max_rate[2] == 32.0 and min_depth[11] == 8.0 and max_rate[11] == 4.0
        want, _ = R.width(min_depth, max_rate, seen, [cam], rule=rule)
        assert same_bits(got["filter"], want)
        # a Gaussian seen by no view is filtered as the farthest seen one (z = 8: the largest depth, the smallest rate)
        sd = np.sqrt(F(0.2))
        far = (F(8.0) / F(32.0)) * sd if rule == "mip_splatting" else sd / F(4.0)
        assert (want[~want_seen] == far).all() and want[11] == far and want[2] < far
    # a table in which no Gaussian is seen: filter 0 everywhere and the flag
    behind = np.eye(4, dtype=F)
    behind[3, 2] = -100.0                                        # every point lies behind this camera
    away = R.camera(64, 32, 32.0, 32.0, behind)
    for cams in ([away], [away, away]):
        flag, got = host_check(xyz, cams, near=0.25, margin=0.25)
        assert flag == 1 and not got["seen"].any() and same_bits(got["filter"], np.zeros(len(xyz), dtype=F))
        assert R.compute(xyz, cams, near=0.25, margin=0.25)[1] == 1
    # the focal maximum is taken over ALL views, also over one that sees nothing
    tele = R.camera(64, 32, 256.0, 256.0, behind)
    flag, got = host_check(xyz, [cam, tele], near=0.25, margin=0.25)
    want, _ = R.compute(xyz, [cam, tele], near=0.25, margin=0.25)
    assert flag == 0 and same_bits(got["filter"], want) and want[2] == (F(1.0) / F(256.0)) * np.sqrt(F(0.2))


def _apply_case(n=4000, seed=0):
    """Raw scales in [-12, 4], raw opacities in [-12, 12], filters from 0 to 10 times the scale, and rows with f = 0."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-12.0, 4.0, size=(n, 3)).astype(F)
    o = rng.uniform(-12.0, 12.0, size=n).astype(F)
    f = (np.exp(s.astype(np.float64).mean(axis=1)) * rng.uniform(0.0, 10.0, size=n)).astype(F)
    f[::7] = 0.0
    g_s = rng.standard_normal((n, 3)).astype(F)
    g_o = rng.standard_normal(n).astype(F)
    return s, o, f, g_s, g_o


def test_closed_forms_are_the_definition():
    s, o, f, _, _ = _apply_case()
    s_eff, o_eff = R.apply_torch(*(torch.from_numpy(a.astype(np.float64)) for a in (s, o, f)))
    scale, opacity = R.apply_direct(s, o, f)
    assert np.allclose(np.exp(s_eff.numpy()), scale, rtol=1e-12, atol=0)
    # sigmoid(o') = sigmoid(o) c; 1 - sigmoid(o) c loses digits near 1, so compare on the logit's own terms
    assert np.allclose(1.0 / (1.0 + np.exp(-o_eff.numpy())), opacity, rtol=1e-9, atol=0)
    zero = f == 0
    se, oe = R.apply(s, o, f)
    assert zero.sum() > 100 and same_bits(se[zero], s[zero])
    assert R.ulps(oe[zero], o[zero].astype(np.float64)).max() <= 1          # the kernel's own pass-through is exact
    assert (se >= s).all() and (oe <= o).all(), "the filter only widens a Gaussian and only lowers its opacity"


def test_host_build_of_the_application_is_within_one_float32_place(host_check):
    s, o, f, g_s, g_o = _apply_case(seed=1)
    rows = np.concatenate([s, o[:, None], f[:, None], g_s, g_o[:, None]], axis=1)
    _, got = host_check(np.zeros((len(s), 3), dtype=F), [], rows=rows)
    se, oe = R.apply(s, o, f)
    print(f"[filter3d host] forward bit-equal: scaling {np.mean(got['s'].view(np.uint32) == se.view(np.uint32)):.4f}, "
          f"opacity {np.mean(got['o'].view(np.uint32) == oe.view(np.uint32)):.4f}")
    assert R.ulps(got["s"], se.astype(np.float64)).max() <= 1 and R.ulps(got["o"], oe.astype(np.float64)).max() <= 1
    zero = f == 0
    assert same_bits(got["s"][zero], s[zero]) and same_bits(got["o"][zero], o[zero]), "f = 0 returns s and o bit for bit"
    assert same_bits(got["ds"][zero], g_s[zero]) and same_bits(got["do"][zero], g_o[zero])
    d_s, d_o, cond = R.apply_bwd(s, o, f, g_s, g_o)
    # one float32 place, plus what 64 places of float64 rounding can move a sum of two terms of this size
    assert (np.abs(got["do"].astype(np.float64) - d_o) <= np.spacing(np.abs(d_o).astype(F)) + 1e-14 * np.abs(d_o)).all()
    assert (np.abs(got["ds"].astype(np.float64) - d_s) <= np.spacing(np.abs(d_s).astype(F)) + 1e-14 * cond).all()


# ---- the application against the definition itself, at range ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact():
    """The rows of ``R.exact_case`` and ``R.apply_exact`` of them, computed once and left unchanged."""
    s, o, f, _, _ = _apply_case(300, seed=2)
    s, o, f, g_s, g_o, n_grid = R.exact_case((s, o, f))
    return types.SimpleNamespace(s=s, o=o, f=f, g_s=g_s, g_o=g_o, n_grid=n_grid, ex=R.apply_exact(s, o, f))


def test_the_exact_grid_drops_six_scale_ratio_pairs_and_nothing_else():
    """``f = float32(e^s0 ratio)``: e^87 = 6.1e37 overflows from ratio 100 on (float32 ends at 3.4e38), e^-87 = 1.6e-38
    falls below half the smallest denormal (7e-46) from ratio 1e-8 down; e^-87 x 1e-4 = 1.6e-42 is a denormal and stays."""
    s, o, f, dropped = R.exact_grid()
    assert dropped == {(-87.0, 1e-12), (-87.0, 1e-8), (87.0, 1e2), (87.0, 1e4), (87.0, 1e8), (87.0, 1e12)}
    assert len(o) == 1023 == 11 * (99 - 6) and s.dtype == o.dtype == f.dtype == F
    assert np.isfinite(f).all() and (f > 0).all() and f.min() < 2.0 ** -126 and np.abs(s).max() < 88.4
    # every (s0, o, ratio) that stays is there once, in the grid's order
    want = [(s0, o_, F(math.exp(s0) * ratio)) for s0 in R.GRID_S0 for ratio in R.GRID_RATIO if (s0, ratio) not in dropped
            for o_ in R.GRID_O]
    assert [(float(a), float(b), c) for a, b, c in zip(s[:, 0], o, f)] == [(float(F(a)), float(F(b)), c) for a, b, c in want]
    assert same_bits(s[:, 1], (s[:, 0].astype(np.float64) + 0.7).astype(F)) and \
        same_bits(s[:, 2], (s[:, 0].astype(np.float64) - 1.3).astype(F))


def test_the_exact_reference_is_the_definition_and_its_derivatives():
    """``apply_exact`` against itself: its activations are the definition's, and its three derivative factors are central
    differences of its own ``s'`` and ``o'`` in ``decimal`` (h = 1e-25 at 80 digits: a truncation error of h^2) -- so a
    sign or a factor written down wrongly there cannot pass."""
    import decimal as dec
    rows = [((-87.0, -86.3, -88.3), -88.0, 1.6e-42), ((0.0, 0.7, -1.3), 1.0, 100.0), ((5.0, 5.7, 3.7), 88.0, 1.5e-6),
            ((-3.0, -2.3, -4.3), -1e-3, 0.05), ((87.0, 87.7, 85.7), 40.0, 6.0e25), ((-20.0, -19.3, -21.3), 17.0, 2.0e3)]
    s = np.array([r[0] for r in rows], dtype=F)
    o, f = np.array([r[1] for r in rows], dtype=F), np.array([r[2] for r in rows], dtype=F)
    ex = R.apply_exact(s, o, f)

    def value(sd, od, f2):
        af, p, c, omx = R._filtered(dec, sd, od, f2)
        return [y.ln() / 2 for y in af], (p * c / omx).ln()

    with dec.localcontext() as ctx:
        ctx.prec = R.EXACT_DIGITS
        h = dec.Decimal("1e-25")
        for i in range(len(rows)):
            sd, od, f2 = [dec.Decimal(float(v)) for v in s[i]], dec.Decimal(float(o[i])), dec.Decimal(float(f[i])) ** 2
            so, oo = value(sd, od, f2)
            assert [float(v) for v in so] == list(ex.s[i]) and float(oo) == ex.o[i]
            assert np.allclose(np.exp(ex.s[i]), np.sqrt(np.exp(2.0 * s[i].astype(np.float64)) + float(f[i]) ** 2), rtol=1e-13)
            d_o = (value(sd, od + h, f2)[1] - value(sd, od - h, f2)[1]) / (2 * h)
            assert abs(float(d_o) / ex.do_do[i] - 1.0) < 1e-15, (i, "do'/do")
            for j in range(3):
                up, down = list(sd), list(sd)
                up[j], down[j] = sd[j] + h, sd[j] - h
                (su, ou), (sl, ol) = value(up, od, f2), value(down, od, f2)
                assert abs(float((su[j] - sl[j]) / (2 * h)) / ex.ds_ds[i, j] - 1.0) < 1e-15, (i, j, "ds'/ds")
                assert abs(float((ou - ol) / (2 * h)) / ex.do_ds[i, j] - 1.0) < 1e-15, (i, j, "do'/ds")
    assert (ex.do_ds > 0).all() and (ex.ds_ds > 0).all() and (ex.do_do > 0).all()


def test_closed_forms_against_the_exact_definition_at_range(exact):
    """``R.apply_torch`` / ``R.apply_bwd`` (float64, the header's algebra written a second time) against ``apply_exact``
    over |s| <= 87, |o| <= 88 and f from 1e-12 to 1e12 times the scale: every branch of ``o'`` and of the backward.
    Measured: the float64 closed form is within 1.4e-13 relative of the exact ``o'`` and 1.6e-15 of ``s'`` on the grid
    (8.4e-15 with the random rows, where ``s'`` passes near 0); rounded once it is the exact value's float32 in every row
    (0 places), and the backward stays inside the 1e-14 allowance (0.00 spacings over it)."""
    assert exact.n_grid == 1023 and len(exact.o) == 1023 + 300 + 3
    se, oe = R.apply(exact.s, exact.o, exact.f)
    d_s, d_o, cond = R.apply_bwd(exact.s, exact.o, exact.f, exact.g_s, exact.g_o)
    s64, o64 = (t.numpy() for t in R.apply_torch(*(torch.from_numpy(a.astype(np.float64)) for a in (exact.s, exact.o, exact.f))))
    moved = exact.f != 0
    rel_s = np.max(np.abs(s64[moved] / exact.ex.s[moved] - 1.0))
    rel_o = np.max(np.abs(o64[moved] / exact.ex.o[moved] - 1.0))
    print(f"[filter3d exact] float64 closed form: s' within {rel_s:.1e} relative, o' within {rel_o:.1e}")
    assert rel_s < 1e-14 and rel_o < 1e-12
    R.assert_exact_bars(se, oe, d_s, d_o, exact, "float64 closed form")
    assert np.allclose(cond, R.exact_bwd(exact.ex, exact.g_s, exact.g_o)[2], rtol=1e-12, atol=0)


def test_host_build_of_the_application_against_the_exact_definition(host_check, exact):
    """csrc/filter3d_math.h itself, built by the host compiler, on the same rows against ``apply_exact``.  Measured: forward
    0 places in every branch; backward at most 0.50 of a spacing (the one rounding to float32)."""
    rows = np.concatenate([exact.s, exact.o[:, None], exact.f[:, None], exact.g_s, exact.g_o[:, None]], axis=1)
    _, got = host_check(np.zeros((len(rows), 3), dtype=F), [], rows=rows)
    R.assert_exact_bars(got["s"], got["o"], got["ds"], got["do"], exact, "host build")


# ---- the global reduction: the premise of every planted case (tests/test_gpu_filter3d.py runs them) -----------------------------
def test_planted_cases_reach_the_reduce_lanes_waves_and_trips_they_claim():
    """csrc/filter3d.hip: ``filter3d_sample_kernel`` writes the pair of rows 64 k .. 64 k + 63 to slot k;
    ``filter3d_reduce_kernel`` is one workgroup of F3D_REDUCE_BLOCK lanes whose lane t folds pairs t, t + block, ...
    (trip = pair / block), whose waves of 64 fold their lanes, and whose lane 0 folds waves 1 .. block / 64 - 1 in.  Read
    from the source, so that a change of the block size cannot hollow the cases out unnoticed."""
    with open(os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "filter3d.hip")) as f:
        src = f.read()
    block = int(re.search(r"constexpr int F3D_REDUCE_BLOCK = (\d+);", src).group(1))
    assert int(re.search(r"constexpr int F3D_BLOCK = (\d+);", src).group(1)) % R.WAVE == 0, "a wave's first row: 64 k"
    assert "k += F3D_REDUCE_BLOCK" in src and "for (int w = 1; w < F3D_REDUCE_BLOCK / WAVE; ++w)" in src
    assert "dim3(1), dim3(F3D_REDUCE_BLOCK)" in src
    reach = {k: (k % block, k % block // R.WAVE, k // block) for k in R.PLANT_PAIRS}             # lane, wave, trip
    assert reach == {0: (0, 0, 0), 15: (15, 0, 0), 16: (16, 0, 0), 63: (63, 0, 0), 64: (64, 1, 0), 1023: (1023, 15, 0),
                     1024: (0, 0, 1), 1087: (63, 0, 1), 2047: (1023, 15, 1), 2048: (0, 0, 2)}
    assert R.PLANT_SIZES == (4097, 65536, 65537, 131073)
    last = {P: R.plant_pairs(P)[-1] for P in R.PLANT_SIZES}
    assert last == {4097: 64, 65536: 1023, 65537: 1024, 131073: 2048}
    # 4097: reduce wave 1 holds data; 65536: every lane one pair, one trip; 65537: lane 0 alone a second; 131073: a third
    assert {P: (last[P] % block // R.WAVE, last[P] // block + 1, P - R.WAVE * last[P]) for P in R.PLANT_SIZES} == \
        {4097: (1, 1, 1), 65536: (15, 1, 64), 65537: (0, 2, 1), 131073: (0, 3, 1)}
    assert [len(R.plant_pairs(P)) for P in R.PLANT_SIZES] == [5, 6, 7, 10]
    for P in R.PLANT_SIZES:
        rows = [R.plant_row(P, k) for k in R.plant_pairs(P)]
        assert all(0 <= i < P and i // R.WAVE == k for i, k in zip(rows, R.plant_pairs(P)))
        assert {i % R.WAVE for i in rows} == {0, 15, 16, 63}, "k % 64: a lane that differs between neighbours in the list"
        for name, d, r, hit in R.planted_cases(P):
            m = re.fullmatch(r"D in pair (\d+), R in pair (\d+)", name)
            if m:
                kd, kr = int(m.group(1)), int(m.group(2))
                assert kd != kr and d[R.plant_row(P, kd)] == 9.0 and r[R.plant_row(P, kr)] == 0.5
                seen = hit.astype(bool)
                assert d[seen].max() == 9.0 and r[seen].min() == 0.5 and (d[seen] == 9.0).sum() == (r[seen] == 0.5).sum() == 1
                assert 0.1 < 1.0 - seen.mean() < 0.2
    pairs = {(kd // block, kr // block) for P in R.PLANT_SIZES for kd, kr in
             (map(int, re.findall(r"\d+", n)) for n, *_ in R.planted_cases(P) if n.startswith("D in"))}
    assert {(0, 1), (1, 0), (1, 2), (2, 1)} <= pairs, "D in one trip while R sits in another"


def test_a_model_of_the_reduction_tells_the_planted_cases_from_a_broken_combine_or_stride():
    """The planted cases through a host model of the reduce kernel's data flow: the kernel's own parameters give D, R and
    the flag of the definition in every case; a serial combine that starts at wave 2, or a strided loop that steps by
    2048, is told apart by at least one case (the broken kernels themselves are never run)."""
    broken = {"combine from w = 2": dict(first_wave=2), "stride 2048": dict(step=2048)}
    caught = {name: [] for name in broken}
    for P in R.PLANT_SIZES:
        for name, d, r, hit in R.planted_cases(P):
            seen = hit.astype(bool)
            pairs = R.wave_pairs(d, r, hit)
            want = (d[seen].max(), r[seen].min(), 0)
            assert R.reduce_model(pairs) == want, (P, name)
            for what, kw in broken.items():
                if R.reduce_model(pairs, **kw) != want:
                    caught[what].append((P, name))
    print({k: len(v) for k, v in caught.items()})
    assert (4097, "one seen row, pair 64") in caught["combine from w = 2"]
    assert (65537, "one seen row, pair 1024") in caught["stride 2048"]
    assert all(len(v) >= 4 for v in caught.values())
    d, r, hit = R._unseen(65537)
    assert R.reduce_model(R.wave_pairs(d, r, hit)) == (F(-np.inf), F(np.inf), 1)


# ---- the model: checkpoints, PLY files, staleness --------------------------------------------------------------------------------
def cpu_model(P=30, degree=1, seed=0, with_filter=False):
    from mvs_gaussian_splatting_amd import GaussianModel
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    g = torch.Generator().manual_seed(seed)
    k = (degree + 1) ** 2 - 1
    m = GaussianModel(degree)
    shapes = {"_xyz": (P, 3), "_features_dc": (P, 1, 3), "_features_rest": (P, k, 3), "_opacity": (P, 1), "_scaling": (P, 3),
              "_rotation": (P, 4)}
    for a, shape in shapes.items():
        setattr(m, a, nn.Parameter(torch.randn(*shape, generator=g).requires_grad_(True)))
    m.max_radii2D = torch.zeros(P)
    m.training_setup(OptimizationParams(), torch.optim.Adam)
    for a in GROUP_ATTR.values():
        p = getattr(m, a)
        m.optimizer.state[p] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(p.shape, generator=g),
                                "exp_avg_sq": torch.rand(p.shape, generator=g)}
    if with_filter:
        m.filter_3D = torch.rand(P, generator=g) * 0.1
    return m


def test_a_new_model_has_no_filter_and_its_getters_say_so():
    m = cpu_model()
    assert m.filter_3D is None and m.checked_filter_3D() is None and m.fuse_filter_3D_() is m
    for name in ("get_scaling_with_3D_filter", "get_opacity_with_3D_filter"):
        with pytest.raises(ValueError, match="compute_3D_filter"):
            getattr(m, name)
    from mvs_gaussian_splatting_amd import _lib
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        m.compute_3D_filter([R.camera(64, 48, 60.0, 60.0)])


def test_capture_and_restore_with_and_without_a_filter():
    from mvs_gaussian_splatting_amd import GaussianModel
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    opt = OptimizationParams()
    plain = cpu_model()
    cap = plain.capture()
    assert len(cap) == 12 and not any(isinstance(v, dict) and "filter_3D" in v for v in cap)
    m = cpu_model(with_filter=True)
    cap_f = m.capture()
    assert len(cap_f) == 13 and set(cap_f[-1]) == {"filter_3D", "filter_3D_stale"} and cap_f[-1]["filter_3D"] is m.filter_3D
    assert all(a is b for a, b in zip(cap_f[:10], (m.active_sh_degree, m._xyz, m._features_dc, m._features_rest, m._scaling,
                                                   m._rotation, m._opacity, m.max_radii2D, m.xyz_gradient_accum, m.denom)))
    back = GaussianModel(1)
    back.restore(cap_f, opt, torch.optim.Adam)
    assert back.filter_3D is m.filter_3D and not back._filter_3D_stale and back._xyz is m._xyz
    assert torch.equal(back.optimizer.state[back._opacity]["exp_avg"], m.optimizer.state[m._opacity]["exp_avg"])
    back.restore(cap, opt, torch.optim.Adam)                     # the old form: a model without a filter
    assert back.filter_3D is None and back._xyz is plain._xyz
    # behind the absolute-gradient accumulator's dict, which stays recognisable
    m.xyz_gradient_accum_abs = torch.zeros(30, 1)
    cap_both = m.capture()
    assert len(cap_both) == 14 and set(cap_both[-2]) == {"xyz_gradient_accum_abs"} and "filter_3D" in cap_both[-1]
    again = GaussianModel(1)
    again.restore(cap_both, opt, torch.optim.Adam)
    assert again.filter_3D is m.filter_3D and again.xyz_gradient_accum_abs is m.xyz_gradient_accum_abs
    m._filter_3D_stale = True                                    # a stale filter stays stale through a checkpoint
    again.restore(m.capture(), opt, torch.optim.Adam)
    assert again._filter_3D_stale


def _standard_ply_bytes(m):
    """The file ``save_ply`` writes for a model without a filter, built here from the documented layout."""
    P = m._xyz.shape[0]
    cols = [m._xyz, torch.zeros(P, 3), m._features_dc.transpose(1, 2).flatten(1), m._features_rest.transpose(1, 2).flatten(1),
            m._opacity, m._scaling, m._rotation]
    data = torch.cat([c.detach() for c in cols], dim=1).numpy().astype("<f4")
    n_rest = m._features_rest.shape[1] * 3
    names = ["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(n_rest)] + \
        ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {P}"] + [f"property float {n}" for n in names] + \
        ["end_header"]
    return ("\n".join(header) + "\n").encode("ascii") + data.tobytes()


def test_ply_round_trips_with_and_without_a_filter(tmp_path):
    from mvs_gaussian_splatting_amd import _lib, ply_io
    plain, m = cpu_model(seed=4), cpu_model(seed=4, with_filter=True)
    a, b, c = (str(tmp_path / n) for n in ("plain.ply", "direct.ply", "filtered.ply"))
    plain.save_ply(a)
    ply_io.save_ply(plain, b)
    want = _standard_ply_bytes(plain)
    assert open(a, "rb").read() == open(b, "rb").read() == want, "the payload of a model without a filter must not move"
    m.save_ply(c)
    got = open(c, "rb").read()
    head, _, body = got.partition(b"end_header\n")
    wh, _, wb = want.partition(b"end_header\n")
    assert head == wh + b"property float filter_3D\n" and b"filter_3D" not in want
    rows = np.frombuffer(body, dtype="<f4").reshape(30, -1)
    assert np.array_equal(rows[:, :-1], np.frombuffer(wb, dtype="<f4").reshape(30, -1)) and \
        np.array_equal(rows[:, -1], m.filter_3D.numpy())
    std, ext = ply_io.load_ply(a, 1), ply_io.load_ply(c, 1)
    assert "filter_3D" not in std and list(ext)[:-1] == list(std) and list(ext)[-1] == "filter_3D"
    assert torch.equal(ext["filter_3D"], m.filter_3D) and ext["filter_3D"].shape == (30,)
    for k in std:
        assert k == "active_sh_degree" or torch.equal(std[k], ext[k]), k
    with pytest.raises(ValueError, match="filter_3D has 29"):
        ply_io.save_ply(m, c, filter_3D=m.filter_3D[:29])
    with pytest.raises(_lib.GsrError, match="no CPU path"):      # the fused file needs the kernel
        m.save_ply(c, fuse_filter=True)
    plain.save_ply(b, fuse_filter=True)                          # ... and without a filter it is the standard file
    assert open(b, "rb").read() == want
    m._filter_3D_stale = True
    with pytest.raises(ValueError, match="compute_3D_filter"):
        m.save_ply(c)


def test_every_row_operation_marks_the_filter_stale_and_render_refuses_it():
    from mvs_gaussian_splatting_amd import layout, render
    from mvs_gaussian_splatting_amd.densify import mark_filter_stale, swap_rows_
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cam = types.SimpleNamespace()                                # never read: the refusal comes first
    for op in ("prune", "reorder", "swap"):
        m = cpu_model(with_filter=True)
        assert m.checked_filter_3D() is m.filter_3D
        if op == "prune":
            keep = torch.ones(30, dtype=torch.bool)
            keep[3] = False
            assert layout.prune_points_(m, keep) == 29
        elif op == "reorder":
            layout.reorder_gaussians_(m)                         # the Morton reorder: P stays, the rows move
        else:
            new = {k: torch.cat([getattr(m, a).detach(), getattr(m, a).detach()[:2]]) for k, a in GROUP_ATTR.items()}
            swap_rows_(m, GROUP_ATTR, new, lambda t: torch.cat([t, torch.zeros_like(t[:2])]))      # every row plan ends here
        assert m._filter_3D_stale and m.filter_3D is not None, op
        with pytest.raises(ValueError, match="compute_3D_filter"):
            render(cam, m, PipelineParams(), torch.zeros(3))
        with pytest.raises(ValueError, match="stale"):
            m.get_scaling_with_3D_filter
        with pytest.raises(ValueError, match="stale"):
            m.fuse_filter_3D_()
    # a filter of the wrong size is refused in the same words, stale or not
    m = cpu_model(with_filter=True)
    m.filter_3D = m.filter_3D[:29]
    with pytest.raises(ValueError, match="compute_3D_filter"):
        render(cam, m, PipelineParams(), torch.zeros(3))
    m.filter_3D = torch.zeros(30, 1)
    with pytest.raises(ValueError, match="compute_3D_filter"):
        render(cam, m, PipelineParams(), torch.zeros(3))
    # a model without a filter is left exactly as it is: no flag appears
    plain = cpu_model()
    layout.reorder_gaussians_(plain)
    mark_filter_stale(plain)
    assert plain.filter_3D is None and not plain._filter_3D_stale
    # MCMC's relocation and growth go through the same two hooks
    import inspect
    from mvs_gaussian_splatting_amd import mcmc
    assert "mark_filter_stale(model)" in inspect.getsource(mcmc.relocate_gs)
    assert "swap_rows_(model" in inspect.getsource(mcmc.add_new_gs)


def test_compress_model_refuses_a_model_that_still_has_a_filter():
    from mvs_gaussian_splatting_amd import compress_model
    m = cpu_model(with_filter=True)
    with pytest.raises(ValueError, match="fuse_filter_3D_"):
        compress_model(m)
    d = {a: getattr(m, a).detach() for a in GROUP_ATTR.values()}
    d.update(active_sh_degree=1, filter_3D=m.filter_3D)
    with pytest.raises(ValueError, match="fuse_filter_3D_"):
        compress_model(d)


def test_trainer_options_and_their_refusals():
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    opt = OptimizationParams()
    assert (opt.filter_3d, opt.filter_3d_interval, opt.filter_3d_rule, opt.filter_3d_variance) == (False, 100, "mip_splatting", 0.2)
    m, cam = cpu_model(), types.SimpleNamespace()
    call = lambda o, **kw: training_iteration(m, cam, o, PipelineParams(), torch.zeros(3), 1, cameras_extent=1.0, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="filter_cameras"):
        call(OptimizationParams(filter_3d=True))
    with pytest.raises(ValueError, match="filter_3d_rule"):
        call(OptimizationParams(filter_3d=True, filter_3d_rule="mip"), filter_cameras=[cam])
    with pytest.raises(ValueError, match="filter_3d_interval"):
        call(OptimizationParams(filter_3d=True, filter_3d_interval=0), filter_cameras=[cam])
    with pytest.raises(ValueError, match="grow / learned-split"):
        call(OptimizationParams(filter_3d=True), filter_cameras=[cam], dataset=types.SimpleNamespace(grow_dir=True))
