"""Per-image bilateral grids without a GPU: the float64 restatement against central differences, the
kernels' arithmetic (csrc/bilagrid_math.h) built for the host and held to the GPU test's bar on the GPU test's inputs,
the identity properties, every refusal of the wrappers, of ``BilateralGrids`` and of the four C entry points, the ABI,
the trainer's switch, the census of the fragile pixels of the inputs tests/test_gpu_bilagrid.py runs on, and that the
cases at the limits of the accepted shapes reach the lanes, row shares, blocks and passes they are there for."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess

import pytest
import torch

from conftest import ROOT
import bilagrid_restate as R
from mvs_gaussian_splatting_amd import BilateralGrids, bilateral_grid_tv_loss, slice_bilateral_grid

F64 = torch.float64
CSRC = os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc")


def test_restated_float64_gradients_agree_with_central_finite_differences():
    H, W, shape = 7, 5, (3, 5, 4)
    x, grid, up = R.make_image(H, W).to(F64), R.make_grid(shape).to(F64), R.make_upstream(H, W).to(F64)
    firm = ~R.fragile(x, shape[2])
    assert int(firm.sum()) >= H * W - 1
    _, dx, dg = R.slice_with_grads(x, grid, up)
    loss = lambda xx, gg: float((R.slice_grid(xx, gg) * up).sum())      # noqa: E731
    eps = 1e-6
    fd_x = torch.zeros_like(x)
    for i in range(x.numel()):
        hi, lo = x.clone().view(-1), x.clone().view(-1)
        hi[i] += eps
        lo[i] -= eps
        fd_x.view(-1)[i] = (loss(hi.view_as(x), grid) - loss(lo.view_as(x), grid)) / (2 * eps)
    fd_g = torch.zeros_like(grid)
    for i in range(grid.numel()):
        hi, lo = grid.clone().view(-1), grid.clone().view(-1)
        hi[i] += eps
        lo[i] -= eps
        fd_g.view(-1)[i] = (loss(x, hi.view_as(grid)) - loss(x, lo.view_as(grid))) / (2 * eps)
    assert R.rel_err(dx[:, firm], fd_x[:, firm]) < 1e-6 and R.rel_err(dg, fd_g) < 1e-6
    assert float(dx.abs().max()) > 0 and float(dg.abs().max()) > 0
    tvg = R.make_grids(2, shape).to(F64)
    _, dtv = R.tv_with_grad(tvg)
    fd_tv = torch.zeros_like(tvg)
    for i in range(tvg.numel()):
        hi, lo = tvg.clone().view(-1), tvg.clone().view(-1)
        hi[i] += eps
        lo[i] -= eps
        fd_tv.view(-1)[i] = (float(R.tv(hi.view_as(tvg))) - float(R.tv(lo.view_as(tvg)))) / (2 * eps)
    assert R.rel_err(dtv, fd_tv) < 1e-6


def _cxx():
    return os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _build(out, *flags):
    subprocess.run([_cxx(), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", *flags, "-I" + CSRC,
                    os.path.join(ROOT, "tests", "bilagrid_host_check.cpp"), "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """``csrc/bilagrid_math.h`` -- the arithmetic the kernels run -- built by the host compiler into the stand-alone
    program ``tests/bilagrid_host_check.cpp`` with the kernels' ``-ffp-contract=off``."""
    return _build(str(tmp_path_factory.mktemp("bilagrid_host") / "bilagrid_host_check"))


def _run_host(program, workdir, x, grid, up, env=None):
    H, W = x.shape[1:]
    L, Hg, Wg = grid.shape[1:]
    src, dst = os.path.join(str(workdir), "in.bin"), os.path.join(str(workdir), "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<5i", H, W, Wg, Hg, L))
        for t in (x, grid, up):
            f.write(t.contiguous().numpy().astype("<f4").tobytes())
    done = subprocess.run([program, src, dst], env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(dst, "rb") as f:
        raw = torch.frombuffer(bytearray(f.read()), dtype=torch.float32)
    n = 3 * H * W
    assert raw.numel() == 2 * n + grid.numel()
    return raw[:n].view(3, H, W), raw[n:2 * n].view(3, H, W), raw[2 * n:].view_as(grid)


def test_the_kernels_arithmetic_built_for_the_host_meets_the_gpu_tests_bar(host_program, tmp_path):
    for H, W in R.IMAGE_SHAPES:
        for shape in R.GRID_SHAPES:
            x, grid, up = R.make_image(H, W), R.make_grid(shape), R.make_upstream(H, W)
            got = _run_host(host_program, tmp_path, x, grid, up)
            R.check_slice(got, x, grid, up, f"{H}x{W} grid {shape}")
            assert all(bool(torch.isfinite(t).all()) for t in got)


def test_the_host_program_is_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    program = _build(str(tmp_path / "bilagrid_host_check_san"), "-g", "-fsanitize=address,undefined",
                     "-fno-sanitize-recover=all")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    for (H, W), shape in (((1, 1), (2, 2, 2)), ((70, 37), (16, 16, 8))):
        x, grid, up = R.make_image(H, W), R.make_grid(shape), R.make_upstream(H, W)
        y, _, _ = _run_host(program, tmp_path, x, grid, up, env=env)
        assert bool(torch.isfinite(y).all())


def test_identity_and_constant_grids_on_the_host_build(host_program, tmp_path):
    H, W, shape = 7, 5, (3, 5, 4)
    x, up = R.make_image(H, W), R.make_upstream(H, W)
    y, dx, dg = _run_host(host_program, tmp_path, x, R.identity_grid(shape), up)
    assert torch.equal(y, x), "the identity grid returns the image bit for bit"
    assert torch.equal(dx, up), "the identity grid passes the gradient through bit for bit"
    # dG does not read the grid: of a constant grid it is the float64 sums, rounded once
    ref = R.slice_with_grads(x, R.identity_grid(shape), up)[2]
    assert torch.equal(dg, ref.to(torch.float32))
    const = torch.full((12, shape[2], shape[1], shape[0]), 0.0)
    values = torch.tensor([0.3, -1.7, 0.01, 2.5, 1e-3, 0.7, -0.2, 0.9, 1.1, -0.6, 0.4, 0.05])
    const += values.reshape(12, 1, 1, 1)
    y, dx, _ = _run_host(host_program, tmp_path, x, const, up)
    A = values.double().reshape(3, 4)
    xd = x.double()
    want = torch.stack([((A[c, 0] * xd[0] + A[c, 1] * xd[1]) + A[c, 2] * xd[2]) + A[c, 3] for c in range(3)])
    assert torch.equal(y, want.to(torch.float32)), "a constant grid is its cell's affine, rounded once"
    ud = up.double()
    want = torch.stack([(A[0, k] * ud[0] + A[1, k] * ud[1]) + A[2, k] * ud[2] for k in range(3)])
    assert torch.equal(dx, want.to(torch.float32)), "no slope in z: the luminance path adds an exact zero"


def test_census_of_the_gpu_test_inputs():
    for H, W in R.IMAGE_SHAPES:
        for L in sorted({s[2] for s in R.GRID_SHAPES}):
            n, pixels, cap = R.census(R.make_image(H, W), L)
            print(f"census {H}x{W} L={L}: {n} fragile of {pixels} (cap {cap})")
            assert n <= cap


def test_every_python_refusal_comes_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib
    x, g = torch.zeros(3, 4, 5), torch.zeros(12, 4, 3, 2)
    with pytest.raises(TypeError, match="torch.Tensor"):
        slice_bilateral_grid([1.0], g)
    with pytest.raises(TypeError, match="torch.Tensor"):
        slice_bilateral_grid(x, None)
    with pytest.raises(TypeError, match="float32"):
        slice_bilateral_grid(x.double(), g)
    with pytest.raises(TypeError, match="float32"):
        slice_bilateral_grid(x, g.half())
    for bad in (torch.zeros(4, 5), torch.zeros(1, 4, 5), torch.zeros(3, 0, 5), torch.zeros(1, 3, 4, 5)):
        with pytest.raises(ValueError):
            slice_bilateral_grid(bad, g)
    for bad in (torch.zeros(12, 3, 2), torch.zeros(9, 4, 3, 2), torch.zeros(12, 1, 3, 2), torch.zeros(12, 17, 3, 2),
                torch.zeros(12, 4, 65, 2), torch.zeros(12, 4, 3, 1), torch.zeros(1, 12, 4, 3, 2)):
        with pytest.raises(ValueError):
            slice_bilateral_grid(x, bad)
    with pytest.raises(ValueError, match="is on"):
        slice_bilateral_grid(x, g.to("meta"))
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        slice_bilateral_grid(x, g)
    with pytest.raises(TypeError):
        bilateral_grid_tv_loss([g])
    with pytest.raises(TypeError, match="float32"):
        bilateral_grid_tv_loss(g[None].double())
    for bad in (g, torch.zeros(0, 12, 4, 3, 2), torch.zeros(1, 11, 4, 3, 2), torch.zeros(1, 12, 1, 3, 2),
                torch.zeros(1, 12, 4, 3, 65), torch.zeros(1, 12, 17, 3, 2)):
        with pytest.raises(ValueError):
            bilateral_grid_tv_loss(bad)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        bilateral_grid_tv_loss(g[None])


def test_bilateral_grids_object_on_the_host(tmp_path):
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    for names in ([], ["a", "a"]):
        with pytest.raises(ValueError):
            BilateralGrids(names, device="cpu")
    for shape in ((1, 16, 8), (16, 65, 8), (16, 16, 17), (16, 16), "abc", None):
        with pytest.raises(ValueError):
            BilateralGrids(["a"], shape=shape, device="cpu")
    grids = BilateralGrids(["a", "b", "c"], shape=(3, 5, 4), device="cpu")
    assert grids.shape == (3, 5, 4) and tuple(grids.grids.shape) == (3, 12, 4, 5, 3) and grids.grids.requires_grad
    assert torch.equal(grids.grids.detach()[1], R.identity_grid((3, 5, 4)))
    assert tuple(BilateralGrids(["a"], device="cpu").grids.shape) == (1, 12, 8, 16, 16)
    row = grids.grid_for("b")
    assert row.shape == (12, 4, 5, 3) and row.data_ptr() == grids.grids[1].data_ptr()
    with pytest.raises(KeyError, match="no bilateral grid"):
        grids.grid_for("d")
    with pytest.raises(ValueError, match="training_setup"):
        grids.update_learning_rate(1)
    opt = OptimizationParams(iterations=100)
    assert (opt.bilateral_grid_lr_init, opt.bilateral_grid_lr_final, opt.lambda_tv) == (2e-3, 2e-5, 10.0)
    optimizer = grids.training_setup(opt)
    assert optimizer is grids.optimizer and optimizer.param_groups[0]["eps"] == 1e-15
    assert optimizer.param_groups[0]["params"][0] is grids.grids
    assert grids.update_learning_rate(0) == pytest.approx(2e-3) and optimizer.param_groups[0]["lr"] == pytest.approx(2e-3)
    assert grids.update_learning_rate(100) == pytest.approx(2e-5)
    assert 2e-5 < grids.update_learning_rate(50) < 2e-3
    # files: the parameter travels exactly; a state for other images, another shape or without a set-up is refused
    with torch.no_grad():
        grids.grids.add_(torch.randn(grids.grids.shape, generator=torch.Generator().manual_seed(5)))
    path = str(tmp_path / "bilateral_grid_7.pt")
    grids.save(path)
    other = BilateralGrids(["a", "b", "c"], shape=(3, 5, 4), device="cpu")
    with pytest.raises(ValueError, match="training_setup"):
        other.load(path)
    other.training_setup(opt)
    other.load(path)
    assert torch.equal(other.grids.detach(), grids.grids.detach())
    for wrong in (BilateralGrids(["a", "b", "x"], shape=(3, 5, 4), device="cpu"),
                  BilateralGrids(["a", "b", "c"], shape=(3, 5, 5), device="cpu")):
        wrong.training_setup(opt)
        with pytest.raises(ValueError, match="other images"):
            wrong.load(path)
    with pytest.raises(ValueError, match="has no"):
        other.load_state_dict({"grids": grids.grids.detach()})


ENTRY_POINTS = ("gsr_bilagrid_slice_fwd", "gsr_bilagrid_slice_bwd", "gsr_bilagrid_tv_fwd_bwd",
                "gsr_bilagrid_workspace_bytes")


def test_library_exports_the_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    import mvs_gaussian_splatting_amd as pkg
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 38
    for name in ("slice_bilateral_grid", "bilateral_grid_tv_loss", "BilateralGrids"):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(pkg.bilagrid, name)


def test_raw_abi_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 256)()
    ptr = C.addressof(buf)
    ptr += (-ptr) % 16
    sizes = [{"H": 0}, {"W": 0}, {"H": -2}, {"H": 2 ** 14 + 1, "W": 2 ** 14}, {"Wg": 1}, {"Wg": 65}, {"Hg": 1}, {"Hg": 65},
             {"L": 1}, {"L": 17}]

    good = dict(x=ptr, grid=ptr, H=4, W=4, Wg=2, Hg=2, L=2, staging=0, y=ptr)
    fwd = lambda **kw: lib.gsr_bilagrid_slice_fwd(*{**good, **kw}.values(), None)         # noqa: E731
    for kw in [{"x": None}, {"grid": None}, {"y": None}, {"staging": 3}, {"staging": -1},
               {"staging": 2, "Wg": 64, "Hg": 64, "L": 16}] + sizes:
        assert fwd(**kw) == -1, kw
        assert lib.gsr_last_error()
    for k in ("x", "grid", "y"):
        assert fwd(**{k: ptr + 2}) == -3, k

    good = dict(x=ptr, grid=ptr, g=ptr, H=4, W=4, Wg=2, Hg=2, L=2, staging=0, dx=ptr, dgrid=ptr, ws=ptr)
    bwd = lambda **kw: lib.gsr_bilagrid_slice_bwd(*{**good, **kw}.values(), None)         # noqa: E731
    for kw in [{"x": None}, {"g": None}, {"grid": None}, {"ws": None}, {"staging": 3}, {"staging": -1},
               {"staging": 2, "Wg": 64, "Hg": 64, "L": 16}] + sizes:
        assert bwd(**kw) == -1, kw
        assert lib.gsr_last_error()
    for k in ("x", "grid", "g", "dx", "dgrid"):
        assert bwd(**{k: ptr + 1}) == -3, k
    assert bwd(ws=ptr + 4) == -3
    # neither gradient asked for: a successful no-op, the grid and the workspace are not needed
    assert bwd(dx=None, dgrid=None, grid=None, ws=None) == 0

    good = dict(grids=ptr, N=1, Wg=2, Hg=2, L=2, value=ptr, dgrids=ptr, ws=ptr)
    tv = lambda **kw: lib.gsr_bilagrid_tv_fwd_bwd(*{**good, **kw}.values(), None)         # noqa: E731
    for kw in [{"grids": None}, {"value": None}, {"ws": None}, {"N": 0}, {"N": -1}, {"N": 2 ** 16 + 1}] + \
            [kw for kw in sizes if set(kw) & {"Wg", "Hg", "L"}]:
        assert tv(**kw) == -1, kw
        assert lib.gsr_last_error()
    for k in ("grids", "value", "dgrids"):
        assert tv(**{k: ptr + 2}) == -3, k
    assert tv(ws=ptr + 4) == -3

    ws = lib.gsr_bilagrid_workspace_bytes
    assert ws(1080, 1920, 16, 16, 8) > 0 and ws(1080, 1920, 16, 16, 8) % 256 == 0
    assert ws(0, 0, 16, 16, 8) > 0                                     # the TV term's
    for bad in ((0, 5, 16, 16, 8), (5, 0, 16, 16, 8), (-1, -1, 16, 16, 8), (8, 8, 1, 16, 8), (8, 8, 16, 65, 8),
                (8, 8, 16, 16, 17), (0, 0, 16, 16, 1), (2 ** 15, 2 ** 15, 16, 16, 8)):
        assert ws(*bad) == 0, bad


class _Cam:
    FoVx = FoVy = 1.0
    image_width, image_height = 8, 8
    original_image = torch.zeros(3, 8, 8)
    image_name = "a"


def test_the_trainer_switch_is_off_by_default_and_refuses_before_rendering(monkeypatch):
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration

    class Plain:
        def __init__(self):
            self.rates = []

        def update_learning_rate(self, iteration):
            self.rates.append(iteration)

    class Stop(Exception):
        pass

    calls = []

    def render(camera, model, pipe, bg, **kw):
        calls.append(kw)
        raise Stop
    monkeypatch.setattr(trainer, "render", render)
    sliced = []
    monkeypatch.setattr(trainer, "slice_bilateral_grid", lambda *a: sliced.append(a))
    monkeypatch.setattr(trainer, "bilateral_grid_tv_loss", lambda *a: sliced.append(a))

    def kwargs(opt, **kw):
        model = Plain()
        with pytest.raises(Stop):
            training_iteration(model, _Cam, opt, None, torch.zeros(3), 10, cameras_extent=1.0, **kw)
        assert model.rates == [10]
        return calls[-1]

    opt = OptimizationParams()
    today = kwargs(opt)
    assert {k: v for k, v in kwargs(opt, bilateral_grids=None).items() if k != "opt"} == \
        {k: v for k, v in today.items() if k != "opt"}
    grids = BilateralGrids(["a"], shape=(2, 2, 2), device="cpu")
    n = len(calls)
    with pytest.raises(ValueError, match="training_setup"):
        training_iteration(Plain(), _Cam, opt, None, torch.zeros(3), 10, cameras_extent=1.0, bilateral_grids=grids)
    grids.training_setup(opt)

    class Other(_Cam):
        image_name = "z"
    with pytest.raises(KeyError, match="no bilateral grid"):
        training_iteration(Plain(), Other, opt, None, torch.zeros(3), 10, cameras_extent=1.0, bilateral_grids=grids)
    assert len(calls) == n, "both refusals come before anything is rendered"
    # with grids the frame is rendered exactly as without them: the grid acts on the image, not on the render call
    on = kwargs(opt, bilateral_grids=grids)
    assert {k: v for k, v in on.items() if k != "opt"} == {k: v for k, v in today.items() if k != "opt"}
    assert grids.optimizer.param_groups[0]["lr"] == pytest.approx(grids.scheduler_args(10))
    assert not sliced


# ---- the limits of the accepted shapes, the large image, black pixels and the TV term past its block cap -------------
WAVE, BG_TERMS, BG_MAX_XY, BG_MAX_L = 64, 12, 64, 16               # the constants of csrc/bilagrid.hip, mirrored
BG_STAGE_FLOATS, BG_STAGE_BLOCKS, BG_STAGE_THREADS, BG_MAX_SHARES = 24576, 256, 1024, 8
BG_TV_THREADS, BG_TV_MAX_BLOCKS, BG_TV_FIN_THREADS = 256, 1024, 256


def _shares(H, Hg):
    """``bilagrid_shares`` of csrc/bilagrid.hip."""
    rows = 2 * (H // (Hg - 1) + 1) + 3
    return min(max((rows + 15) // 16, 1), BG_MAX_SHARES)


def _vertex_range(i, n_px, n_v):
    """``bg_vertex_range`` of csrc/bilagrid_math.h."""
    scale = n_px / (n_v - 1)
    lo, hi = math.floor((i - 1) * scale - 0.5) - 1.0, math.ceil((i + 1) * scale - 0.5) + 1.0
    return int(max(lo, 0.0)), int(min(hi, n_px - 1.0))


def _tv_launch(N, shape):
    """(elements, blocks of bilagrid_tv_kernel, passes of its grid stride, trips of the finish kernel over the slots)."""
    Wg, Hg, L = shape
    total = N * BG_TERMS * L * Hg * Wg
    blocks = min(-(-total // BG_TV_THREADS), BG_TV_MAX_BLOCKS)
    return total, blocks, -(-total // (blocks * BG_TV_THREADS)), -(-blocks // BG_TV_FIN_THREADS)


def test_the_mirrored_constants_are_the_sources():
    text = ""
    for name in ("bilagrid.hip", "bilagrid_math.h", "gsr_common.h"):
        with open(os.path.join(CSRC, name)) as f:
            text += f.read()
    for name, value in (("BG_TERMS", BG_TERMS), ("BG_MAX_XY", BG_MAX_XY), ("BG_MAX_L", BG_MAX_L),
                        ("BG_STAGE_BLOCKS", BG_STAGE_BLOCKS), ("BG_STAGE_THREADS", BG_STAGE_THREADS),
                        ("BG_MAX_SHARES", BG_MAX_SHARES), ("BG_TV_THREADS", BG_TV_THREADS),
                        ("BG_TV_MAX_BLOCKS", BG_TV_MAX_BLOCKS), ("BG_TV_FIN_THREADS", BG_TV_FIN_THREADS), ("WAVE", WAVE)):
        found = re.search(r"\b%s = (\d+)\b" % name, text)
        assert found and int(found.group(1)) == value, name
    assert "BG_STAGE_FLOATS = BG_TERMS * 8 * 16 * 16;" in text and BG_STAGE_FLOATS == BG_TERMS * 8 * 16 * 16
    assert "__launch_bounds__(WAVE * BG_MAX_L)" in text


def test_the_limit_cases_have_the_shapes_they_are_there_for():
    assert len(R.LIMIT_CASES) <= 16
    for (H, W), (Wg, Hg, L), lanes, fits, shares in R.LIMIT_CASES:
        assert 2 <= Wg <= BG_MAX_XY and 2 <= Hg <= BG_MAX_XY and 2 <= L <= BG_MAX_L
        assert lanes == WAVE * L <= WAVE * BG_MAX_L
        assert fits == (BG_TERMS * L * Hg * Wg <= BG_STAGE_FLOATS), ((H, W), (Wg, Hg, L))
        assert shares == _shares(H, Hg), ((H, W), (Wg, Hg, L))
    cases = [c[:2] for c in R.LIMIT_CASES]
    by_shape = {shape: (lanes, fits) for _, shape, lanes, fits, _ in R.LIMIT_CASES}
    # L = 16: the block of 1024 lanes, beside the smallest extents, odd ones and the default ones
    for shape in ((2, 2, 16), (5, 3, 16), (16, 16, 16)):
        assert by_shape[shape][0] == 1024 and ((70, 37), shape) in cases and ((3, 130), shape) in cases
    # each extent at 64 on an image narrower than the grid and on a wider one; (16,16,16) and (64,64,2) do not fit LDS
    for shape in ((64, 2, 2), (2, 64, 2), (64, 64, 2), (64, 64, 16)):
        assert ((7, 5), shape) in cases and ((70, 37), shape) in cases
    assert not by_shape[(16, 16, 16)][1] and not by_shape[(64, 64, 2)][1] and not by_shape[(64, 64, 16)][1]
    assert by_shape[(64, 64, 16)][0] == 1024 and ((65, 9), (33, 17, 9)) in cases
    assert {c[4] for c in R.LIMIT_CASES} >= {1, 2, 5, 8}, "one share, a few and the most"
    # no case widens the tables that were there
    assert not {shape for _, shape in cases} & set(R.GRID_SHAPES)


def test_census_of_the_new_gpu_test_inputs():
    H, W = R.LARGE_IMAGE
    inputs = [(f"{h}x{w}", R.make_image(h, w), shape[2]) for (h, w), shape, *_ in R.LIMIT_CASES]
    inputs += [(f"{H}x{W}", R.make_image(H, W), shape[2]) for shape in R.LARGE_GRIDS]
    inputs += [("black %dx%d" % R.BLACK_IMAGE, R.make_image_with_black(*R.BLACK_IMAGE)[0], shape[2])
               for shape in R.BLACK_GRIDS]
    seen = set()
    for label, x, L in inputs:
        if (label, L) in seen:
            continue
        seen.add((label, L))
        n, pixels, cap = R.census(x, L)
        print(f"census {label} L={L}: {n} fragile of {pixels} (cap {cap})")
        assert n <= cap


def test_the_host_build_meets_the_bar_at_the_limits_of_the_shape_range(host_program, tmp_path):
    for (H, W), shape, *_ in R.LIMIT_CASES:
        x, grid, up = R.make_image(H, W), R.make_grid(shape), R.make_upstream(H, W)
        got = _run_host(host_program, tmp_path, x, grid, up)
        label = f"{H}x{W} grid {shape}"
        R.check_slice(got, x, grid, up, label)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        none = R.check_untouched(got[2], x, shape, label)
        if (H, W) == (7, 5) and max(shape[:2]) == 64:
            assert 2 * none > shape[0] * shape[1] * shape[2], "narrower than the grid: most vertices see no pixel"


def test_the_large_image_has_several_row_shares_and_column_trips_and_the_host_build_meets_the_bar(host_program, tmp_path):
    H, W = R.LARGE_IMAGE
    assert H * W >= BG_STAGE_BLOCKS * BG_STAGE_THREADS > (H - 2) * W, "staged by AUTO, and the first such height but one"
    assert H * W > BG_STAGE_BLOCKS * BG_STAGE_THREADS, "more than one pass of the staged kernel's grid stride"
    fits = [BG_TERMS * L * Hg * Wg <= BG_STAGE_FLOATS for Wg, Hg, L in R.LARGE_GRIDS]
    assert fits == [True, False]
    for Wg, Hg, L in R.LARGE_GRIDS:
        assert _shares(H, Hg) == 5
        widths = [hi - lo + 1 for lo, hi in (_vertex_range(i, W, Wg) for i in range(Wg))]
        print(f"{H}x{W} grid {(Wg, Hg, L)}: {_shares(H, Hg)} row shares, {min(widths)}..{max(widths)} columns a vertex")
        assert max(widths) > WAVE and sorted(widths)[Wg // 2] > WAVE, "more than one 64-lane trip along a row"
    shape = R.LARGE_GRIDS[0]
    x, grid, up = R.make_image(H, W), R.make_grid(shape), R.make_upstream(H, W)
    R.check_slice(_run_host(host_program, tmp_path, x, grid, up), x, grid, up, f"{H}x{W} grid {shape}")


def test_grid_sample_has_no_coordinate_gradient_on_the_border_and_black_pixels_meet_the_bar_on_the_host(host_program,
                                                                                                      tmp_path):
    """torch's ``grid_sample(padding_mode="border")`` gives a coordinate exactly on the border a zero gradient, as
    ``bg_pixel`` does with ``gray > 0``: so the restatement is the reference at a black pixel as it stands."""
    import torch.nn.functional as F
    grid = R.make_grid((3, 5, 4)).to(F64)[None]
    for z, zero in ((-1.0, True), (1.0, True), (-1.0 + 1e-9, False), (1.0 - 1e-9, False)):
        for dtype in (F64, torch.float32):
            c = torch.tensor([[[[[0.3, -0.2, z]]]]], dtype=dtype, requires_grad=True)
            F.grid_sample(grid.to(dtype), c, mode="bilinear", padding_mode="border", align_corners=True).sum().backward()
            assert (float(c.grad[..., 2]) == 0.0) == (zero or dtype == torch.float32), (z, dtype)
            assert float(c.grad[..., 0]) != 0.0
    H, W = R.BLACK_IMAGE
    x, black = R.make_image_with_black(H, W)
    up = R.make_upstream(H, W)
    assert 30 < int(black.sum()) < 40 and bool((R.gray(x.to(F64))[black] == 0).all())
    assert bool((x[:, black] == 0).all()) and torch.equal(x[:, ~black], R.make_image(H, W)[:, ~black])
    for shape in R.BLACK_GRIDS:
        Wg, Hg, L = shape
        grid = R.make_grid(shape)
        # the rectangle lies across a cell boundary in x and in y
        ys, xs = torch.nonzero(black[H // 2 - 20:H // 2 - 14].any(1)), torch.nonzero(black[H // 2 - 17])
        ys = ys.flatten() + H // 2 - 20
        assert len({int((int(py) + 0.5) / H * (Hg - 1)) for py in ys}) > 1
        assert len({int((int(px) + 0.5) / W * (Wg - 1)) for px in xs.flatten()}) > 1
        _, dx64, _ = R.slice_with_grads(x, grid, up)
        want = R.image_grad_without_the_luminance(x, grid, up)
        assert R.rel_err(dx64[:, black], want[:, black]) < 1e-14, "autograd of the restatement: nothing through z"
        assert R.rel_err(dx64[:, ~black], want[:, ~black]) > 1e-3, "elsewhere the luminance path carries weight"
        got = _run_host(host_program, tmp_path, x, grid, up)
        label = f"black {H}x{W} grid {shape}"
        R.check_slice(got, x, grid, up, label)
        R.check_black(got[1], x, black, grid, up, label)


def test_the_tv_limit_cases_reach_the_blocks_and_passes_they_claim():
    assert max(_tv_launch(N, shape)[1] for N, shape in R.TV_CASES) <= BG_TV_FIN_THREADS, "what was there: one trip each"
    for N, shape, blocks, passes in R.TV_LIMIT_CASES:
        assert _tv_launch(N, shape)[1:3] == (blocks, passes), (N, shape)
    launch = {(N, shape): _tv_launch(N, shape) for N, shape, *_ in R.TV_LIMIT_CASES}
    assert launch[(3, (16, 16, 8))] == (73728, 288, 1, 2), "the finish kernel's second trip over the slots"
    assert launch[(11, (16, 16, 8))] == (270336, 1024, 2, 4) and 270336 - 1024 * 256 == 8192
    assert launch[(1, (64, 64, 16))] == (786432, 1024, 3, 4)
    for shape in ((2, 2, 16), (64, 2, 2), (2, 64, 2)):
        assert any(s == shape for _, s, *_ in R.TV_LIMIT_CASES)
    assert _tv_launch(*R.TV_STRUCTURAL_CASE)[1:3] == (1024, 2) and _tv_launch(10, (16, 16, 8))[2] == 1
    # the structural grids: every difference inside a term is 0, so the value and the gradient are exact zeros
    grids = R.make_constant_term_grids(*R.TV_STRUCTURAL_CASE)
    assert grids.unique().numel() == 12 * R.TV_STRUCTURAL_CASE[0] and bool((grids == grids.round()).all())
    value, grad = R.tv_with_grad(grids)
    assert float(value) == 0.0 and bool((grad == 0).all())
