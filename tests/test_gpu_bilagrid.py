"""Per-image bilateral grids on the GPU: the slice, both of its gradients and the total-variation term
against the float64 restatement at the bar of tests/bilagrid_restate.py (twice the float32 restatement's own error, not
less than 2^-22), the bit-for-bit properties, and the training iteration with grids."""
import os
import sys

import pytest
import torch

from conftest import ROOT
import bilagrid_restate as R

pytestmark = pytest.mark.gpu

CASES = [(hw, shape) for hw in R.IMAGE_SHAPES for shape in R.GRID_SHAPES]
NAMES = ["view_a", "view_b"]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _call(dev, x, grid, up, want_dx=True, want_dg=True, fill=None):
    """One forward and one backward through the wrapper -> (Y, dX or None, dG or None) on the CPU.  fill: the caching
    allocator is primed with blocks of that value, so that the outputs the wrapper allocates start as garbage."""
    from mvs_gaussian_splatting_amd import slice_bilateral_grid
    if fill is not None:
        junk = [torch.full_like(x, fill, device=dev), torch.full_like(x, fill, device=dev),
                torch.full_like(grid, fill, device=dev)]
        del junk
    xg = x.to(dev).requires_grad_(want_dx)
    gg = grid.to(dev).requires_grad_(want_dg)
    y = slice_bilateral_grid(xg, gg)
    y.backward(up.to(dev))
    return y.detach().cpu(), None if xg.grad is None else xg.grad.cpu(), None if gg.grad is None else gg.grad.cpu()


@pytest.mark.parametrize("hw,shape", CASES, ids=[f"{h}x{w}-{'x'.join(map(str, s))}" for (h, w), s in CASES])
def test_slice_and_gradients_meet_the_bar_and_are_the_same_bits_every_way(gpu_device, hw, shape):
    (H, W) = hw
    x, grid, up = R.make_image(H, W), R.make_grid(shape), R.make_upstream(H, W)
    got = _call(gpu_device, x, grid, up)
    R.check_slice(got, x, grid, up, f"{H}x{W} grid {shape}")
    again = _call(gpu_device, x, grid, up, fill=float("nan"))
    for a, b in zip(got, again):
        assert torch.equal(_bits(a), _bits(b)), "two runs, the second into garbage-filled buffers, give the same bits"
    only_dx = _call(gpu_device, x, grid, up, want_dg=False)
    only_dg = _call(gpu_device, x, grid, up, want_dx=False)
    assert only_dx[2] is None and only_dg[1] is None
    assert torch.equal(_bits(only_dx[1]), _bits(got[1])) and torch.equal(_bits(only_dg[2]), _bits(got[2]))
    y, dx, _ = _call(gpu_device, x, R.identity_grid(shape), up)
    assert torch.equal(y, x) and torch.equal(dx, up), "the identity grid changes no bit of the image or of its gradient"


def test_raw_calls_write_every_element_and_do_not_depend_on_the_staging(gpu_device):
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    (H, W), shape = (70, 37), (16, 16, 8)
    Wg, Hg, L = shape
    x, grid, up = (t.to(gpu_device) for t in (R.make_image(H, W), R.make_grid(shape), R.make_upstream(H, W)))
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    outs = []
    for staging in (_lib.BILAGRID_STAGE_AUTO, _lib.BILAGRID_STAGE_CACHE, _lib.BILAGRID_STAGE_LDS):
        y = torch.full_like(x, float("nan"))
        _lib.check(lib.gsr_bilagrid_slice_fwd(x.data_ptr(), grid.data_ptr(), H, W, Wg, Hg, L, staging, y.data_ptr(),
                                              stream), "fwd")
        outs.append(y)
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
    assert bool(torch.isfinite(outs[0]).all())
    # both gradients into NaN-filled buffers, from a 0xff-filled workspace, under every staging: the wrapper's bits
    want = _call(gpu_device, x.cpu(), grid.cpu(), up.cpu())
    assert torch.equal(_bits(outs[0].cpu()), _bits(want[0]))
    for staging in (_lib.BILAGRID_STAGE_AUTO, _lib.BILAGRID_STAGE_CACHE, _lib.BILAGRID_STAGE_LDS):
        dx, dg = torch.full_like(x, float("nan")), torch.full_like(grid, float("nan"))
        ws = torch.full((lib.gsr_bilagrid_workspace_bytes(H, W, Wg, Hg, L),), 0xff, dtype=torch.uint8, device=gpu_device)
        _lib.check(lib.gsr_bilagrid_slice_bwd(x.data_ptr(), grid.data_ptr(), up.data_ptr(), H, W, Wg, Hg, L, staging,
                                              dx.data_ptr(), dg.data_ptr(), ws.data_ptr(), stream), "bwd")
        assert torch.equal(_bits(dx.cpu()), _bits(want[1])) and torch.equal(_bits(dg.cpu()), _bits(want[2]))
    # a 3 x 130 image under a 16 x 16 grid: most vertices receive no pixel and are written as zeros over the garbage
    (H, W) = (3, 130)
    x, up = R.make_image(H, W).to(gpu_device), R.make_upstream(H, W).to(gpu_device)
    dg = torch.full_like(grid, float("nan"))
    ws = torch.full((lib.gsr_bilagrid_workspace_bytes(H, W, Wg, Hg, L),), 0xff, dtype=torch.uint8, device=gpu_device)
    _lib.check(lib.gsr_bilagrid_slice_bwd(x.data_ptr(), None, up.data_ptr(), H, W, Wg, Hg, L, 0, None, dg.data_ptr(),
                                          ws.data_ptr(), stream), "bwd")
    assert bool(torch.isfinite(dg).all()) and int((dg == 0).sum()) > 0


def test_at_the_size_where_the_library_turns_to_lds_the_bits_stay(gpu_device):
    """512 x 512 = 262144 pixels is the first size at which GSR_BILAGRID_STAGE_AUTO stages the default grid in LDS, 511 x
    512 the last at which it does not: at both, the wrapper's Y and dX are the bits of the forced cache path, and more
    than one pass of the staged kernel's grid stride is walked at 513 x 512."""
    from mvs_gaussian_splatting_amd import _lib, slice_bilateral_grid
    lib = _lib.load()
    shape = (16, 16, 8)
    Wg, Hg, L = shape
    grid = R.make_grid(shape).to(gpu_device)
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    for H, W in ((511, 512), (512, 512), (513, 512)):
        x = R.make_image(H, W).to(gpu_device).requires_grad_(True)
        up = R.make_upstream(H, W).to(gpu_device)
        y = slice_bilateral_grid(x, grid)
        y.backward(up)
        for staging in (_lib.BILAGRID_STAGE_CACHE, _lib.BILAGRID_STAGE_LDS):
            y2, dx2 = torch.full_like(y, float("nan")), torch.full_like(y, float("nan"))
            _lib.check(lib.gsr_bilagrid_slice_fwd(x.data_ptr(), grid.data_ptr(), H, W, Wg, Hg, L, staging, y2.data_ptr(),
                                                  stream), "fwd")
            _lib.check(lib.gsr_bilagrid_slice_bwd(x.data_ptr(), grid.data_ptr(), up.data_ptr(), H, W, Wg, Hg, L, staging,
                                                  dx2.data_ptr(), None, None, stream), "bwd")
            assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(dx2), _bits(x.grad))


def test_non_contiguous_inputs_give_the_results_of_their_contiguous_copies(gpu_device):
    from mvs_gaussian_splatting_amd import slice_bilateral_grid, bilateral_grid_tv_loss
    (H, W), shape = (7, 5), (3, 5, 4)
    x = R.make_image(H, W).to(gpu_device).permute(1, 2, 0).contiguous().permute(2, 0, 1)          # HWC memory
    grid = R.make_grid(shape).to(gpu_device).permute(3, 2, 1, 0).contiguous().permute(3, 2, 1, 0)
    up = R.make_upstream(H, W).to(gpu_device).permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not x.is_contiguous() and not grid.is_contiguous() and not up.is_contiguous()
    res = []
    for xi, gi, ui in ((x, grid, up), (x.contiguous(), grid.contiguous(), up.contiguous())):
        xi, gi = xi.detach().requires_grad_(True), gi.detach().requires_grad_(True)
        y = slice_bilateral_grid(xi, gi)
        y.backward(ui)
        res.append((y.detach(), xi.grad, gi.grad))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
    grids = R.make_grids(3, shape).to(gpu_device)
    strided = grids.permute(0, 1, 4, 3, 2).contiguous().permute(0, 1, 4, 3, 2)
    assert not strided.is_contiguous()
    assert torch.equal(_bits(bilateral_grid_tv_loss(strided)), _bits(bilateral_grid_tv_loss(grids)))


def _check_tv(gpu_device, N, shape):
    from mvs_gaussian_splatting_amd import bilateral_grid_tv_loss
    grids = R.make_grids(N, shape)
    v64, g64 = R.tv_with_grad(grids)
    v32, g32 = R.tv_with_grad(grids, torch.float32)
    runs = []
    for _ in range(2):
        dev_grids = grids.to(gpu_device).requires_grad_(True)
        value = bilateral_grid_tv_loss(dev_grids)
        assert value.dim() == 0 and value.device == dev_grids.device
        (4.0 * value).backward()                              # a power of two: the upstream gradient rounds nothing
        runs.append((value.detach().cpu(), dev_grids.grad.cpu() / 4.0))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    for name, got, a, b in (("value", runs[0][0], v64, v32), ("gradient", runs[0][1], g64, g32)):
        err, own = R.rel_err(got, a), R.rel_err(b, a)
        print(f"tv N={N} grid {shape} {name}: error {err:.3e}  float32 restatement {own:.3e}  bar {R.bar(own):.3e}")
        assert err <= R.bar(own), f"tv {name}: {err:.3e} above the bar {R.bar(own):.3e}"
    no_grad = bilateral_grid_tv_loss(grids.to(gpu_device))
    assert torch.equal(_bits(no_grad.cpu()), _bits(runs[0][0])) and not no_grad.requires_grad


@pytest.mark.parametrize("N,shape", R.TV_CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s in R.TV_CASES])
def test_tv_value_and_gradient_meet_the_bar_and_are_reproducible(gpu_device, N, shape):
    _check_tv(gpu_device, N, shape)


@pytest.mark.parametrize("N,shape", [c[:2] for c in R.TV_LIMIT_CASES],
                         ids=[f"{n}-{'x'.join(map(str, s))}" for n, s, *_ in R.TV_LIMIT_CASES])
def test_tv_past_256_slots_past_the_block_cap_and_at_every_extent(gpu_device, N, shape):
    """More blocks than one trip of the finish kernel reads, more elements than one pass of the capped launch covers
    (tests/test_bilagrid_host.py asserts the block and pass counts), and each extent at the largest accepted."""
    _check_tv(gpu_device, N, shape)


def test_tv_of_grids_constant_within_each_term_is_exactly_zero_past_the_block_cap(gpu_device):
    """Every difference inside a term of an image is exactly 0 and every difference across a row, slab, term or image
    boundary is a non-zero integer: a kernel that takes one of those, in the first pass or in the grid stride's second,
    gives a value or a gradient element that is not zero."""
    from mvs_gaussian_splatting_amd import bilateral_grid_tv_loss
    grids = R.make_constant_term_grids(*R.TV_STRUCTURAL_CASE).to(gpu_device).requires_grad_(True)
    value = bilateral_grid_tv_loss(grids)
    value.backward()
    value = float(value.detach())
    print(f"tv of constant terms: value {value!r}, {int((grids.grad != 0).sum())} gradient elements not zero, "
          f"largest {float(grids.grad.abs().max())!r}")
    assert value == 0.0
    assert bool((grids.grad == 0).all()), "every gradient element is an exact zero, of either sign"


# ---- the limits of the shape range, the large image, black pixels ----------------------------------------------------
GSR_E_BADARG = -1
STAGINGS = ("AUTO", "CACHE", "LDS")


def _raw(dev, lib, x, grid, up, staging):
    """The two raw entry points under one staging, into NaN-filled outputs and from a 0xff-filled workspace ->
    (status of the forward, status of the backward, Y, dX, dG), the tensors on the device."""
    H, W = x.shape[1:]
    L, Hg, Wg = grid.shape[1:]
    stream = torch.cuda.current_stream(dev).cuda_stream
    y, dx, dg = torch.full_like(x, float("nan")), torch.full_like(x, float("nan")), torch.full_like(grid, float("nan"))
    ws = torch.full((lib.gsr_bilagrid_workspace_bytes(H, W, Wg, Hg, L),), 0xff, dtype=torch.uint8, device=dev)
    fwd = lib.gsr_bilagrid_slice_fwd(x.data_ptr(), grid.data_ptr(), H, W, Wg, Hg, L, staging, y.data_ptr(), stream)
    bwd = lib.gsr_bilagrid_slice_bwd(x.data_ptr(), grid.data_ptr(), up.data_ptr(), H, W, Wg, Hg, L, staging,
                                     dx.data_ptr(), dg.data_ptr(), ws.data_ptr(), stream)
    return fwd, bwd, y, dx, dg


def _every_staging_gives(dev, want, x, grid, up, fits, label):
    """Every accepted staging writes every element of NaN-filled outputs, from a 0xff-filled workspace, with the bits of
    ``want``; GSR_BILAGRID_STAGE_LDS with a grid that does not fit LDS is refused with the bad-argument status and leaves
    the NaN-filled outputs as they were, bit for bit."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    xd, gd, ud = x.to(dev), grid.to(dev), up.to(dev)
    for name in STAGINGS:
        fwd, bwd, y, dx, dg = _raw(dev, lib, xd, gd, ud, getattr(_lib, "BILAGRID_STAGE_" + name))
        if name == "LDS" and not fits:
            assert (fwd, bwd) == (GSR_E_BADARG, GSR_E_BADARG), f"{label}: a grid that does not fit LDS is refused"
            assert b"24576" in lib.gsr_last_error()
            for t in (y, dx, dg):
                assert torch.equal(_bits(t), _bits(torch.full_like(t, float("nan")))), "a refusal writes nothing"
            continue
        assert (fwd, bwd) == (0, 0), f"{label} {name}: {lib.gsr_last_error()}"
        for what, t, w in zip(("Y", "dX", "dG"), (y, dx, dg), want):
            assert torch.equal(_bits(t.cpu()), _bits(w)), f"{label}: {what} under {name} has the wrapper's bits"


LIMITS = [(c[0], c[1], c[3]) for c in R.LIMIT_CASES]


@pytest.mark.parametrize("hw,shape,fits", LIMITS, ids=[f"{h}x{w}-{'x'.join(map(str, s))}" for (h, w), s, _ in LIMITS])
def test_at_the_limits_of_the_shape_range_the_bar_is_met_and_the_bits_are_the_same_every_way(gpu_device, hw, shape, fits):
    """L = 16 (a grid-gradient block of 1024 lanes), each extent at 64, a grid that LDS does not hold, an image narrower
    than the grid and an odd shape: tests/test_bilagrid_host.py asserts that the cases are those."""
    (H, W) = hw
    x, grid, up = R.make_image(H, W), R.make_grid(shape), R.make_upstream(H, W)
    label = f"{H}x{W} grid {shape}"
    got = _call(gpu_device, x, grid, up)
    R.check_slice(got, x, grid, up, label)
    R.check_untouched(got[2], x, shape, label)
    again = _call(gpu_device, x, grid, up, fill=float("nan"))
    for a, b in zip(got, again):
        assert torch.equal(_bits(a), _bits(b)), "two runs, the second into garbage-filled buffers, give the same bits"
    _every_staging_gives(gpu_device, got, x, grid, up, fits, label)


@pytest.fixture(scope="module")
def large_inputs():
    H, W = R.LARGE_IMAGE
    return R.make_image(H, W), R.make_upstream(H, W)


def test_the_large_image_meets_the_bar_and_its_grid_gradient_is_the_same_bits_under_every_staging(gpu_device, large_inputs):
    """513 x 512 under the default grid: AUTO stages the grid in LDS and walks more than one pass of its grid stride,
    the grid gradient has 5 row shares and more than one 64-lane trip per row (tests/test_bilagrid_host.py)."""
    x, up = large_inputs
    shape = R.LARGE_GRIDS[0]
    grid = R.make_grid(shape)
    label = "%dx%d grid %s" % (*R.LARGE_IMAGE, shape)
    got = _call(gpu_device, x, grid, up)
    R.check_slice(got, x, grid, up, label)
    _every_staging_gives(gpu_device, got, x, grid, up, True, label)


def test_the_large_image_under_a_grid_that_lds_does_not_hold_takes_the_cache_path_and_refuses_lds(gpu_device, large_inputs):
    """513 x 512 under (16,16,16): AUTO must not stage 49152 floats, so its bits are the forced cache path's; forcing LDS
    is refused on valid memory with every output untouched, and the call after the refusal is right."""
    x, up = large_inputs
    shape = R.LARGE_GRIDS[1]
    grid = R.make_grid(shape)
    label = "%dx%d grid %s" % (*R.LARGE_IMAGE, shape)
    got = _call(gpu_device, x, grid, up)
    _every_staging_gives(gpu_device, got, x, grid, up, False, label)
    after = _call(gpu_device, x, grid, up, fill=float("nan"))
    R.check_slice(after, x, grid, up, label + " after the refusal")
    for a, b in zip(got, after):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("shape", R.BLACK_GRIDS, ids=["x".join(map(str, s)) for s in R.BLACK_GRIDS])
def test_exactly_black_pixels_meet_the_bar_and_their_gradient_is_the_affines_alone(gpu_device, shape):
    """A luminance of exactly 0 is the strict side of ``gray > 0``: ``dz/dgray = 0`` and ``dX = A^T g``."""
    H, W = R.BLACK_IMAGE
    (x, black), grid, up = R.make_image_with_black(H, W), R.make_grid(shape), R.make_upstream(H, W)
    label = f"black {H}x{W} grid {shape}"
    got = _call(gpu_device, x, grid, up)
    R.check_slice(got, x, grid, up, label)
    R.check_black(got[1], x, black, grid, up, label)
    again = _call(gpu_device, x, grid, up, fill=float("nan"))
    for a, b in zip(got, again):
        assert torch.equal(_bits(a), _bits(b))


# ---- the training iteration ------------------------------------------------------------------------------------------
def _example():
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import train as example
    return example


@pytest.fixture(scope="module")
def problem(gpu_device):
    """64 x 48, a few hundred Gaussians, two named cameras; the photograph of the first is multiplied by a smooth
    left-to-right gain ramp, which no global exposure explains."""
    cams, bg, cloud = _example().make_problem(gpu_device, P=600, W=64, H=48, n_views=2)
    for cam, name in zip(cams, NAMES):
        cam.image_name = name
    ramp = torch.linspace(0.7, 1.3, 64, device=gpu_device)
    cams[0].original_image = (cams[0].original_image * ramp[None, None, :]).contiguous()
    return cams, bg, cloud


def _run(problem, opt, iterations, grids=None, pass_argument=True, frame=0, **kw):
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import training_iteration
    ex = _example()
    cams, bg, _ = problem
    model = ex.make_model(problem, opt)
    if kw.get("train_exposure"):
        model.setup_exposures(NAMES)
        model.training_setup(opt)
    losses = []
    for iteration in range(1, iterations + 1):
        torch.manual_seed(iteration)
        extra = {"bilateral_grids": grids} if pass_argument else {}
        losses.append(training_iteration(model, cams[frame], opt, PipelineParams(), bg, iteration,
                                         cameras_extent=ex.CAMERAS_EXTENT, **extra, **kw))
    return model, losses


def _params(model):
    return [grp["params"][0].detach().clone() for grp in model.optimizer.param_groups]


def test_three_iterations_move_the_frames_grid_only(gpu_device, problem):
    from mvs_gaussian_splatting_amd import BilateralGrids
    ex = _example()
    eye = R.identity_grid((16, 16, 8)).to(gpu_device)
    for lambda_tv in (0.0, 10.0):
        opt = ex.small_opt(40, lambda_tv=lambda_tv)
        grids = BilateralGrids(NAMES, device=gpu_device)
        grids.training_setup(opt)
        _, losses = _run(problem, opt, 3, grids)
        assert all(bool(torch.isfinite(v)) for v in losses)
        moved = grids.grids.detach()
        assert float((moved[0] - eye).abs().max()) > 1e-4, "the grid of the frame's camera has moved"
        assert float((moved[0] - eye).abs().max()) <= 3 * 2e-3 * (1 + 1e-5)      # three Adam steps: at most lr each
        # the other camera's grid receives the TV term's gradient alone: exactly zero at the identity, whose
        # differences are all zero -- so with lambda_tv = 0, and with it on, the grid stays the identity bit for bit
        assert torch.equal(_bits(moved[1]), _bits(eye)), f"lambda_tv={lambda_tv}: the other grid is the identity"
        assert grids.grids.grad is None


def test_the_combined_run_with_exposures_and_sparse_adam_completes(gpu_device, problem):
    from mvs_gaussian_splatting_amd import BilateralGrids
    opt = _example().small_opt(40, optimizer_type="sparse_adam")
    grids = BilateralGrids(NAMES, shape=(8, 6, 4), device=gpu_device)
    grids.training_setup(opt)
    model, losses = _run(problem, opt, 3, grids, train_exposure=True)
    assert all(bool(torch.isfinite(v)) for v in losses)
    assert not torch.equal(model._exposure.detach()[0], torch.eye(3, 4, device=gpu_device))
    assert float((grids.grid_for("view_a").detach() - R.identity_grid((8, 6, 4)).to(gpu_device)).abs().max()) > 0


def test_without_grids_the_iteration_is_the_parents_bit_for_bit(gpu_device, problem):
    opt = _example().small_opt(40)
    with_none, loss_none = _run(problem, opt, 3, None)
    never, loss_never = _run(problem, opt, 3, pass_argument=False)
    for a, b in zip(loss_none, loss_never):
        assert torch.equal(_bits(a), _bits(b))
    for a, b in zip(_params(with_none), _params(never)):
        assert torch.equal(_bits(a), _bits(b))


def test_save_and_load_round_trip_the_parameter_and_the_optimizer_state(gpu_device, problem, tmp_path):
    from mvs_gaussian_splatting_amd import BilateralGrids
    opt = _example().small_opt(40)
    grids = BilateralGrids(NAMES, shape=(8, 6, 4), device=gpu_device)
    grids.training_setup(opt)
    _run(problem, opt, 2, grids)
    path = str(tmp_path / "bilateral_grid_2.pt")
    grids.save(path)
    other = BilateralGrids(NAMES, shape=(8, 6, 4), device=gpu_device)
    other.training_setup(opt)
    other.load(path)
    assert torch.equal(_bits(other.grids), _bits(grids.grids)) and other.grids.device == grids.grids.device
    a, b = grids.optimizer.state[grids.grids], other.optimizer.state[other.grids]
    assert float(a["step"]) == float(b["step"]) == 2.0
    for key in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(a[key]), _bits(b[key])) and float(a[key].abs().max()) > 0
    # and the next iteration of either is the same
    for g in (grids, other):
        _run(problem, opt, 1, g)
    assert torch.equal(_bits(other.grids), _bits(grids.grids))
