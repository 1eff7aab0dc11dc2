"""Absolute-gradient densification (AbsGS) without a GPU: the restatement of tests/abs_grad_restate.py is
proved against the oracle's own autograd, the library's surface, and every refusal of the new switches."""
import ctypes as C
import os
import re
import types

import pytest
import torch

import abs_grad_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_SCENES = ("small", "big", "behind", "stacked")


@pytest.mark.parametrize("name", ALL_SCENES)
def test_the_oracle_alone_leaves_few_covered_pixels_out(name):
    fr = R.oracle_frame(name)
    print(f"[abs_grad] scene {name}: {int(fr['covered'].sum())} covered pixels, share left out {fr['left_out']:.4f}")
    assert fr["left_out"] <= R.MAX_LEFT_OUT


@pytest.mark.parametrize("name", ALL_SCENES)
def test_signed_sum_of_the_pair_gradients_is_the_oracles_means2D_gradient(name):
    """The proof of the restatement: the same per-pair gradients, summed with their sign, are the float64 oracle's
    autograd gradient of means2D to 1e-12 (relative to the column's largest value)."""
    fr = R.oracle_frame(name)
    assert float(fr["settings"].bg.abs().max()) == 0.0, "the scenes' own background is black"
    _, signed = R.reference(name, "black")[torch.float64]
    g = R.oracle_means2D_grad(name)
    assert signed.dtype == g.dtype == torch.float64 and tuple(signed.shape) == tuple(g.shape)
    for c in range(2):
        scale = float(g[:, c].abs().max())
        assert scale > 0.0
        err = float((signed[:, c] - g[:, c]).abs().max()) / scale
        print(f"[abs_grad] scene {name}, component {c}: signed restatement vs oracle autograd {err:.2e}")
        assert err <= 1e-12
    assert float(signed[:, 2].abs().max()) == 0.0 and float(g[:, 2].abs().max()) == 0.0


@pytest.mark.parametrize("bg_name", list(R.BACKGROUNDS))
@pytest.mark.parametrize("name", ALL_SCENES)
def test_abs_dominates_signed_and_culled_rows_are_zero(name, bg_name):
    fr = R.oracle_frame(name)
    for dt in (torch.float64, torch.float32):
        a, s = R.reference(name, bg_name)[dt]
        assert bool((a >= s.abs()).all())
        assert float(a[fr["radii"] == 0].abs().max() if bool((fr["radii"] == 0).any()) else 0.0) == 0.0
        assert float(a[:, 2].abs().max()) == 0.0
    a64, s64 = R.reference(name, bg_name)[torch.float64]
    assert float((a64[:, :2] - s64[:, :2].abs()).max()) > 0.0, "no Gaussian whose per-pixel gradients cancel: a weak scene"
    if name == "behind":
        assert all(int(fr["radii"][i]) == 0 for i in R.BEHIND)


def test_the_background_changes_the_reference():
    """A kernel that forgets the start of U must fail the coloured case: the two references differ by far more than the bar."""
    a0, _ = R.reference("small", "black")[torch.float64]
    a1, _ = R.reference("small", "coloured")[torch.float64]
    assert float((a0 - a1).abs().max()) / float(a0.abs().max()) > 1e-2


def test_library_surface_and_abi():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    for name in ("gsr_abs_grad_backward", "gsr_densify_plan_abs", "gsr_densify_stats_abs"):
        assert hasattr(lib, name) and name in header and name in _lib.SYMBOLS
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 40
    # argument checks come before any HIP call
    assert lib.gsr_abs_grad_backward(None, None, None, None, None) == -1
    params, frame = _lib.GsrParams(), _lib.GsrAuxFrame()
    params.P = frame.P = 4
    params.width = frame.width = 32
    params.height = frame.height = 16
    frame.binning_mode = _lib.BINNING_TWO_LEVEL
    one = (C.c_float * 64)()
    frame.img_ws = C.addressof(one)
    assert lib.gsr_abs_grad_backward(C.byref(params), C.byref(frame), None, None, None) == -1      # NULL dL_dcolor / output / bg
    params.forward_only = 1
    assert lib.gsr_abs_grad_backward(C.byref(params), C.byref(frame), C.addressof(one), C.addressof(one), None) == -1
    assert b"forward_only" in lib.gsr_last_error()
    counts = (C.c_uint32 * 4)()
    assert lib.gsr_densify_plan_abs(-1, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, None, 0, counts, None) == -1
    assert lib.gsr_densify_plan_abs(0, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, None, 0, counts, None) == 0
    assert lib.gsr_densify_plan_abs(8, None, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, None, 0, counts, None) == -1
    assert lib.gsr_densify_stats_abs(8, None, None, None, None) == -1
    assert lib.gsr_densify_stats_abs(0, None, None, None, None) == 0


def _cpu_call(**over):
    """Arguments of ``rasterize_gaussians`` on CPU tensors: a refusal must come before a GPU is asked for."""
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings
    P = 5
    e = torch.empty(0)
    st = GaussianRasterizationSettings(16, 32, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                       False, False)
    kw = dict(means3D=torch.zeros(P, 3, requires_grad=True), means2D=torch.zeros(P, 3, requires_grad=True), sh=e,
              colors_precomp=torch.zeros(P, 3), opacities=torch.ones(P, 1), scales=torch.ones(P, 3),
              rotations=torch.ones(P, 4), cov3Ds_precomp=e, raster_settings=st,
              means2D_abs=torch.zeros(P, 3, requires_grad=True), abs_grad=True)
    kw.update(over)
    return kw


def test_operator_refusals_come_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import GaussianRasterizer, _lib
    from mvs_gaussian_splatting_amd.rasterizer import rasterize_gaussians, rasterize_gaussians_fused
    stats = tuple(torch.zeros(5) for _ in range(3))
    with pytest.raises(ValueError, match="densify_stats"):
        rasterize_gaussians(**_cpu_call(densify_stats=stats))
    st = _cpu_call()["raster_settings"]
    with pytest.raises(ValueError, match="camera tensors"):
        rasterize_gaussians(**_cpu_call(raster_settings=st._replace(viewmatrix=torch.eye(4, requires_grad=True))))
    for bad in (None, torch.zeros(5, 2), torch.zeros(4, 3), torch.zeros(5, 3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="means2D_abs"):
            rasterize_gaussians(**_cpu_call(means2D_abs=bad))
    P = 5
    with pytest.raises(ValueError, match="grown / split"):
        rasterize_gaussians_fused(torch.zeros(P, 3, requires_grad=True), torch.zeros(P, 3), torch.zeros(P, 1, 3),
                                  torch.zeros(P, 15, 3), torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 4), st,
                                  _state_key=("grown", P), means2D_abs=torch.zeros(P, 3, requires_grad=True), abs_grad=True)
    # the module: means2D_abs without the switch is a mistake, and the switch without the tensor too
    kw = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1),
              colors_precomp=torch.zeros(P, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4))
    with pytest.raises(ValueError, match="abs_grad=True"):
        GaussianRasterizer(st)(**kw, means2D_abs=torch.zeros(P, 3))
    with pytest.raises(ValueError, match="means2D_abs"):
        GaussianRasterizer(st, abs_grad=True)(**kw)
    # a request that passes every check reaches the "no CPU path" error, not a fall-back
    with pytest.raises(_lib.GsrError, match="ROCm GPU"):
        rasterize_gaussians(**_cpu_call())


def _plain_model(P=6):
    m = types.SimpleNamespace()
    m._xyz = torch.zeros(P, 3)
    m._features_dc, m._features_rest = torch.zeros(P, 1, 3), torch.zeros(P, 15, 3)
    m._opacity, m._scaling, m._rotation = torch.zeros(P, 1), torch.zeros(P, 3), torch.zeros(P, 4)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P)
    m.percent_dense = 0.01
    return m


def test_densify_and_trainer_refusals():
    from mvs_gaussian_splatting_amd.densify import densify_and_prune
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, PipelineParams, training_iteration
    opt = OptimizationParams()
    assert opt.abs_grad is False and opt.densify_abs_grad_threshold == 0.0008
    assert OptimizationParams(abs_grad=True, densify_abs_grad_threshold=0.001).densify_abs_grad_threshold == 0.001
    m = _plain_model()
    with pytest.raises(ValueError, match="xyz_gradient_accum_abs"):       # no accumulator
        densify_and_prune(m, 0.0002, 0.005, 1.0, None, abs_grad_threshold=0.0008)
    m.xyz_gradient_accum_abs = torch.zeros(3, 1)                          # wrong row count
    with pytest.raises(ValueError, match="xyz_gradient_accum_abs"):
        densify_and_prune(m, 0.0002, 0.005, 1.0, None, abs_grad_threshold=0.0008)
    fork = _plain_model()
    fork.grow_dir = True
    fork.xyz_gradient_accum_abs = torch.zeros(6, 1)
    with pytest.raises(ValueError, match="fork"):
        densify_and_prune(fork, 0.0002, 0.005, 1.0, None, abs_grad_threshold=0.0008, opt=opt, iteration=1)
    bg = torch.zeros(3)
    with pytest.raises(ValueError, match="mcmc"):
        training_iteration(_plain_model(), None, OptimizationParams(abs_grad=True, strategy="mcmc", cap_max=10),
                           PipelineParams(), bg, 1, cameras_extent=1.0)
    with pytest.raises(ValueError, match="fork"):
        training_iteration(fork, None, OptimizationParams(abs_grad=True), PipelineParams(), bg, 1, cameras_extent=1.0)
    with pytest.raises(ValueError, match="fork"):
        training_iteration(_plain_model(), None, OptimizationParams(abs_grad=True), PipelineParams(), bg, 1,
                           cameras_extent=1.0, dataset=types.SimpleNamespace(learn_split_scale=True))
    with pytest.raises(ValueError, match="pose_optimizer"):
        training_iteration(_plain_model(), None, OptimizationParams(abs_grad=True), PipelineParams(), bg, 1,
                           cameras_extent=1.0, pose_optimizer=object())


def test_add_densification_stats_needs_the_backward_and_a_gpu():
    from mvs_gaussian_splatting_amd import _lib
    from mvs_gaussian_splatting_amd.losses import add_densification_stats
    m = _plain_model()
    vs, va = torch.zeros(6, 3, requires_grad=True), torch.zeros(6, 3, requires_grad=True)
    vs.grad = torch.zeros(6, 3)
    with pytest.raises(ValueError, match="viewspace_points_abs has no .grad"):
        add_densification_stats(m, vs, torch.zeros(6, dtype=torch.int32), viewspace_abs=va)
    va.grad = torch.zeros(6, 3)
    with pytest.raises(_lib.GsrError, match="ROCm GPU"):
        add_densification_stats(m, vs, torch.zeros(6, dtype=torch.int32), viewspace_abs=va)
    assert getattr(m, "xyz_gradient_accum_abs", None) is None, "nothing is created on a refused call"


def test_layout_keeps_the_accumulator_in_step():
    from mvs_gaussian_splatting_amd.layout import prune_points_, reorder_gaussians_
    m = _plain_model()
    m._xyz = torch.arange(18, dtype=torch.float32).reshape(6, 3)
    m.xyz_gradient_accum_abs = torch.arange(6, dtype=torch.float32).reshape(6, 1)
    perm = torch.tensor([5, 3, 1, 0, 2, 4])
    reorder_gaussians_(m, perm)
    assert torch.equal(m.xyz_gradient_accum_abs[:, 0], perm.float()) and torch.equal(m._xyz[:, 0], 3.0 * perm.float())
    prune_points_(m, torch.tensor([True, False, True, True, False, False]))
    assert torch.equal(m.xyz_gradient_accum_abs[:, 0], torch.tensor([5.0, 1.0, 0.0]))
    # a model without the accumulator stays without it
    m2 = _plain_model()
    prune_points_(m2, torch.tensor([True, False, True, True, False, False]))
    assert getattr(m2, "xyz_gradient_accum_abs", None) is None
