"""CPU-side checks of the depth-distortion map (csrc/distortion.hip; rasterizer ``distortion=``): the
restatement the GPU tests compare against (tests/distortion_restate.py), what the float32 moments form would lose, the
ABI that carries the map, and the refusals, which all come before a GPU is asked for."""
import ctypes as C
import functools
import os
import re
import types

import pytest
import torch

from conftest import ROOT, make_settings, small_scene
from distortion_restate import (distortion_from_lists, mapped_depth, moments_from_lists, slab_model)
from grad_util import MARGIN, TOL, oracle_operator_inputs

SMALL = dict(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2)


@functools.lru_cache(maxsize=None)
def _frame(dtype, slab=False):
    """The oracle's frame of the `small` scene of test_gpu_distortion.py (or its slab): (pre, lists, settings, aux)."""
    from oracle import rasterize_ref
    model, cam, bg, _ = small_scene(**SMALL)
    if slab:
        slab_model(model)
    st = make_settings(cam, bg, 3)
    _, xyz, m2, op, kw = oracle_operator_inputs(model, dtype)
    with torch.no_grad():
        _, _, aux = rasterize_ref(xyz, m2, op, st, want_aux=True, want_margin=True, **kw)
    return aux["pre"], (aux["point_list"], aux["ranges"], aux["n_contrib"]), st, aux


@pytest.mark.parametrize("mapping", ["linear", "ndc"])
def test_restatement_equals_the_moments_form_in_float64(mapping):
    pre, lists, st, aux = _frame(torch.float64)
    dist = distortion_from_lists(pre, *lists, st, mapping)
    A, M1, M2 = moments_from_lists(pre, *lists, st, mapping)
    assert dist.dtype == torch.float64 and tuple(dist.shape) == (1, 40, 72)
    assert int((aux["n_contrib"] > 1).sum()) > 500 and float(dist.max()) > 0.0
    # A M2 - M1^2 cancels (m / spread)^2 2^-53 of its value: ~1e-12 here
    assert float((A * M2 - M1 * M1 - dist).abs().max()) <= 1e-10 * float(dist.max())
    assert float(dist.min()) >= 0.0 and float(dist[0][aux["n_contrib"] <= 1].abs().sum()) == 0.0


def _tiny_pre(z, dtype=torch.float64):
    """Three Gaussians over one 16x16 tile, all in the tile's list, with view depths ``z``."""
    n = len(z)
    pre = {"v_xy": torch.tensor([[7.0, 8.0], [9.0, 7.5], [8.0, 9.0]], dtype=dtype)[:n],
           "v_conic": torch.tensor([[0.05, 0.01, 0.04]], dtype=dtype).repeat(n, 1),
           "v_opacity": torch.tensor([0.6, 0.5, 0.7], dtype=dtype)[:n], "v_depth": torch.as_tensor(z, dtype=dtype),
           "grid": (1, 1), "radii": torch.ones(n, dtype=torch.int64), "idx": torch.arange(n)}
    st = types.SimpleNamespace(image_height=16, image_width=16)
    import numpy as np
    return pre, (np.arange(n), np.array([[0, n]]), torch.full((16, 16), n)), st


@pytest.mark.parametrize("mapping", ["linear", "ndc"])
def test_autograd_gradients_match_central_differences(mapping):
    pre, lists, st = _tiny_pre([2.0, 2.5, 3.5])
    wts = torch.rand(1, 16, 16, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2 - 1
    names = ("v_depth", "v_opacity", "v_xy", "v_conic")

    def loss(values):
        return (distortion_from_lists(dict(pre, **dict(zip(names, values))), *lists, st, mapping) * wts).sum()
    leaves = [pre[k].clone().requires_grad_(True) for k in names]
    grads = torch.autograd.grad(loss(leaves), leaves)
    for i, (k, g) in enumerate(zip(names, grads)):
        assert float(g.abs().max()) > 0.0, k
        flat = pre[k].reshape(-1)
        for j in range(flat.numel()):
            h = 1e-6
            vals = []
            for sgn in (1.0, -1.0):
                moved = [pre[n].clone() for n in names]
                moved[i].reshape(-1)[j] += sgn * h
                vals.append(float(loss(moved)))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - float(g.reshape(-1)[j])) <= 1e-6 * float(g.abs().max()) + 1e-9, (k, j, fd, float(g.reshape(-1)[j]))


def test_a_pixel_with_one_contributor_is_exactly_zero_and_linear_is_shift_invariant():
    pre, lists, st = _tiny_pre([2.0])
    for mapping in ("linear", "ndc"):
        assert float(distortion_from_lists(pre, *lists, st, mapping).abs().max()) == 0.0
    pre, lists, st = _tiny_pre([2.0, 2.5, 3.5])
    base = distortion_from_lists(pre, *lists, st, "linear")
    # a shift by a power of two keeps every difference of these depths exact: the map is the same bits
    moved = distortion_from_lists(dict(pre, v_depth=pre["v_depth"] + 4.0), *lists, st, "linear")
    assert float(base.max()) > 0.0 and torch.equal(base, moved)
    moved = distortion_from_lists(dict(pre, v_depth=pre["v_depth"] + 0.3), *lists, st, "linear")
    assert float((base - moved).abs().max()) <= 1e-14 * float(base.max())
    assert not torch.equal(distortion_from_lists(pre, *lists, st, "ndc"),
                           distortion_from_lists(dict(pre, v_depth=pre["v_depth"] + 4.0), *lists, st, "ndc"))
    assert float(mapped_depth(torch.tensor(0.2), "ndc")) == 0.0
    assert abs(float(mapped_depth(torch.tensor(100.0, dtype=torch.float64), "ndc")) - 1.0) <= 1e-15


def test_the_float32_moments_form_fails_on_the_slab_by_far_more_than_the_gpu_bar():
    """The `slab` scene of test_gpu_distortion.py (every view depth in 5 +- 0.005, mapping "linear").  The GPU test's bar
    is max(1e-5, 2 x the float32 restatement's error); the float32 moments form A M2 - M1^2 misses the float64 map by more
    than 10 x that.  Observed on the oracle: float32 pairwise restatement 1.1e-6 of the map's maximum (bar 1e-5), float32
    moments 0.94 of it -- a ratio of 9e4: the moments form has no correct digit where the loss converges."""
    pre64, lists64, st, aux = _frame(torch.float64, slab=True)
    pre32, lists32, _, _ = _frame(torch.float32, slab=True)
    z = pre64["v_depth"]
    assert 4.9949 <= float(z.min()) and float(z.max()) <= 5.0051
    robust = aux["margin"] > MARGIN
    truth = distortion_from_lists(pre64, *lists64, st, "linear")[0]
    scale = float(truth[robust].max())
    pairs32 = distortion_from_lists(pre32, *lists32, st, "linear")[0].double()
    A, M1, M2 = moments_from_lists(pre32, *lists32, st, "linear")
    moments32 = (A * M2 - M1 * M1)[0].double()
    e_pairs = float((pairs32 - truth)[robust].abs().max()) / scale
    e_moments = float((moments32 - truth)[robust].abs().max()) / scale
    bar = max(TOL, 2.0 * e_pairs)
    print(f"[distortion slab] float32 pairwise {e_pairs:.2e} (bar {bar:.2e}), float32 moments {e_moments:.2e}: "
          f"ratio {e_moments / bar:.1f}")
    assert scale > 0.0 and e_moments > 10.0 * bar


def test_library_exports_the_entry_points_and_the_three_abi_versions_say_29():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_distortion_forward", "gsr_distortion_backward", "gsr_distortion_backward_bytes"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 29
    assert lib.gsr_distortion_backward_bytes(1000) >= 1000 * 8 * 4


def test_abi_argument_checks_come_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    BADARG, ALIGN = -1, -3
    buf = (C.c_float * 256)()
    ptr = (C.addressof(buf) + 255) & ~255          # host memory: never dereferenced, the checks come first
    frame = _lib.GsrAuxFrame()
    frame.P, frame.width, frame.height, frame.binning_mode = 4, 16, 16, _lib.BINNING_TWO_LEVEL
    frame.num_rendered, frame.num_visible = 8, 4
    frame.img_ws = frame.geom_ws = frame.bin_ws = frame.radii = ptr
    fwd = lib.gsr_distortion_forward
    assert fwd(None, 1, 0.2, 100.0, ptr, ptr, None) == BADARG
    for mapping in (-1, 2):
        assert fwd(C.byref(frame), mapping, 0.2, 100.0, ptr, ptr, None) == BADARG
    for near, far in ((0.0, 100.0), (-1.0, 100.0), (2.0, 1.0), (1.0, 1.0), (0.2, float("inf")), (float("nan"), 100.0),
                      (0.2, float("nan"))):
        assert fwd(C.byref(frame), 1, near, far, ptr, ptr, None) == BADARG, (near, far)
    assert fwd(C.byref(frame), 1, 0.2, 100.0, None, ptr, None) == BADARG
    assert fwd(C.byref(frame), 1, 0.2, 100.0, ptr, None, None) == BADARG
    assert fwd(C.byref(frame), 0, 0.2, 100.0, None, None, None) == BADARG

    params = _lib.GsrParams()
    params.P, params.width, params.height = 4, 16, 16
    params.means3D = params.opacities = params.viewmatrix = params.projmatrix = ptr
    params.scales = params.rotations = ptr
    grads = _lib.GsrAuxGrads(ptr, ptr, ptr, ptr, ptr, None)
    nbytes = lib.gsr_distortion_backward_bytes(4)
    bwd = lib.gsr_distortion_backward
    good = [C.byref(params), C.byref(frame), 1, 0.2, 100.0, ptr, ptr, ptr, nbytes, C.byref(grads), None]

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        return bwd(*args)
    assert call(a0=None) == BADARG and call(a1=None) == BADARG and call(a9=None) == BADARG
    assert call(a2=2) == BADARG and call(a2=-1) == BADARG
    assert call(a3=0.0) == BADARG and call(a4=0.1) == BADARG and call(a4=float("inf")) == BADARG
    assert call(a5=None) == BADARG and call(a6=None) == BADARG and call(a7=None) == BADARG
    assert call(a8=nbytes - 1) == BADARG, "a short workspace"
    assert call(a7=ptr + 16) == ALIGN
    params.forward_only = 1
    assert call() == BADARG
    params.forward_only = 0
    no_out = _lib.GsrAuxGrads(None, ptr, ptr, ptr, ptr, None)
    assert call(a9=C.byref(no_out)) == BADARG


def _cpu_call(distortion, densify_stats=None, view_grad=False):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    if view_grad:
        st = st._replace(viewmatrix=cam.world_view_transform.clone().requires_grad_(True))
    return GaussianRasterizer(st, distortion=distortion)(
        means3D=model.get_xyz, means2D=None, opacities=model.get_opacity, shs=model.get_features,
        scales=model.get_scaling, rotations=model.get_rotation,
        **({} if densify_stats is None else {"densify_stats": densify_stats}))


@pytest.mark.parametrize("bad", [
    dict(mapping="log"), dict(mapping=1), dict(mapping="ndc", near=0.0), dict(mapping="ndc", near=2.0, far=1.0),
    dict(mapping="ndc", far=float("inf")), dict(mapping="ndc", near=float("nan")), dict(maping="ndc"), "ndc", 1,
], ids=["unknown name", "integer mapping", "near 0", "far < near", "far inf", "near nan", "unknown key", "a string", "an int"])
def test_malformed_requests_raise_without_a_gpu(bad):
    with pytest.raises(ValueError, match="distortion"):
        _cpu_call(bad)


def test_refusals_of_aux_maps_are_made_for_distortion_too_without_a_gpu():
    from mvs_gaussian_splatting_amd.rasterizer import (GaussianRasterizationSettings, _grown_key,
                                                       rasterize_gaussians_fused)
    with pytest.raises(ValueError, match="camera"):
        _cpu_call(True, view_grad=True)
    with pytest.raises(ValueError, match="densify_stats"):
        _cpu_call(dict(mapping="linear"), densify_stats=tuple(torch.zeros(12) for _ in range(3)))
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    with pytest.raises(ValueError, match="grown"):
        rasterize_gaussians_fused(model._xyz, None, model._features_dc, model._features_rest, model._opacity,
                                  model._scaling, model._rotation, st, _state_key=_grown_key(10), distortion=True)


def test_render_and_trainer_refusals_without_a_gpu(monkeypatch):
    from mvs_gaussian_splatting_amd import grow, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    with pytest.raises(ValueError, match="return_distortion"):
        render(cam, model, PipelineParams(), bg, distortion_kwargs=dict(mapping="linear"))
    with pytest.raises(ValueError, match="distortion"):
        render(cam, model, PipelineParams(), bg, return_distortion=True, distortion_kwargs=dict(mapping="log"))
    monkeypatch.setattr(grow, "branch", lambda *a, **k: grow.GROW)
    with pytest.raises(ValueError, match="grow"):
        render(cam, model, PipelineParams(), bg, return_distortion=True)
    monkeypatch.undo()
    assert OptimizationParams.lambda_dist == 0.0 and OptimizationParams.dist_from_iter == 3000
    opt = OptimizationParams(lambda_dist=100.0, dist_from_iter=0)
    with pytest.raises(ValueError, match="pose_optimizer"):
        training_iteration(model, cam, opt, PipelineParams(), bg, 1, cameras_extent=1.0, pose_optimizer=object())
    with pytest.raises(ValueError, match="grow / learned-split"):
        training_iteration(model, cam, opt, PipelineParams(), bg, 1, cameras_extent=1.0,
                           dataset=types.SimpleNamespace(grow_dir=True))
    # not yet on: the refusals are not made (the iteration goes on to need a model with a schedule)
    late = OptimizationParams(lambda_dist=100.0, dist_from_iter=3000)
    with pytest.raises(AttributeError):
        training_iteration(model, cam, late, PipelineParams(), bg, 1, cameras_extent=1.0, pose_optimizer=object())


def test_the_plain_call_signature_is_what_it_was():
    """Without ``distortion`` the CPU call reaches the operator's GPU requirement as before (no new refusal in its way)."""
    from mvs_gaussian_splatting_amd import _lib
    with pytest.raises(_lib.GsrError, match="GPU"):
        _cpu_call(None)
    with pytest.raises(_lib.GsrError, match="GPU"):
        _cpu_call(False)
