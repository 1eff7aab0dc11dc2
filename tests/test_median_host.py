"""CPU-side checks of the median-depth map (csrc/median.hip; rasterizer ``median_depth=``): the
restatement the GPU tests compare against (tests/median_restate.py) and what its scenes exercise, the consumers' plain
torch side (``surface_depth``, the ``depth'`` trick, the calls made at ``depth_ratio = 0``), the ABI that carries the map,
and the refusals, which all come before a GPU is asked for."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT, make_settings, small_scene
from depth_restate import maps_from_lists
from median_restate import FRAGILE, MAX_LEFT_OUT, median_from_lists, reference, scene


# ---- the restatement ---------------------------------------------------------------------------------------------------
def _tiny_pre(z, opacity=(0.6, 0.5, 0.7), n_contrib=None, dtype=torch.float64):
    """Up to three Gaussians over one 16x16 tile, all in the tile's list, with view depths ``z``."""
    n = len(z)
    pre = {"v_xy": torch.tensor([[7.0, 8.0], [9.0, 7.5], [8.0, 9.0]], dtype=dtype)[:n],
           "v_conic": torch.tensor([[0.05, 0.01, 0.04]], dtype=dtype).repeat(n, 1),
           "v_opacity": torch.tensor(opacity, dtype=dtype)[:n], "v_depth": torch.as_tensor(z, dtype=dtype),
           "grid": (1, 1), "radii": torch.ones(n, dtype=torch.int64), "idx": torch.arange(n)}
    st = types.SimpleNamespace(image_height=16, image_width=16)
    nc = torch.full((16, 16), n) if n_contrib is None else n_contrib
    return pre, (np.arange(n), np.array([[0, n]]), nc), st


def test_the_median_is_the_depth_of_a_composited_entry_on_the_scenes():
    for name in ("small", "behind"):
        ref = reference(name)
        r64, covered, aux = ref[torch.float64], ref["covered"], ref["aux"]
        gid, pos, med = r64["id"], r64["pos"], r64["median"][0]
        assert bool((gid[covered] >= 0).all()) and bool((gid[~covered] == -1).all())
        assert float(med[~covered].abs().sum()) == 0.0 and bool((pos[~covered] == -1).all())
        assert bool((pos[covered] < aux["n_contrib"].long()[covered]).all()), "the median sits inside the composited prefix"
        slot_of = torch.full((int(ref["radii"].shape[0]),), -1, dtype=torch.int64)
        slot_of[ref["slots"]] = torch.arange(ref["slots"].shape[0])
        assert bool((slot_of[gid[covered]] >= 0).all()) and bool((ref["radii"][gid[covered]] > 0).all())
        assert torch.equal(med[covered], ref["v_depth"][slot_of[gid[covered]]]), "the median is the z of the chosen entry"
        # the list entry at the chosen position of the pixel's tile is that Gaussian
        H, W = covered.shape
        gx = aux["pre"]["grid"][0]
        ys, xs = torch.nonzero(covered, as_tuple=True)
        tiles = (ys // 16) * gx + xs // 16
        starts = torch.from_numpy(aux["ranges"][:, 0].astype(np.int64))[tiles]
        plist = torch.from_numpy(np.asarray(aux["point_list"]).astype(np.int64))
        assert torch.equal(plist[starts + pos[covered]], gid[covered])


def test_a_single_opaque_gaussian_gives_its_own_depth_and_an_empty_pixel_gives_nothing():
    nc = torch.ones(16, 16, dtype=torch.int64)
    nc[0, :] = 0                                        # a row the colour pass composited nothing on
    pre, lists, st = _tiny_pre([2.5], opacity=(0.99,), n_contrib=nc)
    med, gid, pos, frag = median_from_lists(pre, *lists, st)
    near = torch.zeros(16, 16, dtype=torch.bool)
    near[5:12, 5:12] = True                             # alpha >= 1/255 there
    assert bool((med[0][near] == 2.5).all()) and bool((gid[near] == 0).all()) and bool((pos[near] == 0).all())
    assert bool((frag[near] == 0.5).all()), "one entry: T = 1 in front of it"
    assert float(med[0][0].abs().sum()) == 0.0 and bool((gid[0] == -1).all()) and bool((pos[0] == -1).all())
    assert bool(torch.isinf(frag[0]).all())


def test_the_rule_is_the_last_entry_in_front_of_which_t_exceeds_one_half():
    # at the first Gaussian's centre: alpha = 0.6 -> T = 0.4 behind it, so the first entry is the median whatever follows
    pre, lists, st = _tiny_pre([2.0, 2.5, 3.5])
    med, gid, pos, _ = median_from_lists(pre, *lists, st)
    assert float(med[0, 8, 7]) == 2.0 and int(gid[8, 7]) == 0
    # faint entries: T stays above one half to the end, the median is the last composited entry
    pre, lists, st = _tiny_pre([2.0, 2.5, 3.5], opacity=(0.1, 0.1, 0.1))
    med, gid, pos, _ = median_from_lists(pre, *lists, st)
    assert float(med[0, 8, 8]) == 3.5 and int(gid[8, 8]) == 2 and int(pos[8, 8]) == 2
    # the list order decides, not the depth order
    pre, lists, st = _tiny_pre([3.5, 2.0, 2.5], opacity=(0.1, 0.1, 0.1))
    assert float(median_from_lists(pre, *lists, st)[0][0, 8, 8]) == 2.5


def test_the_gradient_equals_central_differences_away_from_fragile_pixels():
    pre, lists, st = _tiny_pre([2.0, 2.5, 3.5])
    wts = torch.rand(1, 16, 16, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2 - 1
    base = median_from_lists(pre, *lists, st)
    assert len(torch.unique(base[1])) >= 3, "the tile must have pixels of several medians"
    wts = wts * (base[3] >= 1e-3)[None]
    names = ("v_depth", "v_opacity", "v_xy", "v_conic")

    def loss(values):
        return (median_from_lists(dict(pre, **dict(zip(names, values))), *lists, st)[0] * wts).sum()
    leaves = [pre[k].clone().requires_grad_(True) for k in names]
    grads = torch.autograd.grad(loss(leaves), leaves, allow_unused=True)
    assert float(grads[0].abs().min()) > 0.0 and all(g is None for g in grads[1:]), "only the depths carry a gradient"
    for i, k in enumerate(names):
        flat = pre[k].reshape(-1)
        for j in range(flat.numel()):
            h = 1e-6
            vals = []
            for sgn in (1.0, -1.0):
                moved = [pre[n].clone() for n in names]
                moved[i].reshape(-1)[j] += sgn * h
                vals.append(float(loss(moved)))
            fd = (vals[0] - vals[1]) / (2 * h)
            want = 0.0 if grads[i] is None else float(grads[i].reshape(-1)[j])
            assert abs(fd - want) <= 1e-6 * float(grads[0].abs().max()) + 1e-9, (k, j, fd, want)


def test_the_scenes_exercise_what_can_go_wrong():
    """On the reference alone (figures as measured: the left-out shares 0.0024 / 0.0044 / 0.0086; 2515 of 2880 pixels of
    `small` cross one half; in `big` 247 ids are the median of pixels in more than one tile and one id is chosen by 2991
    pixels; in `faint` about 3340 kept pixels have their median at list position >= 256, at most 461; in `big` at most 147)."""
    refs = {name: reference(name) for name in ("small", "big", "faint")}
    for name, ref in refs.items():
        assert ref["left_out"] <= MAX_LEFT_OUT
        r64, r32 = ref[torch.float64], ref[torch.float32]
        assert torch.equal(r64["id"][ref["covered"]], r32["id"][ref["covered"]]), f"{name}: float32 picks another id"
        assert bool((ref["frag"][ref["keep"]] >= FRAGILE).all())
    small = refs["small"]
    model, cam, bg = scene("small")
    aux = small["aux"]
    with torch.no_grad():
        alpha = maps_from_lists(aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], make_settings(cam, bg, 3))[2]
    crosses = (1.0 - alpha) <= 0.5
    n_cross, n_cov = int((crosses & small["covered"]).sum()), int(small["covered"].sum())
    print(f"[median scenes] small: {n_cross} of {n_cov} covered pixels cross one half")
    assert 0 < n_cross < n_cov
    big = refs["big"]
    gid, covered = big[torch.float64]["id"], big["covered"]
    ys, xs = torch.nonzero(covered, as_tuple=True)
    gx = big["aux"]["pre"]["grid"][0]
    pairs = torch.unique(torch.stack((gid[covered], (ys // 16) * gx + xs // 16), dim=1), dim=0)
    tiles_per_id = torch.unique(pairs[:, 0], return_counts=True)[1]
    pixels_per_id = torch.unique(gid[covered], return_counts=True)[1]
    print(f"[median scenes] big: {int((tiles_per_id > 1).sum())} ids are the median in more than one tile; one id is chosen "
          f"by {int(pixels_per_id.max())} pixels; largest kept position {int(big[torch.float64]['pos'][big['keep']].max())}")
    assert int((tiles_per_id > 1).sum()) > 0 and int(pixels_per_id.max()) > 1000
    assert int(big[torch.float64]["pos"][big["keep"]].max()) < 256, "plain `big` never leaves the first round"
    faint = refs["faint"]
    pos = faint[torch.float64]["pos"][faint["keep"]]
    print(f"[median scenes] faint: {int((pos >= 256).sum())} kept pixels have their median at list position >= 256, "
          f"largest {int(pos.max())}")
    assert int((pos >= 256).sum()) > 1000


# ---- consumers: plain torch ------------------------------------------------------------------------------------------------
def _maps(seed=5):
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand(1, 6, 7, generator=g)
    alpha[0, 0, :3] = torch.tensor([0.0, 0.49, 0.5])
    depth = alpha * (2.0 + torch.rand(1, 6, 7, generator=g))
    median = 2.0 + torch.rand(1, 6, 7, generator=g)
    return depth, alpha, median


def test_surface_depth_at_both_ends_and_between():
    from mvs_gaussian_splatting_amd import surface_depth
    depth, alpha, median = _maps()
    today = torch.where(alpha >= 0.5, depth / alpha, torch.zeros_like(depth))        # tsdf.fuse_views as it was
    assert torch.equal(surface_depth(depth, alpha, median, 0.0), today)
    assert torch.equal(surface_depth(depth, alpha, None, 0.0), today)
    at_one = surface_depth(depth, alpha, median, 1.0)
    assert torch.equal(at_one, torch.where(alpha >= 0.5, median, torch.zeros_like(depth)))
    assert float(at_one[0, 0, 0]) == 0.0 and float(at_one[0, 0, 1]) == 0.0 and float(at_one[0, 0, 2]) == float(median[0, 0, 2])
    half = surface_depth(depth, alpha, median, 0.5, alpha_min=0.25)
    want = torch.where(alpha >= 0.25, 0.5 * (depth / alpha) + 0.5 * median, torch.zeros_like(depth))
    assert torch.allclose(half, want, rtol=1e-6, atol=0.0) and bool(torch.isfinite(half).all())
    assert torch.equal(surface_depth(depth[0], alpha[0], median, 1.0), at_one[0]), "[H,W] maps with a [1,H,W] median"
    for bad in (-0.1, 1.5, float("nan"), "1"):
        with pytest.raises(ValueError, match="depth_ratio"):
            surface_depth(depth, alpha, median, bad)
    with pytest.raises(ValueError, match="median"):
        surface_depth(depth, alpha, None, 0.5)
    with pytest.raises(ValueError, match="shape"):
        surface_depth(depth, alpha, median[:, :3], 0.5)
    with pytest.raises(TypeError, match="median"):
        surface_depth(depth, alpha, median.double(), 0.5)


def test_the_weighted_blend_is_the_same_tensor_at_ratio_zero_and_divides_to_the_blend():
    from mvs_gaussian_splatting_amd.surface import blend_weighted_depth, surface_depth
    depth, alpha, median = _maps()
    assert blend_weighted_depth(depth, alpha, None, 0.0) is depth
    assert blend_weighted_depth(depth, alpha, median, 0.0) is depth, "r = 0: the tensor passed today, not a copy"
    depth.requires_grad_(True)
    median.requires_grad_(True)
    alpha.requires_grad_(True)
    blended = blend_weighted_depth(depth, alpha, median, 0.7)
    ok = alpha >= 0.5
    assert torch.allclose((blended / alpha)[ok], surface_depth(depth, alpha, median, 0.7)[ok], rtol=1e-6, atol=0.0)
    blended.sum().backward()
    assert torch.allclose(depth.grad, torch.full_like(depth, 0.3)) and torch.allclose(median.grad, 0.7 * alpha.detach())
    assert torch.allclose(alpha.grad, 0.7 * median.detach())
    with pytest.raises(ValueError, match="median"):
        blend_weighted_depth(depth, alpha, None, 0.5)


def test_normal_loss_arguments_are_checked_without_a_gpu():
    from mvs_gaussian_splatting_amd import _lib, depth_to_normals, normal_consistency_loss
    depth, alpha, median = _maps()
    normal = torch.zeros(3, 6, 7)
    with pytest.raises(ValueError, match="depth_ratio"):
        normal_consistency_loss(depth, alpha, normal, 0.5, 0.5, median=median, depth_ratio=2.0)
    with pytest.raises(ValueError, match="median"):
        normal_consistency_loss(depth, alpha, normal, 0.5, 0.5, depth_ratio=0.5)
    with pytest.raises(ValueError, match="shape"):
        depth_to_normals(depth, alpha, 0.5, 0.5, median=median[:, :2], depth_ratio=1.0)
    # accepted: the calls go on to the kernel's GPU requirement, as without the arguments
    for kw in ({}, {"median": median, "depth_ratio": 0.0}, {"median": median, "depth_ratio": 1.0}):
        with pytest.raises(_lib.GsrError, match="GPU"):
            normal_consistency_loss(depth, alpha, normal, 0.5, 0.5, **kw)
        with pytest.raises(_lib.GsrError, match="GPU"):
            depth_to_normals(depth, alpha, 0.5, 0.5, **kw)


class _Volume:
    with_color = False

    def __init__(self):
        self.calls = []

    def integrate(self, depth, camera, color=None, max_depth=None):
        self.calls.append((depth, camera, color, max_depth))


def test_fuse_views_calls_the_renderer_as_before_at_ratio_zero():
    from mvs_gaussian_splatting_amd import fuse_views, surface_depth
    depth, alpha, median = _maps()
    seen = []

    def renderer(*args, **kw):
        seen.append((args, kw))
        return {"depth": depth, "alpha": alpha, "median_depth": median, "render": None}
    today = torch.where(alpha >= 0.5, depth / alpha, torch.zeros_like(depth))
    for kw in ({}, {"depth_ratio": 0.0}):
        seen.clear()
        vol = fuse_views(["cam"], "model", "pipe", "bg", _Volume(), renderer=renderer, **kw)
        assert seen == [(("cam", "model", "pipe", "bg"), {"return_depth": True})], "exactly today's call"
        assert torch.equal(vol.calls[0][0], today)
    seen.clear()
    vol = fuse_views(["cam"], "model", "pipe", "bg", _Volume(), depth_ratio=0.25, alpha_min=0.3, max_depth=9.0,
                     renderer=renderer)
    assert seen == [(("cam", "model", "pipe", "bg"), {"return_depth": True, "return_median_depth": True})]
    assert torch.equal(vol.calls[0][0], surface_depth(depth, alpha, median, 0.25, 0.3)) and vol.calls[0][3] == 9.0
    with pytest.raises(ValueError, match="depth_ratio"):
        fuse_views(["cam"], "model", "pipe", "bg", _Volume(), depth_ratio=1.5, renderer=renderer)


class _Stop(Exception):
    pass


def test_training_iteration_calls_render_as_before_at_ratio_zero(monkeypatch):
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    assert OptimizationParams.depth_ratio == 0.0
    seen = {}

    def render(*args, **kw):
        seen["args"], seen["kw"] = args, kw
        raise _Stop()
    monkeypatch.setattr(trainer, "render", render)
    model = types.SimpleNamespace(update_learning_rate=lambda it: None, oneupSHdegree=lambda: None)
    bg = torch.zeros(3)

    def keywords(opt):
        with pytest.raises(_Stop):
            training_iteration(model, "camera", opt, "pipe", bg, 1, cameras_extent=1.0)
        assert seen["args"][:3] == ("camera", model, "pipe")
        return {k: v for k, v in seen["kw"].items() if k.startswith("return_")}
    normal = dict(lambda_normal=0.05, normal_from_iter=0)
    parent = types.SimpleNamespace(**{k: getattr(OptimizationParams(**normal), k) for k in dir(OptimizationParams)
                                      if not k.startswith("_") and k != "depth_ratio"})
    today = {"return_depth": True, "return_normals": True}
    assert keywords(parent) == today, "options that do not know the field"
    full = dict(seen["kw"])
    assert keywords(OptimizationParams(**normal)) == today
    assert set(seen["kw"]) == set(full), "depth_ratio = 0 adds no keyword argument"
    assert keywords(OptimizationParams(**normal, depth_ratio=1.0)) == dict(today, return_median_depth=True)
    assert keywords(OptimizationParams(depth_ratio=1.0)) == {}, "read only while the normal term is on"
    assert keywords(OptimizationParams(lambda_normal=0.05, normal_from_iter=7000, depth_ratio=1.0)) == {}
    for bad in (-0.5, 1.5):
        with pytest.raises(ValueError, match="depth_ratio"):
            training_iteration(model, "camera", OptimizationParams(**normal, depth_ratio=bad), "pipe", bg, 1,
                               cameras_extent=1.0)
    # the refusals of the normal term stand with the blend
    with pytest.raises(ValueError, match="pose_optimizer"):
        training_iteration(model, "camera", OptimizationParams(**normal, depth_ratio=1.0), "pipe", bg, 1,
                           cameras_extent=1.0, pose_optimizer=object())
    with pytest.raises(ValueError, match="grow / learned-split"):
        training_iteration(model, "camera", OptimizationParams(**normal, depth_ratio=1.0), "pipe", bg, 1,
                           cameras_extent=1.0, dataset=types.SimpleNamespace(grow_dir=True))


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_three_abi_versions_say_30():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_median_depth_forward", "gsr_median_depth_backward", "gsr_median_depth_backward_bytes"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 30
    assert lib.gsr_median_depth_backward_bytes(1000) >= 1000 * 4 and lib.gsr_median_depth_backward_bytes(1000) % 256 == 0
    assert lib.gsr_median_depth_backward_bytes(0) > 0


def test_abi_argument_checks_come_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    BADARG, CAPACITY, ALIGN = -1, -2, -3
    buf = (C.c_float * 256)()
    ptr = (C.addressof(buf) + 255) & ~255          # host memory: never dereferenced, the checks come first
    frame = _lib.GsrAuxFrame()
    frame.P, frame.width, frame.height, frame.binning_mode = 4, 16, 16, _lib.BINNING_TWO_LEVEL
    frame.num_rendered, frame.num_visible = 8, 4
    frame.img_ws = frame.geom_ws = frame.bin_ws = frame.radii = ptr
    fwd = lib.gsr_median_depth_forward
    assert fwd(None, ptr, ptr, ptr, None) == BADARG
    assert fwd(C.byref(frame), None, ptr, ptr, None) == BADARG
    assert fwd(C.byref(frame), ptr, None, ptr, None) == BADARG
    assert fwd(C.byref(frame), ptr, ptr, None, None) == BADARG
    frame.binning_mode = 99
    assert fwd(C.byref(frame), ptr, ptr, ptr, None) == BADARG
    frame.binning_mode = _lib.BINNING_TWO_LEVEL

    params = _lib.GsrParams()
    params.P, params.width, params.height = 4, 16, 16
    params.viewmatrix = ptr
    nbytes = lib.gsr_median_depth_backward_bytes(4)
    bwd = lib.gsr_median_depth_backward
    good = [C.byref(params), C.byref(frame), ptr, ptr, ptr, nbytes, ptr, None]

    def call(**change):
        args = list(good)
        for k, v in change.items():
            args[int(k[1:])] = v
        return bwd(*args)
    assert call(a0=None) == BADARG and call(a1=None) == BADARG
    assert call(a2=None) == BADARG and call(a3=None) == BADARG and call(a4=None) == BADARG and call(a6=None) == BADARG
    assert call(a5=nbytes - 1) == CAPACITY, "a short workspace"
    assert call(a4=ptr + 16) == ALIGN
    params.forward_only = 1
    assert call() == BADARG
    params.forward_only = 0
    params.viewmatrix = None
    assert call() == BADARG
    params.viewmatrix = ptr
    params.width = 32
    assert call() == BADARG, "frame and params disagree"


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _cpu_call(median_depth, densify_stats=None, view_grad=False):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    if view_grad:
        st = st._replace(viewmatrix=cam.world_view_transform.clone().requires_grad_(True))
    return GaussianRasterizer(st, **({"median_depth": median_depth} if median_depth is not None else {}))(
        means3D=model.get_xyz, means2D=None, opacities=model.get_opacity, shs=model.get_features,
        scales=model.get_scaling, rotations=model.get_rotation,
        **({} if densify_stats is None else {"densify_stats": densify_stats}))


def test_refusals_of_aux_maps_are_made_for_the_median_too_without_a_gpu():
    from mvs_gaussian_splatting_amd import _lib
    from mvs_gaussian_splatting_amd.rasterizer import (GaussianRasterizationSettings, _grown_key,
                                                       rasterize_gaussians_fused)
    with pytest.raises(ValueError, match="median_depth=True cannot be combined with camera"):
        _cpu_call(True, view_grad=True)
    with pytest.raises(ValueError, match="median_depth=True cannot be combined with densify_stats"):
        _cpu_call(True, densify_stats=tuple(torch.zeros(12) for _ in range(3)))
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    with pytest.raises(ValueError, match="median_depth=True is not available on a frame with grown"):
        rasterize_gaussians_fused(model._xyz, None, model._features_dc, model._features_rest, model._opacity,
                                  model._scaling, model._rotation, st, _state_key=_grown_key(10), median_depth=True)
    # accepted, and without the map: the CPU call reaches the operator's GPU requirement as before
    for value in (True, False, None):
        with pytest.raises(_lib.GsrError, match="GPU"):
            _cpu_call(value)


def test_render_refuses_the_map_on_a_grown_frame_without_a_gpu(monkeypatch):
    from mvs_gaussian_splatting_amd import grow, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    monkeypatch.setattr(grow, "branch", lambda *a, **k: grow.GROW)
    with pytest.raises(ValueError, match="return_median_depth=True is not available"):
        render(cam, model, PipelineParams(), bg, return_median_depth=True)
