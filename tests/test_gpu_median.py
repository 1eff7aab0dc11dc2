"""The median-depth map and the Gaussian id map of the HIP path (csrc/median.hip; GaussianRasterizer(median_depth=True),
render(return_median_depth=True)) against the float64 restatement of tests/median_restate.py.

Scenes (median_restate.scene; conftest.small_scene):
  small   P = 400 at 72x40: the last tile column and the last tile row are partial; pixels that cross one half and pixels
          that never do;
  big     P = 3000 at 320x176: lists longer than one 256-entry round, one Gaussian the median of thousands of pixels in
          many tiles (the backward's one-atomic-per-tile-and-entry path);
  faint   big with every raw opacity lowered by 4: rays stay above one half for long, medians sit past list position 256
          (the forward's second round, the backward's rounds in front of the chosen one);
  behind  small with Gaussians behind the camera and inside the near plane;
  and a frame without any instance.
What the scenes exercise is asserted on the reference alone in tests/test_median_host.py.

Bars.  A pixel is left out of the oracle comparisons when its float64 oracle margin is at most grad_util.MARGIN or its
float64 fragility min |T_i - 0.5| is below 1e-4 (at most 2 % of the covered pixels, asserted by median_restate.reference).
On the kept pixels the id equals the float64 restatement's exactly, and the median is within max(1e-5, 2 x the float32
restatement's own error) of it relative to the map's maximum (grad_util.TOL, the bar of test_gpu_depth._check_forward);
the gradients go through grad_util.compare_grads.  Every pixel, the left-out ones included, is held to the
oracle-independent checks of test 2.  The observed figures are printed (run with -s).
"""
import math
import os
import sys

import pytest
import torch

from conftest import ROOT, small_scene
from gpu_util import product_settings
from grad_util import MARGIN, TOL, compare_grads, linear_weights, weighted_sum
from depth_restate import assert_rounds_covered
from median_restate import BEHIND, SCENES, median_loss, median_weights, reference, scene

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu

GEOMETRY = ("opacity", "means2D", "scaling", "rotation")


def _hip_leaves(dev, model, use_cov):
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.detach().to(dev).requires_grad_(True)
        return leaves[name]

    xyz, op = leaf("xyz", model._xyz), leaf("opacity", model._opacity)
    leaves["means2D"] = torch.zeros(xyz.shape[0], 3, device=dev, requires_grad=True)
    fdc, fr = leaf("f_dc", model._features_dc), leaf("f_rest", model._features_rest)
    kw = {"shs": torch.cat((fdc, fr), dim=1)}
    if use_cov:
        kw["cov3D_precomp"] = leaf("cov3D", model.get_covariance(1.0))
    else:
        kw["scales"] = torch.exp(leaf("scaling", model._scaling))
        kw["rotations"] = torch.nn.functional.normalize(leaf("rotation", model._rotation))
    return leaves, dict(means3D=xyz, means2D=leaves["means2D"], opacities=torch.sigmoid(op), **kw)


def _hip(dev, name, use_cov=False, median_depth=True, **ctor):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    model, cam, bg = scene(name)
    st = product_settings(cam, bg, 3, dev)
    leaves, kw = _hip_leaves(dev, model, use_cov)
    if median_depth:
        ctor["median_depth"] = True
    return leaves, GaussianRasterizer(st, **ctor)(**kw)


def _n_contrib(dev, color, H, W):
    from mvs_gaussian_splatting_amd import _lib
    img = color.grad_fn.saved_tensors[-1]
    out = torch.empty(H, W, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gsr_debug_read_image(img.data_ptr(), W, H, None, out.data_ptr(), None,
                                                torch.cuda.current_stream(dev).cuda_stream), "read_img")
    torch.cuda.synchronize(dev)
    return out.cpu()


def _check_maps(median, median_id, ref, label):
    r64, r32 = ref[torch.float64], ref[torch.float32]
    keep, covered = ref["keep"], ref["covered"]
    H, W = keep.shape
    assert tuple(median.shape) == (1, H, W) and median.dtype == torch.float32
    assert tuple(median_id.shape) == (H, W) and median_id.dtype == torch.int32
    got, gid = median.detach().cpu().double()[0], median_id.cpu().long()
    wrong = int((gid != r64["id"])[keep].sum())
    scale = float(r64["median"][0][keep].abs().max())
    e = float((got - r64["median"][0])[keep].abs().max()) / scale
    e32 = float((r32["median"][0].double() - r64["median"][0])[keep].abs().max()) / scale
    bar = max(TOL, 2.0 * e32)
    print(f"[median forward] {label}: {int(keep.sum())} kept pixels, {wrong} ids differ; median err {e:.2e} (float32 "
          f"restatement {e32:.2e}, bar {bar:.2e}); ids differ on {int((gid != r64['id'])[covered & ~keep].sum())} of the "
          f"{int((covered & ~keep).sum())} pixels left out")
    assert wrong == 0, f"{label}: median_id differs from the float64 restatement on {wrong} kept pixels"
    assert e <= bar, f"{label}: the median map is {e:.2e} off the float64 restatement, bar {bar:.2e}"
    empty = ~covered & (ref["aux"]["margin"] > MARGIN)
    if bool(empty.any()):
        assert float(got[empty].abs().max()) == 0.0 and bool((gid[empty] == -1).all()), "an uncovered pixel is not 0 / -1"


def _median_grads(leaves, median, weights):
    names = tuple(leaves)
    got = torch.autograd.grad(median_loss(median, weights), [leaves[k] for k in names], allow_unused=True)
    return dict(zip(names, got))


def _check_grads(leaves, median, ref, label, behind=False):
    g64, g32 = ref[torch.float64]["grads"], ref[torch.float32]["grads"]
    got = _median_grads(leaves, median, ref["weights"])
    assert got["xyz"] is not None and float(got["xyz"].abs().max()) > 0.0
    compare_grads({"xyz": got["xyz"].cpu()}, {"xyz": g64["xyz"]}, {"xyz": g32["xyz"]}, f"median depth, {label}")
    for k, g in got.items():
        if k != "xyz":
            assert g is None or float(g.abs().max()) == 0.0, f"{label}: {k} received a gradient from the median map"
            assert g64[k] is None, f"the restatement has a gradient for {k}"
    if behind:
        assert float(got["xyz"][list(BEHIND)].abs().max()) == 0.0, "a Gaussian behind the camera received a gradient"


@pytest.mark.parametrize("name,use_cov", [("small", False), ("big", False), ("faint", False), ("behind", False),
                                          ("small", True), ("stacked", False)])
def test_id_median_and_gradient_match_the_float64_restatement(gpu_device, name, use_cov):
    """Tests 1 and 3 of the issue: the two maps on the kept pixels, uncovered pixels exactly 0 / -1, dL/dxyz of
    sum(weights * median) at the bar of compare_grads, every other leaf without a gradient."""
    ref = reference(name, use_cov)
    if name == "stacked":
        assert_rounds_covered(ref["aux"], ref[torch.float64]["pos"])
    label = name + (", cov3D_precomp" if use_cov else "")
    leaves, (color, radii, median, median_id) = _hip(gpu_device, name, use_cov)
    assert torch.equal(radii.cpu(), ref["radii"].to(torch.int32))
    assert not median_id.requires_grad and median.requires_grad
    _check_maps(median, median_id, ref, label)
    _check_grads(leaves, median, ref, label, behind=name == "behind")


@pytest.mark.parametrize("name", ["small", "big", "faint", "behind"])
def test_every_pixel_names_a_visible_gaussian_and_carries_its_view_depth(gpu_device, name):
    """Test 2: oracle-independent, on every pixel, the left-out ones included."""
    model, cam, bg = scene(name)
    H, W = SCENES["small" if name in ("small", "behind") else "big"]["height"], \
        SCENES["small" if name in ("small", "behind") else "big"]["width"]
    _, (color, radii, median, median_id) = _hip(gpu_device, name)
    gid, med, rad = median_id.cpu().long(), median.detach().cpu().double()[0], radii.cpu()
    has = gid >= 0
    assert bool((gid >= -1).all()) and bool((gid < rad.numel()).all())
    assert bool((rad[gid[has]] > 0).all()), "median_id names a Gaussian with radii == 0"
    V = cam.world_view_transform.double()
    z = model._xyz.double() @ V[:3, 2] + V[3, 2]
    err = float(((med[has] - z[gid[has]]).abs() / z[gid[has]].abs()).max())
    print(f"[median every pixel] {name}: {int(has.sum())} pixels with a median, view-depth error {err:.2e}")
    assert err <= 1e-5
    assert float(med[~has].abs().max() if bool((~has).any()) else 0.0) == 0.0
    assert torch.equal(has, _n_contrib(gpu_device, color, H, W) > 0), "median_id >= 0 must hold exactly where n_contrib > 0"


def test_the_colour_path_the_depth_maps_and_the_distortion_map_are_left_alone(gpu_device):
    """Test 4: colour, radii, aux, dist and every colour gradient with and without the map, bit for bit."""
    name = "small"
    H, W = SCENES[name]["height"], SCENES[name]["width"]
    wts = linear_weights((3, H, W))
    names = ("xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation", "means2D")
    runs = []
    for on in (True, False):
        leaves, out = _hip(gpu_device, name, median_depth=on, aux_maps=True, distortion=True)
        cg = torch.autograd.grad(weighted_sum(out[0], wts), [leaves[k] for k in names], retain_graph=True)
        runs.append((out, cg))
    (o1, c1), (o0, c0) = runs
    assert len(o0) == 4 and len(o1) == 6 and tuple(o1[4].shape) == (1, H, W) and tuple(o1[5].shape) == (H, W)
    for i, what in enumerate(("colour", "radii", "aux", "dist")):
        assert torch.equal(o1[i], o0[i]), f"{what} changed with median_depth=True"
    for k, a, b in zip(names, c1, c0):
        assert torch.equal(a, b), f"colour gradient of {k} changed with median_depth=True"
    plain = _hip(gpu_device, name, median_depth=False)[1]
    assert len(plain) == 2 and torch.equal(plain[0], o1[0])


def test_the_maps_are_reproducible_bit_for_bit_on_every_path(gpu_device):
    """Test 5: run to run, with and without requires_grad, render(return_median_depth=True) against the operator on the
    same raw parameters, and the fused raw-parameter path; the gradients of two runs agree at the scene's bar."""
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.rasterizer import rasterize_gaussians_fused
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    name = "big"
    ref = reference(name)
    l1, o1 = _hip(gpu_device, name)
    l2, o2 = _hip(gpu_device, name)
    assert torch.equal(o1[2], o2[2]) and torch.equal(o1[3], o2[3]), "the maps of two runs differ"
    with torch.no_grad():
        _, o3 = _hip(gpu_device, name)
    assert len(o3) == 4 and not o3[2].requires_grad
    assert torch.equal(o3[2], o1[2]) and torch.equal(o3[3], o1[3]) and torch.equal(o3[0], o1[0]), "no_grad differs"
    g64, g32 = ref[torch.float64]["grads"]["xyz"], ref[torch.float32]["grads"]["xyz"]
    ga = _median_grads(l1, o1[2], ref["weights"])["xyz"].cpu().double()
    gb = _median_grads(l2, o2[2], ref["weights"])["xyz"].cpu().double()
    scale = float(g64.abs().max())
    bar = max(TOL, 2.0 * float((g32.double() - g64).abs().max()) / scale)
    e = float((ga - gb).abs().max()) / scale
    print(f"[median reproducibility] xyz: two runs differ by {e:.2e} (bar {bar:.2e})")
    assert e <= bar

    model, cam, bg = scene("small")
    model.to(gpu_device)
    cam.to(gpu_device)
    for p in model.parameters():
        p.requires_grad_(True)
    pkg = render(cam, model, PipelineParams(), bg.to(gpu_device), return_median_depth=True)
    assert tuple(pkg["median_depth"].shape) == (1, 40, 72) and tuple(pkg["median_id"].shape) == (40, 72)
    assert "depth" not in pkg and pkg["median_id"].dtype == torch.int32
    assert not getattr(pkg["viewspace_points"], "_gsr_stats_fused", False)
    st = product_settings(cam, bg, 3, gpu_device)
    out = rasterize_gaussians_fused(model._xyz, None, model._features_dc, model._features_rest, model._opacity,
                                    model._scaling, model._rotation, st, median_depth=True)
    assert len(out) == 4 and torch.equal(out[0], pkg["render"])
    assert torch.equal(out[2], pkg["median_depth"]) and torch.equal(out[3], pkg["median_id"])
    sref = reference("small")
    _check_maps(pkg["median_depth"], pkg["median_id"], sref, "small, fused")
    median_loss(pkg["median_depth"], sref["weights"]).backward()
    compare_grads({"xyz": model._xyz.grad.cpu()}, {"xyz": sref[torch.float64]["grads"]["xyz"]},
                  {"xyz": sref[torch.float32]["grads"]["xyz"]}, "median depth, small, fused")
    for k in ("_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert getattr(model, k).grad is None, f"{k} received a gradient from the median map"
    assert pkg["viewspace_points"].grad is None
    with torch.no_grad():
        pkg0 = render(cam, model, PipelineParams(), bg.to(gpu_device), return_median_depth=True)
    assert torch.equal(pkg0["median_depth"], pkg["median_depth"]) and torch.equal(pkg0["median_id"], pkg["median_id"])
    assert torch.equal(pkg0["render"], pkg["render"])
    plain = render(cam, model, PipelineParams(), bg.to(gpu_device))
    assert "median_depth" not in plain and torch.equal(plain["render"], pkg["render"])
    every = render(cam, model, PipelineParams(), bg.to(gpu_device), return_depth=True, return_normals=True,
                   return_distortion=True, return_median_depth=True)
    assert torch.equal(every["median_depth"], pkg["median_depth"]) and torch.equal(every["median_id"], pkg["median_id"])
    assert tuple(every["normal"].shape) == (3, 40, 72) and tuple(every["distortion"].shape) == (1, 40, 72)
    assert tuple(every["depth"].shape) == (1, 40, 72)


def test_frame_without_any_instance(gpu_device):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    model, cam, bg = scene("small")
    model._xyz[:, 2] = -model._xyz[:, 2].abs() - 1.0
    st = product_settings(cam, bg, 3, gpu_device)
    for _ in range(2):      # the second frame of the shape is issued whole, into the state of the first
        leaves, kw = _hip_leaves(gpu_device, model, False)
        color, radii, median, median_id = GaussianRasterizer(st, median_depth=True)(**kw)
        assert int((radii > 0).sum()) == 0
        assert tuple(median.shape) == (1, 40, 72) and float(median.detach().abs().max()) == 0.0
        assert tuple(median_id.shape) == (40, 72) and bool((median_id == -1).all())
        got = _median_grads(leaves, median, median_weights(40, 72))
        assert got["xyz"].shape == leaves["xyz"].shape and float(got["xyz"].abs().max()) == 0.0
        for k in GEOMETRY:
            assert got[k] is None or float(got[k].abs().max()) == 0.0, k


PLANE = (0.3, -0.2, 4.0)         # view-space plane z = 4 + 0.3 x - 0.2 y (the scene of test_gpu_normal_consistency.py)


def _plane_problem(dev):
    """A 64x48 frame of 400 flat Gaussians on a tilted plane in front of the example's camera."""
    import train as example
    cams, bg, _ = example.make_problem(dev, P=600, W=64, H=48, n_views=1)
    g = torch.Generator().manual_seed(11)
    xy = (torch.rand(400, 2, generator=g) - 0.5) * torch.tensor([1.5, 1.2])
    view = torch.cat((xy, (PLANE[2] + PLANE[0] * xy[:, :1] + PLANE[1] * xy[:, 1:]), torch.ones(400, 1)), dim=1)
    world = (view.to(dev) @ torch.linalg.inv(cams[0].world_view_transform.float()))[:, :3].contiguous()
    colors = torch.rand(400, 3, generator=g).to(dev)
    return cams, bg, (world, colors)


def test_one_training_iteration_on_the_median_blend(gpu_device, monkeypatch):
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    problem = _plane_problem(gpu_device)
    cams, bg, _ = problem
    opt = example.small_opt(40, lambda_normal=0.05, normal_from_iter=0, depth_ratio=1.0)
    model = example.make_model(problem, opt)
    with torch.no_grad():
        model._opacity.fill_(2.0)
        model._scaling[:, :2] = math.log(0.07)
        model._scaling[:, 2] = math.log(0.004)
    seen, real_render = {}, trainer.render

    def spy(*args, **kw):
        pkg = real_render(*args, **kw)
        seen["kw"] = kw
        pkg["median_depth"].register_hook(lambda g: seen.__setitem__("g", g.detach().clone()))
        return pkg
    monkeypatch.setattr(trainer, "render", spy)
    grads = {}
    real_step = model.optimizer.step

    def step(*a, **k):
        for group in model.optimizer.param_groups:
            grads[group["name"]] = None if group["params"][0].grad is None else group["params"][0].grad.detach().clone()
        return real_step(*a, **k)
    monkeypatch.setattr(model.optimizer, "step", step)
    loss = float(trainer.training_iteration(model, cams[0], opt, PipelineParams(), bg, 1,
                                            cameras_extent=example.CAMERAS_EXTENT))
    print(f"[median trainer] loss {loss:.6f} with lambda_normal = 0.05 on depth_ratio = 1")
    assert seen["kw"].get("return_median_depth") is True and seen["kw"].get("return_depth") is True
    assert math.isfinite(loss)
    assert float(seen["g"].abs().max()) > 0.0, "the normal term sent no gradient into the median map"
    assert grads["xyz"] is not None and bool(torch.isfinite(grads["xyz"]).all()) and float(grads["xyz"].abs().max()) > 0.0
    assert float(model.denom.sum()) > 0, "the densification statistics were not taken"


def test_fuse_views_at_depth_ratio_one_equals_the_hand_filled_volume(gpu_device):
    from mvs_gaussian_splatting_amd import TSDFVolume, fuse_views, render, surface_depth
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    dev = gpu_device
    model, cam0, bg, _ = small_scene(scale=0.08)
    cameras = [cam0.to(dev), small_scene(P=1, view=1)[1].to(dev)]
    model.to(dev)
    bg, pipe = bg.to(dev), PipelineParams()
    make = lambda: TSDFVolume((-2.0, -1.5, 3.0), 0.125, (33, 25, 41), 0.5, device=dev)        # noqa: E731
    fused = fuse_views(cameras, model, pipe, bg, make(), alpha_min=0.5, max_depth=7.5, depth_ratio=1.0)
    by_hand, expected_depth = make(), make()
    differs = 0
    with torch.no_grad():
        for cam in cameras:
            pkg = render(cam, model, pipe, bg, return_depth=True, return_median_depth=True)
            surface = surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], 1.0, 0.5)
            assert torch.equal(surface, torch.where(pkg["alpha"] >= 0.5, pkg["median_depth"], torch.zeros_like(surface)))
            differs += int((surface != surface_depth(pkg["depth"], pkg["alpha"], None, 0.0, 0.5)).sum())
            by_hand.integrate(surface, cam, color=pkg["render"], max_depth=7.5)
    fuse_views(cameras, model, pipe, bg, expected_depth, alpha_min=0.5, max_depth=7.5)
    updated = int((fused.weight > 0).sum())
    print(f"[median tsdf] {updated} of {fused.weight.numel()} points updated; the median and the expected depth differ on "
          f"{differs} pixels")
    assert updated > 1000 and differs > 0
    for name in ("tsdf", "weight", "color"):
        assert torch.equal(getattr(fused, name), getattr(by_hand, name)), name
    assert not torch.equal(fused.tsdf, expected_depth.tsdf), "depth_ratio = 1 fused the expected depth"
