"""The depth-distortion map of the HIP path (csrc/distortion.hip; GaussianRasterizer(distortion=...),
render(return_distortion=True)) against the float64 restatement of tests/distortion_restate.py.

Scenes (those of tests/test_gpu_depth.py, conftest.small_scene):
  small   P = 400 at 72x40: the last tile column and the last tile row are partial, several tiles;
  big     P = 3000 at 320x176: tile lists exceed one 256-entry round of the kernels, a pixel composites past the first
          round and some Gaussians have more than 64 instances (asserted below);
  behind  `small` with Gaussians behind the camera and inside the near plane;
  slab    `small` with every view depth in 5 +- 0.005 (mapping "linear"): the state the loss drives towards, where the
          float32 moments form A M2 - M1^2 is wrong in the first digit (tests/test_distortion_host.py);
  and a frame without any instance.

Bars.  The map and the gradients of a random-weighted sum of it are compared on / through the pixels whose float64
oracle margin clears grad_util.MARGIN; at most 5 % of the covered pixels may be left out (asserted on the oracle alone;
the seeds are those of test_gpu_depth.py, checked on the CPU).  Per tensor, max-norm relative:
max(1e-5, 2 x the float32 restatement's own error against float64) -- grad_util.compare_grads.  The observed figures are
printed by every test (run with -s).

The map is a sum in a fixed order (bit-equal from run to run); the gradients go through float atomics and are
reproducible to rounding only, so they are compared at the bar and never bit for bit.
"""
import functools
import math
import os
import sys
import types

import pytest
import torch

from conftest import ROOT, make_settings, small_scene
from depth_restate import assert_rounds_covered, stacked_scene
from distortion_restate import dist_loss, dist_weights, distortion_ref, slab_model
from gpu_util import product_settings
from grad_util import MARGIN, compare_grads, linear_weights, oracle_operator_inputs, weighted_sum

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu

SCENES = {
    "small": dict(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2),
    "big": dict(P=3000, sh_degree=3, width=320, height=176, focal=60.0, scale=0.5, seed=1),
}
MAX_LEFT_OUT = 0.05


def _scene(name):
    if name == "stacked":
        return stacked_scene()
    model, cam, bg, _ = small_scene(**SCENES["big" if name == "big" else "small"])
    if name == "behind":
        model._xyz[3, 2] = -4.0          # behind the camera
        model._xyz[17, 2] = 0.1          # in front of it, inside the near plane (0.2)
        model._xyz[101] = torch.tensor([0.3, -0.2, -0.5])
    if name == "slab":
        slab_model(model)
    return model, cam, bg


@functools.lru_cache(maxsize=None)
def _reference(name, mapping, use_cov=False):
    """float64 and float32 restatement of a scene: the map, the loss weights (zero on threshold-fragile pixels) and the
    gradients of the smooth loss; computed once per (scene, mapping) and shared, never modified."""
    model, cam, bg = _scene(name)
    st = make_settings(cam, bg, 3)
    out = {}
    weights = None
    for dt in (torch.float64, torch.float32):
        leaves, xyz, m2, op, kw = oracle_operator_inputs(model, dt, use_cov=use_cov)
        dist, _, radii, aux = distortion_ref(xyz, m2, op, st, mapping, **kw)
        if weights is None:
            robust = aux["margin"] > MARGIN
            covered = aux["n_contrib"] > 0
            weights = dist_weights(*dist.shape[1:]) * robust[None]
            out.update(robust=robust, covered=covered, weights=weights, radii=radii.clone(), aux=aux)
        dist_loss(dist, weights).backward()
        names = ("xyz", "opacity", "means2D") + (("cov3D",) if use_cov else ("scaling", "rotation"))
        out[dt] = (dist.detach(), {k: leaves[k].grad.detach().clone() for k in names})
    left_out = float((out["covered"] & ~out["robust"]).sum()) / max(1, int(out["covered"].sum()))
    print(f"[distortion] scene {name}, {mapping}: {int(out['covered'].sum())} covered pixels, share left out of the "
          f"comparison {left_out:.4f}")
    assert left_out <= MAX_LEFT_OUT, f"scene {name}: the oracle alone leaves out {left_out:.3f} of the covered pixels"
    return out


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


def _hip(dev, name, mapping, use_cov=False, **ctor):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    model, cam, bg = _scene(name)
    st = product_settings(cam, bg, 3, dev)
    leaves, kw = _hip_leaves(dev, model, use_cov)
    if mapping is not None:
        ctor["distortion"] = dict(mapping=mapping)
    return leaves, GaussianRasterizer(st, **ctor)(**kw)


def _dist_grads(leaves, dist, weights, names):
    got = torch.autograd.grad(dist_loss(dist, weights), [leaves[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if g is None else g).detach().cpu() for k, g in zip(names, got)}


def _check_forward(dist, ref, label):
    d64, d32 = ref[torch.float64][0], ref[torch.float32][0]
    robust, covered = ref["robust"], ref["covered"]
    got = dist.detach().cpu()
    assert tuple(got.shape) == tuple(d64.shape) and got.dtype == torch.float32
    compare_grads({"dist": got * robust[None]}, {"dist": d64 * robust[None]}, {"dist": d32 * robust[None]},
                  f"distortion map, {label}")
    assert float(got[0][~covered].abs().max() if bool((~covered).any()) else 0.0) == 0.0, "an uncovered pixel is not 0"
    assert float(got.min()) >= 0.0


@pytest.mark.parametrize("name,mapping", [("small", "ndc"), ("small", "linear"), ("big", "ndc"), ("behind", "ndc"),
                                          ("slab", "linear"), ("stacked", "ndc")])
def test_map_and_gradients_match_the_float64_restatement(gpu_device, name, mapping):
    ref = _reference(name, mapping)
    if name == "stacked":
        assert_rounds_covered(ref["aux"])
    leaves, (color, radii, dist) = _hip(gpu_device, name, mapping)
    assert torch.equal(radii.cpu(), ref["radii"].to(torch.int32))
    if name == "big":
        aux = ref["aux"]
        assert int((aux["ranges"][:, 1] - aux["ranges"][:, 0]).max()) > 256, "a list must exceed one 256-entry round"
        assert int(aux["n_contrib"].max()) > 256, "a pixel must composite past the first round"
        assert int(aux["pre"]["tiles_touched"].max()) > 64, "a Gaussian must have more than 64 instances"
    if name == "slab":
        z = ref["aux"]["pre"]["v_depth"].detach()
        assert 4.9949 <= float(z.min()) and float(z.max()) <= 5.0051      # 5 +- 0.005, rounded to float32
    assert float(ref[torch.float64][0].max()) > 0.0
    _check_forward(dist, ref, f"{name}, {mapping}")
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    got = _dist_grads(leaves, dist, ref["weights"], tuple(g64))
    compare_grads(got, g64, g32, f"distortion map, {name}, {mapping}")
    assert float(got["means2D"].abs().max()) > 0.0, "dL/dmeans2D of the map must be present"
    assert float(got["means2D"][:, 2].abs().max()) == 0.0
    if name == "behind":
        for k, g in got.items():
            assert float(g[[3, 17, 101]].abs().max()) == 0.0, f"{k}: a Gaussian behind the camera received a gradient"


def test_cov3d_precomp_path(gpu_device):
    ref = _reference("small", "ndc", use_cov=True)
    leaves, (_, _, dist) = _hip(gpu_device, "small", "ndc", use_cov=True)
    _check_forward(dist, ref, "small, ndc, cov3D_precomp")
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    compare_grads(_dist_grads(leaves, dist, ref["weights"], tuple(g64)), g64, g32, "distortion map, small, cov3D_precomp")


def test_the_map_is_reproducible_and_leaves_the_colour_path_and_the_depth_maps_alone(gpu_device):
    """Colour, radii, aux and every colour-path gradient with distortion=True equal those without it bit for bit; two runs
    give bit-equal maps; under no_grad the map is the same bits; gradients of two runs agree within the bar (atomics)."""
    name, mapping = "small", "ndc"
    H, W = SCENES[name]["height"], SCENES[name]["width"]
    wts = linear_weights((3, H, W))
    names = ("xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation", "means2D")
    runs = []
    for m in (mapping, None, mapping):
        leaves, out = _hip(gpu_device, name, m, aux_maps=True)
        cg = torch.autograd.grad(weighted_sum(out[0], wts), [leaves[k] for k in names], retain_graph=True)
        runs.append((leaves, out, cg))
    (l1, o1, c1), (_, o0, c0), (l2, o2, c2) = runs
    assert len(o0) == 3 and len(o1) == 4 and tuple(o1[3].shape) == (1, H, W)
    assert torch.equal(o1[0], o0[0]) and torch.equal(o1[1], o0[1]), "colour / radii changed with distortion=True"
    assert torch.equal(o1[2], o0[2]), "the depth / alpha maps changed with distortion=True"
    for k, a, b in zip(names, c1, c0):
        assert torch.equal(a, b), f"colour gradient of {k} changed with distortion=True"
    assert torch.equal(o1[3], o2[3]), "the maps of two runs differ"
    with torch.no_grad():
        _, o3 = _hip(gpu_device, name, mapping)
    assert len(o3) == 3 and torch.equal(o3[2], o1[3]) and torch.equal(o3[0], o1[0]), "the map under no_grad differs"
    assert not o3[2].requires_grad
    ref = _reference(name, mapping)
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    ga = _dist_grads(l1, o1[3], ref["weights"], tuple(g64))
    gb = _dist_grads(l2, o2[3], ref["weights"], tuple(g64))
    for k in g64:
        scale = float(g64[k].abs().max())
        bar = max(1e-5, 2.0 * float((g32[k].double() - g64[k]).abs().max()) / scale)
        e = float((ga[k].double() - gb[k].double()).abs().max()) / scale
        print(f"[distortion reproducibility] {k}: two runs differ by {e:.2e} (bar {bar:.2e})")
        assert e <= bar


def test_frame_without_any_instance(gpu_device):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    model, cam, bg = _scene("small")
    model._xyz[:, 2] = -model._xyz[:, 2].abs() - 1.0
    st = product_settings(cam, bg, 3, gpu_device)
    for _ in range(2):      # the second frame of the shape is issued whole, into the state of the first
        leaves, kw = _hip_leaves(gpu_device, model, False)
        color, radii, dist = GaussianRasterizer(st, distortion=True)(**kw)
        assert int((radii > 0).sum()) == 0
        assert tuple(dist.shape) == (1, 40, 72) and float(dist.abs().max()) == 0.0
        names = ("xyz", "opacity", "scaling", "rotation", "means2D")
        got = _dist_grads(leaves, dist, dist_weights(40, 72), names)
        for k in names:
            assert got[k].shape == leaves[k].shape and float(got[k].abs().max()) == 0.0, k


def test_fused_raw_parameter_path_through_render(gpu_device):
    """render(return_distortion=True) on the raw parameters: the map and the gradients meet the scene's bar, the map is
    the fused operator's bit for bit, also under no_grad, and the plain frame is what it was."""
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.rasterizer import rasterize_gaussians_fused
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    ref = _reference("small", "ndc")
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    model, cam, bg = _scene("small")
    model.to(gpu_device)
    cam.to(gpu_device)
    for p in model.parameters():
        p.requires_grad_(True)
    pkg = render(cam, model, PipelineParams(), bg.to(gpu_device), return_distortion=True)
    assert tuple(pkg["distortion"].shape) == (1, 40, 72) and "depth" not in pkg
    _check_forward(pkg["distortion"], ref, "small, ndc, fused")
    # the operator on the same raw parameters: the same frame, the same map, bit for bit
    st = product_settings(cam, bg, 3, gpu_device)
    out = rasterize_gaussians_fused(model._xyz, None, model._features_dc, model._features_rest, model._opacity,
                                    model._scaling, model._rotation, st, distortion=True)
    assert torch.equal(out[0], pkg["render"]) and torch.equal(out[2], pkg["distortion"])
    dist_loss(pkg["distortion"], ref["weights"]).backward()
    fused = {"xyz": model._xyz.grad, "opacity": model._opacity.grad, "scaling": model._scaling.grad,
             "rotation": model._rotation.grad, "means2D": pkg["viewspace_points"].grad}
    assert model._features_dc.grad is None, "the map does not depend on the colour"
    compare_grads({k: v.detach().cpu() for k, v in fused.items()}, g64, g32, "distortion map, small, fused")
    with torch.no_grad():
        pkg0 = render(cam, model, PipelineParams(), bg.to(gpu_device), return_distortion=True,
                      distortion_kwargs=dict(mapping="ndc", near=0.2, far=100.0))
    assert torch.equal(pkg0["distortion"], pkg["distortion"]) and torch.equal(pkg0["render"], pkg["render"])
    plain = render(cam, model, PipelineParams(), bg.to(gpu_device))
    assert "distortion" not in plain and torch.equal(plain["render"], pkg["render"])
    both = render(cam, model, PipelineParams(), bg.to(gpu_device), return_depth=True, return_normals=True,
                  return_distortion=True)
    assert torch.equal(both["distortion"], pkg["distortion"]) and tuple(both["normal"].shape) == (3, 40, 72)
    assert tuple(both["depth"].shape) == (1, 40, 72)


PLANE = (0.3, -0.2, 4.0)         # view-space plane z = 4 + 0.3 x - 0.2 y (the scene of test_gpu_normal_consistency.py)


@pytest.fixture(scope="module")
def problem(gpu_device):
    """A 64x48 frame of 400 flat Gaussians on a tilted plane in front of the example's camera."""
    import train as example
    cams, bg, _ = example.make_problem(gpu_device, P=600, W=64, H=48, n_views=1)
    g = torch.Generator().manual_seed(11)
    xy = (torch.rand(400, 2, generator=g) - 0.5) * torch.tensor([1.5, 1.2])
    view = torch.cat((xy, (PLANE[2] + PLANE[0] * xy[:, :1] + PLANE[1] * xy[:, 1:]), torch.ones(400, 1)), dim=1)
    world = (view.to(gpu_device) @ torch.linalg.inv(cams[0].world_view_transform.float()))[:, :3].contiguous()
    colors = torch.rand(400, 3, generator=g).to(gpu_device)
    return cams, bg, (world, colors)


def _plane_model(problem, opt):
    import train as example
    model = example.make_model(problem, opt)
    with torch.no_grad():
        model._opacity.fill_(2.0)
        model._scaling[:, :2] = math.log(0.07)
        model._scaling[:, 2] = math.log(0.004)
    return model


def test_training_iteration_with_the_term_and_bit_identity_without_it(gpu_device, problem, monkeypatch):
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    cams, bg, _ = problem
    pipe = PipelineParams()
    opt = example.small_opt(40, lambda_dist=100.0, dist_from_iter=0, lambda_normal=0.05, normal_from_iter=0)
    model = _plane_model(problem, opt)
    seen, real_render = {}, trainer.render

    def spy(*args, **kw):
        pkg = real_render(*args, **kw)
        seen["kw"] = kw
        if "distortion" in pkg:
            pkg["distortion"].register_hook(lambda g: seen.__setitem__("g", g.detach().clone()))
        return pkg
    monkeypatch.setattr(trainer, "render", spy)
    grads = {}
    real_step = model.optimizer.step

    def step(*a, **k):
        for group in model.optimizer.param_groups:
            grads[group["name"]] = None if group["params"][0].grad is None else group["params"][0].grad.detach().clone()
        return real_step(*a, **k)
    monkeypatch.setattr(model.optimizer, "step", step)
    loss = float(training_iteration(model, cams[0], opt, pipe, bg, 1, cameras_extent=example.CAMERAS_EXTENT))
    monkeypatch.undo()
    base = float(training_iteration(_plane_model(problem, example.small_opt(40, lambda_normal=0.05, normal_from_iter=0)),
                                    cams[0], example.small_opt(40, lambda_normal=0.05, normal_from_iter=0), pipe, bg, 1,
                                    cameras_extent=example.CAMERAS_EXTENT))
    print(f"[distortion trainer] loss {loss:.6f} with lambda_dist = 100 and lambda_normal = 0.05, {base:.6f} without "
          f"the distortion term")
    assert seen["kw"].get("return_distortion") is True and seen["kw"].get("return_normals") is True
    assert math.isfinite(loss) and loss > base, "the term must add to the loss"
    assert torch.allclose(seen["g"], torch.full((1, 48, 64), 100.0 / (48 * 64), device=gpu_device), rtol=1e-6, atol=0.0)
    assert set(grads) >= {"xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"}
    for k, g in grads.items():
        assert g is not None and bool(torch.isfinite(g).all()), f"group {k} has no gradient"
        # (f_rest: the active SH degree is 0 at iteration 1, its gradient is present and zero)
        assert k == "f_rest" or float(g.abs().max()) > 0.0, f"the gradient of group {k} is zero"
    assert float(model.denom.sum()) > 0, "the densification statistics were not taken"
    # lambda_dist = 0 against a parent-equivalent call: options that do not know the two fields at all; and not yet on
    zero = example.small_opt(40)
    late = example.small_opt(40, lambda_dist=100.0, dist_from_iter=3000)
    parent = types.SimpleNamespace(**{k: getattr(zero, k) for k in dir(OptimizationParams)
                                      if not k.startswith("_") and k not in ("lambda_dist", "dist_from_iter")})
    assert zero.lambda_dist == 0.0 and zero.dist_from_iter == 3000 and not hasattr(parent, "lambda_dist")
    results = []
    for o in (zero, parent, late):
        m = _plane_model(problem, zero)
        out = [training_iteration(m, cams[0], o, pipe, bg, it, cameras_extent=example.CAMERAS_EXTENT) for it in (1, 2)]
        results.append((out, [getattr(m, n).detach().clone() for n in ("_xyz", "_features_dc", "_features_rest", "_opacity",
                                                                       "_scaling", "_rotation")]))
    for other in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0][0], other[0])), "the loss differs"
        assert all(torch.equal(x, y) for x, y in zip(results[0][1], other[1])), "a parameter differs"
