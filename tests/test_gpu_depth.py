"""Depth / inverse-depth / alpha maps of the HIP path (csrc/depth.hip; GaussianRasterizer(aux_maps=True),
render(return_depth=True)) against the float64 restatement of tests/depth_restate.py.

Scenes (conftest.small_scene):
  small   P = 400 at 72x40, SH degree 3: the last tile column and the last tile row are partial, several tiles;
  big     P = 3000 at 320x176 with splats large enough that tile lists exceed one 256-entry round of the kernels and
          some Gaussians have more than 64 instances (asserted below);
  behind  `small` with Gaussians behind the camera and inside the near plane;
  and a frame without any instance.

Bars.  Forward maps and gradients are compared on / through the pixels whose float64 oracle margin clears
grad_util.MARGIN (the bar of the parity tests); at most 5 % of the covered pixels may be left out (asserted; the seeds
were chosen on the CPU with the oracle alone).  Per tensor, max-norm relative: max(1e-5, 2 x the float32 restatement's
own error against float64) -- grad_util.compare_grads, the project's standing rule.  The observed figures are printed
by every test (run with -s).
"""
import functools

import pytest
import torch

from conftest import make_settings, small_scene
from depth_restate import assert_rounds_covered, map_weights, maps_from_lists, maps_loss, maps_ref, stacked_scene
from gpu_util import product_settings
from grad_util import MARGIN, TOL, compare_grads, linear_weights, oracle_operator_inputs, weighted_sum

pytestmark = pytest.mark.gpu

SCENES = {
    "small": dict(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2),
    "big": dict(P=3000, sh_degree=3, width=320, height=176, focal=60.0, scale=0.5, seed=1),
}
MAX_LEFT_OUT = 0.05


def _scene(name):
    if name == "stacked":
        return stacked_scene()
    model, cam, bg, _ = small_scene(**SCENES["small" if name == "behind" else name])
    if name == "behind":
        model._xyz[3, 2] = -4.0          # behind the camera
        model._xyz[17, 2] = 0.1          # in front of it, inside the near plane (0.2)
        model._xyz[101] = torch.tensor([0.3, -0.2, -0.5])
    return model, cam, bg


@functools.lru_cache(maxsize=None)
def _reference(name, use_cov=False):
    """float64 and float32 restatement of a scene: maps, the loss weights (zero on threshold-fragile pixels) and the
    gradients of the smooth loss; computed once per scene and shared, never modified."""
    model, cam, bg = _scene(name)
    st = make_settings(cam, bg, 3)
    out = {}
    weights = None
    for dt in (torch.float64, torch.float32):
        leaves, xyz, m2, op, kw = oracle_operator_inputs(model, dt, use_cov=use_cov)
        maps, _, radii, aux = maps_ref(xyz, m2, op, st, **kw)
        if weights is None:
            robust = aux["margin"] > MARGIN
            covered = aux["n_contrib"] > 0
            weights = map_weights(*maps.shape[1:]) * robust[None]
            out.update(robust=robust, covered=covered, weights=weights, radii=radii.clone(), aux=aux)
        maps_loss(maps, weights).backward()
        names = ("xyz", "opacity", "means2D") + (("cov3D",) if use_cov else ("scaling", "rotation"))
        out[dt] = (maps.detach(), {k: leaves[k].grad.detach().clone() for k in names})
    left_out = float((out["covered"] & ~out["robust"]).sum()) / max(1, int(out["covered"].sum()))
    print(f"[depth] scene {name}: {int(out['covered'].sum())} covered pixels, share left out of the comparison "
          f"{left_out:.4f}")
    assert left_out <= MAX_LEFT_OUT, f"scene {name}: the oracle alone leaves out {left_out:.3f} of the covered pixels"
    out["left_out"] = left_out
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


def _hip(dev, name, aux_maps=True, use_cov=False):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    model, cam, bg = _scene(name)
    st = product_settings(cam, bg, 3, dev)
    leaves, kw = _hip_leaves(dev, model, use_cov)
    return leaves, GaussianRasterizer(st, aux_maps=aux_maps)(**kw)


def _map_grads(leaves, maps, weights, names):
    got = torch.autograd.grad(maps_loss(maps, weights), [leaves[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if g is None else g).detach().cpu() for k, g in zip(names, got)}


def _check_forward(maps, ref, label):
    m64, m32 = ref[torch.float64][0], ref[torch.float32][0]
    robust = ref["robust"]
    got = maps.detach().cpu().double()
    rows = []
    for c, cname in enumerate(("depth", "invdepth", "alpha")):
        scale = float(m64[c][robust].abs().max())
        e = float((got[c] - m64[c])[robust].abs().max()) / scale
        e32 = float((m32[c].double() - m64[c])[robust].abs().max()) / scale
        bar = max(TOL, 2.0 * e32)
        rows.append(f"{cname}: err {e:.2e} (float32 restatement {e32:.2e}, bar {bar:.2e})")
        assert e <= bar, f"{label}: {cname} map is {e:.2e} off the float64 restatement, bar {bar:.2e}"
    print(f"[depth forward] {label}: " + "; ".join(rows))
    covered = ref["covered"]
    assert float(got[:, ~covered & robust].abs().max() if bool((~covered & robust).any()) else 0.0) == 0.0


@pytest.mark.parametrize("name", ["small", "big", "behind", "stacked"])
def test_maps_and_gradients_match_the_float64_restatement(gpu_device, name):
    ref = _reference(name)
    if name == "stacked":
        assert_rounds_covered(ref["aux"])
    leaves, (color, radii, maps) = _hip(gpu_device, name)
    assert tuple(maps.shape) == (3,) + tuple(ref["robust"].shape) and maps.dtype == torch.float32
    assert torch.equal(radii.cpu(), ref["radii"].to(torch.int32))
    if name == "big":
        aux = ref["aux"]
        assert int((aux["ranges"][:, 1] - aux["ranges"][:, 0]).max()) > 256, "a list must exceed one 256-entry round"
        assert int(aux["n_contrib"].max()) > 256, "a pixel must composite past the first round"
        assert int(aux["pre"]["tiles_touched"].max()) > 64, "a Gaussian must have more than 64 instances"
    _check_forward(maps, ref, name)
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    got = _map_grads(leaves, maps, ref["weights"], tuple(g64))
    compare_grads(got, g64, g32, f"depth maps, {name}")
    assert leaves["means2D"].grad is None       # autograd.grad leaves .grad alone; the tensor itself is checked above
    assert float(got["means2D"].abs().max()) > 0.0, "dL/dmeans2D of the maps must be present"
    assert float(got["means2D"][:, 2].abs().max()) == 0.0
    if name == "behind":
        for k, g in got.items():
            assert float(g[[3, 17, 101]].abs().max()) == 0.0, f"{k}: a Gaussian behind the camera received a gradient"


def test_cov3d_precomp_path(gpu_device):
    ref = _reference("small", use_cov=True)
    leaves, (_, _, maps) = _hip(gpu_device, "small", use_cov=True)
    _check_forward(maps, ref, "small, cov3D_precomp")
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    compare_grads(_map_grads(leaves, maps, ref["weights"], tuple(g64)), g64, g32, "depth maps, small, cov3D_precomp")


def _saturated(name):
    """Pixels of the scene whose walk the colour pass ended by its T rule (float64 oracle): composited over the WHOLE
    list of their tile, T would fall below 1e-4.  -> (bool [H,W], list length of every pixel's tile [H,W])."""
    ref = _reference(name)
    aux = ref["aux"]
    model, cam, bg = _scene(name)
    st = make_settings(cam, bg, 3)
    H, W = ref["robust"].shape
    gx, gy = aux["pre"]["grid"]
    lens = torch.from_numpy((aux["ranges"][:, 1] - aux["ranges"][:, 0]).astype("int64")).reshape(gy, gx)
    lens = lens.repeat_interleave(16, dim=0).repeat_interleave(16, dim=1)[:H, :W]
    with torch.no_grad():
        whole = maps_from_lists(aux["pre"], aux["point_list"], aux["ranges"], lens, st)
    return (1.0 - whole[2]) < 1e-4, lens


def _final_T(dev, color, H, W):
    from mvs_gaussian_splatting_amd import _lib
    img = color.grad_fn.saved_tensors[-1]
    final_T = torch.empty(H, W, device=dev)
    _lib.check(_lib.load().gsr_debug_read_image(img.data_ptr(), W, H, final_T.data_ptr(), None, None,
                                                torch.cuda.current_stream(dev).cuda_stream), "read_img")
    torch.cuda.synchronize(dev)
    return final_T


@pytest.mark.parametrize("name", ["small", "big"])
def test_the_maps_take_the_colour_passes_decisions_and_leave_the_colour_path_alone(gpu_device, name):
    """alpha == 1 - final_T bit for bit at every pixel; colour, radii and every colour gradient with aux_maps=True equal
    those with aux_maps=False bit for bit; two runs give bit-equal maps and gradients within the bar."""
    H, W = SCENES[name]["height"], SCENES[name]["width"]
    wts = linear_weights((3, H, W))
    names = ("xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation", "means2D")
    runs = []
    for aux_maps in (True, False, True):
        leaves, out = _hip(gpu_device, name, aux_maps=aux_maps)
        cg = torch.autograd.grad(weighted_sum(out[0], wts), [leaves[k] for k in names], retain_graph=True)
        runs.append((leaves, out, cg))
    (l1, o1, c1), (_, o0, c0), (l2, o2, c2) = runs
    assert len(o0) == 2 and len(o1) == 3
    final_T = _final_T(gpu_device, o1[0], H, W)
    assert torch.equal(o1[2][2], 1.0 - final_T), "alpha map and 1 - final_T differ in some bit"
    assert float(final_T.min()) < 0.5, "the scene must have well-covered pixels"
    if name == "big":
        # the prefix + alpha test stand in for the colour pass's T stop rule only where that rule fired: such pixels exist
        saturated, lens = _saturated(name)
        n_sat = int(saturated.sum())
        print(f"[depth decisions] {name}: {n_sat} pixels end their walk by the T rule")
        assert n_sat >= 16, "the scene must have pixels that saturate (stop at T < 1e-4 before the end of their list)"
        assert bool((_reference(name)["aux"]["n_contrib"].long() < lens)[saturated].all())
        assert float(final_T.cpu()[saturated].min()) >= 1e-4 and float(final_T.cpu()[saturated].max()) < 1e-2
    assert torch.equal(o1[0], o0[0]) and torch.equal(o1[1], o0[1]), "colour / radii changed with aux_maps=True"
    for k, a, b in zip(names, c1, c0):
        assert torch.equal(a, b), f"colour gradient of {k} changed with aux_maps=True"
    assert torch.equal(o1[2], o2[2]), "the maps of two runs differ"
    ref = _reference(name)
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    ga = _map_grads(l1, o1[2], ref["weights"], tuple(g64))
    gb = _map_grads(l2, o2[2], ref["weights"], tuple(g64))
    for k in g64:
        scale = float(g64[k].abs().max())
        bar = max(TOL, 2.0 * float((g32[k].double() - g64[k]).abs().max()) / scale)
        e = float((ga[k].double() - gb[k].double()).abs().max()) / scale
        print(f"[depth reproducibility] {name} {k}: two runs differ by {e:.2e} (bar {bar:.2e})")
        assert e <= bar


def test_frame_without_any_instance(gpu_device):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    model, cam, bg = _scene("small")
    model._xyz[:, 2] = -model._xyz[:, 2].abs() - 1.0
    st = product_settings(cam, bg, 3, gpu_device)
    leaves, kw = _hip_leaves(gpu_device, model, False)
    color, radii, maps = GaussianRasterizer(st, aux_maps=True)(**kw)
    assert int((radii > 0).sum()) == 0
    assert tuple(maps.shape) == (3, 40, 72) and float(maps.abs().max()) == 0.0
    names = ("xyz", "opacity", "scaling", "rotation", "means2D")
    got = _map_grads(leaves, maps, map_weights(40, 72), names)
    for k in names:
        assert got[k].shape == leaves[k].shape and float(got[k].abs().max()) == 0.0, k


def test_fused_raw_parameter_path_through_render(gpu_device):
    """render(return_depth=True) on the raw parameters against the getter-fed operator, at the bar of the scene; also
    under no_grad (the maps then come from a frame that still tracks its contributors)."""
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    ref = _reference("small")
    leaves, (color_u, _, maps_u) = _hip(gpu_device, "small")
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    unfused = _map_grads(leaves, maps_u, ref["weights"], tuple(g64))

    model, cam, bg = _scene("small")
    model.to(gpu_device)
    cam.to(gpu_device)
    for p in model.parameters():
        p.requires_grad_(True)
    pkg = render(cam, model, PipelineParams(), bg.to(gpu_device), return_depth=True)
    for k in ("depth", "invdepth", "alpha"):
        assert tuple(pkg[k].shape) == (1, 40, 72)
    maps_f = torch.cat((pkg["depth"], pkg["invdepth"], pkg["alpha"]), dim=0)
    # the fused path takes exp / sigmoid / normalize inside the preprocess kernel: its colour equals the getter-fed
    # operator's up to the activations' rounding (the bar of test_gpu_c5_views), and the plain fused frame's bit for bit
    # (asserted at the end)
    assert float((pkg["render"] - color_u).abs().max()) <= 2.0 / 255.0
    _check_forward(maps_f, ref, "small, fused")
    maps_loss(maps_f, ref["weights"]).backward()
    fused = {"xyz": model._xyz.grad, "opacity": model._opacity.grad, "scaling": model._scaling.grad,
             "rotation": model._rotation.grad, "means2D": pkg["viewspace_points"].grad}
    assert model._features_dc.grad is None, "the maps do not depend on the colour"
    for k, g in fused.items():
        scale = float(unfused[k].abs().max())
        bar = max(TOL, 2.0 * float((g32[k].double() - g64[k]).abs().max()) / float(g64[k].abs().max()))
        e = float((g.detach().cpu().double() - unfused[k].double()).abs().max()) / scale
        print(f"[depth fused] {k}: fused vs getter-fed operator {e:.2e} (bar {bar:.2e})")
        assert e <= bar, k
    compare_grads({k: v.detach().cpu() for k, v in fused.items()}, g64, g32, "depth maps, small, fused")
    with torch.no_grad():
        pkg0 = render(cam, model, PipelineParams(), bg.to(gpu_device), return_depth=True)
    assert torch.equal(pkg0["alpha"], pkg["alpha"]) and torch.equal(pkg0["depth"], pkg["depth"])
    assert torch.equal(pkg0["render"], pkg["render"])
    plain = render(cam, model, PipelineParams(), bg.to(gpu_device))
    assert "depth" not in plain and torch.equal(plain["render"], pkg["render"])


def test_training_iteration_with_a_depth_loss(gpu_device, monkeypatch):
    """training_iteration(depth_loss=(target, weight)): the frame is rendered with the maps, weight * mean|invdepth -
    target| joins the loss (a target 0.05 above the map everywhere adds exactly 0.05 * weight and sends the gradient
    -weight / (H W) into every pixel of the map), the statistics are taken from the summed viewspace gradient and the
    optimizer steps."""
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    W, H, weight = 72, 40, 0.5
    problem = example.make_problem(gpu_device, P=600, W=W, H=H, n_views=2)
    cams, bg, _ = problem
    opt = example.small_opt(40)
    pipe = PipelineParams()
    model = example.make_model(problem, opt)
    with torch.no_grad():
        first = trainer.render(cams[0], model, pipe, bg, return_depth=True)
    assert float(first["alpha"].max()) > 0.01, "the scene must cover some pixels"
    target = (first["invdepth"] + 0.05).cpu()                      # the trainer moves it to the device
    plain = float(trainer.training_iteration(example.make_model(problem, opt), cams[0], opt, pipe, bg, 1,
                                             cameras_extent=example.CAMERAS_EXTENT))
    seen, real_render = {}, trainer.render

    def spy(*args, **kw):
        pkg = real_render(*args, **kw)
        seen["kw"], seen["pkg"] = kw, pkg
        pkg["invdepth"].register_hook(lambda g: seen.__setitem__("g", g.detach().clone()))
        return pkg
    monkeypatch.setattr(trainer, "render", spy)
    before = model._xyz.detach().clone()
    loss = float(trainer.training_iteration(model, cams[0], opt, pipe, bg, 1, cameras_extent=example.CAMERAS_EXTENT,
                                            depth_loss=(target, weight)))
    assert seen["kw"].get("return_depth") is True and tuple(seen["pkg"]["invdepth"].shape) == (1, H, W)
    assert torch.equal(seen["pkg"]["invdepth"].detach(), first["invdepth"])
    print(f"[depth trainer] loss {plain:.6f} without, {loss:.6f} with the depth term")
    assert abs(loss - plain - 0.05 * weight) <= 1e-5, (loss, plain)
    expected = torch.full((1, H, W), -weight / (H * W), device=gpu_device)
    assert torch.allclose(seen["g"], expected, rtol=1e-6, atol=0.0)
    assert not getattr(seen["pkg"]["viewspace_points"], "_gsr_stats_fused", False)
    assert float(model.denom.sum()) > 0 and float(model.xyz_gradient_accum.sum()) > 0, "statistics were not taken"
    assert not torch.equal(model._xyz.detach(), before), "the optimizer did not step"
