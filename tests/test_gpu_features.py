"""Feature maps of the HIP path (csrc/features.hip; ``GaussianRasterizer.forward(..., features=F)``,
``render(features=F, return_normals=True)``) against the float64 restatement of
tests/features_restate.py.

Scenes: exactly those of tests/test_gpu_depth.py (`small`, `big`, `behind`) and a frame without any instance.

Bars.  Maps and gradients are compared on / through the pixels whose float64 oracle margin clears grad_util.MARGIN; at
most 5 % of the covered pixels may be left out (asserted).  Per channel / per tensor, max-norm relative:
max(1e-5, 2 x the float32 restatement's own error against float64) -- grad_util.compare_grads.  ``F = randn(P, C)`` from a
fixed seed in float32, cast up for float64.  The observed figures are printed by every test (run with -s).
"""
import functools

import pytest
import torch

from conftest import make_settings, small_scene
from depth_restate import assert_rounds_covered, stacked_scene
from features_restate import feature_maps_from_lists, feature_rows, feature_weights
from gpu_util import product_settings
from grad_util import MARGIN, TOL, compare_grads, linear_weights, oracle_operator_inputs, weighted_sum

pytestmark = pytest.mark.gpu

SCENES = {
    "small": dict(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2),
    "big": dict(P=3000, sh_degree=3, width=320, height=176, focal=60.0, scale=0.5, seed=1),
}
MAX_LEFT_OUT = 0.05
BEHIND = [3, 17, 101]


def _scene(name):
    if name == "stacked":
        return stacked_scene()
    model, cam, bg, _ = small_scene(**SCENES["small" if name == "behind" else name])
    if name == "behind":
        model._xyz[3, 2] = -4.0          # behind the camera
        model._xyz[17, 2] = 0.1          # in front of it, inside the near plane (0.2)
        model._xyz[101] = torch.tensor([0.3, -0.2, -0.5])
    return model, cam, bg


def _geometry_names(use_cov):
    return ("xyz", "opacity", "means2D") + (("cov3D",) if use_cov else ("scaling", "rotation"))


@functools.lru_cache(maxsize=None)
def _oracle_frame(name, use_cov=False):
    """The oracle's frame of a scene in float64 and float32 with its autograd graph kept (the restatements of every C
    differentiate through it), the robust / covered pixel sets of the float64 run; computed once, never modified."""
    from oracle import rasterize_ref
    model, cam, bg = _scene(name)
    st = make_settings(cam, bg, 3)
    out = {"settings": st}
    for dt in (torch.float64, torch.float32):
        leaves, xyz, m2, op, kw = oracle_operator_inputs(model, dt, use_cov=use_cov)
        _, radii, aux = rasterize_ref(xyz, m2, op, st, want_aux=True, want_margin=True, **kw)
        out[dt] = (leaves, aux)
        if dt == torch.float64:
            out.update(robust=aux["margin"] > MARGIN, covered=aux["n_contrib"] > 0, radii=radii.clone(), aux=aux)
    left_out = float((out["covered"] & ~out["robust"]).sum()) / max(1, int(out["covered"].sum()))
    print(f"[features] scene {name}: {int(out['covered'].sum())} covered pixels, share left out of the comparison "
          f"{left_out:.4f}")
    assert left_out <= MAX_LEFT_OUT, f"scene {name}: the oracle alone leaves out {left_out:.3f} of the covered pixels"
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, C, use_cov=False):
    """float64 and float32 restatement for ``F = feature_rows(P, C)``: the maps, the loss weights (zero on
    threshold-fragile pixels) and the gradients of the smooth loss for ``features`` and the geometry."""
    fr = _oracle_frame(name, use_cov)
    H, W = fr["robust"].shape
    F32 = feature_rows(int(fr["radii"].shape[0]), C)
    weights = feature_weights(C, H, W) * fr["robust"][None]
    out = dict(robust=fr["robust"], covered=fr["covered"], weights=weights, radii=fr["radii"], aux=fr["aux"], F=F32)
    names = _geometry_names(use_cov)
    for dt in (torch.float64, torch.float32):
        leaves, aux = fr[dt]
        F = F32.to(dt).clone().requires_grad_(True)      # (a copy: .to(float32) would hand back the shared rows)
        lists = (aux["point_list"], aux["ranges"], aux["n_contrib"])      # the oracle's own, held fixed
        feat = feature_maps_from_lists(aux["pre"], *lists, fr["settings"], F)
        got = torch.autograd.grad(weighted_sum(feat, weights), [F] + [leaves[k] for k in names], retain_graph=True,
                                  allow_unused=True)
        grads = {k: (torch.zeros_like(t) if g is None else g.detach().clone())
                 for k, g, t in zip(("features",) + names, got, [F] + [leaves[k] for k in names])}
        out[dt] = (feat.detach(), grads)
    return out


def _hip_leaves(dev, model, use_cov, detach_geometry=False):
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.detach().to(dev).requires_grad_(not detach_geometry)
        return leaves[name]

    xyz, op = leaf("xyz", model._xyz), leaf("opacity", model._opacity)
    leaves["means2D"] = torch.zeros(xyz.shape[0], 3, device=dev, requires_grad=not detach_geometry)
    fdc, fr = leaf("f_dc", model._features_dc), leaf("f_rest", model._features_rest)
    kw = {"shs": torch.cat((fdc, fr), dim=1)}
    if use_cov:
        kw["cov3D_precomp"] = leaf("cov3D", model.get_covariance(1.0))
    else:
        kw["scales"] = torch.exp(leaf("scaling", model._scaling))
        kw["rotations"] = torch.nn.functional.normalize(leaf("rotation", model._rotation))
    return leaves, dict(means3D=xyz, means2D=leaves["means2D"], opacities=torch.sigmoid(op), **kw)


def _hip(dev, name, F=None, use_cov=False, feat_grad=True, detach_geometry=False, model=None, **ctor):
    """-> (leaves, results of the call).  ``F``: float32 [P,C] on the CPU (moved, made a leaf) or None: no ``features``."""
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    scene_model, cam, bg = _scene(name)
    st = product_settings(cam, bg, 3, dev)
    leaves, kw = _hip_leaves(dev, scene_model if model is None else model, use_cov, detach_geometry)
    if F is not None:
        leaves["features"] = F.detach().to(dev).requires_grad_(feat_grad)
        kw["features"] = leaves["features"]
    return leaves, GaussianRasterizer(st, **ctor)(**kw)


def _grads(leaves, feat, weights, names):
    got = torch.autograd.grad(weighted_sum(feat, weights), [leaves[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if g is None else g).detach().cpu() for k, g in zip(names, got)}


def _bar(ref, k):
    g64, g32 = ref[torch.float64][1][k], ref[torch.float32][1][k]
    scale = float(g64.abs().max())
    return max(TOL, 2.0 * float((g32.double() - g64).abs().max()) / scale), scale


def _check_forward(feat, ref, label):
    m64, m32 = ref[torch.float64][0], ref[torch.float32][0]
    robust = ref["robust"]
    got = feat.detach().cpu().double()
    assert tuple(got.shape) == tuple(m64.shape)
    worst = (0.0, 0.0, 0.0)
    for c in range(m64.shape[0]):
        scale = float(m64[c][robust].abs().max())
        e = float((got[c] - m64[c])[robust].abs().max()) / scale
        e32 = float((m32[c].double() - m64[c])[robust].abs().max()) / scale
        bar = max(TOL, 2.0 * e32)
        worst = max(worst, (e / bar, e, e32))
        assert e <= bar, f"{label}: channel {c} is {e:.2e} off the float64 restatement, bar {bar:.2e}"
    print(f"[features forward] {label}: {m64.shape[0]} channels, worst err {worst[1]:.2e} (float32 restatement "
          f"{worst[2]:.2e}, {worst[0]:.2f} of its bar)")
    empty = ~ref["covered"] & robust
    assert float(got[:, empty].abs().max() if bool(empty.any()) else 0.0) == 0.0


CASES = [("small", 1), ("small", 3), ("small", 8), ("small", 19), ("big", 19), ("behind", 3), ("stacked", 9)]


@pytest.mark.parametrize("name,C", CASES, ids=[f"{n}-C{c}" for n, c in CASES])
def test_map_and_gradients_match_the_float64_restatement(gpu_device, name, C):
    ref = _reference(name, C)
    if name == "stacked":
        assert_rounds_covered(ref["aux"])
    leaves, (color, radii, feat) = _hip(gpu_device, name, ref["F"])
    assert tuple(feat.shape) == (C,) + tuple(ref["robust"].shape) and feat.dtype == torch.float32
    assert torch.equal(radii.cpu(), ref["radii"].to(torch.int32))
    if name == "big":
        aux = ref["aux"]
        assert int((aux["ranges"][:, 1] - aux["ranges"][:, 0]).max()) > 256, "a list must exceed one 256-entry round"
        assert int(aux["n_contrib"].max()) > 256, "a pixel must composite past the first round"
        assert int(aux["pre"]["tiles_touched"].max()) > 64, "a Gaussian must have more than 64 instances"
    _check_forward(feat, ref, f"{name}, C={C}")
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    got = _grads(leaves, feat, ref["weights"], tuple(g64))
    compare_grads(got, g64, g32, f"feature maps, {name}, C={C}")
    assert got["features"].shape == (ref["F"].shape[0], C) and float(got["features"].abs().max()) > 0.0
    assert float(got["means2D"].abs().max()) > 0.0, "dL/dmeans2D of the maps must be present"
    assert float(got["means2D"][:, 2].abs().max()) == 0.0
    if name == "behind":
        for k, g in got.items():
            assert float(g[BEHIND].abs().max()) == 0.0, f"{k}: a Gaussian behind the camera received a gradient"


def test_cov3d_precomp_path(gpu_device):
    ref = _reference("small", 3, use_cov=True)
    leaves, (_, _, feat) = _hip(gpu_device, "small", ref["F"], use_cov=True)
    _check_forward(feat, ref, "small, C=3, cov3D_precomp")
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    compare_grads(_grads(leaves, feat, ref["weights"], tuple(g64)), g64, g32, "feature maps, small, C=3, cov3D_precomp")


def _final_T(dev, color, H, W):
    from mvs_gaussian_splatting_amd import _lib
    img = color.grad_fn.saved_tensors[-1]
    final_T = torch.empty(H, W, device=dev)
    _lib.check(_lib.load().gsr_debug_read_image(img.data_ptr(), W, H, final_T.data_ptr(), None, None,
                                                torch.cuda.current_stream(dev).cuda_stream), "read_img")
    torch.cuda.synchronize(dev)
    return final_T


def _ones_frame(dev, name):
    H, W, P = SCENES[name]["height"], SCENES[name]["width"], SCENES[name]["P"]
    _, (color, _, aux, feat) = _hip(dev, name, torch.ones(P, 1), aux_maps=True)
    return feat, aux, _final_T(dev, color, H, W)


@pytest.mark.parametrize("name", ["small", "big"])
def test_ones_channel_equals_one_minus_final_T_bit_for_bit(gpu_device, name):
    """F = ones[P,1]: feat[0] == 1 - final_T == aux[2] in every bit.  The kernel's T is the colour pass's, and the forward
    sums about the first contributor's row, so a constant field is that constant times 1 - final_T, rounded once."""
    feat, aux, final_T = _ones_frame(gpu_device, name)
    d = (feat[0].detach() - (1.0 - final_T)).abs()
    print(f"[features decisions] {name}: feat[0] vs 1 - final_T: {int((d > 0).sum())} of {d.numel()} pixels differ, "
          f"max |difference| {float(d.max()):.3e}")
    assert torch.equal(aux[2], 1.0 - final_T)
    assert torch.equal(feat[0], 1.0 - final_T), "ones channel and 1 - final_T differ in some bit"
    assert torch.equal(feat[0], aux[2]), "ones channel and the alpha map differ in some bit"
    assert float(final_T.min()) < 0.5, "the scene must have well-covered pixels"


def test_a_constant_field_is_the_constant_times_the_alpha_map(gpu_device):
    """Rows that are the same for every Gaussian, one constant per channel, across two channel groups (C = 11): channel c
    is fl(k_c * (1 - final_T)) at every pixel, whatever the number of contributors."""
    H, W, P = SCENES["big"]["height"], SCENES["big"]["width"], SCENES["big"]["P"]
    consts = torch.tensor([1.0, -2.5, 0.1, 3.0e-3, 7.0, -1.0, 0.3, 123.456, 0.0, -0.7, 1.0e4])
    _, (color, _, feat) = _hip(gpu_device, "big", consts[None, :].repeat(P, 1))
    alpha = 1.0 - _final_T(gpu_device, color, H, W)
    assert torch.equal(feat.detach(), consts.to(gpu_device)[:, None, None] * alpha[None])


@pytest.mark.parametrize("name", ["small", "big"])
def test_features_leave_the_colour_path_alone_and_the_map_is_reproducible(gpu_device, name):
    H, W, P = SCENES[name]["height"], SCENES[name]["width"], SCENES[name]["P"]
    wts = linear_weights((3, H, W))
    names = ("xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation", "means2D")
    F = feature_rows(P, 19)
    runs = []
    for with_features in (True, False, True):
        leaves, out = _hip(gpu_device, name, F if with_features else None)
        cg = torch.autograd.grad(weighted_sum(out[0], wts), [leaves[k] for k in names], retain_graph=True)
        runs.append((out, cg))
    (o1, c1), (o0, c0), (o2, _) = runs
    assert len(o0) == 2 and len(o1) == 3
    assert torch.equal(o1[0], o0[0]) and torch.equal(o1[1], o0[1]), "colour / radii changed with features"
    for k, a, b in zip(names, c1, c0):
        assert torch.equal(a, b), f"colour gradient of {k} changed with features"
    assert torch.equal(o1[2], o2[2]), "the maps of two runs differ"


def test_geometry_gradients_add_over_channel_groups(gpu_device):
    """One C = 19 call against the sum of the calls on the column blocks [0:8], [8:16], [16:19] (each with its block of
    the loss weights): the geometry gradients agree within the bar of the C = 19 comparison."""
    ref = _reference("small", 19)
    names = _geometry_names(False)
    leaves, (_, _, feat) = _hip(gpu_device, "small", ref["F"])
    whole = _grads(leaves, feat, ref["weights"], names)
    total = {k: torch.zeros_like(v) for k, v in whole.items()}
    for lo, hi in ((0, 8), (8, 16), (16, 19)):
        leaves, (_, _, feat) = _hip(gpu_device, "small", ref["F"][:, lo:hi].contiguous())
        # weighted_sum divides by the block's own element count: rescale to the whole loss's
        part = _grads(leaves, feat, ref["weights"][lo:hi] * ((hi - lo) / 19.0), names)
        for k in names:
            total[k] += part[k]
    for k in names:
        bar, scale = _bar(ref, k)
        e = float((whole[k].double() - total[k].double()).abs().max()) / scale
        print(f"[features additivity] {k}: one call vs the sum of three {e:.2e} (bar {bar:.2e})")
        assert e <= bar, k
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    compare_grads(total, {k: g64[k] for k in names}, g32, "feature maps, small, sum of three column blocks")


def test_needs_input_grad_selects_the_side_that_is_computed(gpu_device):
    ref = _reference("small", 19)
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    names = _geometry_names(False)
    leaves, (_, _, feat) = _hip(gpu_device, "small", ref["F"], feat_grad=False)
    assert feat.requires_grad and not leaves["features"].requires_grad
    weighted_sum(feat, ref["weights"]).backward()
    geometry = {k: leaves[k].grad.detach().cpu() for k in names}
    compare_grads(geometry, {k: g64[k] for k in names}, g32, "feature maps, small, features without grad")
    assert leaves["features"].grad is None, "a feature gradient was returned although none was asked for"

    leaves, (color, _, feat) = _hip(gpu_device, "small", ref["F"], detach_geometry=True)
    assert feat.requires_grad and not color.requires_grad
    only = _grads(leaves, feat, ref["weights"], ("features",))
    compare_grads(only, {"features": g64["features"]}, g32, "feature maps, small, geometry detached")
    for k in names:
        assert leaves[k].grad is None


def test_frame_without_any_instance(gpu_device):
    model, cam, bg = _scene("small")
    model._xyz[:, 2] = -model._xyz[:, 2].abs() - 1.0
    leaves, (color, radii, feat) = _hip(gpu_device, "small", feature_rows(400, 19), model=model)
    assert int((radii > 0).sum()) == 0
    assert tuple(feat.shape) == (19, 40, 72) and float(feat.detach().abs().max()) == 0.0
    names = ("features", "xyz", "opacity", "scaling", "rotation", "means2D")
    got = _grads(leaves, feat, feature_weights(19, 40, 72), names)
    for k in names:
        assert got[k].shape == leaves[k].shape and float(got[k].abs().max()) == 0.0, k


def test_combined_with_the_maps_and_the_contribution_statistics(gpu_device):
    from mvs_gaussian_splatting_amd import ContributionStats
    F = feature_rows(400, 19)
    both = ContributionStats(400, gpu_device)
    _, out = _hip(gpu_device, "small", F, aux_maps=True, contribution=both)
    assert len(out) == 4 and both.views == 1
    color, radii, aux, feat = out
    assert tuple(aux.shape) == (3, 40, 72) and tuple(feat.shape) == (19, 40, 72)
    _, (c_a, r_a, aux_alone) = _hip(gpu_device, "small", aux_maps=True)
    _, (c_f, r_f, feat_alone) = _hip(gpu_device, "small", F)
    alone = ContributionStats(400, gpu_device)
    _, (c_c, r_c) = _hip(gpu_device, "small", contribution=alone)
    for c, r in ((c_a, r_a), (c_f, r_f), (c_c, r_c)):
        assert torch.equal(c, color) and torch.equal(r, radii)
    assert torch.equal(aux, aux_alone) and torch.equal(feat, feat_alone) and torch.equal(both.raw, alone.raw)
    assert int(both.raw[:, 1].sum()) > 0


def test_render_features_normals_and_the_grow_branch_refusal(gpu_device, monkeypatch):
    from mvs_gaussian_splatting_amd import gaussian_normals, grow, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    ref = _reference("small", 3)
    g64, g32 = ref[torch.float64][1], ref[torch.float32][1]
    leaves, (color_u, _, feat_u) = _hip(gpu_device, "small", ref["F"])
    unfused = _grads(leaves, feat_u, ref["weights"], tuple(g64))

    model, cam, bg = _scene("small")
    model.to(gpu_device)
    cam.to(gpu_device)
    for p in model.parameters():
        p.requires_grad_(True)
    pipe, bg = PipelineParams(), bg.to(gpu_device)
    F = ref["F"].detach().to(gpu_device).requires_grad_(True)
    pkg = render(cam, model, pipe, bg, features=F)
    assert tuple(pkg["features"].shape) == (3, 40, 72) and "normal" not in pkg and "depth" not in pkg
    assert float((pkg["render"] - color_u).abs().max()) <= 2.0 / 255.0
    _check_forward(pkg["features"], ref, "small, C=3, fused")
    weighted_sum(pkg["features"], ref["weights"]).backward()
    fused = {"features": F.grad, "xyz": model._xyz.grad, "opacity": model._opacity.grad, "scaling": model._scaling.grad,
             "rotation": model._rotation.grad, "means2D": pkg["viewspace_points"].grad}
    assert model._features_dc.grad is None, "the maps do not depend on the colour"
    for k, g in fused.items():
        bar, _ = _bar(ref, k)
        e = float((g.detach().cpu().double() - unfused[k].double()).abs().max()) / float(unfused[k].abs().max())
        print(f"[features fused] {k}: fused vs getter-fed operator {e:.2e} (bar {bar:.2e})")
        assert e <= bar, k
    compare_grads({k: v.detach().cpu() for k, v in fused.items()}, g64, g32, "feature maps, small, C=3, fused")
    assert not getattr(pkg["viewspace_points"], "_gsr_stats_fused", False)
    plain = render(cam, model, pipe, bg)
    assert "features" not in plain and torch.equal(plain["render"], pkg["render"])

    # normals: return_normals=True is the features path fed with gaussian_normals(...), alone and next to user rows
    for p in model.parameters():
        p.grad = None
    n_rows = gaussian_normals(model.get_scaling, model.get_rotation, model.get_xyz, cam.world_view_transform,
                              cam.camera_center)
    by_hand = render(cam, model, pipe, bg, features=n_rows.detach())["features"]
    pkg_n = render(cam, model, pipe, bg, return_normals=True)
    assert tuple(pkg_n["normal"].shape) == (3, 40, 72) and "features" not in pkg_n
    assert torch.equal(pkg_n["normal"], by_hand)
    both = render(cam, model, pipe, bg, features=F.detach(), return_normals=True)
    assert torch.equal(both["features"], pkg["features"]) and torch.equal(both["normal"], by_hand)
    with torch.no_grad():
        quiet = render(cam, model, pipe, bg, features=F.detach(), return_normals=True, return_depth=True)
    assert torch.equal(quiet["normal"], by_hand) and torch.equal(quiet["features"], pkg["features"])
    assert tuple(quiet["alpha"].shape) == (1, 40, 72) and not quiet["normal"].requires_grad
    weighted_sum(pkg_n["normal"], feature_weights(3, 40, 72)).backward()
    g_rot = model._rotation.grad
    assert g_rot is not None and bool(torch.isfinite(g_rot).all()) and float(g_rot.abs().max()) > 0.0

    monkeypatch.setattr(grow, "branch", lambda *a, **k: grow.GROW)
    for kw in ({"features": F.detach()}, {"return_normals": True}):
        with pytest.raises(ValueError, match="grow"):
            render(cam, model, pipe, bg, **kw)
