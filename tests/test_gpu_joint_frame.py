"""The frame the trainer issues -- the colour node and the four map nodes over ONE rasterised frame, all in one backward --
against the joint float64 reference of tests/joint_restate.py.

The map nodes (rasterizer.py: ``_AuxMaps``, ``_FeatureMaps``, ``_DistortionMap``, ``_MedianDepth``) own no state: they read the
colour node's ``geom`` / ``binning`` / ``img`` / ``radii`` workspaces by reference and return gradients of their own, which autograd
sums.  Each node alone is compared with float64 in tests/test_gpu_{parity,depth,features,distortion,median}.py; here the
contract between them is: the workspaces are read-only after the forward, the gradients add up in any backward order, and
frames issued between a frame's forward and its backward do not disturb it.

Scenes: ``small`` (P = 400 at 72x40, partial last tile column and row) and ``big`` (P = 3000 at 320x176, lists longer than
one 256-entry round) of tests/median_restate.py -- what can go wrong here is bookkeeping between nodes, not throughput.

Bar, everywhere: grad_util.compare_grads -- per tensor, max-norm relative, max(1e-5, 2 x the float32 restatement's own error),
never above 2e-4.  tests/test_joint_frame_host.py asserts on the CPU that the reference meets its own caps.  The loss is
``sum_t c_t term_t`` with ``c_t = 1 / max|d term_t / d xyz|`` from the float64 reference, so that no term hides under another.
Every test prints the figures it observed (run with -s).

Determinism, from the kernels: the colour backward (``render_bwd``) has no atomics and is compared bit for bit.  The four map
backwards all end in float atomic adds (csrc/depth.hip, features.hip and distortion.hip: one per wave into the LDS sums, then
one per tile and entry into the per-Gaussian accumulator; csrc/median.hip: one per pixel into the LDS slot of the chosen entry,
then one per tile and entry), so two runs of them agree to rounding only: they are compared at the bar.

Observed on an MI355X (bar 1e-5 unless stated): joint gradient, one backward, worst tensor -- small 3.0e-6 (xyz), big 5.3e-6 (xyz,
bar 1.06e-5), small with cov3D_precomp 2.7e-6, fused path 2.9e-6 / 5.6e-6; xyz_gradient_accum 1.6e-6 / 1.7e-6; per term in the
three orders at most 0.55 of the bar, except d aux / d scaling on `big`, 4.8e-6 to 9.7e-6: float32 rounding of a cancelling sum
(the float32 restatement is 3.1e-6 off; the same backward without the coefficient lands at 2.8e-6, with it at 6.7e-6 to 9.7e-6
in 30 repetitions, whatever ran before it and whatever the allocator's free blocks held); the float-atomic nodes differ
between orders by at most 4.9e-6 (that tensor; 7e-7 otherwise); with frames in between 2.9e-6; the trainer against the
hand-built loss 2.7e-9 (xyz), 1.9e-8 (rotation), and the three terms move the position gradient by 4.1e-2, 2.7e-2 and 5.1e-5.
"""
import math
import os
import sys

import pytest
import torch

from conftest import ROOT, small_scene
from gpu_util import product_settings
from grad_util import TOL, compare_grads, linear_weights, weighted_sum
from joint_restate import MAPPING, TERMS, bar_of, joint_loss, joint_reference, normal_rows, present, term_losses
from median_restate import SCENES, scene

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu

DETERMINISTIC = ("colour",)         # nodes whose backward is atomic-free (module docstring)
ALL_MAPS = dict(return_depth=True, return_normals=True, return_distortion=True, return_median_depth=True)
FUSED = {"xyz": "_xyz", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation", "f_dc": "_features_dc",
         "f_rest": "_features_rest"}


def _label(name, use_cov=False):
    return name + (", cov3D_precomp" if use_cov else "")


# ---- the getter-fed operator -------------------------------------------------------------------------------------------
def _hip_leaves(dev, model, use_cov, F):
    """The leaves of tests/test_gpu_distortion.py and the user feature rows."""
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
    leaf("F", F)
    return leaves, dict(means3D=xyz, means2D=leaves["means2D"], opacities=torch.sigmoid(op), **kw)


def _getter_frame(dev, name, use_cov=False):
    """-> (leaves, (color, radii, aux, feat, dist, median, median_id), the five un-weighted losses)."""
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    ref = joint_reference(name, use_cov)
    model, cam, bg = scene(name)
    st = product_settings(cam, bg, 3, dev)
    leaves, kw = _hip_leaves(dev, model, use_cov, ref["F"])
    rows = torch.cat((leaves["F"], normal_rows(model, kw, leaves["xyz"], st, torch.float32)), dim=1)
    out = GaussianRasterizer(st, aux_maps=True, distortion=dict(mapping=MAPPING), median_depth=True)(features=rows, **kw)
    assert len(out) == 7
    color, radii, aux, feat, dist, median, _ = out
    return leaves, out, term_losses(color, aux, feat, dist, median, ref["weights"])


@pytest.mark.parametrize("name,use_cov", [("small", False), ("big", False), ("small", True)],
                         ids=["small", "big", "small-cov3D"])
def test_joint_gradient_of_one_backward_on_the_getter_path(gpu_device, name, use_cov):
    """(a) One ``backward()`` of ``sum_t c_t term_t`` through the five nodes: every leaf gradient, ``means2D.grad`` and ``F.grad``
    against the joint float64 sum."""
    ref = joint_reference(name, use_cov)
    r64, r32 = ref[torch.float64]["joint"], ref[torch.float32]["joint"]
    leaves, out, losses = _getter_frame(gpu_device, name, use_cov)
    assert torch.equal(out[1].cpu(), ref["radii"].to(torch.int32))
    joint_loss(losses, ref["coef"]).backward()
    for k in ref["names"]:
        assert leaves[k].grad is not None, f"{k} received no gradient from the joint frame"
    got = {k: leaves[k].grad.detach().cpu() for k in ref["names"]}
    compare_grads(got, r64, r32, f"joint frame, {_label(name, use_cov)}, getter path, one backward")
    assert float(got["means2D"][:, 2].abs().max()) == 0.0, "means2D.grad[:, 2] must be exactly 0"
    assert float(got["means2D"][:, :2].abs().max()) > 0.0
    # F enters the feature node alone: its gradient is the feature term's, times its coefficient
    f64, f32 = (ref[dt]["terms"]["features"]["F"] * ref["coef"]["features"] for dt in (torch.float64, torch.float32))
    compare_grads({"F": got["F"]}, {"F": f64}, {"F": f32}, f"joint frame, {_label(name, use_cov)}, getter path, F")


# ---- the fused raw-parameter path through render -------------------------------------------------------------------------
def _fused_model(dev, name):
    model, cam, bg = scene(name)
    model.to(dev)
    cam.to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    return model, cam, bg.to(dev)


def _pkg_losses(pkg, weights):
    return term_losses(pkg["render"], torch.cat((pkg["depth"], pkg["invdepth"], pkg["alpha"]), dim=0),
                       torch.cat((pkg["features"], pkg["normal"]), dim=0), pkg["distortion"], pkg["median_depth"], weights)


def _fused_grads(model, pkg, F):
    """{name: gradient on the CPU, None where there is none} of the raw parameters, ``viewspace_points`` and ``F``."""
    got = {k: getattr(model, attr).grad for k, attr in FUSED.items()}
    got.update(means2D=pkg["viewspace_points"].grad, F=F.grad)
    return {k: (None if g is None else g.detach().cpu()) for k, g in got.items()}


@pytest.mark.parametrize("name", ["small", "big"])
def test_joint_gradient_statistics_and_maps_on_the_fused_path(gpu_device, name):
    """(a) ``render`` with every map on the raw parameters: the parameter gradients and ``viewspace_points.grad`` against the
    joint float64 sum, the densification statistics taken from the summed gradient, and the forward maps bit for bit those
    of five single-request frames."""
    from mvs_gaussian_splatting_amd import add_densification_stats, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    dev = gpu_device
    ref = joint_reference(name)
    r64, r32 = ref[torch.float64]["joint"], ref[torch.float32]["joint"]
    model, cam, bg = _fused_model(dev, name)
    pipe = PipelineParams()
    F = ref["F"].to(dev).requires_grad_(True)
    pkg = render(cam, model, pipe, bg, features=F, **ALL_MAPS)
    assert not getattr(pkg["viewspace_points"], "_gsr_stats_fused", False)
    joint_loss(_pkg_losses(pkg, ref["weights"]), ref["coef"]).backward()
    got = _fused_grads(model, pkg, F)
    for k in ref["names"]:
        assert got[k] is not None, f"{k} received no gradient from the joint frame"
    compare_grads(got, r64, r32, f"joint frame, {name}, fused path, one backward")
    assert float(got["means2D"][:, 2].abs().max()) == 0.0

    # the densification statistics of such a frame are read from the SUMMED viewspace gradient
    radii = pkg["radii"]
    add_densification_stats(model, pkg["viewspace_points"], radii)
    want, want32 = (r["means2D"][:, :2].norm(dim=1).double() for r in (r64, r32))
    acc = model.xyz_gradient_accum.detach().cpu().double().reshape(-1)
    hip_vis = (radii > 0).cpu()
    vis = hip_vis & (ref["radii"] > 0)
    scale = float(want.abs().max())
    e, e32 = float((acc - want)[vis].abs().max()) / scale, float((want32 - want)[vis].abs().max()) / scale
    print(f"[joint densify stats] {name}: xyz_gradient_accum err {e:.2e} (float32 restatement {e32:.2e}, bar "
          f"{max(TOL, 2.0 * e32):.2e}); {int((hip_vis != (ref['radii'] > 0)).sum())} radii > 0 differ from the oracle's")
    assert e <= max(TOL, 2.0 * e32) <= 2e-4
    assert float(acc[~hip_vis].abs().max() if bool((~hip_vis).any()) else 0.0) == 0.0
    assert torch.equal(model.denom.detach().cpu().reshape(-1), hip_vis.float()), "denom must equal radii > 0"

    # the forward maps of the joint frame: those of five single-request frames, bit for bit
    Fd = F.detach()
    singles = {"colour": render(cam, model, pipe, bg), "aux": render(cam, model, pipe, bg, return_depth=True),
               "features": render(cam, model, pipe, bg, features=Fd, return_normals=True),
               "distortion": render(cam, model, pipe, bg, return_distortion=True),
               "median": render(cam, model, pipe, bg, return_median_depth=True)}
    keys = {"colour": (), "aux": ("depth", "invdepth", "alpha"), "features": ("features", "normal"),
            "distortion": ("distortion",), "median": ("median_depth", "median_id")}
    for t, single in singles.items():
        for k in ("render", "radii") + keys[t]:
            assert torch.equal(single[k], pkg[k]), f"{name}: {k} of the joint frame differs from the {t}-only frame's"
        assert set(single) == {"render", "viewspace_points", "visibility_filter", "radii", "selected_pts_mask"} | set(keys[t])


# ---- additivity and backward order -----------------------------------------------------------------------------------
ORDERS = {"forward order": TERMS, "reverse order": TERMS[::-1], "colour first, then the maps": TERMS[:1] + TERMS[:0:-1]}


@pytest.mark.parametrize("name", ["small", "big"])
def test_per_term_gradients_add_up_in_any_backward_order_and_leave_the_workspaces_alone(gpu_device, name):
    """(b) Fifteen backwards over one frame: per term and per order the gradient meets the term's own float64 reference;
    the colour node's is the same bits in every order, the float-atomic nodes' agree at the bar; a term sends nothing to
    an input it does not depend on; and afterwards the colour node's saved workspaces are the bytes they were after the
    forward."""
    ref = joint_reference(name)
    names = ref["names"]
    leaves, out, losses = _getter_frame(gpu_device, name)
    saved = out[0].grad_fn.saved_tensors[-4:]           # radii, geom, binning, img: as rasterizer._frame_of reads them
    before = [t.clone() for t in saved]
    refs = {t: tuple({k: g * ref["coef"][t] for k, g in present(ref[dt]["terms"][t]).items()}
                     for dt in (torch.float64, torch.float32)) for t in TERMS}
    runs = {}
    for order, terms in ORDERS.items():
        assert sorted(terms) == sorted(TERMS)
        for t in terms:
            got = torch.autograd.grad(ref["coef"][t] * losses[t], [leaves[k] for k in names], retain_graph=True,
                                      allow_unused=True)
            got = dict(zip(names, got))
            g64, g32 = refs[t]
            compare_grads({k: got[k].detach().cpu() for k in g64}, g64, g32, f"joint frame, {name}, {t} alone, {order}")
            for k in names:
                if k not in g64:
                    assert got[k] is None or float(got[k].abs().max()) == 0.0, f"{k} received a gradient from the {t} term"
            runs[order, t] = {k: got[k].detach() for k in g64}
    first = next(iter(ORDERS))
    for t in TERMS:
        g64, g32 = refs[t]
        rows = []
        for order in list(ORDERS)[1:]:
            for k in g64:
                a, b = runs[first, t][k], runs[order, t][k]
                if t in DETERMINISTIC:
                    assert torch.equal(a, b), f"{name}: {k} of the {t} term differs between {first} and {order}"
                else:
                    bar, _ = bar_of(g64[k], g32[k])
                    e = float((a.double() - b.double()).abs().max()) / float(g64[k].abs().max())
                    rows.append(f"{k} {e:.1e}")
                    assert e <= bar, f"{name}: {k} of the {t} term differs by {e:.2e} between {first} and {order}"
        print(f"[joint orders] {name}, {t}: " + ("bit-identical in the three orders" if t in DETERMINISTIC else
                                                  "against the first order: " + ", ".join(rows)))
    # additivity: the per-term results of one order sum to the joint reference
    total = {k: sum(runs[first, t][k].double().cpu() for t in TERMS if k in runs[first, t]) for k in names}
    compare_grads(total, ref[torch.float64]["joint"], ref[torch.float32]["joint"], f"joint frame, {name}, sum of the five terms")
    for what, a, b in zip(("radii", "geom", "binning", "img"), out[0].grad_fn.saved_tensors[-4:], before):
        assert torch.equal(a, b), f"{name}: the {what} workspace changed during the backwards"
    print(f"[joint workspaces] {name}: radii, geom, binning, img ({sum(t.numel() * t.element_size() for t in before)} "
          f"bytes) unchanged after {len(ORDERS) * len(TERMS)} backwards")


# ---- frames in between -------------------------------------------------------------------------------------------------
def _frame_b(model, cam, bg, pipe):
    """Another training view of the same (P, W, H): forward and backward, its gradients taken without touching ``.grad``."""
    from mvs_gaussian_splatting_amd import render
    pkg = render(cam, model, pipe, bg)
    wts = linear_weights((3, SCENES["small"]["height"], SCENES["small"]["width"]), seed=733)
    return torch.autograd.grad(weighted_sum(pkg["render"], wts), model.parameters() + [pkg["viewspace_points"]])


def _sequence(dev, ref, joint, between):
    """Frame A of the ``small`` scene forward, (frames in between,) A backward.  -> (A's gradients, B's or None)."""
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model, cam, bg = _fused_model(dev, "small")
    cam_b = small_scene(**SCENES["small"], view=1)[1].to(dev)
    pipe = PipelineParams()
    F = ref["F"].to(dev).requires_grad_(True)
    pkg = render(cam, model, pipe, bg, features=F, **ALL_MAPS)
    losses = _pkg_losses(pkg, ref["weights"])
    loss = joint_loss(losses, ref["coef"]) if joint else ref["coef"]["colour"] * losses["colour"]
    g_b = None
    if between:
        g_b = _frame_b(model, cam_b, bg, pipe)
        with torch.no_grad():
            for _ in range(2):                  # the second one certainly runs in the cached forward-only workspaces
                render(cam_b, model, pipe, bg)
            render(cam_b, model, pipe, bg, return_depth=True)       # a frame that keeps its state outside autograd
    loss.backward()
    return _fused_grads(model, pkg, F), g_b


@pytest.mark.parametrize("mode", [True, "deferred"], ids=["verified", "deferred"])
def test_frames_issued_between_forward_and_backward_do_not_disturb_the_frame(gpu_device, mode):
    """(c) Between A's forward and A's backward: another view's forward and backward, two ``no_grad`` frames in the shared
    forward-only workspaces and a ``no_grad`` frame that keeps its state -- all of A's (P, W, H)."""
    from mvs_gaussian_splatting_amd import rasterizer as rz
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    dev = gpu_device
    ref = joint_reference("small")
    prev = rz.set_sync_free(mode)
    try:
        alone, _ = _sequence(dev, ref, joint=False, between=False)
        model, _, bg = _fused_model(dev, "small")
        b_alone = _frame_b(model, small_scene(**SCENES["small"], view=1)[1].to(dev), bg, PipelineParams())
        assert all(float(g.abs().max()) > 0.0 for g in b_alone), "frame B must see the scene"
        got, g_b = _sequence(dev, ref, joint=True, between=True)
        compare_grads(got, ref[torch.float64]["joint"], ref[torch.float32]["joint"],
                      f"joint frame, small, fused path, frames in between, sync-free mode {mode!r}")
        for a, b in zip(g_b, b_alone):
            assert torch.equal(a, b), "frame B's gradients differ from those of B alone"
        colour, g_b = _sequence(dev, ref, joint=False, between=True)
        for k, g in alone.items():
            if g is None:
                assert colour[k] is None, k
            else:
                assert torch.equal(colour[k], g), f"A's colour gradient of {k} differs from that of A alone"
        assert alone["F"] is None and alone["xyz"] is not None
        for a, b in zip(g_b, b_alone):
            assert torch.equal(a, b), "frame B's gradients differ from those of B alone"
        print(f"[joint frames in between] sync-free mode {mode!r}: A's colour gradients and B's gradients bit-identical to "
              f"those of the frames alone")
        if mode == "deferred":
            rz.synchronize_counts()
    finally:
        rz.set_sync_free(prev)


# ---- the trainer's wiring ------------------------------------------------------------------------------------------------
PLANE = (0.3, -0.2, 4.0)         # view-space plane z = 4 + 0.3 x - 0.2 y (the scene of test_gpu_normal_consistency.py)
FULL = dict(lambda_normal=0.05, normal_from_iter=0, depth_ratio=0.5, lambda_dist=100.0, dist_from_iter=0)
ATOMIC_FREE_GROUPS = ("f_dc", "f_rest")         # fed by the colour node alone


@pytest.fixture(scope="module")
def problem(gpu_device):
    """A 64x48 frame of 400 flat Gaussians on a tilted plane in front of the example's camera (tests/test_gpu_median.py)."""
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


def _group_grads(model):
    return {g["name"]: (None if g["params"][0].grad is None else g["params"][0].grad.detach().clone())
            for g in model.optimizer.param_groups}


def _trained(problem, opt, iteration=1):
    """One ``training_iteration`` on a fresh plane model -> (loss, the gradients at ``optimizer.step``, the keywords
    ``render`` was called with)."""
    import train as example
    from mvs_gaussian_splatting_amd import trainer
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cams, bg, _ = problem
    model = _plane_model(problem, opt)
    seen, grads = {}, {}
    real_render, real_step = trainer.render, model.optimizer.step

    def spy(*args, **kw):
        seen["kw"] = kw
        return real_render(*args, **kw)

    def step(*a, **k):
        grads.update(_group_grads(model))
        return real_step(*a, **k)
    trainer.render, model.optimizer.step = spy, step
    try:
        loss = trainer.training_iteration(model, cams[0], opt, PipelineParams(), bg, iteration,
                                          cameras_extent=example.CAMERAS_EXTENT)
    finally:
        trainer.render = real_render
    assert float(model.denom.sum()) > 0, "the densification statistics were not taken"
    return loss, grads, seen["kw"]


def test_the_trainers_loss_and_gradients_are_those_of_the_public_ops_by_hand(gpu_device, problem):
    """(d) Scaling, blending and gating of ``trainer.training_iteration`` with the three regularisers on."""
    import train as example
    from mvs_gaussian_splatting_amd import l1_dssim_loss, normal_consistency_loss, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cams, bg, _ = problem
    cam = cams[0]
    opt = example.small_opt(40, **FULL)
    loss, grads, kw = _trained(problem, opt)
    for k in ALL_MAPS:
        assert kw.get(k) is True, f"the trainer did not ask for {k}"
    assert set(grads) >= {"xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"}

    # the same loss by hand, on a copy of the model, through the public ops
    model = _plane_model(problem, opt)
    pkg = render(cam, model, PipelineParams(), bg, **ALL_MAPS)
    hand = l1_dssim_loss(pkg["render"], cam.original_image, opt.lambda_dssim)
    hand = hand + 0.05 * normal_consistency_loss(pkg["depth"], pkg["alpha"], pkg["normal"], math.tan(cam.FoVx * 0.5),
                                                 math.tan(cam.FoVy * 0.5), median=pkg["median_depth"], depth_ratio=0.5)
    hand = hand + 100.0 * pkg["distortion"].mean()
    hand.backward()
    by_hand = _group_grads(model)
    print(f"[joint trainer] loss {float(loss):.8f}, by hand {float(hand.detach()):.8f}")
    assert torch.equal(loss, hand.detach()), "the trainer's loss is not the hand-built one"
    assert set(by_hand) == set(grads)
    rows = []
    for k, g in grads.items():
        assert g is not None and by_hand[k] is not None and bool(torch.isfinite(g).all()), k
        if k in ATOMIC_FREE_GROUPS:
            assert torch.equal(g, by_hand[k]), f"group {k}: fed by the colour node alone, must be the same bits"
            continue
        # float atomics in the map backwards: run-to-run reproducibility, the floor of grad_util.compare_grads (there is
        # no float32 restatement of this scene that could open it further)
        e = float((g.double() - by_hand[k].double()).abs().max()) / float(by_hand[k].abs().max())
        rows.append(f"{k} {e:.1e}")
        assert e <= TOL, f"group {k}: the trainer's gradient is {e:.2e} off the hand-built one"
    print(f"[joint trainer] trainer vs by hand (bar {TOL:.0e}): " + ", ".join(rows) + "; f_dc, f_rest bit-identical")

    # every regularising term moves the gradient: without it the position gradient is another, by more than the bar
    scale = float(grads["xyz"].abs().max())
    gone = {"lambda_normal": ("return_normals", "return_median_depth", "return_depth"), "depth_ratio": ("return_median_depth",),
            "lambda_dist": ("return_distortion",)}
    for off in (dict(lambda_normal=0.0), dict(depth_ratio=0.0), dict(lambda_dist=0.0)):
        loss0, grads0, kw0 = _trained(problem, example.small_opt(40, **dict(FULL, **off)))
        assert set(ALL_MAPS) - set(kw0) == set(gone[next(iter(off))]), kw0
        moved = float((grads0["xyz"].double() - grads["xyz"].double()).abs().max()) / scale
        print(f"[joint trainer] {off}: loss {float(loss0):.8f}, the position gradient moves by {moved:.2e}")
        assert moved > TOL, f"{off}: the term does not reach the position gradient"
        assert not torch.equal(loss0, loss)

    # before normal_from_iter / dist_from_iter the frame is the plain frame: the same keywords, the same values
    late = example.small_opt(40, **dict(FULL, normal_from_iter=5, dist_from_iter=5))
    _, _, kw_late = _trained(problem, late)
    plain = example.small_opt(40)
    _, _, kw_plain = _trained(problem, plain)
    assert kw_late.pop("opt") is late and kw_plain.pop("opt") is plain
    assert kw_late == kw_plain and not set(kw_plain) & set(ALL_MAPS), (kw_late, kw_plain)
