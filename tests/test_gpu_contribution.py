"""Per-Gaussian contribution statistics of the HIP path (csrc/contribution.hip; GaussianRasterizer(contribution=stats),
render(contribution=stats), measure, prune_by_contribution) against the float64 restatement of
tests/contribution_restate.py.

Scenes: those of tests/test_gpu_depth.py -- `small` (P = 400 at 72x40: partial last tile row and column), `big`
(P = 3000 at 320x176: lists beyond one 256-entry round of the kernel, Gaussians with more than 64 instances; asserted on
the oracle), `behind` (Gaussians behind the camera and inside the near plane) -- and a frame without any instance.

Bars.  Against float64 the statistics are taken under a pixel mask = the oracle's robust pixels (margin >
grad_util.MARGIN); at most 5 % of the covered pixels may be left out (asserted on the oracle alone).  Under it the pixel
counts are exact; weight sums and largest weights, max-norm relative: max(1e-5, 2 x the float32 restatement's own error
against float64), the project's standing rule.  The fixed point adds at most 2^-31 per pixel to a sum, far below the
bar.  The observed figures are printed by every test (run with -s).
"""
import functools
import math
import os
import sys
import types

import pytest
import torch

from conftest import ROOT, make_settings
from depth_restate import assert_rounds_covered
from contribution_restate import members_near, stats_from_lists
from gpu_util import product_settings
from grad_util import MARGIN, TOL, linear_weights, oracle_operator_inputs, weighted_sum
from test_gpu_depth import MAX_LEFT_OUT, SCENES, _hip_leaves, _scene

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name):
    """float64 and float32 restatement of a scene under the robust-pixel mask, the float64 one without a mask, and the
    Gaussians none of whose tiles holds a fragile pixel; computed once per scene and shared, never modified."""
    from oracle import rasterize_ref
    model, cam, bg = _scene(name)
    st = make_settings(cam, bg, 3)
    P = int(model._xyz.shape[0])
    out = {}
    for dt in (torch.float64, torch.float32):
        _, xyz, m2, op, kw = oracle_operator_inputs(model, dt)
        with torch.no_grad():
            _, radii, aux = rasterize_ref(xyz, m2, op, st, want_aux=True, want_margin=True, **kw)
            lists = (aux["pre"], aux["point_list"], aux["ranges"], aux["n_contrib"], st)
            if dt == torch.float64:
                robust = aux["margin"] > MARGIN
                covered = aux["n_contrib"] > 0
                out.update(robust=robust, covered=covered, radii=radii.clone(), aux=aux, all=stats_from_lists(*lists),
                           all_robust=~members_near(aux["point_list"], aux["ranges"], aux["pre"]["grid"], ~robust, P))
            out[dt] = stats_from_lists(*lists, mask=out["robust"])
    left_out = float((out["covered"] & ~out["robust"]).sum()) / max(1, int(out["covered"].sum()))
    print(f"[contribution] scene {name}: {int(out['covered'].sum())} covered pixels, share left out of the comparison "
          f"{left_out:.4f}; {int((out['all'][1] > 0).sum())} of {P} Gaussians composited somewhere")
    assert left_out <= MAX_LEFT_OUT, f"scene {name}: the oracle alone leaves out {left_out:.3f} of the covered pixels"
    return out


def _measure(dev, name, mask=None, stats=None, aux_maps=False, model=None, cam=None):
    """One getter-fed frame of the scene with ``contribution=stats``: -> (stats, leaves, operator outputs)."""
    from mvs_gaussian_splatting_amd import ContributionStats, GaussianRasterizer
    scene_model, scene_cam, bg = _scene(name)
    model, cam = (scene_model, scene_cam) if model is None else (model, cam)
    st = product_settings(cam, bg, 3, dev)
    leaves, kw = _hip_leaves(dev, model, False)
    if stats is None:
        stats = ContributionStats(int(model._xyz.shape[0]), dev)
    out = GaussianRasterizer(st, aux_maps=aux_maps, contribution=stats, contribution_mask=mask)(**kw)
    return stats, leaves, out


def _compare(stats, ref, label, rows=None):
    """count exact; weight_sum and max_weight at the bar, over ``rows`` (default: every Gaussian)."""
    (s64, c64, m64), (s32, _, m32) = ref[torch.float64], ref[torch.float32]
    rows = torch.ones_like(c64, dtype=torch.bool) if rows is None else rows
    count = stats.pixel_count().cpu()
    wrong = torch.nonzero((count != c64) & rows).reshape(-1)
    assert wrong.numel() == 0, (f"{label}: pixel counts differ from the float64 restatement at Gaussians "
                                f"{wrong[:8].tolist()}: {count[wrong[:8]].tolist()} vs {c64[wrong[:8]].tolist()}")
    report = []
    for what, got, r64, r32 in (("weight_sum", stats.weight_sum().cpu(), s64, s32),
                                ("max_weight", stats.max_weight().cpu().double(), m64, m32)):
        scale = float(r64[rows].abs().max())
        e = float((got - r64)[rows].abs().max()) / scale
        e32 = float((r32.double() - r64)[rows].abs().max()) / scale
        bar = max(TOL, 2.0 * e32)
        report.append(f"{what}: err {e:.2e} (float32 restatement {e32:.2e}, bar {bar:.2e})")
        assert e <= bar, f"{label}: {what} is {e:.2e} off the float64 restatement, bar {bar:.2e}"
    print(f"[contribution] {label}: counts exact over {int(rows.sum())} Gaussians ({int(c64[rows].sum())} pixels); "
          + "; ".join(report))


@pytest.mark.parametrize("name", ["small", "big", "behind", "stacked"])
def test_statistics_match_the_float64_restatement_on_the_robust_pixels(gpu_device, name):
    ref = _reference(name)
    if name == "stacked":
        assert_rounds_covered(ref["aux"])
    if name == "big":
        aux = ref["aux"]
        assert int((aux["ranges"][:, 1] - aux["ranges"][:, 0]).max()) > 256, "a list must exceed one 256-entry round"
        assert int(aux["n_contrib"].max()) > 256, "a pixel must composite past the first round"
        assert int(aux["pre"]["tiles_touched"].max()) > 64, "a Gaussian must have more than 64 instances"
    mask = ref["robust"].to(torch.uint8).to(gpu_device)
    stats, _, (_, radii) = _measure(gpu_device, name, mask=mask)
    assert stats.views == 1 and stats.raw.dtype == torch.int64 and tuple(stats.raw.shape) == (ref["radii"].numel(), 3)
    assert torch.equal(radii.cpu(), ref["radii"].to(torch.int32))
    assert int(ref[torch.float64][1].sum()) > 1000, "the scene must composite a good number of pixels"
    _compare(stats, ref, name)
    raw = stats.raw.cpu()
    assert int(raw[ref["radii"] == 0].abs().sum()) == 0, "a Gaussian that was culled has statistics"
    assert name == "big" or int((ref["radii"] == 0).sum()) > 0
    if name == "behind":
        assert int(raw[[3, 17, 101]].abs().sum()) == 0 and bool((ref["radii"][[3, 17, 101]] == 0).all())
    assert bool(((raw[:, 2] > 0) == (raw[:, 1] > 0)).all()) and bool(((raw[:, 0] > 0) == (raw[:, 1] > 0)).all())
    assert float(stats.max_weight().max()) <= 0.99


@pytest.mark.parametrize("name", ["small", "big"])
def test_runs_are_bit_equal_and_views_add_up(gpu_device, name):
    from mvs_gaussian_splatting_amd import ContributionStats
    from conftest import small_scene
    a1, _, _ = _measure(gpu_device, name)
    a2, _, _ = _measure(gpu_device, name)
    assert int(a1.raw[:, 1].sum()) > 1000
    assert torch.equal(a1.raw, a2.raw), "two runs of one frame differ"
    H, W = SCENES[name]["height"], SCENES[name]["width"]
    ones, _, _ = _measure(gpu_device, name, mask=torch.ones(H, W, dtype=torch.uint8, device=gpu_device))
    assert torch.equal(ones.raw, a1.raw), "an all-ones mask and no mask differ"
    half = torch.ones(H, W, dtype=torch.uint8, device=gpu_device)
    half[:, W // 2:] = 0
    left, _, _ = _measure(gpu_device, name, mask=half)
    right, _, _ = _measure(gpu_device, name, mask=1 - half)
    assert torch.equal(left.raw[:, :2] + right.raw[:, :2], a1.raw[:, :2]), "the two halves of the image do not add up"
    assert torch.equal(torch.maximum(left.raw[:, 2], right.raw[:, 2]), a1.raw[:, 2])
    # a second view into the same buffer == (add, add, max) of two buffers of their own
    model_b, cam_b, _, _ = small_scene(**SCENES[name], view=1)
    b, _, _ = _measure(gpu_device, name, model=model_b, cam=cam_b)
    assert not torch.equal(b.raw, a1.raw), "the second view must see the scene differently"
    both, _, _ = _measure(gpu_device, name)
    _measure(gpu_device, name, stats=both, model=model_b, cam=cam_b)
    assert both.views == 2
    expected = torch.stack((a1.raw[:, 0] + b.raw[:, 0], a1.raw[:, 1] + b.raw[:, 1], torch.maximum(a1.raw[:, 2], b.raw[:, 2])),
                           dim=1)
    assert torch.equal(both.raw, expected)
    merged = ContributionStats(a1.raw.shape[0], gpu_device).merge(a1).merge(b)
    assert torch.equal(merged.raw, both.raw) and merged.views == 2


@pytest.mark.parametrize("name", ["small", "big"])
def test_the_colour_path_and_the_maps_are_left_alone(gpu_device, name):
    """Colour, radii and every colour gradient with contribution=stats equal those without it bit for bit; with
    aux_maps=True as well, the maps equal the maps alone, and the statistics are the same with and without the maps."""
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    H, W = SCENES[name]["height"], SCENES[name]["width"]
    wts = linear_weights((3, H, W))
    names = ("xyz", "opacity", "f_dc", "f_rest", "scaling", "rotation", "means2D")

    def plain(aux_maps):
        model, cam, bg = _scene(name)
        leaves, kw = _hip_leaves(gpu_device, model, False)
        return leaves, GaussianRasterizer(product_settings(cam, bg, 3, gpu_device), aux_maps=aux_maps)(**kw)

    def grads(leaves, color):
        return torch.autograd.grad(weighted_sum(color, wts), [leaves[k] for k in names], retain_graph=True)

    s1, l1, o1 = _measure(gpu_device, name)
    l0, o0 = plain(False)
    assert len(o1) == 2 and o1[0].requires_grad and not s1.raw.requires_grad
    assert torch.equal(o1[0], o0[0]) and torch.equal(o1[1], o0[1]), "colour / radii changed with contribution=stats"
    for k, a, b in zip(names, grads(l1, o1[0]), grads(l0, o0[0])):
        assert torch.equal(a, b), f"colour gradient of {k} changed with contribution=stats"
    s2, l2, o2 = _measure(gpu_device, name, aux_maps=True)
    l3, o3 = plain(True)
    assert len(o2) == 3 and torch.equal(o2[2], o3[2]), "the maps changed with contribution=stats"
    assert torch.equal(o2[0], o0[0]) and torch.equal(s2.raw, s1.raw)
    for k, a, b in zip(names, grads(l2, o2[0]), grads(l0, o0[0])):
        assert torch.equal(a, b), f"colour gradient of {k} changed with contribution=stats and aux_maps=True"
    # the weights the statistics sum are the maps': sum_g sum[g] == sum of the alpha map up to rounding.  A pixel's float32
    # alpha = 1 - T carries at most (entries walked) x 2^-24 of relative error and each w at most 2^-24 + 2^-31 / w; with
    # lists of a few hundred entries that is below 1e-5 for every pixel, hence for the sums
    total, alpha = float(s1.weight_sum().sum()), float(o3[2][2].detach().double().sum())
    print(f"[contribution] {name}: sum of the weight sums {total:.6f}, sum of the alpha map {alpha:.6f}")
    assert abs(total - alpha) <= 1e-5 * alpha


def test_frame_without_any_instance(gpu_device):
    from mvs_gaussian_splatting_amd import ContributionStats, GaussianRasterizer
    model, cam, bg = _scene("small")
    model._xyz[:, 2] = -model._xyz[:, 2].abs() - 1.0
    stats = ContributionStats(400, gpu_device)
    stats.raw.copy_(torch.arange(1200, device=gpu_device).reshape(400, 3))
    before = stats.raw.clone()
    _, kw = _hip_leaves(gpu_device, model, False)
    mask = torch.ones(40, 72, dtype=torch.uint8, device=gpu_device)
    for m in (None, mask):
        color, radii = GaussianRasterizer(product_settings(cam, bg, 3, gpu_device), contribution=stats,
                                          contribution_mask=m)(**kw)
        assert int((radii > 0).sum()) == 0
    assert torch.equal(stats.raw, before) and stats.views == 2


def test_render_fused_path_and_no_grad(gpu_device):
    """render(contribution=stats) on the raw parameters against the getter-fed operator: the pixel counts agree on the
    Gaussians none of whose tiles holds a fragile pixel (the fused activations round differently, which may flip a
    fragile decision and nothing else) and the sums there are within the bar; under the robust mask the fused path meets
    the float64 restatement like the operator; no_grad and grad mode give the same bits."""
    from mvs_gaussian_splatting_amd import ContributionStats, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    ref = _reference("small")
    unfused, _, _ = _measure(gpu_device, "small")
    model, cam, bg = _scene("small")
    model.to(gpu_device)
    cam.to(gpu_device)
    for p in model.parameters():
        p.requires_grad_(True)
    bg = bg.to(gpu_device)
    pipe = PipelineParams()
    fused = ContributionStats(400, gpu_device)
    pkg = render(cam, model, pipe, bg, contribution=fused)
    assert fused.views == 1 and pkg["render"].requires_grad and "depth" not in pkg
    plain = render(cam, model, pipe, bg)
    assert torch.equal(plain["render"], pkg["render"]) and torch.equal(plain["radii"], pkg["radii"])
    rows = ref["all_robust"] & (ref["all"][1] > 0)
    print(f"[contribution fused] {int(rows.sum())} of {int((ref['all'][1] > 0).sum())} composited Gaussians have no fragile "
          f"pixel in any of their tiles")
    assert int(rows.sum()) >= 20, "the scene must have Gaussians away from every fragile pixel"
    assert torch.equal(fused.pixel_count().cpu()[ref["all_robust"]], unfused.pixel_count().cpu()[ref["all_robust"]])
    scale = float(ref["all"][0][rows].max())
    e = float((fused.weight_sum().cpu() - unfused.weight_sum().cpu())[rows].abs().max()) / scale
    e32 = float((ref[torch.float32][0].double() - ref[torch.float64][0]).abs().max()) / float(ref[torch.float64][0].max())
    print(f"[contribution fused] weight sums, fused vs getter-fed operator: {e:.2e} (bar {max(TOL, 2.0 * e32):.2e})")
    assert e <= max(TOL, 2.0 * e32)
    mask = ref["robust"].to(torch.uint8).to(gpu_device)
    masked = ContributionStats(400, gpu_device)
    with torch.no_grad():
        pkg0 = render(cam, model, pipe, bg, contribution=masked, contribution_mask=mask, return_depth=True)
    assert torch.equal(pkg0["render"], pkg["render"]) and tuple(pkg0["alpha"].shape) == (1, 40, 72)
    _compare(masked, ref, "small, fused, no_grad, with the maps")
    again = ContributionStats(400, gpu_device)
    with torch.no_grad():
        render(cam, model, pipe, bg, contribution=again)
    assert torch.equal(again.raw, fused.raw), "no_grad and grad mode give different statistics"


def test_pruning_a_trained_model(gpu_device):
    import train as example
    from mvs_gaussian_splatting_amd import measure, prune_by_contribution, trainer
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    problem = example.make_problem(gpu_device, P=600, W=72, H=40, n_views=2)
    cams, bg, _ = problem
    opt = example.small_opt(40)
    pipe = PipelineParams()
    model = example.make_model(problem, opt)
    for iteration in (1, 2, 3):
        trainer.training_iteration(model, cams[iteration % 2], opt, pipe, bg, iteration, cameras_extent=example.CAMERAS_EXTENT)

    def renders():
        with torch.no_grad():
            return [trainer.render(c, model, pipe, bg)["render"].clone() for c in cams]

    def snapshot():
        snap = {a: getattr(model, a).detach().clone() for a in GROUP_ATTR.values()}
        for group in model.optimizer.param_groups:
            state = model.optimizer.state[group["params"][0]]
            snap["m:" + group["name"]], snap["v:" + group["name"]] = state["exp_avg"].clone(), state["exp_avg_sq"].clone()
        return snap

    def assert_rows(snap, keep):
        for a in GROUP_ATTR.values():
            assert torch.equal(getattr(model, a).detach(), snap[a][keep]), a
        for group in model.optimizer.param_groups:
            state = model.optimizer.state[group["params"][0]]
            assert torch.equal(state["exp_avg"], snap["m:" + group["name"]][keep]), group["name"]
            assert torch.equal(state["exp_avg_sq"], snap["v:" + group["name"]][keep]), group["name"]
        n = int(keep.sum())
        assert model.xyz_gradient_accum.shape[0] == model.denom.shape[0] == model.max_radii2D.shape[0] == n

    # 1. dropping the Gaussians no view composited leaves the pictures as they are
    P = int(model._xyz.shape[0])
    stats = measure(model, cams, pipe, bg)
    assert stats.views == 2 and stats.raw.shape[0] == P
    never = stats.pixel_count() == 0
    assert 0 < int(never.sum()) < P, "the scene must have Gaussians no view composites, and some it does"
    before, snap = renders(), snapshot()
    assert float(before[0].max()) > 0.05
    out = prune_by_contribution(model, stats, kind="count", min_score=1)
    assert out == {"points": P - int(never.sum()), "pruned": int(never.sum())}
    assert_rows(snap, ~never)
    diff = max(float((a - b).abs().max()) for a, b in zip(renders(), before))
    print(f"[contribution prune] {out['pruned']} of {P} Gaussians never composited; largest change of a pixel {diff:.2e}")
    assert diff <= 1e-5
    # 2. keep_ratio = 0.5 keeps the rows a host-side ranking of the downloaded scores selects
    P = out["points"]
    stats = measure(model, cams, pipe, bg)
    score = stats.score("sum").cpu().tolist()
    chosen = sorted(range(P), key=lambda i: (-score[i], i))[:math.ceil(0.5 * P)]
    keep = torch.zeros(P, dtype=torch.bool)
    keep[chosen] = True
    snap = snapshot()
    out = prune_by_contribution(model, stats, kind="sum", keep_ratio=0.5)
    assert out == {"points": math.ceil(0.5 * P), "pruned": P - math.ceil(0.5 * P)}
    assert_rows(snap, keep.to(gpu_device))
    # 3. the pruned model trains on
    xyz = model._xyz.detach().clone()
    loss = trainer.training_iteration(model, cams[0], opt, pipe, bg, 4, cameras_extent=example.CAMERAS_EXTENT)
    assert math.isfinite(float(loss)) and model._xyz.shape[0] == out["points"]
    assert not torch.equal(model._xyz.detach(), xyz), "the optimizer did not step"


def test_refusals(gpu_device):
    from mvs_gaussian_splatting_amd import ContributionStats, GaussianRasterizer, _lib, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model, cam, bg = _scene("small")
    st = product_settings(cam, bg, 3, gpu_device)
    _, kw = _hip_leaves(gpu_device, model, False)
    with pytest.raises(ValueError, match="rows"):
        GaussianRasterizer(st, contribution=ContributionStats(399, gpu_device))(**kw)
    good = ContributionStats(400, gpu_device)
    for mask in (torch.ones(40, 71, dtype=torch.uint8, device=gpu_device), torch.ones(72, 40, dtype=torch.uint8, device=gpu_device),
                 torch.ones(40, 72, dtype=torch.bool, device=gpu_device)):
        with pytest.raises(ValueError, match="contribution_mask"):
            GaussianRasterizer(st, contribution=good, contribution_mask=mask)(**kw)
    with pytest.raises(_lib.GsrError):
        GaussianRasterizer(st, contribution=ContributionStats(400))(**kw)                       # statistics on the CPU
    with pytest.raises(_lib.GsrError):
        GaussianRasterizer(st, contribution=good, contribution_mask=torch.ones(40, 72, dtype=torch.uint8))(**kw)
    model.to(gpu_device)
    cam.to(gpu_device)
    split = types.SimpleNamespace(learn_split_distance=True, learn_split_scale=False)
    opt = types.SimpleNamespace(densify_from_iter=500, densification_interval=100, densify_until_iter=15000,
                                opacity_reset_interval=3000)
    with pytest.raises(ValueError, match="grow / learned-split"):
        render(cam, model, PipelineParams(), bg.to(gpu_device), iteration=1, opt=opt, modelcg=split, contribution=good)
    assert good.views == 0 and int(good.raw.abs().sum()) == 0, "a refused request must leave the statistics alone"
