"""Absolute-gradient densification on the HIP path (csrc/abs_grad.hip; ``GaussianRasterizer(settings, abs_grad=True)``,
``render(abs_grad=True)``, ``densify_and_prune(abs_grad_threshold=)``) against the float64 restatement
of tests/abs_grad_restate.py.

Scenes: those of tests/test_gpu_features.py (`small`, `big`, `behind`, `stacked`): partial tiles (72x40, 40x24), Gaussians
spanning several tiles, early-terminated pixels, a tile list past one 256-entry round (`stacked`, 720 entries), culled rows
(`behind`).

Bar.  The loss weights are zero on the pixels whose float64 oracle margin does not clear grad_util.MARGIN.  Per component,
normalised by the column's largest value: max(1e-5, 2 x the float32 restatement's own error against float64), the bar of
tests/test_gpu_features.py.  The observed figures are printed by every test (run with -s).
"""
import copy
import math
import types

import pytest
import torch
from torch import nn

import abs_grad_restate as R
from depth_restate import assert_rounds_covered
from gpu_util import product_settings
from grad_util import TOL, weighted_sum

pytestmark = pytest.mark.gpu
ALL_SCENES = ("small", "big", "behind", "stacked")
GRADS = ("xyz", "opacity", "scaling", "rotation", "f_dc", "f_rest", "means2D")


def _run(dev, name, bg_name="black", abs_grad=True, model=None):
    """One frame of the operator and the backward of the frame's weighted-sum loss -> dict(color, radii, grads, abs)."""
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    fr = R.oracle_frame(name)
    scene_model = fr["model"] if model is None else model
    bg = torch.tensor(R.BACKGROUNDS[bg_name], dtype=torch.float32)
    st = product_settings(fr["cam"], bg, 3, dev)
    leaves = {k: getattr(scene_model, a).detach().to(dev).requires_grad_(True)
              for k, a in (("xyz", "_xyz"), ("opacity", "_opacity"), ("scaling", "_scaling"), ("rotation", "_rotation"),
                           ("f_dc", "_features_dc"), ("f_rest", "_features_rest"))}
    P = int(leaves["xyz"].shape[0])
    leaves["means2D"] = torch.zeros(P, 3, device=dev, requires_grad=True)
    kw = dict(means3D=leaves["xyz"], means2D=leaves["means2D"], opacities=torch.sigmoid(leaves["opacity"]),
              shs=torch.cat((leaves["f_dc"], leaves["f_rest"]), dim=1), scales=torch.exp(leaves["scaling"]),
              rotations=torch.nn.functional.normalize(leaves["rotation"]))
    m2abs = None
    if abs_grad:
        m2abs = torch.zeros(P, 3, device=dev, requires_grad=True)
        color, radii = GaussianRasterizer(st, abs_grad=True)(**kw, means2D_abs=m2abs)
    else:
        color, radii = GaussianRasterizer(st)(**kw)
    weighted_sum(color, fr["weights"]).backward()
    torch.cuda.synchronize()
    return dict(color=color.detach().cpu(), radii=radii.cpu(), grads={k: leaves[k].grad.cpu() for k in GRADS},
                abs=None if m2abs is None else m2abs.grad.cpu())


def _bars(name, bg_name):
    """Per component: (bar, scale, the float32 restatement's own error)."""
    a64, a32 = R.reference(name, bg_name)[torch.float64][0], R.reference(name, bg_name)[torch.float32][0]
    out = []
    for c in range(2):
        scale = float(a64[:, c].max())
        e32 = float((a32[:, c].double() - a64[:, c]).abs().max()) / scale
        out.append((max(TOL, 2.0 * e32), scale, e32))
    return out


@pytest.mark.parametrize("bg_name", list(R.BACKGROUNDS))
@pytest.mark.parametrize("name", ALL_SCENES)
def test_abs_gradient_matches_the_float64_restatement(gpu_device, name, bg_name):
    fr = R.oracle_frame(name)
    if name == "stacked":
        assert_rounds_covered(fr["aux"])
    got = _run(gpu_device, name, bg_name)
    assert torch.equal(got["radii"], fr["radii"].to(torch.int32))
    a = got["abs"]
    assert tuple(a.shape) == (int(fr["radii"].shape[0]), 3) and a.dtype == torch.float32 and bool(torch.isfinite(a).all())
    a64 = R.reference(name, bg_name)[torch.float64][0]
    for c, (bar, scale, e32) in enumerate(_bars(name, bg_name)):
        e = float((a[:, c].double() - a64[:, c]).abs().max()) / scale
        print(f"[abs_grad] {name}, bg {bg_name}, component {c}: err {e:.2e} (float32 restatement {e32:.2e}, bar {bar:.2e})")
        assert e <= bar, f"{name}, bg {bg_name}: component {c} is {e:.2e} off the float64 restatement, bar {bar:.2e}"


@pytest.mark.parametrize("name", ALL_SCENES)
def test_abs_dominates_the_signed_gradient_and_zeros_are_exact(gpu_device, name):
    fr = R.oracle_frame(name)
    got = _run(gpu_device, name, "coloured")
    a, g = got["abs"], got["grads"]["means2D"]
    for c, (bar, scale, _) in enumerate(_bars(name, "coloured")):
        short = float((g[:, c].abs() - a[:, c]).max())
        print(f"[abs_grad] {name}, component {c}: largest |signed| - abs = {short:.3e} (allowed {bar * scale:.3e})")
        assert short <= bar * scale
    assert float(a[:, 2].abs().max()) == 0.0, "the z column is exactly zero"
    culled = got["radii"] == 0
    assert float(a[culled].abs().max() if bool(culled.any()) else 0.0) == 0.0, "rows with radii == 0 are exactly zero"
    assert bool((a >= 0).all()) and float(a.max()) > 0.0
    if name == "behind":
        assert all(bool(culled[i]) for i in R.BEHIND)


@pytest.mark.parametrize("name", ["small", "stacked"])
def test_the_colour_path_is_untouched(gpu_device, name):
    on, off = _run(gpu_device, name, "coloured", abs_grad=True), _run(gpu_device, name, "coloured", abs_grad=False)
    assert torch.equal(on["color"], off["color"]) and torch.equal(on["radii"], off["radii"])
    for k in GRADS:
        assert torch.equal(on["grads"][k], off["grads"][k]), f"dL/d{k} changed with abs_grad=True"


def test_empty_frame_and_reproducibility(gpu_device):
    fr = R.oracle_frame("small")
    away = copy.deepcopy(fr["model"])
    away._xyz = away._xyz.clone()
    away._xyz[:, 2] = -5.0                       # every Gaussian behind the camera: not a single instance
    got = _run(gpu_device, "small", "coloured", model=away)
    assert int((got["radii"] != 0).sum()) == 0 and float(got["abs"].abs().max()) == 0.0
    assert tuple(got["abs"].shape) == tuple(got["grads"]["means2D"].shape)
    a, b = _run(gpu_device, "stacked", "coloured")["abs"], _run(gpu_device, "stacked", "coloured")["abs"]
    for c, (bar, scale, _) in enumerate(_bars("stacked", "coloured")):
        d = float((a[:, c] - b[:, c]).abs().max()) / scale
        print(f"[abs_grad] two runs, component {c}: {d:.2e} apart (bar {bar:.2e})")
        assert d <= bar


# ---- statistics and plan ----------------------------------------------------------------------------------------------
THR, ABS_THR, EXTENT = 0.0002, 0.0008, 1.0
#        grad      abs       big    denom  what the rule does with the row
ROWS = [(0.0001, 0.0010, True, 1.0, "split"),      # only the absolute gradient selects it
        (0.0001, 0.0010, False, 1.0, "keep"),      # small: the absolute gradient clones nothing
        (0.0003, 0.0001, True, 1.0, "split"),      # the signed rule, as before
        (0.0003, 0.0010, False, 1.0, "clone"),     # clone unchanged
        (0.0001, 0.0001, True, 1.0, "keep"),
        (0.0001, 0.0008, True, 1.0, "split"),      # abs == abs_thr: >=
        (0.0001, 0.00079, True, 1.0, "keep"),
        (0.0, 0.0, True, 0.0, "keep"),             # 0 / 0 -> NaN -> 0 on both
        (0.0004, 0.0016, True, 2.0, "split"),      # the quotients decide: 0.0002 and 0.0008
        (0.00039, 0.00159, True, 2.0, "keep")]


def _plan_model(dev, with_abs=True):
    m = types.SimpleNamespace()
    P = 3 * len(ROWS)                      # the table three times over
    rows = ROWS * 3
    g = torch.Generator().manual_seed(5)
    m.percent_dense = 0.01
    m._xyz = nn.Parameter(torch.randn(P, 3, generator=g).to(dev))
    m._features_dc = nn.Parameter(torch.randn(P, 1, 3, generator=g).to(dev))
    m._features_rest = nn.Parameter(torch.randn(P, 15, 3, generator=g).to(dev))
    m._opacity = nn.Parameter((2.0 + 0.01 * torch.arange(P, dtype=torch.float32))[:, None].to(dev))      # a row's own tag
    m._scaling = nn.Parameter(torch.tensor([[math.log(0.5 if r[2] else 0.001)] * 3 for r in rows]).to(dev))
    m._rotation = nn.Parameter(torch.randn(P, 4, generator=g).to(dev))
    m.xyz_gradient_accum = torch.tensor([[r[0]] for r in rows], device=dev)
    m.denom = torch.tensor([[r[3]] for r in rows], device=dev)
    m.max_radii2D = torch.zeros(P, device=dev)
    if with_abs:
        m.xyz_gradient_accum_abs = torch.tensor([[r[1]] for r in rows], device=dev)
    return m, rows


def test_plan_splits_exactly_the_restated_set(gpu_device):
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR, densify_and_prune
    m, rows = _plan_model(gpu_device)
    tags = m._opacity.detach().cpu()[:, 0]
    want = {k: {int(i) for i, r in enumerate(rows) if r[4] == k} for k in ("split", "clone", "keep")}
    noise = torch.randn(2 * len(want["split"]), 3, generator=torch.Generator().manual_seed(9)).to(gpu_device)
    info = densify_and_prune(m, THR, 0.005, EXTENT, None, noise=noise, abs_grad_threshold=ABS_THR)
    n_keep, n_clone, n_child = info["kept"], info["cloned"], info["children_per_copy"]
    assert info["split_selected"] == n_child == len(want["split"]) and n_clone == len(want["clone"])
    assert n_keep == len(want["keep"]) + len(want["clone"]) and info["points"] == n_keep + n_clone + 2 * n_child
    out = m._opacity.detach().cpu()[:, 0]
    row_of = lambda v: int(torch.nonzero(tags == v)[0])      # noqa: E731
    assert {row_of(v) for v in out[:n_keep]} == want["keep"] | want["clone"]
    assert {row_of(v) for v in out[n_keep:n_keep + n_clone]} == want["clone"]
    first = [row_of(v) for v in out[n_keep + n_clone:n_keep + n_clone + n_child]]
    assert set(first) == want["split"] and first == [row_of(v) for v in out[n_keep + n_clone + n_child:]]
    for a in ("xyz_gradient_accum", "denom", "xyz_gradient_accum_abs"):
        t = getattr(m, a)
        assert tuple(t.shape) == (info["points"], 1) and float(t.abs().max()) == 0.0, a
    # None, and a threshold nothing reaches, are the existing call bit for bit under the same noise
    base, _ = _plan_model(gpu_device, with_abs=False)
    n_sel = sum(1 for r in rows if r[0] / max(r[3], 1e-30) >= THR and r[2] and r[3] > 0)
    noise = torch.randn(2 * n_sel, 3, generator=torch.Generator().manual_seed(10)).to(gpu_device)
    densify_and_prune(base, THR, 0.005, EXTENT, None, noise=noise)
    for thr in (None, math.inf):
        other, _ = _plan_model(gpu_device)
        densify_and_prune(other, THR, 0.005, EXTENT, None, noise=noise, abs_grad_threshold=thr)
        for a in GROUP_ATTR.values():
            assert torch.equal(getattr(other, a).detach(), getattr(base, a).detach()), (thr, a)


def test_statistics_after_one_frame(gpu_device):
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.losses import add_densification_stats
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    fr = R.oracle_frame("small")
    cam = copy.deepcopy(fr["cam"]).to(gpu_device)
    bg = torch.tensor(R.BACKGROUNDS["coloured"], device=gpu_device)
    models = []
    for abs_grad in (True, False):
        model = copy.deepcopy(fr["model"]).to(gpu_device)
        for p in model.parameters():
            p.requires_grad_(True)
        pkg = render(cam, model, PipelineParams(), bg, **({"abs_grad": True} if abs_grad else {}))
        assert ("viewspace_points_abs" in pkg) == abs_grad
        weighted_sum(pkg["render"], fr["weights"]).backward()
        add_densification_stats(model, pkg["viewspace_points"], pkg["radii"],
                                **({"viewspace_abs": pkg["viewspace_points_abs"]} if abs_grad else {}))
        models.append((model, pkg))
    (on, pkg), (off, _) = models
    vis = pkg["radii"] > 0
    want = torch.where(vis, pkg["viewspace_points_abs"].grad[:, :2].double().norm(dim=1), torch.zeros((), dtype=torch.float64,
                                                                                                      device=gpu_device))
    got = on.xyz_gradient_accum_abs
    assert tuple(got.shape) == (int(vis.shape[0]), 1) and float(got.max()) > 0.0
    assert float(got[~vis].abs().max() if bool((~vis).any()) else 0.0) == 0.0
    # sqrt(fma(x, x, y * y)) in float32: three roundings, 1e-6 relative is ample and no more
    assert float(((got[:, 0].double() - want).abs() / want.clamp(min=1e-30)).max()) <= 1e-6
    for a in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(getattr(on, a), getattr(off, a)), f"{a} changed with the abs tensor"
    assert getattr(off, "xyz_gradient_accum_abs", None) is None


# ---- the training loop ------------------------------------------------------------------------------------------------
def _trainable(dev, opt, **model_kw):
    from mvs_gaussian_splatting_amd import GaussianModel
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    fr = R.oracle_frame("small")
    src = fr["model"]
    m = GaussianModel(3, **model_kw)
    torch.manual_seed(0)
    m.create_from_pcd(src._xyz.to(dev), torch.rand(src._xyz.shape[0], 3).to(dev), 1.0)
    for a in GROUP_ATTR.values():
        setattr(m, a, nn.Parameter(getattr(src, a).detach().clone().to(dev).requires_grad_(True)))
    m.training_setup(opt)
    return m


def test_training_iterations_across_a_densification(gpu_device, tmp_path):
    from mvs_gaussian_splatting_amd import GaussianModel
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import (OptimizationParams, load_checkpoint, save_checkpoint,
                                                    training_iteration)
    from conftest import small_scene
    fr = R.oracle_frame("small")
    cam = copy.deepcopy(fr["cam"]).to(gpu_device)
    target = small_scene(**R.SCENES["small"])[3].to(gpu_device)
    bg = torch.zeros(3, device=gpu_device)
    over = dict(iterations=30, position_lr_max_steps=30, densify_from_iter=1, densification_interval=2,
                densify_until_iter=10, densify_abs_grad_threshold=1e-9)
    opt = OptimizationParams(abs_grad=True, **over)
    m = _trainable(gpu_device, opt)
    assert tuple(m.xyz_gradient_accum_abs.shape) == (m._xyz.shape[0], 1)
    pipe = PipelineParams()
    pipe.fuse_densify_stats = True           # not honoured on an abs_grad frame
    sizes = []
    for it in (1, 2, 3):
        torch.manual_seed(it)
        print(f"[abs_grad] iteration {it}: {int(m._xyz.shape[0])} Gaussians, accumulators "
              f"{[(tuple(getattr(m, a).shape), getattr(m, a).dtype) for a in ('xyz_gradient_accum', 'denom', 'max_radii2D')]}")
        loss = training_iteration(m, cam, opt, pipe, bg, it, cameras_extent=1.0, gt_image=target)
        assert bool(torch.isfinite(loss))
        sizes.append(int(m._xyz.shape[0]))
        if it == 1:
            assert float(m.xyz_gradient_accum_abs.max()) > 0.0 and float(m.denom.max()) == 1.0
        if it == 2:                          # the densification step: new row count, everything zero
            for a in ("xyz_gradient_accum", "denom", "xyz_gradient_accum_abs"):
                t = getattr(m, a)
                assert tuple(t.shape) == (sizes[-1], 1) and float(t.abs().max()) == 0.0, a
    print(f"[abs_grad] Gaussians over three iterations: {sizes}")
    assert sizes[1] > sizes[0] and sizes[2] == sizes[1]
    assert tuple(m.xyz_gradient_accum_abs.shape) == (sizes[2], 1) and float(m.xyz_gradient_accum_abs.max()) > 0.0
    # checkpoints: with the accumulator (13 entries) and without it (the 12 the parent writes)
    path = str(tmp_path / "with.pth")
    save_checkpoint(m, 3, path)
    assert len(m.capture()) == 13 and set(m.capture()[-1]) == {"xyz_gradient_accum_abs"}
    back = GaussianModel(3)
    assert load_checkpoint(back, path, opt) == 3
    assert torch.equal(back.xyz_gradient_accum_abs, m.xyz_gradient_accum_abs) and torch.equal(back._xyz, m._xyz)
    assert torch.equal(back.xyz_gradient_accum, m.xyz_gradient_accum) and torch.equal(back.denom, m.denom)
    off_opt = OptimizationParams(**over)
    plain = _trainable(gpu_device, off_opt)
    training_iteration(plain, cam, off_opt, PipelineParams(), bg, 1, cameras_extent=1.0, gt_image=target)
    assert plain.xyz_gradient_accum_abs is None and len(plain.capture()) == 12
    path = str(tmp_path / "without.pth")
    save_checkpoint(plain, 1, path)
    for o in (off_opt, opt):                 # an old checkpoint restores into either kind of run
        back = GaussianModel(3)
        assert load_checkpoint(back, path, o) == 1 and torch.equal(back._xyz, plain._xyz)
        assert (back.xyz_gradient_accum_abs is None) == (o is off_opt)
    # refusals
    with pytest.raises(ValueError, match="fork"):
        training_iteration(_trainable(gpu_device, opt, grow_dir=True, num_dirs=8), cam, opt, PipelineParams(), bg, 1,
                           cameras_extent=1.0, gt_image=target)
    with pytest.raises(ValueError, match="mcmc"):
        training_iteration(_trainable(gpu_device, opt), cam, OptimizationParams(abs_grad=True, strategy="mcmc", cap_max=1000,
                                                                                **over),
                           PipelineParams(), bg, 1, cameras_extent=1.0, gt_image=target)
