"""The 3D smoothing filter on the device (csrc/filter3d.hip; filter3d.py): the sampling pass and the width
against the float32 restatement (tests/filter3d_restate.py) bit for bit, the fused application and its gradient against
the float64 restatement rounded once, ``render`` with a filter on both paths, and three training iterations across a
densification."""
import numpy as np
import pytest
import torch
from torch import nn

from conftest import small_scene
import filter3d_restate as R

pytestmark = pytest.mark.gpu
F = np.float32


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- sampling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257, 1000])
def test_sampling_is_the_restatements_bits(gpu_device, P, monkeypatch):
    """V in {1, 2, 3} in one launch, and V = 5 fed in chunks of two views that accumulate; both rules; twice."""
    from mvs_gaussian_splatting_amd import compute_3d_filter, filter3d
    for V, chunk in ((1, None), (2, None), (3, None), (5, 2)):
        xyz, cams = R.gate_scene(P, V)
        dev_xyz = torch.from_numpy(xyz).to(gpu_device)
        monkeypatch.setattr(filter3d, "VIEW_CHUNK", chunk or filter3d.MAX_VIEWS)
        min_depth, max_rate, seen = R.sample(xyz, cams)
        if P >= 257:
            assert 0 < seen.sum() < P, "points on both sides of the gates"
        for rule in ("mip_splatting", "paper"):
            want, want_flag = R.width(min_depth, max_rate, seen, cams, rule=rule)
            out = torch.full((P,), float("nan"), device=gpu_device)
            got, flag = compute_3d_filter(dev_xyz, cams, rule=rule, out=out)
            again, flag2 = compute_3d_filter(dev_xyz, cams, rule=rule)
            assert got is out and got.dtype == torch.float32 and flag.dtype == torch.int32 and tuple(flag.shape) == (1,)
            assert np.array_equal(bits(got), want.view(np.uint32)), (V, rule)
            assert np.array_equal(bits(again), bits(got)) and int(flag) == int(flag2) == want_flag, (V, rule)


def test_sampling_arrays_boundaries_and_the_unseen(gpu_device):
    """Through the entry points themselves, into arrays full of garbage: the three per-Gaussian values, the dyadic
    boundary case (z == near out; u == -m W and u == (1 + m) W in), a table that sees nothing, and P = 0."""
    from mvs_gaussian_splatting_amd import _lib, compute_3d_filter, filter3d
    lib, dev = _lib.load(), gpu_device
    cam = R.camera(64, 32, 32.0, 32.0)
    xyz = np.array([[0.0, 0.0, 0.25], [0.0, 0.0, 0.2500001], [-1.5, 0.0, 1.0], [1.5, 0.0, 1.0], [-1.5000001, 0.0, 1.0],
                    [1.500001, 0.0, 1.0], [0.0, -0.75, 1.0], [0.0, 0.75, 1.0], [0.0, 0.7500001, 1.0], [0.0, 0.0, -3.0],
                    [np.nan, 0.0, 1.0], [0.0, 0.0, 8.0]], dtype=F)
    want_seen = np.array([0, 1, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1], dtype=bool)
    P = len(xyz)
    rows, focal_max = filter3d.view_table([cam])
    table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
    dev_xyz = torch.from_numpy(xyz).to(dev)
    min_depth, max_rate = torch.full((P,), -7.0, device=dev), torch.full((P,), 1e9, device=dev)
    seen = torch.full((P,), 9, dtype=torch.uint8, device=dev)
    ws_bytes = lib.gsr_filter3d_workspace_bytes(P)
    ws = torch.full((ws_bytes,), 0xAB, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.gsr_filter3d_sample(dev_xyz.data_ptr(), P, table.data_ptr(), 1, 0.25, 0.25, 0, min_depth.data_ptr(),
                                       max_rate.data_ptr(), seen.data_ptr(), ws.data_ptr(), ws_bytes, stream), "sample")
    w_depth, w_rate, w_seen = R.sample(xyz, [cam], near=0.25, margin=0.25)
    assert np.array_equal(w_seen, want_seen) and np.array_equal(seen.cpu().numpy().astype(bool), want_seen)
    assert np.array_equal(bits(min_depth), w_depth.view(np.uint32)) and np.array_equal(bits(max_rate), w_rate.view(np.uint32))
    for rule in ("mip_splatting", "paper"):
        got, flag = compute_3d_filter(dev_xyz, [cam], near=0.25, margin=0.25, rule=rule)
        want, _ = R.compute(xyz, [cam], near=0.25, margin=0.25, rule=rule)
        assert int(flag) == 0 and np.array_equal(bits(got), want.view(np.uint32))
        assert (got[torch.from_numpy(~want_seen).to(dev)] == got[11]).all(), "the unseen take the farthest seen one's"
    behind = np.eye(4, dtype=F)
    behind[3, 2] = -100.0
    got, flag = compute_3d_filter(dev_xyz, [R.camera(64, 32, 32.0, 32.0, behind)] * 2, near=0.25, margin=0.25)
    assert int(flag) == 1 and not bits(got).any(), "no Gaussian seen: filter 0 everywhere and the flag"
    got, flag = compute_3d_filter(dev_xyz[:0], [cam])
    assert tuple(got.shape) == (0,) and int(flag) == 1


# ---- application ----------------------------------------------------------------------------------------------------------------
def _apply_case(n, seed=0):
    """Raw scales in [-12, 4], raw opacities in [-12, 12], filters from 0 to 10 times the scale, and rows with f = 0."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-12.0, 4.0, size=(n, 3)).astype(F)
    o = rng.uniform(-12.0, 12.0, size=(n, 1)).astype(F)
    f = (np.exp(s.astype(np.float64).mean(axis=1)) * rng.uniform(0.0, 10.0, size=n)).astype(F)
    f[::7] = 0.0
    return s, o, f, rng.standard_normal((n, 3)).astype(F), rng.standard_normal((n, 1)).astype(F)


@pytest.mark.parametrize("n", [1, 65, 257, 20000])
def test_application_and_its_gradient_against_float64(gpu_device, n):
    """Forward: at most one float32 place from the float64 restatement rounded once (two correctly rounded float64
    evaluations differ by no more: host and device exp / log1p disagree only in the last place of a double).  Backward:
    the same one-place bar on every component -- it applied to all of them: the kernel evaluates the gradient in float64
    and rounds once, so a component that is a difference of two terms loses double places, not float32 ones; the
    allowance for that is 1e-14 of the terms' magnitudes (64 double roundings), far below one float32 place."""
    from mvs_gaussian_splatting_amd import apply_3d_filter, filtered_scaling_opacity
    s, o, f, g_s, g_o = _apply_case(n, seed=n)
    dev = gpu_device
    ds, do, df = (torch.from_numpy(a).to(dev) for a in (s, o, f))
    ds.requires_grad_(True)
    do.requires_grad_(True)
    se, oe = apply_3d_filter(ds, do, df)
    assert se.shape == ds.shape and oe.shape == do.shape and se.dtype == oe.dtype == torch.float32
    want_s, want_o = R.apply(s, o, f)
    got_s, got_o = se.detach().cpu().numpy(), oe.detach().cpu().numpy()
    eq_s, eq_o = np.mean(got_s.view(np.uint32) == want_s.view(np.uint32)), np.mean(got_o.view(np.uint32) == want_o.view(np.uint32))
    print(f"[filter3d] n={n}: forward bit-equal share: scaling {eq_s:.5f}, opacity {eq_o:.5f}; "
          f"worst {R.ulps(got_s, want_s.astype(np.float64)).max():.0f} / {R.ulps(got_o, want_o.astype(np.float64)).max():.0f} places")
    assert R.ulps(got_s, want_s.astype(np.float64)).max() <= 1 and R.ulps(got_o, want_o.astype(np.float64)).max() <= 1
    zero = f == 0
    assert np.array_equal(got_s[zero].view(np.uint32), s[zero].view(np.uint32)), "f = 0 rows exactly unchanged"
    assert np.array_equal(got_o[zero].view(np.uint32), o[zero].view(np.uint32))
    torch.autograd.backward([se, oe], [torch.from_numpy(g_s).to(dev), torch.from_numpy(g_o).to(dev)])
    w_ds, w_do, cond = R.apply_bwd(s, o, f, g_s, g_o)
    got_ds, got_do = ds.grad.cpu().numpy(), do.grad.cpu().numpy().reshape(-1)
    err_s = np.abs(got_ds.astype(np.float64) - w_ds) - 1e-14 * cond
    err_o = np.abs(got_do.astype(np.float64) - w_do) - 1e-14 * np.abs(w_do)
    print(f"[filter3d] n={n}: backward worst {np.max(err_s / np.spacing(np.abs(w_ds).astype(F))):.2f} / "
          f"{np.max(err_o / np.spacing(np.abs(w_do).astype(F))):.2f} places; bit-equal share "
          f"{np.mean(got_ds == w_ds.astype(F)):.5f} / {np.mean(got_do == w_do.astype(F)):.5f}")
    assert (err_s <= np.spacing(np.abs(w_ds).astype(F))).all() and (err_o <= np.spacing(np.abs(w_do).astype(F))).all()
    assert np.array_equal(got_ds[zero].view(np.uint32), g_s[zero].view(np.uint32))
    assert np.array_equal(got_do[zero].view(np.uint32), g_o.reshape(-1)[zero].view(np.uint32))
    # the getter path's activated values are the activations of the same tensors, and the definition's to float32
    with torch.no_grad():
        scale, opacity = filtered_scaling_opacity(ds, do, df)
    assert torch.equal(scale, torch.exp(se.detach())) and torch.equal(opacity, torch.sigmoid(oe.detach()))
    d_scale, d_opacity = R.apply_direct(s, o, f)
    assert np.allclose(scale.cpu().numpy(), d_scale, rtol=2e-6, atol=0)
    assert np.allclose(opacity.cpu().numpy().reshape(-1), d_opacity, rtol=2e-5, atol=1e-30)


# ---- render ---------------------------------------------------------------------------------------------------------------------
def _scene(dev, P=300):
    model, cam, bg, target = small_scene(P=P, sh_degree=3, width=64, height=48, focal=60.0, scale=0.08)
    model.to(dev)
    cam.to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    return model, cam, bg.to(dev), target.to(dev)


def _frame(model, cam, bg, target, fused):
    from mvs_gaussian_splatting_amd import l1_loss, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    for p in model.parameters():
        p.grad = None
    pipe = PipelineParams()
    pipe.fuse_activations = fused
    pkg = render(cam, model, pipe, bg)
    l1_loss(pkg["render"], target).backward()
    return pkg["render"].detach().clone(), pkg["radii"].clone(), model._scaling.grad.clone(), model._opacity.grad.clone()


def test_render_with_a_filter_on_both_paths(gpu_device):
    from mvs_gaussian_splatting_amd import compute_3d_filter
    from mvs_gaussian_splatting_amd.synthetic import orbit_camera
    model, cam, bg, target = _scene(gpu_device)
    plain = {fused: _frame(model, cam, bg, target, fused) for fused in (True, False)}
    cams = [cam] + [orbit_camera(v, 8, 64, 48, 60.0, 60.0) for v in (1, 7)]
    model.filter_3D, flag = compute_3d_filter(model._xyz.detach(), cams)
    assert int(flag) == 0 and float(model.filter_3D.min()) > 0.0
    filtered = {fused: _frame(model, cam, bg, target, fused) for fused in (True, False)}
    # the two paths agree within the bar test_gpu_parity.py holds them to without a filter
    assert int((filtered[True][1] != filtered[False][1]).sum()) <= 2
    assert float((filtered[True][0] - filtered[False][0]).abs().max()) <= 2.0 / 255.0
    for fused in (True, False):
        img, radii, g_s, g_o = filtered[fused]
        assert float((img - plain[fused][0]).abs().max()) > 1e-3, "the filtered frame differs from the unfiltered one"
        assert bool(torch.isfinite(g_s).all()) and bool(torch.isfinite(g_o).all())
        assert float(g_s.abs().max()) > 0.0 and float(g_o.abs().max()) > 0.0, "gradients reach _scaling and _opacity"
    # a filter of zeros is the unfiltered frame, bit for bit, on the fused path -- gradients included
    model.filter_3D = torch.zeros_like(model.filter_3D)
    zero = _frame(model, cam, bg, target, True)
    for a, b in zip(zero, plain[True]):
        assert torch.equal(a, b)
    # the maps' glue runs with a filter too, and the planes keep their normals (the unfiltered scales decide them)
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model.filter_3D, _ = compute_3d_filter(model._xyz.detach(), cams)
    with torch.no_grad():
        pkg = render(cam, model, PipelineParams(), bg, return_depth=True, return_normals=True)
    assert bool(torch.isfinite(pkg["normal"]).all()) and float(pkg["alpha"].max()) > 0.0
    model._filter_3D_stale = True
    with pytest.raises(ValueError, match="compute_3D_filter"):
        render(cam, model, PipelineParams(), bg)


# ---- the model and the training loop ----------------------------------------------------------------------------------------------
def _trainable(dev, opt, P=300):
    from mvs_gaussian_splatting_amd import GaussianModel
    from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
    src = small_scene(P=P, sh_degree=3, width=64, height=48, focal=60.0, scale=0.08)[0]
    m = GaussianModel(3)
    torch.manual_seed(0)
    m.create_from_pcd(src._xyz.to(dev), torch.rand(P, 3).to(dev), 1.0)
    for a in GROUP_ATTR.values():
        setattr(m, a, nn.Parameter(getattr(src, a).detach().clone().to(dev).requires_grad_(True)))
    m.active_sh_degree = 3
    m.training_setup(opt)
    return m


def test_model_filter_fuse_and_files(gpu_device, tmp_path):
    from mvs_gaussian_splatting_amd import GaussianModel, compress_model, layout, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams
    _, cam, bg, _ = _scene(gpu_device)
    m = _trainable(gpu_device, OptimizationParams())
    assert m.filter_3D is None
    f = m.compute_3D_filter([cam], rule="paper")
    assert f is m.filter_3D and tuple(f.shape) == (300,) and int(m.filter_3D_none_seen) == 0
    with torch.no_grad():
        want = render(cam, m, PipelineParams(), bg)["render"]
        scale, opacity = m.get_scaling_with_3D_filter, m.get_opacity_with_3D_filter
    assert tuple(scale.shape) == (300, 3) and tuple(opacity.shape) == (300, 1)
    assert (scale > m.get_scaling).all() and (opacity < m.get_opacity).all()
    # the filtered PLY round trip, and the fused PLY: a standard file that renders the same frame without a filter
    a, b = str(tmp_path / "filtered.ply"), str(tmp_path / "fused.ply")
    m.save_ply(a)
    m.save_ply(b, fuse_filter=True)
    back = GaussianModel(3)
    back.load_ply(a)
    assert torch.equal(back.filter_3D, m.filter_3D) and torch.equal(back._scaling, m._scaling)
    fused = GaussianModel(3)
    fused.load_ply(b)
    assert fused.filter_3D is None and not torch.equal(fused._scaling, m._scaling)
    with torch.no_grad():
        assert torch.equal(render(cam, back, PipelineParams(), bg)["render"], want)
        assert torch.equal(render(cam, fused, PipelineParams(), bg)["render"], want)
    with pytest.raises(ValueError, match="fuse_filter_3D_"):
        compress_model(m)
    # pruning marks it stale; recomputing clears that; fusing bakes it in place and drops it
    keep = torch.ones(300, dtype=torch.bool, device=gpu_device)
    keep[::3] = False
    layout.prune_points_(m, keep)
    with pytest.raises(ValueError, match="compute_3D_filter"):
        render(cam, m, PipelineParams(), bg)
    m.compute_3D_filter([cam], rule="paper")
    assert tuple(m.filter_3D.shape) == (200,) and not m._filter_3D_stale and bool(torch.isfinite(m.filter_3D).all())
    scaling_param = m._scaling
    with torch.no_grad():
        want = render(cam, m, PipelineParams(), bg)["render"]
    assert m.fuse_filter_3D_() is m and m.filter_3D is None and m._scaling is scaling_param
    with torch.no_grad():
        assert torch.equal(render(cam, m, PipelineParams(), bg)["render"], want)
    assert compress_model(m, codebook_size=256).num_points == 200


def test_training_iterations_across_a_densification(gpu_device):
    from mvs_gaussian_splatting_amd.rasterizer import rasterize_gaussians_fused
    from mvs_gaussian_splatting_amd.renderer import _settings, _zero_leaf, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams, orbit_camera
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    _, cam, bg, target = _scene(gpu_device)
    cams = [cam, orbit_camera(1, 8, 64, 48, 60.0, 60.0)]
    over = dict(iterations=30, position_lr_max_steps=30, densify_from_iter=1, densification_interval=2,
                densify_until_iter=10, densify_grad_threshold=1e-9)
    opt = OptimizationParams(filter_3d=True, **over)
    m = _trainable(gpu_device, opt)
    sizes, filters = [], []
    for it in (1, 2, 3):
        torch.manual_seed(it)
        loss = training_iteration(m, cam, opt, PipelineParams(), bg, it, cameras_extent=1.0, gt_image=target,
                                  filter_cameras=cams)
        assert bool(torch.isfinite(loss)) and not m._filter_3D_stale
        sizes.append(int(m._xyz.shape[0]))
        filters.append(m.filter_3D)
        assert tuple(m.filter_3D.shape) == (sizes[-1],) and float(m.filter_3D.min()) > 0.0
    print(f"[filter3d] Gaussians over three iterations: {sizes}")
    assert sizes[1] > sizes[0] and sizes[2] == sizes[1], "iteration 2 densifies"
    assert filters[1] is not filters[0] and filters[2] is filters[1], "recomputed after the densification, then kept"
    want, _ = R.compute(m._xyz.detach().cpu().numpy(), cams)
    # the optimizer steps since moved the points a little: nearly every row is close to, not equal to, a fresh filter
    assert np.mean(np.isclose(filters[2].cpu().numpy(), want, rtol=0.05)) > 0.9
    # filter_3d = False: the calls made before -- with or without cameras the same bits, and the frame the operator
    # gives for the model's own tensors
    off = OptimizationParams(**over)
    a, b = _trainable(gpu_device, off), _trainable(gpu_device, off)
    for it in (1, 2, 3):
        for model, kw in ((a, {"filter_cameras": cams}), (b, {})):
            torch.manual_seed(it)
            training_iteration(model, cam, off, PipelineParams(), bg, it, cameras_extent=1.0, gt_image=target, **kw)
    assert a.filter_3D is None and b.filter_3D is None and len(a.capture()) == 12
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    with torch.no_grad():
        pipe = PipelineParams()
        frame = render(cam, a, pipe, bg)["render"]
        visible = torch.empty(a._xyz.shape[0], dtype=torch.bool, device=gpu_device)
        parent, _ = rasterize_gaussians_fused(a._xyz, _zero_leaf(a._xyz), a._features_dc, a._features_rest, a._opacity,
                                              a._scaling, a._rotation, _settings(cam, a, pipe, bg, 1.0), visible=visible)
    assert torch.equal(frame, parent)
