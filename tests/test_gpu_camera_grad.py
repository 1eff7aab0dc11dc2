"""Camera gradients of the HIP backward (dL/dviewmatrix, dL/dprojmatrix, dL/dcampos) against the float64 oracle, at the
bar of tests/grad_util.py: 1e-5 max-norm relative per tensor, or 2 x the float32 oracle's own error, capped at 2e-4
(``compare_grads``, unchanged, with the three camera tensors added beside the model's).  Also: the entries that must be
exact zeros, bit-reproducibility, that nothing else of the backward moves when the camera gradients are asked for, the
block / finish reduction at a million Gaussians (an identity that needs no oracle), the raw ABI's errors and the pose
refinement of examples/refine_pose.py.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, make_settings, small_scene

pytestmark = pytest.mark.gpu

CAM_KEYS = ("viewmatrix", "projmatrix", "campos")


def _cam_leaves(cam, dtype, dev="cpu"):
    return {k: t.detach().to(dtype).to(dev).clone().contiguous().requires_grad_(True)
            for k, t in zip(CAM_KEYS, (cam.world_view_transform, cam.full_proj_transform, cam.camera_center))}


def _oracle(model, cam, bg, deg, target, dtype, weight=None, loss_kind="l1", **kw):
    """grads_oracle with the three camera tensors as leaves of the run's dtype; their gradients join the dict."""
    from grad_util import grads_oracle
    leaves = _cam_leaves(cam, dtype)
    st = make_settings(cam, bg, deg)._replace(viewmatrix=leaves["viewmatrix"], projmatrix=leaves["projmatrix"],
                                              campos=leaves["campos"])
    grads, weight, aux, col = grads_oracle(model, st, target, dtype=dtype, weight=weight, loss_kind=loss_kind, **kw)
    for k, t in leaves.items():
        grads[k] = torch.zeros_like(t) if t.grad is None else t.grad.detach()
    return grads, weight, aux, col


def _product_settings(cam, bg, deg, dev, camera_grad=True):
    from gpu_util import product_settings
    st = product_settings(cam, bg, deg, dev)
    if not camera_grad:
        return st, {}
    leaves = _cam_leaves(cam, torch.float32, dev)
    return st._replace(viewmatrix=leaves["viewmatrix"], projmatrix=leaves["projmatrix"], campos=leaves["campos"]), leaves


def _product(dev, model, cam, bg, deg, target, weight, use_cov=False, use_colors=None, loss_kind="l1", camera_grad=True):
    """gpu_util.grads_product (the getter-fed operator) with a camera that requires grad."""
    from gpu_util import grads_product
    st, leaves = _product_settings(cam, bg, deg, dev, camera_grad)
    got, col = grads_product(dev, model, st, target, weight, use_cov, use_colors, loss_kind=loss_kind)
    for k, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape and t.grad.dtype == torch.float32, k
        got[k] = t.grad.detach().cpu()
    return got, col


class _LeafCamera:
    """A camera object for render() whose three tensors are float32 leaves on the device."""

    def __init__(self, cam, dev, camera_grad=True):
        self.image_width, self.image_height, self.FoVx, self.FoVy = cam.image_width, cam.image_height, cam.FoVx, cam.FoVy
        t = [x.detach().to(dev).clone().contiguous() for x in (cam.world_view_transform, cam.full_proj_transform,
                                                               cam.camera_center)]
        if camera_grad:
            for x in t:
                x.requires_grad_(True)
        self.world_view_transform, self.full_proj_transform, self.camera_center = t

    def grads(self):
        return {k: t.grad.detach().cpu() for k, t in zip(CAM_KEYS, (self.world_view_transform, self.full_proj_transform,
                                                                   self.camera_center))}


def _render_grads(dev, model, cam, bg, target, weight, loss_kind="l1", camera_grad=True, model_grad=True, stats=False):
    """render() on the fused raw-parameter path; returns (grads incl. camera, image, accumulators or None)."""
    from grad_util import loss_of
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.renderer import _can_fuse
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model.to(dev)
    for p in model.parameters():
        p.grad = None
        p.requires_grad_(model_grad)
    pipe = PipelineParams()
    assert _can_fuse(model, pipe, None)
    acc = None
    if stats:
        P = model._xyz.shape[0]
        model.xyz_gradient_accum = torch.full((P, 1), 0.25, device=dev)
        model.denom = torch.ones(P, 1, device=dev)
        model.max_radii2D = torch.full((P,), 1.5, device=dev)
        pipe.fuse_densify_stats = True
    lc = _LeafCamera(cam, dev, camera_grad)
    pkg = render(lc, model, pipe, bg.to(dev))
    loss_of(pkg["render"], target, weight, loss_kind).backward()
    torch.cuda.synchronize(dev)
    got = {}
    if model_grad:
        got = {"xyz": model._xyz.grad, "f_dc": model._features_dc.grad, "f_rest": model._features_rest.grad,
               "opacity": model._opacity.grad, "scaling": model._scaling.grad, "rotation": model._rotation.grad}
        got = {k: (v.detach().cpu() if v is not None else torch.zeros_like(getattr(model, "_features_rest")).cpu())
               for k, v in got.items()}
    got["means2D"] = pkg["viewspace_points"].grad.detach().cpu()
    if camera_grad:
        got.update(lc.grads())
    if stats:
        acc = tuple(t.detach().cpu().clone() for t in (model.xyz_gradient_accum, model.denom, model.max_radii2D))
    for p in model.parameters():
        p.requires_grad_(False)
    model.to("cpu")
    return got, pkg["render"].detach().cpu(), acc


def _assert_zero_columns(got, label):
    assert int(torch.count_nonzero(got["viewmatrix"][:, 3])) == 0, f"{label}: viewmatrix column 3 must be exact zeros"
    assert int(torch.count_nonzero(got["projmatrix"][:, 2])) == 0, f"{label}: projmatrix column 2 must be exact zeros"
    assert got["viewmatrix"].shape == (4, 4) and got["projmatrix"].shape == (4, 4) and got["campos"].shape == (3,)


def _parity(dev, model, cam, bg, target, deg, label, path="operator", use_cov=False, use_colors=None, campos_zero=False):
    """Masked L1 run and the all-pixel linear run (threshold-fragile pixels, if any, at weight zero in the second) of one
    scene, compare_grads on the model's tensors and the camera's."""
    from grad_util import compare_grads, linear_weights
    kw = dict(use_cov=use_cov, use_colors=use_colors)
    ref, weight, aux, _ = _oracle(model, cam, bg, deg, target, torch.float64, **kw)
    n_fragile = int((aux["margin"] <= 1e-4).sum())
    wts = linear_weights(weight.shape) * (aux["margin"] > 1e-4)[None].to(torch.float64)
    for kind, w in (("l1", weight), ("linear", wts)):
        if kind == "linear":
            ref, _, _, _ = _oracle(model, cam, bg, deg, target, torch.float64, weight=w, loss_kind=kind, **kw)
        ref32, _, _, _ = _oracle(model, cam, bg, deg, target, torch.float32, weight=w, loss_kind=kind, **kw)
        if path == "operator":
            got, _ = _product(dev, model, cam, bg, deg, target, w, use_cov, use_colors, loss_kind=kind)
        else:
            model.active_sh_degree = deg
            got, _, _ = _render_grads(dev, model, cam, bg, target, w, loss_kind=kind)
        lab = f"{label}, {path}, loss {kind} ({n_fragile} threshold-fragile pixels at weight zero)"
        for k in CAM_KEYS[:2]:
            assert float(ref[k].abs().max()) > 0.0, f"{lab}: {k} carries no signal"
        compare_grads(got, ref, ref32, lab)
        _assert_zero_columns(got, lab)
        if campos_zero:
            assert int(torch.count_nonzero(ref["campos"])) == 0 and int(torch.count_nonzero(got["campos"])) == 0, lab
        else:
            assert float(ref["campos"].abs().max()) > 0.0, f"{lab}: campos carries no signal"


def _scene(P=2500, deg=3, seed=0, view=1, scale=0.06, width=208, height=128):
    model, cam, _, target = small_scene(P=P, sh_degree=deg, width=width, height=height, scale=scale, seed=seed, view=view)
    return model, cam, torch.tensor([0.3, 0.1, 0.2]), target


@pytest.mark.parametrize("seed,view", [(0, 1), (2, 3)])
def test_operator_with_sh_matches_fp64_oracle(gpu_device, seed, view):
    model, cam, bg, target = _scene(seed=seed, view=view)
    _parity(gpu_device, model, cam, bg, target, 3, f"SH degree 3, seed {seed} view {view}")


def test_colors_precomp_matches_fp64_oracle_and_campos_is_zero(gpu_device):
    model, cam, bg, target = _scene(deg=0)
    colors = torch.rand(2500, 3, generator=torch.Generator().manual_seed(3))
    _parity(gpu_device, model, cam, bg, target, 0, "colors_precomp", use_colors=colors, campos_zero=True)


def test_cov3d_precomp_matches_fp64_oracle(gpu_device):
    model, cam, bg, target = _scene()
    _parity(gpu_device, model, cam, bg, target, 3, "cov3D_precomp", use_cov=True)


@pytest.mark.parametrize("stored,active", [(3, 3), (0, 0)])
def test_fused_raw_parameter_path_matches_fp64_oracle(gpu_device, stored, active):
    model, cam, bg, target = _scene(deg=stored)
    _parity(gpu_device, model, cam, bg, target, active, f"render() stored degree {stored}, active {active}", path="fused",
            campos_zero=active == 0)


@pytest.mark.parametrize("path", ["operator", "fused"])
@pytest.mark.parametrize("active", [0, 1])
def test_active_degree_below_degree_3_storage(gpu_device, active, path):
    model, cam, bg, target = _scene(deg=3)
    _parity(gpu_device, model, cam, bg, target, active, f"degree-3 storage at active degree {active}", path=path,
            campos_zero=active == 0)


def test_frame_without_a_visible_gaussian_gives_exact_zeros(gpu_device):
    model, cam, bg, target = _scene(P=300)
    model._xyz = (model._xyz * torch.tensor([1.0, 1.0, -1.0])).contiguous()          # all behind the camera
    weight = torch.ones(3, 128, 208, dtype=torch.float64)
    for got in (_product(gpu_device, model, cam, bg, 3, target, weight)[0],
                _render_grads(gpu_device, model, cam, bg, target, weight)[0]):
        for k in CAM_KEYS:
            assert int(torch.count_nonzero(got[k])) == 0 and bool(torch.isfinite(got[k]).all()), k
        assert int(torch.count_nonzero(got["xyz"])) == 0
    # no Gaussian at all
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    dev = gpu_device
    st, leaves = _product_settings(cam, bg, 0, dev)
    z = torch.zeros(0, 3, device=dev, requires_grad=True)
    col, _ = GaussianRasterizer(st)(means3D=z, means2D=torch.zeros(0, 3, device=dev), opacities=torch.zeros(0, 1, device=dev),
                                    shs=torch.zeros(0, 1, 3, device=dev), scales=torch.zeros(0, 3, device=dev),
                                    rotations=torch.zeros(0, 4, device=dev))
    col.sum().backward()
    for k, t in leaves.items():
        assert t.grad is not None and int(torch.count_nonzero(t.grad)) == 0, k


def test_nothing_else_moves_and_the_result_is_reproducible(gpu_device):
    """Model gradients, dL/dmeans2D and the fused densification statistics are bit-identical with and without camera
    gradients; two runs, and the three GSR_SYNC_FREE modes, give bit-identical camera gradients."""
    from mvs_gaussian_splatting_amd import rasterizer as rz
    model, cam, bg, target = _scene()
    weight = torch.ones(3, 128, 208, dtype=torch.float64)
    base, img0, acc0 = _render_grads(gpu_device, model, cam, bg, target, weight, camera_grad=False, stats=True)
    prev = rz.sync_free_mode()
    try:
        first = None
        for mode in (True, True, False, "deferred", "deferred"):
            rz.set_sync_free(mode)
            got, img, acc = _render_grads(gpu_device, model, cam, bg, target, weight, camera_grad=True, stats=True)
            rz.synchronize_counts()
            assert torch.equal(img, img0)
            for k, v in base.items():
                assert torch.equal(got[k], v), f"{k} moved when the camera gradients were asked for (mode {mode})"
            for a, b in zip(acc, acc0):
                assert torch.equal(a, b), "the fused densification statistics moved"
            assert float(acc[0].max()) > 0.25
            if first is None:
                first = got
                assert all(float(got[k].abs().max()) > 0.0 for k in CAM_KEYS)
            for k in CAM_KEYS:
                assert torch.equal(got[k], first[k]), f"{k} differs between runs / sync-free modes (mode {mode})"
    finally:
        rz.set_sync_free(prev)
    # the getter-fed operator too
    a, _ = _product(gpu_device, model, cam, bg, 3, target, weight, camera_grad=False)
    b, _ = _product(gpu_device, model, cam, bg, 3, target, weight)
    c, _ = _product(gpu_device, model, cam, bg, 3, target, weight)
    for k, v in a.items():
        assert torch.equal(b[k], v), k
    for k in CAM_KEYS:
        assert torch.equal(b[k], c[k]), k


@pytest.mark.parametrize("P", [1, 63, 64, 257, 1000])
def test_gaussian_counts_around_wave_and_block_sizes(gpu_device, P):
    """One lane, a wave short of one lane, a full wave, a block plus one, a partial last wave (1000 = 3 blocks + 3 waves +
    40 lanes)."""
    from grad_util import compare_grads
    model, cam, bg, target = _scene(P=P, scale=0.25)
    if P == 1:
        model._xyz = torch.tensor([[0.3, -0.2, 5.0]])
    ref, weight, aux, _ = _oracle(model, cam, bg, 3, target, torch.float64)
    ref32, _, _, _ = _oracle(model, cam, bg, 3, target, torch.float32, weight=weight)
    assert int((aux["radii"] > 0).sum()) > 0 and float(ref["viewmatrix"].abs().max()) > 0.0
    for got in (_product(gpu_device, model, cam, bg, 3, target, weight)[0],
                _render_grads(gpu_device, model, cam, bg, target, weight)[0]):
        compare_grads(got, ref, ref32, f"P = {P}")
        _assert_zero_columns(got, f"P = {P}")


def test_scene_with_cooperatively_summed_big_splats(gpu_device):
    """Splats of more than 64 tiles have their gradient rows folded by sum_big_rows_kernel before the per-Gaussian
    backward reads them."""
    from grad_util import compare_grads
    model, cam, bg, target = _scene(P=400, scale=0.06)
    model._scaling[:12] = math.log(1.2)
    ref, weight, aux, _ = _oracle(model, cam, bg, 3, target, torch.float64)
    ref32, _, _, _ = _oracle(model, cam, bg, 3, target, torch.float32, weight=weight)
    assert int((aux["pre"]["tiles_touched"] > 64).sum()) >= 3, "the scene must hold splats of more than ROWS_COOP tiles"
    got, _ = _product(gpu_device, model, cam, bg, 3, target, weight)
    compare_grads(got, ref, ref32, "big splats")
    _assert_zero_columns(got, "big splats")


def test_frozen_model_with_a_camera_that_requires_grad(gpu_device):
    model, cam, bg, target = _scene()
    weight = torch.ones(3, 128, 208, dtype=torch.float64)
    full, img0, _ = _render_grads(gpu_device, model, cam, bg, target, weight)
    got, img, _ = _render_grads(gpu_device, model, cam, bg, target, weight, model_grad=False)
    assert all(p.grad is None for p in model.parameters())
    assert torch.equal(img, img0)
    for k in CAM_KEYS:
        assert float(got[k].abs().max()) > 0.0 and torch.equal(got[k], full[k]), k
    # the getter-fed operator with nothing but the camera requiring grad (no means2D leaf either)
    from grad_util import loss_of
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    dev = gpu_device
    st, leaves = _product_settings(cam, bg, 3, dev)
    # the inputs gpu_util.grads_product builds, activations on the device, but none of them a leaf
    raw = {k: getattr(model, k).detach().to(dev) for k in ("_xyz", "_opacity", "_features_dc", "_features_rest", "_scaling",
                                                           "_rotation")}
    col, _ = GaussianRasterizer(st)(means3D=raw["_xyz"], means2D=None, opacities=torch.sigmoid(raw["_opacity"]),
                                    shs=torch.cat((raw["_features_dc"], raw["_features_rest"]), dim=1),
                                    scales=torch.exp(raw["_scaling"]),
                                    rotations=torch.nn.functional.normalize(raw["_rotation"]))
    assert col.requires_grad
    loss_of(col, target, weight, "l1").backward()
    with_model, _ = _product(dev, model, cam, bg, 3, target, weight)
    for k, t in leaves.items():
        assert torch.equal(t.grad.cpu(), with_model[k]), k


def test_block_and_finish_reduction_at_a_million_gaussians(gpu_device):
    """C3 size, no oracle.  Moving the camera by t in world space is moving every Gaussian by -t, so the total derivative
    of the loss with respect to t -- through V(t), M(t) = V(t) P and campos + t -- equals -sum_i dL/dmeans3D_i in exact
    arithmetic, on every path (the SH direction included).  Both sides in float64 from the float32 outputs; per component
    the bar is 1e-5 x sum_i |dL/dmeans3D_i|: the per-Gaussian gradient bar carried through the sum.  3907 block slots go
    through the finish kernel."""
    from mvs_gaussian_splatting_amd import render
    from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene
    dev = gpu_device
    cfg = CONFIGS["C3"]
    model, cam, bg, _ = make_scene(cfg, seed=0, view=1)
    model.to(dev)
    model._xyz.requires_grad_(True)
    lc = _LeafCamera(cam, dev)
    w = torch.rand(3, cfg.height, cfg.width, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 2.0 - 1.0
    pkg = render(lc, model, PipelineParams(), bg.to(dev))
    ((pkg["render"] * w).sum() / w.numel()).backward()
    torch.cuda.synchronize(dev)
    g = lc.grads()
    _assert_zero_columns(g, "C3")
    gx = model._xyz.grad.detach().double().cpu()
    assert int((gx.abs().sum(dim=1) > 0).sum()) > 100_000
    V0, c0 = cam.world_view_transform.double().cpu(), cam.camera_center.double().cpu()
    Pm = cam.projection_matrix.double().cpu()
    t = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    shift = torch.cat([torch.cat([torch.eye(3, dtype=torch.float64), torch.zeros(3, 1, dtype=torch.float64)], 1),
                       torch.cat([-t, torch.ones(1, dtype=torch.float64)]).unsqueeze(0)], 0)
    V = shift @ V0
    total = (g["viewmatrix"].double() * V).sum() + (g["projmatrix"].double() * (V @ Pm)).sum() + (g["campos"].double() * (c0 + t)).sum()
    lhs, = torch.autograd.grad(total, t)
    rhs = -gx.sum(dim=0)
    bar = 1e-5 * gx.abs().sum(dim=0)
    print(f"[camera identity, P = {cfg.P}] d/dt {lhs.tolist()}  -sum dL/dxyz {rhs.tolist()}  |diff| {(lhs - rhs).abs().tolist()}  "
          f"bar {bar.tolist()}")
    assert bool(((lhs - rhs).abs() <= bar).all()), ((lhs - rhs).abs() / gx.abs().sum(dim=0)).tolist()
    model._xyz.requires_grad_(False)


def test_raw_abi_rejects_a_half_set_camera_group_and_a_missing_workspace(gpu_device):
    from mvs_gaussian_splatting_amd import _lib
    from mvs_gaussian_splatting_amd.rasterizer import _make_params
    from gpu_util import product_settings
    lib = _lib.load()
    dev = gpu_device
    model, cam, bg, _ = _scene(P=64)
    e = torch.empty(0, device=dev)
    t = [x.to(dev).contiguous() for x in (model.get_xyz, model.get_features, model.get_opacity, model.get_scaling,
                                          model.get_rotation)]
    with torch.cuda.device(dev):
        params, keep = _make_params(dev, product_settings(cam, bg, 3, dev), t[0], t[1], e, t[2], t[3], t[4], e)
    out = torch.zeros(64, device=dev)
    ws = torch.zeros(lib.gsr_camera_grad_bytes(64) + 256, dtype=torch.uint8, device=dev)
    base = ws.data_ptr() + (-ws.data_ptr()) % 256

    def call(view, proj, pos, cws):
        g = _lib.GsrGrads(out.data_ptr(), out.data_ptr(), out.data_ptr(), None, out.data_ptr(), out.data_ptr(), out.data_ptr())
        g.dL_dviewmatrix, g.dL_dprojmatrix, g.dL_dcampos, g.camera_ws = view, proj, pos, cws
        rc = lib.gsr_backward(C.byref(params), None, None, None, None, 0, 0, None, None, 0, C.byref(g), None)
        return rc, lib.gsr_last_error().decode()

    p = out.data_ptr()
    for trio in ((p, None, None), (None, p, None), (None, None, p), (p, p, None), (p, None, p), (None, p, p)):
        rc, msg = call(*trio, base)
        assert rc == -1 and "together" in msg, (trio, rc, msg)
    rc, msg = call(p, p, p, None)
    assert rc == -1 and "camera_ws" in msg, (rc, msg)
    rc, msg = call(p, p, p, base + 8)
    assert rc == -3 and "aligned" in msg, (rc, msg)
    rc, msg = call(p, p, p, base)               # a whole group passes these checks and fails on the NULL workspaces instead
    assert rc == -1 and "camera" not in msg, (rc, msg)
    del keep


def test_pose_refinement_recovers_a_perturbed_camera(gpu_device):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import refine_pose
    finally:
        sys.path.pop(0)
    out = refine_pose.refine(gpu_device, iterations=300)
    first, last = float(np.mean(out["loss"][:5])), float(np.mean(out["loss"][-5:]))
    r0, r1 = out["rot_err"]
    t0, t1 = out["trans_err"]
    print(f"[pose refinement] loss {first:.6f} -> {last:.6f} (x{first / last:.1f}); rotation error {r0:.4f} -> {r1:.4f} deg "
          f"(x{r0 / max(r1, 1e-12):.1f}); translation error {t0:.5f} -> {t1:.5f} (x{t0 / max(t1, 1e-12):.1f})")
    assert last < first and r1 < r0 and t1 < t0
