"""Camera gradients, the parts that need no GPU: the float64 oracle as the truth for dL/dviewmatrix, dL/dprojmatrix and
dL/dcampos (autograd against central differences), ``scene.PoseCamera``, the binding of the four new ``GsrGrads`` members
and of ``gsr_camera_grad_bytes``, and the operator's forward-only decision.

The probe scene: 600 Gaussians, SH degree 3, a 96 x 64 image, orbit view 1, the loss ``grad_util.weighted_sum`` (linear in
the image: no discontinuity of its own).
"""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, make_settings, small_scene

FD_H = 1e-6
FD_TOL = 1e-5      # every checked entry, relative to that entry's autograd value ...
# ... plus what a central difference of two float64 losses cannot resolve: each loss is a sum of 3 H W products whose
# rounding (pairwise summation, log2(18432) < 16 levels) is at most 16 eps S with S = sum |w . colour| / (3 H W), so the
# quotient carries up to 2 . 16 eps S / (2 h).  About 1e-11 on the probe scene: it matters for entries below 1e-6 only.
FD_EPS = 16.0 * float(np.finfo(np.float64).eps)


def probe_scene(seed=0, view=1, P=600, sh_degree=3):
    return small_scene(P=P, sh_degree=sh_degree, width=96, height=64, seed=seed, view=view)


def _oracle_loss(model, cam, bg, deg, view, proj, campos, wts, colors=None, upstream_grad=True, want_margin=False):
    from oracle import rasterize_ref
    from grad_util import weighted_sum
    st = make_settings(cam, bg.double(), deg)._replace(viewmatrix=view, projmatrix=proj, campos=campos)
    d = lambda t: t.detach().double()  # noqa: E731
    kw = dict(colors_precomp=d(colors)) if colors is not None else dict(shs=d(model.get_features))
    out = rasterize_ref(d(model.get_xyz), None, d(model.get_opacity), st, scales=d(model.get_scaling),
                        rotations=d(model.get_rotation), upstream_grad=upstream_grad, want_aux=True, want_margin=True, **kw)
    loss = weighted_sum(out[0], wts)
    return (loss, out[2]["margin"], float((out[0].detach() * wts).abs().sum()) / wts.numel()) if want_margin else loss


def _camera_leaves(cam):
    return [t.detach().double().clone().requires_grad_(True)
            for t in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]


def _robust_weights(model, cam, bg):
    """grad_util.linear_weights with the threshold-fragile pixels of the float64 forward (grad_util.MARGIN) at weight zero,
    as in every gradient comparison of this suite: a pixel whose alpha sits within 1e-4 of 1/255 crosses the threshold
    under a perturbation of 1e-6 of an entry with a long lever (projmatrix row 2 multiplies the depth), and the jump,
    divided by 2h, buries the derivative -- the probe scene has one such pixel (margin 3.6e-5)."""
    from grad_util import MARGIN, linear_weights
    wts = linear_weights((3, 64, 96))
    with torch.no_grad():
        _, margin, size = _oracle_loss(model, cam, bg, 3, cam.world_view_transform.double(), cam.full_proj_transform.double(),
                                 cam.camera_center.double(), wts, want_margin=True)
    return wts * (margin > MARGIN)[None].to(wts.dtype), int((margin <= MARGIN).sum()), size


@pytest.mark.parametrize("seed,view", [(0, 1), (3, 2)])
def test_oracle_camera_gradients_match_central_differences(seed, view):
    """Float64 autograd of ``rasterize_ref`` with respect to viewmatrix, projmatrix and campos against central differences
    (h = 1e-6) on EVERY entry the rasterizer reads, on the probe scene and on a second seed and view.

    The oracle's default backward is upstream's, which departs from the exact derivative on purpose in documented places
    (oracle/rasterizer_ref.py: alpha clamp, the conic's 1e-7, the guard-band rule).  Only the guard-band rule is visible
    here: it drops the dependence of the clamped tx / ty on the depth, i.e. on viewmatrix column 2, for the Gaussians
    outside the band.  A finite difference knows no such rule, so column 2 is checked with ``upstream_grad=False`` (the
    exact derivative), everything else with the default backward the GPU tests compare against."""
    model, cam, bg, _ = probe_scene(seed=seed, view=view)
    wts, n_fragile, size = _robust_weights(model, cam, bg)
    floor = FD_EPS * size / FD_H
    print(f"[camera fd] seed {seed} view {view}: {n_fragile} threshold-fragile pixels out of the loss; a central difference "
          f"resolves {floor:.1e}")
    worst = 0.0
    for upstream in (True, False):
        leaves = _camera_leaves(cam)
        _oracle_loss(model, cam, bg, 3, *leaves, wts, upstream_grad=upstream).backward()
        g_view, g_proj, g_pos = (t.grad for t in leaves)
        # entries the rasterizer does not read are exact zeros, every other entry carries a signal
        assert int(torch.count_nonzero(g_view[:, 3])) == 0 and int(torch.count_nonzero(g_proj[:, 2])) == 0
        assert float(g_view[:, :3].abs().min()) > 0.0 and float(g_proj[:, [0, 1, 3]].abs().min()) > 0.0
        assert float(g_pos.abs().min()) > 0.0
        entries = [(0, (i, c)) for i in range(4) for c in ((0, 1) if upstream else (2,))]
        if upstream:
            entries += [(1, (i, c)) for i in range(4) for c in (0, 1, 3)] + [(2, (k,)) for k in range(3)]
        with torch.no_grad():
            for which, idx in entries:
                vals = []
                for sign in (1.0, -1.0):
                    args = [t.detach().clone() for t in leaves]
                    args[which][idx] += sign * FD_H
                    vals.append(float(_oracle_loss(model, cam, bg, 3, *args, wts, upstream_grad=upstream)))
                fd = (vals[0] - vals[1]) / (2.0 * FD_H)
                ad = float(leaves[which].grad[idx])
                raw = abs(fd - ad) / abs(ad)
                rel = max(abs(fd - ad) - floor, 0.0) / abs(ad)
                worst = max(worst, raw)
                print(f"[camera fd] seed {seed} view {view} {'upstream' if upstream else 'exact'} backward, tensor {which} "
                      f"entry {idx}: autograd {ad:+.6e} fd {fd:+.6e} rel {raw:.1e}")
                assert rel <= FD_TOL, (which, idx, ad, fd, rel)
    print(f"[camera fd] seed {seed} view {view}: worst relative difference {worst:.1e} (before the resolution allowance)")


def test_oracle_campos_gradient_is_exactly_zero_with_colors_precomp():
    from grad_util import linear_weights
    model, cam, bg, _ = probe_scene()
    colors = torch.rand(600, 3, generator=torch.Generator().manual_seed(4))
    leaves = _camera_leaves(cam)
    _oracle_loss(model, cam, bg, 3, *leaves, linear_weights((3, 64, 96)), colors=colors).backward()
    assert leaves[2].grad is None or int(torch.count_nonzero(leaves[2].grad)) == 0
    assert float(leaves[0].grad.abs().max()) > 0.0 and float(leaves[1].grad.abs().max()) > 0.0


# ---- PoseCamera --------------------------------------------------------------------------------------------------------
def _rodrigues64(w):
    w = np.asarray(w, dtype=np.float64)
    t = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if t == 0.0:
        return np.eye(3)
    return np.eye(3) + math.sin(t) / t * K + (1.0 - math.cos(t)) / (t * t) * (K @ K)


def _base_cameras():
    from mvs_gaussian_splatting_amd.scene import Camera, MiniCam
    from mvs_gaussian_splatting_amd.synthetic import orbit_camera
    syn = orbit_camera(3, 8, 96, 64, 200.0, 180.0)
    img = torch.rand(3, 64, 96, generator=torch.Generator().manual_seed(1))
    cam = Camera(7, syn.R, syn.T, syn.FoVx, syn.FoVy, img, None, "view_7", 0, data_device="cpu", device="cpu")
    mini = MiniCam(96, 64, syn.FoVy, syn.FoVx, 0.01, 100.0, syn.world_view_transform.clone(), syn.full_proj_transform.clone())
    return {"synthetic": syn, "camera": cam, "minicam": mini}


@pytest.mark.parametrize("kind", ["synthetic", "camera", "minicam"])
def test_pose_camera_zero_delta_is_the_base_camera(kind):
    from mvs_gaussian_splatting_amd import PoseCamera
    base = _base_cameras()[kind]
    cam = PoseCamera(base)
    assert sorted(n for n, _ in cam.named_parameters()) == ["rot_delta", "trans_delta"]
    assert cam.rot_delta.shape == (3,) and cam.trans_delta.shape == (3,)
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        got, want = getattr(cam, name), getattr(base, name)
        assert got.requires_grad and got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(got.detach(), want), name
    for name in ("image_width", "image_height", "FoVx", "FoVy", "znear", "zfar"):
        assert getattr(cam, name) == getattr(base, name)
    if kind == "camera":
        assert cam.original_image is base.original_image and cam.image_name == "view_7"
    with pytest.raises(AttributeError):
        cam.no_such_attribute


@pytest.mark.parametrize("kind", ["synthetic", "minicam"])
def test_pose_camera_matches_a_float64_rodrigues_restatement(kind):
    from mvs_gaussian_splatting_amd import PoseCamera
    base = _base_cameras()[kind]
    cam = PoseCamera(base)
    rot, trans = [0.11, -0.07, 0.05], [0.3, -0.2, 0.15]
    with torch.no_grad():
        cam.rot_delta.copy_(torch.tensor(rot))
        cam.trans_delta.copy_(torch.tensor(trans))
    D = np.eye(4)
    D[:3, :3] = _rodrigues64(rot)
    D[:3, 3] = trans
    w2c = base.world_view_transform.double().numpy().T           # column-vector world-to-camera
    proj = np.linalg.inv(w2c.T) @ base.full_proj_transform.double().numpy()
    w2c_new = D @ w2c                                            # the increment multiplies from the left
    want_view = w2c_new.T
    want_full = want_view @ proj
    want_center = np.linalg.inv(w2c_new)[:3, 3]
    view, full, center = cam.transforms()
    assert np.abs(view.detach().double().numpy() - want_view).max() <= 4e-6 * np.abs(want_view).max()
    assert np.abs(full.detach().double().numpy() - want_full).max() <= 4e-6 * np.abs(want_full).max()
    assert np.abs(center.detach().double().numpy() - want_center).max() <= 4e-6 * np.abs(want_center).max()
    R, T = cam.pose()
    assert R.dtype == np.float64 and np.abs(R - w2c_new[:3, :3].T).max() <= 1e-6 and np.abs(T - w2c_new[:3, 3]).max() <= 1e-6
    # the small-angle series and the closed form agree where they meet
    from mvs_gaussian_splatting_amd.scene import so3_exp
    for scale in (0.0, 1e-9, 5e-4, 9.99e-4, 1.01e-3, 0.5, 3.0):
        w = np.array([0.6, -0.64, 0.48]) * scale
        got = so3_exp(torch.tensor(w, dtype=torch.float64)).numpy()
        assert np.abs(got - _rodrigues64(w)).max() <= 1e-15 + 1e-13 * scale, scale
    assert torch.equal(so3_exp(torch.zeros(3)), torch.eye(3))


@pytest.mark.parametrize("with_projection", [True, False])
@pytest.mark.parametrize("at_zero", [True, False])
def test_pose_transforms_gradcheck_float64(with_projection, at_zero):
    from mvs_gaussian_splatting_amd.scene import pose_transforms
    base = _base_cameras()["synthetic"]
    wv, full = base.world_view_transform.double(), base.full_proj_transform.double()
    proj = base.projection_matrix.double() if with_projection else None
    rot = torch.zeros(3, dtype=torch.float64) if at_zero else torch.tensor([0.2, -0.1, 0.3], dtype=torch.float64)
    trans = torch.zeros(3, dtype=torch.float64) if at_zero else torch.tensor([0.1, 0.05, -0.2], dtype=torch.float64)
    rot.requires_grad_(True)
    trans.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda r, t: pose_transforms(wv, proj, full, r, t), (rot, trans), eps=1e-6, atol=1e-7)


@pytest.mark.parametrize("kind", ["synthetic", "camera", "minicam"])
def test_pose_camera_bake_round_trips(kind):
    from mvs_gaussian_splatting_amd import PoseCamera
    base = _base_cameras()[kind]
    cam = PoseCamera(base)
    baked0 = cam.bake()
    assert type(baked0) is type(base)
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert torch.allclose(getattr(baked0, name), getattr(base, name), rtol=0, atol=2e-6), name
    with torch.no_grad():
        cam.rot_delta.copy_(torch.tensor([0.02, 0.05, -0.03]))
        cam.trans_delta.copy_(torch.tensor([0.1, -0.05, 0.2]))
    baked = cam.bake()
    view, full, center = (t.detach() for t in cam.transforms())
    assert not baked.world_view_transform.requires_grad
    assert torch.allclose(baked.world_view_transform, view, rtol=0, atol=4e-6)
    assert torch.allclose(baked.full_proj_transform, full, rtol=0, atol=4e-6 * float(full.abs().max()))
    assert torch.allclose(baked.camera_center, center, rtol=0, atol=2e-5)
    again = PoseCamera(baked)             # a fresh wrapper of the baked camera starts at the refined pose
    assert torch.equal(again.world_view_transform.detach(), baked.world_view_transform)
    if kind != "minicam":
        R, T = cam.pose()
        assert np.abs(np.asarray(baked.R) - R).max() == 0.0 and np.abs(np.asarray(baked.T) - T).max() == 0.0


# ---- binding -----------------------------------------------------------------------------------------------------------
def test_gsr_grads_has_the_camera_members_after_the_statistics():
    from mvs_gaussian_splatting_amd import _lib
    names = [n for n, _ in _lib.GsrGrads._fields_]
    at = names.index("stats_max_radii2D")
    assert names[at + 1:] == ["dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos", "camera_ws"]
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    body = header[header.index("typedef struct GsrGrads {"):header.index("} GsrGrads;")]
    members = re.findall(r"^\s*(?:float|void)\s*\*\s*(\w+);", body, flags=re.M)
    assert members == names
    # existing positional constructions (twelve pointers) keep working and leave the camera group NULL
    g = _lib.GsrGrads(*range(1, 13))
    assert g.stats_max_radii2D == 12 and g.dL_dviewmatrix is None and g.camera_ws is None


def test_camera_grad_bytes_is_declared_exported_monotone_and_aligned():
    from mvs_gaussian_splatting_amd import _lib
    header = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert re.search(r"size_t\s+gsr_camera_grad_bytes\(int32_t P\);", header)
    assert "gsr_camera_grad_bytes" in _lib.SYMBOLS
    lib = _lib.load()
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 20
    prev = 0
    for P in (0, 1, 63, 64, 256, 257, 1000, 100_000, 1_000_000, 6_000_000):
        n = lib.gsr_camera_grad_bytes(P)
        assert n > 0 and n % 256 == 0 and n >= prev, (P, n)
        assert n >= 27 * 8 * ((P + 255) // 256)                # 27 double sums per block of 256 Gaussians
        prev = n
    assert lib.gsr_camera_grad_bytes(1_000_000) > lib.gsr_camera_grad_bytes(1000)
    assert lib.gsr_camera_grad_bytes(6_000_000) < 8 * 1024 * 1024


# ---- the operator's forward-only decision ----------------------------------------------------------------------------------
def test_forward_only_is_false_for_a_frozen_model_with_a_camera_that_requires_grad():
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings, _camera_inputs, _forward_only
    model, cam, bg, _ = probe_scene(P=16)
    frozen = [model.get_xyz, None, model.get_features, model.get_opacity, model.get_scaling, model.get_rotation]
    assert not any(t is not None and t.requires_grad for t in frozen)

    def settings(view, proj, pos):
        return GaussianRasterizationSettings(64, 96, 0.5, 0.5, bg, 1.0, view, proj, 3, pos, False, False)

    plain = settings(cam.world_view_transform, cam.full_proj_transform, cam.camera_center)
    assert _camera_inputs(plain) == () and _forward_only(*frozen, *_camera_inputs(plain))
    for k in range(3):
        trio = [cam.world_view_transform.clone(), cam.full_proj_transform.clone(), cam.camera_center.clone()]
        trio[k].requires_grad_(True)
        st = settings(*trio)
        assert len(st) == 12
        got = _camera_inputs(st)
        assert len(got) == 3 and all(a is b for a, b in zip(got, trio))
        assert not _forward_only(*frozen, *got)
        with torch.no_grad():
            assert _camera_inputs(st) == () and _forward_only(*frozen, *_camera_inputs(st))
