"""CPU-side checks of the depth-normal consistency loss (csrc/normal_consistency.hip; normal_consistency.py; DESIGN.md
§7.15): the ABI, every refusal -- all before a GPU is asked for --, the restatement the GPU tests compare against
(tests/normal_consistency_restate.py) held to an analytic plane, to ``gaussian_normals`` for the sign and to central finite
differences, the caps on threshold-fragile pixels of the shared inputs, and the trainer's switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import normal_consistency_restate as R


def test_library_exports_the_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_normal_consistency_workspace_bytes", "gsr_normal_consistency_fwd_bwd"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 28
    # one (double, uint32) pair per 16x16 workgroup; 0 for a shape the call refuses
    assert lib.gsr_normal_consistency_workspace_bytes(1080, 1920) == 68 * 120 * 12
    assert lib.gsr_normal_consistency_workspace_bytes(17, 33) == 2 * 3 * 12
    assert lib.gsr_normal_consistency_workspace_bytes(0, 5) == 0 and lib.gsr_normal_consistency_workspace_bytes(5, -1) == 0


def test_every_argument_error_of_the_entry_point_fires_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()                                            # 8-byte aligned at least; used for every pointer
    p = (C.addressof(buf) + 15) & ~15
    good = dict(depth=p, alpha=p, normal=p, H=5, W=7, tanx=0.7, tany=0.5, amin=0.5, record=p, gd=p, ga=p, gn=p, dn=p, ws=p)

    def call(**kw):
        a = {**good, **kw}
        return lib.gsr_normal_consistency_fwd_bwd(a["depth"], a["alpha"], a["normal"], a["H"], a["W"], a["tanx"], a["tany"],
                                                  a["amin"], a["record"], a["gd"], a["ga"], a["gn"], a["dn"], a["ws"], None)

    bad = [dict(H=0), dict(W=0), dict(H=-3), dict(H=1 << 20, W=1 << 20), dict(tanx=0.0), dict(tany=-1.0),
           dict(tanx=float("nan")), dict(tany=float("inf")), dict(amin=0.0), dict(amin=-0.5), dict(amin=1.5),
           dict(amin=float("nan")), dict(depth=None), dict(alpha=None), dict(normal=None), dict(record=None),
           dict(ws=None), dict(gd=None), dict(ga=None), dict(gn=None), dict(gd=None, ga=None), dict(ga=None, gn=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.gsr_last_error()
    for kw in (dict(depth=p + 2), dict(normal=p + 1), dict(gd=p + 2), dict(dn=p + 3), dict(record=p + 4), dict(ws=p + 4)):
        assert call(**kw) == -3, kw


def _maps(H=29, W=37, dtype=torch.float32, device="cpu"):
    return (torch.ones(1, H, W, dtype=dtype, device=device), torch.ones(1, H, W, dtype=dtype, device=device),
            torch.zeros(3, H, W, dtype=dtype, device=device))


def test_every_refusal_of_the_python_functions_comes_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, depth_to_normals, normal_consistency_loss
    d, a, n = _maps()
    for args in ((d.double(), a, n), (d, a.half(), n), (d, a, n.double()), (d.numpy(), a, n), (d, a, None)):
        with pytest.raises(TypeError):
            normal_consistency_loss(*args, 0.7, 0.5)
    for args in ((d[:, :-1], a, n), (d, a[:, :, :-1], n), (d, a, n[:2]), (d, a, n.permute(1, 2, 0)), (d.expand(2, -1, -1), a, n),
                 (torch.ones(1, 0, 37), torch.ones(1, 0, 37), torch.zeros(3, 0, 37)), (d, a, n.to("meta"))):
        with pytest.raises(ValueError):
            normal_consistency_loss(*args, 0.7, 0.5)
    for kw in (dict(tanfovx=0.0), dict(tanfovy=-1.0), dict(tanfovx=float("nan")), dict(tanfovy=float("inf")),
               dict(alpha_min=0.0), dict(alpha_min=1.5), dict(alpha_min=float("nan")), dict(alpha_min=None)):
        with pytest.raises(ValueError):
            normal_consistency_loss(d, a, n, **{**dict(tanfovx=0.7, tanfovy=0.5), **kw})
        with pytest.raises(ValueError):
            depth_to_normals(d, a, **{**dict(tanfovx=0.7, tanfovy=0.5), **kw})
    with pytest.raises(TypeError):
        depth_to_normals(d.double(), a, 0.7, 0.5)
    with pytest.raises(ValueError):
        depth_to_normals(d, a[:, :-1], 0.7, 0.5)
    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError):
        normal_consistency_loss(d, a, n, 0.7, 0.5)
    with pytest.raises(_lib.GsrError):
        depth_to_normals(d, a, 0.7, 0.5)


def test_restated_normal_of_a_tilted_plane_is_its_camera_facing_normal_and_agrees_with_gaussian_normals():
    """The definition and its sign: under full coverage the central differences of points of a plane lie in the plane,
    so n_d is the plane's normal exactly; it must be the one that faces the camera, the one gaussian_normals gives a
    disc lying in that plane; and with normal = alpha * that normal the loss is 0 to rounding."""
    from mvs_gaussian_splatting_amd import gaussian_normals
    H, W = 13, 17
    tanx, tany = R.TANFOV
    n_plane = torch.tensor(R.plane_normal())
    assert n_plane[2] < 0, "a camera-facing normal points against +z"
    z = R.plane_depth(H, W, tanx, tany)
    alpha = 0.7 + 0.3 * torch.rand(H, W, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    normal = alpha * n_plane.view(3, 1, 1)
    ref = R.restate(z * alpha, alpha, normal, tanx, tany)
    assert ref["n_valid"] == (H - 2) * (W - 2) and bool(ref["valid"][1:-1, 1:-1].all()) and not bool(ref["valid"][0].any())
    err = (ref["depth_normal"][:, 1:-1, 1:-1] - n_plane.view(3, 1, 1)).abs().max()
    print(f"plane: n_d off the analytic normal by {float(err):.2e}, loss {float(ref['loss']):.2e}")
    assert float(err) < 1e-9
    assert abs(float(ref["loss"])) < 1e-12
    assert bool((ref["depth_normal"][:, 0] == 0).all()) and bool((ref["depth_normal"][:, :, -1] == 0).all())
    # a fronto-parallel plane: (0, 0, -1)
    flat = R.restate(torch.full((H, W), 3.0, dtype=torch.float64), torch.ones(H, W, dtype=torch.float64),
                     torch.zeros(3, H, W, dtype=torch.float64), tanx, tany)
    assert torch.allclose(flat["depth_normal"][:, 1:-1, 1:-1],
                          torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).view(3, 1, 1).expand(3, H - 2, W - 2), atol=1e-12)
    # a flat disc in the tilted plane, seen by the identity camera: its smallest axis is the plane's normal
    m = -n_plane                                                         # rotate +z onto m; the function picks the sign
    q = torch.tensor([[1.0 + float(m[2]), -float(m[1]), float(m[0]), 0.0]], dtype=torch.float64)
    scales = torch.tensor([[1.0, 0.7, 0.01]], dtype=torch.float64)
    mean = torch.tensor([[0.0, 0.0, R.PLANE_Z0]], dtype=torch.float64)
    got = gaussian_normals(scales, q, mean, torch.eye(4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    assert torch.allclose(got[0], n_plane, atol=1e-12), "gaussian_normals and the depth normal disagree in sign"
    # against the wrong sign the loss is 2 mean(alpha) over the valid pixels, not 0
    wrong = R.restate(z * alpha, alpha, -normal, tanx, tany)
    assert float(wrong["loss"]) == pytest.approx(2.0 * float(alpha[1:-1, 1:-1].sum()) / (H * W), rel=1e-9)


def test_restated_float64_gradients_agree_with_central_finite_differences():
    H, W = 9, 11
    depth, alpha, normal = (t.double() for t in R.make_case("random", H, W))
    tanx, tany = R.TANFOV
    ref = R.restate(depth, alpha, normal, tanx, tany)
    assert ref["n_valid"] == (H - 2) * (W - 2)
    loss = lambda d, a, n: float(R.restate(d, a, n, tanx, tany)["loss"])        # noqa: E731
    h = 1e-6
    worst = 0.0
    for which, grad in ((0, ref["d_depth"]), (1, ref["d_alpha"]), (2, ref["d_normal"])):
        base = [depth, alpha, normal]
        fd = torch.zeros_like(grad)
        flat = fd.view(-1)
        for i in range(flat.numel()):
            hi, lo = [t.clone() for t in base], [t.clone() for t in base]
            hi[which].view(-1)[i] += h
            lo[which].view(-1)[i] -= h
            flat[i] = (loss(*hi) - loss(*lo)) / (2 * h)
        rel = float((fd - grad).abs().max() / grad.abs().max())
        worst = max(worst, rel)
        print(f"finite differences, input {which}: max-norm relative difference {rel:.2e}")
    # central differences with h = 1e-6 on O(1) values: truncation O(h^2), rounding O(1e-16 / h)
    assert worst < 1e-6
    # a corner pixel is nobody's neighbour; an edge pixel is a neighbour of one valid pixel and still gets a gradient
    assert float(ref["d_depth"][0, 0]) == 0.0 and float(ref["d_depth"][0, 5]) != 0.0
    assert float(ref["d_alpha"][0, 5]) != 0.0 and bool((ref["d_normal"][:, 0, 5] == 0).all())


def test_fragile_share_of_every_shared_input_is_within_its_cap():
    """A condition of the GPU comparison, not a measurement: 0 for the plane and the sphere, below 1 % for the random field."""
    tanx, tany = R.TANFOV
    seen_valid = 0
    for H, W in R.SHAPES:
        for kind in R.KINDS:
            depth, alpha, normal = R.make_case(kind, H, W)
            ref = R.restate(depth, alpha, normal, tanx, tany)
            share = float(R.fragile_mask(ref).double().mean())
            print(f"{kind} {H}x{W}: {ref['n_valid']} valid of {H * W}, fragile share {share:.2e}")
            assert share == 0.0 if kind != "random" else share < 0.01
            if kind == "sphere":
                a = alpha.view(-1)
                assert bool(((a == 0) | (a >= 0.6)).all())
                if H * W > 500:
                    inner = ref["valid"][1:-1, 1:-1]
                    assert 0.1 < float(inner.double().mean()) < 0.9, "the sphere must leave a ragged valid mask"
            elif H >= 3 and W >= 3:
                assert ref["n_valid"] == (H - 2) * (W - 2)
            if min(H, W) < 3:
                assert ref["n_valid"] == 0 and float(ref["loss"]) == 0.0 and float(ref["d_depth"].abs().max()) == 0.0
            seen_valid += ref["n_valid"]
    assert seen_valid > 10000


class _Cam:
    FoVx = FoVy = 1.0
    image_width, image_height = 8, 8
    original_image = torch.zeros(3, 8, 8)


def test_optimization_params_gain_the_two_fields_and_the_trainer_refuses_up_front():
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    opt = OptimizationParams()
    assert opt.lambda_normal == 0.0 and opt.normal_from_iter == 7000
    opt = OptimizationParams(lambda_normal=0.05, normal_from_iter=0)
    assert opt.lambda_normal == 0.05 and opt.normal_from_iter == 0

    class Plain:
        pass

    class Fork:
        _dirs_prob = torch.zeros(4, 3)

    class Dataset:
        grow_dir = True

    with pytest.raises(ValueError, match="pose_optimizer"):
        training_iteration(Plain(), _Cam, opt, None, torch.zeros(3), 10, cameras_extent=1.0, pose_optimizer=object())
    with pytest.raises(ValueError, match="grow / learned-split"):
        training_iteration(Plain(), _Cam, opt, None, torch.zeros(3), 10, cameras_extent=1.0, dataset=Dataset())
    from mvs_gaussian_splatting_amd.densify import is_fork
    if is_fork(Fork()):
        with pytest.raises(ValueError, match="grow / learned-split"):
            training_iteration(Fork(), _Cam, opt, None, torch.zeros(3), 10, cameras_extent=1.0)
