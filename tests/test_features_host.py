"""CPU-side checks of the feature maps (csrc/features.hip; rasterizer ``features=``): the ABI that
carries them, the restatement the GPU tests compare against (tests/features_restate.py) against the depth maps'
restatement, ``features.gaussian_normals``, and the refusals, which all come before a GPU is asked for."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT, make_settings, small_scene
from depth_restate import maps_from_lists
from features_restate import feature_maps_from_lists
from grad_util import oracle_operator_inputs


def test_library_exports_the_feature_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_feature_maps_forward", "gsr_feature_maps_backward", "gsr_feature_maps_backward_bytes"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 26
    assert lib.gsr_feature_maps_backward_bytes(1000) >= 1000 * 8 * 4
    # argument checks run before any HIP call: NULL frame; C < 1 and NULL features on a well-formed frame
    assert lib.gsr_feature_maps_forward(None, None, 3, None, None) == -1
    assert lib.gsr_feature_maps_backward(None, None, None, 3, None, None, None, 0, None, None) == -1
    frame = _lib.GsrAuxFrame()
    frame.P, frame.width, frame.height, frame.binning_mode = 0, 16, 16, _lib.BINNING_TWO_LEVEL
    frame.img_ws = 256
    one = (C.c_float * 4)()
    assert lib.gsr_feature_maps_forward(C.byref(frame), C.addressof(one), 0, C.addressof(one), None) == -1
    assert lib.gsr_feature_maps_forward(C.byref(frame), None, 3, C.addressof(one), None) == -1
    params = _lib.GsrParams()
    params.P, params.width, params.height = 0, 16, 16
    assert lib.gsr_feature_maps_backward(C.byref(params), C.byref(frame), C.addressof(one), 0, None, None, None, 0, None,
                                         None) == -1
    assert lib.gsr_feature_maps_backward(C.byref(params), C.byref(frame), None, 3, None, None, None, 0, None, None) == -1


def test_restatement_with_the_depth_triple_equals_the_depth_restatement_to_the_last_bit():
    """F = (z, 1/z, 1) per Gaussian: the feature maps are the depth / inverse-depth / alpha maps.  float64, the `small`
    scene of test_gpu_depth.py.  Depth and alpha to the last bit; inverse depth to the rounding of 1 / z (see below)."""
    from oracle import rasterize_ref
    model, cam, bg, _ = small_scene(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2)
    st = make_settings(cam, bg, 3)
    _, xyz, m2, op, kw = oracle_operator_inputs(model, torch.float64)
    with torch.no_grad():
        _, _, aux = rasterize_ref(xyz, m2, op, st, want_aux=True, want_margin=True, **kw)
        pre = aux["pre"]
        lists = (aux["point_list"], aux["ranges"], aux["n_contrib"])
        maps = maps_from_lists(pre, *lists, st)
        z = torch.ones(400, dtype=torch.float64)
        z[pre["idx"]] = pre["v_depth"]
        feat = feature_maps_from_lists(pre, *lists, st, torch.stack((z, 1.0 / z, torch.ones_like(z)), dim=1))
    assert feat.dtype == torch.float64 and tuple(feat.shape) == (3, 40, 72)
    assert int((aux["n_contrib"] > 0).sum()) > 500, "the scene must cover a good part of the image"
    # depth and alpha: the same products and the same sums, bit for bit
    assert torch.equal(feat[0], maps[0]) and torch.equal(feat[2], maps[2]), \
        f"max difference {float((feat - maps)[[0, 2]].abs().max()):.3e}"
    # inverse depth: depth_restate divides (w / z) where a feature map can only multiply by the row's value (w * (1 / z)):
    # two roundings instead of one per term, so the terms differ by up to 1.5 units of 2^-53 relative, and the n sums of
    # all-positive terms carry that plus their own n roundings on either side -- no arithmetic makes this channel bit-equal
    n_max = int(aux["n_contrib"].max())
    bound = (1.5 + 2.0 * n_max) * 2.0 ** -53 * maps[1]
    assert bool(((feat[1] - maps[1]).abs() <= bound).all()), f"max difference {float((feat[1] - maps[1]).abs().max()):.3e}"


def _normal_inputs(P, seed=5):
    g = torch.Generator().manual_seed(seed)
    base = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)      # well separated: the argmin is stable under gradcheck
    scales = torch.stack([base[torch.randperm(3, generator=g)] for _ in range(P)]) * \
        (0.5 + torch.rand(P, 1, generator=g, dtype=torch.float64))
    rot = torch.randn(P, 4, generator=g, dtype=torch.float64)
    means = torch.randn(P, 3, generator=g, dtype=torch.float64) * 2.0
    _, cam, _, _ = small_scene(P=4, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    return scales, rot, means, cam.world_view_transform.double(), cam.camera_center.double()


def test_gaussian_normals_are_unit_face_the_camera_and_equal_a_per_row_loop():
    from mvs_gaussian_splatting_amd import gaussian_normals
    scales, rot, means, view, campos = _normal_inputs(64)
    n = gaussian_normals(scales, rot, means, view, campos)
    assert n.dtype == torch.float64 and tuple(n.shape) == (64, 3)
    assert float((n.norm(dim=1) - 1.0).abs().max()) <= 1e-12
    means_view = means @ view[:3, :3] + view[3, :3]      # the camera sits at the origin of view space
    assert float((n * -means_view).sum(dim=1).min()) >= -1e-12, "a normal faces away from the camera"
    flipped = 0
    for i in range(64):
        r, x, y, z = (rot[i] / rot[i].norm()).tolist()
        R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                          [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                          [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)
        col = R[:, int(torch.argmin(scales[i]))]
        if float(col @ (campos - means[i])) < 0:
            col, flipped = -col, flipped + 1
        want = torch.stack([sum(col[k] * view[k, j] for k in range(3)) for j in range(3)])
        assert float((n[i] - want).abs().max()) <= 1e-14, i
    assert 8 <= flipped <= 56, "the rows must exercise both signs"


def test_gaussian_normals_gradcheck_in_the_rotations():
    from mvs_gaussian_splatting_amd import gaussian_normals
    scales, rot, means, view, campos = _normal_inputs(16, seed=9)
    rot = rot.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda q: gaussian_normals(scales, q, means, view, campos), (rot,))


def _cpu_call(features, densify_stats=None, view_grad=False, aux_maps=False):
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    if view_grad:
        st = st._replace(viewmatrix=cam.world_view_transform.clone().requires_grad_(True))
    return GaussianRasterizer(st, aux_maps=aux_maps)(
        means3D=model.get_xyz, means2D=None, opacities=model.get_opacity, shs=model.get_features,
        scales=model.get_scaling, rotations=model.get_rotation, features=features,
        **({} if densify_stats is None else {"densify_stats": densify_stats}))


@pytest.mark.parametrize("bad", [
    torch.zeros(12, 3, dtype=torch.float64), torch.zeros(12, 3, dtype=torch.float16), torch.zeros(12), torch.zeros(12, 3, 1),
    torch.zeros(11, 3), torch.zeros(12, 0), torch.zeros(12, 3, device="meta"), [[0.0] * 3] * 12,
], ids=["float64", "float16", "1-D", "3-D", "P-1 rows", "C=0", "other device", "not a tensor"])
def test_malformed_features_raise_without_a_gpu(bad):
    with pytest.raises(ValueError, match="features"):
        _cpu_call(bad)


def test_features_with_a_camera_that_requires_grad_raise_without_a_gpu():
    with pytest.raises(ValueError, match="camera"):
        _cpu_call(torch.zeros(12, 3), view_grad=True)


def test_features_together_with_in_backward_statistics_raise_without_a_gpu():
    with pytest.raises(ValueError, match="densify_stats"):
        _cpu_call(torch.zeros(12, 3), densify_stats=tuple(torch.zeros(12) for _ in range(3)))


def test_features_on_grown_rows_raise_without_a_gpu():
    from mvs_gaussian_splatting_amd.rasterizer import (GaussianRasterizationSettings, _grown_key,
                                                       rasterize_gaussians_fused)
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    with pytest.raises(ValueError, match="grown"):
        rasterize_gaussians_fused(model._xyz, None, model._features_dc, model._features_rest, model._opacity,
                                  model._scaling, model._rotation, st, _state_key=_grown_key(10),
                                  features=torch.zeros(12, 3))


def test_render_refuses_features_on_the_open_grow_branch_without_a_gpu(monkeypatch):
    from mvs_gaussian_splatting_amd import grow, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    monkeypatch.setattr(grow, "branch", lambda *a, **k: grow.GROW)
    for kw in ({"features": torch.zeros(12, 3)}, {"return_normals": True}):
        with pytest.raises(ValueError, match="grow"):
            render(cam, model, PipelineParams(), bg, **kw)


def test_the_plain_call_signature_is_what_it_was():
    """Without ``features`` the CPU call reaches the operator's GPU requirement as before (no new refusal in its way)."""
    from mvs_gaussian_splatting_amd import _lib
    with pytest.raises(_lib.GsrError, match="GPU"):
        _cpu_call(None)
