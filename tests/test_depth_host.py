"""CPU-side checks of the depth / inverse-depth / alpha maps: the restatement the GPU tests compare against
(tests/depth_restate.py) is itself checked against the oracle's colour pass and against finite differences, and the
built library and the binding agree on the ABI that carries the maps."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT, make_settings, small_scene
from depth_restate import map_weights, maps_from_lists, maps_loss, maps_ref
from grad_util import MARGIN, oracle_operator_inputs


def test_restated_alpha_is_one_minus_the_colour_passes_final_T():
    model, cam, bg, _ = small_scene(P=400, width=72, height=40)
    st = make_settings(cam, bg, 3)
    _, xyz, m2, op, kw = oracle_operator_inputs(model, torch.float64)
    with torch.no_grad():
        maps, _, _, aux = maps_ref(xyz, m2, op, st, **kw)
    assert maps.dtype == torch.float64 and tuple(maps.shape) == (3, 40, 72)
    covered = aux["n_contrib"] > 0
    assert int(covered.sum()) > 500, "the scene must cover a good part of the image"
    err = float((maps[2] - (1.0 - aux["final_T"])).abs().max())
    print(f"[depth restate] max |alpha - (1 - final_T)| = {err:.2e} over {int(covered.sum())} covered pixels")
    assert err <= 1e-12
    assert float(maps[:, ~covered].abs().max()) == 0.0, "a pixel outside every list is 0 in all three maps"
    # depth / alpha is a weighted mean of view depths: inside the range of the depths of the visible Gaussians
    z = aux["pre"]["v_depth"][aux["pre"]["keep"]]
    mean_z = maps[0][covered] / maps[2][covered]
    assert float(mean_z.min()) >= float(z.min()) - 1e-9 and float(mean_z.max()) <= float(z.max()) + 1e-9


def test_restated_gradients_match_central_differences():
    """float64 autograd of the restatement (through the oracle's preprocess) against central differences along random
    directions in the space of all raw parameters, P = 12.  The lists and contributor counts are held at the base
    point's (they are decisions); pixels within MARGIN of a threshold carry no weight, so that no alpha test flips
    inside the stencil.  The oracle's backward deviates from the true derivative in two documented places (the 1e-7 in
    the conic's denominator, the guard-band mask): ``upstream_grad=False`` takes the exact derivative here, which is
    what a finite difference measures."""
    model, cam, bg, _ = small_scene(P=12, sh_degree=1, width=48, height=32, focal=12.0, scale=1.0, seed=3)
    st = make_settings(cam, bg, 1)
    leaves, xyz, m2, op, kw = oracle_operator_inputs(model, torch.float64)
    names = ("xyz", "opacity", "scaling", "rotation")

    def operator_inputs(values):
        return (values["xyz"], torch.sigmoid(values["opacity"]),
                dict(kw, scales=torch.exp(values["scaling"]), rotations=torch.nn.functional.normalize(values["rotation"])))

    maps, _, _, aux = maps_ref(xyz, m2, op, st, upstream_grad=False, **kw)
    assert int((aux["n_contrib"] > 0).sum()) > 100
    weights = map_weights(32, 48) * (aux["margin"] > MARGIN)[None]
    maps_loss(maps, weights).backward()
    grads = {k: leaves[k].grad.clone() for k in names}
    assert all(float(g.abs().max()) > 0 for g in grads.values())

    from oracle import preprocess_ref

    def loss_at(values):
        with torch.no_grad():
            x, o, k2 = operator_inputs(values)
            pre = preprocess_ref(x, o, st, upstream_grad=False, **k2)
            return float(maps_loss(maps_from_lists(pre, aux["point_list"], aux["ranges"], aux["n_contrib"], st), weights))

    gen = torch.Generator().manual_seed(11)
    base = {k: leaves[k].detach() for k in names}
    h = 1e-6
    for trial in range(4):
        d = {k: torch.randn(base[k].shape, generator=gen, dtype=torch.float64) for k in names}
        if trial < len(names):      # one direction per tensor alone, then all of them together
            d = {k: (v if k == names[trial] else torch.zeros_like(v)) for k, v in d.items()}
        fd = (loss_at({k: base[k] + h * d[k] for k in names}) - loss_at({k: base[k] - h * d[k] for k in names})) / (2 * h)
        an = float(sum((grads[k] * d[k]).sum() for k in names))
        print(f"[depth restate] direction {trial}: autograd {an:.9e}, central difference {fd:.9e}")
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-3), (trial, fd, an)


def test_library_exports_the_map_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("gsr_aux_maps_forward", "gsr_aux_maps_backward", "gsr_aux_maps_backward_bytes"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    assert "gsr_aux_maps_forward" in header and "gsr_aux_maps_backward" in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 22
    assert lib.gsr_aux_maps_backward_bytes(1000) >= 1000 * 8 * 4
    # the new structs, as the header lays them out: six 32-bit words, then four pointers / six pointers
    assert C.sizeof(_lib.GsrAuxFrame) == 24 + 4 * C.sizeof(C.c_void_p) and _lib.GsrAuxFrame.geom_ws.offset == 24
    assert C.sizeof(_lib.GsrAuxGrads) == 6 * C.sizeof(C.c_void_p)
    # argument checks run before any HIP call
    assert lib.gsr_aux_maps_forward(None, None, None) == -1
    assert lib.gsr_aux_maps_backward(None, None, None, None, 0, None, None) == -1


def test_maps_with_a_camera_that_requires_grad_raise_without_a_gpu():
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    view = cam.world_view_transform.clone().requires_grad_(True)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)._replace(viewmatrix=view)
    rast = GaussianRasterizer(st, aux_maps=True)
    with pytest.raises(ValueError, match="camera"):
        rast(means3D=model.get_xyz, means2D=None, opacities=model.get_opacity, shs=model.get_features,
             scales=model.get_scaling, rotations=model.get_rotation)
    # the plain constructor and call signature are what they were
    assert GaussianRasterizer(st).aux_maps is False


def test_depth_png_is_16_bit_and_round_trips_through_its_scale(tmp_path):
    """examples/render.py --depth: depth / alpha as a 16-bit greyscale PNG, 65535 at the view's largest value, 0 where
    nothing was composited; file value x returned step gives the depth back to half a step."""
    import importlib.util
    import numpy as np
    from PIL import Image
    spec = importlib.util.spec_from_file_location("example_render", os.path.join(ROOT, "examples", "render.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    g = torch.Generator().manual_seed(5)
    alpha = torch.rand(1, 21, 37, generator=g)
    alpha[0, :3] = 0.0                                    # rows nothing was composited on
    expected = 0.5 + 7.0 * torch.rand(1, 21, 37, generator=g)
    depth = expected * alpha
    path = str(tmp_path / "00000.png")
    step = example.save_depth_png(depth, alpha, path)
    img = Image.open(path)
    assert img.mode in ("I;16", "I;16B", "I;16L") and img.size == (37, 21)
    got = np.asarray(img).astype(np.float64)
    assert got.max() == 65535 and np.all(got[:3] == 0)
    want = torch.where(alpha > 0, depth / alpha.clamp_min(1e-12), torch.zeros_like(depth))[0].double().numpy()
    assert abs(step - want.max() / 65535.0) <= 1e-12 * want.max()
    assert np.abs(got * step - want).max() <= 0.5 * step * (1 + 1e-6) + 1e-6 * want.max()
    # an empty view: all zeros, a step of 1
    assert example.save_depth_png(torch.zeros(1, 4, 5), torch.zeros(1, 4, 5), path) == 1.0
    assert np.asarray(Image.open(path)).max() == 0


def test_maps_together_with_in_backward_statistics_raise_without_a_gpu():
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings
    model, cam, bg, _ = small_scene(P=12, sh_degree=0, width=48, height=32, focal=12.0, scale=1.0)
    st = make_settings(cam, bg, 0, cls=GaussianRasterizationSettings)
    trio = tuple(torch.zeros(12) for _ in range(3))
    with pytest.raises(ValueError, match="densify_stats"):
        GaussianRasterizer(st, aux_maps=True)(means3D=model.get_xyz, means2D=None, opacities=model.get_opacity,
                                              shs=model.get_features, scales=model.get_scaling,
                                              rotations=model.get_rotation, densify_stats=trio)
