"""The depth-normal consistency loss on the HIP path (csrc/normal_consistency.hip; normal_consistency.py)
against the float64 restatement of tests/normal_consistency_restate.py.

Shapes, the smallest at which the kernel can go wrong: 2x5 and 5x2 (no interior), 3x3 (exactly one stencil), 5x7
(sub-wave), 17x33 (one pixel past a 16-pixel workgroup edge both ways: the halo crosses workgroups and the last
workgroups are one pixel wide), 67x131 (ragged both ways).  Inputs per shape: a tilted plane under full coverage, a
sphere over empty background (ragged valid mask), a smooth random field with random ``normal``.

Bars.  On the pixels no decision of whose footprint is within 1e-4 relative of flipping (the host test caps their share:
0 for the plane and the sphere, below 1 % for the random field) the valid mask and ``n_valid`` are exact, and ``loss``,
``depth_normal`` and the three gradients, each divided by the float64 tensor's max-abs, lie within max(1e-5, 2 x the
float32 restatement's own error) -- the project's bar.  The observed figures are printed (-s).
"""
import functools
import math
import os
import sys
import types

import pytest
import torch

from conftest import ROOT
import normal_consistency_restate as R

sys.path.insert(0, os.path.join(ROOT, "examples"))

pytestmark = pytest.mark.gpu

NAMES = ("depth_normal", "d_depth", "d_alpha", "d_normal")


@functools.lru_cache(maxsize=None)
def _reference(kind, H, W):
    """Inputs, float64 and float32 restatement, fragile mask; computed once, never modified."""
    case = R.make_case(kind, H, W)
    ref = R.restate(*case, *R.TANFOV)
    ref32 = R.restate(*case, *R.TANFOV, dtype=torch.float32)
    return case, ref, ref32, R.fragile_mask(ref)


def _run(dev, case, grads=True):
    """The kernel on a case -> dict like the restatement's (tensors on the CPU), from one call."""
    from mvs_gaussian_splatting_amd import normal_consistency as nc
    depth, alpha, normal = (t.to(dev) for t in case)
    H, W = depth.shape[-2:]
    record, g, dn = nc._call(depth, alpha, normal, H, W, *R.TANFOV, 0.5, grads, True)
    out = {"record": record.cpu(), "loss": record[0].cpu(), "n_valid": int(record.view(torch.int32)[1]),
           "depth_normal": dn.cpu()}
    if grads:
        out.update(d_depth=g[0].cpu().view(H, W), d_alpha=g[1].cpu().view(H, W), d_normal=g[2].cpu())
    return out


def _rel_err(got, ref, ok):
    """max |got - ref| over the pixels of ``ok``, relative to max |ref| (None: ref is all zero there)."""
    scale = float(ref.abs().max())
    if scale == 0.0:
        return None
    keep = ok if ref.dim() == 2 else ok.unsqueeze(0).expand_as(ref)
    if not bool(keep.any()):
        return 0.0
    return float((got.double() - ref.double()).abs()[keep].max()) / scale


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_loss_normals_and_gradients_match_the_float64_restatement(gpu_device, kind, H, W):
    case, ref, ref32, fragile = _reference(kind, H, W)
    ok = ~fragile
    got = _run(gpu_device, case)
    if kind != "random":
        assert not bool(fragile.any())
    got_valid = (got["depth_normal"] != 0).any(dim=0)
    assert torch.equal(got_valid[ok], ref["valid"][ok]), "the valid mask differs on robust pixels"
    if not bool(fragile.any()):
        assert got["n_valid"] == ref["n_valid"]
    assert got["n_valid"] == int(got_valid.sum())
    assert tuple(got["record"][2:].tolist()) == (0.0, 0.0)
    if min(H, W) < 3:
        assert got["n_valid"] == 0 and float(got["loss"]) == 0.0
    figures = []
    for name in NAMES:
        err, err32 = _rel_err(got[name], ref[name], ok), _rel_err(ref32[name], ref[name], ok)
        if err is None:
            assert not bool(got[name].any()), f"{name}: the reference is all zero, the kernel's output is not"
            figures.append(f"{name} zero")
            continue
        bar = max(1e-5, 2.0 * err32)
        figures.append(f"{name} {err:.2e} (float32 {err32:.2e}, bar {bar:.2e})")
        assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"
    l64 = float(ref["loss"])
    if l64 == 0.0:
        assert float(got["loss"]) == 0.0
        figures.append("loss zero")
    else:
        err, err32 = abs(float(got["loss"]) - l64) / abs(l64), abs(float(ref32["loss"]) - l64) / abs(l64)
        bar = max(1e-5, 2.0 * err32)
        figures.append(f"loss {err:.2e} (float32 {err32:.2e}, bar {bar:.2e})")
        if not bool(fragile.any()):
            assert err <= bar, f"loss: {err:.3e} > {bar:.3e}"
    print(f"[normal] {kind} {H}x{W}: n_valid {got['n_valid']}, fragile {int(fragile.sum())}; " + "; ".join(figures))


@pytest.mark.parametrize("H,W", [(3, 3), (17, 33), (67, 131)])
def test_same_bits_from_run_to_run_forward_only_and_through_depth_to_normals(gpu_device, H, W):
    from mvs_gaussian_splatting_amd import depth_to_normals, normal_consistency_loss
    case = _reference("sphere" if H > 3 else "random", H, W)[0]
    a, b, fwd = _run(gpu_device, case), _run(gpu_device, case), _run(gpu_device, case, grads=False)
    for name in ("record", "depth_normal", "d_depth", "d_alpha", "d_normal"):
        assert torch.equal(a[name], b[name]), f"{name} differs between two calls"
    assert torch.equal(a["record"], fwd["record"]) and torch.equal(a["depth_normal"], fwd["depth_normal"])
    depth, alpha, normal = (t.to(gpu_device) for t in case)
    assert torch.equal(depth_to_normals(depth, alpha, *R.TANFOV).cpu(), a["depth_normal"])
    assert torch.equal(depth_to_normals(depth[0], alpha[0], *R.TANFOV, alpha_min=0.5).cpu(), a["depth_normal"])
    # the public function: no input requires a gradient -> the forward-only call, the same value
    loss, record = normal_consistency_loss(depth, alpha, normal, *R.TANFOV, return_record=True)
    assert loss.dim() == 0 and loss.is_cuda and not loss.requires_grad and torch.equal(record.cpu(), a["record"])
    # an upstream gradient of 3 scales the unit gradients; an input that asks for none gets none
    leaves = [t.clone().requires_grad_(True) for t in (depth, alpha, normal)]
    (3.0 * normal_consistency_loss(*leaves, *R.TANFOV)).backward()
    for leaf, name in zip(leaves, ("d_depth", "d_alpha", "d_normal")):
        assert leaf.grad.shape == leaf.shape
        assert torch.equal(leaf.grad.cpu().view(a[name].shape), a[name] * 3.0), name
    only = depth.clone().requires_grad_(True)
    out = normal_consistency_loss(only, alpha, normal, *R.TANFOV)
    out.backward()
    assert torch.equal(only.grad.cpu().view(H, W), a["d_depth"]) and torch.equal(out.detach().cpu(), a["loss"])


def test_alpha_min_moves_the_covered_set_and_an_uncovered_image_gives_zeros(gpu_device):
    from mvs_gaussian_splatting_amd import normal_consistency as nc
    case, ref, _, _ = _reference("plane", 17, 33)                        # alpha in [0.7, 1]
    depth, alpha, normal = (t.to(gpu_device) for t in case)
    hi = R.restate(*case, *R.TANFOV, alpha_min=0.9)
    assert 0 < hi["n_valid"] < ref["n_valid"]
    record, g, dn = nc._call(depth, alpha, normal, 17, 33, *R.TANFOV, 0.9, True, True)
    assert int(record.view(torch.int32)[1]) == hi["n_valid"]
    assert torch.equal((dn != 0).any(dim=0).cpu(), hi["valid"])
    record, g, dn = nc._call(depth, alpha * 0.4, normal, 17, 33, *R.TANFOV, 0.5, True, True)       # nothing covered
    assert not record.any() and not dn.any() and not any(bool(t.any()) for t in g)


# ---- end to end ----------------------------------------------------------------------------------------------------------
PLANE = (0.3, -0.2, 4.0)         # view-space plane z = 4 + 0.3 x - 0.2 y


@pytest.fixture(scope="module")
def problem(gpu_device):
    """A 64x48 frame of 400 flat Gaussians on a tilted plane in front of the example's camera."""
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


def test_render_loss_backward_end_to_end_and_the_frame_path_is_left_alone(gpu_device, problem):
    import train as example
    from mvs_gaussian_splatting_amd import normal_consistency_loss, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cams, bg, _ = problem
    cam, pipe = cams[0], PipelineParams()
    model = _plane_model(problem, example.small_opt(40))
    with torch.no_grad():
        before = render(cam, model, pipe, bg)["render"].clone()
    pkg = render(cam, model, pipe, bg, return_depth=True, return_normals=True)
    tan = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    loss, record = normal_consistency_loss(pkg["depth"], pkg["alpha"], pkg["normal"], *tan, return_record=True)
    loss.backward()
    n_valid = int(record.view(torch.int32)[1])
    print(f"[normal] end to end: loss {float(loss.detach()):.4f}, {n_valid} valid pixels of {64 * 48}")
    assert n_valid > 1500 and 0.0 < float(loss.detach()) < 1.0
    for name in ("_xyz", "_rotation", "_scaling", "_opacity"):
        grad = getattr(model, name).grad
        assert grad is not None and bool(torch.isfinite(grad).all()), name
    assert float(model._xyz.grad.abs().max()) > 0 and float(model._rotation.grad.abs().max()) > 0
    # the depth normals of the rendered plane face the camera and lean the way the plane's normal (a, b, -1) does
    a, b, _ = PLANE
    n_plane = torch.tensor([a, b, -1.0]) / math.sqrt(a * a + b * b + 1.0)
    from mvs_gaussian_splatting_amd import depth_to_normals
    dn = depth_to_normals(pkg["depth"].detach(), pkg["alpha"].detach(), *tan).cpu()
    inner = dn[:, 12:36, 16:48]
    mean = inner.mean(dim=(1, 2))
    print(f"[normal] mean depth normal of the inner frame {mean.tolist()}, plane normal {n_plane.tolist()}")
    assert bool((inner != 0).any(dim=0).all()) and bool((inner[2] < 0).all())
    assert float(mean[0]) > 0 and float(mean[1]) < 0
    with torch.no_grad():
        after = render(cam, model, pipe, bg)["render"]
    assert torch.equal(before, after), "the plain frame changed across the new path"


def test_three_training_iterations_with_the_term_and_bit_identity_without_it(gpu_device, problem):
    import train as example
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    cams, bg, _ = problem
    pipe = PipelineParams()
    opt = example.small_opt(40, lambda_normal=0.05, normal_from_iter=0)
    model = _plane_model(problem, opt)
    plain = _plane_model(problem, example.small_opt(40))
    losses = [float(training_iteration(model, cams[0], opt, pipe, bg, it, cameras_extent=example.CAMERAS_EXTENT))
              for it in (1, 2, 3)]
    base = float(training_iteration(plain, cams[0], example.small_opt(40), pipe, bg, 1, cameras_extent=example.CAMERAS_EXTENT))
    print(f"[normal] three iterations with lambda_normal = 0.05: {losses}; without: {base}")
    assert all(math.isfinite(v) for v in losses) and losses[0] > base, "the term must add to the first loss"
    assert bool(torch.isfinite(model._xyz).all()) and bool(torch.isfinite(model._rotation).all())
    # not yet switched on: the same iteration as without the term
    late = example.small_opt(40, lambda_normal=0.05, normal_from_iter=7000)
    # lambda_normal = 0 against a parent-equivalent call: options that do not know the two fields at all
    zero = example.small_opt(40)
    parent = types.SimpleNamespace(**{k: getattr(zero, k) for k in dir(OptimizationParams)
                                      if not k.startswith("_") and k not in ("lambda_normal", "normal_from_iter")})
    assert zero.lambda_normal == 0.0 and not hasattr(parent, "lambda_normal")
    results = []
    for o in (zero, parent, late):
        m = _plane_model(problem, zero)
        out = [training_iteration(m, cams[0], o, pipe, bg, it, cameras_extent=example.CAMERAS_EXTENT) for it in (1, 2)]
        results.append((out, [getattr(m, n).detach().clone() for n in ("_xyz", "_features_dc", "_features_rest", "_opacity",
                                                                       "_scaling", "_rotation")]))
    for other in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0][0], other[0])), "the loss differs"
        assert all(torch.equal(x, y) for x, y in zip(results[0][1], other[1])), "a parameter differs"
