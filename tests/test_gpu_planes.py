"""PGSR's unbiased plane depth on the GPU: ``csrc/planes.hip`` and ``csrc/plane_depth.hip`` against the
float64 restatement (tests/planes_restate.py) at the bar of twice the float32 restatement's own error, their decisions,
bit-reproducibility, and the feature through ``render``, ``training_iteration`` and ``fuse_views``."""
import functools
import math
import os
import sys
import types

import pytest
import torch

from conftest import ROOT
import planes_restate as R

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(ROOT, "examples"))


def _bar(tag, got, r32, r64, mask=None):
    """got within twice the float32 restatement's own error of the float64 one (the project's standing rule); both as
    a share of the largest magnitude of the float64 tensor."""
    got, r32, r64 = got.detach().cpu(), r32.detach(), r64.detach()
    if mask is not None:
        got, r32, r64 = got[..., mask], r32[..., mask], r64[..., mask]
    err, own = R.rel_err(got, r64), R.rel_err(r32, r64)
    print(f"[planes] {tag}: error {err:.3e}, float32 restatement {own:.3e}, bar {2 * own:.3e}")
    assert err <= 2 * own, f"{tag}: {err:.3e} above twice the float32 restatement's {own:.3e}"


@functools.lru_cache(maxsize=None)
def _rows_reference(P):
    """The rows, a random upstream, and the restatement at float64 and float32 with both gradients: computed once."""
    vm, cp = R.row_camera()
    s, q, m = R.make_rows(P)
    up = torch.randn(P, 4, generator=torch.Generator().manual_seed(17))
    refs = []
    for dtype in (torch.float64, torch.float32):
        qg, mg = q.clone().to(dtype).requires_grad_(True), m.clone().to(dtype).requires_grad_(True)
        out = R.planes(s, qg, mg, vm, cp, dtype)
        out["planes"].backward(up.to(dtype))
        refs.append(dict(out, planes=out["planes"].detach(), d_rot=qg.grad, d_mean=mg.grad))
    return (s, q, m, vm, cp, up), refs[0], refs[1]


def _raw_rows(dev, s, q, m, vm, cp, up, fill=None):
    from mvs_gaussian_splatting_amd import features as F
    sd, qd, md, ud = (t.to(dev).contiguous() for t in (s, q, m, up))
    cam = F._host_camera(vm, cp)
    P = q.shape[0]
    outs = None
    if fill is not None:
        outs = [torch.full(shape, fill, dtype=torch.float32, device=dev) for shape in ((P, 4), (P, 4), (P, 3))]
    planes = F.planes_forward_raw(sd, qd, md, *cam, out=None if outs is None else outs[0])
    d_rot, d_mean = F.planes_backward_raw(sd, qd, md, *cam, ud, out=None if outs is None else (outs[1], outs[2]))
    return planes, d_rot, d_mean


@pytest.mark.parametrize("P", R.ROW_SIZES)
def test_planes_kernel_matches_the_restatement_and_its_decisions(gpu_device, P):
    inputs, r64, r32 = _rows_reference(P)
    planes, d_rot, d_mean = _raw_rows(gpu_device, *inputs)
    torch.cuda.synchronize()
    firm = ~r64["fragile"]
    # a wrong axis or sign moves the unit normal by order one: decisions are read off it, exact ties and a facing of
    # exactly 0 (which the restatement resolves by the stated rules) included
    off = (planes.cpu().double()[:, :3] - r64["planes"][:, :3]).abs().max(dim=1).values
    assert float(off[firm].max()) < 1e-5, "axis or sign differs from the float64 restatement on a firm row"
    assert float(planes[:, 3].min()) >= 0.0 and bool(torch.isfinite(planes).all())
    assert bool(torch.isfinite(d_rot).all()) and bool(torch.isfinite(d_mean).all())
    if P > 6:
        assert not bool(d_rot[6].any()), "the all-zero quaternion has no gradient"
    same = firm & ~r32["fragile"] & (r32["axis"] == r64["axis"]) & (r32["sign"].double() == r64["sign"])
    rows = same.nonzero().view(-1)
    for tag, got, key in (("planes", planes, "planes"), ("dL/drotations", d_rot, "d_rot"), ("dL/dmeans3D", d_mean, "d_mean")):
        g = got.cpu()[rows]
        err, own = R.rel_err(g, r64[key][rows]), R.rel_err(r32[key][rows], r64[key][rows])
        print(f"[planes] P={P} {tag}: error {err:.3e}, float32 restatement {own:.3e}, bar {2 * own:.3e}")
        assert err <= 2 * own, f"P={P} {tag}: {err:.3e} above twice the float32 restatement's {own:.3e}"
    # the same bits from run to run and into garbage-filled outputs
    for fill in (None, float("nan"), -7.0):
        again = _raw_rows(gpu_device, *inputs, fill=fill)
        for a, b in zip(again, (planes, d_rot, d_mean)):
            assert torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _maps_reference(W, H):
    N, D, A = R.make_maps(W, H)
    return (N, D, A), R.plane_depth(N, D, A, *R.TANFOV), R.plane_depth(N, D, A, *R.TANFOV, dtype=torch.float32)


def _raw_maps(dev, N, D, A, want_grads=True, fill=None):
    from mvs_gaussian_splatting_amd import surface as S
    H, W = D.shape
    out = None
    if fill is not None:
        out = [torch.full(shape, fill, dtype=torch.float32, device=dev) for shape in ((H, W), (H, W), (3, H, W))]
        if not want_grads:
            out[1] = out[2] = None
    return S.plane_depth_raw(N.to(dev).contiguous(), D.to(dev).contiguous(), A.to(dev).contiguous(), H, W, *R.TANFOV,
                             0.5, 0.05, want_grads, out=out)


@pytest.mark.parametrize("shape", R.MAP_SHAPES)
def test_plane_depth_kernel_matches_the_restatement_and_its_mask(gpu_device, shape):
    from mvs_gaussian_splatting_amd import surface as S
    (N, D, A), r64, r32 = _maps_reference(*shape)
    z, ud, un = _raw_maps(gpu_device, N, D, A)
    torch.cuda.synchronize()
    firm = ~r64["fragile"]
    valid = (ud != 0).cpu()
    assert torch.equal(valid[firm], r64["valid"][firm]), "the validity mask differs off the fragile pixels"
    for t in (z, ud, un):
        assert not bool(torch.isnan(t).any())
        assert not bool(t.cpu()[..., ~valid].any()), "a pixel that is not valid is exactly 0 in every output"
    mask = firm & r64["valid"] & r32["valid"]
    tag = f"{shape[0]}x{shape[1]}"
    _bar(f"{tag} z", z, r32["z"], r64["z"], mask)
    _bar(f"{tag} dz/dD", ud, r32["dz_dD"], r64["dz_dD"], mask)
    _bar(f"{tag} dz/dN", un, r32["dz_dN"], r64["dz_dN"], mask)
    # the backward launch: the unit gradients times an upstream map, 0 where the pixel is not valid whatever it holds
    H, W = D.shape
    up = torch.randn(H, W, generator=torch.Generator().manual_seed(23)).to(gpu_device)
    up[~valid.to(gpu_device)] = float("nan")
    g_d, g_n = S.plane_depth_backward_raw(up, ud, un, H, W)
    clean = torch.where(valid.to(gpu_device), up, torch.zeros_like(up))
    assert torch.equal(g_d, clean * ud) and torch.equal(g_n, clean * un)
    # repeat runs, garbage-filled outputs, and the value-only call: the same bits
    for fill in (None, float("nan"), 3.0):
        again = _raw_maps(gpu_device, N, D, A, fill=fill)
        assert all(torch.equal(a, b) for a, b in zip(again, (z, ud, un)))
        assert torch.equal(_raw_maps(gpu_device, N, D, A, want_grads=False, fill=fill)[0], z)
        outs = None if fill is None else (torch.full_like(g_d, fill), torch.full_like(g_n, fill))
        assert all(torch.equal(a, b) for a, b in zip(S.plane_depth_backward_raw(up, ud, un, H, W, out=outs), (g_d, g_n)))


def test_wrappers_equal_the_raw_calls_autograd_scales_and_no_rows_is_a_no_op(gpu_device):
    from mvs_gaussian_splatting_amd import gaussian_planes, plane_depth
    dev = gpu_device
    (s, q, m, vm, cp, up), _, _ = _rows_reference(257)
    planes, d_rot, d_mean = _raw_rows(dev, s, q, m, vm, cp, up * -2.5)
    qd, md = q.to(dev).requires_grad_(True), m.to(dev).requires_grad_(True)
    out = gaussian_planes(s.to(dev), qd, md, vm.to(dev), cp.to(dev))
    assert torch.equal(out, planes)
    (out * up.to(dev)).sum().mul(-2.5).backward()
    assert torch.equal(qd.grad, d_rot) and torch.equal(md.grad, d_mean)
    # an incoming gradient that is not 16-byte aligned is copied, not refused
    shifted = torch.zeros(257 * 4 + 4, device=dev)[1:1 + 257 * 4].view(257, 4).copy_(up.to(dev) * -2.5)
    assert shifted.data_ptr() % 16 != 0 and shifted.is_contiguous()
    q2, m2 = q.to(dev).requires_grad_(True), m.to(dev).requires_grad_(True)
    gaussian_planes(s.to(dev), q2, m2, vm, cp).backward(shifted)
    assert torch.equal(q2.grad, d_rot) and torch.equal(m2.grad, d_mean)
    # a view that is not 16-byte aligned is copied, not refused
    block = torch.zeros(258, 4, device=dev).view(-1)[1:1 + 257 * 4].view(257, 4).copy_(q.to(dev))
    assert block.data_ptr() % 16 != 0 and torch.equal(gaussian_planes(s.to(dev), block, m.to(dev), vm, cp), planes)
    empty = gaussian_planes(torch.zeros(0, 3, device=dev), torch.zeros(0, 4, device=dev, requires_grad=True),
                            torch.zeros(0, 3, device=dev), vm, cp)
    assert tuple(empty.shape) == (0, 4)
    empty.sum().backward()

    (N, D, A), _, _ = _maps_reference(70, 37)
    z, ud, un = _raw_maps(dev, N, D, A)
    Nd, Dd = N.to(dev).requires_grad_(True), D.to(dev)[None].requires_grad_(True)
    got = plane_depth(Nd, Dd, A.to(dev)[None], *R.TANFOV)
    assert tuple(got.shape) == (1, 37, 70) and torch.equal(got[0], z)
    assert torch.equal(plane_depth(N.to(dev), D.to(dev), A.to(dev), *R.TANFOV)[0], z), "value only: the same bits"
    upz = torch.randn(1, 37, 70, generator=torch.Generator().manual_seed(29)).to(dev)
    (got * upz).sum().mul(-2.5).backward()
    assert torch.equal(Dd.grad[0], (upz[0] * -2.5) * ud) and torch.equal(Nd.grad, (upz[0] * -2.5) * un)
    assert bool(torch.isfinite(Nd.grad).all()) and float(Nd.grad.abs().max()) > 0


# ---- through render, the trainer and TSDF fusion ---------------------------------------------------------------------
PLANE = (0.8, -0.2, 4.0)         # view-space plane z = 4 + 0.8 x - 0.2 y in the first camera: tilted about 39 degrees


@pytest.fixture(scope="module")
def problem(gpu_device):
    """Two 64x48 views, 15 degrees apart, of 400 flat Gaussians lying IN a tilted plane (their normals are the plane's)."""
    import train as example
    cams, bg, _ = example.make_problem(gpu_device, P=600, W=64, H=48, n_views=24)
    g = torch.Generator().manual_seed(11)
    xy = (torch.rand(400, 2, generator=g) - 0.5) * torch.tensor([1.5, 1.2])
    view = torch.cat((xy, (PLANE[2] + PLANE[0] * xy[:, :1] + PLANE[1] * xy[:, 1:]), torch.ones(400, 1)), dim=1)
    world = (view.to(gpu_device) @ torch.linalg.inv(cams[0].world_view_transform.float()))[:, :3].contiguous()
    colors = torch.rand(400, 3, generator=g).to(gpu_device)
    n_view = torch.tensor([PLANE[0], PLANE[1], -1.0])
    n_view = n_view / n_view.norm()
    n_world = (n_view.to(gpu_device) @ cams[0].world_view_transform.float()[:3, :3].t()).contiguous()
    return cams[:2], bg, (world, colors), n_world


def _plane_model(problem, opt):
    import train as example
    model = example.make_model(problem[:3], opt)
    n = problem[3]
    zaxis = torch.tensor([0.0, 0.0, 1.0], device=n.device)
    quat = torch.cat(((1.0 + zaxis @ n).view(1), torch.linalg.cross(zaxis, n)))      # takes the z axis to n
    with torch.no_grad():
        model._opacity.fill_(2.0)
        model._scaling[:, :2] = math.log(0.07)
        model._scaling[:, 2] = math.log(0.004)
        model._rotation.copy_((quat / quat.norm()).expand_as(model._rotation))
    return model


def test_render_returns_the_plane_maps_with_gradients_and_leaves_the_normal_path_alone(gpu_device, problem):
    import train as example
    from mvs_gaussian_splatting_amd import gaussian_planes, plane_depth, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cams, bg, _, _ = problem
    cam, pipe = cams[0], PipelineParams()
    model = _plane_model(problem, example.small_opt(40))
    tan = (math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
    before = render(cam, model, pipe, bg, return_normals=True)["normal"].detach().clone()
    pkg = render(cam, model, pipe, bg, return_plane_depth=True)
    for key, channels in (("distance", 1), ("plane_depth", 1), ("normal", 3), ("depth", 1), ("alpha", 1)):
        assert tuple(pkg[key].shape) == (channels, 48, 64), key
    rows = gaussian_planes(model.get_scaling, model.get_rotation, model.get_xyz, cam.world_view_transform, cam.camera_center)
    user = torch.rand(400, 2, generator=torch.Generator().manual_seed(5)).to(gpu_device)
    explicit = render(cam, model, pipe, bg, return_depth=True, features=torch.cat([user, rows], dim=1))
    assert torch.equal(explicit["features"][2:5], pkg["normal"]) and torch.equal(explicit["features"][5:6], pkg["distance"])
    assert torch.equal(plane_depth(explicit["features"][2:5], explicit["features"][5:6], explicit["alpha"], *tan),
                       pkg["plane_depth"])
    both = render(cam, model, pipe, bg, return_plane_depth=True, features=user, return_median_depth=True,
                  return_distortion=True)
    assert torch.equal(both["plane_depth"], pkg["plane_depth"]) and torch.equal(both["features"], explicit["features"][:2])
    assert "median_depth" in both and "distortion" in both
    covered = pkg["plane_depth"] > 0
    assert int(covered.sum()) > 1000
    # on Gaussians that lie in one plane the map IS that plane's depth; depth / alpha is not
    fx, fy = 64 / (2 * tan[0]), 48 / (2 * tan[1])
    ys, xs = torch.meshgrid(torch.arange(48.0), torch.arange(64.0), indexing="ij")
    rx, ry = ((xs - 31.5) / fx).to(gpu_device), ((ys - 23.5) / fy).to(gpu_device)
    truth = PLANE[2] / (1.0 - PLANE[0] * rx - PLANE[1] * ry)
    err_plane = float((pkg["plane_depth"][0] - truth).abs()[covered[0]].mean())
    err_expected = float((pkg["depth"][0] / pkg["alpha"][0] - truth).abs()[covered[0]].mean())
    print(f"[planes] rendered plane: mean |z - truth| {err_plane:.3e} (plane depth), {err_expected:.3e} (depth / alpha)")
    assert err_plane < err_expected
    model.optimizer.zero_grad(set_to_none=True)
    pkg["plane_depth"].sum().backward()
    # the exact sets, from the colour pass's own blending weights: the rows composited at one pixel with a plane depth
    # at least must all have a gradient, the rows composited nowhere must have none
    from mvs_gaussian_splatting_amd import ContributionStats
    on_surface, anywhere = ContributionStats(400, gpu_device), ContributionStats(400, gpu_device)
    with torch.no_grad():
        render(cam, model, pipe, bg, contribution=on_surface, contribution_mask=covered[0].to(torch.uint8).contiguous())
        render(cam, model, pipe, bg, contribution=anywhere)
    contributes, nowhere = on_surface.weight_sum() > 0, anywhere.pixel_count() == 0
    print(f"[planes] {int(contributes.sum())} of 400 rows are composited at a pixel with a plane depth, "
          f"{int(nowhere.sum())} nowhere; {int(pkg['visibility_filter'].sum())} lie in the frustum")
    assert int(contributes.sum()) > 100 and int(nowhere.sum()) > 0, "both sets are present"
    for name in ("_xyz", "_rotation"):
        grad = getattr(model, name).grad
        assert grad is not None and bool(torch.isfinite(grad).all()), name
        assert bool((grad[contributes].abs().sum(dim=1) > 0).all()), f"{name}: a row of the surface got no gradient"
        assert not bool(grad[nowhere].any()), f"{name}: a row that is composited nowhere got a gradient"
    after = render(cam, model, pipe, bg, return_normals=True)["normal"]
    assert torch.equal(before, after), "render(return_normals=True) changed its bits"
    assert "distance" not in render(cam, model, pipe, bg, return_normals=True, return_depth=True)


def test_training_iterations_on_the_unbiased_depth_and_bit_identity_with_the_switch_off(gpu_device, problem):
    import train as example
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    from mvs_gaussian_splatting_amd.trainer import OptimizationParams, training_iteration
    cams, bg, _, _ = problem
    pipe, extent = PipelineParams(), example.CAMERAS_EXTENT
    names = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
    snapshot = lambda m: [getattr(m, n).detach().clone() for n in names]      # noqa: E731
    terms = (dict(lambda_normal=0.05, normal_from_iter=0),
             dict(lambda_multi_view_geo=0.05, multi_view_from_iter=0, multi_view_pix_max=8.0),
             dict(lambda_multi_view_ncc=0.15, multi_view_from_iter=0, multi_view_ncc_samples=2000, multi_view_pix_max=8.0,
                  multi_view_ncc_max=2.0),
             dict(lambda_normal=0.05, normal_from_iter=0, depth_ratio=0.5))
    for optimizer_type in ("default", "sparse_adam"):
        for term in terms:
            on = example.small_opt(40, optimizer_type=optimizer_type, unbiased_depth=True, **term)
            model = _plane_model(problem, on)
            before = snapshot(model)
            loss = training_iteration(model, cams[0], on, pipe, bg, 1, cameras_extent=extent, source_camera=cams[1])
            after = snapshot(model)
            print(f"[planes] one iteration ({optimizer_type}) with unbiased_depth and {term}: {float(loss):.6f}")
            assert math.isfinite(float(loss)) and all(bool(torch.isfinite(a).all()) for a in after)
            assert not torch.equal(after[0], before[0]) and not torch.equal(after[5], before[5]), "the parameters moved"
            assert float(model.denom.sum()) > 0, "the densification statistics were not taken"
    # the switch off, the switch on without a geometry term, and options that do not know the field: the same bits
    zero = example.small_opt(40)
    off = example.small_opt(40, unbiased_depth=False)
    idle = example.small_opt(40, unbiased_depth=True, lambda_dist=0.0)
    parent = types.SimpleNamespace(**{k: getattr(zero, k) for k in dir(OptimizationParams)
                                      if not k.startswith("_") and k != "unbiased_depth"})
    assert not hasattr(parent, "unbiased_depth")
    results = []
    for o in (zero, off, idle, parent):
        m = _plane_model(problem, zero)
        out = [training_iteration(m, cams[0], o, pipe, bg, it, cameras_extent=extent) for it in (1, 2)]
        results.append((out, snapshot(m)))
    for other in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0][0], other[0])), "the loss differs"
        assert all(torch.equal(x, y) for x, y in zip(results[0][1], other[1])), "a parameter differs"


def test_fusing_the_unbiased_depth_puts_the_mesh_closer_to_the_plane(gpu_device, problem):
    import train as example
    from mvs_gaussian_splatting_amd import fuse_views, volume_for_points
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    cams, bg, (world, _), n_world = problem
    model = _plane_model(problem, example.small_opt(40))
    distance = {}
    for unbiased in (False, True):
        volume = volume_for_points(world, resolution=64)
        fuse_views(cams, model, PipelineParams(), bg, volume, **({"unbiased_depth": True} if unbiased else {}))
        vertices, faces, _ = volume.extract_mesh()
        assert vertices.shape[0] > 500 and faces.shape[0] > 500
        distance[unbiased] = float(((vertices - world[0]) @ n_world).abs().mean())
    print(f"[planes] mesh of a planar cloud, mean |distance to the plane|: {distance[False]:.3e} fusing depth / alpha, "
          f"{distance[True]:.3e} fusing the plane depth")
    assert distance[True] < distance[False]
