"""TSDF fusion and marching-tetrahedra extraction on the HIP path (csrc/tsdf.hip; ``tsdf.TSDFVolume``, ``tsdf.fuse_views``;
DESIGN.md §7.14) against the float64 restatement of tests/tsdf_restate.py.

Shapes are chosen for tails: a 19 x 13 x 11 volume (odd x extent, nothing a multiple of 64) under three 37 x 29 views
(no multiple of the 16-pixel tile), the 24 x 20 x 22 sphere of the host test, a 17 x 9 x 21 plane with holes.

Bars.  Integration is compared on the points none of whose float64 comparisons is within tsdf_restate.MARGIN of
flipping (the host test caps their share): ``weight`` exactly (a sum of small integers), ``tsdf`` and ``color`` max-norm
within max(1e-5, 2 x the float32 restatement's own error against float64).  Mesh faces integer for integer; vertices
and colours within the same bar, vertices relative to the volume's extent.  The observed figures are printed (-s).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import small_scene
import tsdf_restate as R

pytestmark = pytest.mark.gpu


def _bar(ref32, ref64, scale=1.0):
    return max(1e-5, 2.0 * float(np.abs(ref32.astype(np.float64) - ref64).max()) / scale)


@functools.lru_cache(maxsize=None)
def _case():
    return R.integration_case()


@functools.lru_cache(maxsize=None)
def _reference(with_color, max_weight):
    """float64 and float32 restatement of the three views; computed once, never modified."""
    _, views = _case()
    return R.run_case(views, with_color, max_weight), R.run_case(views, with_color, max_weight, np.float32)


def _fuse(dev, with_color, max_weight):
    from mvs_gaussian_splatting_amd import TSDFVolume
    cameras, views = _case()
    vol = TSDFVolume(R.CASE_ORIGIN, R.CASE_VOXEL, R.CASE_DIMS, R.CASE_TRUNC, with_color=with_color, device=dev)
    for n, (cam, view) in enumerate(zip(cameras, views)):
        depth = torch.from_numpy(view["depth"]).to(dev)
        vol.integrate(depth if n != 1 else depth.unsqueeze(0), cam,
                      color=torch.from_numpy(view["color"]).to(dev) if with_color else None, weight=1.0,
                      max_depth=view["max_depth"], max_weight=max_weight)
    return vol


@pytest.mark.parametrize("with_color,max_weight", [(True, None), (False, None), (True, 2.0)])
def test_integration_matches_the_float64_restatement(gpu_device, with_color, max_weight):
    (ref, touched, fragile), (ref32, _, _) = _reference(with_color, max_weight)
    vol = _fuse(gpu_device, with_color, max_weight)
    again = _fuse(gpu_device, with_color, max_weight)
    ok = ~fragile
    got_w = vol.weight.cpu().numpy()
    assert np.array_equal(got_w[ok], ref["weight"][ok].astype(np.float32)), "weights differ on robust points"
    if max_weight is not None:
        assert got_w.max() == max_weight and (ref["weight"] == max_weight).sum() > 100
    names = ("tsdf", "color") if with_color else ("tsdf",)
    for name in names:
        got = getattr(vol, name).cpu().numpy().astype(np.float64)
        err = float(np.abs(got - ref[name])[ok].max())
        bar = _bar(ref32[name][ok], ref[name][ok])
        print(f"[tsdf] color={with_color} max_weight={max_weight} {name}: max error {err:.2e}, bar {bar:.2e}, "
              f"{int(touched.sum())} updated points, {int((touched & fragile).sum())} left out")
        assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"
    # points that no view updates (and that are not near a threshold) keep their initial bits
    idle = torch.from_numpy(~touched & ok).to(gpu_device)
    assert bool((vol.tsdf[idle] == 1).all()) and bool((vol.weight[idle] == 0).all())
    if with_color:
        assert bool((vol.color[idle] == 0).all())
    # the same bits from run to run
    assert torch.equal(vol.tsdf, again.tsdf) and torch.equal(vol.weight, again.weight)
    if with_color:
        assert torch.equal(vol.color, again.color)


def _load(field, dev):
    from mvs_gaussian_splatting_amd import TSDFVolume
    nz, ny, nx = field["tsdf"].shape
    vol = TSDFVolume(field["origin"], field["voxel_size"], (nx, ny, nz), field["sdf_trunc"],
                     with_color=field["color"] is not None, device=dev)
    vol.tsdf = torch.from_numpy(field["tsdf"]).to(dev)
    vol.weight = torch.from_numpy(field["weight"]).to(dev)
    if field["color"] is not None:
        vol.color = torch.from_numpy(field["color"]).to(dev)
    return vol


@functools.lru_cache(maxsize=None)
def _mesh_reference(which):
    field = {"sphere": R.sphere_field, "plane": R.plane_field}[which]()
    return field, R.extract(field), R.extract(field, dtype=np.float32)


def _extent(field):
    nz, ny, nx = field["tsdf"].shape
    return field["voxel_size"] * max(nx - 1, ny - 1, nz - 1)


def test_extraction_of_the_closed_sphere(gpu_device):
    field, (rv, rf, rc), (rv32, _, rc32) = _mesh_reference("sphere")
    vol = _load(field, gpu_device)
    vertices, faces, colors = vol.extract_mesh()
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32 and colors.dtype == torch.float32
    assert tuple(vertices.shape) == rv.shape and tuple(colors.shape) == rc.shape
    f = faces.cpu().numpy()
    assert np.array_equal(f, rf), "faces differ from the restatement"
    v, c = vertices.cpu().numpy().astype(np.float64), colors.cpu().numpy().astype(np.float64)
    ext = _extent(field)
    err_v, bar_v = float(np.abs(v - rv).max()) / ext, _bar(rv32, rv, ext)
    err_c, bar_c = float(np.abs(c - rc).max()), _bar(rc32, rc)
    print(f"[tsdf] sphere: V {len(v)} F {len(f)}, vertex error {err_v:.2e} of the extent (bar {bar_v:.2e}), colour error "
          f"{err_c:.2e} (bar {bar_c:.2e})")
    assert err_v <= bar_v and err_c <= bar_c
    R.assert_closed_oriented_sphere(v, f)
    v2, f2, c2 = vol.extract_mesh()
    assert torch.equal(v2, vertices) and torch.equal(f2, faces) and torch.equal(c2, colors)


def test_extraction_of_the_open_plane_with_holes(gpu_device):
    field, (rv, rf, _), (rv32, _, _) = _mesh_reference("plane")
    assert (field["tsdf"] == 0).sum() == 1 and 200 < len(rf) and (field["weight"] == 0).sum() > 300
    vol = _load(field, gpu_device)
    vertices, faces, colors = vol.extract_mesh()
    assert colors is None
    f, v = faces.cpu().numpy(), vertices.cpu().numpy().astype(np.float64)
    assert np.array_equal(f, rf), "faces differ from the restatement"
    assert f.min() >= 0 and f.max() < len(v), "a face index is out of range"
    assert len(np.unique(f)) == len(v), "a vertex is unreferenced"
    ext = _extent(field)
    err, bar = float(np.abs(v - rv).max()) / ext, _bar(rv32, rv, ext)
    print(f"[tsdf] plane: V {len(v)} F {len(f)}, vertex error {err:.2e} of the extent (bar {bar:.2e})")
    assert err <= bar
    # an open surface: some edge has no opposite, none is used twice in one direction
    counts = R.directed_edge_counts(f)
    assert all(n == 1 for n in counts.values()) and any((b, a) not in counts for a, b in counts)


def test_volume_without_a_crossing_gives_empty_tensors(gpu_device):
    from mvs_gaussian_splatting_amd import TSDFVolume
    for with_color in (True, False):
        vol = TSDFVolume((0, 0, 0), 0.5, (7, 5, 3), 1.0, with_color=with_color, device=gpu_device)
        vol.weight.fill_(1.0)                                             # all ones, weighted: processed, no crossing
        vertices, faces, colors = vol.extract_mesh()
        assert tuple(vertices.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and faces.dtype == torch.int32
        assert (colors is None) != with_color and (colors is None or tuple(colors.shape) == (0, 3))
    flat = TSDFVolume((0, 0, 0), 0.5, (9, 1, 4), 1.0, device=gpu_device)   # no cube at all
    flat.weight.fill_(1.0)
    flat.tsdf[:, :, ::2] = -1.0
    assert tuple(flat.extract_mesh()[1].shape) == (0, 3)


def test_fuse_views_equals_the_hand_filled_volume_and_leaves_the_frame_path_alone(gpu_device):
    from mvs_gaussian_splatting_amd import TSDFVolume, fuse_views, render
    from mvs_gaussian_splatting_amd.synthetic import PipelineParams
    dev = gpu_device
    model, cam0, bg, _ = small_scene(scale=0.08)
    cameras = [cam0.to(dev)] + [small_scene(P=1, view=v)[1].to(dev) for v in (1, 3)]
    model.to(dev)
    bg, pipe = bg.to(dev), PipelineParams()
    make = lambda: TSDFVolume((-2.0, -1.5, 3.0), 0.125, (33, 25, 41), 0.5, device=dev)        # noqa: E731
    with torch.no_grad():
        before = render(cameras[1], model, pipe, bg, return_depth=True)
    fused = fuse_views(cameras, model, pipe, bg, make(), alpha_min=0.5, max_depth=7.5)
    by_hand = make()
    with torch.no_grad():
        for cam in cameras:
            pkg = render(cam, model, pipe, bg, return_depth=True)
            expected = torch.where(pkg["alpha"] >= 0.5, pkg["depth"] / pkg["alpha"], torch.zeros_like(pkg["depth"]))
            by_hand.integrate(expected, cam, color=pkg["render"], max_depth=7.5)
        after = render(cameras[1], model, pipe, bg, return_depth=True)
    updated = int((fused.weight > 0).sum())
    print(f"[tsdf] fuse_views: {updated} of {fused.weight.numel()} points updated, largest weight {float(fused.weight.max())}")
    assert updated > 1000
    for name in ("tsdf", "weight", "color"):
        assert torch.equal(getattr(fused, name), getattr(by_hand, name)), name
    for name in ("render", "depth", "invdepth", "alpha", "radii"):
        assert torch.equal(before[name], after[name]), f"{name} of the same frame changed across the fusion"
