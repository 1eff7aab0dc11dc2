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


# ---- past one x-chunk, one weight, one frustum ----------------------------------------------------------------------------
# Inputs and their census: tests/tsdf_restate.py (wide_case, random_field, seam_sphere_field, fusion_case) and
# tests/test_tsdf_host.py.  Every comparison is against the float64 restatement, with the bar of the tests above.
@functools.lru_cache(maxsize=None)
def _wide(n):
    return R.wide_case(n)


@functools.lru_cache(maxsize=None)
def _wide_reference(n, with_color, max_weight, preload):
    """float64 and float32 restatement of the case's views; computed once, never modified."""
    return (R.run_wide(_wide(n), with_color, max_weight, preload),
            R.run_wide(_wide(n), with_color, max_weight, preload, np.float32))


def _wide_start(n, with_color, preload, dev):
    from mvs_gaussian_splatting_amd import TSDFVolume
    case = _wide(n)
    vol = TSDFVolume(case["origin"], case["voxel_size"], case["dims"], case["sdf_trunc"], with_color=with_color, device=dev)
    if preload:
        vol.tsdf = torch.from_numpy(case["preload"]["tsdf"]).to(dev)
        vol.weight = torch.from_numpy(case["preload"]["weight"]).to(dev)
        if with_color:
            vol.color = torch.from_numpy(case["preload"]["color"]).to(dev)
    return vol


def _fuse_wide(dev, n, with_color, max_weight, preload):
    case = _wide(n)
    vol = _wide_start(n, with_color, preload, dev)
    for v, (cam, view) in enumerate(zip(case["cameras"], case["views"])):
        depth = torch.from_numpy(view["depth"]).to(dev)
        if v == 0:                                                           # [1,H,W], a valid row directly above and below it
            guard = torch.from_numpy(view["guard"]).to(dev)
            padded = torch.cat((guard[:1], depth, guard[1:]))
            depth = padded[1:-1].unsqueeze(0)
            assert depth.is_contiguous() and depth.data_ptr() == padded.data_ptr() + 4 * view["W"]
        if v == 2:                                                           # every other column of a wider map
            wider = torch.ones((view["H"], 2 * view["W"]), dtype=torch.float32, device=dev)
            wider[:, ::2] = depth
            depth = wider[:, ::2]
            assert not depth.is_contiguous()
        vol.integrate(depth, cam, color=torch.from_numpy(view["color"]).to(dev) if with_color else None,
                      weight=view["weight"], max_depth=view["max_depth"], max_weight=max_weight)
    return vol


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("with_color,max_weight,preload", [(True, None, False), (False, None, False), (True, 3.0, False),
                                                           (False, 3.0, False), (True, 3.0, True)])
@pytest.mark.parametrize("n", range(len(R.WIDE_DIMS)))
def test_integration_past_one_x_chunk_with_points_outside_the_frustum(gpu_device, n, with_color, max_weight, preload):
    """Volumes of 65, 130 and 128 points in x (two or three x-chunks, ragged in x and in rows) under a camera inside
    the volume, an image the volume overflows on all four sides, invalid depth of every kind, weights 0.5 / 2.25 / 1 and
    a pre-loaded state.  Fails if the ``%`` and ``/`` of ``tsdf_point`` are swapped or ``i < nx`` is dropped (points of
    the second chunk land on other rows: wrong values, idle points written), if ``z > 0.2`` is dropped (the points
    behind the inside camera project into its image and are updated), if one of the four bounds tests is dropped or
    relaxed by a pixel (``fpx < W`` to ``<=``, ``fpx >= 0`` to ``>= -1``: in the 13 x 11 view the pixel then read, the
    far end of the neighbouring row, is a valid depth inside the band for 20 or more robust points; ``fpy`` likewise in
    the overview, whose map lies between two rows of valid depth in one allocation: the host census counts these points
    per side), if a NaN depth updates, if ``d > 0`` becomes ``d >= 0`` (volume 1 only, where sdf_trunc = 0.3 > 0.2 leaves
    points over 0 pixels that no later test stops), if ``view.weight`` is ignored (weights and averages differ), and
    if the average divides by the clamped sum (the last view lifts 2.75 to 3.75, clamped to 3; pre-loaded weights of 4
    are clamped by the first).  Not visible here: a negative depth that passes ``d > 0`` -- with z > 0.2 its sdf is
    below -sdf_trunc for any truncation a volume of this size can have, so the next test skips it."""
    (ref, touched, fragile, _), (ref32, _, _, _) = _wide_reference(n, with_color, max_weight, preload)
    vol = _fuse_wide(gpu_device, n, with_color, max_weight, preload)
    again = _fuse_wide(gpu_device, n, with_color, max_weight, preload)
    start = _wide_start(n, with_color, preload, gpu_device)
    ok = ~fragile
    got_w = vol.weight.cpu().numpy()
    assert np.array_equal(got_w[ok], ref["weight"][ok].astype(np.float32)), "weights differ on robust points"
    if max_weight is not None and not preload:
        assert got_w.max() == max_weight and int((got_w == max_weight).sum()) > 20
    names = ("tsdf", "color") if with_color else ("tsdf",)
    for name in names:
        got = getattr(vol, name).cpu().numpy().astype(np.float64)
        err = float(np.abs(got - ref[name])[ok].max())
        bar = _bar(ref32[name][ok], ref[name][ok])
        print(f"[tsdf] wide {R.WIDE_DIMS[n]} color={with_color} max_weight={max_weight} preload={preload} {name}: max error "
              f"{err:.2e}, bar {bar:.2e}, {int(touched.sum())} updated points, {int(fragile.sum())} left out")
        assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"
    # points that no view updates keep the bits they started with
    idle = torch.from_numpy(~touched & ok).to(gpu_device)
    assert int(idle.sum()) > 200
    for name in ("tsdf", "weight") + (("color",) if with_color else ()):
        assert _same_bits(getattr(vol, name)[idle], getattr(start, name)[idle]), f"{name} of a skipped point was written"
        assert _same_bits(getattr(vol, name), getattr(again, name)), f"{name} differs from run to run"


@functools.lru_cache(maxsize=None)
def _field(which):
    return R.seam_sphere_field() if which == "seam" else R.random_field(int(which))


@functools.lru_cache(maxsize=None)
def _field_reference(which, min_weight):
    field = _field(which)
    return R.extract(field, min_weight), R.extract(field, min_weight, np.float32), R.mesh_census(field, min_weight)


def _check_mesh(label, field, vol, min_weight, ref, ref32, census):
    """The device's mesh of ``vol`` against the restatement's (faces exactly, vertices and colours within the bar), and
    on its own: index range, every vertex referenced and on the grid edge its rank in the (owner, direction) order names."""
    (rv, rf, rc), (rv32, _, rc32) = ref, ref32
    vertices, faces, colors = vol.extract_mesh(min_weight=min_weight)
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32
    assert vertices.dim() == 2 and vertices.shape[1] == 3 and faces.dim() == 2 and faces.shape[1] == 3
    assert (colors is None) == (field["color"] is None)
    if colors is not None:
        assert colors.dtype == torch.float32 and colors.shape == vertices.shape
    assert tuple(vertices.shape) == rv.shape and tuple(faces.shape) == rf.shape, "another number of vertices or faces"
    f, v = faces.cpu().numpy(), vertices.cpu().numpy().astype(np.float64)
    assert np.array_equal(f, rf), "faces differ from the restatement"
    assert f.min() >= 0 and f.max() < len(v), "a face index is out of range"
    assert len(np.unique(f)) == len(v), "a vertex is unreferenced"
    ext = _extent(field)
    err_v, bar_v = float(np.abs(v - rv).max()) / ext, _bar(rv32, rv, ext)
    line = f"[tsdf] {label}: V {len(v)} F {len(f)}, vertex error {err_v:.2e} of the extent (bar {bar_v:.2e})"
    assert err_v <= bar_v, line
    if colors is not None:
        err_c, bar_c = float(np.abs(colors.cpu().numpy().astype(np.float64) - rc).max()), _bar(rc32, rc)
        line += f", colour error {err_c:.2e} (bar {bar_c:.2e})"
        assert err_c <= bar_c, line
    # without the restatement's vertices: vertex n lies on the segment from its owner to the owner's neighbour
    assert len(census["ends"]) == len(v)
    pa, pb = (np.array(field["origin"]) + field["voxel_size"] * census["ends"][:, e, :].astype(np.float64) for e in (0, 1))
    ab = pb - pa
    s = np.einsum("ni,ni->n", v - pa, ab) / np.einsum("ni,ni->n", ab, ab)
    away = float(np.linalg.norm(v - pa - s[:, None] * ab, axis=1).max()) / ext
    slack = bar_v * ext / field["voxel_size"]
    print(line + f", {away:.2e} of the extent off the owners' edges, s in [{s.min():.6f}, {s.max():.6f}]")
    assert away <= bar_v and s.min() >= -slack and s.max() <= 1.0 + slack
    v2, f2, c2 = vol.extract_mesh(min_weight=min_weight)
    assert torch.equal(f2, faces) and _same_bits(v2, vertices) and (colors is None or _same_bits(c2, colors))
    return v, f


@pytest.mark.parametrize("which", ["0", "1", "2"])
def test_extraction_of_random_sign_fields_across_x_chunks(gpu_device, which):
    """65 x 3 x 7, 70 x 6 x 5 and 130 x 5 x 3 fields of random sign with holes and signed zeros: every mixed cube pattern,
    several sheets per cube, edges shared by processed and unprocessed cubes, neighbours in another workgroup's chunk.
    Fails if one row of ``CASE_EDGE`` has two entries swapped or a ``TET_CORNER`` row is wrong (faces differ: all 84
    (tetrahedron, case) pairs occur), if ``tsdf <= 0`` counts as inside (the 0.0 and -0.0 samples change faces), if the
    ``%`` and ``/`` of ``tsdf_point`` are swapped or the chunk of a neighbour is mistaken (counts and indices differ
    beyond i = 63), if an edge of an unprocessed cube alone is emitted or one shared with a processed cube is dropped
    (V differs), and if ``DIR_OF_BITS`` / ``BITS_OF_DIR`` disagree (vertices leave their owners' edges)."""
    field = _field(which)
    ref, ref32, census = _field_reference(which, 1e-6)
    _check_mesh(f"random {R.RANDOM_DIMS[int(which)]}", field, _load(field, gpu_device), 1e-6, ref, ref32, census)


@pytest.mark.parametrize("min_weight", [0.0, 2.0, float("inf")])
def test_extraction_honours_min_weight(gpu_device, min_weight):
    """70 x 6 x 5 random field, weights in {0, 1, 2, 3}.  0: the weight-0 cubes are processed too; 2: cubes with a corner
    of weight 1 are not; inf: nothing is, ``[0,3]`` tensors.  Fails if ``min_weight`` is ignored or compared with ``>``
    (at 2.0 the corners of weight exactly 2 would drop out), and if the empty case launches or returns other shapes."""
    field = _field("1")
    vol = _load(field, gpu_device)
    if min_weight == float("inf"):
        vertices, faces, colors = vol.extract_mesh(min_weight=min_weight)
        assert tuple(vertices.shape) == (0, 3) and tuple(faces.shape) == (0, 3) and tuple(colors.shape) == (0, 3)
        assert vertices.dtype == torch.float32 and faces.dtype == torch.int32 and colors.dtype == torch.float32
        assert len(R.extract(field, min_weight)[1]) == 0
        return
    ref, ref32, census = _field_reference("1", min_weight)
    _, f = _check_mesh(f"random {R.RANDOM_DIMS[1]} min_weight={min_weight}", field, vol, min_weight, ref, ref32, census)
    assert len(f) != len(_field_reference("1", 1e-6)[0][1]), "min_weight changed nothing"


def test_extraction_of_a_closed_sphere_across_the_chunk_seam(gpu_device):
    """The sphere of radius 8 centred at x = 63.6 in 96 x 20 x 22: its surface crosses i = 63 | 64, so cubes of chunk 0 read
    corners in chunk 1 and vertices owned at i = 63 are referenced from both.  Fails if a neighbour across the seam is
    mislocated (faces differ, the mesh opens) or if vertex ranks of the two chunks' workgroups disagree."""
    field = _field("seam")
    ref, ref32, census = _field_reference("seam", 1e-6)
    v, f = _check_mesh("seam sphere", field, _load(field, gpu_device), 1e-6, ref, ref32, census)
    R.assert_closed_oriented_sphere(v, f)
    e = census["ends"]
    assert int(((e[:, 0, 0] == 63) & (e[:, 1, 0] == 64)).sum()) >= 50


@functools.lru_cache(maxsize=None)
def _fusion_reference():
    cameras, views = R.fusion_case()
    return cameras, views, R.run_fusion(views), R.run_fusion(views, np.float32)


def test_fusing_a_sphere_from_six_views_and_meshing_it_across_the_seam(gpu_device):
    """Depth of an analytic sphere from six free-pose cameras into 80 x 24 x 23 (two x-chunks, the sphere on the seam),
    then the mesh of what was fused.  Integration against the float64 restatement as above; extraction against the
    restatement run on the device's own fused fields, so a sign that differs at a fragile point cannot fail it; and every
    vertex between two samples of weight >= 2 within one voxel of the sphere.  Fails if either half mislocates points of
    the second chunk: the fused surface would break at i = 64 and leave the sphere."""
    from mvs_gaussian_splatting_amd import TSDFVolume
    cameras, views, (ref, fragile), (ref32, _) = _fusion_reference()
    vol = TSDFVolume(R.FUSE_ORIGIN, R.FUSE_VOXEL, R.FUSE_DIMS, R.FUSE_TRUNC, with_color=False, device=gpu_device)
    for cam, view in zip(cameras, views):
        vol.integrate(torch.from_numpy(view["depth"]).to(gpu_device), cam)
    ok = ~fragile
    tsdf, weight = vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy()
    assert np.array_equal(weight[ok], ref["weight"][ok].astype(np.float32)), "weights differ on robust points"
    err, bar = float(np.abs(tsdf.astype(np.float64) - ref["tsdf"])[ok].max()), _bar(ref32["tsdf"][ok], ref["tsdf"][ok])
    print(f"[tsdf] fused sphere tsdf: max error {err:.2e}, bar {bar:.2e}, {int((weight > 0).sum())} updated points, "
          f"{int(fragile.sum())} left out")
    assert err <= bar
    field = {"tsdf": tsdf, "weight": weight, "color": None, "origin": R.FUSE_ORIGIN, "voxel_size": R.FUSE_VOXEL,
             "sdf_trunc": R.FUSE_TRUNC}
    census = R.mesh_census(field, 1.0)
    v, f = _check_mesh("fused sphere", field, vol, 1.0, R.extract(field, 1.0), R.extract(field, 1.0, np.float32), census)
    e = census["ends"]
    solid = (weight[e[:, :, 2], e[:, :, 1], e[:, :, 0]] >= 2).all(axis=1)
    off = np.abs(np.linalg.norm(v - np.array(R.FUSE_C), axis=1) - R.FUSE_R) / R.FUSE_VOXEL
    across = int(((e[:, 0, 0] == 63) & (e[:, 1, 0] == 64)).sum())
    print(f"[tsdf] fused sphere: {int(solid.sum())} vertices between samples of weight >= 2, at most {off[solid].max():.3f} "
          f"voxels off the sphere; {across} vertices across the seam")
    assert solid.sum() > 1000 and off[solid].max() < 1.0 and across >= 50
