"""CPU-side checks of the TSDF fusion and mesh extraction (csrc/tsdf.hip; tsdf.py): the restatement the
GPU tests compare against (tests/tsdf_restate.py) held to properties no oracle is needed for, the share of
threshold-fragile points in the shared integration inputs, the refusals -- which all come before a GPU is asked for --
the ABI, and the mesh PLY writer."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import tsdf_restate as R


@pytest.fixture(scope="module")
def sphere_mesh():
    return R.extract(R.sphere_field())


def test_restated_sphere_is_closed_consistently_oriented_and_has_euler_characteristic_two(sphere_mesh):
    """Validates the hand-derived case rule: every undirected edge in exactly two faces, once per direction; V - E + F =
    2; positive signed volume (normals from inside to outside)."""
    vertices, faces, colors = sphere_mesh
    assert len(faces) > 5000 and colors.shape == vertices.shape
    R.assert_closed_oriented_sphere(vertices, faces)
    # close to the volume of the ball: a gross orientation or placement error would show
    assert abs(R.signed_volume(vertices, faces) / (4.0 / 3.0 * math.pi * R.SPHERE_R ** 3) - 1.0) < 0.02


def test_restated_sphere_vertices_lie_within_the_curvature_bound_of_linear_interpolation(sphere_mesh):
    vertices, _, _ = sphere_mesh
    L = math.sqrt(3.0)                                                   # the longest edge, voxel_size = 1
    off = np.abs(np.linalg.norm(vertices - np.array(R.SPHERE_C), axis=1) - R.SPHERE_R)
    print(f"largest distance to the sphere {off.max():.4f}, bound {L * L / (8 * (R.SPHERE_R - L)):.4f}")
    assert off.max() <= L * L / (8.0 * (R.SPHERE_R - L))
    nx, ny, nz = R.SPHERE_DIMS
    assert vertices.min() > 1.0 and np.all(vertices.max(axis=0) < np.array([nx, ny, nz]) - 2.0), "surface at the border"


def test_kuhn_tetrahedra_tile_the_cube_and_agree_across_cube_faces():
    tets = R.kuhn_tetrahedra()
    assert len(tets) == 6 and all(t[0] == (0, 0, 0) and t[3] == (1, 1, 1) for t in tets)
    vol = [np.linalg.det(np.array([np.subtract(t[n], t[0]) for n in (1, 2, 3)], dtype=np.float64)) / 6 for t in tets]
    assert all(v > 0 for v in vol) and abs(sum(vol) - 1.0) < 1e-12
    # translation invariance: the diagonal a cube draws on its x = 1 face is the one its neighbour draws on x = 0
    for axis in range(3):
        def face_edges(side):
            out = set()
            for t in tets:
                on = [p for p in t if p[axis] == side]
                out |= {tuple(sorted((tuple(np.delete(a, axis)), tuple(np.delete(b, axis)))))
                        for a in on for b in on if a != b}
            return out
        assert face_edges(0) == face_edges(1)


def test_fragile_share_of_the_integration_inputs_is_below_one_percent():
    """The band is 2e-4 pixels wide per axis: about 4e-4 of the points are expected inside it."""
    _, views = R.integration_case()
    _, touched, fragile = R.run_case(views, with_color=True)
    share = float((touched & fragile).sum()) / float(touched.sum())
    print(f"{int(touched.sum())} of {touched.size} points updated by some view, fragile share {share:.2e}")
    assert touched.sum() > 500 and (~touched).sum() > 500, "the case must both update and leave out many points"
    assert share <= 0.01


def test_missing_max_depth_is_no_limit():
    from mvs_gaussian_splatting_amd import tsdf
    assert tsdf._limit(None, "max_depth") == math.inf and tsdf._limit(2.5, "max_depth") == 2.5
    with pytest.raises(ValueError):
        tsdf._limit(0.0, "max_depth")
    _, views = R.integration_case()
    free = [dict(v, max_depth=None) for v in views]
    huge = [dict(v, max_depth=1e30) for v in views]
    a, ta, _ = R.run_case(free, True)
    b, tb, _ = R.run_case(huge, True)
    c, tc, _ = R.run_case(views, True)
    assert np.array_equal(ta, tb) and all(np.array_equal(a[k], b[k]) for k in ("tsdf", "weight", "color"))
    assert ta.sum() > tc.sum(), "the case's max_depth must cut something"


class _Cam:
    image_width, image_height = 37, 29
    FoVx = FoVy = 1.0
    world_view_transform = torch.eye(4)


def test_every_refusal_is_a_value_error_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import TSDFVolume, _lib
    make = lambda **kw: TSDFVolume(**{**dict(origin=(0, 0, 0), voxel_size=0.1, dims=(5, 4, 3), sdf_trunc=0.4,    # noqa: E731
                                             device="cpu"), **kw})
    for dims in ((0, 4, 3), (5, -1, 3), (5, 4, 0)):
        with pytest.raises(ValueError):
            make(dims=dims)
    with pytest.raises(ValueError):
        make(dims=(1024, 1024, 293), device="cuda")          # 7 * N >= 2^31: refused before any allocation
    assert 7 * 1024 * 1024 * 292 < 2 ** 31 <= 7 * 1024 * 1024 * 293
    for kw in ({"voxel_size": 0.0}, {"voxel_size": -1.0}, {"sdf_trunc": 0.0}, {"sdf_trunc": -0.5},
               {"voxel_size": float("nan")}):
        with pytest.raises(ValueError):
            make(**kw)
    vol = make()
    assert tuple(vol.tsdf.shape) == (3, 4, 5) and tuple(vol.color.shape) == (3, 4, 5, 3)
    assert bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all()) and bool((vol.color == 0).all())
    assert make(with_color=False).color is None
    good_d, good_c = torch.ones(29, 37), torch.zeros(3, 29, 37)
    bad_depths = (torch.ones(29, 37, dtype=torch.float64), torch.ones(37, 29), torch.ones(2, 29, 37),
                  torch.ones(29, 37).numpy(), torch.ones(29, 37, device="meta"))
    for d in bad_depths:
        with pytest.raises(ValueError):
            vol.integrate(d, _Cam, color=good_c)
    for c in (torch.zeros(3, 29, 36), torch.zeros(29, 37, 3), torch.zeros(3, 29, 37, dtype=torch.float16), None):
        with pytest.raises(ValueError):
            vol.integrate(good_d, _Cam, color=c)
    with pytest.raises(ValueError):
        make(with_color=False).integrate(good_d, _Cam, color=good_c)
    for kw in ({"weight": 0.0}, {"max_depth": -1.0}, {"max_weight": 0.0}):
        with pytest.raises(ValueError):
            vol.integrate(good_d, _Cam, color=good_c, **kw)
    # well-formed arguments on a CPU volume: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError):
        vol.integrate(good_d.unsqueeze(0), _Cam, color=good_c)
    with pytest.raises(_lib.GsrError):
        vol.extract_mesh()
    vol.tsdf = vol.tsdf.double()
    with pytest.raises(ValueError):
        vol.extract_mesh()


def test_volume_for_points_bounds_the_bulk_of_the_points():
    from mvs_gaussian_splatting_amd import volume_for_points
    g = torch.Generator().manual_seed(3)
    xyz = torch.randn(5000, 3, generator=g) * torch.tensor([2.0, 1.0, 0.5])
    xyz[0] = torch.tensor([500.0, 0.0, 0.0])                              # an outlier must not blow the box up
    vol = volume_for_points(xyz, resolution=64, device="cpu")
    assert max(vol.dims) == 64 and vol.dims[0] > vol.dims[1] > vol.dims[2] >= 2
    assert vol.sdf_trunc == pytest.approx(4 * vol.voxel_size)
    hi = [o + vol.voxel_size * (n - 1) for o, n in zip(vol.origin, vol.dims)]
    inside = ((xyz > torch.tensor(vol.origin)) & (xyz < torch.tensor(hi))).all(dim=1).float().mean()
    assert 0.93 < float(inside) < 1.0 and hi[0] < 20
    by_size = volume_for_points(xyz, voxel_size=0.25, device="cpu")
    assert by_size.voxel_size == 0.25 and by_size.dims[0] > by_size.dims[1]
    with pytest.raises(ValueError):
        volume_for_points(xyz, voxel_size=0.25, resolution=64)


def test_library_exports_the_tsdf_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_tsdf_integrate", "gsr_tsdf_mesh_count", "gsr_tsdf_mesh_emit"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 27
    # argument checks run before any HIP call
    one = (C.c_float * 64)()
    ptr = C.addressof(one)
    vol = _lib.GsrTsdfVolume()
    view = _lib.GsrTsdfView()
    assert lib.gsr_tsdf_integrate(None, C.byref(view), None) == -1
    vol.nx, vol.ny, vol.nz, vol.voxel_size, vol.sdf_trunc = 2, 2, 2, 1.0, 1.0
    vol.tsdf, vol.weight = ptr, ptr
    view.width, view.height, view.fx, view.fy, view.weight = 4, 4, 1.0, 1.0, 1.0
    view.max_depth = view.max_weight = math.inf
    assert lib.gsr_tsdf_integrate(C.byref(vol), None, None) == -1
    assert lib.gsr_tsdf_integrate(C.byref(vol), C.byref(view), None) == -1            # NULL viewmatrix / depth
    view.viewmatrix, view.depth = ptr, ptr
    for field, bad in (("nx", 0), ("voxel_size", 0.0), ("sdf_trunc", -1.0)):
        keep = getattr(vol, field)
        setattr(vol, field, bad)
        assert lib.gsr_tsdf_integrate(C.byref(vol), C.byref(view), None) == -1, field
        setattr(vol, field, keep)
    for field, bad in (("width", 0), ("fx", 0.0), ("weight", 0.0), ("max_depth", 0.0), ("max_weight", float("nan"))):
        keep = getattr(view, field)
        setattr(view, field, bad)
        assert lib.gsr_tsdf_integrate(C.byref(vol), C.byref(view), None) == -1, field
        setattr(view, field, keep)
    view.color = ptr                                                                 # colour image without a colour field
    assert lib.gsr_tsdf_integrate(C.byref(vol), C.byref(view), None) == -1
    vol.tsdf = ptr + 1
    assert lib.gsr_tsdf_integrate(C.byref(vol), C.byref(view), None) == -3
    vol.tsdf = ptr
    vol.nx, vol.ny, vol.nz = 1024, 1024, 293                                         # 7 N >= 2^31: never wrap
    assert lib.gsr_tsdf_mesh_count(C.byref(vol), 0.0, ptr, ptr, ptr, None) == -1
    vol.nx, vol.ny, vol.nz = 2, 2, 2
    assert lib.gsr_tsdf_mesh_count(C.byref(vol), 0.0, None, ptr, ptr, None) == -1
    assert lib.gsr_tsdf_mesh_count(C.byref(vol), float("nan"), ptr, ptr, ptr, None) == -1
    assert lib.gsr_tsdf_mesh_emit(C.byref(vol), ptr, ptr, ptr, ptr, 0, 1, ptr, None, ptr, None) == -1
    assert lib.gsr_tsdf_mesh_emit(C.byref(vol), ptr, ptr, ptr, ptr, 57, 1, ptr, None, ptr, None) == -1    # V > 7 N
    assert lib.gsr_tsdf_mesh_emit(C.byref(vol), ptr, ptr, ptr, ptr, 1, 1, ptr, ptr, ptr, None) == -1      # colours, no field
    assert lib.gsr_tsdf_mesh_emit(C.byref(vol), ptr, ptr, ptr + 4, ptr, 1, 1, ptr, None, ptr, None) == -3


# ---- PLY ---------------------------------------------------------------------------------------------------------------
def _read_ply_mesh(path):
    """A reader of this test's own for the files write_ply_mesh writes."""
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, cur = {}, {}, None
    for line in lines[2:]:
        tok = line.split()
        if tok and tok[0] == "element":
            cur = tok[1]
            counts[cur], props[cur] = int(tok[2]), []
        elif tok and tok[0] == "property":
            props[cur].append(tok[1:])
    assert list(counts) == ["vertex", "face"] and props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    vdt = np.dtype([(p[1], {"float": "<f4", "uchar": "u1"}[p[0]]) for p in props["vertex"]])
    vert = np.frombuffer(body, dtype=vdt, count=counts["vertex"])
    fdt = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
    face = np.frombuffer(body, dtype=fdt, count=counts["face"], offset=vert.nbytes)
    assert vert.nbytes + face.nbytes == len(body) and np.all(face["n"] == 3)
    xyz = np.stack([vert[k] for k in "xyz"], axis=1) if counts["vertex"] else np.zeros((0, 3), np.float32)
    rgb = None
    if "red" in vdt.names:
        rgb = np.stack([vert[k] for k in ("red", "green", "blue")], axis=1) if counts["vertex"] else np.zeros((0, 3), np.uint8)
    return xyz, face["idx"].reshape(-1, 3), rgb


def test_write_ply_mesh_round_trips_with_colours_without_and_empty(tmp_path, sphere_mesh):
    from mvs_gaussian_splatting_amd.ply_io import write_ply_mesh
    vertices, faces, colors = sphere_mesh
    v32 = vertices.astype(np.float32)
    p = str(tmp_path / "a" / "mesh.ply")
    write_ply_mesh(p, torch.from_numpy(v32), torch.from_numpy(faces.astype(np.int32)), torch.from_numpy(colors))
    xyz, idx, rgb = _read_ply_mesh(p)
    assert np.array_equal(xyz, v32) and np.array_equal(idx, faces)
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, np.floor(np.clip(colors, 0, 1) * 255 + 0.5).astype(np.uint8))
    p = str(tmp_path / "plain.ply")
    write_ply_mesh(p, v32, faces)
    xyz, idx, rgb = _read_ply_mesh(p)
    assert np.array_equal(xyz, v32) and np.array_equal(idx, faces) and rgb is None
    for col in (None, torch.zeros(0, 3)):
        p = str(tmp_path / "empty.ply")
        write_ply_mesh(p, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), col)
        xyz, idx, rgb = _read_ply_mesh(p)
        assert xyz.shape == (0, 3) and idx.shape == (0, 3) and (rgb is None) == (col is None)
    with pytest.raises(ValueError):
        write_ply_mesh(p, v32[:10], faces)


# ---- census of the inputs past one x-chunk (tests/test_gpu_tsdf.py runs them on the GPU) ---------------------------------
# Conditions of the inputs, from the float64 restatement alone: they keep the inputs from decaying into ones that leave the
# kernels' branches unexercised.
@pytest.mark.parametrize("n", range(len(R.WIDE_DIMS)))
def test_wide_integration_inputs_reach_every_test_of_the_kernel(n):
    case = R.wide_case(n)
    nx, ny, nz = case["dims"]
    assert nx > 64 and [(65, 1), (130, 2), (128, 0)][n] == (nx, nx % 64) and ((ny * nz) % 4 != 0 or n != 1)
    assert [v["weight"] for v in case["views"]] == [0.5, 2.25, 1.0]
    assert all(v["W"] % 2 == 1 and v["H"] % 2 == 1 and v["W"] % 16 and v["H"] % 16 for v in case["views"])
    for v in case["views"]:                                  # every rotation mixes all three axes
        assert np.abs(v["viewmatrix"][:3, :3]).max() < 0.999
    vol, touched, fragile, per_view = R.run_wide(case, with_color=True)
    robust = ~fragile
    best = {}
    for v, view in enumerate(case["views"]):
        classes = R.view_classes(R.wide_volume(case, True, False), view)
        assert np.array_equal(classes["updated"][robust], per_view[v][robust]), "the census disagrees with integrate()"
        for name, mask in classes.items():
            best[name] = max(best.get(name, 0), int((mask & robust).sum()))
        if v == 1:
            assert view["max_depth"] is None and int((classes["inf_update"] & robust).sum()) >= 1
            assert int((classes["behind"] & robust).sum()) >= 100, "the inside camera has much of the grid behind it"
        if v == 2:                                           # the small image: all four sides, negative u + 0.5 and v + 0.5 too
            assert all(int((classes[k] & robust).sum()) >= 20 for k in ("off_left", "off_right", "off_top", "off_bottom"))
    print(f"wide case {n} {case['dims']}: " + ", ".join(f"{k} {best[k]}" for k in best))
    for name in R.CLASSES:
        assert best[name] >= 20, f"{name}: only {best[name]} robust points in the best view"
    # a side's test is only visible where the other coordinate is inside the image
    for name in ("only_left", "only_right", "only_top", "only_bottom"):
        assert best[name] >= 20, f"{name}: only {best[name]} robust points in the best view"
    # and only where a test that is off by one pixel would turn the point into an update: the pixel it would read is a
    # valid depth inside the band.  A handful suffices: each is a written point that must keep its bits.
    for name in ("relaxed_left", "relaxed_right", "relaxed_top", "relaxed_bottom"):
        assert best[name] >= 5, f"{name}: only {best[name]} robust points would be updated"
    assert "guard" in case["views"][0] and "guard" not in case["views"][2]
    if n == 1:                                               # sdf_trunc > 0.2: a 0 depth is stopped by d > 0 alone
        assert case["sdf_trunc"] > 0.2 and best["zero_visible"] >= 5, f"zero_visible {best['zero_visible']}"
    share = float(fragile.sum()) / fragile.size
    assert share < 0.01, f"fragile share {share:.3f}"
    assert touched.sum() > 200 and (~touched).sum() > 200
    assert len(np.unique(vol["weight"])) >= 6, "the views must overlap in different combinations"
    clamped, _, _, _ = R.run_wide(case, True, max_weight=R.WIDE_MAX_WEIGHT)
    assert int(((clamped["weight"] == R.WIDE_MAX_WEIGHT) & robust).sum()) > 20
    assert clamped["weight"].max() == R.WIDE_MAX_WEIGHT < vol["weight"].max()
    # the pre-loaded state: w_old differs from point to point, and some pre-loaded weights exceed the clamp
    pre = case["preload"]
    assert set(np.unique(pre["weight"]).tolist()) == {0.0, 0.5, 4.0} and pre["tsdf"].min() < -0.9 and pre["tsdf"].max() > 0.9
    loaded, up, _, _ = R.run_wide(case, True, max_weight=R.WIDE_MAX_WEIGHT, preload=True)
    assert np.array_equal(up, touched), "which points a view updates does not depend on the state"
    assert all(np.array_equal(loaded[k][~up], pre[k][~up].astype(np.float64)) for k in ("tsdf", "weight", "color"))
    # the float32 restatement takes every decision as float64 does on the robust points: the margin is wide enough
    _, _, _, per_view32 = R.run_wide(case, True, dtype=np.float32)
    assert all(np.array_equal(a[robust], b[robust]) for a, b in zip(per_view, per_view32))


def test_existing_integration_inputs_never_leave_the_frustum():
    """Why the wide inputs exist: in ``integration_case`` no point is behind a camera or outside an image."""
    _, views = R.integration_case()
    vol = R.empty_volume(R.CASE_DIMS, R.CASE_ORIGIN, R.CASE_VOXEL, R.CASE_TRUNC, True)
    for view in views:
        classes = R.view_classes(vol, view)
        assert not any(classes[k].any() for k in ("near", "behind", "off_left", "off_right", "off_top", "off_bottom"))


@pytest.fixture(scope="module")
def random_censuses():
    return [R.mesh_census(R.random_field(n)) for n in range(len(R.RANDOM_DIMS))]


def _end_values(field, census):
    e = census["ends"]
    return field["tsdf"][e[:, :, 2], e[:, :, 1], e[:, :, 0]]


def test_random_fields_reach_the_cube_patterns_cases_polarities_and_hole_borders(random_censuses):
    union = lambda key: set().union(*(c[key] for c in random_censuses))                     # noqa: E731
    patterns, tet_cases, polarities = union("patterns"), union("tet_cases"), union("polarities")
    orphans, shared = sum(c["orphans"] for c in random_censuses), sum(c["shared"] for c in random_censuses)
    print(f"{len(patterns)} of 254 mixed cube patterns, {len(tet_cases)} of 84 (tetrahedron, case) pairs, "
          f"{len(polarities)} of 14 (direction, polarity) pairs, {orphans} crossed edges without a processed cube, "
          f"{shared} held by a processed and an unprocessed cube")
    assert len(patterns) >= 250 and 0 not in patterns and 255 not in patterns
    assert tet_cases == {(t, m) for t in range(6) for m in range(1, 15)}
    assert polarities == {(d, s) for d in range(7) for s in (False, True)}
    assert orphans >= 10 and shared >= 10
    plus = minus = 0
    for n, census in enumerate(random_censuses):
        field = R.random_field(n)
        nx, ny, nz = R.RANDOM_DIMS[n]
        assert nx > 64 and tuple(field["tsdf"].shape) == (nz, ny, nx)
        share = float((field["weight"] == 0).mean())
        assert 0.01 < share < 0.06 and set(np.unique(field["weight"]).tolist()) == {0.0, 1.0, 2.0, 3.0}
        vals = _end_values(field, census)
        plus += int(((vals == 0) & ~np.signbit(vals)).sum())
        minus += int(((vals == 0) & np.signbit(vals)).sum())
        # the census, found edge by edge, names the vertices extract() finds triangle by triangle
        vertices, faces, _ = R.extract(field)
        assert len(census["keys"]) == len(vertices) and len(faces) > 4000
        e = census["ends"]
        # the smallest cross-section has 15 points, each with four edges that advance in x, about half of them crossed
        assert int(((e[:, 0, 0] == 63) & (e[:, 1, 0] == 64)).sum()) >= 10, "vertices on edges across the chunk seam"
    assert plus >= 1 and minus >= 1, "an emitted edge ends at 0.0, another at -0.0"


def test_min_weight_variants_change_which_cubes_are_processed():
    field = R.random_field(1)
    sizes = {mw: len(R.extract(field, min_weight=mw)[1]) for mw in (0.0, 1e-6, 2.0, float("inf"))}
    print(f"faces by min_weight: {sizes}")
    assert sizes[0.0] > sizes[1e-6] > sizes[2.0] > 100 and sizes[float("inf")] == 0
    empty = R.extract(field, min_weight=float("inf"))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0, 3)


def test_seam_sphere_is_closed_and_crosses_the_chunk_seam():
    field = R.seam_sphere_field()
    vertices, faces, _ = R.extract(field)
    R.assert_closed_oriented_sphere(vertices, faces)
    assert abs(R.signed_volume(vertices, faces) / (4.0 / 3.0 * math.pi * R.SEAM_R ** 3) - 1.0) < 0.02
    census = R.mesh_census(field)
    e = census["ends"]
    across = int(((e[:, 0, 0] == 63) & (e[:, 1, 0] == 64)).sum())
    print(f"seam sphere: V {len(vertices)} F {len(faces)}, {across} vertices on edges from i = 63 to i = 64")
    assert len(census["keys"]) == len(vertices) and across >= 50
    assert vertices[:, 0].min() < 63 < 64 < vertices[:, 0].max()


def test_fused_sphere_lies_within_a_voxel_of_the_analytic_one_where_two_views_agree():
    _, views = R.fusion_case()
    vol, fragile = R.run_fusion(views)
    assert fragile.mean() < 0.01 and R.FUSE_DIMS[0] > 64
    vertices, faces, _ = R.extract(vol, min_weight=1.0)
    census = R.mesh_census(vol, 1.0)
    e = census["ends"]
    solid = (vol["weight"][e[:, :, 2], e[:, :, 1], e[:, :, 0]] >= 2).all(axis=1)
    off = np.abs(np.linalg.norm(vertices - np.array(R.FUSE_C), axis=1) - R.FUSE_R) / R.FUSE_VOXEL
    across = int(((e[:, 0, 0] == 63) & (e[:, 1, 0] == 64)).sum())
    print(f"fused sphere: V {len(vertices)} F {len(faces)}, {int(solid.sum())} vertices between samples of weight >= 2, "
          f"at most {off[solid].max():.3f} voxels off the sphere; {across} vertices across the seam")
    assert solid.sum() > 1000 and off[solid].max() < 1.0 and across >= 50
