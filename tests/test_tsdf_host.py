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
