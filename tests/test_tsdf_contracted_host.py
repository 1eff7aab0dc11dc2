"""CPU-side checks of TSDF fusion in contracted space (csrc/tsdf.hip, ABI v33; tsdf.py): the contraction and
its inverse, ``bounding_sphere``, the box of ``contracted_volume_for_points``, the refusals -- which all come before a GPU
is asked for -- the ABI, the restatement's mesh of a sphere beyond the unit ball, and the share of threshold-fragile
points in the inputs tests/test_gpu_tsdf_contracted.py runs on the GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import tsdf_restate as R
import tsdf_contracted_restate as CR


def test_uncontract_inverts_contract_from_the_centre_to_fifty_radii():
    rng = np.random.default_rng(5)
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    norms = np.concatenate(([0.0, 1.0, 1.0, 50.0], rng.uniform(0.0, 50.0, 1996), rng.uniform(0.0, 1.5, 2000)))
    x = d * norms[:, None]
    x[2] = (0.0, -1.0, 0.0)                                               # |x| = 1 exactly
    q = CR.contract(x)
    assert np.array_equal(q[0], np.zeros(3)) and np.array_equal(q[2], x[2]) and np.linalg.norm(q, axis=1).max() < 2.0
    inner = norms <= 1.0
    assert np.array_equal(q[inner], x[inner]), "the unit ball is kept"
    assert np.allclose(np.linalg.norm(q[~inner], axis=1), 2.0 - 1.0 / norms[~inner], rtol=1e-14)
    back = CR.uncontract(q, (0.0, 0.0, 0.0), 1.0)
    err = np.linalg.norm(back - x, axis=1) / np.maximum(norms, 1.0)
    print(f"largest relative round-trip error {err.max():.2e}")
    assert err.max() <= 1e-12
    center, radius = (0.375, -0.25, 0.5), 1.5
    assert np.allclose(CR.uncontract(q, center, radius), np.array(center) + radius * x, rtol=1e-12, atol=1e-12)
    # the package's torch contraction is the same function
    from mvs_gaussian_splatting_amd.tsdf import contract
    assert np.allclose(contract(torch.from_numpy(x)).numpy(), q, rtol=1e-14, atol=0.0)


class _Pose:
    """A camera as ``bounding_sphere`` reads it: a float64 ``world_view_transform`` in the row-vector convention."""

    def __init__(self, Rc2w, pos):
        M = np.eye(4)
        M[:3, :3], M[3, :3] = Rc2w, -Rc2w.T @ pos                          # p_view = p_world @ Rc2w - pos @ Rc2w
        self.world_view_transform = torch.from_numpy(M)


def _look_at(pos, target):
    fwd = (np.asarray(target, np.float64) - pos) / np.linalg.norm(np.asarray(target, np.float64) - pos)
    right = np.cross(fwd, (0.0, 0.3, 1.0))
    right /= np.linalg.norm(right)
    Rc2w = np.stack((right, np.cross(fwd, right), fwd), axis=1)           # columns: right, down, forward
    return _Pose(Rc2w, np.asarray(pos, np.float64))


def test_bounding_sphere_of_a_ring_of_cameras_is_their_target_and_the_ring_radius():
    from mvs_gaussian_splatting_amd import bounding_sphere
    target, ring = np.array([0.7, -1.3, 2.1]), 4.5
    tilt = R._rotation((1.0, 2.0, 0.5), 25.0)
    cams = [_look_at(target + tilt @ (ring * np.array([math.cos(a), math.sin(a), 0.0])), target)
            for a in np.arange(8) * (2 * math.pi / 8)]
    center, radius = bounding_sphere(cams)
    print(f"center off by {np.abs(np.array(center) - target).max():.2e}, radius off by {abs(radius - ring):.2e}")
    assert isinstance(radius, float) and len(center) == 3
    assert np.abs(np.array(center) - target).max() <= 1e-9 and abs(radius - ring) <= 1e-9
    # one camera nearer than the others: the radius is the smallest distance
    near = _look_at(target + np.array([0.0, 0.0, 2.0]), target)
    c2, r2 = bounding_sphere(cams + [near])
    assert np.abs(np.array(c2) - target).max() <= 1e-9 and abs(r2 - 2.0) <= 1e-9


def test_bounding_sphere_refuses_one_camera_and_parallel_axes():
    from mvs_gaussian_splatting_amd import bounding_sphere
    a = _look_at(np.array([0.0, 0.0, 0.0]), (0.0, 0.0, 5.0))
    b = _look_at(np.array([1.0, 0.5, 0.0]), (1.0, 0.5, 5.0))                # the same direction from another place
    with pytest.raises(ValueError):
        bounding_sphere([a])
    with pytest.raises(ValueError):
        bounding_sphere([])
    with pytest.raises(ValueError, match="parallel"):
        bounding_sphere([a, b])
    with pytest.raises(ValueError, match="parallel"):
        bounding_sphere([a, b, _look_at(np.array([1.0, 0.5, 9.0]), (1.0, 0.5, 5.0))])     # antiparallel: the same axis


def test_contracted_volume_for_points_is_the_hand_computed_box():
    from mvs_gaussian_splatting_amd import ContractedTSDFVolume, contracted_volume_for_points
    center, radius = (0.375, -0.25, 0.5), 1.5
    # 21 points on a ray from the centre at |x| = 0, 0.5, .. 10: contracted norms 0, 0.5, 1, 2 - 1 / |x|
    steps = 0.5 * torch.arange(21, dtype=torch.float32)
    xyz = torch.tensor(center) + radius * steps[:, None] * torch.tensor([0.6, 0.0, -0.8])
    xyz = xyz[torch.randperm(21, generator=torch.Generator().manual_seed(1))]
    vol = contracted_volume_for_points(xyz, center, radius, resolution=17, quantile=0.5, device="cpu")
    R_box = (2.0 - 1.0 / 5.0) + 0.01                                       # the median is the point at |x| = 5
    assert isinstance(vol, ContractedTSDFVolume) and vol.dims == (17, 17, 17)
    assert vol.origin == pytest.approx((-R_box,) * 3, rel=1e-6) and vol.voxel_size == pytest.approx(2 * R_box / 16, rel=1e-6)
    assert vol.sdf_trunc == pytest.approx(5 * radius * vol.voxel_size) and vol.q_max == 1.9
    assert vol.center == center and vol.radius == radius and vol.with_color
    between = contracted_volume_for_points(xyz, center, radius, resolution=9, quantile=0.525, sdf_trunc=0.25,
                                           with_color=False, device="cpu")
    R_mid = 0.5 * ((2.0 - 1.0 / 5.0) + (2.0 - 1.0 / 5.5)) + 0.01           # half way between the neighbours
    assert between.origin[0] == pytest.approx(-R_mid, rel=1e-6) and between.sdf_trunc == 0.25 and between.color is None
    capped = contracted_volume_for_points(xyz, center, radius, resolution=5, device="cpu")       # 0.95: |x| = 9.5
    assert capped.origin == (-1.9, -1.9, -1.9) and capped.voxel_size == pytest.approx(3.8 / 4)
    with pytest.raises(ValueError, match="overflows the 32-bit index space"):
        contracted_volume_for_points(xyz, center, radius, resolution=700, device="cuda")
    assert 7 * 512 ** 3 < 2 ** 31 <= 7 * 700 ** 3
    for kw in ({"resolution": 1}, {"quantile": 1.5}):
        with pytest.raises(ValueError):
            contracted_volume_for_points(xyz, center, radius, device="cpu", **kw)
    with pytest.raises(ValueError):
        contracted_volume_for_points(xyz[:, :2], center, radius, device="cpu")


class _Cam:
    image_width, image_height = 37, 29
    FoVx = FoVy = 1.0
    world_view_transform = torch.eye(4)


def test_every_new_refusal_is_a_value_error_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import ContractedTSDFVolume, TSDFVolume, _lib, contracted_volume_for_points
    make = lambda **kw: ContractedTSDFVolume(**{**dict(origin=(-1.9,) * 3, voxel_size=0.95, dims=(5, 5, 5),     # noqa: E731
                                                       sdf_trunc=0.4, center=(0, 0, 0), radius=2.0, device="cuda"), **kw})
    bad = ({"radius": 0.0}, {"radius": -1.0}, {"radius": float("inf")}, {"radius": float("nan")}, {"q_max": 1.0},
           {"q_max": 2.0}, {"q_max": 0.5}, {"q_max": float("nan")}, {"center": (0.0, 0.0)}, {"center": (0.0, float("nan"), 0.0)},
           {"center": (float("inf"), 0.0, 0.0)})
    for kw in bad:                                                         # device="cuda": refused before any allocation
        with pytest.raises(ValueError):
            make(**kw)
    for kw in ({"radius": 0.0}, {"q_max": 2.5}, {"center": (0.0, float("nan"), 0.0)}):
        with pytest.raises(ValueError):
            contracted_volume_for_points(torch.zeros(4, 3), **{**dict(center=(0, 0, 0), radius=1.0, device="cuda"), **kw})
    with pytest.raises(ValueError):
        make(dims=(0, 5, 5))                                               # the base's refusals still hold
    vol = make(device="cpu", q_max=1.5)
    assert isinstance(vol, TSDFVolume) and (vol.center, vol.radius, vol.q_max) == ((0.0, 0.0, 0.0), 2.0, 1.5)
    assert make(device="cpu").q_max == 1.9
    assert tuple(vol.tsdf.shape) == (5, 5, 5) and bool((vol.tsdf == 1).all()) and bool((vol.weight == 0).all())
    good_d, good_c = torch.ones(29, 37), torch.zeros(3, 29, 37)
    for d in (torch.ones(29, 37, dtype=torch.float64), torch.ones(37, 29)):       # the base's validation
        with pytest.raises(ValueError):
            vol.integrate(d, _Cam, color=good_c)
    with pytest.raises(ValueError):
        vol.integrate(good_d, _Cam, color=None)
    with pytest.raises(ValueError):
        vol.integrate(good_d, _Cam, color=good_c, weight=0.0)
    # well-formed arguments on a CPU volume: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError):
        vol.integrate(good_d, _Cam, color=good_c)
    with pytest.raises(_lib.GsrError):
        vol.extract_mesh()
    with pytest.raises(_lib.GsrError):
        vol.extract_mesh(contracted=True)


def test_library_exports_the_contracted_entry_points_and_the_three_abi_versions_agree():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ("gsr_tsdf_integrate_contracted", "gsr_tsdf_uncontract_points"):
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and name in header
    assert "GsrTsdfContraction" in header and C.sizeof(_lib.GsrTsdfContraction) == 20
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 33
    # argument checks run before any HIP call
    one = (C.c_float * 64)()
    ptr = C.addressof(one)
    vol, view, con = _lib.GsrTsdfVolume(), _lib.GsrTsdfView(), _lib.GsrTsdfContraction()
    vol.nx, vol.ny, vol.nz, vol.voxel_size, vol.sdf_trunc = 2, 2, 2, 1.0, 1.0
    vol.tsdf, vol.weight = ptr, ptr
    view.width, view.height, view.fx, view.fy, view.weight = 4, 4, 1.0, 1.0, 1.0
    view.max_depth = view.max_weight = math.inf
    view.viewmatrix, view.depth = ptr, ptr
    con.radius, con.q_max = 1.0, 1.9
    call = lambda: lib.gsr_tsdf_integrate_contracted(C.byref(vol), C.byref(con), C.byref(view), None)      # noqa: E731
    assert lib.gsr_tsdf_integrate_contracted(None, C.byref(con), C.byref(view), None) == -1
    assert lib.gsr_tsdf_integrate_contracted(C.byref(vol), None, C.byref(view), None) == -1
    assert lib.gsr_tsdf_integrate_contracted(C.byref(vol), C.byref(con), None, None) == -1
    for field, values in (("radius", (0.0, -1.0, math.inf, math.nan)), ("q_max", (1.0, 2.0, 0.5, 2.5, math.nan))):
        keep = getattr(con, field)
        for bad in values:
            setattr(con, field, bad)
            assert call() == -1, (field, bad)
            assert lib.gsr_tsdf_uncontract_points(ptr, 1, C.byref(con), None) == -1, (field, bad)
            assert lib.gsr_tsdf_uncontract_points(None, 0, C.byref(con), None) == -1, "n = 0 still checks the contraction"
        setattr(con, field, keep)
    con.center[1] = math.nan
    assert call() == -1 and b"center" in lib.gsr_last_error()
    con.center[1] = 0.0
    for obj, field, bad in ((vol, "nx", 0), (vol, "sdf_trunc", 0.0), (view, "width", 0), (view, "weight", 0.0),
                            (view, "max_weight", math.nan)):              # what gsr_tsdf_integrate checks
        keep = getattr(obj, field)
        setattr(obj, field, bad)
        assert call() == -1, field
        setattr(obj, field, keep)
    view.color = ptr                                                       # colour image without a colour field
    assert call() == -1
    view.color = None
    vol.tsdf = ptr + 1
    assert call() == -3
    vol.tsdf = ptr
    assert lib.gsr_tsdf_uncontract_points(None, 0, C.byref(con), None) == 0           # a successful no-op
    assert lib.gsr_tsdf_uncontract_points(ptr, 0, C.byref(con), None) == 0
    assert lib.gsr_tsdf_uncontract_points(None, 1, C.byref(con), None) == -1
    assert lib.gsr_tsdf_uncontract_points(ptr, -1, C.byref(con), None) == -1
    assert lib.gsr_tsdf_uncontract_points(ptr, 2 ** 31, C.byref(con), None) == -1
    assert lib.gsr_tsdf_uncontract_points(ptr, 1, None, None) == -1
    assert lib.gsr_tsdf_uncontract_points(ptr + 2, 1, C.byref(con), None) == -3


def test_restated_sphere_beyond_the_unit_ball_is_closed_oriented_and_within_a_cube_diagonal():
    """33^3 samples of [-1.9, 1.9]^3, the sphere |x| = 3 (|q| = 5/3): extracted on the grid and uncontracted, the mesh
    is closed, consistently oriented and of Euler characteristic 2, and every vertex lies within the world-space diagonal
    of the contracted cube based at its owner -- the largest distance between two of its eight uncontracted corners --
    of the sphere."""
    field = CR.shell_sphere_field()
    m = np.sqrt(CR.squared_norm(CR.grid_points((CR.SHELL_RES,) * 3, field["origin"], field["voxel_size"])))
    assert np.array_equal(field["weight"] == 1, m < CR.SHELL_Q_MAX) and (field["weight"] == 0).sum() > 5000
    assert (m >= 2).sum() > 1000, "box corners lie beyond the contraction's range"
    grid_v, faces, _ = CR.extract(field, contracted=True)
    vertices, faces2, _ = CR.extract(field)
    assert np.array_equal(faces, faces2) and len(faces) > 5000
    R.assert_closed_oriented_sphere(grid_v, faces)
    R.assert_closed_oriented_sphere(vertices, faces)
    assert np.linalg.norm(grid_v, axis=1).max() < CR.SHELL_Q_MAX
    volume = R.signed_volume(vertices - np.array(CR.SHELL_CENTER), faces)
    assert abs(volume / (4.0 / 3.0 * math.pi * CR.SHELL_SPHERE ** 3) - 1.0) < 0.05
    census = R.mesh_census(field)
    base = census["ends"][:, 0, :]                                          # the owner: every owned edge lies in its cube
    assert len(base) == len(vertices) and base.max() < CR.SHELL_RES - 1
    corners = np.stack([base + np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1]) for c in range(8)], axis=1)     # [V,8,3]
    q = np.array(field["origin"]) + field["voxel_size"] * corners
    assert np.linalg.norm(q, axis=-1).max() < 2.0
    p = CR.uncontract(q, CR.SHELL_CENTER, CR.SHELL_RADIUS)
    diagonal = np.linalg.norm(p[:, :, None, :] - p[:, None, :, :], axis=-1).max(axis=(1, 2))
    off = np.abs(np.linalg.norm(vertices - np.array(CR.SHELL_CENTER), axis=1) - CR.SHELL_SPHERE)
    print(f"V {len(vertices)} F {len(faces)}; largest distance to the sphere {off.max():.3f} world units, "
          f"{(off / diagonal).max():.3f} of the cube's diagonal (diagonals {diagonal.min():.2f} .. {diagonal.max():.2f})")
    assert np.all(off <= diagonal)


def test_fragile_share_of_the_contracted_integration_inputs_is_below_one_percent():
    """The cap of tests/test_tsdf_host.py, on the inputs of tests/test_gpu_tsdf_contracted.py; and what those inputs
    must hold: q = 0, |q| = 1, both sides of q_max, corners beyond 2, points behind a camera and outside an image."""
    nx, ny, nz = CR.CASE_DIMS
    assert (nx, ny, nz) == (70, 9, 6) and nx % 64 != 0
    m = np.sqrt(CR.squared_norm(CR.grid_points(CR.CASE_DIMS, CR.CASE_ORIGIN, CR.CASE_VOXEL)))
    assert (m == 0).sum() == 1 and (m == 1).sum() >= 1 and (m == CR.CASE_Q_MAX).sum() >= 1
    assert ((m > 1) & (m < CR.CASE_Q_MAX)).sum() > 500 and (m >= CR.CASE_Q_MAX).sum() > 200
    assert all(m[k, j, i] > 2 for k in (0, nz - 1) for j in (0, ny - 1) for i in (0, nx - 1)) and (m == 2).sum() >= 1
    assert any(c != 0 for c in CR.CASE_CENTER) and CR.CASE_RADIUS != 1
    _, views = CR.integration_case()
    assert all(v["W"] == 48 and v["H"] == 40 and (v["depth"] == 0).sum() > 50 and (v["depth"] > v["max_depth"]).sum() > 10
               for v in views)
    assert [v["weight"] for v in views] == [0.5, 2.25]
    vol, touched, fragile = CR.run_case(views, with_color=True)
    share_touched = float((touched & fragile).sum()) / float(touched.sum())
    share = float(fragile.sum()) / fragile.size
    print(f"{int(touched.sum())} of {touched.size} points updated, fragile share {share:.2e} of all, {share_touched:.2e} of "
          f"the updated; weights {np.unique(vol['weight'], return_counts=True)}")
    assert share <= 0.01 and share_touched <= 0.01
    assert touched.sum() > 500 and (~touched & (m < CR.CASE_Q_MAX)).sum() > 100
    assert not touched[m >= CR.CASE_Q_MAX].any()
    assert (touched & (m > 1.5)).sum() > 200, "the shell is updated too"
    assert len(np.unique(vol["weight"])) == 4, "untouched, either view, both"
    clamped, _, _ = CR.run_case(views, True, max_weight=CR.CASE_MAX_WEIGHT)
    assert int(((clamped["weight"] == CR.CASE_MAX_WEIGHT) & ~fragile).sum()) > 50 and vol["weight"].max() > CR.CASE_MAX_WEIGHT
    # points behind a camera and outside an image, inside q_max
    inside = m < CR.CASE_Q_MAX
    q = CR.grid_points(CR.CASE_DIMS, CR.CASE_ORIGIN, CR.CASE_VOXEL)
    p = CR.uncontract(np.where(inside[..., None], q, 0.0), CR.CASE_CENTER, CR.CASE_RADIUS)
    behind = off = 0
    for v in views:
        M = v["viewmatrix"]
        x, y, z = (p @ M[:3, c] + M[3, c] for c in range(3))
        with np.errstate(all="ignore"):
            px, py = np.floor(v["fx"] * x / z + (v["W"] - 1) / 2 + 0.5), np.floor(v["fy"] * y / z + (v["H"] - 1) / 2 + 0.5)
        behind += int(((z <= 0.2) & inside).sum())
        off += int(((z > 0.2) & inside & ~((px >= 0) & (px < v["W"]) & (py >= 0) & (py < v["H"]))).sum())
    assert behind > 100 and off > 100
    # the float32 restatement takes every decision as float64 does on the robust points
    _, touched32, _ = CR.run_case(views, True, dtype=np.float32)
    assert np.array_equal(touched[~fragile], touched32[~fragile])
    # the unit-ball inputs: every |q| <= 1, and the views update much of it
    mb = np.sqrt(CR.squared_norm(CR.grid_points(CR.BALL_DIMS, CR.BALL_ORIGIN, CR.BALL_VOXEL)))
    assert mb.max() <= 1.0 and CR.BALL_DIMS[0] > 64


# ---- the example -------------------------------------------------------------------------------------------------------
def test_example_with_unbounded_takes_the_cameras_sphere_and_writes_the_unbounded_mesh(monkeypatch, tmp_path, capsys):
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("example_extract_mesh_unbounded", os.path.join(ROOT, "examples", "extract_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    calls = []
    mesh = tuple(types.SimpleNamespace(shape=(n, 3), name=m) for n, m in zip((8, 12, 8), ("vertices", "faces", "colors")))

    class Volume:
        dims, voxel_size, sdf_trunc = (4, 4, 4), 0.5, 2.0

        def extract_mesh(self, *a, **kw):
            calls.append(("extract_mesh", a, kw))
            return mesh

    class Scene:
        loaded_iter = 7

        def __init__(self, *a, **kw):
            pass

        def getTrainCameras(self):
            return ["cam"]

    monkeypatch.setattr(mod, "GaussianModel", lambda d: types.SimpleNamespace(get_xyz="xyz"))
    monkeypatch.setattr(mod, "Scene", Scene)
    monkeypatch.setattr(mod, "bounding_sphere", lambda cams: calls.append(("bounding_sphere", cams)) or ((1.0, 2.0, 3.0), 4.0))
    monkeypatch.setattr(mod, "volume_for_points", lambda xyz, **kw: calls.append(("volume_for_points", kw)) or Volume())
    monkeypatch.setattr(mod, "contracted_volume_for_points",
                        lambda xyz, c, r, **kw: calls.append(("contracted_volume_for_points", xyz, c, r, kw)) or Volume())
    monkeypatch.setattr(mod, "fuse_views", lambda *a, **kw: calls.append(("fuse_views", kw)))
    monkeypatch.setattr(mod, "write_ply_mesh", lambda path, *a: calls.append(("write_ply_mesh", path) + tuple(x.name for x in a)))
    monkeypatch.setattr(mod, "clean_mesh", lambda *a, **kw: calls.append(("clean_mesh", kw)) or mesh)
    monkeypatch.setattr(mod, "torch", types.SimpleNamespace(no_grad=torch.no_grad, float32=torch.float32,
                                                            tensor=lambda *a, **kw: "background"))
    monkeypatch.setattr(mod, "ModelParams", lambda **kw: types.SimpleNamespace(sh_degree=3, white_background=False, **kw))
    base = ["-m", str(tmp_path), "-s", "dataset"]
    mod.main(base + ["--unbounded"])
    raw = os.path.join(str(tmp_path), "mesh", "iteration_7", "tsdf_mesh_unbounded.ply")
    assert calls == [("bounding_sphere", ["cam"]),
                     ("contracted_volume_for_points", "xyz", (1.0, 2.0, 3.0), 4.0, {"resolution": 512, "sdf_trunc": None}),
                     ("fuse_views", {"alpha_min": 0.5, "max_depth": None}), ("extract_mesh", (), {}),
                     ("write_ply_mesh", raw, "vertices", "faces", "colors")]
    del calls[:]
    mod.main(base + ["--unbounded", "--mesh_res", "128", "--num_cluster", "50", "--sdf_trunc", "0.25"])
    assert calls[1][4] == {"resolution": 128, "sdf_trunc": 0.25} and calls[4][1] == raw
    assert calls[5] == ("clean_mesh", {"keep_largest": 50, "min_faces": 50})
    assert calls[6][1] == os.path.join(os.path.dirname(raw), "tsdf_mesh_unbounded_post.ply") and len(calls) == 7
    del calls[:]
    mod.main(base)                                                         # the bounded default is unchanged
    assert [c[0] for c in calls] == ["volume_for_points", "fuse_views", "extract_mesh", "write_ply_mesh"]
    assert calls[-1][1] == os.path.join(os.path.dirname(raw), "tsdf_mesh.ply")
    for flags in (["--mesh_res", "128"], ["--unbounded", "--mesh_res", "1"], ["--unbounded", "--resolution", "64"],
                  ["--unbounded", "--voxel_size", "0.1"]):
        with pytest.raises(SystemExit):
            mod.main(base + flags)
