"""CPU-side checks of the geometry evaluation (csrc/nearest.hip; geometry_eval.py): the ABI and the
refusals of the four entry points -- which all come before a GPU is asked for --, the case table of tests/nearest_restate.py
proved well-posed (its float32 definition against the float64 truth), ``sample_surface`` on CPU tensors against a numpy
restatement, the argument checks of ``evaluate_points``, ``read_ply_mesh`` and the flags of examples/eval_mesh.py."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import nearest_restate as N
import tsdf_restate as T

ENTRY_POINTS = ("gsr_nn_index_bytes", "gsr_nn_build", "gsr_nn_query_workspace_bytes", "gsr_nn_query")
BAD, CAPACITY, ALIGN = -1, -2, -3


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_four_entry_points_and_the_three_abi_versions_agree():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib, geometry_eval
    for name in ("NearestIndex", "nearest_points", "sample_surface", "evaluate_points", "evaluate_mesh"):
        assert getattr(pkg, name) is getattr(geometry_eval, name) and name in pkg.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\b(int|size_t) " + name + r"\(", header), name
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("gsr_nn_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 32


def test_sizes_grow_with_the_counts_and_are_multiples_of_256():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    last_i = last_w = 0
    for n in (0, 1, 127, 128, 129, 8192, 8193, 1_000_000):
        i, w = lib.gsr_nn_index_bytes(n), lib.gsr_nn_query_workspace_bytes(n)
        assert i % 256 == 0 and w % 256 == 0 and i >= last_i and w >= last_w and i > 24 * n and w > 16 * n
        assert i == lib.gsr_knn3_workspace_bytes(n), "one index layout serves distCUDA2 and the cross-set query"
        last_i, last_w = i, w


def test_every_entry_point_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 1024)()
    p = (C.addressof(buf) + 255) // 256 * 256                            # 256-byte aligned, 768 bytes behind it
    R = Q = 1000
    ib, wb = lib.gsr_nn_index_bytes(R), lib.gsr_nn_query_workspace_bytes(Q)

    build = lib.gsr_nn_build
    assert build(p, -1, p, ib, None) == BAD
    assert build(p, 2 ** 31 - 255, p, 2 ** 40, None) == BAD                # past GSR_NN_MAX_POINTS: 32-bit indices would wrap
    assert build(None, R, p, ib, None) == BAD
    assert build(p, R, None, ib, None) == BAD
    assert build(p, R, p, ib - 1, None) == CAPACITY and b"index" in lib.gsr_last_error()
    assert build(p, R, p, 0, None) == CAPACITY
    assert build(p, R, p + 128, ib, None) == ALIGN
    assert build(p + 2, R, p, ib, None) == ALIGN
    assert build(None, 0, None, 0, None) == 0                             # an empty reference needs no build

    query = lib.gsr_nn_query
    good = [p, ib, R, p, Q, p, p, p, wb]
    assert query(p, ib, -1, p, Q, p, p, p, wb, None) == BAD
    assert query(p, ib, R, p, -1, p, p, p, wb, None) == BAD
    assert query(p, 2 ** 40, 2 ** 31 - 255, p, Q, p, p, p, wb, None) == BAD
    assert query(p, ib, R, p, 2 ** 31 - 255, p, p, p, 2 ** 40, None) == BAD
    assert int(re.search(r"#define GSR_NN_MAX_POINTS (\d+)", open(os.path.join(ROOT, "include", "gsr.h")).read()).group(1)) == 2 ** 31 - 256
    for n in (0, 3, 5, 6, 7):                                            # every pointer
        args = list(good)
        args[n] = None
        assert query(*args, None) == BAD, n
    args = list(good)
    args[1] = ib - 1
    assert query(*args, None) == CAPACITY and b"index" in lib.gsr_last_error()
    args = list(good)
    args[8] = wb - 1
    assert query(*args, None) == CAPACITY and b"workspace" in lib.gsr_last_error()
    for n, off in ((0, 128), (7, 128), (0, 4), (7, 64), (3, 2), (5, 1), (6, 2)):
        args = list(good)
        args[n] = p + off
        assert query(*args, None) == ALIGN, n
    assert query(None, 0, R, None, 0, None, None, None, 0, None) == 0     # no queries: nothing to do
    # an empty reference still checks the arrays it would fill
    assert query(None, 0, 0, None, Q, p, p, None, 0, None) == BAD
    assert query(None, 0, 0, p, Q, p + 2, p, None, 0, None) == ALIGN


# ---- the case table is well-posed ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.CASE_NAMES)
def test_float32_definition_agrees_with_the_float64_truth(name):
    ref, query = N.case(name)
    d2, idx, ties = N.case_brute(name)
    assert d2.dtype == np.float32 and idx.dtype == np.int32 and d2.shape == idx.shape == (len(query),)
    if len(ref) == 0:
        assert np.isposinf(d2).all() and (idx == -1).all()
        return
    if len(query) == 0:
        return
    assert ((idx >= 0) & (idx < len(ref))).all() and (ties >= 1).all() and np.isfinite(d2).all()
    truth, _ = N.nearest_f64(query, ref)
    mine = N.dist2_f64(query, ref, idx)                                   # the float64 distance to the index float32 chose
    zero = truth == 0
    assert (mine[zero] == 0).all() and (d2[zero] == 0).all()
    err_idx = np.abs(mine[~zero] - truth[~zero]) / truth[~zero]
    err_val = np.abs(d2[~zero].astype(np.float64) - truth[~zero]) / truth[~zero]
    print(f"{name}: R = {len(ref)}, Q = {len(query)}, {int(zero.sum())} exact zeros, {int((ties > 1).sum())} queries with "
          f"ties, worst index error {err_idx.max(initial=0) / N.U:.2f} ulp, worst value error {err_val.max(initial=0) / N.U:.2f} ulp")
    assert err_idx.max(initial=0) <= N.BOUND and err_val.max(initial=0) <= N.BOUND
    assert truth[~zero].min(initial=1.0) > 1e-30, "a subnormal squared distance: the bound does not hold there"


def test_cases_have_the_shapes_they_are_there_for():
    shape = lambda n: (len(N.case(n)[0]), len(N.case(n)[1]))              # noqa: E731
    assert [shape(n)[0] for n in ("R1", "R127", "R128", "R129", "R8192", "R8193", "R0")] == [1, 127, 128, 129, 8192, 8193, 0]
    assert [shape(n)[1] for n in ("Q1", "Q255", "Q257", "Q0")] == [1, 255, 257, 0]
    assert shape("uniform_20000x10000") == (10000, 20000)
    d2, idx, ties = N.case_brute("self")
    assert (d2 == 0).all() and np.array_equal(idx, np.arange(3000)) and not N.has_ties("self")
    d2, idx, ties = N.case_brute("duplicated")
    ref = N.case("duplicated")[0]
    assert (ties % 2 == 0).all() and (d2[:700] == 0).all()
    for q in range(0, 1400, 97):                                         # the twin with the larger index loses
        twins = np.flatnonzero((ref == ref[idx[q]]).all(axis=1))
        assert len(twins) == 2 and idx[q] == twins.min()
    ref, query = N.case("coincident")
    assert (ref == ref[0]).all() and (N.case_brute("coincident")[1] == 0).all() and (N.case_brute("coincident")[2] == 500).all()
    assert (N.case_brute("coincident")[0][:3] == 0).all()
    ref, _ = N.case("collinear")
    assert (ref[:, 1:] == 0).all() and len(np.unique(ref[:, 0])) > 1400
    d2, idx, ties = N.case_brute("lattice_centres")
    assert (ties == 8).all() and (d2 == np.float32(3 * 0.125 ** 2)).all() and len(d2) == 11 ** 3
    ref, query = N.case("two_sheets")
    d2, idx, ties = N.case_brute("two_sheets")
    assert len(ref) > BOX_SUPER and set(np.sign(ref[idx, 2]).tolist()) == {-1.0, 1.0}
    ref, query = N.case("cluster_and_outliers")
    d = np.sqrt(N.case_brute("cluster_and_outliers")[0])
    assert (d[:300] < 4e-3).all() and (d[300:360] < 2.0).all() and d[360:].max() > 10.0
    ref, query = N.case("far_queries")
    box = (ref.max(axis=0) - ref.min(axis=0)).max() / (len(ref) / N.BOX) ** (1 / 3)
    outside = np.maximum(np.maximum(ref.min(axis=0) - query, query - ref.max(axis=0)), 0).max(axis=1)
    assert (outside > 1000 * box).all(), "every query lies 1000 box sizes or more outside the bounding box"
    assert sum(N.has_ties(n) for n in N.CASE_NAMES) >= 3 and not N.has_ties("uniform_20000x10000")


BOX_SUPER = N.BOX * N.SUPER


# ---- sample_surface ------------------------------------------------------------------------------------------------------
def _mesh():
    """The sphere of the TSDF tests with three zero-area faces put in (a repeated vertex, three collinear vertices, and one at
    the very end), float32 vertices."""
    v, f, _ = T.extract(T.sphere_field())
    v = np.concatenate([v.astype(np.float32), np.float32([[0, 0, 0], [1, 1, 1], [2, 2, 2]])])
    n = len(v)
    f = np.concatenate([f[:100], [[5, 5, 9]], f[100:], [[n - 3, n - 2, n - 1]], [[7, 8, 8]]]).astype(np.int64)
    return v, f


def _sample_restated(v, f, n, r):
    v64 = v.astype(np.float64)
    a, b, c = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    cum = np.cumsum(area)
    t = (np.arange(n) + r[:, 0].astype(np.float64)) * cum[-1] / n
    face = np.minimum(np.searchsorted(cum, t, side="right"), np.flatnonzero(area > 0)[-1])
    s, r2 = np.sqrt(r[:, 1].astype(np.float64))[:, None], r[:, 2].astype(np.float64)[:, None]
    pts = (1 - s) * a[face] + s * (1 - r2) * b[face] + s * r2 * c[face]
    return face, pts, area


def test_sample_surface_matches_its_restatement_and_never_lands_on_a_zero_area_face():
    from mvs_gaussian_splatting_amd import sample_surface
    v, f = _mesh()
    n = 5003
    r = torch.rand((n, 3), generator=torch.Generator().manual_seed(5)).numpy()
    pts, face = sample_surface(torch.from_numpy(v), torch.from_numpy(f), n, generator=torch.Generator().manual_seed(5))
    assert pts.shape == (n, 3) and pts.dtype == torch.float32 and face.shape == (n,) and face.dtype == torch.int64
    want_face, want_pts, area = _sample_restated(v, f, n, r)
    assert (area == 0).sum() == 3 and area[-1] == 0 and area[-2] == 0
    assert np.array_equal(face.numpy(), want_face)
    assert (area[face.numpy()] > 0).all(), "a sample landed on a zero-area face"
    err = np.abs(pts.numpy().astype(np.float64) - want_pts).max()
    bar = 16 * 2.0 ** -24 * np.abs(v).max()
    print(f"sample_surface: worst point error {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    # the same seed gives the same samples; int32 faces and float64 vertices are taken too
    pts2, face2 = sample_surface(torch.from_numpy(v).double(), torch.from_numpy(f).int(), n, generator=torch.Generator().manual_seed(5))
    assert torch.equal(face2, face) and pts2.dtype == torch.float64 and float((pts2 - pts.double()).abs().max()) <= bar


def test_sample_surface_is_stratified(monkeypatch):
    """At r0 = const sample i sits at (i + r0) total / n: a face of area A takes n A / total samples, give or take one."""
    from mvs_gaussian_splatting_amd import geometry_eval, sample_surface
    v, f = _mesh()
    n = 4001
    real = torch.rand
    monkeypatch.setattr(geometry_eval.torch, "rand", lambda *a, **kw: torch.cat((torch.full((n, 1), 0.37), real(n, 2)), dim=1))
    _, face = sample_surface(torch.from_numpy(v), torch.from_numpy(f), n)
    monkeypatch.undo()
    _, _, area = _sample_restated(v, f, 1, np.zeros((1, 3), np.float32))
    count = np.bincount(face.numpy(), minlength=len(f))
    want = n * area / area.sum()
    assert count.sum() == n and np.abs(count - want).max() <= 1.0 + 1e-9, np.abs(count - want).max()
    assert (count[area == 0] == 0).all()


def test_sample_surface_refusals():
    from mvs_gaussian_splatting_amd import sample_surface
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = torch.tensor([[0, 1, 2]])
    assert sample_surface(v, f, 0)[0].shape == (0, 3)
    assert sample_surface(v, f, 7)[0].shape == (7, 3)
    with pytest.raises(ValueError, match="no faces"):
        sample_surface(v, torch.zeros((0, 3), dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="no area"):
        sample_surface(v, torch.tensor([[0, 1, 1], [2, 2, 2]]), 5)
    for bad_v, bad_f, bad_n in ((v[:, :2], f, 5), (v.long(), f, 5), (v, f.float(), 5), (v, f[:, :2], 5), (v, f, -1), (v, f, 2.5),
                                (v, torch.tensor([[0, 1, 3]]), 5), (v, torch.tensor([[0, -1, 2]]), 5), (v.numpy(), f, 5)):
        with pytest.raises(ValueError):
            sample_surface(bad_v, bad_f, bad_n)


# ---- evaluate_points -------------------------------------------------------------------------------------------------------
def test_evaluate_points_argument_checks_come_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, NearestIndex, evaluate_mesh, evaluate_points, nearest_points
    a, b = torch.rand(10, 3), torch.rand(12, 3)
    for bad in (a[:, :2], a.reshape(-1), a.long(), a.numpy(), None):
        with pytest.raises(ValueError):
            evaluate_points(bad, b)
        with pytest.raises(ValueError):
            evaluate_points(a, bad)
        with pytest.raises(ValueError):
            nearest_points(bad, b)
        with pytest.raises(ValueError):
            NearestIndex(bad)
    for taus in ((0.0,), (-1.0,), (float("nan"),), (float("inf"),), ("a",), (0.1, 0.1), (True,)):
        with pytest.raises(ValueError):
            evaluate_points(a, b, thresholds=taus)
    for md in (0, -2.0, float("nan"), float("inf"), "far", True):
        with pytest.raises(ValueError):
            evaluate_points(a, b, max_dist=md)
    for bounds in ((0, 1), ([0, 0, 0],), ([0, 0, 0], [1, 1]), ([1, 1, 1], [0, 2, 2]), "box", ([0, 0, 0], [1, 1, 1], [2, 2, 2])):
        with pytest.raises(ValueError):
            evaluate_points(a, b, bounds=bounds)
    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        evaluate_points(a, b, thresholds=(0.1, 0.2), max_dist=1.0, bounds=([0, 0, 0], [1, 1, 1]))
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        nearest_points(a, b)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        NearestIndex(b.double())
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        evaluate_mesh(torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), torch.tensor([[0, 1, 2]]), b, 16)


def _eval_clouds():
    """The two pairs of clouds of the GPU test, made on the host from the restated sphere mesh."""
    from mvs_gaussian_splatting_amd import sample_surface
    v, f, _ = T.extract(T.sphere_field())
    v, f = torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f.astype(np.int64))
    gt = N.sphere_gt_points()
    out = {}
    for name, shift in (("sphere", (0.0, 0.0, 0.0)), ("shifted", N.EVAL_SHIFT)):
        pts, _ = sample_surface(v + torch.tensor(shift), f, N.EVAL_SAMPLES, generator=torch.Generator().manual_seed(11))
        out[name] = (pts.numpy(), gt)
    return out


def test_no_distance_of_the_evaluation_clouds_lies_near_a_threshold():
    """From the truth alone: what lets tests/test_gpu_nearest.py ask for exactly the truth's precision, recall and F-score."""
    for name, (pred, gt) in _eval_clouds().items():
        res, dists = N.evaluate_f64(pred, gt, N.EVAL_THRESHOLDS)
        N.assert_thresholds_are_clear(dists, N.EVAL_THRESHOLDS, name)
        print(name, res)
        shares = [t[k] for t in res["thresholds"] for k in ("precision", "recall")]
        assert 0.0 < min(shares) and any(s < 1.0 for s in shares), "a threshold that every distance passes checks nothing"
    assert res["accuracy"] > 0.1, "the shifted sphere is a third of a voxel off"


# ---- read_ply_mesh -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("empty", ["", "F", "VF"])
def test_read_ply_mesh_round_trips_write_ply_mesh(tmp_path, with_colors, empty):
    from mvs_gaussian_splatting_amd.ply_io import read_ply_mesh, write_ply_mesh
    rng = np.random.default_rng(3)
    V, F = (0 if "V" in empty else 57), (0 if "F" in empty else 101)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    f = rng.integers(0, max(V, 1), size=(F, 3)).astype(np.int32)
    c = rng.random((V, 3)).astype(np.float32) if with_colors else None
    path = str(tmp_path / "m.ply")
    write_ply_mesh(path, v, f, c)
    rv, rf, rc = read_ply_mesh(path)
    assert rv.dtype == np.float32 and rv.shape == (V, 3) and np.array_equal(rv.view(np.uint32), v.view(np.uint32))
    assert rf.dtype == np.int32 and rf.shape == (F, 3) and np.array_equal(rf, f)
    if with_colors:
        assert rc.dtype == np.uint8 and np.array_equal(rc, np.floor(np.clip(c.astype(np.float64), 0, 1) * 255.0 + 0.5).astype(np.uint8))
        again = str(tmp_path / "again.ply")
        write_ply_mesh(again, rv, rf, rc.astype(np.float64) / 255.0)
        assert open(again, "rb").read() == open(path, "rb").read(), "written, read and written again: the same bytes"
    else:
        assert rc is None
        again = str(tmp_path / "again.ply")
        write_ply_mesh(again, rv, rf)
        assert open(again, "rb").read() == open(path, "rb").read()


def test_read_ply_mesh_reads_ascii_and_uint_lists_and_refuses_other_polygons(tmp_path):
    from mvs_gaussian_splatting_amd.ply_io import read_ply_mesh
    head = "ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
    path = str(tmp_path / "a.ply")
    with open(path, "w") as f:
        f.write(head + "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\n"
                "property list uchar uint vertex_indices\nend_header\n"
                "0 0 0 255 0 0\n1 0 0.5 0 255 0\n0 1 0 0 0 255\n1 1 -2.25 9 8 7\n3 0 1 2\n3 2 1 3\n")
    v, fc, c = read_ply_mesh(path)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0.5], [0, 1, 0], [1, 1, -2.25]] and fc.tolist() == [[0, 1, 2], [2, 1, 3]]
    assert c.tolist() == [[255, 0, 0], [0, 255, 0], [0, 0, 255], [9, 8, 7]] and fc.dtype == np.int32
    quad = str(tmp_path / "q.ply")
    with open(quad, "w") as f:
        f.write(head + "element face 1\nproperty list uchar int vertex_index\nend_header\n0 0 0\n1 0 0\n0 1 0\n1 1 0\n4 0 1 3 2\n")
    with pytest.raises(ValueError, match="triangles"):
        read_ply_mesh(quad)
    # binary: uint indices read like int; a quad is refused
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
           "element face 1\nproperty list uchar uint vertex_indices\nend_header\n").encode()
    xyz = np.arange(9, dtype="<f4").tobytes()
    b = str(tmp_path / "b.ply")
    with open(b, "wb") as f:
        f.write(hdr + xyz + bytes([3]) + np.array([2, 0, 1], dtype="<u4").tobytes())
    v, fc, c = read_ply_mesh(b)
    assert fc.tolist() == [[2, 0, 1]] and c is None and v[2].tolist() == [6.0, 7.0, 8.0]
    with open(b, "wb") as f:
        f.write(hdr + xyz + bytes([4]) + np.array([2, 0, 1, 1], dtype="<u4").tobytes())
    with pytest.raises(ValueError, match="triangle"):
        read_ply_mesh(b)
    with open(b, "wb") as f:
        f.write(hdr + xyz + bytes([3]) + np.array([2, 0, 3], dtype="<u4").tobytes())
    with pytest.raises(ValueError, match="outside"):
        read_ply_mesh(b)
    with open(b, "wb") as f:
        f.write(b"plx\n")
    with pytest.raises(ValueError, match="not a PLY"):
        read_ply_mesh(b)


# ---- the example -------------------------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("example_eval_mesh", os.path.join(ROOT, "examples", "eval_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_help_flags_and_the_file_it_writes(monkeypatch, tmp_path, capsys):
    from mvs_gaussian_splatting_amd.ply_io import write_ply_mesh, write_ply_vertices
    mod = _example()
    with pytest.raises(SystemExit) as e:
        mod.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--mesh", "--gt", "--samples", "--tau", "--max_dist", "--seed"):
        assert flag in out
    mesh, gt = str(tmp_path / "tsdf_mesh_post.ply"), str(tmp_path / "gt.ply")
    write_ply_mesh(mesh, np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]]))
    cloud = np.zeros(5, dtype=[("x", "f4"), ("y", "f4"), ("z", "f4")])
    cloud["x"] = np.arange(5)
    write_ply_vertices(gt, cloud)
    base = ["--mesh", mesh, "--gt", gt]
    for flags in (["--samples", "0"], ["--tau", "0"], ["--tau", "-1"], ["--tau", "0.1", "0.1"], ["--max_dist", "0"],
                  ["--samples", "many"], ["--tau", "nan"]):
        with pytest.raises(SystemExit) as e:
            mod.main(base + flags)
        assert e.value.code == 2, flags
    for missing in (["--mesh", mesh], ["--gt", gt], ["--mesh", mesh + "x", "--gt", gt]):
        with pytest.raises(SystemExit):
            mod.main(missing)
    calls = []

    def fake(vertices, faces, gt_points, n_samples, **kw):
        calls.append((tuple(vertices.shape), tuple(faces.shape), tuple(gt_points.shape), n_samples, kw["thresholds"], kw["max_dist"],
                      kw["generator"].initial_seed()))
        return {"accuracy": 1.0, "completeness": 3.0, "chamfer": 2.0, "n_pred": n_samples, "n_gt": 5, "dropped_pred": 0.0,
                "dropped_gt": 0.25, "max_dist": kw["max_dist"], "n_samples": n_samples,
                "thresholds": [{"tau": t, "precision": 0.5, "recall": 0.25, "fscore": 1 / 3} for t in kw["thresholds"]]}

    monkeypatch.setattr(mod, "evaluate_mesh", fake)
    monkeypatch.setattr(mod.torch.Tensor, "to", lambda self, *a, **kw: self)
    res = mod.main(base + ["--samples", "64", "--tau", "0.5", "2", "--max_dist", "20", "--seed", "9"])
    assert calls == [((3, 3), (1, 3), (5, 3), 64, (0.5, 2.0), 20.0, 9)]
    import json
    with open(str(tmp_path / "results_mesh.json")) as f:
        saved = json.load(f)
    assert saved["chamfer"] == 2.0 and saved["seed"] == 9 and saved["faces"] == 1 and saved == json.loads(json.dumps(res))
    out = capsys.readouterr().out
    assert "chamfer 2" in out and "tau 0.5: precision 0.5000" in out and "results_mesh.json" in out
