"""CPU-side checks of the registration layer (csrc/icp.hip, csrc/icp_math.h; geometry_eval.py): the ABI and
the refusals of the entry points -- all before a GPU is asked for --, ``estimate_similarity`` on exact pairs, ``crop_points``
on CPU tensors, the restatement the GPU tests compare against (tests/icp_restate.py) against the kernel's own body built
by the host compiler (csrc/icp_math.h through tests/icp_host_check.cpp) and against a dictionary of cells, and the
condition on the registration case that makes the GPU comparison mean something."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import icp_restate as R
import nearest_restate as NR
from mvs_gaussian_splatting_amd.geometry_eval import (CropVolume, IcpSums, align_cameras, crop_points, estimate_similarity,
                                                      icp_registration, icp_step, load_crop_volume, register_tnt,
                                                      tnt_stages, transform_points, uniform_down_sample, voxel_down_sample)

ENTRY_POINTS = ("gsr_icp_transform", "gsr_icp_workspace_bytes", "gsr_icp_accumulate")
BAD, CAPACITY, ALIGN = -1, -2, -3


# ---- ABI and refusals ----------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_abi_versions_agree():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib, geometry_eval
    for name in ("transform_points", "voxel_down_sample", "estimate_similarity", "align_cameras", "icp_step",
                 "icp_registration", "register_tnt", "load_crop_volume", "crop_points"):
        assert getattr(pkg, name) is getattr(geometry_eval, name) and name in pkg.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\b(int|size_t) " + name + r"\(", header), name
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("gsr_icp_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 43
    assert int(re.search(r"#define GSR_ICP_WORDS (\d+)", header).group(1)) == geometry_eval.ICP_WORDS == 1 + R.TERMS


def test_workspace_holds_one_partial_per_workgroup():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    last = 0
    for q in (0, 1, 256, 257, 65536, 65537, 262144, 262145, 10_000_000):
        w = lib.gsr_icp_workspace_bytes(q)
        blocks = min(1024, -(-q // 256))
        assert w % 256 == 0 and w >= 18 * 8 * max(1, blocks) and w >= last and w <= 18 * 8 * 1024 + 256
        last = w


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 8192)()
    p = (C.addressof(buf) + 255) // 256 * 256
    m = (C.c_double * 12)(*np.eye(4)[:3].reshape(-1))
    piv = (C.c_double * 6)()
    tr, acc = lib.gsr_icp_transform, lib.gsr_icp_accumulate
    assert tr(p, -1, m, p, None) == BAD
    assert tr(p, 2 ** 31 - 255, m, p, None) == BAD
    assert tr(p, 10, None, p, None) == BAD
    assert tr(None, 10, m, p, None) == BAD and tr(p, 10, m, None, None) == BAD
    assert tr(p + 2, 10, m, p, None) == ALIGN
    nan = (C.c_double * 12)(*([float("nan")] + [0.0] * 11))
    assert tr(p, 10, nan, p, None) == BAD and b"finite" in lib.gsr_last_error()
    assert tr(None, 0, m, None, None) == 0                                      # nothing to do
    Q = 10
    wb = lib.gsr_icp_workspace_bytes(Q)
    good = [p, p, p, Q, p, 5, 1.0, piv, p, wb, p]
    for n, code in ((0, BAD), (1, BAD), (2, BAD), (4, BAD), (7, BAD), (8, BAD), (10, BAD)):
        args = list(good)
        args[n] = None
        assert acc(*args, None) == code, n
    for n, value, code in ((3, -1, BAD), (5, -1, BAD), (3, 2 ** 31 - 255, BAD), (6, -1.0, BAD), (6, float("nan"), BAD),
                           (9, wb - 1, CAPACITY), (8, p + 128, ALIGN), (0, p + 2, ALIGN), (10, p + 4, ALIGN)):
        args = list(good)
        args[n] = value
        assert acc(*args, None) == code, (n, value)
    inf = (C.c_double * 6)(*([float("inf")] + [0.0] * 5))
    args = list(good)
    args[7] = inf
    assert acc(*args, None) == BAD and b"pivots" in lib.gsr_last_error()


def test_python_functions_refuse_bad_arguments_and_cpu_tensors():
    from mvs_gaussian_splatting_amd import _lib
    pts = torch.zeros(5, 3)
    bad_row = np.eye(4)
    bad_row[3] = [0, 0, 1e-9, 1]
    for T in (bad_row, np.eye(3), np.full((4, 4), np.nan), "x"):
        with pytest.raises(ValueError):
            transform_points(pts, T)
        with pytest.raises(ValueError):
            icp_step(pts, pts, T, 1.0)
        with pytest.raises(ValueError):
            icp_registration(pts, pts, 1.0, init=T)
    for fn in (lambda: transform_points(pts, np.eye(4)), lambda: voxel_down_sample(pts, 0.1),
               lambda: icp_step(pts, pts, np.eye(4), 1.0), lambda: icp_registration(pts, pts, 1.0),
               lambda: register_tnt(pts, pts, np.eye(4), None, 0.1)):
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            fn()
    for bad in (0, -1.0, float("inf"), float("nan"), True, "1"):
        with pytest.raises(ValueError):
            voxel_down_sample(pts, bad)
        with pytest.raises(ValueError):
            icp_step(pts, pts, np.eye(4), bad)
    with pytest.raises(ValueError):
        voxel_down_sample(pts, 0.1, origin=(0, 0))
    with pytest.raises(ValueError):
        voxel_down_sample(torch.zeros(5, 2), 0.1)
    with pytest.raises(ValueError):
        icp_step(pts, pts, np.eye(4), 1.0, pivots=((0, 0, 0), (0, 0)))
    with pytest.raises(ValueError):
        icp_registration(pts, pts, 1.0, max_iterations=-1)
    with pytest.raises(ValueError):
        uniform_down_sample(pts, 0)
    assert uniform_down_sample(torch.arange(21.0).reshape(7, 3), 3)[:, 0].tolist() == [0.0, 9.0, 18.0]
    st = tnt_stages(0.01)
    assert [(s.kind, s.max_dist, s.max_iterations) for s in st] == [("voxel", 0.8, 20), ("voxel", 0.2, 20), ("every", 0.02, 20)]
    assert st[0].param == 0.01 and st[1].param == 0.005


# ---- estimate_similarity ---------------------------------------------------------------------------------------------------
def _dyadic_points(rng, n):
    return np.round(rng.uniform(-4, 4, size=(n, 3)) * 1024) / 1024


@pytest.mark.parametrize("scale", [1.0, 0.37, 2.5])
def test_estimate_similarity_recovers_known_transforms_to_1e_12(scale):
    rng = np.random.default_rng(5)
    a = _dyadic_points(rng, 40)
    T = R.similarity([20.0, -35.0, 50.0], [0.3, -1.2, 2.0], scale)
    b = a @ T[:3, :3].T + T[:3, 3]
    got = estimate_similarity(a, b, with_scaling=True)
    assert np.abs(got - T).max() <= 1e-12
    assert np.array_equal(got[3], [0, 0, 0, 1])
    if scale == 1.0:
        rigid = estimate_similarity(torch.tensor(a), torch.tensor(b))
        assert np.abs(rigid - T).max() <= 1e-12
        assert np.abs(align_cameras(a, b) - T).max() <= 1e-12
    else:                                                     # without scaling: the best rotation, and a rotation exactly
        rigid = estimate_similarity(a, b)
        assert np.abs(rigid[:3, :3] @ rigid[:3, :3].T - np.eye(3)).max() <= 1e-14
        assert np.abs(rigid[:3, :3] - T[:3, :3] / scale).max() <= 1e-12


def test_estimate_similarity_from_sums_about_any_pivots_is_the_one_from_arrays():
    rng = np.random.default_rng(6)
    a = _dyadic_points(rng, 30) + 100.0
    T = R.similarity([5.0, 8.0, -3.0], [1.0, 2.0, 3.0], 1.1)
    b = a @ T[:3, :3].T + T[:3, 3]
    for cq, cr in ((a.mean(axis=0), b.mean(axis=0)), (np.array([99.0, 101.0, 100.0]), np.array([120.0, 90.0, 115.0]))):
        x, y = a - cq, b - cr
        sums = IcpSums(30, x.sum(axis=0), y.sum(axis=0), x.T @ y, float((x * x).sum()), 0.0, cq, cr, 30)
        assert np.abs(estimate_similarity(sums, with_scaling=True) - T).max() <= 1e-10


def test_a_mirrored_pair_set_yields_a_proper_rotation():
    rng = np.random.default_rng(7)
    a = _dyadic_points(rng, 25)
    b = a * [1.0, 1.0, -1.0]
    for ws in (False, True):
        T = estimate_similarity(a, b, with_scaling=ws)
        Rm = T[:3, :3] / np.cbrt(np.linalg.det(T[:3, :3]))
        assert np.linalg.det(T[:3, :3]) > 0 and np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12


def test_collinear_and_too_few_pairs_raise():
    line = np.outer(np.arange(10.0), [1.0, 2.0, -0.5]) + [3.0, 1.0, 2.0]
    with pytest.raises(ValueError, match="rank"):
        estimate_similarity(line, line * 2.0)
    with pytest.raises(ValueError, match="rank"):
        estimate_similarity(np.ones((5, 3)), np.ones((5, 3)))
    with pytest.raises(ValueError, match="at least 3"):
        estimate_similarity(np.eye(3)[:2], np.eye(3)[:2])
    with pytest.raises(ValueError):
        estimate_similarity(np.zeros((4, 3)), np.zeros((5, 3)))
    with pytest.raises(ValueError):
        estimate_similarity(np.zeros((4, 3)))
    plane = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.0]])          # rank 2 determines the rotation
    assert np.abs(estimate_similarity(plane, plane) - np.eye(4)).max() <= 1e-14


# ---- crop ------------------------------------------------------------------------------------------------------------------
L_SHAPE = [(0, 0), (3, 0), (3, 1), (1, 1), (1, 3), (0, 3)]           # concave: (2, 2) is in its hull and outside it


def _inside_l(u, v):
    return (0 < u < 3 and 0 < v < 1) or (0 < u < 1 and 0 < v < 3)


def _volume(axis, lo=-0.5, hi=0.75):
    u, v = [a for a in (0, 1, 2) if a != axis]
    poly = np.full((len(L_SHAPE), 3), 77.0)                          # the coordinate along the axis is not used
    poly[:, u], poly[:, v] = [p[0] for p in L_SHAPE], [p[1] for p in L_SHAPE]
    return CropVolume(axis, lo, hi, poly)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_crop_points_on_a_concave_polygon_per_orthogonal_axis(axis, tmp_path):
    u, v = [a for a in (0, 1, 2) if a != axis]
    g = np.arange(-0.25, 3.5, 0.5)                                   # no grid point on the outline
    pts = np.zeros((g.size * g.size * 3, 3))
    uu, vv, ww = np.meshgrid(g, g, [-1.0, 0.0, 1.0], indexing="ij")
    pts[:, u], pts[:, v], pts[:, axis] = uu.ravel(), vv.ravel(), ww.ravel()
    want = np.array([_inside_l(p[u], p[v]) and -0.5 <= p[axis] <= 0.75 for p in pts])
    assert 0 < want.sum() < len(pts) and not want[(pts[:, u] == 2.25) & (pts[:, v] == 2.25)].any()
    path = tmp_path / "crop.json"
    vol = _volume(axis)
    path.write_text(json.dumps({"class_name": "SelectionPolygonVolume", "orthogonal_axis": "XYZ"[axis], "axis_min": -0.5,
                                "axis_max": 0.75, "bounding_polygon": vol.polygon.tolist(), "version_major": 1}))
    loaded = load_crop_volume(str(path))
    assert loaded.orthogonal_axis == axis and np.array_equal(loaded.polygon, vol.polygon)
    for dtype in (torch.float32, torch.float64):
        t = torch.tensor(pts, dtype=dtype)
        got, mask = crop_points(t, loaded, return_mask=True)
        assert np.array_equal(mask.numpy(), want) and torch.equal(got, t[torch.tensor(want)]) and got.dtype == dtype
    rev = CropVolume(axis, -0.5, 0.75, vol.polygon[::-1].copy())    # the winding does not matter
    assert np.array_equal(crop_points(torch.tensor(pts), rev, return_mask=True)[1].numpy(), want)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_points_on_the_slab_faces_are_kept(axis):
    u, v = [a for a in (0, 1, 2) if a != axis]
    lo, hi = -0.5, 0.75
    w = np.array([lo, hi, np.nextafter(lo, -1), np.nextafter(hi, 2), 0.0])
    pts = np.zeros((5, 3))
    pts[:, u], pts[:, v], pts[:, axis] = 0.5, 0.5, w
    assert crop_points(torch.tensor(pts), _volume(axis, lo, hi), return_mask=True)[1].tolist() == [True, True, False, False, True]


def test_load_crop_volume_refuses_what_is_not_one(tmp_path):
    path = tmp_path / "bad.json"
    for d in ({"orthogonal_axis": "W", "axis_min": 0, "axis_max": 1, "bounding_polygon": [[0, 0, 0]] * 3},
              {"orthogonal_axis": "X", "axis_min": 0, "axis_max": 1, "bounding_polygon": [[0, 0, 0]] * 2},
              {"orthogonal_axis": "X", "axis_min": 2, "axis_max": 1, "bounding_polygon": [[0, 0, 0]] * 3},
              {"axis_min": 0, "axis_max": 1, "bounding_polygon": [[0, 0, 0]] * 3}):
        path.write_text(json.dumps(d))
        with pytest.raises(ValueError):
            load_crop_volume(str(path))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def test_restated_voxel_down_sample_against_a_dictionary_of_cells():
    rng = np.random.default_rng(3)
    cloud = R.asymmetric_cloud(2000)
    faces = (rng.integers(-8, 8, size=(300, 3)) * 0.25).astype(np.float32)              # every coordinate on a cell face
    for pts, h, origin in ((cloud, 0.3, None), (cloud, 0.05, None), (cloud, 100.0, None), (cloud[:1], 0.3, None),
                           (faces, 0.25, (-2.0, -2.0, -2.0)), (cloud, 0.3, (-1.0, -2.0, -3.0))):
        rows, keys = R.voxel_down_sample(pts, h, origin)
        means, triples = R.voxel_cells(pts, h, origin)
        assert [(int(k) >> 42, (int(k) >> 21) & (2 ** 21 - 1), int(k) & (2 ** 21 - 1)) for k in keys] == triples
        assert np.all(np.diff(keys) > 0)
        assert np.abs(rows.astype(np.float64) - means).max() <= 2.0 ** -24 * max(1.0, np.abs(means).max()) * 1.0000001
    assert len(R.voxel_down_sample(cloud, 100.0)[0]) == 1 and len(R.voxel_down_sample(cloud, 0.05)[0]) > 1500
    lone = R.voxel_down_sample(np.array([[-0.0, 1.5, 2.0]], dtype=np.float32), 1.0)[0]
    assert lone.view(np.uint32).tolist() == [[0x80000000, 0x3FC00000, 0x40000000]], "a cell of one point is a bit-copy"


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """``csrc/icp_math.h`` built by the host compiler from ``tests/icp_host_check.cpp`` into a program of its own, with the
    kernel's ``-ffp-contract=off``."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    folder = tmp_path_factory.mktemp("icp_host")
    exe = str(folder / "icp_host_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "icp_host_check.cpp"), "-o", exe], check=True)

    def run(T, cq, cr, t2, n_target, p, r, dist2, nearest):
        path = str(folder / "pairs.bin")
        rec = np.zeros(len(p), dtype=[("p", "<f4", 3), ("r", "<f4", 3), ("d", "<f4"), ("n", "<i4")])
        rec["p"], rec["r"], rec["d"], rec["n"] = p, r, dist2, nearest
        with open(path, "wb") as f:
            f.write(np.asarray(T, dtype="<f8")[:3].tobytes() + np.asarray(cq, dtype="<f8").tobytes() +
                    np.asarray(cr, dtype="<f8").tobytes() + struct.pack("<fii", float(t2), n_target, len(p)) + rec.tobytes())
        rows = [line.split() for line in subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()]
        accepted = np.array([int(w[0]) for w in rows], dtype=bool)
        q = np.array([[int(x, 16) for x in w[1:4]] for w in rows], dtype=np.uint32).reshape(-1, 3)
        terms = np.array([[int(x, 16) for x in w[4:]] for w in rows], dtype=np.uint64).reshape(-1, R.TERMS)
        return accepted, q, terms
    return run


@pytest.mark.parametrize("offset", [0.0, 1e4])
def test_host_build_of_the_kernels_body_gives_the_restatements_bits(host_check, offset):
    src = R.asymmetric_cloud(700, offset=offset)
    tgt = R.asymmetric_cloud(500, seed=8, offset=offset)
    T = R.about(R.similarity([3.0, -2.0, 1.0], [0.05, -0.02, 0.01], 1.02), src.astype(np.float64).mean(axis=0))
    max_dist = 0.2
    cq, cr = src.astype(np.float64).mean(axis=0) + 0.123, tgt.astype(np.float64).mean(axis=0) - 0.321
    st = R.step(src, tgt, T, max_dist, (cq, cr))
    assert 50 < st.count < len(src) - 50, "both sides of the threshold are exercised"
    nearest = st.nearest.copy()
    nearest[::97] = -1                                                        # an empty-target answer is never accepted
    accepted, q, terms = host_check(T, cq, cr, R.thr2(max_dist), len(tgt), src, tgt[st.nearest], st.dist2, nearest)
    want_accept = st.accepted.copy()
    want_accept[::97] = False
    assert np.array_equal(accepted, want_accept)
    assert np.array_equal(q, st.q.view(np.uint32)), "the transformed coordinates differ in their float32 bits"
    want = R.pair_terms(st.q, tgt[st.nearest], st.dist2, cq, cr)
    assert np.array_equal(terms, want.view(np.uint64)), "a pair term differs in its float64 bits"


def test_transform_restatement_rounds_once_and_is_not_the_float32_product():
    src = R.asymmetric_cloud(2000, offset=1e4)
    T = R.about(R.similarity([3.0, -2.0, 1.0], [0.05, -0.02, 0.01], 1.02), src.astype(np.float64).mean(axis=0))
    q = R.transform(src, T)
    exact = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert np.abs(q.astype(np.float64) - exact).max() <= np.spacing(np.float32(np.abs(exact).max())) * 0.5000001
    f32 = (src @ T[:3, :3].T.astype(np.float32) + T[:3, 3].astype(np.float32)).astype(np.float32)
    assert not np.array_equal(f32, q), "a float32 product would pass for it: the case checks nothing"


def test_restated_icp_converges_onto_the_known_similarity():
    """The condition on the reference alone: rotation 3 degrees, shift 2 % of the extent, scale 1.02."""
    src, tgt, T, max_dist = R.registration_case(True)
    assert len(src) == 2000 and np.array_equal(tgt, R.transform(src, T))
    scale = np.cbrt(np.linalg.det(T[:3, :3]))
    assert abs(scale - 1.02) < 1e-12
    assert abs(np.degrees(np.arccos((np.trace(T[:3, :3] / scale) - 1) / 2)) - 3.0) < 1e-9
    ext = R.extent(src)
    moved = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - src
    assert np.linalg.norm(moved, axis=1).max() > 0.02 * ext
    res = R.registration_restated(True)
    err = R.max_point_error(res.transformation, T, src)
    print(f"restated ICP: {res.iterations} iterations, fitness {res.fitness}, rmse {res.inlier_rmse:.3e}, "
          f"max point error {err:.3e} = {err / ext:.3e} of the extent")
    assert res.converged and res.iterations <= 30 and res.fitness == 1.0
    assert err <= 1e-5 * ext
    rigid = R.registration_restated(False)
    _, _, T_rigid, _ = R.registration_case(False)
    assert rigid.converged and R.max_point_error(rigid.transformation, T_rigid, src) <= 1e-5 * ext


def test_zero_pivots_would_miss_the_bound_on_the_offset_cloud():
    """On a cloud 1e4 from the origin at unit spread the centred moments H = sum a b^T - (sum a)(sum b)^T / n that
    estimate_similarity decomposes are of order n, while with zero pivots each term a_i b_j is of order 1e8 and carries a
    rounding of 1e-8: H formed from zero-pivot sums -- even exactly rounded ones -- is further from H formed about the
    centroids than the whole bound the device sums get there.  The pivots of the GPU case are therefore doing something."""
    src = R.asymmetric_cloud(2000, offset=1e4)
    tgt = R.asymmetric_cloud(2000, seed=8, offset=1e4)
    q = R.transform(src, np.eye(4))
    dist2, nearest, _ = NR.nearest_f32_brute(q, tgt)
    t2 = R.thr2(0.3)
    zero = R.accumulate(q, dist2, nearest, tgt, t2)
    cq, cr = q[zero.accepted].astype(np.float64).mean(axis=0), tgt[nearest[zero.accepted]].astype(np.float64).mean(axis=0)
    piv = R.accumulate(q, dist2, nearest, tgt, t2, cq, cr)
    assert piv.count == zero.count > 500
    gap = np.abs(R.centred_moments(zero) - R.centred_moments(piv))
    bound = piv.bound[6:15].reshape(3, 3)
    print(f"H from zero pivots is off by up to {gap.max():.3e}; the bound about the centroids is {bound.max():.3e}")
    assert (gap > bound).any() and gap.max() > 100 * bound.max()
    assert zero.bound[6:15].min() > 1e6 * bound.max(), "and the same bound about zero is no bound on H at all"
