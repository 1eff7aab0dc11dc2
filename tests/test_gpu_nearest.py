"""The cross-set nearest point and the geometry evaluation on the MI355X (mvs_gaussian_splatting_amd/geometry_eval.py,
csrc/nearest.hip on the index of csrc/knn.hip) against the restatements of tests/nearest_restate.py, on the case table
tests/test_nearest_host.py proves well-posed (run on the GPU box: pytest -m gpu).

Bars.  ``dist2`` and ``nearest`` equal the float32 brute force bit for bit and index for index, through ``NearestIndex.query``,
``nearest_points`` and the C entries; repeat runs, an index and workspace full of 0xFF or 0x00 bytes, and permuted queries
give the same bits; a permuted reference moves ``nearest`` through the permutation alone (with ties: to the smallest new
index).  ``evaluate_points``: accuracy, completeness and chamfer within 1e-6 relative of the float64 cKDTree truth (the
8 * 2^-24 of a squared distance, halved by the root, is below 3e-7), precision, recall and F-score exactly the truth's --
no float64 distance of those inputs lies within 1e-5 relative of a threshold, asserted here on the very inputs and in
the host test on the restated mesh.  ``distCUDA2`` returns, on four cases,
the bits recorded from it before its index build was shared (which are not those of knn_restate's unfused restatement).
"""
import zlib

import numpy as np
import pytest
import torch

import knn_restate as K
import nearest_restate as N
import tsdf_restate as T

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gd.shape == wd.shape and gi.shape == wi.shape, (what, gd.shape, wd.shape)
    bad = np.flatnonzero((_bits(gd) != _bits(wd)) | (gi != wi))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(wd)} results differ, first at query {bad[0]}: got "
                           f"({gd[bad[0]]!r}, {gi[bad[0]]}), want ({wd[bad[0]]!r}, {wi[bad[0]]})")


def _host(pair):
    d, i = pair
    assert d.dtype == torch.float32 and i.dtype == torch.int32 and d.is_cuda and i.is_cuda and not d.requires_grad
    return d.cpu().numpy(), i.cpu().numpy()


def _c_query(dev, ref, query, fill=None):
    """gsr_nn_build + gsr_nn_query on buffers of the caller's, pre-filled with `fill` bytes when given."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    R, Q = len(ref), len(query)
    r, q = torch.tensor(ref).to(dev).contiguous(), torch.tensor(query).to(dev).contiguous()
    ib, wb = lib.gsr_nn_index_bytes(R), lib.gsr_nn_query_workspace_bytes(Q)
    make = (lambda n: torch.empty(n, dtype=torch.uint8, device=dev)) if fill is None else \
        (lambda n: torch.full((n,), fill, dtype=torch.uint8, device=dev))
    index, ws = make(ib), make(wb)
    dist2 = torch.full((Q,), -1.0, dtype=torch.float32, device=dev)
    nearest = torch.full((Q,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        assert lib.gsr_nn_build(r.data_ptr(), R, index.data_ptr(), ib, s) == 0
        assert lib.gsr_nn_query(index.data_ptr(), ib, R, q.data_ptr(), Q, dist2.data_ptr(), nearest.data_ptr(), ws.data_ptr(),
                                wb, s) == 0
        torch.cuda.synchronize()
    return dist2.cpu().numpy(), nearest.cpu().numpy()


# ---- values: every case, every way in ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", N.CASE_NAMES)
def test_every_way_in_gives_the_bits_and_indices_of_the_float32_definition(gpu_device, name):
    from mvs_gaussian_splatting_amd import NearestIndex, nearest_points
    ref, query = N.case(name)
    want = N.case_brute(name)[:2]
    r, q = torch.tensor(ref).to(gpu_device), torch.tensor(query).to(gpu_device)
    index = NearestIndex(r)
    first = _host(index.query(q))
    _assert_same(first, want, f"NearestIndex.query, {name}")
    _assert_same(_host(index.query(q)), want, f"a second query of the same index, {name}")
    _assert_same(_host(nearest_points(q, r)), want, f"nearest_points, {name}")
    _assert_same(_c_query(gpu_device, ref, query), want, f"the C entries, {name}")
    if len(ref):
        assert ((first[1] >= 0) & (first[1] < len(ref))).all()


@pytest.mark.parametrize("name", ["R8193", "two_sheets", "lattice_centres", "cluster_and_outliers"])
def test_results_do_not_depend_on_what_the_index_and_workspace_held(gpu_device, name):
    ref, query = N.case(name)
    want = N.case_brute(name)[:2]
    for fill in (0xFF, 0x00):
        _assert_same(_c_query(gpu_device, ref, query, fill), want, f"{name}, buffers pre-filled with {fill:#04x}")


@pytest.mark.parametrize("name", ["R8193", "duplicated", "lattice_centres", "two_sheets", "far_queries", "uniform_20000x10000"])
def test_permuted_queries_and_a_permuted_reference(gpu_device, name):
    from mvs_gaussian_splatting_amd import nearest_points
    ref, query = N.case(name)
    wd, wi, _ = N.case_brute(name)
    rng = np.random.default_rng(len(ref))
    r = torch.tensor(ref).to(gpu_device)
    for what, perm in (("random", rng.permutation(len(query))), ("reversed", np.arange(len(query))[::-1].copy())):
        got = _host(nearest_points(torch.tensor(query[perm]).to(gpu_device), r))
        _assert_same(got, (wd[perm], wi[perm]), f"{name}, {what} permutation of the queries")
    perm = rng.permutation(len(ref))                                     # new reference point j is old point perm[j]
    got = _host(nearest_points(torch.tensor(query).to(gpu_device), torch.tensor(ref[perm]).to(gpu_device)))
    if N.has_ties(name):
        want = N.nearest_f32_brute(query, ref[perm])[:2]                  # the smallest NEW index among the ties
        assert not np.array_equal(perm[want[1]], wi), "the permutation moved no tie: the case checks nothing"
    else:
        inverse = np.empty(len(ref), dtype=np.int32)
        inverse[perm] = np.arange(len(ref), dtype=np.int32)
        want = (wd, inverse[wi])
    _assert_same(got, want, f"{name}, permuted reference")
    assert np.array_equal(_bits(got[0]), _bits(wd)), "the distances do not depend on the order of the reference"


# ---- the wrapper's input forms ---------------------------------------------------------------------------------------------
def test_wrapper_takes_views_float64_half_grad_tensors_and_empty_clouds(gpu_device):
    from mvs_gaussian_splatting_amd import NearestIndex, nearest_points
    ref, query = N.case("Q257")
    want = N.case_brute("Q257")[:2]
    view_q = torch.from_numpy(np.ascontiguousarray(query.T)).to(gpu_device).T
    view_r = torch.from_numpy(np.ascontiguousarray(ref.T)).to(gpu_device).T
    assert not view_q.is_contiguous() and not view_r.is_contiguous()
    _assert_same(_host(nearest_points(view_q, view_r)), want, "[3, N].T views")
    leaf = torch.tensor(query).to(gpu_device).requires_grad_(True)
    _assert_same(_host(nearest_points(leaf, torch.tensor(ref).to(gpu_device).requires_grad_(True))), want, "requires_grad")
    # float64 is rounded to float32 first
    rng = np.random.default_rng(64)
    r64, q64 = rng.random((500, 3)) * 3 - 1, rng.random((300, 3)) * 3 - 1
    got = _host(nearest_points(torch.from_numpy(q64).to(gpu_device), torch.from_numpy(r64).to(gpu_device)))
    _assert_same(got, N.nearest_f32_brute(q64.astype(np.float32), r64.astype(np.float32))[:2], "float64 input")
    # the edge shapes of the contract
    d, i = _host(nearest_points(torch.tensor(query).to(gpu_device), torch.empty(0, 3, device=gpu_device)))
    assert np.isposinf(d).all() and (i == -1).all() and d.shape == (257,)
    d, i = _host(NearestIndex(torch.tensor(ref).to(gpu_device)).query(torch.empty(0, 3, device=gpu_device)))
    assert d.shape == (0,) and i.shape == (0,)
    with pytest.raises(ValueError):
        nearest_points(torch.zeros(5, 2, device=gpu_device), torch.zeros(5, 3, device=gpu_device))


def test_non_finite_coordinates_end_and_stay_in_range(gpu_device):
    """NaN / Inf coordinates give an unspecified value; the call must end, every index must be -1 or a reference index,
    and the finite queries of the same call against a finite reference keep their bits."""
    from mvs_gaussian_splatting_amd import nearest_points
    ref, query = N.case("R8193")
    wd, wi, _ = N.case_brute("R8193")
    q = query.copy()
    q[0], q[1], q[2], q[3] = (np.nan, 0, 0), (np.inf, 0, 0), (0, -np.inf, np.nan), (np.nan, np.nan, np.nan)
    d, i = _host(nearest_points(torch.tensor(q).to(gpu_device), torch.tensor(ref).to(gpu_device)))
    assert ((i >= -1) & (i < len(ref))).all()
    _assert_same((d[4:], i[4:]), (wd[4:], wi[4:]), "the finite queries next to the non-finite ones")
    r = ref.copy()
    r[5], r[77] = (np.nan, 1, 1), (np.inf, -np.inf, 0)
    d, i = _host(nearest_points(torch.tensor(query).to(gpu_device), torch.tensor(r).to(gpu_device)))
    assert ((i >= -1) & (i < len(ref))).all() and d.shape == (len(query),)


# ---- evaluate_points against the float64 truth -------------------------------------------------------------------------------
def _sphere_mesh(dev):
    from mvs_gaussian_splatting_amd import TSDFVolume
    field = T.sphere_field()
    nz, ny, nx = field["tsdf"].shape
    vol = TSDFVolume(field["origin"], field["voxel_size"], (nx, ny, nz), field["sdf_trunc"], with_color=True, device=dev)
    vol.tsdf = torch.from_numpy(field["tsdf"]).to(dev)
    vol.weight = torch.from_numpy(field["weight"]).to(dev)
    vol.color = torch.from_numpy(field["color"]).to(dev)
    vertices, faces, _ = vol.extract_mesh()
    return vertices, faces


@pytest.mark.parametrize("shape", ["sphere", "shifted"])
def test_evaluate_points_matches_the_float64_truth(gpu_device, shape):
    from mvs_gaussian_splatting_amd import evaluate_mesh, evaluate_points, sample_surface
    vertices, faces = _sphere_mesh(gpu_device)
    assert vertices.shape[0] > 1000 and faces.shape[0] > 2000
    if shape == "shifted":
        vertices = vertices + torch.tensor(N.EVAL_SHIFT, device=gpu_device)
    gt = torch.from_numpy(N.sphere_gt_points()).to(gpu_device)
    pred, _ = sample_surface(vertices, faces, N.EVAL_SAMPLES, generator=torch.Generator().manual_seed(11))
    truth, dists = N.evaluate_f64(pred.cpu().numpy(), gt.cpu().numpy(), N.EVAL_THRESHOLDS)
    N.assert_thresholds_are_clear(dists, N.EVAL_THRESHOLDS, shape)
    got = evaluate_points(pred, gt, thresholds=N.EVAL_THRESHOLDS)
    for key in ("accuracy", "completeness", "chamfer"):
        err = abs(got[key] - truth[key]) / truth[key]
        print(f"{shape}: {key} {got[key]:.9g}, truth {truth[key]:.9g}, relative error {err:.2e} (bar 1e-6)")
        assert err <= 1e-6, (key, got[key], truth[key])
    assert got["n_pred"] == N.EVAL_SAMPLES and got["n_gt"] == N.EVAL_GT and got["dropped_pred"] == got["dropped_gt"] == 0.0
    assert len(got["thresholds"]) == len(N.EVAL_THRESHOLDS)
    for g, t in zip(got["thresholds"], truth["thresholds"]):
        print(f"{shape}: tau {t['tau']}: precision {g['precision']}, recall {g['recall']}, fscore {g['fscore']}")
        assert g["tau"] == t["tau"] and g["precision"] == t["precision"] and g["recall"] == t["recall"] and g["fscore"] == t["fscore"]
    # DTU's rule and the observation box, against the same truth
    md = 0.35
    truth_md, _ = N.evaluate_f64(pred.cpu().numpy(), gt.cpu().numpy(), (), max_dist=md)
    got_md = evaluate_points(pred, gt, max_dist=md)
    for key in ("accuracy", "completeness", "chamfer"):
        assert abs(got_md[key] - truth_md[key]) <= 1e-6 * truth_md[key], key
    assert got_md["dropped_pred"] == truth_md["dropped_pred"] and got_md["dropped_gt"] == truth_md["dropped_gt"]
    lo, hi = (0.0, 0.0, 0.0), (float(T.SPHERE_C[0]), 100.0, 100.0)
    p_np = pred.cpu().numpy()
    inside = ((p_np.astype(np.float64) >= lo) & (p_np.astype(np.float64) <= hi)).all(axis=1)
    truth_box, _ = N.evaluate_f64(p_np[inside], gt.cpu().numpy())
    got_box = evaluate_points(pred, gt, bounds=(lo, hi))
    assert got_box["n_pred"] == int(inside.sum()) < N.EVAL_SAMPLES
    assert abs(got_box["chamfer"] - truth_box["chamfer"]) <= 1e-6 * truth_box["chamfer"]
    # evaluate_mesh is sample_surface + evaluate_points
    again = evaluate_mesh(vertices, faces, gt, N.EVAL_SAMPLES, thresholds=N.EVAL_THRESHOLDS,
                          generator=torch.Generator().manual_seed(11))
    assert again["n_samples"] == N.EVAL_SAMPLES and {k: v for k, v in again.items() if k != "n_samples"} == got


# ---- distCUDA2 on the shared build ---------------------------------------------------------------------------------------------
# crc32 of the float32 bytes distCUDA2 returned on the parent of the commit that made the index build a shared step, on the
# MI355X, for four cases of knn_restate.  They are NOT the bits of knn_restate.dist2_knn3_f32_brute: knn.o is compiled with
# the compiler's default contraction, so the kernel forms dx*dx + dy*dy + dz*dz with two fused multiply-adds where numpy
# rounds every operation (on uniform_8193 659 of 8193 results differ in their last bits; the restatement's crc32 is
# 2108159095).  What is pinned is that the refactoring, and anything later, moves no bit of distCUDA2.
DIST2_PARENT_CRC32 = {"uniform_8193": 4134879569, "two_sheets_z": 314405474, "collapsed_cluster": 4226533935,
                      "lattice": 1690540240}


@pytest.mark.parametrize("case", sorted(DIST2_PARENT_CRC32))
def test_distCUDA2_kept_its_bits_on_the_shared_build(gpu_device, case):
    """distCUDA2 returns the bits it returned before its index build was shared with the cross-set query."""
    from mvs_gaussian_splatting_amd.knn import distCUDA2
    p = K.case_points(case)
    got = distCUDA2(torch.tensor(p).to(gpu_device)).cpu().numpy()
    K.assert_within_bound(got, K.case_truth(case), f"distCUDA2, {case}")
    diff = int((_bits(got) != _bits(K.dist2_knn3_f32_brute(p))).sum()) if case == "uniform_8193" else None
    print(f"distCUDA2 on {case}: crc32 {zlib.crc32(got.tobytes())}, recorded {DIST2_PARENT_CRC32[case]}"
          + (f"; {diff} of {len(got)} results differ from the unfused float32 restatement" if diff is not None else ""))
    assert zlib.crc32(got.tobytes()) == DIST2_PARENT_CRC32[case]
