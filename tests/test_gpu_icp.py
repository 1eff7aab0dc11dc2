"""The registration layer on the MI355X (mvs_gaussian_splatting_amd/geometry_eval.py; csrc/icp.hip; the down-sampler on the
kernels of csrc/mesh_simplify.hip) against the restatement of tests/icp_restate.py, whose own conditions
tests/test_icp_host.py checks without a GPU (run on the GPU box: pytest -m gpu).

Bars.  ``transform_points`` gives the restatement's float32 bits.  ``icp_step`` gives the restatement's count, and each of
its 17 sums lies within ``(n + 8) 2^-53 sum |term|`` of the ``math.fsum`` value (derived in icp_restate's docstring: both
sides add the same float64 terms, in different orders); two runs, and a run on a workspace full of 0xFF bytes, give the
same bits.  ``icp_registration`` makes the restatement's iterations to the restatement's fitness and ends within 4x the
restatement's own distance from the truth.  ``voxel_down_sample`` gives the restatement's bits in its row order.  The
example script without the new flags writes the bytes recorded from the commit before them (tests/golden/).
"""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import ROOT
import icp_restate as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
BLOCK, MAX_BLOCKS, FINISH_TRIP = 256, 1024, 256            # csrc/icp.hip


def _dev(a, dev, dtype=None):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- transform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 257])
def test_transform_gives_the_restatements_bits(gpu_device, Q):
    from mvs_gaussian_splatting_amd import transform_points
    for offset in (0.0, 1e4):
        src = R.asymmetric_cloud(400, offset=offset)[:Q]
        T = R.about(R.similarity([3.0, -2.0, 1.0], [0.05, -0.02, 0.01], 1.02), [offset + 2, offset + 1, offset + 0.5])
        got = transform_points(_dev(src, gpu_device), T)
        assert got.dtype == torch.float32 and got.shape == (Q, 3) and got.is_cuda
        assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(R.transform(src, T))), (Q, offset)


def test_transform_takes_strided_and_float64_input_and_tensor_matrices(gpu_device):
    from mvs_gaussian_splatting_amd import transform_points
    src = R.asymmetric_cloud(400, offset=1e4)
    T = R.about(R.similarity([3.0, -2.0, 1.0], [0.05, -0.02, 0.01], 1.02), [1e4, 1e4, 1e4])
    want = _bits32(R.transform(src, T))
    wide = torch.zeros((400, 7), dtype=torch.float64, device=gpu_device)
    wide[:, 1:6:2] = _dev(src, gpu_device).double()
    view = wide[:, 1:6:2]
    assert not view.is_contiguous()
    keep = view.clone()
    for points, matrix in ((view, T), (view.float(), torch.tensor(T)), (view, T.tolist())):
        assert np.array_equal(_bits32(transform_points(points, matrix).cpu().numpy()), want)
    assert torch.equal(view, keep), "the input is not written"
    jitter = src.astype(np.float64) + 1e-5                  # float64 input is rounded to float32 first
    got = transform_points(_dev(jitter, gpu_device), T)
    assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(R.transform(jitter.astype(np.float32), T)))


# ---- accumulate / icp_step -----------------------------------------------------------------------------------------------------
def _c_accumulate(dev, q, dist2, nearest, target, t2, cq, cr, fill=None):
    """gsr_icp_accumulate on buffers of the caller's, the workspace and the result pre-filled with `fill` bytes."""
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    Q, Rn = len(q), len(target)
    tq, td, tn, tt = _dev(q, dev, torch.float32), _dev(dist2, dev, torch.float32), _dev(nearest, dev, torch.int32), \
        _dev(np.asarray(target, dtype=np.float32).reshape(-1, 3), dev, torch.float32)
    wb = lib.gsr_icp_workspace_bytes(Q)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev) if fill is None else torch.full((wb,), fill, dtype=torch.uint8, device=dev)
    out = torch.full((18,), -1, dtype=torch.int64, device=dev)
    piv = np.concatenate([np.asarray(cq, dtype=np.float64), np.asarray(cr, dtype=np.float64)])
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev).cuda_stream
        assert lib.gsr_icp_accumulate(tq.data_ptr(), td.data_ptr(), tn.data_ptr(), Q, tt.data_ptr(), Rn, float(t2),
                                      piv.ctypes.data, ws.data_ptr(), wb, out.data_ptr(), s) == 0
        torch.cuda.synchronize()
    words = out.cpu().numpy()
    return int(words[0]), words[1:].view(np.float64).copy()


def _flat(sums):
    return np.concatenate([sums.sum_a, sums.sum_b, sums.sum_ab.reshape(-1), [sums.sum_aa, sums.sum_d2]])


def _assert_within_bound(count, got, st, what):
    assert count == st.count, (what, count, st.count)
    err = np.abs(got - st.sums)
    print(f"{what}: n = {st.count}, largest error / bound = {np.max(err / np.maximum(st.bound, 1e-300)):.3f}")
    bad = np.flatnonzero(~(err <= st.bound))
    assert bad.size == 0, f"{what}: sum {bad[0]} is {err[bad[0]]:.3e} off, the bound is {st.bound[bad[0]]:.3e}"


# one wave and one past it; one workgroup's share and one past it; one past the partials the finish reads in one trip;
# one past the points the capped grid takes in one trip of the lane loop
STEP_SIZES = [(1, 40), (64, 300), (65, 300), (BLOCK, 300), (BLOCK + 1, 300), (BLOCK * FINISH_TRIP + 1, 300),
              (BLOCK * MAX_BLOCKS + 1, 64)]


@pytest.mark.parametrize("Q,Rn", STEP_SIZES)
def test_icp_step_matches_the_restatement(gpu_device, Q, Rn):
    from mvs_gaussian_splatting_amd.geometry_eval import IcpTarget, NearestIndex, icp_step
    rng = np.random.default_rng([Q, Rn])
    tgt = (rng.random((Rn, 3)) * [4.0, 2.0, 1.0]).astype(np.float32)
    src = (rng.random((Q, 3)) * [4.0, 2.0, 1.0]).astype(np.float32)
    T = R.about(R.similarity([3.0, -2.0, 1.0], [0.05, -0.02, 0.01], 1.02), [2.0, 1.0, 0.5])
    max_dist = 0.2 if Rn >= 300 else 0.35
    piv = (np.array([2.1, 0.9, 0.6]), np.array([1.9, 1.1, 0.4]))
    st = R.step(src, tgt, T, max_dist, piv)
    if Q >= 64:
        assert 0.15 * Q < st.count < 0.85 * Q, "both sides of the threshold are exercised"
    s, t = _dev(src, gpu_device), _dev(tgt, gpu_device)
    target = IcpTarget(t)
    first = icp_step(s, target, T, max_dist, pivots=piv)
    assert first.num_source == Q and np.array_equal(first.pivot_q, piv[0]) and np.array_equal(first.pivot_r, piv[1])
    _assert_within_bound(first.count, _flat(first), st, f"icp_step, Q = {Q}")
    assert first.fitness == st.count / Q
    for way in (target, (NearestIndex(t), t), t):                               # every form of a target, and a second run
        again = icp_step(s, way, T, max_dist, pivots=piv)
        assert again.count == first.count and np.array_equal(_flat(again).view(np.uint64), _flat(first).view(np.uint64))
    for fill in (None, 0xFF, 0x00):                                             # the entry point on the restatement's pairs
        count, sums = _c_accumulate(gpu_device, st.q, st.dist2, st.nearest, tgt, R.thr2(max_dist), *piv, fill=fill)
        assert count == first.count and np.array_equal(sums.view(np.uint64), _flat(first).view(np.uint64)), fill


def test_every_pair_rejected_and_an_empty_target_give_zero(gpu_device):
    from mvs_gaussian_splatting_amd.geometry_eval import icp_step
    src = R.asymmetric_cloud(700)
    tgt = R.asymmetric_cloud(500, seed=8) + np.float32(50.0)
    for target in (_dev(tgt, gpu_device), torch.empty((0, 3), device=gpu_device)):
        got = icp_step(_dev(src, gpu_device), target, np.eye(4), 0.3, pivots=((1, 2, 3), (4, 5, 6)))
        assert got.count == 0 and got.fitness == 0.0 and got.inlier_rmse == 0.0
        assert np.array_equal(_flat(got).view(np.uint64), np.zeros(17, dtype=np.uint64)), "the sums are +0.0"
    empty = icp_step(torch.empty((0, 3), device=gpu_device), _dev(tgt, gpu_device), np.eye(4), 0.3)
    assert empty.count == 0 and empty.num_source == 0 and not _flat(empty).any()
    # an answer of -1 (or any index outside the target) is not accepted whatever its distance
    q = src[:300]
    nearest = np.full(300, -1, dtype=np.int32)
    nearest[::7] = 500
    count, sums = _c_accumulate(gpu_device, q, np.zeros(300, dtype=np.float32), nearest, tgt, np.inf, (0, 0, 0), (0, 0, 0), 0xFF)
    assert count == 0 and not sums.any()


def test_a_pair_at_the_threshold_exactly_is_accepted(gpu_device):
    from mvs_gaussian_splatting_amd.geometry_eval import icp_step
    t2 = np.float32(0.25)
    above, below = np.nextafter(t2, np.float32(1)), np.nextafter(t2, np.float32(0))
    q = np.float32([[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0]])
    tgt = q + np.float32([0.5, 0, 0])
    dist2 = np.array([t2, above, below, np.nan], dtype=np.float32)
    count, sums = _c_accumulate(gpu_device, q, dist2, np.arange(4, dtype=np.int32), tgt, t2, (0, 0, 0), (0, 0, 0))
    assert count == 2 and sums[0] == 20.0 and sums[3] == 21.0 and sums[16] == float(t2) + float(below)
    # and through the query: |dx| = 0.5 squares to 0.25 = float32(0.5^2) exactly
    got = icp_step(_dev(q, gpu_device), _dev(tgt, gpu_device), np.eye(4), 0.5)
    assert got.count == 4 and got.sum_d2 == 1.0 and got.inlier_rmse == 0.5
    assert icp_step(_dev(q, gpu_device), _dev(tgt, gpu_device), np.eye(4), float(np.nextafter(np.float32(0.5), np.float32(0)))).count == 0


def test_pivots_keep_the_digits_of_a_cloud_far_from_the_origin(gpu_device):
    """The 1e4-offset cloud about its correspondence centroids: the bound there is 1e-10 absolute, which the sums about
    zero pivots cannot meet (tests/test_icp_host.py: test_zero_pivots_would_miss_the_bound_on_the_offset_cloud)."""
    from mvs_gaussian_splatting_amd.geometry_eval import icp_step
    src = R.asymmetric_cloud(2000, offset=1e4)
    tgt = R.asymmetric_cloud(2000, seed=8, offset=1e4)
    zero = R.step(src, tgt, np.eye(4), 0.3)
    cq = zero.q[zero.accepted].astype(np.float64).mean(axis=0)
    cr = tgt[zero.nearest[zero.accepted]].astype(np.float64).mean(axis=0)
    st = R.step(src, tgt, np.eye(4), 0.3, (cq, cr))
    got = icp_step(_dev(src, gpu_device), _dev(tgt, gpu_device), np.eye(4), 0.3, pivots=(cq, cr))
    _assert_within_bound(got.count, _flat(got), st, "offset cloud, pivots at the centroids")
    assert st.bound[6:15].max() < 1e-9
    from_zero = icp_step(_dev(src, gpu_device), _dev(tgt, gpu_device), np.eye(4), 0.3)
    _assert_within_bound(from_zero.count, _flat(from_zero), zero, "offset cloud, zero pivots (its own, far wider bound)")


# ---- registration ------------------------------------------------------------------------------------------------------------
def test_icp_registration_follows_the_restatement_onto_the_known_similarity(gpu_device):
    from mvs_gaussian_splatting_amd.geometry_eval import IcpTarget, icp_registration
    src, tgt, T, max_dist = R.registration_case(True)
    want = R.registration_restated(True)
    got = icp_registration(_dev(src, gpu_device), IcpTarget(_dev(tgt, gpu_device)), max_dist, with_scaling=True)
    err, ref = R.max_point_error(got.transformation, T, src), R.max_point_error(want.transformation, T, src)
    print(f"ICP: {got.iterations} iterations (restated {want.iterations}), fitness {got.fitness}, max point error {err:.3e} "
          f"(restated {ref:.3e})")
    assert got.converged and want.converged and got.iterations == want.iterations and got.fitness == want.fitness
    assert err <= 4.0 * ref
    assert got.transformation.dtype == np.float64 and np.array_equal(got.transformation[3], [0, 0, 0, 1])
    assert abs(got.inlier_rmse - want.inlier_rmse) <= 1e-6 * max(want.inlier_rmse, 1e-12) + 1e-12
    # from an init that is the answer nothing moves: one update at most, then the stop
    again = icp_registration(_dev(src, gpu_device), _dev(tgt, gpu_device), max_dist, init=got.transformation, with_scaling=True)
    assert again.converged and again.iterations == 1 and R.max_point_error(again.transformation, T, src) <= 4.0 * ref


def test_without_scaling_rigid_data_keeps_the_scale_at_one(gpu_device):
    """The update of a rigid step is R | t with the rotation of the SVD applied as it is -- no factor is formed -- so the
    cumulative matrix is a product of `iterations` rotations, each orthonormal to a few 2^-53: its determinant is 1 to
    that rounding, where an estimated scale would sit 1e-9 off (the size of the data's float32 noise)."""
    from mvs_gaussian_splatting_amd.geometry_eval import icp_registration
    src, tgt, T, max_dist = R.registration_case(False)
    want = R.registration_restated(False)
    got = icp_registration(_dev(src, gpu_device), _dev(tgt, gpu_device), max_dist)
    A = got.transformation[:3, :3]
    assert got.converged and got.iterations == want.iterations and got.fitness == want.fitness == 1.0
    assert abs(np.cbrt(np.linalg.det(A)) - 1.0) <= 16 * got.iterations * 2.0 ** -53
    assert np.abs(A @ A.T - np.eye(3)).max() <= 16 * got.iterations * 2.0 ** -53
    assert R.max_point_error(got.transformation, T, src) <= 4.0 * R.max_point_error(want.transformation, T, src)


def test_too_few_pairs_end_the_loop_unconverged_with_the_transformation_unchanged(gpu_device):
    from mvs_gaussian_splatting_amd.geometry_eval import icp_registration
    src, tgt, _, _ = R.registration_case(True)
    init = R.similarity([0.0, 0.0, 0.0], [100.0, 0.0, 0.0], 1.0)
    got = icp_registration(_dev(src, gpu_device), _dev(tgt, gpu_device), 0.05, init=init)
    assert not got.converged and got.iterations == 0 and got.fitness == 0.0 and np.array_equal(got.transformation, init)
    got = icp_registration(_dev(src, gpu_device), torch.empty((0, 3), device=gpu_device), 0.05)
    assert not got.converged and got.iterations == 0 and np.array_equal(got.transformation, np.eye(4))


# ---- voxel down-sampling -----------------------------------------------------------------------------------------------------
def test_voxel_down_sample_gives_the_restatements_bits_and_row_order(gpu_device):
    from mvs_gaussian_splatting_amd import _lib, voxel_down_sample
    rng = np.random.default_rng(3)
    cloud = R.asymmetric_cloud(2000)
    faces = (rng.integers(-8, 8, size=(300, 3)) * 0.25).astype(np.float32)              # every coordinate on a cell face
    signed = np.float32([[-0.0, 1.5, 2.0]])
    for what, pts, h, origin in (("cloud", cloud, 0.3, None), ("fine", cloud, 0.05, None), ("one cell", cloud, 100.0, None),
                                 ("one point", cloud[:1], 0.3, None), ("cell faces", faces, 0.25, (-2.0, -2.0, -2.0)),
                                 ("given origin", cloud, 0.3, (-1.0, -2.0, -3.0)), ("minus zero", signed, 1.0, None),
                                 ("far", R.asymmetric_cloud(2000, offset=1e4), 0.3, None)):
        want, _ = R.voxel_down_sample(pts, h, origin)
        got = voxel_down_sample(_dev(pts, gpu_device), h, origin=origin)
        assert got.dtype == torch.float32 and got.is_cuda and got.shape == want.shape, (what, got.shape, want.shape)
        assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(want)), what
    assert voxel_down_sample(_dev(cloud, gpu_device), 100.0).shape == (1, 3)
    assert voxel_down_sample(torch.empty((0, 3), device=gpu_device), 0.5).shape == (0, 3)
    wide = torch.zeros((2000, 5), dtype=torch.float64, device=gpu_device)
    wide[:, ::2] = _dev(cloud, gpu_device).double()
    got = voxel_down_sample(wide[:, ::2], 0.3)
    assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(R.voxel_down_sample(cloud, 0.3)[0]))
    with pytest.raises(_lib.GsrError, match="too small"):
        voxel_down_sample(_dev(cloud, gpu_device), 1e-7)
    bad = cloud.copy()
    bad[5, 1] = np.inf
    with pytest.raises(_lib.GsrError, match="not finite"):
        voxel_down_sample(_dev(bad, gpu_device), 0.3)


# ---- evaluate_points, register_tnt, the example ---------------------------------------------------------------------------------
def _golden_pair(dev):
    from mvs_gaussian_splatting_amd.ply_io import read_ply_mesh, read_ply_vertices
    vertices, faces, _ = read_ply_mesh(os.path.join(GOLDEN, "eval_mesh_mesh.ply"))
    gt, _ = read_ply_vertices(os.path.join(GOLDEN, "eval_mesh_gt.ply"))
    gt = np.stack([np.asarray(gt[n], dtype=np.float32) for n in ("x", "y", "z")], axis=1)
    return _dev(vertices, dev), _dev(faces, dev), _dev(gt, dev)


def test_evaluate_points_without_down_sample_returns_what_it_always_did(gpu_device, monkeypatch):
    from mvs_gaussian_splatting_amd import geometry_eval as G
    with open(os.path.join(GOLDEN, "eval_mesh_results.json")) as f:
        recorded = json.load(f)
    vertices, faces, gt = _golden_pair(gpu_device)
    pred, _ = G.sample_surface(vertices, faces, 3000, torch.Generator(device="cpu").manual_seed(3))
    real = G.voxel_down_sample
    monkeypatch.setattr(G, "voxel_down_sample", lambda *a, **kw: pytest.fail("down-sampled without being asked"))
    for res in (G.evaluate_points(pred, gt, (0.05, 0.2), 0.5), G.evaluate_points(pred, gt, (0.05, 0.2), 0.5, down_sample=None)):
        assert list(res) == [k for k in recorded if k in res] and "down_sample" not in res
        assert all(res[k] == recorded[k] for k in res), "a value differs from the one recorded before the feature"
    monkeypatch.setattr(G, "voxel_down_sample", real)
    coarse = G.evaluate_points(pred, gt, (0.05, 0.2), 0.5, down_sample=0.1)
    p, g = (R.voxel_down_sample(x.cpu().numpy(), 0.1)[0] for x in (pred, gt))
    assert coarse["n_pred"] == len(p) < 3000 and coarse["n_gt"] == len(g) < 400
    assert coarse == G.evaluate_points(_dev(p, gpu_device), _dev(g, gpu_device), (0.05, 0.2), 0.5)


def test_register_tnt_returns_the_fscore_of_the_unperturbed_pair(gpu_device):
    """3000 predicted points: 2400 of the ground truth's own and 600 outliers above it, which the crop volume keeps out of
    the registration (and which stay in the score).  Moved by the inverse of a known similarity, registered from the
    identity, moved back by the result: the score is the unperturbed pair's."""
    from mvs_gaussian_splatting_amd.geometry_eval import CropVolume, evaluate_points, register_tnt, transform_points
    rng = np.random.default_rng(12)
    gt = R.asymmetric_cloud(3000)
    outliers = (rng.random((600, 3)) * [4.0, 2.0, 0.5] + [0.0, 0.0, 6.0]).astype(np.float32)
    pred0 = np.concatenate([gt[:2400], outliers])
    c = gt.astype(np.float64).mean(axis=0)
    T = R.about(R.similarity([1.2, -2.0, 1.9], [0.05, 0.06, -0.04], 1.02), c)
    pred = R.transform(pred0, np.linalg.inv(T))
    crop = CropVolume(2, -1.0, 3.0, np.array([[-1.0, -1.0, 0], [5.0, -1.0, 0], [5.0, 3.0, 0], [-1.0, 3.0, 0]]))
    dtau = 0.02
    reg = register_tnt(_dev(pred, gpu_device), _dev(gt, gpu_device), np.eye(4), crop, dtau)
    err = R.max_point_error(reg.transformation, T, pred[:2400])
    print(f"register_tnt: {reg.iterations} iterations, fitness {reg.fitness:.4f}, max point error {err:.3e}")
    assert reg.converged and reg.fitness == 1.0 and err <= 1e-5 * R.extent(gt)
    taus = (dtau, 5 * dtau)
    want = evaluate_points(_dev(pred0, gpu_device), _dev(gt, gpu_device), taus)
    got = evaluate_points(transform_points(_dev(pred, gpu_device), reg.transformation), _dev(gt, gpu_device), taus)
    assert want["thresholds"][0]["precision"] == 0.8 and 0.8 <= want["thresholds"][0]["recall"] < 1.0
    assert got["thresholds"] == want["thresholds"]
    before = evaluate_points(_dev(pred, gpu_device), _dev(gt, gpu_device), taus)
    assert before["thresholds"][0]["fscore"] < 0.2 < want["thresholds"][0]["fscore"], "the perturbation mattered"


def _example():
    spec = importlib.util.spec_from_file_location("example_eval_mesh", os.path.join(ROOT, "examples", "eval_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_without_the_new_flags_writes_the_recorded_bytes(gpu_device, tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("make_golden_eval_mesh", os.path.join(GOLDEN, "make_golden_eval_mesh.py"))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    mesh, gt = (shutil.copy(os.path.join(GOLDEN, n), str(tmp_path)) for n in ("eval_mesh_mesh.ply", "eval_mesh_gt.ply"))
    _example().main(["--mesh", mesh, "--gt", gt] + maker.ARGS)
    with open(str(tmp_path / "results_mesh.json"), "rb") as f:
        raw = f.read()
    with open(os.path.join(GOLDEN, "eval_mesh_results.json"), "rb") as f:
        want = f.read()
    for path, tag in ((mesh, "@MESH@"), (gt, "@GT@")):
        want = want.replace(json.dumps(tag).encode(), json.dumps(os.path.abspath(path)).encode())
    assert raw == want


def test_example_with_the_new_flags_reports_the_registration(gpu_device, tmp_path, capsys):
    mesh, gt = (shutil.copy(os.path.join(GOLDEN, n), str(tmp_path)) for n in ("eval_mesh_mesh.ply", "eval_mesh_gt.ply"))
    align = str(tmp_path / "T.txt")
    T = R.similarity([0.0, 0.0, 2.0], [0.02, -0.01, 0.01], 1.0)
    np.savetxt(align, T)
    crop = str(tmp_path / "crop.json")
    with open(crop, "w") as f:
        json.dump({"orthogonal_axis": "Z", "axis_min": -2.0, "axis_max": 2.0,
                   "bounding_polygon": [[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]]}, f)
    mod = _example()
    res = mod.main(["--mesh", mesh, "--gt", gt, "--samples", "3000", "--tau", "0.05", "0.2", "--seed", "3", "--align", align,
                    "--crop", crop, "--icp", "--dtau", "0.05", "--down_sample", "0.025"])
    with open(str(tmp_path / "results_mesh.json")) as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(res))
    assert np.array(saved["transformation"]).shape == (4, 4) and saved["transformation"][3] == [0.0, 0.0, 0.0, 1.0]
    assert 0.0 < saved["icp"]["fitness"] <= 1.0 and saved["icp"]["inlier_rmse"] > 0.0 and saved["icp"]["iterations"] >= 1
    assert saved["n_pred"] < 3000 and saved["down_sample"] == 0.025 and saved["crop"] == crop and saved["align"] == align
    with pytest.raises(SystemExit):
        mod.main(["--mesh", mesh, "--gt", gt, "--icp"])
