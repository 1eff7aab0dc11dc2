"""distCUDA2 on the MI355X (mvs_gaussian_splatting_amd/knn.py, csrc/knn.hip) against the restatements of
tests/knn_restate.py, on the case table tests/test_knn_host.py proves well-posed (run on the GPU box: pytest -m gpu).

What runs: knn_bbox / knn_morton / the 30-bit pair sort / knn_boxes / knn_super / knn_query, through ``distCUDA2`` and through
``gsr_dist2_knn3`` itself.

Bars.  N >= 4: |got - f64| <= 8 * 2^-24 * f64 per point against the float64 truth (knn_restate.BOUND, derived there),
exactly 0 where the truth is 0.  N < 4: the bit pattern of the float32 restatement.  Repeat runs, permuted input and the
C entry with a workspace full of 0xFF or 0x00 bytes: bit-identical results.  The reference side of a value check is always
a restatement; a second run of the kernel is only ever compared for identity, on cases whose values are checked too.

Every distance is a symmetric expression evaluated in x, y, z order, keep3 keeps the three smallest VALUES whatever the
scan order, and the result is scattered by the original index: so a permutation of the input permutes the output, bit for
bit.  A wrong scatter index or a dependence on the scan order breaks that.
"""
import types

import numpy as np
import pytest
import torch

import knn_restate as K

pytestmark = pytest.mark.gpu

GSR_E_BADARG, GSR_E_CAPACITY, GSR_E_ALIGN = -1, -2, -3         # include/gsr.h
POISON_BYTE = 0xA5                                               # as a float: -2.9e-16, which no result can be
STRUCTURED = ["two_sheets_z", "lattice", "jittered_lattice", "collapsed_cluster", "uniform_8193"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dist2(points, dev):
    from mvs_gaussian_splatting_amd.knn import distCUDA2
    t = points if isinstance(points, torch.Tensor) else torch.tensor(points).to(dev)
    out = distCUDA2(t)
    assert out.dtype == torch.float32 and out.shape == (t.shape[0],) and out.device == t.device and not out.requires_grad
    return out.cpu().numpy()


# ---- values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.FULL_CASES)
def test_distCUDA2_is_within_the_float32_bound_of_float64(gpu_device, case):
    K.assert_within_bound(_dist2(K.case_points(case), gpu_device), K.case_truth(case), f"distCUDA2, {case}")


@pytest.mark.parametrize("case", K.SMALL_CASES)
def test_fewer_than_four_points_follow_the_contract(gpu_device, case):
    """+inf at N = 1, 2; (d1 + d2 + FLT_MAX) / 3 at N = 3: the float32 restatement, bit for bit."""
    want = K.dist2_knn3_f32_brute(K.case_points(case))
    got = _dist2(K.case_points(case), gpu_device)
    print(f"{case}: got {got}, contract {want}")
    assert np.array_equal(np.isinf(got), np.isinf(want)) and not np.isnan(got).any() and (got > 0).all()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isinf(want).all() if want.shape[0] < 3 else np.isfinite(want).all()


# ---- identity: repeat runs and permuted input ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STRUCTURED)
def test_repeat_and_permuted_runs_are_bit_identical(gpu_device, case):
    p = K.case_points(case)
    n = p.shape[0]
    first = _dist2(p, gpu_device)
    K.assert_within_bound(first, K.case_truth(case), f"distCUDA2, {case}")
    assert np.array_equal(_bits(_dist2(p, gpu_device)), _bits(first)), "a repeat run differs"
    for what, perm in (("random", np.random.default_rng(n).permutation(n)), ("reversed", np.arange(n)[::-1])):
        got = _dist2(p[perm], gpu_device)
        diff = np.flatnonzero(_bits(got) != _bits(first[perm]))
        assert diff.size == 0, (f"{what} permutation: {diff.size} results differ, first at permuted index {diff[0]}: "
                                f"{got[diff[0]]!r} against {first[perm][diff[0]]!r}")


# ---- the C entry ---------------------------------------------------------------------------------------------------------
def _poisoned(nbytes, dev, byte=POISON_BYTE):
    return torch.empty(nbytes, dtype=torch.uint8, device=dev).fill_(byte)


def _c_knn(dev, pts, n, out, ws_ptr, ws_bytes):
    from mvs_gaussian_splatting_amd import _lib
    with torch.cuda.device(dev):
        rc = _lib.load().gsr_dist2_knn3(pts.data_ptr(), n, out.data_ptr(), ws_ptr, ws_bytes,
                                        torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_c_entry_does_not_depend_on_what_the_workspace_holds(gpu_device, fill):
    """gsr_dist2_knn3 at N = 8193 with every workspace byte preset: the min / max words of the cloud's extent are
    initialised by the entry itself, nothing else is read before it is written.  Every output element is overwritten."""
    from mvs_gaussian_splatting_amd import _lib
    p = K.case_points("uniform_8193")
    n = p.shape[0]
    want = _dist2(p, gpu_device)
    K.assert_within_bound(want, K.case_truth("uniform_8193"), "distCUDA2, uniform_8193")
    nbytes = _lib.load().gsr_knn3_workspace_bytes(n)
    pts = torch.tensor(p).to(gpu_device)
    ws, out = _poisoned(nbytes, gpu_device, fill), _poisoned(4 * n, gpu_device).view(torch.float32)
    assert ws.data_ptr() % 256 == 0 and (out.cpu().numpy() < 0).all()
    assert _c_knn(gpu_device, pts, n, out, ws.data_ptr(), nbytes) == 0
    got = out.cpu().numpy()
    assert (got >= 0).all(), f"{int((got < 0).sum())} output elements still hold the poison"
    assert np.array_equal(_bits(got), _bits(want))


def test_c_entry_refuses_bad_arguments_and_touches_nothing(gpu_device):
    from mvs_gaussian_splatting_amd import _lib
    p = K.case_points("uniform_8193")
    n = p.shape[0]
    nbytes = _lib.load().gsr_knn3_workspace_bytes(n)
    assert nbytes > 0 and nbytes % 256 == 0
    pts = torch.tensor(p).to(gpu_device)
    ws, out = _poisoned(nbytes + 256, gpu_device), _poisoned(4 * n, gpu_device).view(torch.float32)
    assert ws.data_ptr() % 256 == 0

    def untouched():
        return bool((out.view(torch.uint8) == POISON_BYTE).all()) and bool((ws == POISON_BYTE).all())

    assert _c_knn(gpu_device, pts, 0, out, ws.data_ptr(), nbytes) == 0 and untouched()            # N = 0: success, no work
    assert _c_knn(gpu_device, pts, -1, out, ws.data_ptr(), nbytes) == GSR_E_BADARG and untouched()
    assert _c_knn(gpu_device, pts, n, out, ws.data_ptr(), nbytes - 1) == GSR_E_CAPACITY and untouched()
    assert b"workspace" in _lib.load().gsr_last_error()
    assert _c_knn(gpu_device, pts, n, out, ws.data_ptr() + 128, nbytes) == GSR_E_ALIGN and untouched()
    assert _c_knn(gpu_device, pts, n, out, None, nbytes) == GSR_E_BADARG and untouched()


# ---- the wrapper's input forms ---------------------------------------------------------------------------------------------
def test_wrapper_takes_views_float64_grad_tensors_and_side_streams(gpu_device):
    p = K.case_points("uniform_257")
    truth = K.case_truth("uniform_257")
    want = _dist2(p, gpu_device)
    K.assert_within_bound(want, truth, "distCUDA2, uniform_257")
    # a [3, N].T view: not contiguous
    view = torch.from_numpy(np.ascontiguousarray(p.T)).to(gpu_device).T
    assert view.shape == (257, 3) and not view.is_contiguous()
    assert np.array_equal(_bits(_dist2(view, gpu_device)), _bits(want))
    # requires_grad: the result is detached
    leaf = torch.tensor(p).to(gpu_device).requires_grad_(True)
    assert np.array_equal(_bits(_dist2(leaf, gpu_device)), _bits(want))
    # a non-default stream: the input is ready before the side stream starts, the result is read after it ends
    side = torch.cuda.Stream(device=gpu_device)
    ready = torch.tensor(p).to(gpu_device)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        from mvs_gaussian_splatting_amd.knn import distCUDA2
        on_side = distCUDA2(ready)
    side.synchronize()
    assert np.array_equal(_bits(on_side.cpu().numpy()), _bits(want))
    # float64 input is rounded to float32 first: the truth is that of the rounded coordinates
    p64 = np.random.default_rng(64).random((257, 3)) * [4.0, 2.0, 1.0] - 1.0
    assert not np.array_equal(p64.astype(np.float32).astype(np.float64), p64)
    got = _dist2(torch.from_numpy(p64).to(gpu_device), gpu_device)
    K.assert_within_bound(got, K.dist2_knn3_f64(p64.astype(np.float32)), "distCUDA2, float64 input")


def test_wrapper_edge_shapes_and_refusals(gpu_device):
    from mvs_gaussian_splatting_amd import _lib
    from mvs_gaussian_splatting_amd.knn import distCUDA2
    empty = distCUDA2(torch.empty(0, 3, device=gpu_device))
    assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.is_cuda
    with pytest.raises(ValueError):
        distCUDA2(torch.zeros(5, 2, device=gpu_device))
    with pytest.raises(ValueError):
        distCUDA2(torch.zeros(6, device=gpu_device))
    with pytest.raises(_lib.GsrError):
        distCUDA2(torch.zeros(5, 3))


# ---- create_from_pcd on the real k-NN -------------------------------------------------------------------------------------
def _scaling_close(got, want, what):
    """test_gpu_model.py's bar for computed rows: |got - want| <= 1e-6 max(|want|, 1).  The 8 * 2^-24 of the distance
    becomes 4 * 2^-24 = 2.4e-7 absolute under log(sqrt(.)); sqrt and log add a few 2^-24 relative to |want|."""
    err = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
    print(f"{what}: max error {err:.3e} (bar 1e-6)")
    assert got.shape == want.shape and err <= 1e-6, (what, err)


def test_create_from_pcd_on_five_points(gpu_device):
    from mvs_gaussian_splatting_amd import GaussianModel
    p = K.case_points("uniform_5")
    m = GaussianModel(3).create_from_pcd(types.SimpleNamespace(points=p, colors=np.full((5, 3), 0.5, np.float32)), 1.0,
                                         device=gpu_device)
    ref = torch.tensor(K.case_truth("uniform_5")).clamp_min(1e-7)
    assert (ref > 1e-7).all()
    want = torch.log(torch.sqrt(ref)).float()[:, None].repeat(1, 3)
    assert torch.isfinite(m._scaling).all()
    _scaling_close(m._scaling.detach().cpu(), want, "scaling of 5 points")


def test_create_from_pcd_on_three_points_pins_the_contract(gpu_device):
    """Three points have no third neighbour: distCUDA2 gives FLT_MAX / 3 and create_from_pcd takes log(sqrt(.)) of it, a
    log-scale of 43.8 on every axis of every Gaussian: finite, and far too large to be of use.  This pins what happens;
    what ought to happen to clouds this small is model.py's to decide."""
    from mvs_gaussian_splatting_amd import GaussianModel
    p = K.case_points("uniform_3")
    m = GaussianModel(3).create_from_pcd(types.SimpleNamespace(points=p, colors=np.full((3, 3), 0.5, np.float32)), 1.0,
                                         device=gpu_device)
    d2 = torch.from_numpy(K.dist2_knn3_f32_brute(p))
    assert torch.isfinite(d2).all()
    want = torch.log(torch.sqrt(d2.double())).float()[:, None].repeat(1, 3)
    assert abs(float(want[0, 0]) - 43.81) < 0.01
    assert torch.isfinite(m._scaling).all()
    _scaling_close(m._scaling.detach().cpu(), want, "scaling of 3 points")
