"""Mesh simplification on the HIP path (csrc/mesh_simplify.hip; ``mesh.simplify_mesh``) against the
sequential restatement of tests/mesh_simplify_restate.py.

Everything but the means is integers and is compared exactly: ``faces`` and ``vertex_cluster`` integer for integer.  The
means: both sides round to float32 a float64 sum of float32 values whose own error is far below half a float32 ulp for runs
shorter than 2^24, but may add in a different order, so they can differ by at most one float32 spacing at the magnitude of
the largest member: ``|got - want| <= 2^-23 max_i |x_i|`` per cluster and component.  A cluster of one member is a
bit-copy.  Each case runs twice (the same bits) and leaves its inputs alone.  The cases are the smallest at which the
kernels can go wrong; tests/test_mesh_simplify_host.py checks that they have the shapes they are there for."""
import math

import numpy as np
import pytest
import torch

import mesh_simplify_restate as R

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view(torch.int32)


def _run(case, dev, colors=True, **kw):
    from mvs_gaussian_splatting_amd import simplify_mesh
    tv, tf = torch.from_numpy(case["vertices"]).to(dev), torch.from_numpy(case["faces"]).to(dev)
    tc = torch.from_numpy(case["colors"]).to(dev) if colors else None
    kw.setdefault("voxel_size", case["voxel_size"])
    kw.setdefault("origin", case["origin"])
    return simplify_mesh(tv, tf, tc, return_map=True, **kw), (tv, tf, tc)


def _within(got, want, max_abs, what):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 2.0 ** -23 * max_abs
    worst = float((err - bound).max()) if err.size else 0.0
    print(f"{what}: max |got - want| = {float(err.max()) if err.size else 0.0:.3e}, largest bound {float(bound.max()) if err.size else 0.0:.3e}")
    assert np.all(err <= bound), f"{what}: {worst:.3e} beyond 2^-23 max|x_i|"


@pytest.mark.parametrize("name", R.CASES)
def test_case_matches_the_restatement_twice_and_leaves_its_inputs_alone(gpu_device, name):
    case, want = R.cases()[name], R.reference(name)
    (v, f, c, m), (tv, tf, tc) = _run(case, gpu_device)
    keep = tv.clone(), tf.clone(), tc.clone()
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and c.dtype == torch.float32 and m.dtype == torch.int32
    assert v.is_cuda and f.is_cuda and c.is_cuda and m.is_cuda
    assert tuple(v.shape) == want.vertices.shape and tuple(f.shape) == want.faces.shape, "V' or F' differs"
    assert tuple(c.shape) == want.colors.shape and tuple(m.shape) == want.vertex_cluster.shape
    assert v.shape[1] == 3 and f.shape[1] == 3
    assert np.array_equal(f.cpu().numpy(), want.faces), "faces differ from the restatement"
    assert np.array_equal(m.cpu().numpy(), want.vertex_cluster), "vertex_cluster differs from the restatement"
    got_v, got_c = v.cpu().numpy(), c.cpu().numpy()
    if len(want.vertices):
        _within(got_v, want.vertices, want.max_abs, f"{name} positions")
        _within(got_c, want.colors, want.max_abs_colors, f"{name} colours")
        alone = np.array([len(g) == 1 for g in want.members])
        first = np.array([g[0] for g in want.members])
        assert np.array_equal(got_v[alone].view(np.int32), case["vertices"][first[alone]].view(np.int32)), \
            "a cluster of one member is not a bit-copy"
        assert np.array_equal(got_c[alone].view(np.int32), case["colors"][first[alone]].view(np.int32))
    if name == "identity_small_h":
        assert np.array_equal(got_v.view(np.int32), want.vertices.view(np.int32))
        assert np.array_equal(got_c.view(np.int32), want.colors.view(np.int32))
    if name == "one_cell_fan_65":
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(c.shape) == (0, 3) and bool((m == -1).all())
    (v2, f2, c2, m2), _ = _run(case, gpu_device)
    assert torch.equal(_bits(v), _bits(v2)) and torch.equal(f, f2) and torch.equal(_bits(c), _bits(c2)) and torch.equal(m, m2), \
        "not the same bits from run to run"
    assert torch.equal(_bits(tv), _bits(keep[0])) and torch.equal(tf, keep[1]) and torch.equal(_bits(tc), _bits(keep[2])), \
        "an input was written"


def test_return_map_false_returns_three_values_and_no_colors_returns_none(gpu_device):
    from mvs_gaussian_splatting_amd import simplify_mesh
    case, want = R.cases()["sphere_tsdf"], R.reference("sphere_tsdf")
    tv, tf = torch.from_numpy(case["vertices"]).to(gpu_device), torch.from_numpy(case["faces"]).to(gpu_device)
    tc = torch.from_numpy(case["colors"]).to(gpu_device)
    (v, f, c, m), _ = _run(case, gpu_device)
    out = simplify_mesh(tv, tf, tc, voxel_size=case["voxel_size"], origin=case["origin"])
    assert isinstance(out, tuple) and len(out) == 3
    assert torch.equal(_bits(out[0]), _bits(v)) and torch.equal(out[1], f) and torch.equal(_bits(out[2]), _bits(c))
    out = simplify_mesh(tv, tf, voxel_size=case["voxel_size"], origin=case["origin"])
    assert len(out) == 3 and out[2] is None and torch.equal(_bits(out[0]), _bits(v)) and torch.equal(out[1], f)
    out = simplify_mesh(tv, tf, None, voxel_size=case["voxel_size"], origin=case["origin"], return_map=True)
    assert len(out) == 4 and out[2] is None and torch.equal(out[3], m)
    # nothing left, and no faces at all: [0,3] tensors, None stays None, the map is -1
    fan = R.cases()["one_cell_fan_65"]
    fv, ff = torch.from_numpy(fan["vertices"]).to(gpu_device), torch.from_numpy(fan["faces"]).to(gpu_device)
    for faces in (ff, ff[:0]):
        out = simplify_mesh(fv, faces, voxel_size=1.0, origin=(0.0, 0.0, 0.0), return_map=True)
        assert tuple(out[0].shape) == (0, 3) and tuple(out[1].shape) == (0, 3) and out[2] is None
        assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[3].tolist() == [-1] * 65
        assert len(simplify_mesh(fv, faces, fv, voxel_size=1.0)) == 3


def test_default_origin_is_the_lowest_referenced_vertex_minus_half_a_cell(gpu_device):
    case = R.cases()["sphere_tsdf"]
    want = R.simplify(case["vertices"], case["faces"], case["colors"], voxel_size=1.7)
    (v, f, c, m), _ = _run(case, gpu_device, voxel_size=1.7, origin=None)
    assert np.array_equal(f.cpu().numpy(), want.faces) and np.array_equal(m.cpu().numpy(), want.vertex_cluster)
    _within(v.cpu().numpy(), want.vertices, want.max_abs, "default origin positions")
    explicit, _ = _run(case, gpu_device, voxel_size=1.7, origin=tuple(want.origin.tolist()))
    assert torch.equal(_bits(explicit[0]), _bits(v)) and torch.equal(explicit[1], f)


@pytest.mark.parametrize("name", ["run_257", "grid_70k", "sphere_tsdf"])
def test_face_order_changes_no_vertex_bit_and_no_face(gpu_device, name):
    case = R.cases()[name]
    (v, f, c, m), _ = _run(case, gpu_device)
    perm = R.permutation(len(case["faces"]))
    shuffled = dict(case, faces=np.ascontiguousarray(case["faces"][perm]))
    (pv, pf, pc, pm), _ = _run(shuffled, gpu_device)
    assert torch.equal(_bits(pv), _bits(v)) and torch.equal(_bits(pc), _bits(c)) and torch.equal(pm, m)
    assert R.rotated_set(pf.cpu().numpy()) == R.rotated_set(f.cpu().numpy()) and pf.shape == f.shape


@pytest.mark.parametrize("name", ["run_257", "unreferenced_nan", "grid_70k", "sphere_tsdf"])
def test_vertex_order_changes_no_cluster(gpu_device, name):
    case, want = R.cases()[name], R.reference(name)
    V = len(case["vertices"])
    perm = R.permutation(V)                                   # new vertex n is old vertex perm[n]
    new_of_old = np.empty(V, dtype=np.int64)
    new_of_old[perm] = np.arange(V)
    origin = case["origin"] if case["origin"] is not None else tuple(want.origin.tolist())
    shuffled = dict(case, vertices=np.ascontiguousarray(case["vertices"][perm]), colors=np.ascontiguousarray(case["colors"][perm]),
                    faces=new_of_old[case["faces"]].astype(np.int32), origin=origin)
    (pv, pf, pc, pm), _ = _run(shuffled, gpu_device)
    assert R.vertex_partition(pm.cpu().numpy(), perm) == R.vertex_partition(want.vertex_cluster)
    # clusters are numbered by key, which the order of the vertices does not enter
    assert np.array_equal(pm.cpu().numpy(), want.vertex_cluster[perm]) and np.array_equal(pf.cpu().numpy(), want.faces)
    _within(pv.cpu().numpy(), want.vertices, want.max_abs, f"{name} positions, vertices permuted")
    _within(pc.cpu().numpy(), want.colors, want.max_abs_colors, f"{name} colours, vertices permuted")


def test_strided_views_spare_vertices_and_a_side_stream_give_the_same_result(gpu_device):
    from mvs_gaussian_splatting_amd import simplify_mesh
    case = R.cases()["sphere_tsdf"]
    (v, f, c, m), (tv, tf, tc) = _run(case, gpu_device)
    V, F = tv.shape[0], tf.shape[0]
    wide_f = torch.zeros((F, 5), dtype=torch.int32, device=gpu_device)
    wide_f[:, 1:4] = tf
    wide_v = torch.full((V + 40, 7), float("nan"), device=gpu_device)      # spare trailing vertices, full of NaN
    wide_v[:V, 2:5] = tv
    wide_c = torch.full((V + 40, 4), float("nan"), device=gpu_device)
    wide_c[:V, 0:3] = tc
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        sv, sf, sc, sm = simplify_mesh(wide_v[:, 2:5], wide_f[:, 1:4], wide_c[:, 0:3], voxel_size=case["voxel_size"],
                                       origin=case["origin"], return_map=True)
    side.synchronize()
    assert torch.equal(_bits(sv), _bits(v)) and torch.equal(sf, f) and torch.equal(_bits(sc), _bits(c))
    assert torch.equal(sm[:V], m) and sm[V:].tolist() == [-1] * 40


def test_status_word_refusals_raise_and_the_next_call_is_right(gpu_device):
    """Status-word checks on valid memory, like the one ``connected_components`` has: nothing here faults."""
    from mvs_gaussian_splatting_amd import _lib, simplify_mesh
    case, want = R.cases()["sphere_tsdf"], R.reference("sphere_tsdf")
    tv, tf = torch.from_numpy(case["vertices"]).to(gpu_device), torch.from_numpy(case["faces"]).to(gpu_device)
    V = tv.shape[0]
    referenced = int(case["faces"][1234, 1])
    for value in (float("nan"), float("inf"), float("-inf")):
        bad = tv.clone()
        bad[referenced, 2] = value
        for origin in (None, (0.0, 0.0, 0.0)):
            with pytest.raises(_lib.GsrError, match="not finite"):
                simplify_mesh(bad, tf, voxel_size=2.0, origin=origin)
    for index in (V, -1, 2 ** 31 - 1):
        bad = tf.clone()
        bad[1700, 2] = index
        with pytest.raises(_lib.GsrError, match="outside"):
            simplify_mesh(tv, bad, voxel_size=2.0)
    extent = float(case["vertices"].max() - case["vertices"].min())
    with pytest.raises(_lib.GsrError, match="too small"):
        simplify_mesh(tv, tf, voxel_size=extent / 2 ** 21 / 1.5)            # 2^21 cells or more along an axis
    fine = extent / 2 ** 21 * 4                                             # 2^19 cells: accepted
    want_fine = R.simplify(case["vertices"], case["faces"], voxel_size=fine)
    assert np.array_equal(simplify_mesh(tv, tf, voxel_size=fine)[1].cpu().numpy(), want_fine.faces) and len(want_fine.faces)
    above = case["vertices"].min(axis=0).astype(np.float64) + (0.0, 0.25, 0.0)
    with pytest.raises(_lib.GsrError, match="origin lies above"):
        simplify_mesh(tv, tf, voxel_size=2.0, origin=tuple(above.tolist()))
    torch.cuda.synchronize()
    (v, f, c, m), _ = _run(case, gpu_device)
    assert np.array_equal(f.cpu().numpy(), want.faces) and np.array_equal(m.cpu().numpy(), want.vertex_cluster)


def test_clean_then_simplify_then_components_runs_end_to_end(gpu_device):
    from mvs_gaussian_splatting_amd import clean_mesh, connected_components, simplify_mesh
    case = R.cases()["sphere_tsdf"]
    tv, tf = torch.from_numpy(case["vertices"]).to(gpu_device), torch.from_numpy(case["faces"]).to(gpu_device)
    tc = torch.from_numpy(case["colors"]).to(gpu_device)
    cv, cf, cc = clean_mesh(tv, tf, tc, keep_largest=1)
    h = 2.0
    sv, sf, sc = simplify_mesh(cv, cf, cc, voxel_size=h)
    assert 0 < sf.shape[0] < cf.shape[0] and 0 < sv.shape[0] < cv.shape[0] and sc.shape == sv.shape
    face_component, component_faces = connected_components(sf, sv.shape[0])
    assert int(component_faces.sum()) == sf.shape[0] and face_component.shape[0] == sf.shape[0]
    out, src = sv.cpu().numpy().astype(np.float64), cv.cpu().numpy().astype(np.float64)
    nearest = np.sqrt(((out[:, None, :] - src[None, :, :]) ** 2).sum(axis=2).min(axis=1))
    assert nearest.max() <= math.sqrt(3.0) * h, "an output vertex is further than a cell's diagonal from every input vertex"
    lo, hi = src.min(axis=0), src.max(axis=0)
    assert np.all(out >= lo - 1e-6) and np.all(out <= hi + 1e-6), "a mean lies outside the box of the input"
