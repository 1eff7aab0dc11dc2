"""Mesh cleaning on the HIP path (csrc/mesh.hip; ``mesh.connected_components``, ``mesh.clean_mesh``)
against the sequential restatement of tests/mesh_restate.py.

Everything here is integers and bit-copies, so every comparison is exact: ``face_component`` and ``component_faces``
integer for integer, the cleaned faces integer for integer, the cleaned vertex and colour rows the bits of the kept input
rows.  Each case runs twice (the same bits) and once more with its faces permuted (the same partition).  The cases are
the smallest at which the kernels can go wrong; tests/test_mesh_host.py checks that they have the shapes they are there
for."""
import functools

import numpy as np
import pytest
import torch

import mesh_restate as M
import tsdf_restate as T

pytestmark = pytest.mark.gpu

MODES = ("edge", "vertex")
CASES = sorted(M.cases())


@functools.lru_cache(maxsize=None)
def _reference(name, connectivity):
    """The restatement's components of a case; computed once, never modified."""
    faces, V = M.cases()[name]
    return M.components(faces, V, connectivity)


def _components(faces, V, connectivity, dev):
    from mvs_gaussian_splatting_amd import connected_components
    fc, cf = connected_components(torch.from_numpy(np.ascontiguousarray(faces)).to(dev), V, connectivity)
    assert fc.dtype == torch.int32 and cf.dtype == torch.int64 and fc.device == cf.device and fc.is_cuda
    return fc, cf


@pytest.mark.parametrize("connectivity", MODES)
@pytest.mark.parametrize("name", CASES)
def test_components_match_the_restatement_twice_and_under_a_face_permutation(gpu_device, name, connectivity):
    faces, V = M.cases()[name]
    want_fc, want_cf = _reference(name, connectivity)
    fc, cf = _components(faces, V, connectivity, gpu_device)
    assert np.array_equal(fc.cpu().numpy(), want_fc), "face_component differs from the restatement"
    assert np.array_equal(cf.cpu().numpy(), want_cf), "component_faces differs from the restatement"
    fc2, cf2 = _components(faces, V, connectivity, gpu_device)
    assert torch.equal(fc, fc2) and torch.equal(cf, cf2), "not the same bits from run to run"
    perm = M.face_permutation(len(faces))
    pfc, pcf = _components(faces[perm], V, connectivity, gpu_device)
    assert M.partition(pfc.cpu().numpy(), perm) == M.partition(want_fc), "the partition depends on the face order"
    assert sorted(pcf.tolist()) == sorted(want_cf.tolist())
    if name.startswith("strip_"):
        assert cf.tolist() == [M.STRIP_FACES] and int(fc.max()) == 0, "the strip is a single component"
    if name == "isolated_1000":
        assert cf.shape[0] == len(faces) and fc.tolist() == list(range(len(faces)))
    if name == "bow_tie":
        assert cf.shape[0] == (1 if connectivity == "vertex" else 2)


def test_num_vertices_defaults_to_the_largest_index_plus_one_and_layouts_do_not_matter(gpu_device):
    from mvs_gaussian_splatting_amd import connected_components
    faces, V = M.cases()["soup"]
    want_fc, want_cf = _reference("soup", "edge")
    dev_faces = torch.from_numpy(faces).to(gpu_device)
    fc, cf = connected_components(dev_faces)
    assert np.array_equal(fc.cpu().numpy(), want_fc) and np.array_equal(cf.cpu().numpy(), want_cf)
    wide = torch.zeros((len(faces), 5), dtype=torch.int32, device=gpu_device)
    wide[:, 1:4] = dev_faces
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        fc2, cf2 = connected_components(wide[:, 1:4], V + 40, "edge")        # a strided view, spare vertices, a side stream
    side.synchronize()
    assert torch.equal(fc, fc2) and torch.equal(cf, cf2)


def _bits(rng, n):
    """float32 rows of arbitrary bits (NaNs, infinities, negative zeros among them): a bit-copy must keep them all."""
    return rng.integers(-2 ** 31, 2 ** 31, size=(n, 3), dtype=np.int64).astype(np.int32).view(np.float32)


def _clean_and_compare(faces, vertices, colors, dev, **kw):
    from mvs_gaussian_splatting_amd import clean_mesh
    want_v, want_f, want_c, kept_v, kept_f = M.clean(vertices, faces, colors, **kw)
    tv, tf = torch.from_numpy(vertices).to(dev), torch.from_numpy(faces).to(dev)
    tc = None if colors is None else torch.from_numpy(colors).to(dev)
    keep_v, keep_f = tv.clone(), tf.clone()
    got = clean_mesh(tv, tf, tc, **kw)
    again = clean_mesh(tv, tf, tc, **kw)
    assert torch.equal(tv.view(torch.int32), keep_v.view(torch.int32)) and torch.equal(tf, keep_f), "an input was written"
    v, f, c = got
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert tuple(v.shape) == want_v.shape and tuple(f.shape) == want_f.shape and v.shape[1] == 3 and f.shape[1] == 3
    assert np.array_equal(f.cpu().numpy(), want_f), "cleaned faces differ from the restatement"
    assert np.array_equal(v.cpu().numpy().view(np.int32), want_v.view(np.int32)), "kept vertex rows are not bit-copies"
    if colors is None:
        assert c is None
    else:
        assert np.array_equal(c.cpu().numpy().view(np.int32), want_c.view(np.int32)), "kept colour rows are not bit-copies"
        assert torch.equal(c.view(torch.int32), again[2].view(torch.int32))
    assert torch.equal(v.view(torch.int32), again[0].view(torch.int32)) and torch.equal(f, again[1])
    return got, kept_v, kept_f


@pytest.mark.parametrize("connectivity", MODES)
@pytest.mark.parametrize("name", CASES)
def test_clean_mesh_matches_the_restatement_bit_for_bit(gpu_device, name, connectivity):
    faces, V = M.cases()[name]
    rng = np.random.default_rng(len(name))
    vertices, colors = _bits(rng, V), _bits(rng, V)
    _, sizes = _reference(name, connectivity)
    second = int(np.sort(sizes)[::-1][min(1, len(sizes) - 1)])
    settings = [dict(), dict(keep_largest=1), dict(keep_largest=2, min_faces=2), dict(min_faces=second + 1),
                dict(keep_largest=len(sizes) + 3)]
    for n, kw in enumerate(settings):
        _clean_and_compare(faces, vertices, colors if n % 2 == 0 else None, gpu_device, connectivity=connectivity, **kw)


@pytest.mark.parametrize("connectivity", MODES)
def test_ties_at_the_threshold_all_survive(gpu_device, connectivity):
    faces, V = M.cases()["forty_equal"]
    vertices = _bits(np.random.default_rng(40), V)
    (v, f, c), kept_v, kept_f = _clean_and_compare(faces, vertices, None, gpu_device, keep_largest=3, connectivity=connectivity)
    assert len(kept_f) == len(faces) and tuple(f.shape) == faces.shape and tuple(v.shape) == (V, 3)
    assert torch.equal(f.cpu(), torch.from_numpy(faces))


@pytest.mark.parametrize("connectivity", MODES)
def test_min_faces_above_every_component_gives_empty_tensors(gpu_device, connectivity):
    from mvs_gaussian_splatting_amd import clean_mesh, connected_components
    faces, V = M.cases()["soup"]
    tf = torch.from_numpy(faces).to(gpu_device)
    tv = torch.zeros((V, 3), device=gpu_device)
    biggest = int(_reference("soup", connectivity)[1].max())
    for colors in (None, torch.ones((V, 3), device=gpu_device)):
        v, f, c = clean_mesh(tv, tf, colors, min_faces=biggest + 1, connectivity=connectivity)
        assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32
        assert (c is None) == (colors is None) and (c is None or tuple(c.shape) == (0, 3))
        v, f, c = clean_mesh(tv, tf, colors, min_faces=biggest, connectivity=connectivity)
        assert f.shape[0] >= biggest
    # no faces at all: no native call, empty outputs
    none = torch.empty((0, 3), dtype=torch.int32, device=gpu_device)
    fc, cf = connected_components(none, V, connectivity)
    assert tuple(fc.shape) == (0,) and tuple(cf.shape) == (0,) and fc.dtype == torch.int32 and cf.dtype == torch.int64
    v, f, c = clean_mesh(tv, none, None, keep_largest=1, connectivity=connectivity)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and c is None


@pytest.mark.parametrize("connectivity", MODES)
def test_a_face_index_equal_to_V_is_refused_and_nothing_faults(gpu_device, connectivity):
    from mvs_gaussian_splatting_amd import _lib, clean_mesh, connected_components
    faces, V = M.cases()["strip_permuted"]
    bad = faces.copy()
    bad[1700, 2] = V
    tv = torch.zeros((V, 3), device=gpu_device)
    for broken in (bad, np.where(bad == V, -1, bad).astype(np.int32)):
        tf = torch.from_numpy(broken).to(gpu_device)
        with pytest.raises(_lib.GsrError, match="outside"):
            connected_components(tf, V, connectivity)
        with pytest.raises(_lib.GsrError, match="outside"):
            clean_mesh(tv, tf, keep_largest=1, connectivity=connectivity)
    torch.cuda.synchronize()
    # the device is fine and the next call is right
    fc, cf = _components(faces, V, connectivity, gpu_device)
    assert cf.tolist() == [len(faces)]


def _load(field, dev):
    from mvs_gaussian_splatting_amd import TSDFVolume
    nz, ny, nx = field["tsdf"].shape
    vol = TSDFVolume(field["origin"], field["voxel_size"], (nx, ny, nz), field["sdf_trunc"], with_color=True, device=dev)
    vol.tsdf = torch.from_numpy(field["tsdf"]).to(dev)
    vol.weight = torch.from_numpy(field["weight"]).to(dev)
    vol.color = torch.from_numpy(field["color"]).to(dev)
    return vol


@pytest.mark.parametrize("connectivity", MODES)
def test_sphere_with_two_floaters_cleans_to_the_closed_sphere(gpu_device, connectivity):
    from mvs_gaussian_splatting_amd import clean_mesh, connected_components
    _, ref_faces, _ = M.floater_mesh()
    vertices, faces, colors = _load(M.floater_field(), gpu_device).extract_mesh()
    f_np = faces.cpu().numpy()
    assert np.array_equal(f_np, ref_faces), "the extracted faces differ from the restatement's"
    fc, cf = connected_components(faces, vertices.shape[0], connectivity)
    want_fc, want_cf = M.components(f_np, vertices.shape[0], connectivity)
    assert np.array_equal(fc.cpu().numpy(), want_fc) and np.array_equal(cf.cpu().numpy(), want_cf) and len(want_cf) == 3
    v_np, c_np = vertices.cpu().numpy(), colors.cpu().numpy()
    want_v, want_f, want_c, kept_v, kept_f = M.clean(v_np, f_np, c_np, keep_largest=1, connectivity=connectivity)
    v, f, c = clean_mesh(vertices, faces, colors, keep_largest=1, connectivity=connectivity)
    assert np.array_equal(f.cpu().numpy(), want_f), "cleaned faces differ from the restatement"
    assert torch.equal(v.view(torch.int32), vertices[torch.from_numpy(kept_v).to(gpu_device)].view(torch.int32))
    assert torch.equal(c.view(torch.int32), colors[torch.from_numpy(kept_v).to(gpu_device)].view(torch.int32))
    assert 0 < v.shape[0] < vertices.shape[0] and 0 < f.shape[0] < faces.shape[0]
    T.assert_closed_oriented_sphere(v.cpu().numpy().astype(np.float64), f.cpu().numpy())       # closed, Euler characteristic 2
    v2, f2, c2 = clean_mesh(vertices, faces, colors, keep_largest=1, connectivity=connectivity)
    assert torch.equal(v2, v) and torch.equal(f2, f) and torch.equal(c2, c)
