"""CPU-side checks of the mesh cleaning (csrc/mesh.hip; mesh.py): the restatement the GPU tests compare
against (tests/mesh_restate.py) held to scipy's connected components and to the topology of a cleaned sphere, the ABI and
the refusals of every entry point -- which all come before a GPU is asked for -- the Python argument checks, and the
flags of examples/extract_mesh.py."""
import ctypes as C
import importlib.util
import os
import re
import types

import numpy as np
import pytest
import torch
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components as scipy_components

from conftest import ROOT
import mesh_restate as M
import tsdf_restate as T

ENTRY_POINTS = ("gsr_mesh_cc_init", "gsr_mesh_cc_hook_faces", "gsr_mesh_edge_keys", "gsr_mesh_cc_hook_runs",
                "gsr_mesh_cc_flatten", "gsr_mesh_cc_mark", "gsr_mesh_cc_label", "gsr_mesh_mark_vertices",
                "gsr_mesh_compact")


def _scipy_face_labels(faces, V, connectivity):
    faces = np.asarray(faces, dtype=np.int64)
    F = len(faces)
    if connectivity == "vertex":
        rows = np.concatenate((faces[:, 0], faces[:, 0]))
        cols = np.concatenate((faces[:, 1], faces[:, 2]))
        _, labels = scipy_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
        return labels[faces[:, 0]]
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    keys = np.minimum(a, b) * V + np.maximum(a, b)
    owner = np.repeat(np.arange(F), 3)
    order = np.argsort(keys, kind="stable")
    same = keys[order][1:] == keys[order][:-1]
    rows, cols = owner[order][:-1][same], owner[order][1:][same]
    _, labels = scipy_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(F, F)), directed=False)
    return labels


@pytest.mark.parametrize("connectivity", ["edge", "vertex"])
@pytest.mark.parametrize("name", sorted(M.cases()))
def test_restatement_agrees_with_scipy_after_canonical_renumbering(name, connectivity):
    faces, V = M.cases()[name]
    face_component, component_faces = M.components(faces, V, connectivity)
    want = M.canonical(_scipy_face_labels(faces, V, connectivity))
    assert np.array_equal(face_component, want), "the restatement's components differ from scipy's"
    assert np.array_equal(component_faces, np.bincount(want)) and component_faces.sum() == len(faces)
    # numbered in the order of the smallest face index
    firsts = [int(np.nonzero(face_component == c)[0][0]) for c in range(len(component_faces))]
    assert firsts == sorted(firsts)


def test_cases_have_the_shapes_they_are_there_for():
    c = M.cases()
    count = lambda name, mode: len(M.components(*c[name], mode)[1])                    # noqa: E731
    assert len(c["one_face"][0]) == 1
    assert count("two_faces_one_edge", "edge") == 1
    assert count("bow_tie", "vertex") == 1 and count("bow_tie", "edge") == 2
    for numbering in ("ascending", "descending", "permuted"):
        faces, V = c[f"strip_{numbering}"]
        assert len(faces) == 3000 > 256 and V == 3002
        assert count(f"strip_{numbering}", "edge") == count(f"strip_{numbering}", "vertex") == 1
    assert int(c["strip_descending"][0][-1].min()) == 0 and int(c["strip_ascending"][0][0].min()) == 0
    assert count("isolated_1000", "edge") == count("isolated_1000", "vertex") == 1000
    sizes = M.components(*c["forty_equal"], "edge")[1]
    assert len(sizes) == 40 and len(set(sizes.tolist())) == 1
    faces, V = c["smallest_vertex_last"]
    comp, _ = M.components(faces, V, "vertex")
    assert faces[comp == 0].min() == 0 and 0 not in faces[:-1] and comp[-1] == 0 and comp[2] == 1
    faces, V = c["unreferenced_vertices"]
    assert sorted(set(range(V)) - set(faces.reshape(-1).tolist())) == [0, 1, 4, 7, 10, 12]
    assert M.components(*c["three_faces_one_edge"], "edge")[1].tolist() == [3, 1]
    comp, _ = M.components(*c["degenerate_faces"], "edge")
    assert comp.tolist() == [0, 0, 1, 2, 1]
    faces, V = c["soup"]
    assert (V, len(faces)) == (500, 700) and count("soup", "edge") > 100 > count("soup", "vertex") >= 1


def test_clean_rule_thresholds_ties_and_empty_results():
    faces, V = M.cases()["forty_equal"]
    vertices = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    v, f, _, kept_v, kept_f = M.clean(vertices, faces, keep_largest=3)
    assert len(f) == len(faces) and len(v) == V, "ties at the threshold all survive"
    v, f, _, _, _ = M.clean(vertices, faces, min_faces=8)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    faces, V = M.cases()["three_faces_one_edge"]
    vertices = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    v, f, _, kept_v, kept_f = M.clean(vertices, faces, keep_largest=1)
    assert kept_f.tolist() == [0, 1, 2] and kept_v.tolist() == [0, 1, 2, 3, 4] and f.max() == 4
    assert len(M.clean(vertices, faces, keep_largest=2)[1]) == len(M.clean(vertices, faces, keep_largest=7)[1]) == 4
    faces, V = M.cases()["unreferenced_vertices"]
    vertices = np.arange(3 * V, dtype=np.float32).reshape(V, 3)
    v, f, _, kept_v, _ = M.clean(vertices, faces)
    assert kept_v.tolist() == [2, 3, 5, 6, 8, 9, 11] and np.array_equal(v, vertices[kept_v])
    assert f.tolist() == [[0, 1, 2], [2, 1, 3], [4, 5, 6]]


def test_tsdf_case_is_a_sphere_and_two_floaters_and_cleans_to_euler_characteristic_two():
    vertices, faces, colors = M.floater_mesh()
    for connectivity in ("edge", "vertex"):
        _, sizes = M.components(faces, len(vertices), connectivity)
        assert len(sizes) == 3 and sorted(sizes.tolist())[1] >= 8 and sizes.max() > 5000, sizes
    with pytest.raises(AssertionError):
        T.assert_closed_oriented_sphere(vertices, faces)                 # three shells: Euler characteristic 6
    v, f, c, kept_v, _ = M.clean(vertices, faces, colors, keep_largest=1)
    assert 0 < len(kept_v) < len(vertices) and np.array_equal(c, colors[kept_v])
    T.assert_closed_oriented_sphere(v, f)
    sphere_v, sphere_f, _ = T.extract(T.sphere_field())
    assert np.array_equal(v, sphere_v) and len(f) == len(sphere_f), "what is left is the sphere of the TSDF tests"


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_mesh_entry_points_and_the_abi_is_at_least_31():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib, mesh
    assert pkg.connected_components is mesh.connected_components and pkg.clean_mesh is mesh.clean_mesh
    assert "connected_components" in pkg.__all__ and "clean_mesh" in pkg.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\bint " + name + r"\(", header), name
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("gsr_mesh_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 31


def test_every_entry_point_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    big = 2 ** 31
    BAD, ALIGN = -1, -3

    assert lib.gsr_mesh_cc_init(0, p, None, None) == BAD
    assert lib.gsr_mesh_cc_init(big, p, None, None) == BAD
    assert lib.gsr_mesh_cc_init(4, None, p, None) == BAD
    assert lib.gsr_mesh_cc_init(4, p + 2, None, None) == ALIGN
    assert lib.gsr_mesh_cc_init(4, p, p + 1, None) == ALIGN
    assert b"aligned" in lib.gsr_last_error()

    hook = lib.gsr_mesh_cc_hook_faces
    assert hook(None, 4, 4, p, p, None, None) == BAD
    assert hook(p, 4, 4, None, p, None, None) == BAD
    assert hook(p, 4, 4, p, None, None, None) == BAD                     # the status word is required
    for F, V in ((0, 4), (-1, 4), (big, 4), (4, 0), (4, big)):
        assert hook(p, F, V, p, p, None, None) == BAD, (F, V)
    assert hook(p + 1, 4, 4, p, p, None, None) == ALIGN
    assert hook(p, 4, 4, p, p + 2, None, None) == ALIGN
    assert hook(p, 4, 4, p, p, p + 4, None) == ALIGN                     # stats: uint64

    keys = lib.gsr_mesh_edge_keys
    for args in ((None, 4, 4, p, p, p), (p, 4, 4, None, p, p), (p, 4, 4, p, None, p), (p, 4, 4, p, p, None),
                 (p, 0, 4, p, p, p), (p, 4, 0, p, p, p), (p, big, 4, p, p, p), (p, 4, big, p, p, p)):
        assert keys(*args, None) == BAD, args
    assert keys(p, 4, 4, p + 4, p, p, None) == ALIGN                     # keys: int64
    assert keys(p, 4, 4, p, p + 2, p, None) == ALIGN

    runs = lib.gsr_mesh_cc_hook_runs
    for args in ((None, p, p, 12, 4, p, p, None), (p, None, p, 12, 4, p, p, None), (p, p, None, 12, 4, p, p, None),
                 (p, p, p, 12, 4, None, p, None), (p, p, p, 12, 4, p, None, None), (p, p, p, 0, 4, p, p, None),
                 (p, p, p, 12, 0, p, p, None), (p, p, p, 12, big, p, p, None), (p, p, p, 3 * big, 4, p, p, None)):
        assert runs(*args, None) == BAD, args
    assert runs(p + 4, p, p, 12, 4, p, p, None, None) == ALIGN
    assert runs(p, p + 4, p, 12, 4, p, p, None, None) == ALIGN
    assert runs(p, p, p + 1, 12, 4, p, p, None, None) == ALIGN
    assert runs(p, p, p, 12, 4, p, p, p + 4, None) == ALIGN

    assert lib.gsr_mesh_cc_flatten(0, p, None) == BAD
    assert lib.gsr_mesh_cc_flatten(big, p, None) == BAD
    assert lib.gsr_mesh_cc_flatten(4, None, None) == BAD
    assert lib.gsr_mesh_cc_flatten(4, p + 3, None) == ALIGN

    mark = lib.gsr_mesh_cc_mark
    assert mark(None, 0, 0, p, None, None, p, None) == BAD
    assert mark(None, big, 0, p, None, None, p, None) == BAD
    assert mark(None, 4, 0, None, None, None, p, None) == BAD
    assert mark(None, 4, 0, p, None, None, None, None) == BAD
    assert mark(p, 4, 4, p, None, p, p, None) == BAD                     # faces, first and face_root: all or none
    assert mark(p, 4, 4, p, p, None, p, None) == BAD
    assert mark(None, 4, 4, p, p, p, p, None) == BAD
    assert mark(p, 4, 0, p, p, p, p, None) == BAD                        # vertex nodes need V
    assert mark(p, 4, big, p, p, p, p, None) == BAD
    assert mark(None, 4, 0, p + 2, None, None, p, None) == ALIGN
    assert mark(p, 4, 4, p, p, p + 1, p, None) == ALIGN

    label = lib.gsr_mesh_cc_label
    for args in ((None, p, 4, 2, p, p), (p, None, 4, 2, p, p), (p, p, 4, 2, None, p), (p, p, 4, 2, p, None),
                 (p, p, 0, 1, p, p), (p, p, big, 1, p, p), (p, p, 4, 0, p, p), (p, p, 4, 5, p, p)):
        assert label(*args, None) == BAD, args
    assert label(p + 2, p, 4, 2, p, p, None) == ALIGN
    assert label(p, p + 4, 4, 2, p, p, None) == ALIGN
    assert label(p, p, 4, 2, p, p + 4, None) == ALIGN

    mv = lib.gsr_mesh_mark_vertices
    for args in ((None, p, 4, 4, p, p), (p, None, 4, 4, p, p), (p, p, 4, 4, None, p), (p, p, 4, 4, p, None),
                 (p, p, 0, 4, p, p), (p, p, 4, 0, p, p), (p, p, big, 4, p, p), (p, p, 4, big, p, p)):
        assert mv(*args, None) == BAD, args
    assert mv(p + 1, p, 4, 4, p, p, None) == ALIGN
    assert mv(p, p + 1, 4, 4, p + 1, p + 2, None) == ALIGN               # the byte arrays may sit anywhere; status may not

    compact = lib.gsr_mesh_compact
    good = [p, p, p, p, p, p, p, 4, 4, 2, 2, p, p, p, p]
    for n in (0, 2, 3, 4, 5, 6, 11, 13, 14):                             # every required pointer
        args = list(good)
        args[n] = None
        assert compact(*args, None) == BAD, n
    for n, bad in ((7, 0), (7, big), (8, 0), (8, big), (9, 0), (9, 5), (10, 0), (10, 5)):
        args = list(good)
        args[n] = bad
        assert compact(*args, None) == BAD, (n, bad)
    args = list(good)
    args[1] = None                                                       # colours without out_colors and the reverse
    assert compact(*args, None) == BAD
    args = list(good)
    args[12] = None
    assert compact(*args, None) == BAD
    for n, off, in ((0, 2), (1, 2), (2, 1), (11, 2), (12, 2), (13, 2), (14, 2), (5, 4), (6, 4)):
        args = list(good)
        args[n] = p + off
        assert compact(*args, None) == ALIGN, n


# ---- Python argument checks ------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, clean_mesh, connected_components
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    vertices = torch.zeros(4, 3)
    for bad in (faces.long(), faces.float(), faces.reshape(-1), faces[:, :2], faces.numpy(), None):
        with pytest.raises(ValueError):
            connected_components(bad, 4)
        with pytest.raises(ValueError):
            clean_mesh(vertices, bad)
    for nv in (-1, 2 ** 31, 4.0, True, 0):
        with pytest.raises(ValueError):
            connected_components(faces, nv)
    for mode in ("face", "Edge", None, 1):
        with pytest.raises(ValueError):
            connected_components(faces, 4, connectivity=mode)
        with pytest.raises(ValueError):
            clean_mesh(vertices, faces, connectivity=mode)
    for bad in (vertices.double(), torch.zeros(4, 2), torch.zeros(12), vertices.numpy()):
        with pytest.raises(ValueError):
            clean_mesh(bad, faces)
    for bad in (torch.zeros(3, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 4), torch.zeros(4, 3, device="meta")):
        with pytest.raises(ValueError):
            clean_mesh(vertices, faces, bad)
    with pytest.raises(ValueError):
        clean_mesh(vertices, faces.to("meta"))
    with pytest.raises(ValueError):
        clean_mesh(torch.zeros(0, 3), faces)                             # faces without vertices
    for kw in ({"keep_largest": 0}, {"keep_largest": -3}, {"keep_largest": 1.5}, {"keep_largest": True},
               {"min_faces": -1}, {"min_faces": 2.0}, {"min_faces": None}):
        with pytest.raises(ValueError):
            clean_mesh(vertices, faces, **kw)
    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        connected_components(faces, 4)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        connected_components(faces, connectivity="vertex")
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        clean_mesh(vertices, faces, torch.zeros(4, 3), keep_largest=1, min_faces=5)


# ---- the example -------------------------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("example_extract_mesh", os.path.join(ROOT, "examples", "extract_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stub(mod, monkeypatch, calls):
    """A stub scene, renderer and volume: every call the example makes is recorded by name."""
    mesh = ("vertices", "faces", "colors")

    class Volume:
        dims, voxel_size, sdf_trunc = (4, 4, 4), 0.5, 2.0

        def extract_mesh(self, *a, **kw):
            calls.append(("extract_mesh", a, kw))
            return tuple(types.SimpleNamespace(shape=(n, 3), name=m) for n, m in zip((8, 12, 8), mesh))

    class Scene:
        loaded_iter = 7

        def __init__(self, *a, **kw):
            calls.append(("Scene", kw))

        def getTrainCameras(self):
            return ["cam"]

    def record(name, result=None):
        def fn(*a, **kw):
            calls.append((name, tuple(getattr(x, "name", x) for x in a if isinstance(x, (str, types.SimpleNamespace))), kw))
            return result
        return fn

    monkeypatch.setattr(mod, "GaussianModel", lambda d: types.SimpleNamespace(get_xyz="xyz"))
    monkeypatch.setattr(mod, "Scene", Scene)
    monkeypatch.setattr(mod, "volume_for_points", lambda xyz, **kw: calls.append(("volume_for_points", kw)) or Volume())
    monkeypatch.setattr(mod, "fuse_views", lambda *a, **kw: calls.append(("fuse_views", kw)))
    monkeypatch.setattr(mod, "write_ply_mesh", record("write_ply_mesh"))
    small = tuple(types.SimpleNamespace(shape=(n, 3), name=m + "_post") for n, m in zip((5, 6, 5), mesh))
    monkeypatch.setattr(mod, "clean_mesh", record("clean_mesh", small))
    monkeypatch.setattr(mod, "torch", types.SimpleNamespace(no_grad=torch.no_grad, float32=torch.float32,
                                                            tensor=lambda *a, **kw: "background"))
    monkeypatch.setattr(mod, "ModelParams", lambda **kw: types.SimpleNamespace(sh_degree=3, white_background=False, **kw))


def test_example_without_the_flags_makes_the_calls_it_made_and_with_them_writes_the_cleaned_mesh_too(monkeypatch, tmp_path, capsys):
    mod = _example()
    base = ["-m", str(tmp_path), "-s", "dataset", "--resolution", "32"]
    calls = []
    _stub(mod, monkeypatch, calls)
    mod.main(base)
    plain = list(calls)
    assert [c[0] for c in plain] == ["Scene", "volume_for_points", "fuse_views", "extract_mesh", "write_ply_mesh"]
    raw = os.path.join(str(tmp_path), "mesh", "iteration_7", "tsdf_mesh.ply")
    assert plain[-1] == ("write_ply_mesh", (raw, "vertices", "faces", "colors"), {})
    assert plain[3] == ("extract_mesh", (), {}) and plain[2][1] == {"alpha_min": 0.5, "max_depth": None}
    assert "cleaned" not in capsys.readouterr().out

    for flags, want in ((["--num_cluster", "50"], {"keep_largest": 50, "min_faces": 50}),
                        (["--min_cluster_faces", "20"], {"keep_largest": None, "min_faces": 20}),
                        (["--num_cluster", "3", "--min_cluster_faces", "0"], {"keep_largest": 3, "min_faces": 0})):
        del calls[:]
        mod.main(base + flags)
        assert calls[:5] == plain, "the raw mesh is extracted and written exactly as without the flags"
        assert calls[5] == ("clean_mesh", ("vertices", "faces", "colors"), want)
        post = os.path.join(os.path.dirname(raw), "tsdf_mesh_post.ply")
        assert calls[6] == ("write_ply_mesh", (post, "vertices_post", "faces_post", "colors_post"), {}) and len(calls) == 7
        out = capsys.readouterr().out
        assert "8 vertices, 12 faces" in out and "5 of 8 vertices, 6 of 12 faces" in out

    for flags in (["--num_cluster", "0"], ["--min_cluster_faces", "-1"], ["--num_cluster", "many"]):
        with pytest.raises(SystemExit):
            mod.main(base + flags)
