"""CPU-side checks of the mesh simplification (csrc/mesh_simplify.hip; ``mesh.simplify_mesh``): the
restatement the GPU tests compare against (tests/mesh_simplify_restate.py) has the cases it is named for and keeps its
invariants, the cell arithmetic of csrc/mesh_simplify_math.h built by the host compiler agrees with numpy's float64
floor, the ABI and the refusals of every entry point -- which all come before a GPU is asked for -- the Python argument
checks, and the flag of examples/extract_mesh.py."""
import ctypes as C
import importlib.util
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
import mesh_simplify_restate as R

ENTRY_POINTS = ("gsr_simplify_default_origin", "gsr_simplify_cell_keys", "gsr_simplify_run_heads", "gsr_simplify_reduce", "gsr_simplify_face_keys",
                "gsr_simplify_face_unique", "gsr_simplify_vertex_map")


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_case_table_is_the_one_the_tests_name():
    assert sorted(R.cases()) == sorted(R.CASES) and len(R.CASES) == 10


def test_cases_have_the_shapes_they_are_there_for():
    c, ref = R.cases(), R.reference
    for name in R.CASES:
        case = c[name]
        assert case["vertices"].dtype == np.float32 and case["faces"].dtype == np.int32 and case["colors"].dtype == np.float32
        assert case["colors"].shape == case["vertices"].shape
        assert (case["origin"] is None) == (name == "unreferenced_nan"), "only that case leaves the origin to the default"

    r = ref("one_cell_fan_65")
    assert len(c["one_cell_fan_65"]["vertices"]) == 65 > 64 and len(c["one_cell_fan_65"]["faces"]) == 64
    assert r.vertices.shape == (0, 3) and r.faces.shape == (0, 3) and r.colors.shape == (0, 3)
    assert np.all(r.vertex_cluster == -1), "the one cluster has no face left and is dropped"
    cells = np.floor(c["one_cell_fan_65"]["vertices"].astype(np.float64))
    assert np.all(cells == 0), "every vertex of the fan lies in the cell (0, 0, 0)"

    r = ref("run_257")
    assert sorted(len(m) for m in r.members) == [1] * 8 + [257] and 257 > 256
    assert r.faces.shape == (8, 3) and r.kept_faces.tolist() == list(range(8)), "of each triple the earliest face stays"
    assert len(c["run_257"]["faces"]) == 257

    r, coords = ref("boundaries"), R.boundary_coordinates()
    assert np.any(np.signbit(coords) & (coords == 0)) and np.any(~np.signbit(coords) & (coords == 0)) and np.any(coords < 0)
    steps = (coords.astype(np.float64) - R.BOUNDARY_ORIGIN[0]) / R.BOUNDARY_H
    assert np.sum(steps == np.round(steps)) >= 8, "coordinates at exact multiples of h from the origin"
    assert all(o < coords.min() or o == coords.min() for o in R.BOUNDARY_ORIGIN)
    v = c["boundaries"]["vertices"]
    at = lambda x: int(r.vertex_cluster[int(np.nonzero(coords.view(np.int32) == np.float32(x).view(np.int32))[0][0])])  # noqa: E731
    f = np.float32
    # both zeros, 0.1 and the subnormal below zero (which the float64 subtraction absorbs) share the cell that starts at 0
    assert at(-0.0) == at(0.0) == at(0.1) == at(np.nextafter(f(0), f(1))) == at(np.nextafter(f(0), f(-1)))
    for edge in (-1.25, -0.25, 0.25, 1.0):                            # half-open: the edge belongs to the cell above it
        assert at(edge) != at(np.nextafter(f(edge), f(-2))), edge
    assert at(-1.5) == at(np.nextafter(f(-1.5), f(2))) == at(-1.4) == 0, "the origin itself is in cell 0"
    assert len(v) == 3 * len(coords) and 0 < len(r.vertices) < len(v)

    same, opposite = ref("dup_same"), ref("dup_opposite")
    assert same.kept_faces.tolist() == [0, 2] and opposite.kept_faces.tolist() == [0, 1, 2]
    assert R.rotate(tuple(opposite.faces[0])) == (0, 1, 2) and R.rotate(tuple(opposite.faces[1])) == (0, 2, 1)
    assert same.vertex_cluster.tolist() == [0, 0, 1, 2, 3]

    r = ref("orphan_cluster")
    assert r.vertex_cluster.tolist() == [0, -1, -1, 2, 3, 1], "the cluster in the middle is dropped, the later ones move down"
    assert r.faces.tolist() == [[0, 2, 3], [2, 1, 3]] and r.kept_faces.tolist() == [1, 2]

    case, r = c["unreferenced_nan"], ref("unreferenced_nan")
    unreferenced = sorted(set(range(len(case["vertices"]))) - set(case["faces"].reshape(-1).tolist()))
    assert len(unreferenced) == 6 and unreferenced[0] == 0 and unreferenced[-1] == len(case["vertices"]) - 1
    assert not np.isfinite(case["vertices"][unreferenced]).all() and np.all(r.vertex_cluster[unreferenced] == -1)
    assert np.isfinite(case["vertices"][unreferenced]).all(axis=1).any(), "one of them is finite and far below the mesh"
    keep = np.setdiff1d(np.arange(len(case["vertices"])), unreferenced)
    rename = np.cumsum(np.isin(np.arange(len(case["vertices"])), keep)) - 1
    bare = R.simplify(case["vertices"][keep], rename[case["faces"]], case["colors"][keep], voxel_size=case["voxel_size"])
    assert np.array_equal(bare.vertices.view(np.int32), r.vertices.view(np.int32)) and np.array_equal(bare.faces, r.faces)
    assert np.array_equal(bare.colors.view(np.int32), r.colors.view(np.int32)) and np.array_equal(bare.origin, r.origin)
    assert len(r.faces) > 0 and max(len(m) for m in r.members) == 2 and np.isfinite(r.colors).all()

    case, r = c["identity_small_h"], ref("identity_small_h")
    referenced = np.unique(case["faces"])
    assert all(len(m) == 1 for m in r.members) and len(r.vertices) == len(referenced) < len(case["vertices"])
    assert len(r.faces) == len(case["faces"])
    order = [m[0] for m in r.members]
    assert sorted(order) == referenced.tolist() and order != referenced.tolist(), "key order, not vertex order"
    assert np.array_equal(r.vertices.view(np.int32), case["vertices"][order].view(np.int32)), "bit-copies"
    assert np.array_equal(r.colors.view(np.int32), case["colors"][order].view(np.int32))
    assert np.signbit(case["vertices"][7, 0]) and np.signbit(r.vertices[r.vertex_cluster[7], 0]), "-0.0 stays -0.0"

    case, r = c["grid_70k"], ref("grid_70k")
    assert len(case["vertices"]) == 265 * 265 == 70225 > 65536 and len(case["faces"]) == 139392 > 65536
    assert len(r.vertices) == 133 * 133 and max(len(m) for m in r.members) == 4 and 0 < len(r.faces) < len(case["faces"])

    case, r = c["sphere_tsdf"], ref("sphere_tsdf")
    assert len(case["vertices"]) > 3000 and len(case["faces"]) > 6000 and case["voxel_size"] == 2.0
    assert 0 < len(r.faces) < len(case["faces"]) / 4 and 0 < len(r.vertices) < len(case["vertices"]) / 4
    on_boundary = (case["vertices"].astype(np.float64) / 2.0) % 1.0 == 0
    assert on_boundary.any(axis=1).sum() > 500, "many vertices of a TSDF mesh lie exactly on a cell boundary"


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_keeps_its_invariants(name):
    case, r = R.cases()[name], R.reference(name)
    h, V = case["voxel_size"], len(case["vertices"])
    Vk, Fk = len(r.vertices), len(r.faces)
    assert r.vertices.dtype == np.float32 and r.faces.dtype == np.int32 and r.vertex_cluster.dtype == np.int32
    assert r.vertices.shape == (Vk, 3) and r.faces.shape == (Fk, 3) and r.colors.shape == (Vk, 3)
    assert r.vertex_cluster.shape == (V,)
    if Vk:
        # every output vertex lies inside the cell of its members, up to the rounding of the mean to float32
        lo = r.origin + r.cells * h
        slack = 2.0 ** -23 * r.max_abs
        got = r.vertices.astype(np.float64)
        assert np.all(got >= lo - slack) and np.all(got <= lo + h + slack)
        keys = (r.cells[:, 0] << 42) | (r.cells[:, 1] << 21) | r.cells[:, 2]
        assert np.all(np.diff(keys) > 0), "the output vertices ascend in key order"
        for n, group in enumerate(r.members):
            assert np.all(r.vertex_cluster[group] == n) and group == sorted(group)
            assert np.all(np.floor((case["vertices"][group].astype(np.float64) - r.origin) / h) == r.cells[n])
            assert np.all(np.linalg.norm(case["vertices"][group].astype(np.float64) - got[n], axis=1) <= math_sqrt3 * h)
    # no degenerate and no duplicate face, every vertex referenced, the map consistent with the faces
    f = r.faces.astype(np.int64)
    assert np.all((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]))
    assert len(R.rotated_set(f)) == Fk
    assert sorted(set(f.reshape(-1).tolist())) == list(range(Vk))
    referenced = np.zeros(V, dtype=bool)
    referenced[case["faces"].reshape(-1)] = True
    assert np.all(r.vertex_cluster[~referenced] == -1) and np.all(r.vertex_cluster < Vk)
    assert sum(len(m) for m in r.members) == int((r.vertex_cluster >= 0).sum())
    mapped = r.vertex_cluster[case["faces"][r.kept_faces]]
    assert np.array_equal(mapped, r.faces), "a kept face is its input face through the map, corner for corner"
    assert np.all(np.diff(r.kept_faces) > 0)
    # every input face is dropped for a reason
    kept = set(r.kept_faces.tolist())
    seen = set()
    with np.errstate(invalid="ignore", over="ignore"):
        all_cells = [tuple(row) for row in np.floor((case["vertices"].astype(np.float64) - r.origin) / h).tolist()]
    for n, corners in enumerate(case["faces"].tolist()):
        cells = [all_cells[v] for v in corners]
        alive = len(set(cells)) == 3
        t = tuple(cells)
        t = min((t[k:] + t[:k] for k in range(3)))
        assert (n in kept) == (alive and t not in seen), n
        if alive:
            seen.add(t)


math_sqrt3 = 3.0 ** 0.5 * (1 + 2.0 ** -20)


def test_restatement_refuses_what_simplify_mesh_refuses():
    case = R.cases()["dup_same"]
    v, f = case["vertices"], case["faces"]
    bad = v.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        R.simplify(bad, f, voxel_size=1.0)
    with pytest.raises(ValueError, match="face index"):
        R.simplify(v, np.where(f == 4, 5, f), voxel_size=1.0)
    with pytest.raises(ValueError, match="face index"):
        R.simplify(v, np.where(f == 4, -1, f), voxel_size=1.0)
    with pytest.raises(ValueError, match="cell index"):
        R.simplify(v, f, voxel_size=1.0, origin=(0.0, 0.45, 0.0))            # above a vertex
    with pytest.raises(ValueError, match="cell index"):
        R.simplify(v, f, voxel_size=3.3 / 2 ** 21, origin=(0.2, 0.0, 0.0))   # 2^21 cells or more
    assert len(R.simplify(v, f, voxel_size=3.3 / (2 ** 21 - 1), origin=(0.2, 0.0, 0.0)).faces) == 3


# ---- the cell arithmetic on the host -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """``csrc/mesh_simplify_math.h`` -- the arithmetic the key kernel runs -- built by the host compiler from
    ``tests/mesh_simplify_host_check.cpp`` into a program of its own, with the kernels' ``-ffp-contract=off``."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path_factory.mktemp("mesh_simplify_host") / "mesh_simplify_host_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mesh_simplify_host_check.cpp"), "-o", exe], check=True)

    def run(h, origin, coords):
        coords = np.ascontiguousarray(coords, dtype=np.float32)
        out = subprocess.run([exe, float(h).hex(), float(origin).hex()] + [str(int(b)) for b in coords.view(np.uint32)],
                             check=True, capture_output=True, text=True).stdout.split("\n")
        cells = [int(line) for line in out[:len(coords)]]
        keys = [int(line.split()[1]) for line in out[len(coords):] if line.startswith("key")]
        return cells, keys
    return run


def test_host_build_of_the_cell_arithmetic_agrees_with_numpy(host_check):
    coords = R.boundary_coordinates()
    h, o = R.BOUNDARY_H, R.BOUNDARY_ORIGIN[0]
    want = np.floor((coords.astype(np.float64) - o) / h).astype(np.int64)
    cells, keys = host_check(h, o, coords)
    assert cells == want.tolist()
    assert want[coords == 0].tolist() == [6, 6] and want.min() == 0, "both zeros share a cell; the origin itself is cell 0"
    triples = want[:len(coords) // 3 * 3].reshape(-1, 3)
    assert keys == ((triples[:, 0] << 42) | (triples[:, 1] << 21) | triples[:, 2]).tolist()
    # a cell size and an origin that are no float32, coordinates that straddle boundaries by one float32
    h, o = 0.1, -1.0 / 3.0
    edges = np.float32(o + h * np.arange(0, 40, dtype=np.float64))
    coords = np.concatenate((edges, np.nextafter(edges, np.float32(-9)), np.nextafter(edges, np.float32(9))))
    want = np.floor((coords.astype(np.float64) - o) / h)
    cells, _ = host_check(h, o, coords)
    assert cells == [int(w) if w >= 0 else -4 for w in want]
    # refusals: not finite, below the origin, 2^21 cells or more; the last cell is accepted
    f = np.float32
    coords = np.array([np.nan, np.inf, -np.inf, -0.5, 2.0 ** 21, np.nextafter(f(2.0 ** 21), f(0)), 3e38, 0.0, 1.0, 2.0], dtype=f)
    cells, keys = host_check(1.0, 0.0, coords)
    assert cells == [-2, -2, -2, -4, -4, 2 ** 21 - 1, -4, 0, 1, 2]
    assert keys == [-2, -4, -4]


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_simplify_entry_points_and_the_abi_is_at_least_39():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib, mesh
    assert pkg.simplify_mesh is mesh.simplify_mesh and "simplify_mesh" in pkg.__all__ and "simplify_mesh" in mesh.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\bint " + name + r"\(", header), name
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("gsr_simplify_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 39
    for name, bit in (("BAD_INDEX", 1), ("NOT_FINITE", 2), ("OUT_OF_RANGE", 4)):
        assert re.search(rf"GSR_SIMPLIFY_{name} = {bit}\b", header)
    assert "mesh_simplify.o" in open(os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "Makefile")).read()


def test_every_entry_point_refuses_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)
    big = 2 ** 31
    BAD, ALIGN = -1, -3

    default = lib.gsr_simplify_default_origin
    good = [p, p, 4, 1.0, p, p]
    assert [n for n in (0, 1, 4, 5) if default(*(good[:n] + [None] + good[n + 1:]), None) != BAD] == []
    for V in (0, -1, big):
        assert default(p, p, V, 1.0, p, p, None) == BAD
    for h in (0.0, -1.0, float("nan"), float("inf")):
        assert default(p, p, 4, h, p, p, None) == BAD, h
    assert default(p + 2, p, 4, 1.0, p, p, None) == ALIGN and default(p, p + 1, 4, 1.0, p + 2, p, None) == ALIGN
    assert default(p, p, 4, 1.0, p, p + 4, None) == ALIGN                # origin: doubles

    keys = lib.gsr_simplify_cell_keys
    good = [p, p, 4, p, 1.0, p, p]
    assert [n for n in (0, 1, 3, 5, 6) if keys(*(good[:n] + [None] + good[n + 1:]), None) != BAD] == []
    for V in (0, -1, big):
        assert keys(p, p, V, p, 1.0, p, p, None) == BAD
    for h in (0.0, -1.0, float("nan"), float("inf")):
        assert keys(p, p, 4, p, h, p, p, None) == BAD, h
    assert b"voxel_size" in lib.gsr_last_error()
    assert keys(p + 2, p, 4, p, 1.0, p, p, None) == ALIGN
    assert keys(p, p + 1, 4, p, 1.0, p, p + 2, None) == ALIGN            # the marks may sit anywhere; status may not
    assert keys(p, p, 4, p + 4, 1.0, p, p, None) == ALIGN                # origin: doubles
    assert keys(p, p, 4, p, 1.0, p + 4, p, None) == ALIGN                # keys: int64

    heads = lib.gsr_simplify_run_heads
    assert heads(None, 4, p, None) == BAD and heads(p, 4, None, None) == BAD
    assert heads(p, 0, p, None) == BAD and heads(p, big, p, None) == BAD
    assert heads(p + 4, 4, p, None) == ALIGN

    reduce = lib.gsr_simplify_reduce
    good = [p, p, p, p, p, 8, 4, p, p, p, p, p]
    for n in (0, 2, 3, 4, 7, 8, 10, 11):                                 # every required pointer
        assert reduce(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    assert reduce(*(good[:1] + [None] + good[2:]), None) == BAD          # colours without out_colors and the reverse
    assert reduce(*(good[:9] + [None] + good[10:]), None) == BAD
    for V, K in ((0, 1), (big, 1), (8, 0), (8, 9)):
        assert reduce(*(good[:5] + [V, K] + good[7:]), None) == BAD, (V, K)
    for n, off in ((0, 2), (1, 2), (7, 2), (8, 2), (9, 2), (10, 2), (11, 2), (2, 4), (3, 4), (4, 4)):
        assert reduce(*(good[:n] + [p + off] + good[n + 1:]), None) == ALIGN, n

    fkeys = lib.gsr_simplify_face_keys
    good = [p, p, 4, 8, 4, p, p, p, p, p]
    for n in (0, 1, 5, 6, 7, 8, 9):
        assert fkeys(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    for F, V, K in ((0, 8, 4), (big, 8, 4), (4, 0, 1), (4, big, 4), (4, 8, 0), (4, 8, 9)):
        assert fkeys(p, p, F, V, K, p, p, p, p, p, None) == BAD, (F, V, K)
    for n, off in ((0, 2), (1, 2), (5, 2), (8, 2), (9, 2), (7, 4)):
        assert fkeys(*(good[:n] + [p + off] + good[n + 1:]), None) == ALIGN, n

    unique = lib.gsr_simplify_face_unique
    good = [p, p, p, 4, p, p]
    for n in (0, 1, 2, 4, 5):
        assert unique(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    assert unique(p, p, p, 0, p, p, None) == BAD and unique(p, p, p, big, p, p, None) == BAD
    for n, off in ((0, 4), (1, 4), (2, 2), (5, 2)):
        assert unique(*(good[:n] + [p + off] + good[n + 1:]), None) == ALIGN, n

    vmap = lib.gsr_simplify_vertex_map
    good = [p, p, p, 8, 4, p]
    for n in (0, 1, 2, 5):
        assert vmap(*(good[:n] + [None] + good[n + 1:]), None) == BAD, n
    for V, K in ((0, 1), (big, 1), (8, 0), (8, 9)):
        assert vmap(p, p, p, V, K, p, None) == BAD
    for n, off in ((0, 2), (2, 4), (5, 2)):
        assert vmap(*(good[:n] + [p + off] + good[n + 1:]), None) == ALIGN, n


# ---- Python argument checks ------------------------------------------------------------------------------------------------
def test_python_refusals_come_before_a_gpu_is_asked_for():
    from mvs_gaussian_splatting_amd import _lib, simplify_mesh
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    vertices = torch.zeros(4, 3)
    for bad in (faces.long(), faces.float(), faces.reshape(-1), faces[:, :2], faces.numpy(), None, faces.to("meta")):
        with pytest.raises(ValueError):
            simplify_mesh(vertices, bad, voxel_size=1.0)
    for bad in (vertices.double(), torch.zeros(4, 2), torch.zeros(12), vertices.numpy(), None):
        with pytest.raises(ValueError):
            simplify_mesh(bad, faces, voxel_size=1.0)
    with pytest.raises(ValueError):
        simplify_mesh(torch.zeros(0, 3), faces, voxel_size=1.0)           # faces without vertices
    for bad in (torch.zeros(3, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 4), torch.zeros(4, 3, device="meta")):
        with pytest.raises(ValueError):
            simplify_mesh(vertices, faces, bad, voxel_size=1.0)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), True, None, "1", 10 ** 400, torch.tensor(1.0)):
        with pytest.raises(ValueError, match="voxel_size"):
            simplify_mesh(vertices, faces, voxel_size=bad)
    with pytest.raises(TypeError):
        simplify_mesh(vertices, faces)                                    # voxel_size has no default
    with pytest.raises(TypeError):
        simplify_mesh(vertices, faces, None, 1.0)                         # and is given by keyword
    for bad in ((0.0, 1.0), (0.0, 1.0, 2.0, 3.0), (0.0, 1.0, float("nan")), (0.0, float("-inf"), 0.0), 5.0, "abc",
                (0.0, None, 0.0)):
        with pytest.raises(ValueError, match="origin"):
            simplify_mesh(vertices, faces, voxel_size=1.0, origin=bad)
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="return_map"):
            simplify_mesh(vertices, faces, voxel_size=1.0, return_map=bad)
    # well-formed arguments on the CPU: no CPU path, and no quiet fallback
    for kw in ({}, {"origin": (0.0, -1.0, 2.5)}, {"origin": np.zeros(3), "return_map": True}, {"origin": [-1, -1, -1]}):
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            simplify_mesh(vertices, faces, torch.zeros(4, 3), voxel_size=0.5, **kw)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        simplify_mesh(vertices, faces[:0], voxel_size=2)


def test_docstring_says_what_vertex_clustering_does_not_preserve():
    from mvs_gaussian_splatting_amd import simplify_mesh
    doc = " ".join(simplify_mesh.__doc__.split())
    assert "manifoldness" in doc and "closedness" in doc and "sqrt(3) * voxel_size" in doc


# ---- the example -------------------------------------------------------------------------------------------------------
def _example():
    spec = importlib.util.spec_from_file_location("example_extract_mesh_simplify", os.path.join(ROOT, "examples", "extract_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _stub(mod, monkeypatch, calls):
    """A stub scene, renderer and volume: every call the example makes is recorded by name."""
    mesh = ("vertices", "faces", "colors")
    named = lambda sizes, suffix: tuple(types.SimpleNamespace(shape=(n, 3), name=m + suffix)           # noqa: E731
                                        for n, m in zip(sizes, mesh))

    class Volume:
        dims, voxel_size, sdf_trunc = (4, 4, 4), 0.5, 2.0

        def extract_mesh(self, *a, **kw):
            calls.append(("extract_mesh", a, kw))
            return named((8, 12, 8), "")

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
    monkeypatch.setattr(mod, "clean_mesh", record("clean_mesh", named((5, 6, 5), "_post")))
    monkeypatch.setattr(mod, "simplify_mesh", record("simplify_mesh", named((2, 3, 2), "_small")))
    monkeypatch.setattr(mod, "torch", types.SimpleNamespace(no_grad=torch.no_grad, float32=torch.float32,
                                                            tensor=lambda *a, **kw: "background"))
    monkeypatch.setattr(mod, "ModelParams", lambda **kw: types.SimpleNamespace(sh_degree=3, white_background=False, **kw))


def test_example_simplifies_after_the_cleaning_and_without_the_flag_does_what_it_did(monkeypatch, tmp_path, capsys):
    mod = _example()
    base = ["-m", str(tmp_path), "-s", "dataset", "--resolution", "32"]
    calls = []
    _stub(mod, monkeypatch, calls)
    mod.main(base)
    plain = list(calls)
    assert [c[0] for c in plain] == ["Scene", "volume_for_points", "fuse_views", "extract_mesh", "write_ply_mesh"]
    assert "simplified" not in capsys.readouterr().out
    mod.main(base + ["--num_cluster", "50"])
    cleaned = list(calls[5:])
    assert [c[0] for c in cleaned] == plain_names(plain) + ["clean_mesh", "write_ply_mesh"]
    capsys.readouterr()
    folder = os.path.join(str(tmp_path), "mesh", "iteration_7")

    del calls[:]
    mod.main(base + ["--simplify_voxel", "0.25"])
    assert calls[:5] == plain, "the raw mesh is extracted and written exactly as without the flag"
    assert calls[5] == ("simplify_mesh", ("vertices", "faces", "colors"), {"voxel_size": 0.25})
    small = os.path.join(folder, "tsdf_mesh_simplified.ply")
    assert calls[6] == ("write_ply_mesh", (small, "vertices_small", "faces_small", "colors_small"), {}) and len(calls) == 7
    out = capsys.readouterr().out
    assert "8 vertices, 12 faces" in out and "2 of 8 vertices, 3 of 12 faces" in out

    del calls[:]
    mod.main(base + ["--num_cluster", "50", "--simplify_voxel", "0.25"])
    assert calls[:7] == cleaned, "the cleaned mesh is made and written exactly as without the flag"
    assert calls[7] == ("simplify_mesh", ("vertices_post", "faces_post", "colors_post"), {"voxel_size": 0.25})
    assert calls[8] == ("write_ply_mesh", (small, "vertices_small", "faces_small", "colors_small"), {}) and len(calls) == 9
    assert "2 of 5 vertices, 3 of 6 faces" in capsys.readouterr().out

    for flags in (["--simplify_voxel", "0"], ["--simplify_voxel", "-1"], ["--simplify_voxel", "nan"],
                  ["--simplify_voxel", "inf"], ["--simplify_voxel", "big"]):
        with pytest.raises(SystemExit):
            mod.main(base + flags)


def plain_names(calls):
    return [c[0] for c in calls]
