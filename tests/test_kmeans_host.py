"""CPU-side checks of the compression layer (csrc/kmeans.hip, csrc/kmeans_math.h; compress.py): the ABI
and the refusals of the entry points and of the Python functions -- all before a GPU is asked for --, the rule built by
the host compiler (tests/kmeans_host_check.cpp) against the numpy restatement (tests/kmeans_restate.py), and the
container: file round trip, index dtype, payload size, ``decode``'s layout, the N <= K short-cut, SH degree 0."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import kmeans_restate as R
from mvs_gaussian_splatting_amd import compress
from mvs_gaussian_splatting_amd.compress import (CompressedGaussians, compress_model, kmeans, kmeans_assign, kmeans_update,
                                                 load_compressed, save_compressed)

ENTRY_POINTS = ("gsr_kmeans_code_norms", "gsr_kmeans_assign", "gsr_kmeans_assign_valu", "gsr_kmeans_update")
BAD, ALIGN = -1, -3


# ---- ABI and refusals ----------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_points_and_the_abi_versions_agree():
    import mvs_gaussian_splatting_amd as pkg
    from mvs_gaussian_splatting_amd import _lib
    for name in ("kmeans_assign", "kmeans", "compress_model", "CompressedGaussians", "save_compressed", "load_compressed"):
        assert getattr(pkg, name) is getattr(compress, name) and name in pkg.__all__
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SYMBOLS and re.search(r"\bint " + name + r"\(", header), name
    assert sorted(n for n in _lib.SYMBOLS if n.startswith("gsr_kmeans_")) == sorted(ENTRY_POINTS)
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 46
    assert int(re.search(r"#define GSR_KMEANS_MAX_D (\d+)", header).group(1)) == compress.MAX_D == 64
    assert int(re.search(r"#define GSR_KMEANS_MAX_K (\d+)", header).group(1)) == compress.MAX_K == 65536


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    p = (C.addressof(buf) + 255) // 256 * 256
    norms = lib.gsr_kmeans_code_norms
    assert norms(p, 0, 3, p, None) == BAD and norms(p, 65537, 3, p, None) == BAD
    assert norms(p, 4, 0, p, None) == BAD and norms(p, 4, 65, p, None) == BAD
    assert norms(None, 4, 3, p, None) == BAD and norms(p, 4, 3, None, None) == BAD
    assert norms(p + 2, 4, 3, p, None) == ALIGN
    for fn in (lib.gsr_kmeans_assign, lib.gsr_kmeans_assign_valu):
        good = [p, 10, 3, p, p, 4, p, p]
        for n, value, code in ((0, None, BAD), (3, None, BAD), (4, None, BAD), (6, None, BAD), (1, 0, BAD), (1, 2 ** 31, BAD),
                               (2, 0, BAD), (2, 65, BAD), (5, 0, BAD), (5, 65537, BAD), (0, p + 1, ALIGN), (7, p + 2, ALIGN)):
            args = list(good)
            args[n] = value
            assert fn(*args, None) == code, (n, value)
    good = [p, 10, 5, p, p, 4, p, p]
    assert lib.gsr_kmeans_assign_valu(*good, None) == BAD and b"1..4" in lib.gsr_last_error()
    good = [p, p, 10, 3, p, p, p, 4, p, p, p]
    for n, value, code in ((0, None, BAD), (4, None, BAD), (5, None, BAD), (6, None, BAD), (8, None, BAD), (9, None, BAD),
                           (10, None, BAD), (2, 0, BAD), (2, 2 ** 31, BAD), (3, 65, BAD), (7, 65537, BAD), (4, p + 4, ALIGN),
                           (1, p + 2, ALIGN), (10, p + 1, ALIGN)):
        args = list(good)
        args[n] = value
        assert lib.gsr_kmeans_update(*args, None) == code, (n, value)


def test_python_functions_refuse_bad_arguments_and_cpu_tensors():
    from mvs_gaussian_splatting_amd import _lib
    x, cb = torch.zeros(10, 3), torch.zeros(4, 3)
    nan = x.clone()
    nan[3, 1] = float("nan")
    inf = cb.clone()
    inf[0, 0] = float("inf")
    for a, b in ((x.double(), cb), (x, cb.half()), (x[0], cb), (x, cb[:, :2]), (torch.zeros(10, 65), torch.zeros(4, 65)),
                 (x, torch.zeros(65537, 3)), (torch.zeros(0, 3), cb), (nan, cb), (x, inf), (x.numpy(), cb)):
        with pytest.raises(ValueError):
            kmeans_assign(a, b)
    with pytest.raises(ValueError):
        kmeans_assign(torch.zeros(10, 5), torch.zeros(4, 5), path="valu")
    with pytest.raises(ValueError):
        kmeans_assign(x, cb, path="fast")
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        kmeans_assign(x, cb)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        kmeans(x, 4)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        kmeans_update(x, torch.zeros(10, dtype=torch.int32), cb)
    for bad in (dict(K=0), dict(K=65537), dict(K=2.0), dict(K=True), dict(K=4, iters=-1), dict(K=4, seed="0"),
                dict(K=4, weights=torch.ones(9)), dict(K=4, weights=-torch.ones(10)), dict(K=4, weights=torch.ones(10).double()),
                dict(K=4, weights=torch.full((10,), float("nan")))):
        with pytest.raises(ValueError):
            kmeans(x, **bad)
    with pytest.raises(ValueError):
        kmeans(nan, 4)
    with pytest.raises(ValueError):
        kmeans_update(x, torch.zeros(10, dtype=torch.int64), cb)


# ---- the rule: host build against the restatement ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """``csrc/kmeans_math.h`` built by the host compiler from ``tests/kmeans_host_check.cpp`` into a program of its own,
    with the kernel's ``-ffp-contract=off``."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or \
        os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    folder = tmp_path_factory.mktemp("kmeans_host")
    exe = str(folder / "kmeans_host_check")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off",
                    "-I" + os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc"),
                    os.path.join(ROOT, "tests", "kmeans_host_check.cpp"), "-o", exe], check=True)

    def run(x, cb):
        path = str(folder / "case.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<iii", len(x), len(cb), x.shape[1]) + np.ascontiguousarray(x, dtype="<f4").tobytes()
                    + np.ascontiguousarray(cb, dtype="<f4").tobytes())
        rows = [ln.split() for ln in subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()]
        ints = np.array([[int(v) for v in w[:3]] for w in rows], dtype=np.int32).reshape(-1, 3)
        words = np.array([[int(v, 16) for v in w[3:]] for w in rows], dtype=np.uint32).reshape(-1, 3)
        return ints, words
    return run


@pytest.mark.parametrize("N,K,D", [(40, 1, 1), (60, 70, 3), (50, 33, 4), (40, 100, 9), (30, 50, 45), (20, 40, 64),
                                   (30, 40, 17), (30, 40, 24), (30, 40, 32), (30, 40, 33)])
def test_host_build_of_the_rule_gives_the_restatements_bits(host_check, N, K, D):
    rng = np.random.default_rng(100 * K + D)
    x = (rng.standard_normal((N, D)) * 10.0 ** rng.uniform(-2, 2, size=(N, 1))).astype(np.float32)
    cb = (rng.standard_normal((K, D)) * 10.0 ** rng.uniform(-2, 2, size=(K, 1))).astype(np.float32)
    cb[: K // 2] = x[rng.integers(0, N, size=K // 2)]                    # exact hits: dist2 clamps at 0
    cb = np.concatenate((cb, cb[: (K + 1) // 2]))                        # ties: duplicates at a higher index
    ints, words = host_check(x, cb)
    index, dist2 = R.assign(x, cb)
    best = R.scores(x, cb)[np.arange(N), index]
    assert np.array_equal(ints[:, 0], index), "the rule's index"
    assert np.array_equal(ints[:, 1], index) and np.array_equal(ints[:, 2], index), "padding to even D / the merge of halves"
    assert ints.max() < K, "a duplicate at the higher index was chosen"
    assert np.array_equal(words[:, 0], best.view(np.uint32)) and np.array_equal(words[:, 1], best.view(np.uint32))
    assert np.array_equal(words[:, 2], dist2.view(np.uint32))
    hit = (x[:, None, :] == cb[None, :, :]).all(axis=2).any(axis=1)
    assert (hit.any() or K == 1) and (dist2[hit] == 0).all() and (dist2 >= 0).all()


def test_fma32_is_correctly_rounded():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(2000).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        got = Fraction(float(R.fma32(a[i], b[i], c[i])))
        lo, hi = np.nextafter(np.float32(got), np.float32(-np.inf)), np.nextafter(np.float32(got), np.float32(np.inf))
        assert abs(exact - got) <= abs(exact - Fraction(float(lo))) and abs(exact - got) <= abs(exact - Fraction(float(hi)))


# ---- the premises of the GPU tests' inputs (kmeans_restate.py), checked on the restatement -----------------------------------
def _host_permutation(N, seed):
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    return torch.randperm(N, generator=gen)


def _dispatch_of_the_matrix_core_kernel():
    """[(largest D, STEPS)] read from gsr_kmeans_assign in csrc/kmeans.hip, the last entry for every larger D."""
    with open(os.path.join(ROOT, "mvs_gaussian_splatting_amd", "csrc", "kmeans.hip")) as f:
        body = f.read().split("int gsr_kmeans_assign(", 1)[1].split("#undef GSR_KMEANS_LAUNCH", 1)[0]
    table = [(int(d), int(s)) for d, s in re.findall(r"if \(D <= (\d+)\) GSR_KMEANS_LAUNCH\((\d+)\);", body)]
    table.append((compress.MAX_D, int(re.search(r"\belse GSR_KMEANS_LAUNCH\((\d+)\);", body).group(1))))
    return table


def test_every_assignment_edge_case_reaches_the_instantiation_it_is_listed_for():
    table = _dispatch_of_the_matrix_core_kernel()
    assert table == [(4, 2), (16, 8), (32, 16), (48, 24), (64, 32)], "the dispatch moved: the edge cases are to move with it"
    steps_of = lambda D: next(s for d, s in table if D <= d)                                      # noqa: E731
    for N, K, D, steps, why in R.ASSIGN_EDGE_CASES:
        assert steps_of(D) == steps and 2 * steps >= D, (N, K, D, why)
    reached = {steps_of(D) for _, _, D, _, _ in R.ASSIGN_EDGE_CASES}
    assert reached == {s for _, s in table}, "an instantiation without an edge case"
    Ds = {D for _, _, D, _, _ in R.ASSIGN_EDGE_CASES}
    # (D = 48 is among the first ten cases of tests/test_gpu_kmeans.py)
    assert {d for d, _ in table[:-1]} | {d + 1 for d, _ in table[:-1]} <= Ds | {48}, "both sides of every threshold on D"
    ends = {((N - 1) % 256 // 64, (N - 1) % 64 // 32) for N, _, _, _, _ in R.ASSIGN_EDGE_CASES}      # (wave, tile) of the last point
    assert {(1, 1), (2, 1), (3, 0), (0, 0), (0, 1), (3, 1)} <= ends
    Ks = {K for _, K, _, _, _ in R.ASSIGN_EDGE_CASES}
    assert {128, 256, 129} <= Ks and all(1 <= K <= compress.MAX_K and N * K * D <= 3.5e7 for N, K, D, _, _ in R.ASSIGN_EDGE_CASES)
    assert len({c[:3] for c in R.ASSIGN_EDGE_CASES}) == len(R.ASSIGN_EDGE_CASES)


def test_largest_codebook_case_has_its_copies_where_it_says():
    x, cb, rows, codes = R.largest_codebook_case()
    assert cb.shape == (compress.MAX_K, 3) and x.shape == (97, 3) and len(set(rows)) == len(rows) == len(codes) == 8
    assert list(codes) == [65535, 65534, 65408, 65407, 32768, 127, 128, 0] and 65408 % 128 == 0
    assert np.array_equal(x[rows].view(np.uint32), cb[codes].view(np.uint32))
    assert len(np.unique(cb.view(np.uint32), axis=0)) == len(cb), "two equal codes: the copy of the higher one would lose"
    index, dist2 = R.assign(x, cb)
    assert np.array_equal(index[rows], codes) and (dist2[rows] == 0).all() and index.max() == 65535


def test_trajectory_input_has_duplicates_in_its_init_an_empty_code_and_codebooks_that_move():
    x, w, K, iters, seed = R.trajectory_input()
    assert x.shape == (1500, 6) and (K, iters) == (40, 5) and w.min() == 0 and w.max() <= 3
    assert len(x) - len(np.unique(x.view(np.uint32), axis=0)) == 300 and 0.07 <= (w == 0).mean() <= 0.13
    perm = _host_permutation(len(x), seed).numpy()
    first = R.first_distinct(x, perm, K)
    assert len(first) == K and not np.array_equal(first, perm[:K]), "the init meets no duplicate"
    assert len(np.unique(x[first].view(np.uint32), axis=0)) == K
    for weights in (None, w):
        books, index, empties, dist2s = R.lloyd(x, first, iters, weights)
        assert len(books) == len(dist2s) == iters + 1 and len(empties) == iters and np.array_equal(books[0], x[first])
        assert np.array_equal(index, R.assign(x, books[-1])[0])
        assert sum(not np.array_equal(books[t], books[t + 1]) for t in range(iters)) >= 2
        if weights is not None:
            assert min(empties) >= 1, "no code without weight in the weighted run"
    books0, index0, empties0, _ = R.lloyd(x, first, 0)
    assert len(books0) == 1 and empties0 == [] and np.array_equal(index0, R.assign(x, x[first])[0])


def test_init_input_sends_the_init_round_its_loop_again_and_the_host_init_is_the_restatements():
    x, seed = R.init_input()
    perm = _host_permutation(len(x), seed)
    assert len(np.unique(x.view(np.uint32), axis=0)) == 90 and len(x) == 5000
    assert len(np.unique(x[perm.numpy()[:64]].view(np.uint32), axis=0)) < 64, "the first chunk of 64 would do"
    assert len(np.unique(x[perm.numpy()[:64 + 128]].view(np.uint32), axis=0)) < 90, "K = 128 would be done after two chunks"
    for K, rows in ((64, 64), (128, 90), (1, 1), (90, 90)):
        want = R.first_distinct(x, perm.numpy(), K)
        assert len(want) == rows and len(np.unique(x[want].view(np.uint32), axis=0)) == rows
        order = np.argsort(perm.numpy())                       # the position of every row in the permutation
        assert (np.diff(order[want]) > 0).all(), "not in the order of the permutation"
        assert np.array_equal(compress._distinct_rows(torch.from_numpy(x), perm, K).numpy(), want), K     # torch ops only


def test_update_input_has_its_runs_on_workgroup_edges():
    x, index, cb, w = R.workgroup_edge_update_input()
    assert len(x) == len(index) == len(w) == 768 and cb.shape == (5, x.shape[1]) and (w > 0).all()
    assert np.array_equal(np.flatnonzero(np.diff(index)) + 1, [256, 512]) and sorted(set(index)) == [0, 1, 3]
    assert R.update(x, index, cb)[1] == R.update(x, index, cb, w)[1] == 2


# ---- the container -----------------------------------------------------------------------------------------------------------
def _model_dict(P, degree, seed=0):
    g = torch.Generator().manual_seed(seed)
    k = (degree + 1) ** 2 - 1
    r = lambda *s: torch.randn(*s, generator=g)                                                   # noqa: E731
    return {"_xyz": r(P, 3), "_features_dc": r(P, 1, 3), "_features_rest": r(P, k, 3), "_opacity": r(P, 1),
            "_scaling": r(P, 3), "_rotation": r(P, 4), "active_sh_degree": degree}


def _direct(P, K, degree=1, seed=0):
    rng = np.random.default_rng(seed)
    k = 3 * ((degree + 1) ** 2 - 1)
    vq = lambda D: {"codebook": rng.standard_normal((K, D)).astype(np.float32),               # noqa: E731
                    "index": rng.integers(0, K, size=P).astype(np.int32)}
    groups = {"f_dc": vq(3), "scaling": {"half": rng.standard_normal((P, 3)).astype(np.float16)}, "rotation": vq(4)}
    if degree:
        groups["f_rest"] = vq(k)
    return CompressedGaussians(degree, rng.standard_normal((P, 3)).astype(np.float32),
                               rng.standard_normal((P, 1)).astype(np.float16), groups)


def test_npz_round_trip_is_bit_for_bit(tmp_path):
    cg = _direct(300, 50)
    path = str(tmp_path / "sub" / "model_vq.npz")
    save_compressed(path, cg)
    assert os.path.exists(path)
    with np.load(path, allow_pickle=False) as z:
        assert str(z["format"]) == "gsr-vq" and int(z["version"]) == 1 and int(z["sh_degree"]) == 1
        assert sorted(z.files) == sorted(["format", "version", "sh_degree"] + list(cg.arrays()))
    back = load_compressed(path)
    assert back.sh_degree == cg.sh_degree and sorted(back.arrays()) == sorted(cg.arrays())
    for name, a in cg.arrays().items():
        b = back.arrays()[name]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    bogus = str(tmp_path / "other.npz")
    np.savez(bogus, xyz=np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="gsr-vq"):
        load_compressed(bogus)


@pytest.mark.parametrize("K,dtype", [(65536, np.uint16), (65537, np.int32)])
def test_index_dtype_at_the_16_bit_boundary(K, dtype):
    cg = _direct(100, K, degree=0)
    cg.groups["f_dc"]["index"][:] = K - 1
    for name in ("f_dc", "rotation"):
        assert cg.groups[name]["index"].dtype == dtype
    cg = CompressedGaussians(0, cg.xyz, cg.opacity, {n: dict(g) for n, g in cg.groups.items()})
    assert int(cg.groups["f_dc"]["index"][0]) == K - 1
    dec = cg.decode("cpu")
    assert np.array_equal(dec["_features_dc"][:, 0].numpy(), cg.groups["f_dc"]["codebook"][K - 1][None].repeat(100, 0))
    with pytest.raises(ValueError):
        bad = {n: dict(g) for n, g in cg.groups.items()}
        bad["f_dc"]["index"] = np.full(100, K, dtype=np.int32)
        CompressedGaussians(0, cg.xyz, cg.opacity, bad)


def test_nbytes_is_the_sum_of_size_times_itemsize():
    P, K = 300, 50
    cg = _direct(P, K)
    want = P * 3 * 4 + P * 2 + (K * 3 * 4 + P * 2) + (K * 9 * 4 + P * 2) + P * 3 * 2 + (K * 4 * 4 + P * 2)
    assert cg.nbytes() == want == sum(a.size * a.itemsize for a in cg.arrays().values())


def test_decode_gives_load_plys_keys_shapes_and_dtypes(tmp_path):
    from mvs_gaussian_splatting_amd import ply_io

    class M:
        pass
    m, d = M(), _model_dict(40, 2)
    for k, v in d.items():
        setattr(m, k, v)
    ply = str(tmp_path / "m.ply")
    ply_io.save_ply(m, ply)
    ref = ply_io.load_ply(ply, 2, "cpu")
    cg = compress_model(d, codebook_size=64)                      # 40 <= 64: every group takes the short-cut
    dec = cg.decode("cpu")
    assert list(dec) == list(ref)
    for k in ref:
        if k == "active_sh_degree":
            assert dec[k] == ref[k] == 2
        else:
            assert dec[k].dtype == ref[k].dtype and dec[k].shape == ref[k].shape and dec[k].is_contiguous(), k
    for k in ("_features_dc", "_features_rest", "_scaling"):
        assert torch.equal(dec[k], ref[k]), k
    assert torch.equal(dec["_rotation"], compress.canonical_rotation(ref["_rotation"]))
    assert torch.equal(dec["_xyz"], ref["_xyz"]) and torch.equal(dec["_opacity"], ref["_opacity"].half().float())
    q = dec["_rotation"].double().numpy()
    assert np.allclose(np.linalg.norm(q, axis=1), 1.0, atol=8 * R.U) and (q[:, 0] >= 0).all()
    assert np.allclose(q, R.canonical_rotation(ref["_rotation"].numpy()), atol=8 * R.U)
    half = compress_model(d, codebook_size=64, groups=("f_rest",), xyz_dtype="float16")
    assert half.xyz.dtype == np.float16 and set(half.groups["scaling"]) == {"half"} and set(half.groups["f_rest"]) != {"half"}
    assert torch.equal(half.decode()["_scaling"], ref["_scaling"].half().float())


def test_shortcut_when_there_are_no_more_rows_than_codes():
    x = torch.randn(37, 5, generator=torch.Generator().manual_seed(1))
    for K in (37, 100):
        codebook, index, info = kmeans(x, K, iters=3)
        assert torch.equal(codebook, x) and codebook.data_ptr() != x.data_ptr() and info["shortcut"]
        assert index.dtype == torch.int32 and index.tolist() == list(range(37))


def test_compress_model_on_a_dict_of_sh_degree_0(tmp_path):
    d = _model_dict(25, 0)
    cg = compress_model(d, codebook_size=32)
    assert cg.sh_degree == 0 and "f_rest" not in cg.groups and cg.num_points == 25
    path = str(tmp_path / "deg0.npz")
    save_compressed(path, cg)
    dec = load_compressed(path).decode()
    assert dec["_features_rest"].shape == (25, 0, 3) and dec["_features_rest"].dtype == torch.float32
    assert torch.equal(dec["_features_dc"], d["_features_dc"]) and dec["active_sh_degree"] == 0
    bad = dict(d)
    bad["_scaling"] = d["_scaling"].clone()
    bad["_scaling"][3, 0] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        compress_model(bad)
    for kw in (dict(codebook_size=0), dict(codebook_size=65537), dict(groups=("sh",)), dict(xyz_dtype="bfloat16"),
               dict(weights=torch.ones(24)), dict(iters=-1)):
        with pytest.raises(ValueError):
            compress_model(d, **kw)
    with pytest.raises(ValueError):
        compress_model({"_xyz": d["_xyz"]})


def test_sh_degree_4_is_refused_by_name_before_kmeans_is_entered(monkeypatch):
    """f_rest at SH degree 4 has D = 72 > MAX_D: with f_rest listed (the default) nothing is clustered first."""
    def entered(*a, **k):
        raise AssertionError("kmeans was entered")
    monkeypatch.setattr(compress, "kmeans", entered)
    d = _model_dict(300, 4)
    for kw in (dict(), dict(codebook_size=64), dict(codebook_size=300), dict(groups=("rotation", "f_rest"))):
        with pytest.raises(ValueError) as e:
            compress_model(d, **kw)
        message = str(e.value)
        assert "f_rest" in message and "72" in message and "64" in message and "groups" in message and "float16" in message
    with pytest.raises(AssertionError, match="kmeans was entered"):          # what the patch does to a call that is let through
        compress_model(d, groups=("f_dc",))
    with pytest.raises(AssertionError, match="kmeans was entered"):          # D = 45 at degree 3 is still clustered
        compress_model(_model_dict(300, 3))


def test_sh_degree_4_compresses_with_f_rest_left_as_float16(tmp_path):
    P = 120
    d = _model_dict(P, 4)
    cg = compress_model(d, codebook_size=P, groups=("f_dc", "scaling", "rotation"))          # P <= K: the short-cut, no launch
    assert cg.sh_degree == 4 and set(cg.groups["f_rest"]) == {"half"} and cg.groups["f_rest"]["half"].shape == (P, 72)
    want = d["_features_rest"].reshape(P, 72).half()
    assert np.array_equal(cg.groups["f_rest"]["half"].view(np.uint16), want.numpy().view(np.uint16))
    path = str(tmp_path / "deg4.npz")
    save_compressed(path, cg)
    back = load_compressed(path)
    assert back.sh_degree == 4 and back.groups["f_rest"]["half"].tobytes() == cg.groups["f_rest"]["half"].tobytes()
    dec = back.decode()
    assert dec["_features_rest"].shape == (P, 24, 3) and dec["active_sh_degree"] == 4
    assert torch.equal(dec["_features_rest"], want.float().reshape(P, 24, 3))
    for key in ("_features_dc", "_scaling"):
        assert torch.equal(dec[key], d[key]), key
    assert torch.equal(dec["_rotation"], compress.canonical_rotation(d["_rotation"]))
