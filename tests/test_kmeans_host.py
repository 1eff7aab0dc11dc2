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


@pytest.mark.parametrize("N,K,D", [(40, 1, 1), (60, 70, 3), (50, 33, 4), (40, 100, 9), (30, 50, 45), (20, 40, 64)])
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
