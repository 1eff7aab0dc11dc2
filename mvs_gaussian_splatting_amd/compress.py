"""Compressing a trained model: k-means vector quantisation of the per-Gaussian attributes against small codebooks
(Compact3D's grouping; LightGaussian's importance weighting through ``weights``), a compressed container and its ``.npz``
file (csrc/kmeans.hip, csrc/kmeans_math.h).

The assignment rule, one op order for host and device.  For a point ``x[D]`` and a code ``c[D]``::

    dot   = fmaf(x[D-1], c[D-1], ... fmaf(x[1], c[1], fmaf(x[0], c[0], 0.0f)) ...)
    cnorm = the same chain of c with itself
    score = fmaf(-2.0f, dot, cnorm)

The assignment of ``x`` is the code with the smallest score; of equal scores the smallest index wins.  ``dist2`` is
``max(0, xnorm + score)`` with ``xnorm`` the chain of ``x`` with itself: a diagnostic.  The dot products run on the matrix
cores (``v_mfma_f32_32x32x2_f32``, whose accumulator is that chain bit for bit), so the result does not depend on the path;
``tests/kmeans_restate.py`` restates the rule in numpy and bounds its float64 gap to the true nearest code.

The update: indices are sorted stably by ``torch.sort``, run heads found, and every code becomes the float64 mean of its
rows, summed in ascending row index (``sum w x / sum w`` with weights), rounded to float32 once.  A code with no row or
with ``sum w = 0`` keeps its centre.  No float atomics: the same input gives the same bits.

Limits: ``1 <= D <= 64``, ``1 <= K <= 65536``, ``1 <= N < 2^31``.  There is no CPU path for the kernels; the container,
its file and ``decode`` are host code and work anywhere.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_D = 64
MAX_K = 65536
FORMAT_TAG = "gsr-vq"
FORMAT_VERSION = 1
UNIT_TOLERANCE = 8 * 2.0 ** -24     # |1 - |q|| up to which a quaternion counts as unit
GROUPS = ("f_dc", "f_rest", "scaling", "rotation")
_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation"}


# ---- argument checks: everything that can be refused is refused before a launch ------------------------------------------
def _check_rows(t, name: str, cols: Optional[int] = None) -> Tuple[int, int]:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError(f"{name} must be a float32 [N,D] tensor, got {getattr(t, 'dtype', type(t))} "
                         f"{tuple(getattr(t, 'shape', ()))}")
    n, d = int(t.shape[0]), int(t.shape[1])
    if not 1 <= d <= MAX_D:
        raise ValueError(f"{name} has D = {d}; D must lie in 1..{MAX_D}")
    if cols is not None and d != cols:
        raise ValueError(f"{name} has D = {d}, expected {cols}")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"{name} has {n} rows; the count must lie in 1..2^31-1")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} holds a value that is not finite")
    return n, d


def _check_weights(w, n: int, like: torch.Tensor):
    if w is None:
        return None
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or tuple(w.shape) != (n,):
        raise ValueError(f"weights must be a float32 [{n}] tensor, got {getattr(w, 'dtype', type(w))} "
                         f"{tuple(getattr(w, 'shape', ()))}")
    if w.device != like.device:
        raise ValueError(f"weights must be on the device of the rows ({like.device}), got {w.device}")
    if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError("weights must be finite and not negative")
    return w.detach().contiguous()


def _check_int(v, name: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def _need_gpu(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise _lib.GsrError(f"{name} needs ROCm GPU tensors (no CPU path)")


# ---- the three native steps ----------------------------------------------------------------------------------------------
def _code_norms(lib, codebook: torch.Tensor, stream) -> torch.Tensor:
    K, D = codebook.shape
    cnorm = torch.empty(K, dtype=torch.float32, device=codebook.device)
    _lib.check(lib.gsr_kmeans_code_norms(codebook.data_ptr(), K, D, cnorm.data_ptr(), stream), "gsr_kmeans_code_norms")
    return cnorm


def _assign(lib, x: torch.Tensor, codebook: torch.Tensor, stream, path: Optional[str] = None):
    N, D = x.shape
    cnorm = _code_norms(lib, codebook, stream)
    index = torch.empty(N, dtype=torch.int32, device=x.device)
    dist2 = torch.empty(N, dtype=torch.float32, device=x.device)
    fn, what = (lib.gsr_kmeans_assign_valu, "gsr_kmeans_assign_valu") if path == "valu" else \
        (lib.gsr_kmeans_assign, "gsr_kmeans_assign")
    _lib.check(fn(x.data_ptr(), N, D, codebook.data_ptr(), cnorm.data_ptr(), int(codebook.shape[0]), index.data_ptr(),
                  dist2.data_ptr(), stream), what)
    return index, dist2


def _update(lib, x: torch.Tensor, weights, index: torch.Tensor, codebook: torch.Tensor, counters: torch.Tensor, stream):
    N, D = x.shape
    K = int(codebook.shape[0])
    # stable, so that the rows of a code stay in ascending row index (plumbing: stays in torch, as in mesh.simplify_mesh)
    keys_sorted, order = torch.sort(index.to(torch.int64), stable=True)
    head = torch.empty(N, dtype=torch.uint8, device=x.device)
    _lib.check(lib.gsr_simplify_run_heads(keys_sorted.data_ptr(), N, head.data_ptr(), stream), "gsr_simplify_run_heads")
    runs = torch.empty(2 * K, dtype=torch.int32, device=x.device)
    _lib.check(lib.gsr_kmeans_update(x.data_ptr(), None if weights is None else weights.data_ptr(), N, D,
                                     keys_sorted.data_ptr(), order.data_ptr(), head.data_ptr(), K, runs.data_ptr(),
                                     codebook.data_ptr(), counters.data_ptr(), stream), "gsr_kmeans_update")


def kmeans_assign(x: torch.Tensor, codebook: torch.Tensor, path: Optional[str] = None):
    """-> ``(index int32 [N], dist2 float32 [N])``: the code of every row of ``x`` (float32 ``[N,D]``) in ``codebook``
    (float32 ``[K,D]``, same device) by the module's rule.  ``path``: None for the matrix-core kernel, ``"valu"`` for the
    vector-ALU kernel (``D <= 4``; the same bits, a cross-check).  Refused with ``ValueError``: a wrong dtype or shape,
    ``D > 64``, ``K > 65536``, a value that is not finite; with ``GsrError``: CPU tensors."""
    N, D = _check_rows(x, "x")
    K, _ = _check_rows(codebook, "codebook", D)
    if K > MAX_K:
        raise ValueError(f"codebook has {K} rows; K must lie in 1..{MAX_K}")
    if path not in (None, "mfma", "valu") or (path == "valu" and D > 4):
        raise ValueError(f"path must be None, 'mfma' or (for D <= 4) 'valu', got {path!r} at D = {D}")
    if codebook.device != x.device:
        raise ValueError(f"codebook must be on the device of x ({x.device}), got {codebook.device}")
    _need_gpu(x, "kmeans_assign")
    lib = _lib.load()
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        return _assign(lib, x.detach().contiguous(), codebook.detach().contiguous(), stream, path)


def kmeans_update(x: torch.Tensor, index: torch.Tensor, codebook: torch.Tensor, weights: Optional[torch.Tensor] = None):
    """One centre update -> ``(codebook' float32 [K,D], empty int)``: every code with rows becomes the float64 mean of its
    rows in ascending row index (``sum w x / sum w`` with ``weights``), rounded to float32 once; a code with no row or
    with ``sum w = 0`` keeps its centre and is counted in ``empty``.  ``index``: int32 ``[N]`` in ``0..K-1``."""
    N, D = _check_rows(x, "x")
    K, _ = _check_rows(codebook, "codebook", D)
    if K > MAX_K:
        raise ValueError(f"codebook has {K} rows; K must lie in 1..{MAX_K}")
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or tuple(index.shape) != (N,):
        raise ValueError(f"index must be an int32 [{N}] tensor")
    if index.device != x.device or codebook.device != x.device:
        raise ValueError("x, index and codebook must be on one device")
    weights = _check_weights(weights, N, x)
    _need_gpu(x, "kmeans_update")
    lib = _lib.load()
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        out = codebook.detach().clone().contiguous()
        counters = torch.zeros(2, dtype=torch.int32, device=x.device)
        _update(lib, x.detach().contiguous(), weights, index.contiguous(), out, counters, stream)
        empty, bad = counters.tolist()
    if bad:
        raise _lib.GsrError(f"kmeans_update: an index lies outside 0..{K - 1}")
    return out, empty


def _distinct_rows(x: torch.Tensor, perm: torch.Tensor, K: int) -> torch.Tensor:
    """The first ``K`` entries of ``perm`` whose rows of ``x`` differ bit for bit from every earlier chosen row (fewer if
    ``x`` has fewer distinct rows).  Two equal initial codes would leave the one of higher index without rows for good:
    ties go to the smaller index and an empty code keeps its centre.  Walks ``perm`` in chunks that double."""
    N = int(perm.shape[0])
    chosen = perm[:0]
    pos, chunk = 0, K
    while chosen.shape[0] < K and pos < N:
        cand = torch.cat((chosen, perm[pos:pos + chunk]))
        pos, chunk = pos + chunk, 2 * chunk
        bits = x.index_select(0, cand).view(torch.int32)
        _, inverse = torch.unique(bits, dim=0, return_inverse=True)
        slot = torch.arange(cand.shape[0], device=x.device)
        first = torch.full((int(inverse.max()) + 1,), cand.shape[0], dtype=torch.int64, device=x.device)
        first.scatter_reduce_(0, inverse, slot, reduce="amin")                 # the first slot of every distinct row
        chosen = cand.index_select(0, torch.sort(first).values[:K])
    return chosen


def kmeans(x: torch.Tensor, K: int, iters: int = 10, weights: Optional[torch.Tensor] = None, seed: int = 0,
           history: bool = False):
    """Lloyd's k-means -> ``(codebook float32 [K',D], index int32 [N], info)``.

    Init: the first ``K`` rows, in the order of ``torch.randperm(N)`` of a CPU generator seeded with ``seed``, that differ
    bit for bit from the rows taken before them; ``K'`` is smaller than ``K`` only when ``x`` has fewer distinct rows.  If
    ``N <= K`` the codebook is the rows themselves, ``K' = N`` and ``index = arange(N)`` (no launch; works on any device).  Each of
    the ``iters`` iterations runs norms, assign, update; a last assign follows the last update.  ``info``:
    ``"objective"``, the float64 sum of ``dist2`` of every assign (``iters + 1`` values, the last one the returned
    state's); ``"empty"``, per iteration the number of codes that kept their centre; with ``history=True`` also
    ``"codebooks"``, the ``iters + 1`` codebooks on the host (the one each assign ran against).  One read-back, at the
    end."""
    N, D = _check_rows(x, "x")
    K = _check_int(K, "K", 1, MAX_K)
    iters = _check_int(iters, "iters", 0, 10 ** 6)
    seed = _check_int(seed, "seed", -2 ** 63, 2 ** 63 - 1)
    weights = _check_weights(weights, N, x)
    xc = x.detach().contiguous()
    if N <= K:
        info = {"objective": [0.0], "empty": [], "shortcut": True}
        if history:
            info["codebooks"] = [xc.cpu().numpy().copy()]
        return xc.clone(), torch.arange(N, dtype=torch.int32, device=x.device), info
    _need_gpu(x, "kmeans")
    lib = _lib.load()
    gen = torch.Generator(device="cpu")
    gen.manual_seed(seed)
    first = _distinct_rows(xc, torch.randperm(N, generator=gen).to(x.device), K)
    K = int(first.shape[0])
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        codebook = xc.index_select(0, first).contiguous()
        counters = torch.zeros((max(iters, 1), 2), dtype=torch.int32, device=x.device)
        objective, books = [], []
        for it in range(iters):
            if history:
                books.append(codebook.clone())
            index, dist2 = _assign(lib, xc, codebook, stream)
            objective.append(dist2.sum(dtype=torch.float64))
            _update(lib, xc, weights, index, codebook, counters[it], stream)
        if history:
            books.append(codebook.clone())
        index, dist2 = _assign(lib, xc, codebook, stream)
        objective.append(dist2.sum(dtype=torch.float64))
        record = torch.cat((torch.stack(objective), counters[:iters].to(torch.float64).reshape(-1))).tolist()  # read-back
    n = iters + 1
    if any(record[n + 1::2]):
        raise _lib.GsrError("kmeans: an index left the range of the codebook")
    info = {"objective": record[:n], "empty": [int(v) for v in record[n::2]], "shortcut": False}
    if history:
        info["codebooks"] = [b.cpu().numpy() for b in books]
    return codebook, index, info


# ---- the container ---------------------------------------------------------------------------------------------------------
def index_dtype(k: int):
    """The dtype indices into a codebook of ``k`` rows are stored in."""
    return np.uint16 if k <= 65536 else np.int32


class CompressedGaussians:
    """A compressed model on the host.  ``groups[name]`` is ``{"codebook": float32 [K',D], "index": uint16 / int32 [P]}``
    or ``{"half": float16 [P,D]}`` for ``name`` in f_dc, f_rest (absent at SH degree 0), scaling, rotation; ``xyz`` is
    float32 or float16 ``[P,3]``, ``opacity`` float16 ``[P,1]`` (raw), all numpy arrays.  Rows are in the model's layout
    flattened: f_dc ``[P,1,3] -> [P,3]``, f_rest ``[P,k,3] -> [P,3k]``."""

    def __init__(self, sh_degree: int, xyz: np.ndarray, opacity: np.ndarray, groups: Dict[str, Dict[str, np.ndarray]]):
        self.sh_degree = _check_int(sh_degree, "sh_degree", 0, 4)
        xyz, opacity = np.ascontiguousarray(xyz), np.ascontiguousarray(opacity)
        P = xyz.shape[0]
        if xyz.dtype not in (np.float32, np.float16) or xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError(f"xyz must be float32 or float16 [P,3], got {xyz.dtype} {xyz.shape}")
        if opacity.dtype != np.float16 or opacity.shape != (P, 1):
            raise ValueError(f"opacity must be float16 [{P},1], got {opacity.dtype} {opacity.shape}")
        want = {"f_dc": 3, "f_rest": 3 * ((self.sh_degree + 1) ** 2 - 1), "scaling": 3, "rotation": 4}
        if self.sh_degree == 0:
            del want["f_rest"]
        if set(groups) != set(want):
            raise ValueError(f"groups must be {sorted(want)}, got {sorted(groups)}")
        self.groups = {}
        for name, g in groups.items():
            D = want[name]
            if set(g) == {"half"}:
                h = np.ascontiguousarray(g["half"])
                if h.dtype != np.float16 or h.shape != (P, D):
                    raise ValueError(f"{name}.half must be float16 [{P},{D}], got {h.dtype} {h.shape}")
                self.groups[name] = {"half": h}
            elif set(g) == {"codebook", "index"}:
                cb, idx = np.ascontiguousarray(g["codebook"]), np.ascontiguousarray(g["index"])
                if cb.dtype != np.float32 or cb.ndim != 2 or cb.shape[1] != D or cb.shape[0] < 1:
                    raise ValueError(f"{name}.codebook must be float32 [K,{D}], got {cb.dtype} {cb.shape}")
                if idx.dtype not in (np.uint16, np.int32) or idx.shape != (P,):
                    raise ValueError(f"{name}.index must be uint16 or int32 [{P}], got {idx.dtype} {idx.shape}")
                if P and (int(idx.min()) < 0 or int(idx.max()) >= cb.shape[0]):
                    raise ValueError(f"{name}.index refers to a code outside 0..{cb.shape[0] - 1}")
                self.groups[name] = {"codebook": cb, "index": idx.astype(index_dtype(cb.shape[0]), copy=False)}
            else:
                raise ValueError(f"group {name} must hold 'codebook' + 'index' or 'half', got {sorted(g)}")
        self.xyz, self.opacity = xyz, opacity

    @property
    def num_points(self) -> int:
        return int(self.xyz.shape[0])

    def arrays(self) -> Dict[str, np.ndarray]:
        """The payload, by the names of the file."""
        out = {"xyz": self.xyz, "opacity": self.opacity}
        for name, g in self.groups.items():
            for part, a in g.items():
                out[f"{name}.{part}"] = a
        return out

    def nbytes(self) -> int:
        """The payload size: the sum over the arrays of ``size * itemsize``."""
        return int(sum(a.size * a.itemsize for a in self.arrays().values()))

    def decode(self, device="cpu") -> Dict[str, torch.Tensor]:
        """The dict ``ply_io.load_ply`` returns -- same keys, layouts and dtypes -- on ``device``.  A quantised group is
        ``codebook[index]`` (``torch.index_select``), a float16 group its values widened."""
        P, k = self.num_points, (self.sh_degree + 1) ** 2 - 1
        t = lambda a: torch.from_numpy(a).to(device)                                               # noqa: E731

        def rows(name, D):
            if name not in self.groups:
                return torch.zeros((P, D), dtype=torch.float32, device=device)
            g = self.groups[name]
            if "half" in g:
                return t(g["half"]).to(torch.float32)
            return t(g["codebook"]).index_select(0, t(g["index"].astype(np.int64)))
        return {"_xyz": t(self.xyz).to(torch.float32).contiguous(),
                "_features_dc": rows("f_dc", 3).reshape(P, 1, 3).contiguous(),
                "_features_rest": rows("f_rest", 3 * k).reshape(P, k, 3).contiguous(),
                "_opacity": t(self.opacity).to(torch.float32).contiguous(),
                "_scaling": rows("scaling", 3).contiguous(), "_rotation": rows("rotation", 4).contiguous(),
                "active_sh_degree": self.sh_degree}


def canonical_rotation(rotation: torch.Tensor) -> torch.Tensor:
    """The quaternion rows normalised (a zero row stays zero) with the sign fixed so that ``w >= 0``: the same rotation,
    which the renderer normalises on use anyway."""
    q = rotation / rotation.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return torch.where(q[:, :1] < 0, -q, q)


def _tensors_of(model_or_dict) -> Dict[str, torch.Tensor]:
    get = (lambda a: model_or_dict[a]) if isinstance(model_or_dict, dict) else (lambda a: getattr(model_or_dict, a))
    try:
        out = {name: get(attr) for name, attr in _ATTR.items()}
    except (KeyError, AttributeError) as e:
        raise ValueError(f"the model lacks {e}") from None
    for name, t in out.items():
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{_ATTR[name]} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    out = {name: t.detach() for name, t in out.items()}
    P = int(out["xyz"].shape[0]) if out["xyz"].dim() == 2 else -1
    rest = out["f_rest"]
    ok = P >= 1 and tuple(out["xyz"].shape) == (P, 3) and tuple(out["f_dc"].shape) == (P, 1, 3) and rest.dim() == 3 \
        and rest.shape[0] == P and rest.shape[2] == 3 and tuple(out["opacity"].shape) == (P, 1) \
        and tuple(out["scaling"].shape) == (P, 3) and tuple(out["rotation"].shape) == (P, 4)
    if not ok:
        raise ValueError("the model's tensors must be _xyz [P,3], _features_dc [P,1,3], _features_rest [P,k,3], "
                         "_opacity [P,1], _scaling [P,3], _rotation [P,4] with P >= 1, got "
                         + ", ".join(f"{_ATTR[n]} {tuple(t.shape)}" for n, t in out.items()))
    degree = {0: 0, 3: 1, 8: 2, 15: 3, 24: 4}.get(int(rest.shape[1]))
    if degree is None:
        raise ValueError(f"_features_rest has {int(rest.shape[1])} coefficients: no SH degree in 0..4 has (deg+1)^2 - 1 of them")
    if len({t.device for t in out.values()}) != 1:
        raise ValueError("the model's tensors must be on one device")
    for name, t in out.items():
        if not bool(torch.isfinite(t).all()):
            raise ValueError(f"{_ATTR[name]} holds a value that is not finite")
    out["degree"] = degree
    return out


def compress_model(model_or_dict, codebook_size: int = 4096, iters: int = 10, groups: Sequence[str] = GROUPS,
                   weights: Optional[torch.Tensor] = None, xyz_dtype: str = "float32", seed: int = 0) -> CompressedGaussians:
    """Vector-quantise a model (a ``GaussianModel`` or the dict of ``ply_io.load_ply``) -> ``CompressedGaussians``.

    One codebook of at most ``codebook_size`` rows per group in ``groups`` (Compact3D's grouping): ``f_dc`` (D = 3),
    ``f_rest`` (D = 3((deg+1)^2 - 1); no such group at degree 0), ``scaling`` (D = 3, raw), ``rotation`` (D = 4, first
    normalised with ``w >= 0``: ``canonical_rotation``; its centres are renormalised at the end, so decoded rotations
    are unit).  A group that is not listed is stored as float16 (the rotation
    still canonical).  Positions are float32, or float16 with ``xyz_dtype="float16"``; opacity is raw float16.
    ``weights``: a per-Gaussian importance, float32 ``[P]``, finite and not negative (for instance
    ``ContributionStats``' blending-weight sum: LightGaussian's weighting); the centres are then weighted means.
    A value that is not finite anywhere in the model is refused before any launch, and so is a listed group whose rows
    are wider than ``MAX_D`` = 64, which is ``f_rest`` at SH degree 4 (D = 72): such a model is compressed with
    ``groups=("f_dc", "scaling", "rotation")`` and keeps its ``f_rest`` as float16.  A group with at most
    ``codebook_size`` rows is stored losslessly (``kmeans``' short-cut)."""
    K = _check_int(codebook_size, "codebook_size", 1, MAX_K)
    iters = _check_int(iters, "iters", 0, 10 ** 6)
    seed = _check_int(seed, "seed", -2 ** 63, 2 ** 63 - 1)
    groups = tuple(groups)
    if any(g not in GROUPS for g in groups) or len(set(groups)) != len(groups):
        raise ValueError(f"groups must be distinct names out of {GROUPS}, got {groups}")
    if xyz_dtype not in ("float32", "float16"):
        raise ValueError(f"xyz_dtype must be 'float32' or 'float16', got {xyz_dtype!r}")
    carried = model_or_dict.get("filter_3D") if isinstance(model_or_dict, dict) else getattr(model_or_dict, "filter_3D", None)
    if carried is not None:
        raise ValueError("the model still carries a 3D smoothing filter, which the container has no place for: bake it in "
                         "with fuse_filter_3D_() first (a dict: apply_3d_filter on its _scaling and _opacity)")
    m = _tensors_of(model_or_dict)
    P, degree = int(m["xyz"].shape[0]), m["degree"]
    width = {"f_dc": 3, "f_rest": 3 * int(m["f_rest"].shape[1]), "scaling": 3, "rotation": 4}
    for name in groups:
        if width[name] > MAX_D:
            raise ValueError(f"group {name} has D = {width[name]} at SH degree {degree}; k-means takes D in 1..{MAX_D}.  "
                             f"Leave {name} out of groups and it is stored as float16")
    weights = _check_weights(weights, P, m["xyz"])
    rows = {"f_dc": m["f_dc"].reshape(P, 3), "f_rest": m["f_rest"].reshape(P, -1), "scaling": m["scaling"],
            "rotation": canonical_rotation(m["rotation"])}
    if degree == 0:
        del rows["f_rest"]
    host = lambda t: t.cpu().numpy()                                                               # noqa: E731
    packed = {}
    for name, r in rows.items():
        r = r.contiguous()
        if name in groups:
            codebook, index, _ = kmeans(r, K, iters=iters, weights=weights, seed=seed)
            if name == "rotation":
                # a mean of unit quaternions is shorter than 1: back to unit length, after the last assign.  A centre that
                # is unit to float32 rounding already (a row of the model: the lossless cases) keeps its bits
                off = (codebook.double().norm(dim=1, keepdim=True) - 1.0).abs() > UNIT_TOLERANCE
                codebook = torch.where(off, canonical_rotation(codebook), codebook)
            packed[name] = {"codebook": host(codebook), "index": host(index).astype(index_dtype(codebook.shape[0]))}
        else:
            packed[name] = {"half": host(r.to(torch.float16))}
    return CompressedGaussians(degree, host(m["xyz"].to(getattr(torch, xyz_dtype)).contiguous()),
                               host(m["opacity"].to(torch.float16).contiguous()), packed)


# ---- the file ----------------------------------------------------------------------------------------------------------------
def save_compressed(path: str, cg: CompressedGaussians) -> None:
    """One ``.npz`` written with ``numpy.savez`` (stored, not deflated): ``format`` (the tag), ``version``, ``sh_degree``,
    ``xyz``, ``opacity`` and per group ``<group>.codebook`` + ``<group>.index`` or ``<group>.half``."""
    if not isinstance(cg, CompressedGaussians):
        raise ValueError(f"save_compressed takes a CompressedGaussians, got {type(cg)}")
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:            # an open file: numpy then leaves the name as it is
        np.savez(f, format=np.array(FORMAT_TAG), version=np.array(FORMAT_VERSION, dtype=np.int32),
                 sh_degree=np.array(cg.sh_degree, dtype=np.int32), **cg.arrays())


def load_compressed(path: str) -> CompressedGaussians:
    """What ``save_compressed`` wrote, back; every array is checked as the constructor checks it."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or str(z["format"]) != FORMAT_TAG:
            raise ValueError(f"{path}: not a compressed Gaussian model (no '{FORMAT_TAG}' tag)")
        if int(z["version"]) != FORMAT_VERSION:
            raise ValueError(f"{path}: format version {int(z['version'])}, this reader knows {FORMAT_VERSION}")
        groups: Dict[str, Dict[str, np.ndarray]] = {}
        for key in z.files:
            if "." in key:
                name, part = key.split(".", 1)
                groups.setdefault(name, {})[part] = z[key]
        return CompressedGaussians(int(z["sh_degree"]), z["xyz"], z["opacity"], groups)


__all__ = ["kmeans_assign", "kmeans_update", "kmeans", "compress_model", "CompressedGaussians", "save_compressed",
           "load_compressed", "canonical_rotation", "index_dtype"]
