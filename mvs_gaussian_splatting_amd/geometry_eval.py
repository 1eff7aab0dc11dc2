"""Scoring a mesh against ground-truth points: the exact nearest point of another cloud on the GPU
(``csrc/nearest.hip`` on the Morton-box index of ``csrc/knn.hip``), on top of it DTU's Chamfer distance (accuracy,
completeness, their mean) and the Tanks-and-Temples precision / recall / F-score at distance thresholds, and what the
protocols do BEFORE they measure: a given alignment, the scene's crop volume, point-to-point ICP with or without scale
(``csrc/icp.hip`` between two nearest-point queries) and voxel down-sampling (the kernels of ``csrc/mesh_simplify.hip``).

Contract of the nearest-point query (restated and checked by ``tests/nearest_restate.py`` / ``tests/test_gpu_nearest.py``):
  - inputs are ``[N, 3]`` on a ROCm GPU, any float dtype, any strides; float64 is rounded to float32 first (the contract of
    ``knn.py``) and the distances are those of the rounded coordinates.  Results are detached.  There is no CPU path.
  - ``dist2`` float32 ``[Q]``: the minimum over the reference of ``((dx*dx + dy*dy) + dz*dz)`` with ``dx = q.x - r.x``, every
    operation rounded to float32 on its own; ``nearest`` int32 ``[Q]``: the smallest reference index that attains it.
  - an empty reference gives ``+inf`` and ``-1``; coordinates must be finite.

Contract of the registration (restated and checked by ``tests/icp_restate.py`` / ``tests/test_gpu_icp.py``):
  - a transformation is a 4x4 float64 similarity on the host, bottom row ``0 0 0 1``; points are float32 on the GPU.
    ``transform_points`` forms ``((m0 x + m1 y) + m2 z) + m3`` per axis in float64, no fused multiply-add, and rounds once.
    ICP always transforms the ORIGINAL source by the CUMULATIVE matrix, so rounding does not accumulate over iterations.
  - ``icp_step`` = transform, nearest-point query, and the 18 sums of the pairs with ``dist2 <= float32(max_dist^2)``
    (inclusive) about two float64 pivots, accumulated in float64 in a fixed order without atomics: the same bits from
    run to run.  It reads the 18 values back: the ONE host synchronisation of an ICP iteration.
  - ``estimate_similarity`` (Kabsch / Umeyama, reflection fix ``diag(1, 1, det(V U^T))``) runs on the host in float64.
  - ``voxel_down_sample`` returns the cells in ascending cell key (``ix << 42 | iy << 21 | iz``): this project's order;
    Open3D's is the iteration order of a hash map.
  - ``crop_points`` is plain torch on any device (once per cloud: not hot).

Left out: exact point-to-triangle distance (the protocols sample the mesh), DTU's per-scan visibility masks beyond
``bounds``, gradients (a Chamfer loss, a differentiable registration), k > 1, multi-GPU, point-to-plane ICP, RANSAC /
feature-based global registration, colour ICP.
"""
from __future__ import annotations

import json
import math
import sys
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

_MAX_POINTS = 2 ** 31 - 256          # gsr.h: GSR_NN_MAX_POINTS


def _points(t, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise ValueError(f"{what} must be a float tensor [N, 3]")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what} must be [N, 3], got {tuple(t.shape)}")
    if t.shape[0] > _MAX_POINTS:
        raise ValueError(f"{what} has more than 2^31 - 256 points")
    return t


def _device_points(t, what: str) -> torch.Tensor:
    t = _points(t, what)
    if not t.is_cuda:
        raise _lib.GsrError(f"{what} must be on a ROCm GPU (no CPU path)")
    return t.detach().float().contiguous()


class NearestIndex:
    """The index of a reference cloud ``ref [R, 3]``: build once, ``query`` many times."""

    def __init__(self, ref: torch.Tensor):
        pts = _device_points(ref, "ref")
        lib = _lib.load()
        self.device = pts.device
        self.num_points = int(pts.shape[0])
        self._bytes = int(lib.gsr_nn_index_bytes(self.num_points))
        self._index = torch.empty(self._bytes, dtype=torch.uint8, device=pts.device)
        with torch.cuda.device(pts.device):
            stream = torch.cuda.current_stream(pts.device).cuda_stream
            _lib.check(lib.gsr_nn_build(pts.data_ptr(), self.num_points, self._index.data_ptr(), self._bytes, stream),
                       "gsr_nn_build")

    @torch.no_grad()
    def query(self, points: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (dist2 float32 [Q], nearest int32 [Q]) of ``points [Q, 3]`` against the reference."""
        q = _device_points(points, "points")
        if q.device != self.device:
            raise ValueError(f"points are on {q.device}, the index on {self.device}")
        lib = _lib.load()
        Q = int(q.shape[0])
        dist2 = torch.empty(Q, dtype=torch.float32, device=q.device)
        nearest = torch.empty(Q, dtype=torch.int32, device=q.device)
        nbytes = int(lib.gsr_nn_query_workspace_bytes(Q))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        with torch.cuda.device(q.device):
            stream = torch.cuda.current_stream(q.device).cuda_stream
            _lib.check(lib.gsr_nn_query(self._index.data_ptr(), self._bytes, self.num_points, q.data_ptr(), Q,
                                        dist2.data_ptr(), nearest.data_ptr(), ws.data_ptr(), nbytes, stream), "gsr_nn_query")
        return dist2, nearest


def nearest_points(query: torch.Tensor, ref: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """One-shot ``NearestIndex(ref).query(query)``."""
    _points(query, "query")
    return NearestIndex(ref).query(query)


def sample_surface(vertices: torch.Tensor, faces: torch.Tensor, n: int,
                   generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``n`` points on a triangle mesh, area-weighted and stratified, in plain torch on the mesh's device.
    -> (points [n, 3] in the dtype of ``vertices``, face_index int64 [n]).

    Face areas ``0.5 |(b - a) x (c - a)|`` and their ``cumsum`` are float64.  With ``r = torch.rand((n, 3))`` sample ``i``
    takes ``t = (i + r[i, 0]) * total / n`` and the first face whose cumulative area exceeds ``t``, clamped to the last
    face of positive area: a zero-area face is never chosen.  With ``s = sqrt(r1)`` the point is
    ``(1 - s) a + s (1 - r2) b + s r2 c``."""
    _points(vertices, "vertices")
    if not isinstance(faces, torch.Tensor) or faces.is_floating_point() or faces.dtype == torch.bool or \
            faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be an integer tensor [F, 3]")
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError("n must be a non-negative integer")
    if faces.shape[0] == 0:
        raise ValueError("the mesh has no faces")
    vertices = vertices.detach()
    f = faces.detach().to(device=vertices.device, dtype=torch.int64)
    if int(f.min()) < 0 or int(f.max()) >= vertices.shape[0]:
        raise ValueError(f"a face refers to a vertex outside 0..{vertices.shape[0] - 1}")
    v64 = vertices.double()
    a, b, c = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    area = 0.5 * torch.linalg.cross(b - a, c - a, dim=1).norm(dim=1)
    cum = torch.cumsum(area, dim=0)
    total = cum[-1]
    if not float(total) > 0.0:
        raise ValueError("the mesh has no area")
    r = torch.rand((n, 3), generator=generator, device=generator.device if generator is not None else vertices.device)
    r = r.to(vertices.device)
    t = (torch.arange(n, device=vertices.device, dtype=torch.float64) + r[:, 0].double()) * total / n
    face = torch.searchsorted(cum, t, right=True)
    last = torch.nonzero(area > 0)[-1, 0]
    face = torch.minimum(face, last)
    dt = vertices.dtype
    s = torch.sqrt(r[:, 1].to(dt))[:, None]
    r2 = r[:, 2].to(dt)[:, None]
    tri = vertices[f[face]]
    points = (1 - s) * tri[:, 0] + (s * (1 - r2)) * tri[:, 1] + (s * r2) * tri[:, 2]
    return points, face


def _thresholds(thresholds) -> Tuple[float, ...]:
    if isinstance(thresholds, (int, float)) and not isinstance(thresholds, bool):
        thresholds = (thresholds,)
    out = []
    for tau in thresholds:
        if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not math.isfinite(tau) or tau <= 0:
            raise ValueError(f"a threshold must be a finite positive number, got {tau!r}")
        out.append(float(tau))
    if len(set(out)) != len(out):
        raise ValueError("thresholds repeat")
    return tuple(out)


def evaluate_points(pred: torch.Tensor, gt: torch.Tensor, thresholds: Sequence[float] = (),
                    max_dist: Optional[float] = None, bounds=None, down_sample: Optional[float] = None) -> Dict:
    """Chamfer distance and precision / recall / F-score of a predicted cloud against a ground-truth cloud.

    ``bounds = (lo, hi)`` (two 3-vectors) keeps the points of ``pred`` inside the closed box first (DTU's observation
    box).  Distances are ``sqrt(dist2)`` in float64.  ``max_dist``: distances above it are left out of the means and their
    share is reported (DTU's rule).  -> ``accuracy`` (mean distance pred -> gt), ``completeness`` (gt -> pred), ``chamfer``
    (their mean), ``thresholds``: per tau a dict ``tau``, ``precision`` (share of ALL pred points within tau), ``recall``,
    ``fscore``; ``dropped_pred`` / ``dropped_gt``, ``n_pred`` / ``n_gt``.  All reductions are torch float64 on the device and
    are read back once, at the end; with ``bounds`` the crop of ``pred`` reads its count back before (a boolean mask).

    ``down_sample = v``: after the crop both clouds go through ``voxel_down_sample(., v)`` (the protocols score at a fixed
    density: TnT at ``dTau / 2``), one more read-back each; ``n_pred`` / ``n_gt`` then count the cells.  ``None`` makes
    exactly the calls it always made."""
    _points(pred, "pred")
    _points(gt, "gt")
    taus = _thresholds(thresholds)
    if max_dist is not None and (isinstance(max_dist, bool) or not isinstance(max_dist, (int, float))
                                 or not math.isfinite(max_dist) or max_dist <= 0):
        raise ValueError("max_dist must be None or a finite positive number")
    if bounds is not None:
        try:
            lo, hi = (torch.as_tensor(x, dtype=torch.float64).reshape(-1) for x in bounds)
        except (TypeError, ValueError) as e:
            raise ValueError("bounds must be (lo, hi), two 3-vectors") from e
        if lo.numel() != 3 or hi.numel() != 3 or not bool((lo <= hi).all()):
            raise ValueError("bounds must be (lo, hi), two 3-vectors with lo <= hi")
    if not pred.is_cuda or not gt.is_cuda:
        raise _lib.GsrError("evaluate_points needs ROCm GPU tensors (no CPU path)")
    pred, gt = pred.detach().float(), gt.detach().float().to(pred.device)
    if bounds is not None:
        lo, hi = lo.to(pred.device), hi.to(pred.device)
        p64 = pred.double()
        pred = pred[((p64 >= lo) & (p64 <= hi)).all(dim=1)]
    if down_sample is not None:
        pred, gt = voxel_down_sample(pred, down_sample), voxel_down_sample(gt, down_sample)
    n_pred, n_gt = int(pred.shape[0]), int(gt.shape[0])
    if n_pred == 0 or n_gt == 0:
        raise ValueError(f"nothing to compare: {n_pred} predicted points (after bounds), {n_gt} ground-truth points")
    d_pred = torch.sqrt(NearestIndex(gt).query(pred)[0].double())
    d_gt = torch.sqrt(NearestIndex(pred).query(gt)[0].double())
    vals = []
    for d in (d_pred, d_gt):
        keep = d <= max_dist if max_dist is not None else torch.ones_like(d, dtype=torch.bool)
        kept = keep.sum()
        vals += [torch.where(keep, d, torch.zeros_like(d)).sum() / kept.clamp(min=1).double(), kept.double()]
        vals += [(d <= tau).sum().double() for tau in taus]
    host = torch.stack(vals).tolist()                                      # the one read-back
    k = 2 + len(taus)
    (acc, kept_p), within_p = host[:2], host[2:k]
    (comp, kept_g), within_g = host[k:k + 2], host[k + 2:]
    nan = float("nan")
    acc, comp = (acc if kept_p else nan), (comp if kept_g else nan)
    out = {"accuracy": acc, "completeness": comp, "chamfer": 0.5 * (acc + comp), "n_pred": n_pred, "n_gt": n_gt,
           "dropped_pred": 1.0 - kept_p / n_pred, "dropped_gt": 1.0 - kept_g / n_gt, "max_dist": max_dist, "thresholds": []}
    for tau, wp, wg in zip(taus, within_p, within_g):
        precision, recall = wp / n_pred, wg / n_gt
        fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
        out["thresholds"].append({"tau": tau, "precision": precision, "recall": recall, "fscore": fscore})
    return out


def evaluate_mesh(vertices: torch.Tensor, faces: torch.Tensor, gt_points: torch.Tensor, n_samples: int,
                  thresholds: Sequence[float] = (), max_dist: Optional[float] = None, bounds=None,
                  generator: Optional[torch.Generator] = None, down_sample: Optional[float] = None) -> Dict:
    """``evaluate_points(sample_surface(vertices, faces, n_samples)[0], gt_points, ...)``; the result also carries
    ``n_samples``."""
    points, _ = sample_surface(vertices, faces, n_samples, generator)
    if down_sample is None:
        out = evaluate_points(points, gt_points, thresholds, max_dist, bounds)
    else:
        out = evaluate_points(points, gt_points, thresholds, max_dist, bounds, down_sample=down_sample)
    out["n_samples"] = int(n_samples)
    return out


# ---- alignment, crop, down-sampling and ICP: what the protocols do before they measure -----------------
ICP_WORDS = 18                       # gsr.h: GSR_ICP_WORDS: the int64 count and 17 doubles
CELL_BITS = 21                       # bits per axis of a cell key (csrc/mesh_simplify_math.h)
_NOT_FINITE, _OUT_OF_RANGE = 2, 4    # bits of the status word (include/gsr.h: GSR_SIMPLIFY_*)
_RANK_EPS = 1e-10                    # second singular value / first below this: the pairs are collinear


def _similarity(T, what: str = "T") -> np.ndarray:
    """-> ``T`` as a float64 [4,4] numpy array; a shape other than 4x4, an entry that is not finite or a bottom row other
    than ``0 0 0 1`` raises ``ValueError``."""
    if isinstance(T, torch.Tensor):
        T = T.detach().cpu().numpy()
    try:
        M = np.array(T, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a 4x4 matrix") from None
    if M.shape != (4, 4) or not np.isfinite(M).all():
        raise ValueError(f"{what} must be a finite 4x4 matrix, got shape {M.shape}")
    if not np.array_equal(M[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError(f"{what} must have the bottom row 0 0 0 1, got {M[3].tolist()}")
    return M


def _positive(x, what: str) -> float:
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0 < x <= sys.float_info.max:
        raise ValueError(f"{what} must be a finite positive number, got {x!r}")
    return float(x)


def _transform_into(lib, pts: torch.Tensor, M: np.ndarray, stream) -> torch.Tensor:
    out = torch.empty_like(pts)
    m = np.ascontiguousarray(M[:3], dtype=np.float64)
    _lib.check(lib.gsr_icp_transform(pts.data_ptr(), int(pts.shape[0]), m.ctypes.data, out.data_ptr(), stream),
               "gsr_icp_transform")
    return out


@torch.no_grad()
def transform_points(points: torch.Tensor, T) -> torch.Tensor:
    """``float32(T p)`` of ``points [N, 3]`` (GPU, any float dtype and strides; rounded to float32 first) by the 4x4 float64
    similarity ``T`` -> a new float32 ``[N, 3]`` tensor.  Per axis ``((m0 x + m1 y) + m2 z) + m3`` in float64, each operation
    rounded on its own, then one rounding to float32 (csrc/icp_math.h)."""
    M = _similarity(T)
    pts = _device_points(points, "points")
    with torch.cuda.device(pts.device):
        return _transform_into(_lib.load(), pts, M, torch.cuda.current_stream(pts.device).cuda_stream)


@torch.no_grad()
def voxel_down_sample(points: torch.Tensor, voxel_size: float, *, origin=None) -> torch.Tensor:
    """One point per occupied cell of a uniform grid -> float32 ``[K, 3]`` on the device of ``points [N, 3]`` (GPU).

    The cell of a point is ``floor(((double)x - origin) / voxel_size)`` per axis in float64; every index must lie in
    ``0..2^21-1`` or ``GsrError`` says so, as does a coordinate that is not finite (the rules of ``mesh.simplify_mesh``,
    whose kernels run here with every point marked and no faces).  ``origin`` (three finite floats) defaults to that
    function's rule: the per-axis minimum minus ``voxel_size / 2``, formed on the device.  A row of the result is the mean
    of its cell's float32 points, summed in float64 in ascending point index and rounded to float32 once; a cell of one
    point is a bit-copy.  Rows come in ascending cell key ``ix << 42 | iy << 21 | iz``: this project's order (Open3D's is a
    hash map's).  One read-back (K with the status word)."""
    h = _positive(voxel_size, "voxel_size")
    if origin is not None:
        try:
            origin = tuple(float(o) for o in origin)
        except (TypeError, ValueError):
            raise ValueError(f"origin must be None or three finite floats, got {origin!r}") from None
        if len(origin) != 3 or not all(math.isfinite(o) for o in origin):
            raise ValueError(f"origin must be None or three finite floats, got {origin!r}")
    pts = _device_points(points, "points")
    N, dev = int(pts.shape[0]), pts.device
    if N == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        mark = torch.ones(N, dtype=torch.uint8, device=dev)
        if origin is None:
            origin_dev = torch.empty(3, dtype=torch.float64, device=dev)
            lowest = torch.empty(3, dtype=torch.int32, device=dev)
            _lib.check(lib.gsr_simplify_default_origin(pts.data_ptr(), mark.data_ptr(), N, h, lowest.data_ptr(),
                                                       origin_dev.data_ptr(), stream), "gsr_simplify_default_origin")
        else:
            origin_dev = torch.tensor(origin, dtype=torch.float64, device=dev)
        keys = torch.empty(N, dtype=torch.int64, device=dev)
        _lib.check(lib.gsr_simplify_cell_keys(pts.data_ptr(), mark.data_ptr(), N, origin_dev.data_ptr(), h, keys.data_ptr(),
                                              status.data_ptr(), stream), "gsr_simplify_cell_keys")
        keys_sorted, order = torch.sort(keys, stable=True)       # stable: a cell's points stay in ascending index
        head = torch.empty(N, dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_simplify_run_heads(keys_sorted.data_ptr(), N, head.data_ptr(), stream), "gsr_simplify_run_heads")
        ends = torch.cumsum(head, dim=0, dtype=torch.int64)
        K, bad = (int(v) for v in torch.stack((ends[-1], status[0].to(torch.int64))).tolist())       # the read-back
        if bad & _NOT_FINITE:
            raise _lib.GsrError("voxel_down_sample failed: a coordinate is not finite")
        if bad & _OUT_OF_RANGE:
            raise _lib.GsrError(f"voxel_down_sample failed: a cell index lies outside 0..2^{CELL_BITS}-1: voxel_size "
                                f"{voxel_size!r} is too small for the extent of the cloud, or the origin lies above a point")
        if bad or K < 1:
            raise _lib.GsrError(f"voxel_down_sample failed: status {bad}, {K} cells")
        start = torch.empty(K + 1, dtype=torch.int32, device=dev)
        means = torch.empty((K, 3), dtype=torch.float32, device=dev)
        cell_of_point = torch.empty(N, dtype=torch.int32, device=dev)
        _lib.check(lib.gsr_simplify_reduce(pts.data_ptr(), None, keys_sorted.data_ptr(), order.data_ptr(), ends.data_ptr(), N,
                                           K, start.data_ptr(), means.data_ptr(), None, cell_of_point.data_ptr(),
                                           status.data_ptr(), stream), "gsr_simplify_reduce")
    return means


def uniform_down_sample(points: torch.Tensor, every_k: int) -> torch.Tensor:
    """Every ``every_k``-th point, from the first (Open3D's ``uniform_down_sample``): a strided view."""
    _points(points, "points")
    if isinstance(every_k, bool) or not isinstance(every_k, int) or every_k < 1:
        raise ValueError(f"every_k must be a positive integer, got {every_k!r}")
    return points[::every_k]


class IcpSums(NamedTuple):
    """What ``icp_step`` returns: the pairs accepted and their sums about the pivots, ``a = q - pivot_q``, ``b = r -
    pivot_r`` with ``q`` the transformed source point and ``r`` its nearest target point.  numpy float64 on the host."""
    count: int
    sum_a: np.ndarray        # [3]
    sum_b: np.ndarray        # [3]
    sum_ab: np.ndarray       # [3,3]: sum of a b^T
    sum_aa: float            # sum of |a|^2
    sum_d2: float            # sum of the float32 squared distances
    pivot_q: np.ndarray      # [3]
    pivot_r: np.ndarray      # [3]
    num_source: int

    @property
    def fitness(self) -> float:
        return self.count / self.num_source if self.num_source else 0.0

    @property
    def inlier_rmse(self) -> float:
        return math.sqrt(self.sum_d2 / self.count) if self.count else 0.0


def _sums_of_pairs(src, dst) -> IcpSums:
    a, b = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError(f"the pairs must be two [n, 3] arrays of one shape, got {a.shape} and {b.shape}")
    n = a.shape[0]
    cq, cr = (a.mean(axis=0), b.mean(axis=0)) if n else (np.zeros(3), np.zeros(3))
    a, b = a - cq, b - cr
    return IcpSums(n, a.sum(axis=0), b.sum(axis=0), a.T @ b, float((a * a).sum()), float(((a - b + (cq - cr)) ** 2).sum()),
                   cq, cr, n)


def estimate_similarity(src, dst=None, *, with_scaling: bool = False) -> np.ndarray:
    """The least-squares rigid (or, ``with_scaling``, similarity) transformation of paired points -> 4x4 float64, mapping
    source onto target (Kabsch; Umeyama 1991).  On the host, in float64.  Two forms:

    ``estimate_similarity(sums)``        from an ``IcpSums`` (what ``icp_step`` read back);
    ``estimate_similarity(src, dst)``    from two ``[n, 3]`` arrays of pairs (numpy, lists or tensors), summed about their
                                         means.

    With n pairs, ``H = sum a b^T - (sum a)(sum b)^T / n = U S V^T``: ``R = V D U^T`` with ``D = diag(1, 1, det(V U^T))`` (a
    mirrored pair set still gives a proper rotation), ``scale = trace(D S) / (sum |a|^2 - |sum a|^2 / n)`` under
    ``with_scaling`` and the literal 1 otherwise, ``t = mean_r - scale R mean_q``.  Fewer than 3 pairs, or a covariance of
    rank below 2 (all pairs on a line: the rotation about it is free), raise ``ValueError``."""
    if dst is not None:
        if isinstance(src, torch.Tensor):
            src = src.detach().cpu().numpy()
        if isinstance(dst, torch.Tensor):
            dst = dst.detach().cpu().numpy()
        sums = _sums_of_pairs(src, dst)
    elif isinstance(src, IcpSums):
        sums = src
    else:
        raise ValueError("estimate_similarity takes an IcpSums, or two [n, 3] arrays")
    n = int(sums.count)
    if n < 3:
        raise ValueError(f"estimate_similarity needs at least 3 pairs, got {n}")
    sa, sb = np.asarray(sums.sum_a, dtype=np.float64), np.asarray(sums.sum_b, dtype=np.float64)
    H = np.asarray(sums.sum_ab, dtype=np.float64) - np.outer(sa, sb) / n
    var_a = float(sums.sum_aa) - float(sa @ sa) / n
    U, S, Vt = np.linalg.svd(H)
    if not (S[0] > 0.0 and S[1] > _RANK_EPS * S[0]) or not var_a > 0.0:
        raise ValueError("estimate_similarity: the covariance of the pairs has rank below 2 (collinear or coincident "
                         "points): the rotation is not determined")
    D = np.array([1.0, 1.0, 1.0 if np.linalg.det(Vt.T @ U.T) > 0 else -1.0])
    R = (Vt.T * D) @ U.T
    mean_q = np.asarray(sums.pivot_q, dtype=np.float64) + sa / n
    mean_r = np.asarray(sums.pivot_r, dtype=np.float64) + sb / n
    T = np.eye(4)
    if with_scaling:
        scale = float((D * S).sum()) / var_a
        T[:3, :3] = scale * R
    else:
        T[:3, :3] = R
    T[:3, 3] = mean_r - T[:3, :3] @ mean_q
    return T


def align_cameras(src_centres, dst_centres, *, with_scaling: bool = True) -> np.ndarray:
    """The trajectory alignment of the protocols: the similarity that maps the reconstruction's camera centres
    ``src_centres [n, 3]`` onto the ground truth's ``dst_centres [n, 3]`` (same order) -> 4x4 float64, to be passed as
    ``init``.  ``estimate_similarity(src_centres, dst_centres, with_scaling=with_scaling)``."""
    return estimate_similarity(src_centres, dst_centres, with_scaling=with_scaling)


class IcpTarget:
    """A registration target: the float32 points of ``points [R, 3]`` (GPU) and their ``NearestIndex``, built once."""

    def __init__(self, points: torch.Tensor, index: Optional[NearestIndex] = None):
        self.points = _device_points(points, "target")
        self.index = NearestIndex(self.points) if index is None else index
        if not isinstance(self.index, NearestIndex) or self.index.num_points != int(self.points.shape[0]) \
                or self.index.device != self.points.device:
            raise ValueError("the index is not a NearestIndex of these target points")


def _icp_target(target) -> IcpTarget:
    if isinstance(target, IcpTarget):
        return target
    if isinstance(target, (tuple, list)) and len(target) == 2 and isinstance(target[0], NearestIndex):
        return IcpTarget(target[1], target[0])
    return IcpTarget(target)


def _thr2(max_dist) -> float:
    d = _positive(max_dist, "max_dist")
    with np.errstate(over="ignore"):
        return float(np.float32(d * d))             # the float64 square rounded once; +inf when it overflows float32


@torch.no_grad()
def icp_step(source: torch.Tensor, target, T, max_dist: float, *, pivots=None) -> IcpSums:
    """One evaluation of ICP at the transformation ``T``: ``q = transform_points(source, T)``, the nearest target point of
    every ``q``, and the sums of the pairs with ``dist2 <= float32(max_dist^2)`` (csrc/icp.hip) -> ``IcpSums``.

    ``source [Q, 3]`` on the GPU; ``target``: an ``IcpTarget``, a pair ``(NearestIndex, points)``, or a tensor ``[R, 3]`` (its
    index is then built here, every call).  ``pivots = (c_q, c_r)``, two float64 3-vectors the sums are taken about so that
    a cloud far from the origin loses no digits; default: zeros.  Reads the 18 values back: one host synchronisation."""
    M = _similarity(T)
    thr2 = _thr2(max_dist)
    if pivots is None:
        piv = np.zeros(6)
    else:
        piv = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in pivots])
        if piv.shape != (6,) or not np.isfinite(piv).all():
            raise ValueError("pivots must be (c_q, c_r), two finite 3-vectors")
    src = _device_points(source, "source")
    tgt = _icp_target(target)
    if tgt.points.device != src.device:
        raise ValueError(f"source is on {src.device}, the target on {tgt.points.device}")
    lib = _lib.load()
    Q, R, dev = int(src.shape[0]), int(tgt.points.shape[0]), src.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        q = _transform_into(lib, src, M, stream)
        dist2, nearest = tgt.index.query(q)
        nbytes = int(lib.gsr_icp_workspace_bytes(Q))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(ICP_WORDS, dtype=torch.int64, device=dev)
        _lib.check(lib.gsr_icp_accumulate(q.data_ptr(), dist2.data_ptr(), nearest.data_ptr(), Q, tgt.points.data_ptr(), R,
                                          thr2, piv.ctypes.data, ws.data_ptr(), nbytes, out.data_ptr(), stream),
                   "gsr_icp_accumulate")
        words = out.cpu().numpy()                                               # the one read-back of the iteration
    s = words[1:].view(np.float64)
    return IcpSums(int(words[0]), s[0:3].copy(), s[3:6].copy(), s[6:15].reshape(3, 3).copy(), float(s[15]), float(s[16]),
                   piv[:3].copy(), piv[3:].copy(), Q)


class RegistrationResult(NamedTuple):
    transformation: np.ndarray       # 4x4 float64: source -> target
    fitness: float                   # accepted pairs / source points, at `transformation`
    inlier_rmse: float               # sqrt(mean dist2) of the accepted pairs
    iterations: int                  # updates made
    converged: bool


def _icp_loop(step, M: np.ndarray, first_pivots, with_scaling: bool, max_iterations: int, relative_fitness: float,
              relative_rmse: float) -> RegistrationResult:
    """Open3D's ``RegistrationICP`` loop over ``step(T, pivots) -> IcpSums`` (tests/icp_restate.py writes its own)."""
    sums = step(M, first_pivots)
    iterations, converged = 0, False
    for _ in range(max_iterations):
        if sums.count < 3:
            break
        update = estimate_similarity(sums, with_scaling=with_scaling)
        M = update @ M
        M[3] = [0.0, 0.0, 0.0, 1.0]
        iterations += 1
        mean_q = sums.pivot_q + sums.sum_a / sums.count
        mean_r = sums.pivot_r + sums.sum_b / sums.count
        before = sums
        sums = step(M, (update[:3, :3] @ mean_q + update[:3, 3], mean_r))
        if abs(before.fitness - sums.fitness) < relative_fitness and abs(before.inlier_rmse - sums.inlier_rmse) < relative_rmse:
            converged = True
            break
    return RegistrationResult(M, sums.fitness, sums.inlier_rmse, iterations, converged)


@torch.no_grad()
def icp_registration(source: torch.Tensor, target, max_dist: float, *, init=None, with_scaling: bool = False,
                     max_iterations: int = 30, relative_fitness: float = 1e-6,
                     relative_rmse: float = 1e-6) -> RegistrationResult:
    """Point-to-point ICP of ``source [Q, 3]`` onto ``target`` (as ``icp_step`` takes it; pass an ``IcpTarget`` or
    ``(NearestIndex, points)`` to build the index once) -> ``RegistrationResult``.

    Open3D's loop (``registration_icp`` with ``TransformationEstimationPointToPoint(with_scaling)``): evaluate at ``init``
    (default: identity); then up to ``max_iterations`` times estimate the update from the accepted pairs, compose it in
    front of the transformation, evaluate again, and stop (``converged``) when fitness and RMSE both changed by less than
    ``relative_fitness`` / ``relative_rmse``.  An evaluation with fewer than 3 pairs ends the loop with
    ``converged=False`` and the transformation as it stood.  Every evaluation is one ``icp_step`` of the ORIGINAL source
    at the cumulative transformation, with its one read-back: ``iterations + 1`` host synchronisations in all, after
    one for the two bounding boxes.  Pivots: the bounding-box centres at first, then the previous evaluation's
    correspondence centroids.  Without scaling the rotation is applied with the literal scale 1."""
    M = np.eye(4) if init is None else _similarity(init, "init")
    _positive(max_dist, "max_dist")
    if isinstance(max_iterations, bool) or not isinstance(max_iterations, int) or max_iterations < 0:
        raise ValueError(f"max_iterations must be a non-negative integer, got {max_iterations!r}")
    for name, v in (("relative_fitness", relative_fitness), ("relative_rmse", relative_rmse)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v >= 0:
            raise ValueError(f"{name} must be a non-negative number, got {v!r}")
    src = _device_points(source, "source")
    tgt = _icp_target(target)
    if tgt.points.device != src.device:
        raise ValueError(f"source is on {src.device}, the target on {tgt.points.device}")
    Q, R = int(src.shape[0]), int(tgt.points.shape[0])
    if Q == 0 or R == 0:
        return RegistrationResult(M, 0.0, 0.0, 0, False)
    box = torch.stack((src.amin(dim=0), src.amax(dim=0), tgt.points.amin(dim=0), tgt.points.amax(dim=0))).double().cpu().numpy()
    c_src, c_tgt = 0.5 * (box[0] + box[1]), 0.5 * (box[2] + box[3])
    first = (M[:3, :3] @ c_src + M[:3, 3], c_tgt)
    return _icp_loop(lambda T, piv: icp_step(src, tgt, T, max_dist, pivots=piv), M, first, bool(with_scaling),
                     max_iterations, float(relative_fitness), float(relative_rmse))


class CropVolume(NamedTuple):
    """Open3D's ``SelectionPolygonVolume``: a polygon prism along one axis."""
    orthogonal_axis: int             # 0, 1, 2 for X, Y, Z
    axis_min: float
    axis_max: float
    polygon: np.ndarray              # [M, 3] float64; the coordinate along the orthogonal axis is not used


def load_crop_volume(path: str) -> CropVolume:
    """Read a crop volume from the JSON that Open3D and the Tanks-and-Temples scenes use: ``orthogonal_axis`` ("X", "Y" or
    "Z"), ``axis_min``, ``axis_max`` and ``bounding_polygon`` (a list of at least three ``[x, y, z]``); other keys are
    ignored."""
    with open(path, "r") as f:
        d = json.load(f)
    try:
        axis = {"X": 0, "Y": 1, "Z": 2}[str(d["orthogonal_axis"]).upper()]
        lo, hi = float(d["axis_min"]), float(d["axis_max"])
        poly = np.array(d["bounding_polygon"], dtype=np.float64)
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError(f"{path}: not a crop volume (orthogonal_axis, axis_min, axis_max, bounding_polygon): {e!r}") from None
    if poly.ndim != 2 or poly.shape[1] != 3 or poly.shape[0] < 3 or not np.isfinite(poly).all():
        raise ValueError(f"{path}: bounding_polygon must be at least three finite [x, y, z]")
    if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
        raise ValueError(f"{path}: axis_min / axis_max must be finite with axis_min <= axis_max")
    return CropVolume(axis, lo, hi, poly)


@torch.no_grad()
def crop_points(points: torch.Tensor, volume: CropVolume, return_mask: bool = False):
    """The points of ``points [N, 3]`` inside a crop volume (Open3D's ``SelectionPolygonVolume.crop_point_cloud``), in
    their order; with ``return_mask`` also the boolean mask.  Plain torch on the device of ``points``, in float64.

    With ``w`` the orthogonal axis and ``(u, v)`` the other two in ascending order (X: (y, z); Y: (x, z); Z: (x, y)): a
    point is kept when ``axis_min <= p_w <= axis_max`` (both faces belong to the slab) and an even-odd crossing test holds
    on ``(u, v)``: over the polygon's edges ``(i, i + 1 mod M)`` with ``(v_i > p_v) != (v_j > p_v)``, the number of those
    with ``p_u < u_i + (p_v - v_i) (u_j - u_i) / (v_j - v_i)`` is odd.  A point exactly on the polygon's outline falls on
    either side, as in every crossing test."""
    _points(points, "points")
    w = int(volume.orthogonal_axis)
    if w not in (0, 1, 2):
        raise ValueError(f"orthogonal_axis must be 0, 1 or 2, got {volume.orthogonal_axis!r}")
    u, v = [a for a in (0, 1, 2) if a != w]
    p = points.detach().double()
    poly = torch.as_tensor(np.asarray(volume.polygon, dtype=np.float64), device=p.device)
    if poly.dim() != 2 or poly.shape[0] < 3 or poly.shape[1] != 3:
        raise ValueError("the polygon must be [M, 3] with M >= 3")
    inside = torch.zeros(p.shape[0], dtype=torch.bool, device=p.device)
    pu, pv = p[:, u], p[:, v]
    M = int(poly.shape[0])
    for i in range(M):                                   # a handful of edges: the loop is over the polygon, not the points
        ui, vi = poly[i, u], poly[i, v]
        uj, vj = poly[(i + 1) % M, u], poly[(i + 1) % M, v]
        straddles = (vi > pv) != (vj > pv)
        denom = torch.where(vj != vi, vj - vi, torch.ones_like(vj))
        cross = ui + (pv - vi) * (uj - ui) / denom
        inside ^= straddles & (pu < cross)
    mask = inside & (p[:, w] >= volume.axis_min) & (p[:, w] <= volume.axis_max)
    out = points[mask]
    return (out, mask) if return_mask else out


class TntStage(NamedTuple):
    """One stage of ``register_tnt``: ``kind`` "voxel" (``param``: the voxel size) or "every" (``param``: the largest number
    of source points to keep; every k-th point is taken with the smallest k that does), the ICP threshold ``max_dist`` and
    the iteration limit."""
    kind: str
    param: float
    max_dist: float
    max_iterations: int = 20


def tnt_stages(dtau: float, max_points: int = 4_000_000) -> Tuple[TntStage, ...]:
    """The three refinement stages of the Tanks-and-Temples evaluation for the scene's ``dTau``, AS RECALLED FROM MEMORY of
    the published toolbox (it was not at hand when this was written; check against it before quoting a number): voxel
    ``dtau`` with threshold ``80 dtau``; voxel ``dtau / 2`` with ``20 dtau``; every k-th point with ``2 dtau``; 20 iterations
    each, with scaling."""
    dtau = _positive(dtau, "dtau")
    return (TntStage("voxel", dtau, 80.0 * dtau), TntStage("voxel", dtau / 2.0, 20.0 * dtau),
            TntStage("every", float(max_points), 2.0 * dtau))


@torch.no_grad()
def register_tnt(pred: torch.Tensor, gt: torch.Tensor, init, crop: Optional[CropVolume], dtau: float, stages=None,
                 with_scaling: bool = True) -> RegistrationResult:
    """The staged refinement of the Tanks-and-Temples protocol: the alignment ``init`` (4x4, e.g. ``align_cameras``) of
    ``pred [N, 3]`` onto ``gt [R, 3]`` (both GPU), refined by one point-to-point ICP per stage -> the last stage's
    ``RegistrationResult`` with the CUMULATIVE transformation (``iterations`` summed over the stages).

    Per stage: ``pred`` is transformed by the transformation so far and cropped by ``crop`` (``None``: no crop), ``gt`` is
    cropped too, both are down-sampled as the stage says, and ``icp_registration`` runs from the identity with the stage's
    threshold; its result is composed in front.  ``stages``: a sequence of ``TntStage``; the default ``tnt_stages(dtau)`` is
    written down FROM MEMORY of the toolbox, so keep passing your own when a published number depends on it."""
    M = _similarity(init, "init")
    stages = tnt_stages(dtau) if stages is None else tuple(TntStage(*s) for s in stages)
    src, ref = _device_points(pred, "pred"), _device_points(gt, "gt")
    ref_c = ref if crop is None else crop_points(ref, crop)
    result, total = RegistrationResult(M, 0.0, 0.0, 0, False), 0
    for st in stages:
        moved = transform_points(src, M)
        if crop is not None:
            moved = crop_points(moved, crop)
        if st.kind == "voxel":
            s, t = voxel_down_sample(moved, st.param), voxel_down_sample(ref_c, st.param)
        elif st.kind == "every":
            k = max(1, -(-int(moved.shape[0]) // max(1, int(st.param))))
            s, t = uniform_down_sample(moved, k), ref_c
        else:
            raise ValueError(f"a stage is 'voxel' or 'every', got {st.kind!r}")
        r = icp_registration(s, t, st.max_dist, with_scaling=with_scaling, max_iterations=int(st.max_iterations))
        M = r.transformation @ M
        M[3] = [0.0, 0.0, 0.0, 1.0]
        total += r.iterations
        result = RegistrationResult(M, r.fitness, r.inlier_rmse, total, r.converged)
    return result
