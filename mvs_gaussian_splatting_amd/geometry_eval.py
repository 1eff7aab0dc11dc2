"""Scoring a mesh against ground-truth points: the exact nearest point of another cloud on the GPU
(``csrc/nearest.hip`` on the Morton-box index of ``csrc/knn.hip``), and on top of it DTU's Chamfer distance (accuracy,
completeness, their mean) and the Tanks-and-Temples precision / recall / F-score at distance thresholds.

Contract of the nearest-point query (restated and checked by ``tests/nearest_restate.py`` / ``tests/test_gpu_nearest.py``):
  - inputs are ``[N, 3]`` on a ROCm GPU, any float dtype, any strides; float64 is rounded to float32 first (the contract of
    ``knn.py``) and the distances are those of the rounded coordinates.  Results are detached.  There is no CPU path.
  - ``dist2`` float32 ``[Q]``: the minimum over the reference of ``((dx*dx + dy*dy) + dz*dz)`` with ``dx = q.x - r.x``, every
    operation rounded to float32 on its own; ``nearest`` int32 ``[Q]``: the smallest reference index that attains it.
  - an empty reference gives ``+inf`` and ``-1``; coordinates must be finite.

Left out: exact point-to-triangle distance (the protocols sample the mesh), voxel down-sampling of the clouds, DTU's
per-scan visibility masks beyond ``bounds``, gradients (a Chamfer loss), k > 1, multi-GPU.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

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
                    max_dist: Optional[float] = None, bounds=None) -> Dict:
    """Chamfer distance and precision / recall / F-score of a predicted cloud against a ground-truth cloud.

    ``bounds = (lo, hi)`` (two 3-vectors) keeps the points of ``pred`` inside the closed box first (DTU's observation
    box).  Distances are ``sqrt(dist2)`` in float64.  ``max_dist``: distances above it are left out of the means and their
    share is reported (DTU's rule).  -> ``accuracy`` (mean distance pred -> gt), ``completeness`` (gt -> pred), ``chamfer``
    (their mean), ``thresholds``: per tau a dict ``tau``, ``precision`` (share of ALL pred points within tau), ``recall``,
    ``fscore``; ``dropped_pred`` / ``dropped_gt``, ``n_pred`` / ``n_gt``.  All reductions are torch float64 on the device and
    are read back once, at the end; with ``bounds`` the crop of ``pred`` reads its count back before (a boolean mask)."""
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
                  generator: Optional[torch.Generator] = None) -> Dict:
    """``evaluate_points(sample_surface(vertices, faces, n_samples)[0], gt_points, ...)``; the result also carries
    ``n_samples``."""
    points, _ = sample_surface(vertices, faces, n_samples, generator)
    out = evaluate_points(points, gt_points, thresholds, max_dist, bounds)
    out["n_samples"] = int(n_samples)
    return out
