"""Drop-in for ``simple_knn._C.distCUDA2`` (``scene/gaussian_model.py:21,210``): mean squared distance of every
point to its three nearest other points, exact, on the GPU (``csrc/knn.hip``).

Contract (restated and checked by ``tests/knn_restate.py`` / ``tests/test_gpu_knn.py``):
  - ``points`` is ``[N, 3]`` on the GPU, any float dtype, any strides; float64 input is rounded to float32 first and
    the distances are those of the rounded coordinates.  The result is float32 ``[N]``, detached.
  - Coincident points are neighbours at distance 0; a point is left out by its index only.
  - Coordinates must be finite: the result for NaN / Inf input is unspecified.
  - With fewer than four points a missing neighbour counts as FLT_MAX, the start value of the three best distances
    (as in upstream ``simple_knn`` to our knowledge; unpinned, upstream is absent): ``N = 1, 2`` give ``+inf``,
    ``N = 3`` gives ``(d1 + d2 + FLT_MAX) / 3``, a huge finite number.  ``N = 0`` gives an empty result.
"""
from __future__ import annotations

import torch

from . import _lib


@torch.no_grad()
def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    if not points.is_cuda:
        raise _lib.GsrError("distCUDA2 needs a ROCm GPU tensor (no CPU path)")
    pts = points.detach().float().contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [N, 3]")
    N = int(pts.shape[0])
    out = torch.empty(N, dtype=torch.float32, device=pts.device)
    nbytes = lib.gsr_knn3_workspace_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pts.device)
    with torch.cuda.device(pts.device):
        stream = torch.cuda.current_stream(pts.device).cuda_stream
        _lib.check(lib.gsr_dist2_knn3(pts.data_ptr(), N, out.data_ptr(), ws.data_ptr(), nbytes, stream), "gsr_dist2_knn3")
    return out
