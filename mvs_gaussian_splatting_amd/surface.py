"""Which depth is "the surface" of a rendered frame: 2DGS's blend of the expected depth ``depth / alpha`` and the median
depth (``render(return_median_depth=True)``) by its ``depth_ratio`` -- 0 for unbounded scenes, 1 for
bounded ones and for every mesh it publishes.  Plain torch ops on the maps: differentiable where the maps are, on
whatever device they live.

    pkg = render(camera, gaussians, pipe, bg, return_depth=True, return_median_depth=True)
    surface = surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], depth_ratio=1.0)
"""
from __future__ import annotations

import math
from typing import Optional

import torch


def _check_ratio(what: str, depth_ratio, median) -> float:
    if not (isinstance(depth_ratio, (int, float)) and math.isfinite(depth_ratio) and 0.0 <= depth_ratio <= 1.0):
        raise ValueError(f"{what}: depth_ratio must lie in [0, 1], got {depth_ratio!r}")
    if depth_ratio > 0.0 and median is None:
        raise ValueError(f"{what}: depth_ratio > 0 needs the median-depth map (render(return_median_depth=True))")
    return float(depth_ratio)


def _check_median(what: str, depth: torch.Tensor, median) -> None:
    if not isinstance(median, torch.Tensor):
        raise TypeError(f"{what}: median must be a torch.Tensor, got {type(median).__name__}")
    if median.dtype != depth.dtype:
        raise TypeError(f"{what}: median must be {depth.dtype} like depth, got {median.dtype}")
    if median.numel() != depth.numel() or tuple(median.shape[-2:]) != tuple(depth.shape[-2:]):
        raise ValueError(f"{what}: median must have the shape of depth {tuple(depth.shape)}, got {tuple(median.shape)}")
    if median.device != depth.device:
        raise ValueError(f"{what}: depth is on {depth.device}, median on {median.device}")


def surface_depth(depth: torch.Tensor, alpha: torch.Tensor, median: Optional[torch.Tensor], depth_ratio: float,
                  alpha_min: float = 0.5) -> torch.Tensor:
    """``(1 - r) depth / alpha + r median`` where ``alpha >= alpha_min`` and 0 (no surface) elsewhere, ``r = depth_ratio``
    in [0, 1]: ``depth`` and ``alpha`` are the ``"depth"`` (``sum w z``) and ``"alpha"`` entries of ``render``, ``median``
    its ``"median_depth"`` entry (may be None at ``r = 0``).  At ``r = 0`` the result is the expected depth ``tsdf.fuse_views``
    has always integrated, bit for bit; at ``r = 1`` it is the median depth on the covered pixels, bit for bit."""
    r = _check_ratio("surface_depth", depth_ratio, median)
    expected = depth / alpha
    if r > 0.0:
        _check_median("surface_depth", depth, median)
        median = median.view(depth.shape)
        expected = median if r == 1.0 else (1.0 - r) * expected + r * median
    return torch.where(alpha >= alpha_min, expected, torch.zeros_like(depth))


def blend_weighted_depth(depth: torch.Tensor, alpha: torch.Tensor, median: Optional[torch.Tensor],
                         depth_ratio: float, what: str = "blend_weighted_depth") -> torch.Tensor:
    """``depth' = (1 - r) depth + r median alpha``: the alpha-weighted depth whose quotient ``depth' / alpha`` is the
    blend of ``surface_depth``, for consumers that divide by ``alpha`` themselves (the normal-consistency kernel).
    Differentiable torch ops.  With ``median=None`` or ``r = 0`` the result IS ``depth``, the same tensor."""
    r = _check_ratio(what, depth_ratio, median)
    if median is None or r == 0.0:
        return depth
    _check_median(what, depth, median)
    return (1.0 - r) * depth + r * (median.view(depth.shape) * alpha.view(depth.shape))


__all__ = ["surface_depth", "blend_weighted_depth"]
