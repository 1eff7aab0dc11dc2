"""Which depth is "the surface" of a rendered frame: 2DGS's blend of the expected depth ``depth / alpha`` and the median
depth (``render(return_median_depth=True)``) by its ``depth_ratio`` -- 0 for unbounded scenes, 1 for
bounded ones and for every mesh it publishes.  Plain torch ops on the maps: differentiable where the maps are, on
whatever device they live.

    pkg = render(camera, gaussians, pipe, bg, return_depth=True, return_median_depth=True)
    surface = surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], depth_ratio=1.0)

``plane_depth`` is the third depth, PGSR's unbiased one (``csrc/plane_depth.hip``): the pixel's ray met
with the blended plane of ``render(return_plane_depth=True)``, exact on a planar surface at any tilt where the expected
depth bends towards the camera.  It is a HIP kernel and needs GPU maps.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib


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


def blend_plane_depth(plane: torch.Tensor, median: Optional[torch.Tensor], depth_ratio: float,
                      what: str = "blend_plane_depth") -> torch.Tensor:
    """``(1 - r) plane + r median`` where ``plane > 0`` and 0 (no surface) elsewhere: 2DGS's ``depth_ratio`` applied to
    the unbiased depth of ``plane_depth`` as ``surface_depth`` applies it to the expected depth.  With ``median=None`` or
    ``r = 0`` the result IS ``plane``, the same tensor."""
    r = _check_ratio(what, depth_ratio, median)
    if median is None or r == 0.0:
        return plane
    _check_median(what, plane, median)
    median = median.view(plane.shape)
    return torch.where(plane > 0, median if r == 1.0 else (1.0 - r) * plane + r * median, torch.zeros_like(plane))


def plane_depth_raw(normal, distance, alpha, H, W, tanfovx, tanfovy, alpha_min, min_cos, want_grads: bool, out=None):
    """One launch of ``gsr_plane_depth_fwd`` on contiguous device maps -> ``(z [H,W], dz/dD [H,W] or None, dz/dN [3,H,W]
    or None)``; ``out``: the three tensors to write instead of fresh ones."""
    lib = _lib.load()
    dev = distance.device
    if out is None:
        z = torch.empty((H, W), dtype=torch.float32, device=dev)
        ud = torch.empty((H, W), dtype=torch.float32, device=dev) if want_grads else None
        un = torch.empty((3, H, W), dtype=torch.float32, device=dev) if want_grads else None
    else:
        z, ud, un = out
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_plane_depth_fwd(normal.data_ptr(), distance.data_ptr(), alpha.data_ptr(), H, W, float(tanfovx),
                                           float(tanfovy), float(alpha_min), float(min_cos), z.data_ptr(),
                                           None if ud is None else ud.data_ptr(), None if un is None else un.data_ptr(),
                                           stream), "gsr_plane_depth_fwd")
    return z, ud, un


def plane_depth_backward_raw(grad_z, ud, un, H, W, out=None):
    """``gsr_plane_depth_bwd``: the unit gradients times the upstream map -> ``(dL/dD [H,W], dL/dN [3,H,W])``."""
    lib = _lib.load()
    g_d, g_n = (torch.empty_like(ud), torch.empty_like(un)) if out is None else out
    with torch.cuda.device(ud.device):
        stream = torch.cuda.current_stream(ud.device).cuda_stream
        _lib.check(lib.gsr_plane_depth_bwd(grad_z.data_ptr(), ud.data_ptr(), un.data_ptr(), H, W, g_d.data_ptr(),
                                           g_n.data_ptr(), stream), "gsr_plane_depth_bwd")
    return g_d, g_n


class _PlaneDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal, distance, alpha, H, W, tanfovx, tanfovy, alpha_min, min_cos):
        need = any(ctx.needs_input_grad[:2])
        z, ud, un = plane_depth_raw(normal.detach().contiguous(), distance.detach().contiguous(),
                                    alpha.detach().contiguous(), H, W, tanfovx, tanfovy, alpha_min, min_cos, need)
        if need:
            ctx.save_for_backward(ud, un)
        ctx.shapes = (normal.shape, distance.shape, H, W)
        return z.view(1, H, W)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ud, un = ctx.saved_tensors
        n_shape, d_shape, H, W = ctx.shapes
        g_d, g_n = plane_depth_backward_raw(g.to(torch.float32).contiguous(), ud, un, H, W)
        return (g_n.view(n_shape) if ctx.needs_input_grad[0] else None,
                g_d.view(d_shape) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None, None)


def plane_depth(normal: torch.Tensor, distance: torch.Tensor, alpha: torch.Tensor, tanfovx: float, tanfovy: float,
                alpha_min: float = 0.5, min_cos: float = 0.05) -> torch.Tensor:
    """PGSR's unbiased depth ``[1,H,W]`` from the un-normalised maps ``normal [3,H,W]`` (``sum w n``), ``distance
    [1,H,W]`` (``sum w d``) and ``alpha [1,H,W]`` -- the ``"normal"``, ``"distance"`` and ``"alpha"`` entries of
    ``render(return_plane_depth=True)`` -- float32 on one GPU.  With ``r = ((x - cx) / fx, (y - cy) / fy, 1)``, ``fx = W /
    (2 tanfovx)``, ``cx = (W - 1) / 2`` (the convention of ``tsdf.py`` and ``normal_consistency.py``) and ``c = -(N . r)``:
    ``z = D / c``, the depth at which the pixel's ray meets the blended plane, where ``alpha >= alpha_min``, ``D > 0``,
    ``c > 0``, ``c >= min_cos |N| |r|`` and everything is finite; 0 (no surface) elsewhere.  ``alpha`` cancels in the
    quotient: it decides validity and gets no gradient.  One kernel call computes ``z`` and, when ``normal`` or
    ``distance`` requires a gradient, the unit gradients ``dz/dD = 1 / c`` and ``dz/dN = (D / c^2) r``; the backward
    scales them by the upstream map in one more launch.  Validity is a decision and carries no gradient.  The same bits
    from run to run; nothing is read back.  The defaults of ``alpha_min`` and ``min_cos`` are those of ``tsdf.fuse_views``
    and ``mvs.multi_view_ncc_loss``.  Refusals as ``normal_consistency_loss``; ``ValueError`` for ``min_cos`` outside
    [0, 1)."""
    from .normal_consistency import _check_maps
    if not isinstance(normal, torch.Tensor):
        raise TypeError(f"plane_depth: normal must be a torch.Tensor, got {type(normal).__name__}")
    if not (isinstance(min_cos, (int, float)) and 0.0 <= min_cos < 1.0):
        raise ValueError(f"plane_depth: min_cos must lie in [0, 1), got {min_cos!r}")
    H, W = _check_maps("plane_depth", distance, alpha, normal, tanfovx, tanfovy, alpha_min)
    return _PlaneDepth.apply(normal, distance, alpha, H, W, tanfovx, tanfovy, alpha_min, min_cos)


__all__ = ["surface_depth", "blend_weighted_depth", "plane_depth", "blend_plane_depth"]
