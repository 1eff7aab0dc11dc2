"""Depth-normal consistency: the self-supervised normal term of 2DGS (also GOF, PGSR, RaDe-GS) on the maps ``render``
already returns with gradients (``csrc/normal_consistency.hip`` behind ``gsr_normal_consistency_fwd_bwd``; DESIGN.md
§7.15).

    pkg = render(camera, gaussians, pipe, bg, return_depth=True, return_normals=True)
    loss = loss + 0.05 * normal_consistency_loss(pkg["depth"], pkg["alpha"], pkg["normal"],
                                                 math.tan(camera.FoVx * 0.5), math.tan(camera.FoVy * 0.5))

With ``d = depth / alpha`` on the covered pixels (``alpha >= alpha_min``) back-projected to ``P = (d (x - cx) / fx,
d (y - cy) / fy, d)``, ``fx = W / (2 tanfovx)``, ``cx = (W - 1) / 2`` (the convention of ``tsdf.py``), the normal of the
depth surface is ``n_d = c / |c|`` with ``c = (P(x,y+1) - P(x,y-1)) x (P(x+1,y) - P(x-1,y))`` -- it faces the camera, as
``gaussian_normals`` does -- on the interior pixels whose four axis neighbours are covered too and whose ``|c|^2`` is
finite and above 1e-20.  The loss is ``sum_valid (alpha - normal . n_d) / (H W)``: ``alpha (1 - cos)`` where all
contributors of a pixel share one normal.  The gradients reach ``depth`` (through ``n_d`` of the four neighbours),
``alpha`` and ``normal``; which pixels are valid is a decision and carries none.  Value, gradients and the depth normals
come from one launch and are the same bits from run to run.

``median=`` / ``depth_ratio=`` (2DGS's ``depth_ratio``): the surface is the blend ``(1 - r) depth / alpha
+ r median`` of the expected and the median depth (``render(return_median_depth=True)``).  The kernel is fed ``depth' =
(1 - r) depth + r median alpha`` -- built with torch ops, so the gradients reach all three maps -- whose quotient by
``alpha`` is that blend.  With ``median=None`` or ``r = 0`` the tensors passed are the ones passed without the arguments.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from .surface import blend_weighted_depth


def _check_maps(what: str, depth, alpha, normal, tanfovx, tanfovy, alpha_min):
    """Every refusal, before anything is enqueued and before a GPU is asked for.  Returns (H, W)."""
    maps = (("depth", depth), ("alpha", alpha)) + ((("normal", normal),) if normal is not None else ())
    for name, t in maps:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if depth.dim() not in (2, 3) or (depth.dim() == 3 and depth.shape[0] != 1):
        raise ValueError(f"{what}: depth must be [1,H,W] (or [H,W]), got {tuple(depth.shape)}")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if H < 1 or W < 1 or H * W > 1 << 28:
        raise ValueError(f"{what}: the maps must hold between 1 and 2^28 pixels, got {H} x {W}")
    if tuple(alpha.shape) not in ((1, H, W), (H, W)):
        raise ValueError(f"{what}: alpha must be [1,{H},{W}] like depth, got {tuple(alpha.shape)}")
    if normal is not None and tuple(normal.shape) != (3, H, W):
        raise ValueError(f"{what}: normal must be [3,{H},{W}], got {tuple(normal.shape)}")
    for name, t in maps[1:]:
        if t.device != depth.device:
            raise ValueError(f"{what}: depth is on {depth.device}, {name} on {t.device}")
    for name, v in (("tanfovx", tanfovx), ("tanfovy", tanfovy)):
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0):
            raise ValueError(f"{what}: {name} must be a positive finite number, got {v!r}")
    if not (isinstance(alpha_min, (int, float)) and 0.0 < alpha_min <= 1.0):
        raise ValueError(f"{what}: alpha_min must lie in (0, 1], got {alpha_min!r}")
    if not depth.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    return H, W


def _call(depth, alpha, normal, H, W, tanfovx, tanfovy, alpha_min, want_grads: bool, want_normals: bool):
    """One launch of the fused kernel -> (record [4], (dL/ddepth, dL/dalpha, dL/dnormal) or None, depth_normal or None)."""
    lib = _lib.load()
    dev = depth.device
    dc, ac, nc = depth.contiguous(), alpha.contiguous(), normal.contiguous()
    record = torch.empty(4, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.gsr_normal_consistency_workspace_bytes(H, W), dtype=torch.uint8, device=dev)   # block partials
    grads = (torch.empty_like(dc), torch.empty_like(ac), torch.empty_like(nc)) if want_grads else None
    dn = torch.empty((3, H, W), dtype=torch.float32, device=dev) if want_normals else None
    gp = [g.data_ptr() for g in grads] if want_grads else [None, None, None]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_normal_consistency_fwd_bwd(dc.data_ptr(), ac.data_ptr(), nc.data_ptr(), H, W, float(tanfovx),
                                                      float(tanfovy), float(alpha_min), record.data_ptr(), *gp,
                                                      None if dn is None else dn.data_ptr(), ws.data_ptr(), stream),
                   "gsr_normal_consistency_fwd_bwd")
    return record, grads, dn


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, normal, H, W, tanfovx, tanfovy, alpha_min, holder):
        need = any(ctx.needs_input_grad[:3])
        record, grads, _ = _call(depth, alpha, normal, H, W, tanfovx, tanfovy, alpha_min, need, False)
        if need:
            ctx.save_for_backward(*grads)
        ctx.shapes = (depth.shape, alpha.shape, normal.shape)
        holder.append(record)
        return record[0]

    @staticmethod
    def backward(ctx, g):
        g = g.to(torch.float32)                                      # a 0-dim device tensor: never .item()
        out = [(u * g).view(shape) if need else None
               for u, shape, need in zip(ctx.saved_tensors, ctx.shapes, ctx.needs_input_grad[:3])]
        return (*out, None, None, None, None, None, None)


def normal_consistency_loss(depth: torch.Tensor, alpha: torch.Tensor, normal: torch.Tensor, tanfovx: float,
                            tanfovy: float, alpha_min: float = 0.5, return_record: bool = False, median=None,
                            depth_ratio: float = 0.0):
    """The loss of the module docstring as a 0-dim device tensor, from ``depth [1,H,W]``, ``alpha [1,H,W]`` and
    ``normal [3,H,W]`` -- the ``"depth"``, ``"alpha"`` and ``"normal"`` entries of ``render`` -- float32 on one GPU (made
    contiguous if they are not).  One kernel call computes the value and, when an input requires a gradient, the three
    unit gradients; the backward multiplies them by the upstream gradient on the device.  Nothing is read back.
    ``alpha_min`` is the coverage threshold, the default that of ``tsdf.fuse_views``.
    return_record: also return the kernel's record, float32 ``[4]`` on the device: ``(loss, n_valid as uint32 bits, 0,
    0)`` (``record.view(torch.int32)[1]`` is the number of valid pixels).
    median, depth_ratio: the ``"median_depth"`` entry of ``render`` and 2DGS's ``depth_ratio`` in [0, 1] (module
    docstring); ``depth_ratio > 0`` needs ``median``."""
    if not isinstance(normal, torch.Tensor):
        raise TypeError(f"normal_consistency_loss: normal must be a torch.Tensor, got {type(normal).__name__}")
    if median is not None or depth_ratio != 0.0:
        if not isinstance(depth, torch.Tensor) or not isinstance(alpha, torch.Tensor):
            raise TypeError("normal_consistency_loss: depth and alpha must be torch.Tensors")
        depth = blend_weighted_depth(depth, alpha, median, depth_ratio, "normal_consistency_loss")
    H, W = _check_maps("normal_consistency_loss", depth, alpha, normal, tanfovx, tanfovy, alpha_min)
    holder = []
    loss = _NormalConsistency.apply(depth, alpha, normal, H, W, tanfovx, tanfovy, alpha_min, holder)
    return (loss, holder[0]) if return_record else loss


@torch.no_grad()
def depth_to_normals(depth: torch.Tensor, alpha: torch.Tensor, tanfovx: float, tanfovy: float,
                     alpha_min: float = 0.5, median=None, depth_ratio: float = 0.0) -> torch.Tensor:
    """``[3,H,W]`` view-space unit normals of the depth surface ``depth / alpha`` (+z forward, x right, y down; facing
    the camera), zeros on the pixels that are not valid (module docstring).  The loss kernel run forward only: the same
    bits as the normals it uses.  No gradient.  ``median`` / ``depth_ratio``: as in ``normal_consistency_loss``."""
    if median is not None or depth_ratio != 0.0:
        if not isinstance(depth, torch.Tensor) or not isinstance(alpha, torch.Tensor):
            raise TypeError("depth_to_normals: depth and alpha must be torch.Tensors")
        depth = blend_weighted_depth(depth, alpha, median, depth_ratio, "depth_to_normals")
    H, W = _check_maps("depth_to_normals", depth, alpha, None, tanfovx, tanfovy, alpha_min)
    zeros = torch.zeros((3, H, W), dtype=torch.float32, device=depth.device)
    return _call(depth, alpha, zeros, H, W, tanfovx, tanfovy, alpha_min, False, True)[2]


__all__ = ["normal_consistency_loss", "depth_to_normals"]
