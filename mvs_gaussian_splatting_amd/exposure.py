"""Per-image exposure compensation: upstream 3DGS's learnable 3x4 colour affine per training image, applied to the
rendered image before the loss (``csrc/exposure.hip`` behind ``gsr_exposure_apply_fwd`` / ``_bwd``), and the
``exposure.json`` file upstream writes next to the point cloud.

    image = apply_exposure(pkg["render"], gaussians.get_exposure_from_name(camera.image_name))

With ``k`` the input channel and ``c`` the output channel,
``y[c] = x[0]*A[0,c] + x[1]*A[1,c] + x[2]*A[2,c] + A[c,3]`` -- upstream's
``matmul(img.permute(1,2,0), A[:3,:3]).permute(2,0,1) + A[:3,3,None,None]`` -- without a clamp.  The identity
``eye(3,4)`` returns the image and passes the gradient through bit for bit, so a run that starts there begins exactly
as a run without exposures.  ``dL/dA`` is summed in double in a fixed order: the same bits from run to run.
"""
from __future__ import annotations

import json
from typing import Dict, Mapping

import torch

from . import _lib


class _ApplyExposure(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image: torch.Tensor, exposure: torch.Tensor):
        lib = _lib.load()
        xc, ac = image.contiguous(), exposure.contiguous()
        H, W = int(xc.shape[1]), int(xc.shape[2])
        y = torch.empty_like(xc)
        with torch.cuda.device(xc.device):
            stream = torch.cuda.current_stream(xc.device).cuda_stream
            _lib.check(lib.gsr_exposure_apply_fwd(xc.data_ptr(), ac.data_ptr(), H, W, y.data_ptr(), stream),
                       "gsr_exposure_apply_fwd")
        ctx.save_for_backward(xc, ac)
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        xc, ac = ctx.saved_tensors
        need_dx, need_dA = ctx.needs_input_grad
        if not (need_dx or need_dA):
            return None, None
        g = g.to(torch.float32).contiguous()
        H, W = int(xc.shape[1]), int(xc.shape[2])
        dx = torch.empty_like(xc) if need_dx else None
        dA = ws = None
        if need_dA:
            dA = torch.empty((3, 4), dtype=torch.float32, device=xc.device)
            ws = torch.empty(lib.gsr_exposure_workspace_bytes(H, W), dtype=torch.uint8, device=xc.device)   # block sums
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        with torch.cuda.device(xc.device):
            stream = torch.cuda.current_stream(xc.device).cuda_stream
            _lib.check(lib.gsr_exposure_apply_bwd(xc.data_ptr(), ac.data_ptr(), g.data_ptr(), H, W, ptr(dx), ptr(dA),
                                                  ptr(ws), stream), "gsr_exposure_apply_bwd")
        return dx, dA


def apply_exposure(image: torch.Tensor, exposure: torch.Tensor) -> torch.Tensor:
    """``image`` float32 ``[3,H,W]`` (made contiguous if it is not), ``exposure`` float32 ``[3,4]`` on the same device;
    returns the compensated ``[3,H,W]`` image.  Differentiable in both; a gradient is computed only for the input that
    requires one.  The exposure is read on the device: no host synchronisation in either direction."""
    if not isinstance(image, torch.Tensor) or not isinstance(exposure, torch.Tensor) or not image.is_cuda \
            or not exposure.is_cuda:
        raise _lib.GsrError("apply_exposure needs ROCm GPU tensors (no CPU path)")
    if image.dtype != torch.float32 or exposure.dtype != torch.float32:
        raise TypeError(f"apply_exposure expects float32 tensors, got {image.dtype} and {exposure.dtype}")
    if image.dim() != 3 or image.shape[0] != 3 or tuple(exposure.shape) != (3, 4):
        raise ValueError(f"apply_exposure expects a [3,H,W] image and a [3,4] exposure, got {tuple(image.shape)} and "
                         f"{tuple(exposure.shape)}")
    if image.device != exposure.device:
        raise ValueError(f"the image is on {image.device}, the exposure on {exposure.device}")
    if image.shape[1] == 0 or image.shape[2] == 0:
        raise ValueError("apply_exposure needs a non-empty image")
    return _ApplyExposure.apply(image, exposure)


def save_exposures(path: str, mapping: Mapping[str, int], tensor: torch.Tensor) -> None:
    """Write upstream's ``exposure.json``: ``{image_name: 3x4 nested list}`` with row ``mapping[image_name]`` of
    ``tensor [N,3,4]``.  A float32 value is written as the double of the same value, so ``load_exposures`` gets it back
    exactly.  Host code."""
    rows = tensor.detach().cpu()
    if rows.dim() != 3 or tuple(rows.shape[1:]) != (3, 4):
        raise ValueError(f"exposures must be [N,3,4], got {tuple(rows.shape)}")
    out = {}
    for name, idx in mapping.items():
        if not 0 <= int(idx) < rows.shape[0]:
            raise ValueError(f"exposure_mapping[{name!r}] = {idx} is outside the {rows.shape[0]} rows")
        out[name] = rows[int(idx)].tolist()
    with open(path, "w") as f:
        json.dump(out, f, indent=2)


def load_exposures(path: str, device=None) -> Dict[str, torch.Tensor]:
    """Read ``exposure.json`` into ``{image_name: float32 [3,4] tensor}`` (on ``device``; default the CPU): what
    ``GaussianModel.pretrained_exposures`` holds.  Host code."""
    with open(path) as f:
        raw = json.load(f)
    out = {}
    for name, rows in raw.items():
        t = torch.tensor(rows, dtype=torch.float64).to(torch.float32)
        if tuple(t.shape) != (3, 4):
            raise ValueError(f"{path}: the exposure of {name!r} is {tuple(t.shape)}, not 3x4")
        out[name] = t if device is None else t.to(device)
    return out


__all__ = ["apply_exposure", "save_exposures", "load_exposures"]
