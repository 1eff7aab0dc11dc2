"""Depth-prior regularisation: the rendered inverse depth against a per-image prior -- a monocular estimate
(Depth-Anything), DUSt3R or a multi-view stereo depth -- on the map ``render`` already returns with gradients
(``csrc/depth_prior.hip`` behind ``gsr_depth_prior_fwd_bwd``).

    pkg = render(camera, gaussians, pipe, bg, return_depth=True)
    loss = loss + weight * depth_prior_loss(pkg["invdepth"], camera.invdepthmap, camera.depth_mask, mode="pearson")

With ``x`` the rendered value of a pixel, ``y`` the prior and ``w`` the weight (1 without one; upstream's ``depth_mask``,
a multiplier), a pixel is *valid* when ``w > 0`` and ``w``, ``x``, ``y`` are finite; an invalid pixel contributes nothing
and gets gradient 0, never NaN.  The modes:

``"l1"``          ``sum w |x - (scale y + offset)| / (H W)``: upstream 3DGS's term (it divides by all pixels, as the
                  ``.mean()`` of the masked difference does).  Gradient ``w sign(.) / (H W)``, ``sign(0) = 0``.
``"aligned_l1"``  ``sum w |x - (s y + t)| / sum w`` under the weighted least-squares fit of ``x`` on ``y``, ``s = cov_w(x, y)
                  / var_w(y)``, ``t = mean_w(x) - s mean_w(y)``, computed on the device and treated as a constant (no
                  gradient through the fit): the scale-and-shift-invariant form of the sparse-view forks.
``"pearson"``     ``1 - r``, ``r`` the weighted Pearson correlation of ``x`` and ``y``, with its exact gradient
                  ``-(w / Sw) [(y - my) / sqrt(vx vy) - r (x - mx) / vx]``.

The two fitted modes are degenerate below 2 valid pixels or when the weighted variance of ``x`` or of ``y`` is not above
``2^-40`` of its mean square: loss 0, gradient 0, ``s = 1``, ``t = 0``, ``r = 0`` and a flag in the record.  Sums are float64
in a fixed order without atomics: value and gradient are the same bits from run to run.
"""
from __future__ import annotations

import math

import torch

from . import _lib

MODES = {"l1": 0, "aligned_l1": 1, "pearson": 2}
RECORD_WORDS = 8
SUM_WORDS = 7                # int64 count + Sw, Sx, Sy, Sxx, Sxy, Syy
FIT_COUNT_WORD = 16          # where the workspace holds them after a fitted mode, in 8-byte words
BLOCK, MAX_BLOCKS = 256, 1024


def _check_maps(what: str, invdepth, prior, weight, mode, scale, offset):
    """Every refusal, before anything is enqueued and before a GPU is asked for.  Returns (H, W)."""
    maps = (("invdepth", invdepth), ("prior", prior)) + ((("weight", weight),) if weight is not None else ())
    for name, t in maps:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")
    if invdepth.dim() not in (2, 3) or (invdepth.dim() == 3 and invdepth.shape[0] != 1):
        raise ValueError(f"{what}: invdepth must be [1,H,W] (or [H,W]), got {tuple(invdepth.shape)}")
    H, W = int(invdepth.shape[-2]), int(invdepth.shape[-1])
    if H < 1 or W < 1 or H * W > 1 << 28:
        raise ValueError(f"{what}: the maps must hold between 1 and 2^28 pixels, got {H} x {W}")
    for name, t in maps[1:]:
        if tuple(t.shape) not in ((1, H, W), (H, W)):
            raise ValueError(f"{what}: {name} must be [1,{H},{W}] like invdepth, got {tuple(t.shape)}")
        if t.device != invdepth.device:
            raise ValueError(f"{what}: invdepth is on {invdepth.device}, {name} on {t.device}")
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(MODES)}, got {mode!r}")
    for name, v in (("scale", scale), ("offset", offset)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{what}: {name} must be a finite number, got {v!r}")
    if not invdepth.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    return H, W


def _call(invdepth, prior, weight, H, W, mode, scale, offset, want_grad: bool, workspace=None):
    """The launches of one evaluation -> (record float64 [8], dL/dinvdepth or None, workspace)."""
    lib = _lib.load()
    dev = invdepth.device
    xc, yc = invdepth.contiguous(), prior.contiguous()
    wc = None if weight is None else weight.contiguous()
    record = torch.empty(RECORD_WORDS, dtype=torch.float64, device=dev)
    nbytes = lib.gsr_depth_prior_workspace_bytes(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if workspace is None else workspace   # block partials, fit
    grad = torch.empty_like(xc) if want_grad else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_depth_prior_fwd_bwd(xc.data_ptr(), yc.data_ptr(), None if wc is None else wc.data_ptr(), H, W,
                                               MODES[mode], float(scale), float(offset), record.data_ptr(),
                                               None if grad is None else grad.data_ptr(), ws.data_ptr(), ws.numel(),
                                               stream),
                   "gsr_depth_prior_fwd_bwd")
    return record, grad, ws


def _sums(workspace: torch.Tensor):
    """(count int64 0-dim, the six float64 sums ``Sw, Sx, Sy, Sxx, Sxy, Syy``) a fitted mode left in its workspace."""
    words = workspace[8 * FIT_COUNT_WORD:8 * (FIT_COUNT_WORD + SUM_WORDS)]
    return words[:8].view(torch.int64)[0], words[8:].view(torch.float64)


class _DepthPrior(torch.autograd.Function):
    @staticmethod
    def forward(ctx, invdepth, prior, weight, H, W, mode, scale, offset, holder):
        need = ctx.needs_input_grad[0]
        record, grad, _ = _call(invdepth, prior, weight, H, W, mode, scale, offset, need)
        if need:
            ctx.save_for_backward(grad)
        ctx.shape = invdepth.shape
        holder.append(record)
        return record[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        g = g.to(torch.float32)                                      # a 0-dim device tensor: never .item()
        out = (ctx.saved_tensors[0] * g).view(ctx.shape) if ctx.needs_input_grad[0] else None
        return (out, None, None, None, None, None, None, None, None)


def depth_prior_loss(invdepth: torch.Tensor, prior: torch.Tensor, weight=None, *, mode: str = "l1", scale: float = 1.0,
                     offset: float = 0.0, return_record: bool = False):
    """The loss of the module docstring as a 0-dim float32 device tensor, from ``invdepth [1,H,W]`` (or ``[H,W]``) -- the
    ``"invdepth"`` entry of ``render``, the only input that receives a gradient --, ``prior`` of that shape and ``weight``,
    None or of that shape; float32 on one GPU, made contiguous if they are not.  The kernels compute the value and, when
    ``invdepth`` requires a gradient, the unit gradient; the backward multiplies it by the upstream gradient on the
    device.  Nothing is read back.
    scale, offset: the affine applied to the prior in the ``"l1"`` mode (``Camera`` applies ``depth_params.json``'s at load
    and leaves the identity here); ignored by the fitted modes.
    return_record: also return the kernels' record, float64 ``[8]`` on the device: ``(loss, valid pixels, sum w, s, t, r,
    degenerate, 0)``; the loss returned is ``float32(record[0])``."""
    H, W = _check_maps("depth_prior_loss", invdepth, prior, weight, mode, scale, offset)
    holder = []
    loss = _DepthPrior.apply(invdepth, prior, weight, H, W, mode, scale, offset, holder)
    return (loss, holder[0]) if return_record else loss


__all__ = ["depth_prior_loss"]
