"""Training under a per-image mask (``csrc/masked_loss.hip`` behind ``gsr_masked_l1_dssim_loss_fwd_bwd`` and
``gsr_alpha_mask_loss_fwd_bwd``): the colour loss that ignores what the mask hides, and the silhouette
term that keeps the rendered opacity inside it.

    loss = masked_l1_dssim_loss(image, camera.original_image, camera.alpha_mask, opt.lambda_dssim, normalize="image")
    loss = loss + weight * alpha_mask_loss(pkg["alpha"], camera.alpha_mask, mode="bce")

``mask`` is ``[H,W]`` or ``[1,H,W]`` float32 with values in ``[0, 1]``, non-zero keeps the pixel (COLMAP's polarity).  The
range is the caller's to keep: it is not checked on the device.  With ``x' = m x`` and ``y' = m gt`` (float32 products,
``+0`` where ``m`` is 0) and ``S`` the SSIM map of ``x'``, ``y'`` -- the window, padding and constants of ``l1_dssim_loss``:

``normalize="image"``  ``L1 = sum|x' - y'| / (C H W)``, ``Ds = 1 - sum S / (C H W)``: upstream 3DGS's (``alpha_mask``) and
                       gsplat's (``masks``) rule, the unmasked loss of the pre-multiplied images.
``normalize="mask"``   ``Z = C sum m``; ``L1 = sum|x' - y'| / Z``, ``Ds = sum_{c,p} m_p (1 - S_cp) / Z``: the mean over what
                       the mask keeps.  ``Z = 0`` is degenerate: loss 0, gradient 0, a flag in the record.

``loss = (1 - lambda) L1 + lambda Ds``; the gradient goes to the image only, ``dL/dx = m dL/dx'``, exactly 0 where ``m`` is 0.
``alpha_mask_loss`` is ``mean|a - m|`` (``"l1"``) or ``-mean(m log a^ + (1 - m) log(1 - a^))`` with ``a^ = clamp(a, 1e-6,
1 - 1e-6)`` (``"bce"``, gradient 0 where ``a`` was clamped).  Sums are float64 in a fixed order without atomics: value and
gradient are the same bits from run to run.  There is no CPU path.
"""
from __future__ import annotations

import torch

from . import _lib

NORMALIZE = {"image": 0, "mask": 1}
ALPHA_MODES = {"l1": 0, "bce": 1}
RECORD_WORDS = 8             # loss, L1, Ds, Z, sum m, degenerate, 0, 0
ALPHA_RECORD_WORDS = 4       # loss, H W, mode, 0


def _need_f32(what: str, **tensors):
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: {name} must be float32, got {t.dtype}")


def _check_mask(what: str, mask, H: int, W: int, device):
    if tuple(mask.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"{what}: mask must be [{H},{W}] or [1,{H},{W}], got {tuple(mask.shape)}")
    if mask.device != device:
        raise ValueError(f"{what}: the image is on {device}, mask on {mask.device}")


def _check_images(image, gt, mask, lambda_dssim, normalize):
    """Every refusal, before anything is enqueued and before a GPU is asked for.  Returns (C, H, W)."""
    what = "masked_l1_dssim_loss"
    _need_f32(what, image=image, gt=gt, mask=mask)
    if image.dim() != 3 or image.shape != gt.shape:
        raise ValueError(f"{what}: image and gt must be [C,H,W] of one shape, got {tuple(image.shape)} and {tuple(gt.shape)}")
    Cn, H, W = (int(v) for v in image.shape)
    if Cn < 1 or Cn > 65535 or H < 1 or W < 1 or H * W > 1 << 28:
        raise ValueError(f"{what}: needs 1 <= C <= 65535 and between 1 and 2^28 pixels, got {tuple(image.shape)}")
    if gt.device != image.device:
        raise ValueError(f"{what}: image is on {image.device}, gt on {gt.device}")
    _check_mask(what, mask, H, W, image.device)
    if not isinstance(normalize, str) or normalize not in NORMALIZE:
        raise ValueError(f"{what}: normalize must be one of {sorted(NORMALIZE)}, got {normalize!r}")
    if isinstance(lambda_dssim, bool) or not isinstance(lambda_dssim, (int, float)) or not 0.0 <= lambda_dssim <= 1.0:
        raise ValueError(f"{what}: lambda_dssim must be a number in [0, 1], got {lambda_dssim!r}")
    if not image.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    return Cn, H, W


def _call(image, gt, mask, lambda_dssim, normalize, want_grad: bool, workspace=None):
    """The launches of one evaluation -> (record float64 [8], dL/dimage or None, workspace)."""
    lib = _lib.load()
    dev = image.device
    xc, gc, mc = image.contiguous(), gt.contiguous(), mask.contiguous()
    Cn, H, W = (int(v) for v in xc.shape)
    record = torch.empty(RECORD_WORDS, dtype=torch.float64, device=dev)
    nbytes = lib.gsr_masked_l1_dssim_workspace_bytes(Cn, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if workspace is None else workspace   # maps, partials, sum m
    grad = torch.empty_like(xc) if want_grad else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_masked_l1_dssim_loss_fwd_bwd(xc.data_ptr(), gc.data_ptr(), mc.data_ptr(), Cn, H, W,
                                                        float(lambda_dssim), NORMALIZE[normalize], record.data_ptr(),
                                                        None if grad is None else grad.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), stream),
                   "gsr_masked_l1_dssim_loss_fwd_bwd")
    return record, grad, ws


class _MaskedL1Dssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, mask, lambda_dssim, normalize, holder):
        need = ctx.needs_input_grad[0]
        record, grad, _ = _call(image, gt, mask, lambda_dssim, normalize, need)
        if need:
            ctx.save_for_backward(grad)
        ctx.shape = image.shape
        holder.append(record)
        return record[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        g = g.to(torch.float32)                                      # a 0-dim device tensor: never .item()
        out = (ctx.saved_tensors[0] * g).view(ctx.shape) if ctx.needs_input_grad[0] else None
        return (out, None, None, None, None, None)


def masked_l1_dssim_loss(image: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, lambda_dssim: float = 0.2,
                         normalize: str = "image", *, return_record: bool = False):
    """The loss of the module docstring as a 0-dim float32 device tensor, from ``image`` and ``gt`` ``[C,H,W]`` and ``mask``
    ``[H,W]`` or ``[1,H,W]``, float32 on one GPU, made contiguous if they are not.  The kernels compute the value and, when
    ``image`` requires a gradient, the unit gradient; the backward multiplies it by the upstream gradient on the device.
    ``gt`` and ``mask`` receive none.  Nothing is read back: ``sum m`` stays on the device.
    return_record: also return the kernels' record, float64 ``[8]`` on the device: ``(loss, L1, Ds, Z, sum m (0 in image
    mode), degenerate, 0, 0)``; the loss returned is ``float32(record[0])``."""
    _check_images(image, gt, mask, lambda_dssim, normalize)
    holder = []
    loss = _MaskedL1Dssim.apply(image, gt, mask, float(lambda_dssim), normalize, holder)
    return (loss, holder[0]) if return_record else loss


def _check_alpha(alpha, mask, mode):
    what = "alpha_mask_loss"
    _need_f32(what, alpha=alpha, mask=mask)
    if alpha.dim() not in (2, 3) or (alpha.dim() == 3 and alpha.shape[0] != 1):
        raise ValueError(f"{what}: alpha must be [1,H,W] (or [H,W]), got {tuple(alpha.shape)}")
    H, W = int(alpha.shape[-2]), int(alpha.shape[-1])
    if H < 1 or W < 1 or H * W > 1 << 28:
        raise ValueError(f"{what}: the maps must hold between 1 and 2^28 pixels, got {H} x {W}")
    _check_mask(what, mask, H, W, alpha.device)
    if not isinstance(mode, str) or mode not in ALPHA_MODES:
        raise ValueError(f"{what}: mode must be one of {sorted(ALPHA_MODES)}, got {mode!r}")
    if not alpha.is_cuda:
        raise _lib.GsrError(f"{what} needs ROCm GPU tensors (no CPU path)")
    return H, W


def _call_alpha(alpha, mask, mode, want_grad: bool):
    """-> (record float64 [4], dL/dalpha or None)."""
    lib = _lib.load()
    dev = alpha.device
    ac, mc = alpha.contiguous(), mask.contiguous()
    H, W = int(ac.shape[-2]), int(ac.shape[-1])
    record = torch.empty(ALPHA_RECORD_WORDS, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.gsr_alpha_mask_workspace_bytes(H, W), dtype=torch.uint8, device=dev)     # block partials
    grad = torch.empty_like(ac) if want_grad else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_alpha_mask_loss_fwd_bwd(ac.data_ptr(), mc.data_ptr(), H, W, ALPHA_MODES[mode], record.data_ptr(),
                                                   None if grad is None else grad.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   stream),
                   "gsr_alpha_mask_loss_fwd_bwd")
    return record, grad


class _AlphaMask(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, mask, mode):
        need = ctx.needs_input_grad[0]
        record, grad = _call_alpha(alpha, mask, mode, need)
        if need:
            ctx.save_for_backward(grad)
        ctx.shape = alpha.shape
        return record[0].to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        g = g.to(torch.float32)
        out = (ctx.saved_tensors[0] * g).view(ctx.shape) if ctx.needs_input_grad[0] else None
        return (out, None, None)


def alpha_mask_loss(alpha: torch.Tensor, mask: torch.Tensor, mode: str = "bce") -> torch.Tensor:
    """The silhouette term of 2DGS / NeuS / PGSR object captures as a 0-dim float32 device tensor: the rendered opacity
    ``alpha`` (``render(..., return_depth=True)["alpha"]``, ``[1,H,W]`` or ``[H,W]``) against ``mask`` (``[H,W]`` or
    ``[1,H,W]``), both float32 on one GPU.  ``mode``: ``"l1"`` or ``"bce"`` (module docstring).  Only ``alpha`` receives a
    gradient."""
    _check_alpha(alpha, mask, mode)
    return _AlphaMask.apply(alpha, mask, mode)


__all__ = ["masked_l1_dssim_loss", "alpha_mask_loss"]
