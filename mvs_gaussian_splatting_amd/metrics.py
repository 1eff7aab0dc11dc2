"""Evaluation of rendered views, the part of the reference's ``train.py:210-235`` (``training_report``) and
``metrics.py:71-78`` that sits around ``render``: L1, PSNR, SSIM and the 8-bit HWC image of a view from one fused HIP
pass (``csrc/metrics.hip``), accumulated on the device in double so that a report reads back once.

    acc = evaluate_views(scene.getTestCameras(), gaussians, pipe, background)      # {"l1", "psnr", "ssim", "n"}

No function here synchronises with the host except ``EvalAccumulator.result()``.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib

_ROUNDING = {"nearest": 0, "truncate": _lib.EVAL_U8_TRUNCATE}


def _need_gpu(name: str, *tensors: torch.Tensor) -> None:
    for t in tensors:
        if not t.is_cuda:
            raise _lib.GsrError(f"{name} needs ROCm GPU tensors (no CPU path)")


def _image3(name: str, t: torch.Tensor) -> torch.Tensor:
    """[3,H,W] or [1,3,H,W] float32 -> contiguous [3,H,W]."""
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 3 or t.shape[0] != 3 or t.dtype != torch.float32 or t.numel() == 0:
        raise TypeError(f"{name} expects float32 [3,H,W] (or [1,3,H,W]) images, got {t.dtype} {tuple(t.shape)}")
    return t.detach().contiguous()


def _rounding_flag(rounding: str) -> int:
    if rounding not in _ROUNDING:
        raise ValueError(f"rounding must be 'nearest' or 'truncate', got {rounding!r}")
    return _ROUNDING[rounding]


class EvalAccumulator:
    """The running sums of a report, ``double[4] = {sum l1, sum psnr, sum ssim, views}`` on the device (the reference's
    ``l1_test += ....double()``).  Hand it to ``image_metrics(accumulate=...)``; ``result()`` is the one read-back."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.GsrError("EvalAccumulator needs a ROCm GPU device (no CPU path)")
        self.sums = torch.zeros(4, dtype=torch.float64, device=device)
        self._ssim_views = 0
        self._views = 0

    def reset(self) -> None:
        self.sums.zero_()
        self._ssim_views = self._views = 0

    def _note(self, with_ssim: bool) -> None:
        self._views += 1
        self._ssim_views += int(with_ssim)

    def result(self) -> dict:
        """Means over the accumulated views (divided in double): {"l1", "psnr", "ssim" (None unless every view was taken
        with SSIM), "n"}.  Synchronises with the device."""
        if self._ssim_views not in (0, self._views):
            raise ValueError("some views were accumulated with SSIM and some without")
        s = self.sums.cpu()
        n = float(s[3])
        if n == 0:
            return {"l1": float("nan"), "psnr": float("nan"), "ssim": None, "n": 0}
        return {"l1": float(s[0]) / n, "psnr": float(s[1]) / n, "ssim": float(s[2]) / n if self._ssim_views else None,
                "n": int(n)}


def _eval(name: str, image: torch.Tensor, gt: torch.Tensor, flags: int, out_u8: Optional[torch.Tensor] = None,
          accumulate: Optional[EvalAccumulator] = None) -> torch.Tensor:
    """-> the view's float32 record (``_lib.EVAL_VIEW_FLOATS``) on the device."""
    _need_gpu(name, image, gt)
    x, g = _image3(name, image), _image3(name, gt)
    if x.shape != g.shape or x.device != g.device:
        raise TypeError(f"{name}: the two images differ in shape or device ({tuple(x.shape)} vs {tuple(g.shape)})")
    lib = _lib.load()
    _, H, W = (int(v) for v in x.shape)
    if out_u8 is not None and not (out_u8.is_cuda and out_u8.device == x.device and out_u8.dtype == torch.uint8
                                   and out_u8.is_contiguous() and tuple(out_u8.shape) == (H, W, 3)):
        raise TypeError(f"{name}: out_u8 must be a contiguous uint8 [H,W,3] tensor on the image's device")
    if accumulate is not None and accumulate.sums.device != x.device:
        raise TypeError(f"{name}: the accumulator lives on another device")
    view = torch.empty(_lib.EVAL_VIEW_FLOATS, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.gsr_eval_workspace_bytes(3, H, W, flags), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(lib.gsr_eval_image(x.data_ptr(), g.data_ptr(), 3, H, W, flags, view.data_ptr(),
                                      accumulate.sums.data_ptr() if accumulate is not None else None,
                                      out_u8.data_ptr() if out_u8 is not None else None, ws.data_ptr(), stream),
                   "gsr_eval_image")
    if accumulate is not None:
        accumulate._note(bool(flags & _lib.EVAL_SSIM))
    return view


@torch.no_grad()
def psnr(img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
    """Drop-in for ``utils.image_utils.psnr``: ``[B,1]`` with ``B = img1.shape[0]`` -- one value per channel of a
    ``[3,H,W]`` image (``train.py:229``), one per image of a ``[B,3,H,W]`` batch (``metrics.py:76``)."""
    _need_gpu("psnr", img1, img2)
    if img1.dim() == 3:
        return _eval("psnr", img1, img2, 0)[9:12].reshape(3, 1)
    if img1.dim() != 4 or img1.shape != img2.shape:
        raise TypeError(f"psnr expects two [3,H,W] or [B,3,H,W] tensors of one shape, got {tuple(img1.shape)}, {tuple(img2.shape)}")
    return torch.stack([_eval("psnr", a, b, _lib.EVAL_PSNR_WHOLE)[1] for a, b in zip(img1, img2)]).reshape(-1, 1)


@torch.no_grad()
def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """The value of ``utils.loss_utils.ssim`` as ``metrics.py:75`` calls it (window 11, mean over the image), 0-dim.
    A metric only: for a differentiable SSIM term use ``l1_dssim_loss``."""
    if window_size != 11 or not size_average:
        raise ValueError("ssim supports window_size=11, size_average=True only")
    if img1.requires_grad or img2.requires_grad:
        raise RuntimeError("ssim is a metric without a gradient; detach the inputs, or train with l1_dssim_loss")
    return _eval("ssim", img1, img2, _lib.EVAL_SSIM)[2]


@torch.no_grad()
def image_metrics(image: torch.Tensor, gt: torch.Tensor, *, clamp: bool = True, with_ssim: bool = False,
                  out_u8: Optional[torch.Tensor] = None, rounding: str = "nearest",
                  accumulate: Optional[EvalAccumulator] = None, clamp_gt: Optional[bool] = None,
                  whole_image_psnr: bool = False) -> dict:
    """One view of a report: {"l1", "psnr"[, "ssim"]} as 0-dim device tensors (never read back here), plus "record", the
    kernel's float32 record (l1, psnr, ssim, 3 x sum|d|, 3 x sum d^2, 3 x per-channel PSNR).
    clamp / clamp_gt: clamp the image / the ground truth (default: like the image) to [0, 1] on load, as
    ``train.py:222-223``.  psnr is the mean of the per-channel values (``train.py:229``) unless ``whole_image_psnr``
    (``metrics.py:76``).  out_u8: a uint8 [H,W,3] tensor that receives the 8-bit image of ``image`` in the same pass.
    accumulate: an ``EvalAccumulator`` that receives the view on the device."""
    flags = _rounding_flag(rounding)
    flags |= _lib.EVAL_CLAMP_X if clamp else 0
    flags |= _lib.EVAL_CLAMP_GT if (clamp if clamp_gt is None else clamp_gt) else 0
    flags |= _lib.EVAL_SSIM if with_ssim else 0
    flags |= _lib.EVAL_PSNR_WHOLE if whole_image_psnr else 0
    rec = _eval("image_metrics", image, gt, flags, out_u8, accumulate)
    out = {"l1": rec[0], "psnr": rec[1], "record": rec}
    if with_ssim:
        out["ssim"] = rec[2]
    return out


@torch.no_grad()
def to_uint8_hwc(image: torch.Tensor, rounding: str = "nearest") -> torch.Tensor:
    """[3,H,W] float -> [H,W,3] uint8 on the device.  "nearest": ``(clamp(x,0,1) * 255 + 0.5)`` truncated (torchvision's
    ``save_image``); "truncate": ``(clamp(x,0,1) * 255)`` truncated (``train.py:63``).  Bit-identical to torch."""
    flags = _rounding_flag(rounding)
    _need_gpu("to_uint8_hwc", image)
    x = _image3("to_uint8_hwc", image)
    _, H, W = (int(v) for v in x.shape)
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=x.device)
    lib = _lib.load()
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(lib.gsr_image_to_u8(x.data_ptr(), 3, H, W, flags, out.data_ptr(), stream), "gsr_image_to_u8")
    return out


@torch.no_grad()
def evaluate_views(cameras, model, pipe, bg, *, gt_images=None, with_ssim: bool = False, renderer=None,
                   **render_kwargs) -> dict:
    """``training_report``'s loop over one camera set (``train.py:217-235``): render every view, clamp render and ground
    truth to [0, 1], accumulate L1 and PSNR (and SSIM) on the device; one read-back at the end.
    gt_images: one [3,H,W] tensor per camera (default ``cam.original_image``).  renderer: a ``GraphedRenderer`` (its
    ``render(cam)`` is used) or a callable ``cam -> image or render package``; default the drop-in ``render``."""
    cameras = list(cameras)
    if gt_images is not None and len(gt_images) != len(cameras):
        raise ValueError("gt_images must hold one image per camera")
    if not bg.is_cuda:
        raise _lib.GsrError("evaluate_views needs ROCm GPU tensors (no CPU path)")
    if renderer is None:
        from .renderer import render as _render

        def frame(cam):
            return _render(cam, model, pipe, bg, **render_kwargs)
    elif hasattr(renderer, "render"):
        frame = renderer.render
    else:
        frame = renderer
    acc = EvalAccumulator(bg.device)
    for i, cam in enumerate(cameras):
        out = frame(cam)
        image = out["render"] if isinstance(out, dict) else out
        gt = gt_images[i] if gt_images is not None else cam.original_image
        image_metrics(image, gt.to(image.device), clamp=True, with_ssim=with_ssim, accumulate=acc)
    return acc.result()
