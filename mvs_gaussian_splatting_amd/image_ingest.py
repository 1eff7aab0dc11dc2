"""Load-time image ingest on the GPU (``csrc/image.hip``): what the reference does on the host for every image between
the file decode and the float target the loss reads.

    target = load_image(array_u8_hwc, (width, height), "cuda", composite_bg=None)       # [3, H, W] float32

chains, on the device and on the current stream,

a. ``composite_u8``: the Blender reader's alpha composite (``scene/dataset_readers.py:204-210``) in float64.  The
   reference casts ``arr * 255.0`` to ``np.byte`` and hands that int8 array to ``Image.fromarray(..., "RGB")``; current
   Pillow rejects an int8 array with a ``TypeError``, the versions that accepted it took its bytes as they were.  The
   defined result is therefore *the bytes of that int8 array read as uint8*: truncation toward zero, low eight bits.
b. ``resize_u8``: Pillow's ``Image.resize(size)`` with its default bicubic filter for 8-bit images, bit for bit
   (``utils/general_utils.py:22``).  The host builds Pillow's integer tap tables (``resize_tables``), the device runs a
   horizontal and a vertical integer pass.
c. ``to_float_chw``: ``uint8 / 255.0`` as float32, clamped to [0, 1], times the alpha channel ``/ 255.0`` when the image
   has one, as a ``[3, H, W]`` tensor (``PILtoTorch``, ``loadCam``, ``Camera.__init__``).

An RGBA image that is *not* composited and needs resizing goes through Pillow's premultiplied ``RGBa`` resize, which is
not restated here: ``load_image`` resizes such an image on the host with Pillow and runs only (c) on the GPU.

``load_image_host`` is the reference's host-only chain (numpy composite, Pillow resize, torch convert), kept as the
comparison for the tests and for ``tools/bench_ingest.py``.  Pillow is imported only where the host chain needs it.
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 32 - 8 - 2       # Pillow's fixed-point position for 8-bit channels
_BICUBIC_SUPPORT = 2.0
_BICUBIC_A = -0.5


# ---- Pillow's tap tables (src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc) ------------------------
def _bicubic(x: np.ndarray) -> np.ndarray:
    a = _BICUBIC_A
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resize_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """The table of one pass of Pillow's 8-bit bicubic resize from ``in_size`` to ``out_size`` pixels:
    ``bounds`` int32 ``[out_size, 2]`` (first input index, tap count) and ``taps`` int32 ``[out_size, ksize]``
    (fixed point, ``PRECISION_BITS`` fractional bits, zero beyond the count).  Float64 throughout, in Pillow's order of
    operations: the weights are summed one after the other and each is divided by that sum."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"resize_tables: sizes must be positive, got {in_size} -> {out_size}")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = _BICUBIC_SUPPORT * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)          # C's (int): toward zero
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < count[:, None]
    w = np.where(live, _bicubic(((x + xmin[:, None]) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                   # a running sum, as the C loop adds them (not numpy's pairwise sum)
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    fixed = w * float(1 << PRECISION_BITS)
    taps = np.trunc(np.where(w < 0, -0.5 + fixed, 0.5 + fixed)).astype(np.int32)
    taps[~live] = 0
    return np.stack([xmin, count], axis=1).astype(np.int32), taps


@functools.lru_cache(maxsize=64)
def _device_tables(in_size: int, out_size: int, device: torch.device):
    bounds, taps = resize_tables(in_size, out_size)
    return torch.from_numpy(bounds).to(device), torch.from_numpy(taps).to(device), int(taps.shape[1])


# ---- the three kernels ---------------------------------------------------------------------------------------------
def _need_u8_hwc(name: str, image: torch.Tensor, channels: Sequence[int]) -> torch.Tensor:
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8:
        raise TypeError(f"{name}: expected a uint8 tensor")
    if not image.is_cuda:
        raise _lib.GsrError(f"{name} needs a tensor on a ROCm GPU (no CPU path)")
    if image.dim() != 3 or image.shape[2] not in channels or image.shape[0] == 0 or image.shape[1] == 0:
        raise ValueError(f"{name}: expected [H, W, C] with C in {tuple(channels)}, got {tuple(image.shape)}")
    return image.contiguous()


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _bg3(bg) -> Tuple[float, float, float]:
    vals = [float(v) for v in np.asarray(bg, dtype=np.float64).reshape(-1)]
    if len(vals) != 3:
        raise ValueError("composite background needs three values")
    return vals[0], vals[1], vals[2]


@torch.no_grad()
def composite_u8(rgba: torch.Tensor, bg) -> torch.Tensor:
    """(a): ``[H, W, 4]`` uint8 over the background ``bg`` (three values in [0, 1]) -> ``[H, W, 3]`` uint8."""
    x = _need_u8_hwc("composite_u8", rgba, (4,))
    H, W = int(x.shape[0]), int(x.shape[1])
    out = torch.empty(H, W, 3, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().gsr_image_composite_u8(x.data_ptr(), H, W, *_bg3(bg), out.data_ptr(), _stream(x)),
                   "gsr_image_composite_u8")
    return out


@torch.no_grad()
def resize_u8(image: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """(b): ``[H, W, C]`` uint8 with C = 1 or 3 -> ``[size[1], size[0], C]``; ``size`` is Pillow's (width, height)."""
    x = _need_u8_hwc("resize_u8", image, (1, 3))
    H, W, C = (int(v) for v in x.shape)
    out_w, out_h = int(size[0]), int(size[1])
    if out_w <= 0 or out_h <= 0:
        raise ValueError(f"resize_u8: bad size {size}")
    dev = x.device
    hb = ht = vb = vt = None
    hk = vk = 0
    if out_w != W:
        hb, ht, hk = _device_tables(W, out_w, dev)
    if out_h != H:
        vb, vt, vk = _device_tables(H, out_h, dev)
    tmp = torch.empty(H, out_w, C, dtype=torch.uint8, device=dev) if (hb is not None and vb is not None) else None
    out = torch.empty(out_h, out_w, C, dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsr_image_resize_u8(x.data_ptr(), C, H, W, out_h, out_w, ptr(hb), ptr(ht), hk, ptr(vb),
                                                   ptr(vt), vk, ptr(tmp), out.data_ptr(), _stream(x)),
                   "gsr_image_resize_u8")
    return out


@torch.no_grad()
def to_float_chw(image: torch.Tensor) -> torch.Tensor:
    """(c): ``[H, W, 3 or 4]`` uint8 -> ``[3, H, W]`` float32 in [0, 1], multiplied by the alpha channel if there is one."""
    x = _need_u8_hwc("to_float_chw", image, (3, 4))
    H, W, C = (int(v) for v in x.shape)
    out = torch.empty(3, H, W, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().gsr_image_to_float_chw(x.data_ptr(), C, H, W, out.data_ptr(), _stream(x)),
                   "gsr_image_to_float_chw")
    return out


# ---- the chains ----------------------------------------------------------------------------------------------------
def _as_u8_hwc(name: str, array) -> np.ndarray:
    a = array.cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if a.dtype != np.uint8:
        raise TypeError(f"{name}: expected uint8 data, got {a.dtype}")
    if a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1):
        raise ValueError(f"{name}: single-channel images are not supported (the loss needs a 3-channel target)")
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{name}: expected [H, W, 3 or 4], got {a.shape}")
    return np.ascontiguousarray(a)


def _pil_resize(a: np.ndarray, size: Tuple[int, int]) -> np.ndarray:
    from PIL import Image                                       # lazy: the package imports without Pillow
    return np.array(Image.fromarray(a).resize((int(size[0]), int(size[1]))))


@torch.no_grad()
def load_image(array, size: Tuple[int, int], device="cuda", composite_bg=None) -> torch.Tensor:
    """Decoded image -> training target.  array: ``[H, W, 3 or 4]`` uint8 (numpy, or a tensor on any device);
    size: the (width, height) to resize to; composite_bg: three values in [0, 1] to composite an RGBA image over first
    (the Blender reader), None to keep the image as it is.  Returns ``[3, size[1], size[0]]`` float32 on ``device``."""
    device = torch.device(device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise _lib.GsrError("load_image needs a ROCm GPU (no CPU path); load_image_host is the host chain")
    if isinstance(array, torch.Tensor) and array.is_cuda:
        if array.dtype != torch.uint8 or array.dim() != 3 or array.shape[2] not in (3, 4):
            raise ValueError(f"load_image: expected [H, W, 3 or 4] uint8, got {tuple(array.shape)} {array.dtype}")
        x = array.to(device).contiguous()
    else:
        a = _as_u8_hwc("load_image", array)
        if composite_bg is None and a.shape[2] == 4 and (a.shape[1], a.shape[0]) != (int(size[0]), int(size[1])):
            a = _pil_resize(a, size)                            # Pillow's premultiplied RGBa path stays on the host
        x = torch.from_numpy(a).to(device)
    H, W, C = (int(v) for v in x.shape)
    if composite_bg is not None:
        if C != 4:
            raise ValueError("load_image: compositing needs an RGBA image")
        x = composite_u8(x, composite_bg)
        C = 3
    if (W, H) != (int(size[0]), int(size[1])):
        if C == 4:
            x = torch.from_numpy(_pil_resize(x.cpu().numpy(), size)).to(device)
        else:
            x = resize_u8(x, size)
    return to_float_chw(x)


def composite_host(rgba: np.ndarray, bg) -> np.ndarray:
    """``scene/dataset_readers.py:204-210`` in numpy; the int8 array's bytes read as uint8 (see the module text)."""
    bg = np.asarray(bg).reshape(3)
    norm_data = rgba / 255.0
    arr = norm_data[:, :, :3] * norm_data[:, :, 3:4] + bg * (1 - norm_data[:, :, 3:4])
    return np.array(arr * 255.0, dtype=np.byte).view(np.uint8)


def to_float_host(a: np.ndarray) -> torch.Tensor:
    """``PILtoTorch`` after the resize, ``loadCam``'s channel split and ``Camera.__init__``'s clamp and mask, on the CPU."""
    t = (torch.from_numpy(a) / 255.0).permute(2, 0, 1)
    image = t[:3, ...].clamp(0.0, 1.0)
    if t.shape[0] == 4:
        image *= t[3:4, ...]
    else:
        image *= torch.ones((1, image.shape[1], image.shape[2]))
    return image.contiguous()


def load_image_host(array, size: Tuple[int, int], composite_bg=None) -> torch.Tensor:
    """The reference's host-only chain for the same arguments as ``load_image``; a CPU tensor.  Needs Pillow."""
    a = _as_u8_hwc("load_image_host", array)
    if composite_bg is not None:
        if a.shape[2] != 4:
            raise ValueError("load_image_host: compositing needs an RGBA image")
        a = composite_host(a, composite_bg)
    return to_float_host(_pil_resize(a, size))


__all__ = ["resize_tables", "composite_u8", "resize_u8", "to_float_chw", "load_image", "load_image_host",
           "composite_host", "to_float_host", "PRECISION_BITS"]
