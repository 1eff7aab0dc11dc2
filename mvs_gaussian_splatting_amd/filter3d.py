"""Mip-Splatting's 3D smoothing filter on the HIP path (``csrc/filter3d.hip``, ``csrc/filter3d_math.h``).

A model trained at one sampling rate and viewed closer, or at a higher resolution, shows needle and erosion artefacts;
the 3D smoothing filter band-limits every Gaussian to the highest rate at which a training camera sampled it.  It is a
per-Gaussian scalar ``filter [P]``, computed from the training cameras and folded into the scales and opacities before the
rasterizer sees them; ``preprocess`` and the compositing kernels are untouched (the 2D Mip filter is not part of it).

**Sampling pass** (``compute_3d_filter``).  For every Gaussian ``p`` and training view ``v``: ``(x, y, z) = xyz_p through
world_view_transform_v`` (row-vector convention); the view counts when ``z > near`` and the pixel ``u = x / z * fx + W / 2,
w = y / z * fy + H / 2`` lies in ``[-m W, (1 + m) W] x [-m H, (1 + m) H]``, inclusive.  Kept per Gaussian: ``min_depth =
min z`` and ``max_rate = max fx / z`` over the counting views, and ``seen``.

**Width.**  ``rule="mip_splatting"`` (the published code): ``filter = min_depth / max_v fx_v * sqrt(variance)``, the focal
maximum over ALL views.  ``rule="paper"`` (the paper's sampling-rate formula): ``filter = sqrt(variance) / max_rate``.  An
unseen Gaussian takes the largest ``min_depth`` (the smallest ``max_rate``) of the seen ones.  When no Gaussian is seen the
filter is 0 everywhere and the returned device flag is 1.  Nothing is read back.

**Application** (``apply_3d_filter``).  With ``a_i = exp(2 s_i)``: the filtered scale is ``sqrt(a_i + f^2)`` and the
filtered opacity ``sigmoid(o) c``, ``c = sqrt(prod a_i / prod (a_i + f^2))``.  The op emits EFFECTIVE RAW parameters ``s'_i
= s_i + log1p(f^2 exp(-2 s_i)) / 2`` and ``o' = logit(sigmoid(o) c)``, so that the rasterizer's own ``exp`` and ``sigmoid``
produce the filtered values and ``render``'s raw-parameter fast path stays in use.  Forward and backward are one launch
each, float64 inside the lane, rounded once; ``f = 0`` returns ``s`` and ``o`` bit for bit.  The filter has no gradient.

There is no CPU path: the functions check their arguments on the host, then raise ``GsrError`` on CPU tensors.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from . import _lib

RULES = {"mip_splatting": _lib.FILTER3D_MIP_SPLATTING, "paper": _lib.FILTER3D_PAPER}
MAX_VIEWS = _lib.FILTER3D_MAX_VIEWS
VIEW_CHUNK = MAX_VIEWS          # views per launch; a longer table is fed in chunks that accumulate (same result)


def _positive(name: str, v, zero_ok: bool = False) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or (v == 0 and not zero_ok):
        raise ValueError(f"{name} must be a finite {'non-negative' if zero_ok else 'positive'} float, got {v!r}")
    return float(v)


def view_table(cameras):
    """The cameras, checked on the host -> ``(rows, focal_max)``: a ctypes array of ``_lib.GsrFilterView`` and the largest
    ``fx`` of the table as the float32 the rows hold."""
    try:
        cameras = list(cameras)
    except TypeError:
        raise ValueError(f"cameras must be a sequence of cameras, got {type(cameras)}") from None
    if not cameras:
        raise ValueError("compute_3d_filter needs at least one camera")
    from .mvs import _focal
    rows = (_lib.GsrFilterView * len(cameras))()
    for k, cam in enumerate(cameras):
        H, W, fx, fy = _focal(cam)
        if max(H, W) > 2 ** 24:
            raise ValueError(f"camera {k}: an image of {W} x {H} exceeds 2^24 a side")
        M = cam.world_view_transform.detach().to(device="cpu", dtype=torch.float32)
        if tuple(M.shape) != (4, 4):
            raise ValueError(f"camera {k}: world_view_transform must be 4 x 4, got {tuple(M.shape)}")
        if not (bool(torch.isfinite(M).all()) and math.isfinite(fx) and math.isfinite(fy) and fx > 0 and fy > 0):
            raise ValueError(f"camera {k}: world_view_transform and the focal lengths must be finite")
        row = rows[k]
        row.width, row.height, row.fx, row.fy = W, H, fx, fy
        row.world_to_view[:] = M.reshape(-1).tolist()
    return rows, max(float(r.fx) for r in rows)


def compute_3d_filter(xyz: torch.Tensor, cameras, *, near: float = 0.2, margin: float = 0.15, variance: float = 0.2,
                      rule: str = "mip_splatting", out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``xyz`` float32 ``[P,3]`` on a ROCm GPU and the training cameras (``world_view_transform``, ``FoVx``, ``FoVy``,
    ``image_width``, ``image_height``) -> ``(filter float32 [P], none_seen int32 [1])``, both on the device (module
    docstring).  ``out``: a contiguous float32 ``[P]`` tensor on the same device to write the filter into.  The view table
    is one small host-to-device copy per 65535 views; nothing is read back, everything runs on the current stream."""
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must be a float32 [P, 3] tensor, got {getattr(xyz, 'dtype', type(xyz))} "
                         f"{tuple(getattr(xyz, 'shape', ()))}")
    near, margin = _positive("near", near), _positive("margin", margin, zero_ok=True)
    variance = _positive("variance", variance)
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)}, got {rule!r}")
    rows, focal_max = view_table(cameras)
    P, dev = int(xyz.shape[0]), xyz.device
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (P,)
                            or out.device != dev or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 [{P}] tensor on {dev}")
    if not xyz.is_cuda:
        raise _lib.GsrError("compute_3d_filter needs ROCm GPU tensors (no CPU path)")
    lib = _lib.load()
    xyz_c = xyz.detach().contiguous()
    filt = torch.empty(P, dtype=torch.float32, device=dev) if out is None else out
    none_seen = torch.empty(1, dtype=torch.int32, device=dev)
    min_depth = torch.empty(P, dtype=torch.float32, device=dev)
    max_rate = torch.empty(P, dtype=torch.float32, device=dev)
    seen = torch.empty(P, dtype=torch.uint8, device=dev)
    ws_bytes = int(lib.gsr_filter3d_workspace_bytes(P))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    raw = bytes(rows)
    row_bytes = len(raw) // len(rows)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        for first in range(0, len(rows), VIEW_CHUNK):
            n = min(VIEW_CHUNK, len(rows) - first)
            table = torch.frombuffer(bytearray(raw[first * row_bytes:(first + n) * row_bytes]), dtype=torch.uint8).to(dev)
            _lib.check(lib.gsr_filter3d_sample(xyz_c.data_ptr(), P, table.data_ptr(), n, near, margin, int(first > 0),
                                               min_depth.data_ptr(), max_rate.data_ptr(), seen.data_ptr(), ws.data_ptr(),
                                               ws_bytes, stream), "gsr_filter3d_sample")
        _lib.check(lib.gsr_filter3d_finish(P, min_depth.data_ptr(), max_rate.data_ptr(), seen.data_ptr(), RULES[rule],
                                           focal_max, variance, ws.data_ptr(), ws_bytes, filt.data_ptr(),
                                           none_seen.data_ptr(), stream), "gsr_filter3d_finish")
    return filt, none_seen


def _check_apply(scaling_raw, opacity_raw, filter) -> int:
    for name, t in (("scaling_raw", scaling_raw), ("opacity_raw", opacity_raw), ("filter", filter)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor, got {getattr(t, 'dtype', type(t))}")
    if scaling_raw.dim() != 2 or scaling_raw.shape[1] != 3:
        raise ValueError(f"scaling_raw must be [P, 3], got {tuple(scaling_raw.shape)}")
    P = int(scaling_raw.shape[0])
    if tuple(opacity_raw.shape) not in ((P, 1), (P,)):
        raise ValueError(f"opacity_raw must be [{P}, 1] or [{P}], got {tuple(opacity_raw.shape)}")
    if tuple(filter.shape) not in ((P,), (P, 1)):
        raise ValueError(f"filter must be [{P}] (one value per Gaussian; compute_3D_filter makes it), got "
                         f"{tuple(filter.shape)}")
    if not (scaling_raw.device == opacity_raw.device == filter.device):
        raise ValueError("scaling_raw, opacity_raw and filter must live on one device")
    if filter.requires_grad:
        raise ValueError("the 3D filter carries no gradient: pass filter.detach()")
    if not scaling_raw.is_cuda:
        raise _lib.GsrError("apply_3d_filter needs ROCm GPU tensors (no CPU path)")
    return P


class _Apply3DFilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling_raw, opacity_raw, filter):
        P = int(scaling_raw.shape[0])
        s, o, f = scaling_raw.detach().contiguous(), opacity_raw.detach().contiguous(), filter.contiguous()
        s_out, o_out = torch.empty_like(s), torch.empty_like(o)
        with torch.cuda.device(s.device):
            stream = torch.cuda.current_stream(s.device).cuda_stream
            _lib.check(_lib.load().gsr_filter3d_apply(s.data_ptr(), o.data_ptr(), f.data_ptr(), P, s_out.data_ptr(),
                                                      o_out.data_ptr(), stream), "gsr_filter3d_apply")
        ctx.save_for_backward(s, o, f)
        ctx.mark_non_differentiable(filter)
        return s_out, o_out

    @staticmethod
    def backward(ctx, g_s, g_o):
        s, o, f = ctx.saved_tensors
        P = int(s.shape[0])
        g_s = torch.zeros_like(s) if g_s is None else g_s.contiguous()
        g_o = torch.zeros_like(o) if g_o is None else g_o.contiguous()
        d_s, d_o = torch.empty_like(s), torch.empty_like(o)
        with torch.cuda.device(s.device):
            stream = torch.cuda.current_stream(s.device).cuda_stream
            _lib.check(_lib.load().gsr_filter3d_apply_bwd(s.data_ptr(), o.data_ptr(), f.data_ptr(), P, g_s.data_ptr(),
                                                          g_o.data_ptr(), d_s.data_ptr(), d_o.data_ptr(), stream),
                       "gsr_filter3d_apply_bwd")
        return d_s, d_o, None


def apply_3d_filter(scaling_raw: torch.Tensor, opacity_raw: torch.Tensor, filter: torch.Tensor):
    """Raw scales ``[P,3]``, raw opacities ``[P,1]`` (or ``[P]``) and ``filter [P]`` -> the effective raw tensors
    ``(scaling', opacity')`` of the same shapes, differentiable in the first two (module docstring).  Hand them to the
    rasterizer where ``_scaling`` and ``_opacity`` went: ``exp(scaling')`` and ``sigmoid(opacity')`` are the filtered
    values."""
    _check_apply(scaling_raw, opacity_raw, filter)
    return _Apply3DFilter.apply(scaling_raw, opacity_raw, filter)


def filtered_scaling_opacity(scaling_raw: torch.Tensor, opacity_raw: torch.Tensor, filter: torch.Tensor):
    """The ACTIVATED filtered values ``(sqrt(exp(2 s) + f^2) [P,3], sigmoid(o) c)``, for the getter path: the activations
    of ``apply_3d_filter``'s result, so both paths hand the rasterizer the same numbers."""
    s, o = apply_3d_filter(scaling_raw, opacity_raw, filter)
    return torch.exp(s), torch.sigmoid(o)


def checked_filter_3D(pc, what: str = "render"):
    """The 3D filter of a duck-typed model: ``pc.filter_3D``, or None when it has none.  ``ValueError`` -- host code,
    before a GPU is asked for -- for a filter marked stale or without one value per Gaussian."""
    f = getattr(pc, "filter_3D", None)
    if f is None:
        return None
    P = int(pc._xyz.shape[0])
    if getattr(pc, "_filter_3D_stale", False):
        raise ValueError(f"{what}: the model's 3D filter is stale -- rows were removed, added or reordered since it was "
                         f"computed; call compute_3D_filter(cameras) again (or set filter_3D = None)")
    if not isinstance(f, torch.Tensor) or f.dtype != torch.float32 or tuple(f.shape) != (P,):
        raise ValueError(f"{what}: the model's 3D filter must be a float32 [{P}] tensor, one value per Gaussian, got "
                         f"{getattr(f, 'dtype', type(f))} {tuple(getattr(f, 'shape', ()))}; call compute_3D_filter(cameras) again")
    return f


__all__ = ["compute_3d_filter", "apply_3d_filter", "filtered_scaling_opacity"]
