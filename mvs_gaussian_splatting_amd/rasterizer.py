"""Drop-in operator surface for the reference's ``diff_gaussian_rasterization`` import
(``gaussian_renderer/__init__.py:15``): ``GaussianRasterizationSettings`` (the 12 fields built at
``gaussian_renderer/__init__.py:42-55``) and ``GaussianRasterizer`` (constructed at ``:57``, called
with keyword arguments at ``:257-265``).  The arithmetic runs in ``libgsr_hip.so`` through the C ABI
of ``include/gsr.h``; PyTorch only owns the memory and the stream.

No CPU path exists: tensors must live on a ROCm device and the HIP library must be built.

Host synchronisation.  Only the first frame of a (device, P, W, H) combination reads its instance count back; later
frames are enqueued whole and verified before the operator returns (``_frames.py``, which holds that state machine).

``GSR_SYNC_FREE`` (read at import) / ``set_sync_free``:  ``1`` / ``True`` (default) the verified mode above;
``0`` / ``False`` every frame on the two-call path;  ``deferred`` the count is compared with the capacity at the
latest when the frame's backward starts, when the next frame is issued or in ``synchronize_counts()`` -- an overflowed
frame raises ``GsrError`` THERE (its image and gradients are incomplete).  Only for callers that can redo a frame.

Camera gradients.  ``GaussianRasterizationSettings`` stays the 12-field tuple.  When its ``viewmatrix``, ``projmatrix`` or
``campos`` requires grad (and grad mode is on) the three tensors also enter the autograd functions as inputs of their own
and receive gradients of their own shapes ([4,4], [4,4], [3]; entries the rasterizer does not read -- ``viewmatrix``
column 3, ``projmatrix`` column 2 -- are zero): ``scene.PoseCamera`` builds such tensors from a learnable pose.  A frame
whose camera does not require grad takes the path, the kernels and the allocations it always took.

Depth / alpha maps.  ``GaussianRasterizer(settings, aux_maps=True)`` returns ``(color, radii, aux)``: ``aux [3,H,W]`` holds
the depth (``sum w z``), inverse-depth (``sum w / z``) and accumulated-opacity (``sum w``) maps of the frame, from
kernels of their own (``csrc/depth.hip``) behind a second autograd node (``_AuxMaps``) that reads the colour node's frame.
Without ``aux_maps`` nothing of it runs.

Contribution statistics.  ``GaussianRasterizer(settings, contribution=stats)`` (``contribution.ContributionStats``; any
object with ``raw`` -- int64 ``[P,3]`` on the device -- and ``views``) adds the frame's per-Gaussian blending-weight
statistics into ``stats.raw`` after the colour forward (``csrc/contribution.hip``) and counts the view;
``contribution_mask`` (uint8 ``[H,W]``) leaves pixels out.  Nothing enters the autograd graph, and the call's results are
what they are without it.  Without ``contribution`` nothing of it runs.

Feature maps.  ``forward(..., features=F)`` with ``F`` float32 ``[P,C]`` (any C >= 1) appends ``feat [C,H,W]`` =
``sum w F[id]`` to the call's results (after ``aux`` when ``aux_maps=True``): the per-Gaussian rows composited with the
colour pass's blending weights, no background term, no clamp (``csrc/features.hip``), behind a third
autograd node (``_FeatureMaps``) that reads the colour node's frame and returns gradients for ``F`` and the geometry.
Without ``features`` nothing of it runs.

Distortion map.  ``GaussianRasterizer(settings, distortion=True)`` (or ``distortion=dict(mapping="linear" | "ndc", near=,
far=)``; ``True`` is ``"ndc"`` with near 0.2, far 100, what 2DGS trains with) appends ``dist [1,H,W]`` =
``sum_i sum_{j<i} w_i w_j (m_i - m_j)^2`` to the call's results (after ``aux`` and ``feat``): the depth-distortion term of
2DGS over the colour pass's contributors, evaluated without the cancelling ``A M2 - M1^2`` form (``csrc/distortion.hip``;
DESIGN.md §7.16), behind a node of its own (``_DistortionMap``) that reads the colour node's frame.  Without ``distortion``
nothing of it runs.

Median depth.  ``GaussianRasterizer(settings, median_depth=True)`` appends two tensors to the call's results, after ``aux``,
``feat`` and ``dist``: ``median [1,H,W]``, the view depth of the last composited entry in front of which the colour pass's
transmittance still exceeds one half (2DGS's median depth; 0 where nothing was composited), and ``median_id [H,W]`` (int32),
the row of that entry's Gaussian (-1 where nothing was composited) (``csrc/median.hip``), behind a node of
its own (``_MedianDepth``) that reads the colour node's frame.  Only means3D receives a gradient.  Without ``median_depth``
nothing of it runs.

Absolute gradient.  ``GaussianRasterizer(settings, abs_grad=True)`` takes a second dummy ``means2D_abs [P,3]`` in its
call: after ``backward`` its ``.grad`` holds AbsGS's absolute ("homodirectional") view-space gradient of the COLOUR image,
``sum over the Gaussian's pixels of |d L / d mean2D|`` per component in ``means2D.grad``'s scale, z = 0 (``csrc/abs_grad.hip``;
DESIGN.md §7.27).  A node of its own (``_AbsGrad``) that passes the colour image and its incoming gradient through
untouched and reads the colour node's frame: colour, radii and every other gradient are what they are without it.  The
gradient of the map nodes above takes no part in it.  Without ``abs_grad`` nothing of it runs.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _frames, _lib
from ._frames import (_DEPTH_SPAN_TRUSTED, _Frame, _counts_pinned_thread, _grown_key, _ptr, _round_ws,  # noqa: F401
                      _run_backward, _run_forward, _states, _stream, _verify, synchronize_counts)


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _f32c(t: torch.Tensor, name: str, dev: torch.device, align16: bool = False) -> torch.Tensor:
    if t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    t = t.contiguous()
    if align16 and t.data_ptr() % 16 != 0:
        t = t.clone()
    return t


def _check_rows(t: torch.Tensor, name: str, P: int, *tail) -> None:
    """The kernels index raw pointers: a non-empty input must be [P, *tail] (tail entry None = any size >= 1)."""
    if t.numel() == 0:
        return
    ok = t.dim() == 1 + len(tail) and t.shape[0] == P and all(
        (d is None and int(s) >= 1) or (d is not None and int(s) == d) for s, d in zip(t.shape[1:], tail))
    if not ok:
        want = ", ".join("M" if d is None else str(d) for d in tail)
        raise ValueError(f"{name} must have shape [P={P}, {want}], got {list(t.shape)}")


def _require_gpu(t: torch.Tensor) -> torch.device:
    if not t.is_cuda:
        raise _lib.GsrError("GaussianRasterizer needs tensors on a ROCm GPU: this build has no CPU path "
                            f"(means3D is on {t.device})")
    return t.device


# ---- process-wide switches: read from the environment ONCE, at import; changed afterwards only through the setters ----
_BINNING = {"keys64": _lib.BINNING_KEYS64, "two_level": _lib.BINNING_TWO_LEVEL, "culled": _lib.BINNING_TWO_LEVEL_CULLED}


def _binning_from_name(name: str) -> int:
    name = name.lower()
    if name not in _BINNING:
        raise ValueError(f"binning mode must be one of {sorted(_BINNING)}, got {name!r}")
    return _BINNING[name]


_binning_mode_value = _binning_from_name(os.environ.get("GSR_BINNING", "culled"))
_debug_flags_value = 0
SYNC_OFF, SYNC_VERIFIED, SYNC_DEFERRED = 0, 1, 2


def _sync_mode_from(value) -> int:
    if isinstance(value, str):
        v = value.strip().lower()
        if v in ("0", "off", "false", "no"):
            return SYNC_OFF
        if v in ("1", "on", "true", "yes", "verified", ""):
            return SYNC_VERIFIED
        if v in ("2", "deferred"):
            return SYNC_DEFERRED
        raise ValueError(f"sync-free mode must be 0 / 1 / deferred, got {value!r}")
    if value is True or value is False:
        return SYNC_VERIFIED if value else SYNC_OFF
    if value in (SYNC_OFF, SYNC_VERIFIED, SYNC_DEFERRED):
        return int(value)
    raise ValueError(f"sync-free mode must be a bool, 0 / 1 / 2 or a name, got {value!r}")


_sync_free_value = _sync_mode_from(os.environ.get("GSR_SYNC_FREE", "1"))


def set_binning_mode(name: str) -> str:
    """culled (default: two_level minus the instances whose tile the alpha >= 1/255 ellipse cannot reach; colour, radii
    and gradients are bit-identical to the other modes) | two_level (upstream's lists via two 32-bit sorts) | keys64
    (upstream's 64-bit (tile, depth) key sort).  Initial value: GSR_BINNING at import.  Returns the previous name."""
    global _binning_mode_value
    prev = next(k for k, v in _BINNING.items() if v == _binning_mode_value)
    _binning_mode_value = _binning_from_name(name)
    return prev


def set_debug_flags(flags: int) -> int:
    """GsrParams.debug_flags for the calls that follow (``_lib.DEBUG_*``); returns the previous value."""
    global _debug_flags_value
    prev, _debug_flags_value = _debug_flags_value, int(flags)
    return prev


def set_sync_free(mode) -> int:
    """How frames after the first of a shape are issued (module docstring): False / 0 = two calls with the count
    read-back between them; True / 1 = enqueued whole, verified before the operator returns (default);
    "deferred" / 2 = enqueued whole, verified later (an overflowed frame raises GsrError).  Returns the previous
    setting (SYNC_OFF / SYNC_VERIFIED / SYNC_DEFERRED; pass it back to restore)."""
    global _sync_free_value
    prev, _sync_free_value = _sync_free_value, _sync_mode_from(mode)
    return prev


def sync_free_mode() -> int:
    return _sync_free_value


def _make_params(dev, settings: GaussianRasterizationSettings, means3D, sh, colors_precomp, opacities, scales,
                 rotations, cov3Ds_precomp, sh_rest=None, act_flags: int = 0, forward_only: bool = False):
    """Returns (GsrParams, keepalive list).  ``counts_pinned`` is left NULL: the forward paths below attach theirs."""
    bg = _f32c(settings.bg, "bg", dev)
    view = _f32c(settings.viewmatrix, "viewmatrix", dev)
    proj = _f32c(settings.projmatrix, "projmatrix", dev)
    campos = _f32c(settings.campos, "campos", dev)
    if bg.numel() != 3 or view.numel() != 16 or proj.numel() != 16 or campos.numel() != 3:
        raise ValueError("bg/campos must have 3 elements and viewmatrix/projmatrix 16")
    P = int(means3D.shape[0])
    M = int(sh.shape[1]) if sh.numel() else 0
    if sh_rest is not None:
        M = 1 + int(sh_rest.shape[1])
    p = _lib.GsrParams()
    p.P, p.M, p.D = P, M, int(settings.sh_degree)
    p.width, p.height = int(settings.image_width), int(settings.image_height)
    p.tan_fovx, p.tan_fovy = float(settings.tanfovx), float(settings.tanfovy)
    p.scale_modifier = float(settings.scale_modifier)
    p.prefiltered, p.debug = int(bool(settings.prefiltered)), int(bool(settings.debug))
    p.means3D, p.shs, p.colors_precomp = _ptr(means3D), _ptr(sh), _ptr(colors_precomp)
    p.opacities, p.scales, p.rotations = _ptr(opacities), _ptr(scales), _ptr(rotations)
    p.cov3D_precomp = _ptr(cov3Ds_precomp)
    p.viewmatrix, p.projmatrix, p.campos, p.bg = view.data_ptr(), proj.data_ptr(), campos.data_ptr(), bg.data_ptr()
    p.profile = _lib.active_profile_handle()      # raw handle; the owning object travels in ctx.profile
    p.shs_rest = _ptr(sh_rest)
    p.act_flags = int(act_flags)
    p.binning_mode = _binning_mode_value
    p.counts_pinned = None
    p.forward_only = int(bool(forward_only))
    p.debug_flags = _debug_flags_value
    p.visible_out = None
    p.depth_span_lt24 = 0
    return p, [bg, view, proj, campos]


def last_counts(dev, P: int, W: int, H: int, grown: bool = False) -> tuple:
    """(num_rendered, num_visible) of the most recent checked frame of that shape on ``dev`` ((0, 0) if none).
    ``grown``: of the frames of a P-Gaussian model with grown / split rows appended."""
    return _frames._counts_of(dev, P, W, H, grown, _binning_mode_value)[0]


def reissued_frames(dev, P: int, W: int, H: int, grown: bool = False) -> int:
    """Frames of that shape that were issued a second time (verified mode): they did not fit their capacity, or spanned
    2^24 depth-key steps after being issued without the depth sort's fourth pass.  ``grown``: as in last_counts."""
    return _frames._counts_of(dev, P, W, H, grown, _binning_mode_value)[1]


def frame_counts(color: torch.Tensor) -> tuple:
    """(num_rendered, num_visible) of the frame that produced ``color`` (an output of the operator that still carries
    its autograd node).  In deferred mode: waits for the frame's count; raises if it overflowed."""
    ctx = color.grad_fn
    if ctx is None or not hasattr(ctx, "frame_pending"):
        raise ValueError("not an output of the rasterizer with an autograd node (rendered under no_grad?)")
    pend = ctx.frame_pending
    if pend is not None:
        _verify(pend, block=True)
        return pend.counts
    return ctx.counts


def _stats_ptrs(stats, P: int, dev):
    """(accum, denom, max_radii2D) pointers of the fused densification statistics, or three Nones."""
    if stats is None:
        return None, None, None
    out = []
    for t in stats:
        if not (t.is_cuda and t.device == dev and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == P):
            raise TypeError("densification accumulators must be contiguous float32 GPU tensors with one element per Gaussian")
        out.append(t.data_ptr())
    return tuple(out)


def _camera_inputs(settings: GaussianRasterizationSettings):
    """(viewmatrix, projmatrix, campos) when one of them requires grad and grad mode is on -- the autograd functions then
    take the three as inputs of their own -- else the empty tuple (the frame is issued exactly as without this feature)."""
    cam = (settings.viewmatrix, settings.projmatrix, settings.campos)
    if torch.is_grad_enabled() and any(t.requires_grad for t in cam):
        return cam
    return ()


def _camera_grads(lib, grads: "_lib.GsrGrads", cam_shapes, P: int, dev):
    """Attach the camera outputs and their workspace to ``grads``; returns (tensors to keep alive, the three gradients
    in the shapes of the inputs)."""
    g_view = torch.empty(16, dtype=torch.float32, device=dev)
    g_proj = torch.empty(16, dtype=torch.float32, device=dev)
    g_pos = torch.empty(3, dtype=torch.float32, device=dev)
    ws = torch.empty(lib.gsr_camera_grad_bytes(P), dtype=torch.uint8, device=dev)
    grads.dL_dviewmatrix, grads.dL_dprojmatrix, grads.dL_dcampos = g_view.data_ptr(), g_proj.data_ptr(), g_pos.data_ptr()
    grads.camera_ws = ws.data_ptr()
    return ws, tuple(g.view(shape) for g, shape in zip((g_view, g_proj, g_pos), cam_shapes))


def _colour_forward(fn, ctx, lib, dev, P, inputs, means2D, raster_settings, forward_only, stats, cam, act_flags=0,
                    visible=None, state_key=None):
    """The forward of both colour operators once ``fn`` (the operator's class) has checked its ``inputs``: the tensors it
    saves in front of the frame, the first of them means3D.  ``cam``: its three ``cam_*`` arguments."""
    H, W = int(raster_settings.image_height), int(raster_settings.image_width)
    with torch.cuda.device(dev):
        params, keep = _make_params(dev, raster_settings, *fn._params_args(inputs, dev), act_flags=act_flags,
                                    forward_only=forward_only)
        if visible is not None:
            if visible.dtype != torch.bool or visible.numel() != P or not visible.is_contiguous() or visible.device != dev:
                raise TypeError("visible must be a contiguous bool [P] tensor on the Gaussians' device")
            params.visible_out = visible.data_ptr()
        try:
            color, frame = _run_forward(lib, dev, params, P, W, H, _sync_free_value, state_key)
        except _lib.GsrError:
            if raster_settings.debug:
                torch.save(inputs + (tuple(raster_settings),), "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
            raise
    ctx.raster_settings = raster_settings
    ctx.profile = _lib.active_profile()     # backward runs on an autograd thread: carry the (live) object explicitly
    ctx.layout = (frame.layout_R, frame.layout_V)
    ctx.frame_pending = frame.pending
    ctx.counts = frame.counts
    ctx.binning_mode = params.binning_mode
    ctx.act_flags = act_flags
    ctx.stats = stats
    ctx.cam_shapes = None if cam[0] is None else tuple(t.shape for t in cam)
    ctx.has_means2D = means2D is not None       # a caller that wants no dL/dmeans2D may pass None: it gets None back
    ctx.keep = keep
    ctx.save_for_backward(*inputs, frame.radii, frame.geom, frame.binning, frame.img)
    ctx.mark_non_differentiable(frame.radii)
    ctx.set_materialize_grads(False)        # no (24-MB at 6 M Gaussians) zeros_like(radii) per backward for the integer output
    return color, frame.radii


def _colour_backward(fn, ctx, grad_out_color):
    """The backward of both colour operators.  ``fn._grad_buffers`` allocates the operator's gradients and says where
    they sit in ``GsrGrads`` and in the result; ``fn._ARITY`` is the length of that result without the camera's three."""
    if grad_out_color is None:
        return (None,) * (fn._ARITY if ctx.cam_shapes is None else fn._ARITY + 3)
    lib = _lib.load()
    saved = ctx.saved_tensors
    inputs = saved[:-4]
    frame, binning_mode = _frame_of(ctx, saved)
    settings = ctx.raster_settings
    dev, P = inputs[0].device, int(inputs[0].shape[0])
    grad_out_color = _f32c(grad_out_color, "grad_out_color", dev, align16=True)
    with torch.cuda.device(dev):
        params, keep = _make_params(dev, settings, *fn._params_args(inputs, dev), act_flags=ctx.act_flags)
        params.profile = ctx.profile.handle() if ctx.profile is not None else None
        params.binning_mode = binning_mode
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        slots, result = fn._grad_buffers(inputs, new, P)
        grads = _lib.GsrGrads(*slots, *_stats_ptrs(ctx.stats, P, dev))
        cam_ws, g_cam = (None, ()) if ctx.cam_shapes is None else _camera_grads(lib, grads, ctx.cam_shapes, P, dev)
        try:
            _run_backward(lib, dev, params, frame, grad_out_color, grads)
        except _lib.GsrError:
            if settings.debug:
                torch.save(inputs + (frame.radii, grad_out_color, tuple(settings)), "snapshot_bw.dump")
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
            raise
    del keep, cam_ws
    if not ctx.has_means2D:
        result[1] = None
    return tuple(result) + g_cam


class _RasterizeGaussians(torch.autograd.Function):
    _ARITY = 11

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings: GaussianRasterizationSettings, forward_only: bool = False, stats=None,
                cam_view=None, cam_proj=None, cam_pos=None):
        """``cam_view`` / ``cam_proj`` / ``cam_pos``: the settings' three camera tensors again, given when they are to
        receive gradients (``_camera_inputs``); the values are read from ``raster_settings`` either way."""
        lib = _lib.load()
        dev = _require_gpu(means3D)
        P = int(means3D.shape[0])
        means3D = _f32c(means3D, "means3D", dev)
        sh = _f32c(sh, "shs", dev, align16=True)
        colors_precomp = _f32c(colors_precomp, "colors_precomp", dev)
        opacities = _f32c(opacities, "opacities", dev)
        scales = _f32c(scales, "scales", dev)
        rotations = _f32c(rotations, "rotations", dev, align16=True)
        cov3Ds_precomp = _f32c(cov3Ds_precomp, "cov3D_precomp", dev)
        if opacities.numel() != P:
            raise ValueError("opacities must have one value per Gaussian")
        _check_rows(means3D, "means3D", P, 3)
        _check_rows(sh, "shs", P, None, 3)
        _check_rows(colors_precomp, "colors_precomp", P, 3)
        _check_rows(scales, "scales", P, 3)
        _check_rows(rotations, "rotations", P, 4)
        _check_rows(cov3Ds_precomp, "cov3D_precomp", P, 6)
        if means2D is not None and means2D.numel() and means2D.shape[0] != P:
            raise ValueError(f"means2D must have one row per Gaussian, got {list(means2D.shape)}")
        return _colour_forward(_RasterizeGaussians, ctx, lib, dev, P,
                               (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp), means2D,
                               raster_settings, forward_only, stats, (cam_view, cam_proj, cam_pos))

    @staticmethod
    def _params_args(inputs, dev):
        """What ``_make_params`` takes after the settings (seven tensors, ``sh_rest``), of the saved inputs."""
        return inputs

    @staticmethod
    def _grad_buffers(inputs, new, P):
        """(the first nine ``GsrGrads`` slots, the result list of ``backward`` without the camera's gradients)."""
        _means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp = inputs
        g_means3D, g_means2D, g_opac = new(P, 3), new(P, 3), new(*opacities.shape)
        g_sh, g_col, g_scales, g_rot, g_cov = (new(*t.shape) if t.numel() else None      # [P,M,3], [P,3], [P,3], [P,4], [P,6]:
                                               for t in (sh, colors_precomp, scales, rotations, cov3Ds_precomp))  # _check_rows
        slots = (_ptr(g_means3D), _ptr(g_means2D), _ptr(g_sh), _ptr(g_col), _ptr(g_opac), _ptr(g_scales), _ptr(g_rot),
                 _ptr(g_cov), None)
        return slots, [g_means3D, g_means2D, g_sh, g_col, g_opac, g_scales, g_rot, g_cov, None, None, None]

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        return _colour_backward(_RasterizeGaussians, ctx, grad_out_color)


class _RasterizeGaussiansFused(torch.autograd.Function):
    """Same operator fed with the RAW parameters of ``scene/gaussian_model.py`` (``_features_dc``,
    ``_features_rest``, ``_opacity``, ``_scaling``, ``_rotation``): the ``cat`` / ``sigmoid`` / ``exp`` /
    ``normalize`` of the getters at ``scene/gaussian_model.py:151-183`` and their autograd run inside the
    preprocess kernels.  Gradients are w.r.t. the raw parameters."""
    _ARITY = 12

    @staticmethod
    def forward(ctx, means3D, means2D, f_dc, f_rest, raw_opacity, raw_scales, raw_rotations,
                raster_settings: GaussianRasterizationSettings, forward_only: bool = False, stats=None, visible=None,
                state_key=None, cam_view=None, cam_proj=None, cam_pos=None):
        """``visible``: None, or a bool [P] tensor the forward fills with ``radii > 0`` (render()'s visibility_filter).
        ``state_key``: see ``_frames._run_forward``.  ``cam_*``: as in ``_RasterizeGaussians.forward``."""
        lib = _lib.load()
        dev = _require_gpu(means3D)
        P = int(means3D.shape[0])
        means3D = _f32c(means3D, "means3D", dev)
        f_dc = _f32c(f_dc, "f_dc", dev)
        f_rest = _f32c(f_rest, "f_rest", dev, align16=True)
        raw_opacity = _f32c(raw_opacity, "opacity", dev)
        raw_scales = _f32c(raw_scales, "scaling", dev)
        raw_rotations = _f32c(raw_rotations, "rotation", dev, align16=True)
        n_rest = int(f_rest.shape[1]) if f_rest.dim() == 3 else -1
        if f_dc.shape[0] != P or f_dc.numel() != 3 * P or f_rest.shape[0] != P or n_rest not in (0, 15):
            raise ValueError("fused inputs need f_dc [P,1,3] and f_rest [P,15,3] (degree-3 storage) or [P,0,3] (degree 0)")
        _check_rows(means3D, "means3D", P, 3)
        if n_rest:
            _check_rows(f_rest, "f_rest", P, 15, 3)
        _check_rows(raw_scales, "scaling", P, 3)
        _check_rows(raw_rotations, "rotation", P, 4)
        if raw_opacity.numel() != P or raw_scales.numel() != 3 * P or raw_rotations.numel() != 4 * P:
            raise ValueError("fused inputs need opacity [P,1], scaling [P,3] and rotation [P,4]")
        return _colour_forward(_RasterizeGaussiansFused, ctx, lib, dev, P,
                               (means3D, f_dc, f_rest, raw_opacity, raw_scales, raw_rotations), means2D, raster_settings,
                               forward_only, stats, (cam_view, cam_proj, cam_pos),
                               _lib.ACT_SCALE_EXP | _lib.ACT_ROT_NORMALIZE | _lib.ACT_OPACITY_SIGMOID, visible, state_key)

    @staticmethod
    def _params_args(inputs, dev):
        means3D, f_dc, f_rest, raw_opacity, raw_scales, raw_rotations = inputs
        empty = torch.empty(0, dtype=torch.float32, device=dev)
        # degree-0 storage: f_dc [P,1,3] is the whole SH tensor (M = 1), there is no rest to split off
        return means3D, f_dc, empty, raw_opacity, raw_scales, raw_rotations, empty, f_rest if f_rest.shape[1] else None

    @staticmethod
    def _grad_buffers(inputs, new, P):
        _means3D, f_dc, f_rest, raw_opacity, _raw_scales, _raw_rotations = inputs
        g_means3D, g_means2D = new(P, 3), new(P, 3)
        g_dc, g_rest = new(*f_dc.shape), new(*f_rest.shape)
        g_opac, g_scales, g_rot = new(*raw_opacity.shape), new(P, 3), new(P, 4)
        slots = (_ptr(g_means3D), _ptr(g_means2D), _ptr(g_dc), None, _ptr(g_opac), _ptr(g_scales), _ptr(g_rot), None,
                 _ptr(g_rest) if f_rest.shape[1] else None)
        return slots, [g_means3D, g_means2D, g_dc, g_rest, g_opac, g_scales, g_rot, None, None, None, None, None]

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        return _colour_backward(_RasterizeGaussiansFused, ctx, grad_out_color)


def _forward_only(*tensors) -> bool:
    """True when no backward can follow (inference): the library then skips everything only a backward reads."""
    return not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors))


class _NoGraph:
    """Stands in for the autograd context when no backward can follow: the operator's forward runs as a plain function
    (``Function.apply`` and its bookkeeping are ~20 us of host time per frame, a tenth of a 100 k-Gaussian frame)."""

    def save_for_backward(self, *tensors):
        pass

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


class _KeepFrame(_NoGraph):
    """A stand-in context that keeps what the colour forward saves: the frame of a forward that runs outside autograd
    but whose depth / alpha maps are wanted."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def _frame_of(node, saved=None):
    """(_Frame, binning mode) of a colour node: its autograd context, or a ``_KeepFrame``.  The workspaces are the
    tensors the node saved (``saved``: its ``saved_tensors``, where the caller has unpacked them), by reference."""
    radii, geom, binning, img = (node.saved_tensors if saved is None else saved)[-4:]
    return _Frame(geom, binning, img, radii, node.layout[0], node.layout[1], node.frame_pending, node.counts), node.binning_mode


def _aux_frame(frame: _Frame, P: int, W: int, H: int, binning_mode: int) -> "_lib.GsrAuxFrame":
    f = _lib.GsrAuxFrame()
    f.P, f.width, f.height, f.binning_mode = P, W, H, int(binning_mode)
    f.num_rendered, f.num_visible = int(frame.layout_R), int(frame.layout_V)
    f.geom_ws, f.bin_ws, f.img_ws, f.radii = _ptr(frame.geom), _ptr(frame.binning), _ptr(frame.img), _ptr(frame.radii)
    return f


def _geometry_inputs(dev, means3D, opacities, scales, rotations, cov3Ds_precomp):
    """The geometry inputs of a map node as contiguous float32 tensors on ``dev`` (rotations 16-byte aligned)."""
    return (_f32c(means3D, "means3D", dev), _f32c(opacities, "opacities", dev), _f32c(scales, "scales", dev),
            _f32c(rotations, "rotations", dev, align16=True), _f32c(cov3Ds_precomp, "cov3D_precomp", dev))


def _stash_frame(ctx, raster_settings, frame: _Frame, binning_mode: int, tensors, act_flags: int = 0, has_means2D=False):
    """What a map node keeps for its backward: the settings, the frame's layout and counts, and ``tensors`` followed by
    the frame's four workspaces -- ``_frame_of`` takes those from the end of what was saved."""
    ctx.raster_settings = raster_settings
    ctx.layout = (frame.layout_R, frame.layout_V)
    ctx.frame_pending = frame.pending
    ctx.counts = frame.counts
    ctx.binning_mode = binning_mode
    ctx.act_flags = int(act_flags)
    ctx.has_means2D = has_means2D
    ctx.save_for_backward(*tensors, frame.radii, frame.geom, frame.binning, frame.img)


def _open_backward(ctx, saved, means3D, *geometry):
    """The start of a map node's backward: -> (dev, P, params, keep, aux_frame).  ``geometry``: the saved opacities,
    scales, rotations and cov3D_precomp (none for a node that reads means3D alone).  ``keep`` holds what ``params``
    points at; the caller drops it after its library call."""
    frame, binning_mode = _frame_of(ctx, saved)
    settings = ctx.raster_settings
    dev = means3D.device
    P = int(means3D.shape[0])
    H, W = int(settings.image_height), int(settings.image_width)
    if frame.pending is not None:
        _verify(frame.pending, block=True)      # deferred mode: as the colour backward
    empty = torch.empty(0, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        params, keep = _make_params(dev, settings, means3D, empty, empty, *(geometry or (empty,) * 4),
                                    act_flags=ctx.act_flags)
    params.profile = None
    params.binning_mode = binning_mode
    return dev, P, params, keep, _aux_frame(frame, P, W, H, binning_mode)


def _geometry_grads(dev, P, nbytes_of, opacities, scales, rotations, cov3Ds_precomp):
    """The outputs of a map's geometry backward: -> (the six gradient tensors for means3D, means2D, opacities, scales,
    rotations, cov3D_precomp (None where the input is absent), ``GsrAuxGrads`` over them, the accumulator workspace of
    ``nbytes_of(P)`` bytes, that size)."""
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
    g = (new(P, 3), new(P, 3), new(*opacities.shape)) + tuple(
        new(P, n) if t.numel() else None for t, n in ((scales, 3), (rotations, 4), (cov3Ds_precomp, 6)))
    nbytes = nbytes_of(P)
    return g, _lib.GsrAuxGrads(*(_ptr(t) for t in g)), torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def _geometry_result(ctx, g, *rest):
    """``backward``'s return tuple: the six geometry gradients (means2D's only if the input was given), then ``rest``."""
    return (g[0], g[1] if ctx.has_means2D else None) + tuple(g[2:]) + rest


class _AuxMaps(torch.autograd.Function):
    """Depth, inverse-depth and accumulated-opacity maps ``[3,H,W]`` of a frame the colour operator has rendered
    (``include/gsr.h``: gsr_aux_maps_*; ``csrc/depth.hip``).  A node of its own next to the colour node: it reads the
    colour node's frame (the same ``geom`` / ``binning`` / ``img`` tensors, by reference) and returns the maps' own
    gradients for means3D, means2D, opacities and scales / rotations or cov3D_precomp; autograd adds them to the colour
    node's.  ``act_flags``: the geometry inputs are the raw parameters of the fused path."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings: GaussianRasterizationSettings, frame: _Frame, binning_mode: int, act_flags: int = 0):
        lib = _lib.load()
        dev = _require_gpu(means3D)
        P = int(means3D.shape[0])
        geometry = _geometry_inputs(dev, means3D, opacities, scales, rotations, cov3Ds_precomp)
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        maps = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gsr_aux_maps_forward(C.byref(_aux_frame(frame, P, W, H, binning_mode)), maps.data_ptr(),
                                                _stream(dev)), "gsr_aux_maps_forward")
        _stash_frame(ctx, raster_settings, frame, binning_mode, geometry, act_flags, means2D is not None)
        return maps

    @staticmethod
    def backward(ctx, grad_maps):
        if grad_maps is None:
            return (None,) * 10
        lib = _lib.load()
        saved = ctx.saved_tensors
        dev, P, params, keep, aux_frame = _open_backward(ctx, saved, *saved[:5])
        grad_maps = _f32c(grad_maps, "grad_maps", dev)
        with torch.cuda.device(dev):
            g, grads, acc, nbytes = _geometry_grads(dev, P, lib.gsr_aux_maps_backward_bytes, *saved[1:5])
            _lib.check(lib.gsr_aux_maps_backward(C.byref(params), C.byref(aux_frame), grad_maps.data_ptr(), acc.data_ptr(),
                                                 nbytes, C.byref(grads), _stream(dev)), "gsr_aux_maps_backward")
        del keep
        return _geometry_result(ctx, g, None, None, None, None)


def _aux_maps_of(node, grad: bool, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                 act_flags: int = 0):
    frame, mode = _frame_of(node)
    if grad:
        return _AuxMaps.apply(means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, raster_settings, frame,
                              mode, act_flags)
    return _AuxMaps.forward(_NoGraph(), means3D, means2D, opacities, scales, rotations, cov3Ds_precomp,
                            raster_settings, frame, mode, act_flags)


class _FeatureMaps(torch.autograd.Function):
    """``feat [C,H,W] = sum w features[id]`` of a frame the colour operator has rendered (``include/gsr.h``:
    gsr_feature_maps_*; ``csrc/features.hip``).  A node of its own next to the colour node, built like ``_AuxMaps``: it
    reads the colour node's frame and returns the maps' own gradients for ``features`` and for means3D, means2D,
    opacities and scales / rotations or cov3D_precomp.  Only the side ``ctx.needs_input_grad`` asks for is computed."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, features,
                raster_settings: GaussianRasterizationSettings, frame: _Frame, binning_mode: int, act_flags: int = 0):
        lib = _lib.load()
        dev = _require_gpu(means3D)
        P = int(means3D.shape[0])
        geometry = _geometry_inputs(dev, means3D, opacities, scales, rotations, cov3Ds_precomp)
        features = _f32c(features, "features", dev)
        n_ch = int(features.shape[1])
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        maps = torch.empty(n_ch, H, W, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if P == 0:
                maps.zero_()        # no row to point at: nothing was binned
            else:
                _lib.check(lib.gsr_feature_maps_forward(C.byref(_aux_frame(frame, P, W, H, binning_mode)),
                                                        features.data_ptr(), n_ch, maps.data_ptr(), _stream(dev)),
                           "gsr_feature_maps_forward")
        _stash_frame(ctx, raster_settings, frame, binning_mode, geometry + (features,), act_flags, means2D is not None)
        return maps

    @staticmethod
    def backward(ctx, grad_maps):
        if grad_maps is None:
            return (None,) * 11
        need = ctx.needs_input_grad
        want_geom, want_feat = any(need[:6]), bool(need[6])
        if not (want_geom or want_feat):
            return (None,) * 11
        lib = _lib.load()
        saved = ctx.saved_tensors
        features = saved[5]
        dev, P, params, keep, aux_frame = _open_backward(ctx, saved, *saved[:5])
        n_ch = int(features.shape[1])
        grad_maps = _f32c(grad_maps, "grad_maps", dev)
        g, grads, acc, nbytes, g_feat = (None,) * 6, None, None, 0, None
        with torch.cuda.device(dev):
            if want_geom:
                g, grads, acc, nbytes = _geometry_grads(dev, P, lib.gsr_feature_maps_backward_bytes, *saved[1:5])
            if want_feat:
                g_feat = torch.empty(P, n_ch, dtype=torch.float32, device=dev)
            if P > 0:
                _lib.check(lib.gsr_feature_maps_backward(
                    C.byref(params), C.byref(aux_frame), features.data_ptr(), n_ch, grad_maps.data_ptr(), _ptr(g_feat),
                    _ptr(acc), nbytes, None if grads is None else C.byref(grads), _stream(dev)),
                    "gsr_feature_maps_backward")
        del keep
        return _geometry_result(ctx, g, g_feat, None, None, None, None)


def _feature_maps_of(node, grad: bool, features, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp,
                     raster_settings, act_flags: int = 0):
    frame, mode = _frame_of(node)
    if grad:
        return _FeatureMaps.apply(means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, features,
                                  raster_settings, frame, mode, act_flags)
    with torch.no_grad():
        return _FeatureMaps.forward(_NoGraph(), means3D, means2D, opacities, scales, rotations, cov3Ds_precomp,
                                    features, raster_settings, frame, mode, act_flags)


_DIST_MAPPINGS = {"linear": 0, "ndc": 1}


def _distortion_spec(distortion):
    """``distortion`` of the operator as (mapping, near, far), or None when the map is not asked for.  Raises ValueError
    for anything else, before anything is enqueued (the library's own refusals, restated where the caller can read them)."""
    if distortion is None or distortion is False:
        return None
    if distortion is True:
        distortion = {}
    if not isinstance(distortion, dict):
        raise ValueError(f"distortion must be True or a dict(mapping=, near=, far=), got {type(distortion).__name__}")
    unknown = set(distortion) - {"mapping", "near", "far"}
    if unknown:
        raise ValueError(f"distortion: unknown keys {sorted(unknown)}")
    name = distortion.get("mapping", "ndc")
    if name not in _DIST_MAPPINGS:
        raise ValueError(f"distortion mapping must be one of {sorted(_DIST_MAPPINGS)}, got {name!r}")
    near, far = float(distortion.get("near", 0.2)), float(distortion.get("far", 100.0))
    if name == "ndc" and not (0.0 < near < far < float("inf")):
        raise ValueError(f"distortion mapping 'ndc' needs finite 0 < near < far, got near={near}, far={far}")
    return _DIST_MAPPINGS[name], near, far


class _DistortionMap(torch.autograd.Function):
    """``dist [1,H,W]``, the depth-distortion map of a frame the colour operator has rendered (``include/gsr.h``:
    gsr_distortion_*; ``csrc/distortion.hip``).  A node of its own next to the colour node, built like ``_AuxMaps``: it
    reads the colour node's frame and returns the map's own gradients for means3D, means2D, opacities and scales /
    rotations or cov3D_precomp.  The forward also leaves the per-pixel ``state [2,H,W]`` the backward reads."""

    @staticmethod
    def forward(ctx, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings: GaussianRasterizationSettings, frame: _Frame, binning_mode: int, act_flags: int = 0,
                spec=(1, 0.2, 100.0)):
        lib = _lib.load()
        dev = _require_gpu(means3D)
        P = int(means3D.shape[0])
        geometry = _geometry_inputs(dev, means3D, opacities, scales, rotations, cov3Ds_precomp)
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        mapping, near, far = spec
        dist = torch.empty(1, H, W, dtype=torch.float32, device=dev)
        state = torch.empty(2, H, W, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.gsr_distortion_forward(C.byref(_aux_frame(frame, P, W, H, binning_mode)), mapping, near, far,
                                                  dist.data_ptr(), state.data_ptr(), _stream(dev)),
                       "gsr_distortion_forward")
        ctx.spec = (int(mapping), float(near), float(far))
        _stash_frame(ctx, raster_settings, frame, binning_mode, geometry + (state,), act_flags, means2D is not None)
        return dist

    @staticmethod
    def backward(ctx, grad_dist):
        if grad_dist is None:
            return (None,) * 11
        lib = _lib.load()
        saved = ctx.saved_tensors
        state = saved[5]
        dev, P, params, keep, aux_frame = _open_backward(ctx, saved, *saved[:5])
        grad_dist = _f32c(grad_dist, "grad_dist", dev)
        mapping, near, far = ctx.spec
        with torch.cuda.device(dev):
            g, grads, acc, nbytes = _geometry_grads(dev, P, lib.gsr_distortion_backward_bytes, *saved[1:5])
            _lib.check(lib.gsr_distortion_backward(C.byref(params), C.byref(aux_frame), mapping, near, far,
                                                   state.data_ptr(), grad_dist.data_ptr(), acc.data_ptr(), nbytes,
                                                   C.byref(grads), _stream(dev)), "gsr_distortion_backward")
        del keep
        return _geometry_result(ctx, g, None, None, None, None, None)


def _distortion_of(node, grad: bool, spec, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp,
                   raster_settings, act_flags: int = 0):
    frame, mode = _frame_of(node)
    if grad:
        return _DistortionMap.apply(means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                                    frame, mode, act_flags, spec)
    return _DistortionMap.forward(_NoGraph(), means3D, means2D, opacities, scales, rotations, cov3Ds_precomp,
                                  raster_settings, frame, mode, act_flags, spec)


def _check_distortion_request(cam, state_key=None, densify_stats=None) -> None:
    """The refusals of a ``distortion=`` request (those of ``aux_maps=True``), before anything is enqueued."""
    if densify_stats is not None:
        raise ValueError("distortion cannot be combined with densify_stats: the in-backward statistics would see the "
                         "colour node's dL/dmeans2D alone, without the map's share (take them from the summed "
                         "means2D.grad after the backward)")
    if cam:
        raise ValueError("distortion cannot be combined with camera tensors that require grad: the distortion map has no "
                         "camera gradients (detach viewmatrix / projmatrix / campos, or render the map in a frame of "
                         "its own)")
    if state_key is not None:
        raise ValueError("distortion is not available on a frame with grown / split rows appended")


class _MedianDepth(torch.autograd.Function):
    """``median [1,H,W]`` and ``median_id [H,W]`` (int32) of a frame the colour operator has rendered (``include/gsr.h``:
    gsr_median_depth_*; ``csrc/median.hip``).  A node of its own next to the colour node, in the style of
    ``_DistortionMap``: it reads the colour node's frame by reference.  The selection of the median entry is piecewise
    constant, so means3D is the node's only differentiable input (``dL/dmeans3D[id] = sum of the gradient over the
    pixels that chose id, times viewmatrix[0:3, 2]``); means2D, opacities, scales, rotations and cov3D_precomp are not
    inputs of the node and receive nothing from it (``None``, not zeros).  ``median_id`` is marked non-differentiable.  The
    forward also leaves the per-pixel ``state [H,W]`` (uint32) the backward reads."""

    @staticmethod
    def forward(ctx, means3D, raster_settings: GaussianRasterizationSettings, frame: _Frame, binning_mode: int):
        lib = _lib.load()
        dev = _require_gpu(means3D)
        P = int(means3D.shape[0])
        means3D = _f32c(means3D, "means3D", dev)
        H, W = int(raster_settings.image_height), int(raster_settings.image_width)
        median = torch.empty(1, H, W, dtype=torch.float32, device=dev)
        median_id = torch.empty(H, W, dtype=torch.int32, device=dev)
        state = torch.empty(H, W, dtype=torch.int32, device=dev)      # uint32 on the device; opaque here
        with torch.cuda.device(dev):
            _lib.check(lib.gsr_median_depth_forward(C.byref(_aux_frame(frame, P, W, H, binning_mode)), median.data_ptr(),
                                                    median_id.data_ptr(), state.data_ptr(), _stream(dev)),
                       "gsr_median_depth_forward")
        _stash_frame(ctx, raster_settings, frame, binning_mode, (means3D, state))
        ctx.mark_non_differentiable(median_id)
        ctx.set_materialize_grads(False)
        return median, median_id

    @staticmethod
    def backward(ctx, grad_median, _grad_id):
        if grad_median is None:
            return (None,) * 4
        lib = _lib.load()
        saved = ctx.saved_tensors
        state = saved[1]
        dev, P, params, keep, aux_frame = _open_backward(ctx, saved, saved[0])
        grad_median = _f32c(grad_median, "grad_median", dev)
        with torch.cuda.device(dev):
            g_means3D = torch.empty(P, 3, dtype=torch.float32, device=dev)
            nbytes = lib.gsr_median_depth_backward_bytes(P)
            acc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.check(lib.gsr_median_depth_backward(C.byref(params), C.byref(aux_frame), state.data_ptr(),
                                                     grad_median.data_ptr(), acc.data_ptr(), nbytes, _ptr(g_means3D),
                                                     _stream(dev)), "gsr_median_depth_backward")
        del keep
        return (g_means3D, None, None, None)


def _median_of(node, grad: bool, means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
               act_flags: int = 0):
    """(median, median_id) of the colour node's frame; of ``geometry`` only means3D and the settings are read."""
    frame, mode = _frame_of(node)
    if grad:
        return _MedianDepth.apply(means3D, raster_settings, frame, mode)
    return _MedianDepth.forward(_NoGraph(), means3D, raster_settings, frame, mode)


def _check_median_request(cam, state_key=None, densify_stats=None) -> None:
    """The refusals of a ``median_depth=True`` request (those of ``aux_maps=True``), before anything is enqueued."""
    if densify_stats is not None:
        raise ValueError("median_depth=True cannot be combined with densify_stats: a frame that keeps its state for the "
                         "maps takes the densification statistics from the summed means2D.grad after the backward, as "
                         "with aux_maps=True")
    if cam:
        raise ValueError("median_depth=True cannot be combined with camera tensors that require grad: the median-depth map "
                         "has no camera gradients (detach viewmatrix / projmatrix / campos, or render the map in a frame "
                         "of its own)")
    if state_key is not None:
        raise ValueError("median_depth=True is not available on a frame with grown / split rows appended")


def _check_feature_request(features, means3D, cam, state_key=None, densify_stats=None) -> None:
    """The refusals of a ``features=F`` request, before anything is enqueued (and before a GPU is asked for)."""
    if densify_stats is not None:
        raise ValueError("features cannot be combined with densify_stats: the in-backward statistics would see the "
                         "colour node's dL/dmeans2D alone, without the feature maps' share (take them from the summed "
                         "means2D.grad after the backward)")
    if cam:
        raise ValueError("features cannot be combined with camera tensors that require grad: the feature maps have no "
                         "camera gradients (detach viewmatrix / projmatrix / campos, or render the maps in a frame of "
                         "their own)")
    if state_key is not None:
        raise ValueError("features are not available on a frame with grown / split rows appended")
    P = int(means3D.shape[0])
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or \
            int(features.shape[0]) != P or int(features.shape[1]) < 1:
        raise ValueError(f"features must be a float32 [P={P}, C>=1] tensor, got "
                         f"{getattr(features, 'dtype', type(features).__name__)} {list(getattr(features, 'shape', ()))}")
    if features.device != means3D.device:
        raise ValueError(f"features is on {features.device}, expected {means3D.device}")


class _AbsGrad(torch.autograd.Function):
    """AbsGS's absolute view-space gradient of a frame the colour operator has rendered (``include/gsr.h``:
    gsr_abs_grad_backward; ``csrc/abs_grad.hip``).  The node sits on the colour image: the forward hands the image on,
    the backward hands the incoming gradient on (the same tensor: the colour node sees what it sees without this node) and,
    from that gradient and the colour node's frame (read by reference), fills ``means2D_abs``'s gradient ``[P,3]``."""

    @staticmethod
    def forward(ctx, color, means2D_abs, means3D, raster_settings: GaussianRasterizationSettings, frame: _Frame,
                binning_mode: int):
        _stash_frame(ctx, raster_settings, frame, binning_mode, (means3D,))
        return color.view_as(color)

    @staticmethod
    def backward(ctx, grad_color):
        if grad_color is None or not ctx.needs_input_grad[1]:
            return (grad_color, None, None, None, None, None)
        lib = _lib.load()
        saved = ctx.saved_tensors
        dev, P, params, keep, aux_frame = _open_backward(ctx, saved, saved[0])
        g = _f32c(grad_color, "grad_out_color", dev)
        with torch.cuda.device(dev):
            g_abs = torch.empty(P, 3, dtype=torch.float32, device=dev)
            if P > 0:
                _lib.check(lib.gsr_abs_grad_backward(C.byref(params), C.byref(aux_frame), g.data_ptr(), g_abs.data_ptr(),
                                                     _stream(dev)), "gsr_abs_grad_backward")
        del keep
        return (grad_color, g_abs, None, None, None, None)


def _check_abs_request(means2D_abs, means3D, cam, state_key=None, densify_stats=None) -> None:
    """The refusals of an ``abs_grad=True`` request (those of ``aux_maps=True``), before anything is enqueued (and before
    a GPU is asked for)."""
    if densify_stats is not None:
        raise ValueError("abs_grad=True cannot be combined with densify_stats: the in-backward statistics know nothing "
                         "of the absolute gradient (take both from means2D.grad and means2D_abs.grad after the backward)")
    if cam:
        raise ValueError("abs_grad=True cannot be combined with camera tensors that require grad (detach viewmatrix / "
                         "projmatrix / campos)")
    if state_key is not None:
        raise ValueError("abs_grad=True is not available on a frame with grown / split rows appended")
    P = int(means3D.shape[0])
    if not isinstance(means2D_abs, torch.Tensor) or means2D_abs.dtype != torch.float32 or \
            tuple(means2D_abs.shape) != (P, 3):
        raise ValueError(f"abs_grad=True needs means2D_abs, a float32 [P={P}, 3] tensor whose .grad receives the absolute "
                         f"gradient, got {getattr(means2D_abs, 'dtype', type(means2D_abs).__name__)} "
                         f"{list(getattr(means2D_abs, 'shape', ()))}")
    if means2D_abs.device != means3D.device:
        raise ValueError(f"means2D_abs is on {means2D_abs.device}, expected {means3D.device}")


def _check_aux_request(cam, state_key=None, densify_stats=None) -> None:
    if densify_stats is not None:
        raise ValueError("aux_maps=True cannot be combined with densify_stats: the in-backward statistics would see the "
                         "colour node's dL/dmeans2D alone, without the maps' share (take them from the summed "
                         "means2D.grad after the backward)")
    if cam:
        raise ValueError("aux_maps=True cannot be combined with camera tensors that require grad: the depth / alpha maps "
                         "have no camera gradients (detach viewmatrix / projmatrix / campos, or render the maps in a "
                         "frame of their own)")
    if state_key is not None:
        raise ValueError("aux_maps=True is not available on a frame with grown / split rows appended")


def _check_contribution_request(stats, mask, means3D, settings, state_key=None) -> None:
    """The refusals of a ``contribution=stats`` request, before anything is enqueued."""
    if state_key is not None:
        raise ValueError("contribution statistics are not available on a frame with grown / split rows appended")
    raw = getattr(stats, "raw", None)
    P = int(means3D.shape[0])
    if not isinstance(raw, torch.Tensor) or raw.dtype != torch.int64 or raw.dim() != 2 or raw.shape[1] != 3 or \
            not raw.is_contiguous():
        raise ValueError("contribution must carry `raw`, a contiguous int64 [P,3] tensor (contribution.ContributionStats)")
    if raw.shape[0] != P:
        raise ValueError(f"contribution statistics have {int(raw.shape[0])} rows, the frame has P={P} Gaussians")
    H, W = int(settings.image_height), int(settings.image_width)
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or
                             tuple(mask.shape) != (H, W)):
        raise ValueError(f"contribution_mask must be a uint8 [H={H}, W={W}] tensor, got "
                         f"{getattr(mask, 'dtype', type(mask).__name__)} {list(getattr(mask, 'shape', ()))}")
    dev = _require_gpu(means3D)
    for name, t in (("contribution.raw", raw), ("contribution_mask", mask)):
        if t is not None and not t.is_cuda:
            raise _lib.GsrError(f"{name} is on {t.device}: the statistics accumulate on the ROCm GPU (no CPU path)")
        if t is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, expected {dev}")


def _accumulate_contribution(node, stats, mask, means3D, settings) -> None:
    """Add the statistics of the colour node's frame into ``stats.raw`` (``gsr_contribution_accumulate``) and count the
    view.  Reads the frame's saved state only; no host synchronisation, nothing for autograd."""
    frame, mode = _frame_of(node)
    dev = means3D.device
    mask = None if mask is None else mask.contiguous()
    with torch.cuda.device(dev):
        f = _aux_frame(frame, int(means3D.shape[0]), int(settings.image_width), int(settings.image_height), mode)
        _lib.check(_lib.load().gsr_contribution_accumulate(C.byref(f), _ptr(mask), _ptr(stats.raw), _stream(dev)),
                   "gsr_contribution_accumulate")
    stats.views += 1


def _with_frame_outputs(color, radii, node, grad: bool, geometry, aux_maps, contribution, contribution_mask,
                        features=None, grad_features: bool = False, distortion=None, median_depth: bool = False):
    """The results of a frame that kept its state: the statistics are accumulated, the maps appended when asked for
    (``aux``, then ``feat``, then ``dist``, then ``median`` and ``median_id``).  ``grad``: the colour node is an autograd node; ``grad_features``: the feature
    maps get a node although the colour forward ran outside autograd (only ``features`` requires grad).
    ``distortion``: the (mapping, near, far) of ``_distortion_spec``."""
    if contribution is not None:
        _accumulate_contribution(node, contribution, contribution_mask, geometry[0], geometry[6])
    out = (color, radii)
    if aux_maps:
        out += (_aux_maps_of(node, grad, *geometry),)
    if features is not None:
        out += (_feature_maps_of(node, grad or grad_features, features, *geometry),)
    if distortion is not None:
        out += (_distortion_of(node, grad, distortion, *geometry),)
    if median_depth:
        out += tuple(_median_of(node, grad, *geometry))
    return out


def _rasterize(fn, tensors, raster_settings, tail, geometry, densify_stats, aux_maps, contribution, contribution_mask,
               state_key=None, features=None, distortion=None, median_depth=False, means2D_abs=None, abs_grad=False):
    """One frame through the colour operator ``fn``.  ``tensors``: its forward's arguments in front of ``raster_settings``;
    ``tail``: those between ``stats`` and the camera's; ``geometry``: the arguments of ``_aux_maps_of`` after ``grad``
    when ``aux_maps``, ``contribution``, ``features``, ``distortion`` or ``median_depth`` ask for the frame's state, else
    None.
    ``distortion``: None, or the (mapping, near, far) of ``_distortion_spec``.
    ``abs_grad``: ``means2D_abs``'s gradient is wanted (``_AbsGrad``); a frame no backward can follow is issued without."""
    cam = _camera_inputs(raster_settings)
    if abs_grad:
        _check_abs_request(means2D_abs, tensors[0], cam, state_key, densify_stats)
    if aux_maps:
        _check_aux_request(cam, state_key, densify_stats)
    if distortion is not None:
        _check_distortion_request(cam, state_key, densify_stats)
    if median_depth:
        _check_median_request(cam, state_key, densify_stats)
    if features is not None:
        _check_feature_request(features, tensors[0], cam, state_key, densify_stats)
    if contribution is not None:
        _check_contribution_request(contribution, contribution_mask, tensors[0], raster_settings, state_key)
    if _forward_only(*tensors, *cam):
        grad_features = features is not None and not _forward_only(features)
        with torch.no_grad():
            if geometry is None:
                return fn.forward(_NoGraph(), *tensors, raster_settings, True, None, *tail)
            # the frame runs with forward_only = 0, here and below: the requests read the state only a forward that
            node = _KeepFrame()     # tracks its contributors leaves
            color, radii = fn.forward(node, *tensors, raster_settings, False, None, *tail)
            if not grad_features:
                return _with_frame_outputs(color, radii, node, False, geometry, aux_maps, contribution,
                                           contribution_mask, features, distortion=distortion,
                                           median_depth=median_depth)
            head = _with_frame_outputs(color, radii, node, False, geometry, aux_maps, contribution, contribution_mask)
            dist = () if distortion is None else (_distortion_of(node, False, distortion, *geometry),)
            if median_depth:
                dist += tuple(_median_of(node, False, *geometry))
        # only ``features`` requires grad: its node is built with grad mode as the caller has it
        return head + (_feature_maps_of(node, True, features, *geometry),) + dist
    out = fn.apply(*tensors, raster_settings, False, densify_stats, *tail, *cam)
    node = out[0].grad_fn
    if abs_grad and means2D_abs.requires_grad:
        out = (_AbsGrad.apply(out[0], means2D_abs, tensors[0], raster_settings, *_frame_of(node)),) + tuple(out[1:])
    if geometry is None:
        return out
    return _with_frame_outputs(*out, node, True, geometry, aux_maps, contribution, contribution_mask, features,
                               distortion=distortion, median_depth=median_depth)


def rasterize_gaussians_fused(means3D, means2D, f_dc, f_rest, raw_opacity, raw_scales, raw_rotations, raster_settings,
                              densify_stats=None, visible=None, _state_key=None, aux_maps=False, contribution=None,
                              contribution_mask=None, features=None, distortion=None, median_depth=False,
                              means2D_abs=None, abs_grad=False):
    """``densify_stats``: None, or (xyz_gradient_accum, denom, max_radii2D) -- the backward then also accumulates the
    densification statistics of ``scene/gaussian_model.py:775-777`` / ``train.py:130``.
    ``visible``: None, or a bool [P] tensor that receives ``radii > 0`` from the preprocess kernel.
    ``_state_key`` (internal): the capacity state of grown frames (``_grown_key``) instead of the one of P rows.
    ``aux_maps``: also return the depth / inverse-depth / alpha maps ``[3,H,W]`` (``_AuxMaps``) as a third result.
    ``contribution`` / ``contribution_mask``: accumulate the frame's contribution statistics (module docstring).
    ``features``: float32 ``[P,C]``; also return ``feat [C,H,W] = sum w features[id]`` (``_FeatureMaps``) after ``aux``.
    ``distortion``: True or ``dict(mapping=, near=, far=)``; also return ``dist [1,H,W]`` (``_DistortionMap``) after ``feat``.
    ``median_depth``: also return ``median [1,H,W]`` and ``median_id [H,W]`` (``_MedianDepth``) as the last two results.
    ``abs_grad`` / ``means2D_abs``: float32 ``[P,3]`` whose ``.grad`` receives the absolute gradient (``_AbsGrad``)."""
    geometry = None
    distortion = _distortion_spec(distortion)
    median_depth = bool(median_depth)
    if aux_maps or contribution is not None or features is not None or distortion is not None or median_depth:
        empty = torch.empty(0, dtype=torch.float32, device=means3D.device)
        flags = _lib.ACT_SCALE_EXP | _lib.ACT_ROT_NORMALIZE | _lib.ACT_OPACITY_SIGMOID
        geometry = (means3D, means2D, raw_opacity, raw_scales, raw_rotations, empty, raster_settings, flags)
    return _rasterize(_RasterizeGaussiansFused,
                      (means3D, means2D, f_dc, f_rest, raw_opacity, raw_scales, raw_rotations), raster_settings,
                      (visible, _state_key), geometry, densify_stats, aux_maps, contribution, contribution_mask, _state_key,
                      features, distortion, median_depth, means2D_abs, abs_grad)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, densify_stats=None, aux_maps=False, contribution=None, contribution_mask=None,
                        features=None, distortion=None, median_depth=False, means2D_abs=None, abs_grad=False):
    distortion = _distortion_spec(distortion)
    median_depth = bool(median_depth)
    geometry = (means3D, means2D, opacities, scales, rotations, cov3Ds_precomp, raster_settings) \
        if aux_maps or contribution is not None or features is not None or distortion is not None or median_depth else None
    return _rasterize(_RasterizeGaussians,
                      (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp),
                      raster_settings, (), geometry, densify_stats, aux_maps, contribution, contribution_mask,
                      features=features, distortion=distortion, median_depth=median_depth, means2D_abs=means2D_abs,
                      abs_grad=abs_grad)


class GaussianRasterizer(nn.Module):
    """Same call contract as the module the reference constructs per frame
    (``gaussian_renderer/__init__.py:57``) and calls at ``:257-265``."""

    def __init__(self, raster_settings: GaussianRasterizationSettings, aux_maps: bool = False, contribution=None,
                 contribution_mask: Optional[torch.Tensor] = None, distortion=None, median_depth: bool = False,
                 abs_grad: bool = False):
        """``aux_maps=True``: the call returns ``(color, radii, aux)`` with ``aux [3,H,W]`` = the depth
        (``sum w z``), inverse-depth (``sum w / z``) and accumulated-opacity (``sum w``) maps of the frame,
        differentiable in means3D, means2D, opacities and scales / rotations or cov3D_precomp.
        ``contribution``: a ``contribution.ContributionStats`` that every call adds its frame's per-Gaussian statistics
        into; ``contribution_mask``: uint8 ``[H,W]``, pixels with 0 are left out.  Not differentiable.
        ``distortion``: True, or ``dict(mapping="linear" | "ndc", near=0.2, far=100.0)``: the call's results gain a
        trailing ``dist [1,H,W]``, the depth-distortion map (module docstring), differentiable in the geometry inputs.
        ``median_depth=True``: the call's results gain, after everything else, ``median [1,H,W]`` (2DGS's median depth,
        differentiable in means3D alone) and ``median_id [H,W]`` (int32: the Gaussian that owns the pixel, -1 for none).
        ``abs_grad=True``: the call takes ``means2D_abs [P,3]``, whose ``.grad`` holds AbsGS's absolute view-space gradient
        of the colour image after ``backward`` (module docstring); the call's results are what they are without it."""
        super().__init__()
        _distortion_spec(distortion)        # a malformed request is refused here, not at the first frame
        self.raster_settings = raster_settings
        self.aux_maps = bool(aux_maps)
        self.contribution = contribution
        self.contribution_mask = contribution_mask
        self.distortion = distortion
        self.median_depth = bool(median_depth)
        self.abs_grad = bool(abs_grad)

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Frustum (near-plane) visibility of the upstream module's ``markVisible``; bool ``[P]``."""
        lib = _lib.load()
        dev = _require_gpu(positions)
        with torch.no_grad(), torch.cuda.device(dev):
            pos = _f32c(positions, "positions", dev)
            view = _f32c(self.raster_settings.viewmatrix, "viewmatrix", dev)
            vis = torch.empty(pos.shape[0], dtype=torch.uint8, device=dev)
            _lib.check(lib.gsr_mark_visible(int(pos.shape[0]), _ptr(pos), view.data_ptr(), _ptr(vis), _stream(dev)),
                       "gsr_mark_visible")
        return vis.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, densify_stats=None, features=None, means2D_abs=None):
        """``features``: float32 ``[P,C]``, C >= 1: the call's results gain a trailing ``feat [C,H,W] = sum w features[id]``
        (after ``aux`` when ``aux_maps=True``), differentiable in ``features`` and the geometry inputs.
        ``means2D_abs``: with ``abs_grad=True``, the ``[P,3]`` tensor whose ``.grad`` receives the absolute gradient."""
        raster_settings = self.raster_settings
        self._check_means2D_abs(means2D_abs)
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
           ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = torch.empty(0, dtype=torch.float32, device=means3D.device)
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, raster_settings, densify_stats, aux_maps=self.aux_maps,
                                   contribution=self.contribution, contribution_mask=self.contribution_mask,
                                   features=features, **({} if self.distortion is None else {"distortion": self.distortion}),
                                   **({"median_depth": True} if self.median_depth else {}),
                                   **({"means2D_abs": means2D_abs, "abs_grad": True} if self.abs_grad else {}))

    def _check_means2D_abs(self, means2D_abs) -> None:
        if means2D_abs is not None and not self.abs_grad:
            raise ValueError("means2D_abs needs GaussianRasterizer(..., abs_grad=True)")

    def forward_fused(self, means3D, means2D, f_dc, f_rest, raw_opacity, raw_scales, raw_rotations, densify_stats=None,
                      features=None, means2D_abs=None):
        """Raw-parameter entry: see :class:`_RasterizeGaussiansFused`."""
        self._check_means2D_abs(means2D_abs)
        return rasterize_gaussians_fused(means3D, means2D, f_dc, f_rest, raw_opacity, raw_scales, raw_rotations,
                                         self.raster_settings, densify_stats, aux_maps=self.aux_maps,
                                         contribution=self.contribution, contribution_mask=self.contribution_mask,
                                         features=features,
                                         **({} if self.distortion is None else {"distortion": self.distortion}),
                                         **({"median_depth": True} if self.median_depth else {}),
                                         **({"means2D_abs": means2D_abs, "abs_grad": True} if self.abs_grad else {}))
