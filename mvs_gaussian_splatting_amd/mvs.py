"""Multi-view geometric consistency of rendered depth, and the fused point cloud it yields, on the HIP path
(``csrc/mvs.hip`` behind ``gsr_mvs_consistency`` / ``gsr_depth_backproject``), and the same round trip as
a training loss with gradients (``csrc/mvs_loss.hip`` behind ``gsr_mvs_geo_loss_fwd_bwd``), and the
photometric half of that loss, the patch NCC between the two photographs under the rendered plane's homography
(``csrc/mvs_ncc.hip`` behind ``gsr_mvs_ncc_loss_fwd_bwd``).

    sources = select_source_views(cameras, n_sources=4)
    count, fused = depth_consistency(depths[i], cameras[i], [depths[j] for j in sources[i]], [cameras[j] for j in sources[i]])
    xyz, rgb = fuse_depth_points(scene.getTrainCameras(), gaussians, pipe, background)        # a DTU-style cloud
    fuse_views(cameras, gaussians, pipe, background, volume, consistency=dict(min_views=2))   # a filtered TSDF
    loss = loss + 0.05 * multi_view_geo_loss(depth_i, cameras[i], depth_j, cameras[j])        # PGSR's multi-view term
    loss = loss + 0.15 * multi_view_ncc_loss(depth_i, normal_i, cameras[i].original_image, cameras[i],
                                             depth_j, cameras[j].original_image, cameras[j], n_samples=102400)

The check is MVSNet's / COLMAP's: a reference pixel is taken into a source view at its depth, the source's depth is read
there (bilinear, only where all four neighbours hold depth), the result is taken back, and the pixel is consistent with
that source when it lands within ``pix_thresh`` pixels of where it started and within ``depth_thresh`` (relative) of its
own depth.  ``count`` is the number of sources a pixel is consistent with; ``fused`` the mean of its depth and the
round-trip depths where ``count >= min_views`` and 0 elsewhere.  Depth 0 means no depth, the pixel centre convention is
``tsdf.py``'s (``cx = (W - 1) / 2``), and the float32 order of operations is the header comment of ``csrc/mvs.hip``.  There
is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


def _view64(camera) -> np.ndarray:
    """The camera's float32 ``world_view_transform`` (row-vector convention) as float64 on the host."""
    M = camera.world_view_transform.detach().to(device="cpu", dtype=torch.float32).to(torch.float64).numpy()
    if M.shape != (4, 4):
        raise ValueError(f"world_view_transform must be 4 x 4, got {M.shape}")
    return M


def _focal(camera) -> Tuple[int, int, float, float]:
    H, W = int(camera.image_height), int(camera.image_width)
    if H <= 0 or W <= 0:
        raise ValueError("the camera has an empty image")
    return H, W, W / (2.0 * math.tan(float(camera.FoVx) * 0.5)), H / (2.0 * math.tan(float(camera.FoVy) * 0.5))


def _depth_map(depth, camera, dev, what: str) -> torch.Tensor:
    H, W = int(camera.image_height), int(camera.image_width)
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or (dev is not None and depth.device != dev) \
            or tuple(depth.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"{what} must be a float32 [{H},{W}] or [1,{H},{W}] tensor{'' if dev is None else f' on {dev}'}, "
                         f"got {getattr(depth, 'dtype', type(depth))} {tuple(getattr(depth, 'shape', ()))} on "
                         f"{getattr(depth, 'device', None)}")
    return depth.detach().contiguous()


def _thresholds(pix_thresh, depth_thresh, min_views) -> Tuple[float, float, int]:
    pix_thresh, depth_thresh = float(pix_thresh), float(depth_thresh)
    if not pix_thresh > 0.0 or not math.isfinite(pix_thresh):
        raise ValueError(f"pix_thresh must be positive and finite, got {pix_thresh}")
    if not depth_thresh > 0.0 or not math.isfinite(depth_thresh):
        raise ValueError(f"depth_thresh must be positive and finite, got {depth_thresh}")
    if isinstance(min_views, bool) or int(min_views) != min_views or min_views < 0:
        raise ValueError(f"min_views must be a non-negative integer, got {min_views!r}")
    return pix_thresh, depth_thresh, int(min_views)


def select_source_views(cameras, n_sources: int, max_angle_deg: float = 60.0) -> List[List[int]]:
    """For every view the indices of its source views: the other views whose forward direction is within
    ``max_angle_deg`` of its own, the ``n_sources`` of them with the nearest camera centres, nearest first, ties to the
    smaller index; fewer candidates give a shorter list.  Host, float64, from ``world_view_transform`` only: with
    ``V = world_view_transform.T = [R|t]`` the centre is ``-R^T t`` and the forward direction the third row of ``R``."""
    if isinstance(n_sources, bool) or int(n_sources) != n_sources or n_sources < 0:
        raise ValueError(f"n_sources must be a non-negative integer, got {n_sources!r}")
    max_angle_deg = float(max_angle_deg)
    if not 0.0 < max_angle_deg <= 180.0:
        raise ValueError(f"max_angle_deg must lie in (0, 180], got {max_angle_deg}")
    cameras = list(cameras)
    n = len(cameras)
    if n == 0:
        return []
    centres, forwards = np.zeros((n, 3)), np.zeros((n, 3))
    for i, cam in enumerate(cameras):
        V = _view64(cam).T
        R, t = V[:3, :3], V[:3, 3]
        centres[i] = -R.T @ t
        forwards[i] = R[2] / np.linalg.norm(R[2])
    out = []
    for i in range(n):
        angle = np.degrees(np.arccos(np.clip(forwards @ forwards[i], -1.0, 1.0)))
        dist = np.linalg.norm(centres - centres[i], axis=1)
        order = np.argsort(dist, kind="stable")                            # stable: ties keep the smaller index first
        out.append([int(j) for j in order if j != i and angle[j] <= max_angle_deg][:int(n_sources)])
    return out


def depth_consistency(depth: torch.Tensor, camera, src_depths: Sequence[torch.Tensor], src_cameras: Sequence, *,
                      pix_thresh: float = 1.0, depth_thresh: float = 0.01,
                      min_views: int = 2) -> Tuple[torch.Tensor, torch.Tensor]:
    """The consistency of one reference view with up to 64 source views, in one launch on the current stream ->
    ``(count uint8 [H,W], fused float32 [H,W])``.  ``depth`` float32 ``[H,W]`` or ``[1,H,W]`` on a ROCm GPU, 0 where there
    is none; ``camera``: anything with ``world_view_transform``, ``FoVx``, ``FoVy``, ``image_width``, ``image_height``;
    ``src_depths[k]`` the depth map of ``src_cameras[k]``, of that camera's size, which may differ from the reference's.
    ``count``: the number of sources a pixel is consistent with (module docstring), ``fused``: where ``count >=
    min_views`` the mean of the pixel's depth and its round-trip depths from the consistent sources, else 0.  Pixels
    without depth give 0, 0.  The two transforms per source, ``inv(V_ref) V_src`` and ``inv(V_src) V_ref``, are formed here in
    float64 and rounded once.  The table of sources is one small host-to-device copy; nothing is read back."""
    pix_thresh, depth_thresh, min_views = _thresholds(pix_thresh, depth_thresh, min_views)
    H, W, fx, fy = _focal(camera)
    dev = getattr(depth, "device", None)
    depth_c = _depth_map(depth, camera, None, "depth")
    src_depths, src_cameras = list(src_depths), list(src_cameras)
    if len(src_depths) != len(src_cameras):
        raise ValueError(f"{len(src_depths)} source depth maps for {len(src_cameras)} source cameras")
    S = len(src_cameras)
    if S > _lib.MVS_MAX_SOURCES:
        raise ValueError(f"at most {_lib.MVS_MAX_SOURCES} source views, got {S}")
    if H * W > 2 ** 28:
        raise ValueError(f"an image of {W} x {H} exceeds 2^28 pixels")
    M_ref = _view64(camera)
    inv_ref = np.linalg.inv(M_ref)
    table = (_lib.GsrMvsSource * max(S, 1))()
    keep = []
    for k, (sd, sc) in enumerate(zip(src_depths, src_cameras)):
        Hs, Ws, fxs, fys = _focal(sc)
        if Hs * Ws > 2 ** 28:
            raise ValueError(f"source {k}: an image of {Ws} x {Hs} exceeds 2^28 pixels")
        sd_c = _depth_map(sd, sc, dev, f"src_depths[{k}]")
        keep.append(sd_c)
        M_src = _view64(sc)
        row = table[k]
        row.depth, row.width, row.height, row.fx, row.fy = sd_c.data_ptr(), Ws, Hs, fxs, fys
        A = (inv_ref @ M_src).astype(np.float32).reshape(-1)
        B = (np.linalg.inv(M_src) @ M_ref).astype(np.float32).reshape(-1)
        for i in range(16):
            row.ref_to_src[i], row.src_to_ref[i] = float(A[i]), float(B[i])
    if not depth_c.is_cuda:
        raise _lib.GsrError("depth_consistency needs the depth maps on a ROCm GPU (no CPU path)")
    lib = _lib.load()
    count = torch.empty((H, W), dtype=torch.uint8, device=dev)
    fused = torch.empty((H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        table_dev = None
        if S > 0:
            table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.gsr_mvs_consistency(depth_c.data_ptr(), H, W, fx, fy,
                                           None if table_dev is None else table_dev.data_ptr(), S, pix_thresh,
                                           depth_thresh, min_views, count.data_ptr(), fused.data_ptr(), stream),
                   "gsr_mvs_consistency")
    return count, fused


def backproject_depth(depth: torch.Tensor, camera) -> torch.Tensor:
    """``depth`` float32 ``[H,W]`` or ``[1,H,W]`` on a ROCm GPU -> world points ``xyz`` float32 ``[H*W,3]`` in pixel order
    (row ``py * W + px``): the pixel's ray ``((px - cx) / fx, (py - cy) / fy, 1)`` times its depth, through the float64
    inverse of the view matrix rounded once to float32.  Rows of pixels without depth (0) are zeros; compact with a
    boolean index (``xyz[depth.reshape(-1) > 0]``).  One launch, nothing is read back."""
    H, W, fx, fy = _focal(camera)
    depth_c = _depth_map(depth, camera, None, "depth")
    if H * W > 2 ** 28:
        raise ValueError(f"an image of {W} x {H} exceeds 2^28 pixels")
    c2w = (C.c_float * 16)(*[float(v) for v in np.linalg.inv(_view64(camera)).astype(np.float32).reshape(-1)])
    if not depth_c.is_cuda:
        raise _lib.GsrError("backproject_depth needs the depth map on a ROCm GPU (no CPU path)")
    dev = depth_c.device
    xyz = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().gsr_depth_backproject(depth_c.data_ptr(), H, W, fx, fy, C.addressof(c2w), xyz.data_ptr(),
                                                     stream), "gsr_depth_backproject")
    return xyz


def consistency_options(consistency) -> dict:
    """The ``consistency`` argument of ``tsdf.fuse_views`` with its defaults filled in; ``ValueError`` for an unknown key."""
    options = dict(n_sources=4, min_views=2, pix_thresh=1.0, depth_thresh=0.01, max_angle_deg=60.0)
    unknown = set(consistency) - set(options)
    if unknown:
        raise ValueError(f"consistency has unknown keys {sorted(unknown)}: it takes {sorted(options)}")
    options.update(consistency)
    _thresholds(options["pix_thresh"], options["depth_thresh"], options["min_views"])
    return options


def filter_views(cameras, depths, *, n_sources: int, min_views: int, pix_thresh: float, depth_thresh: float,
                 max_angle_deg: float):
    """``depth_consistency`` of every view against its ``select_source_views`` -> a generator of ``(count, fused)`` in view
    order; ``depths[i]`` is the depth map of ``cameras[i]``."""
    sources = select_source_views(cameras, n_sources, max_angle_deg)
    for i, camera in enumerate(cameras):
        yield depth_consistency(depths[i], camera, [depths[j] for j in sources[i]], [cameras[j] for j in sources[i]],
                                pix_thresh=pix_thresh, depth_thresh=depth_thresh, min_views=min_views)


def fuse_depth_points(cameras, model, pipe, bg, *, n_sources: int = 4, min_views: int = 2, pix_thresh: float = 1.0,
                      depth_thresh: float = 0.01, alpha_min: float = 0.5, depth_ratio: float = 0.0,
                      max_angle_deg: float = 60.0, renderer=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The fused point cloud of a trained model, the product DTU-style evaluation is defined on -> ``(xyz float32 [N,3],
    rgb float32 [N,3])`` on the device.  Every view is rendered once under ``no_grad`` with ``renderer`` (default
    ``render``); its surface depth -- the expression ``tsdf.fuse_views`` integrates, ``alpha_min`` and ``depth_ratio``
    included -- and its colour stay on the device (``N_views H W (4 + 12)`` bytes).  Each view is filtered against its
    ``select_source_views(cameras, n_sources, max_angle_deg)``; its ``fused`` depth is back-projected and the pixels with
    ``fused > 0`` are gathered in pixel order, views concatenated in view order.  Duplicate points from overlapping views
    are kept.  One host synchronisation per view (the boolean index)."""
    from .tsdf import render_surface
    _thresholds(pix_thresh, depth_thresh, min_views)
    if not (isinstance(depth_ratio, (int, float)) and 0.0 <= depth_ratio <= 1.0):
        raise ValueError(f"depth_ratio must lie in [0, 1], got {depth_ratio!r}")
    if renderer is None:
        from .renderer import render as renderer
    cameras = list(cameras)
    xyz, rgb = [], []
    with torch.no_grad():
        depths, colors = [], []
        for camera in cameras:
            expected, pkg = render_surface(renderer, camera, model, pipe, bg, alpha_min, depth_ratio)
            depths.append(expected)
            colors.append(pkg["render"])
        filtered = filter_views(cameras, depths, n_sources=n_sources, min_views=min_views, pix_thresh=pix_thresh,
                                depth_thresh=depth_thresh, max_angle_deg=max_angle_deg)
        for camera, color, (_, fused) in zip(cameras, colors, filtered):
            valid = fused.reshape(-1) > 0
            xyz.append(backproject_depth(fused, camera)[valid])
            rgb.append(color.detach().reshape(3, -1).t()[valid].to(torch.float32))
    if not xyz:
        dev = bg.device if isinstance(bg, torch.Tensor) else None
        return torch.zeros((0, 3), device=dev), torch.zeros((0, 3), device=dev)
    return torch.cat(xyz), torch.cat(rgb)


# ---- the multi-view geometric loss (csrc/mvs_loss.hip) -------------------------------------------------
def _loss_map(depth, camera, dev, what: str) -> Tuple[int, int, float, float]:
    """``depth`` is a float32 ``[H,W]`` / ``[1,H,W]`` tensor of ``camera``'s size (on ``dev`` when given); it keeps its graph."""
    H, W, fx, fy = _focal(camera)
    if not isinstance(depth, torch.Tensor):
        raise TypeError(f"multi_view_geo_loss: {what} must be a torch.Tensor, got {type(depth).__name__}")
    if depth.dtype != torch.float32:
        raise TypeError(f"multi_view_geo_loss: {what} must be float32, got {depth.dtype}")
    if tuple(depth.shape) not in ((H, W), (1, H, W)):
        raise ValueError(f"multi_view_geo_loss: {what} must be [{H},{W}] or [1,{H},{W}] like its camera, got "
                         f"{tuple(depth.shape)}")
    if dev is not None and depth.device != dev:
        raise ValueError(f"multi_view_geo_loss: depth is on {dev}, {what} on {depth.device}")
    if H * W > 2 ** 28:
        raise ValueError(f"multi_view_geo_loss: {what} of {W} x {H} exceeds 2^28 pixels")
    if dev is None and ((W + 63) // 64) * ((H + 3) // 4) * 256 >= 2 ** 32:     # the reference: one lane per pixel of a 64 x 4 tile
        raise ValueError(f"multi_view_geo_loss: {what} of {W} x {H} needs a launch of 2^32 work-items or more (64 x 4 tiles)")
    return H, W, fx, fy


class _MultiViewGeo(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, src_depth, H, W, fx, fy, Hs, Ws, row, pix_max, depth_thresh, holder):
        lib = _lib.load()
        dev = depth.device
        need_ref, need_src = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dc, sc = depth.contiguous(), src_depth.contiguous()
        row.depth = sc.data_ptr()
        record = torch.empty(4, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.gsr_mvs_geo_loss_workspace_bytes(H, W), dtype=torch.uint8, device=dev)     # block partials
        g_ref = torch.empty((H, W), dtype=torch.float32, device=dev) if need_ref else None
        g_src = torch.empty((Hs, Ws), dtype=torch.float32, device=dev) if need_src else None
        with torch.cuda.device(dev):
            table = torch.frombuffer(bytearray(bytes(row)), dtype=torch.uint8).to(dev)      # the one small upload
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.gsr_mvs_geo_loss_fwd_bwd(dc.data_ptr(), H, W, fx, fy, table.data_ptr(), pix_max, depth_thresh,
                                                    record.data_ptr(), None if g_ref is None else g_ref.data_ptr(),
                                                    None if g_src is None else g_src.data_ptr(), Hs, Ws, ws.data_ptr(),
                                                    stream), "gsr_mvs_geo_loss_fwd_bwd")
        if need_ref or need_src:
            # 1 / max(n_valid, 1) from the record, on the device: the backward's one factor besides the upstream gradient
            inv_n = record.view(torch.int32)[1].clamp(min=1).to(torch.float32).reciprocal()
            ctx.save_for_backward(inv_n, *(g for g in (g_ref, g_src) if g is not None))
        ctx.shapes = (depth.shape, src_depth.shape)
        holder.append(record)
        return record[0]

    @staticmethod
    def backward(ctx, g):
        inv_n, *units = ctx.saved_tensors
        k = g.to(torch.float32) * inv_n                              # a 0-dim device tensor: never .item()
        units = iter(units)
        out = [(next(units) * k).view(shape) if need else None
               for shape, need in zip(ctx.shapes, ctx.needs_input_grad[:2])]
        return (*out, None, None, None, None, None, None, None, None, None, None)


def multi_view_geo_loss(depth: torch.Tensor, camera, src_depth: torch.Tensor, src_camera, *, pix_max: float = 1.0,
                        depth_thresh: Optional[float] = None, return_record: bool = False):
    """The multi-view geometric term of PGSR between a frame and one neighbouring frame, a 0-dim device tensor with
    gradients to ``depth`` and ``src_depth`` (each only where it requires one).  ``depth`` float32 ``[H,W]`` or ``[1,H,W]``
    on a ROCm GPU, 0 where there is none; ``src_depth`` the depth map of ``src_camera``, of that camera's size, which may
    differ; the cameras as ``depth_consistency`` reads them.  A reference pixel makes the round trip of
    ``depth_consistency`` (the same code, the same bits) and lands ``phi`` pixels from where it started; it is valid when
    every gate of that check passes, ``phi < pix_max`` (PGSR: 1) and, with ``depth_thresh`` given (default None: no depth
    test, as in PGSR), the round-trip depth is within ``depth_thresh`` (relative) of its own.  The loss is
    ``sum_valid exp(-phi) phi / max(n_valid, 1)`` with the weight ``exp(-phi)`` held constant; which pixels are valid is a
    decision and carries no gradient.  One kernel call computes the value and the unit gradients the inputs need; the
    backward multiplies them by ``upstream / max(n_valid, 1)`` on the device.  Nothing the kernel writes is read back.  The
    two ``world_view_transform``s are read on the host, where the float64 products are formed: for cameras that keep them
    on the GPU that is two 64-byte device-to-host copies, one synchronisation per call (as in ``depth_consistency``).  The value and the
    gradient to ``depth`` are the same bits from run to run; the gradient to ``src_depth`` is accumulated with float
    atomic adds and is NOT bit-reproducible.  No camera gradients.  No CPU path.
    return_record: also return the kernel's record, float32 ``[4]`` on the device: ``(loss, n_valid as uint32 bits, the
    raw sum, 0)`` (``record.view(torch.int32)[1]`` is the number of valid pixels)."""
    pix_max = float(pix_max)
    if not pix_max > 0.0 or not math.isfinite(pix_max):
        raise ValueError(f"multi_view_geo_loss: pix_max must be positive and finite, got {pix_max}")
    if depth_thresh is not None:
        depth_thresh = float(depth_thresh)
        if not depth_thresh > 0.0 or not math.isfinite(depth_thresh):
            raise ValueError(f"multi_view_geo_loss: depth_thresh must be None or positive and finite, got {depth_thresh}")
    H, W, fx, fy = _loss_map(depth, camera, None, "depth")
    Hs, Ws, fxs, fys = _loss_map(src_depth, src_camera, depth.device, "src_depth")
    M_ref, M_src = _view64(camera), _view64(src_camera)
    row = _lib.GsrMvsSource()
    row.width, row.height, row.fx, row.fy = Ws, Hs, fxs, fys       # the size grad_src is zeroed by is the row's own
    A = (np.linalg.inv(M_ref) @ M_src).astype(np.float32).reshape(-1)
    B = (np.linalg.inv(M_src) @ M_ref).astype(np.float32).reshape(-1)
    for i in range(16):
        row.ref_to_src[i], row.src_to_ref[i] = float(A[i]), float(B[i])
    if not depth.is_cuda:
        raise _lib.GsrError("multi_view_geo_loss needs the depth maps on a ROCm GPU (no CPU path)")
    holder = []
    loss = _MultiViewGeo.apply(depth, src_depth, H, W, fx, fy, Hs, Ws, row, pix_max,
                               0.0 if depth_thresh is None else depth_thresh, holder)
    return (loss, holder[0]) if return_record else loss


# ---- the multi-view photometric (NCC) loss (csrc/mvs_ncc.hip) -------------------------------------------
GRAY_WEIGHTS = (0.299, 0.587, 0.114)           # PGSR's (ITU-R BT.601)


def gray_image(image, device=None) -> torch.Tensor:
    """The grey image the NCC term compares -> float32 ``[H,W]``, contiguous, on ``device`` (default: the image's own).
    ``image``: a float32 ``[3,H,W]`` tensor (``(0.299 R + 0.587 G) + 0.114 B``, PGSR's weights), a ``[H,W]`` / ``[1,H,W]``
    tensor that is grey already, or a camera (anything with ``original_image``): its result is cached on the camera as
    ``_gray_image`` and reused while ``original_image`` is the same tensor and the device the same, so training converts
    (and, for cameras that keep their photographs on the host, uploads) each photograph once."""
    if not isinstance(image, torch.Tensor):
        photo = getattr(image, "original_image", None)
        if not isinstance(photo, torch.Tensor):
            raise TypeError(f"gray_image: expected a tensor or a camera with original_image, got {type(image).__name__}")
        device = photo.device if device is None else torch.device(device)
        cached = getattr(image, "_gray_image", None)
        if cached is not None and cached[0] is photo and cached[1].device == device:
            return cached[1]
        gray = gray_image(photo).to(device)
        try:
            image._gray_image = (photo, gray)
        except AttributeError:                 # a camera that takes no new attributes: converted every time
            pass
        return gray
    if image.dtype != torch.float32:
        raise TypeError(f"gray_image: the image must be float32, got {image.dtype}")
    if image.dim() == 3 and image.shape[0] == 3:
        r, g, b = image.detach().unbind(0)
        gray = ((GRAY_WEIGHTS[0] * r + GRAY_WEIGHTS[1] * g) + GRAY_WEIGHTS[2] * b).contiguous()
    elif image.dim() == 2 or (image.dim() == 3 and image.shape[0] == 1):
        gray = image.detach().reshape(image.shape[-2:]).contiguous()
    else:
        raise ValueError(f"gray_image: the image must be [3,H,W], [1,H,W] or [H,W], got {tuple(image.shape)}")
    return gray if device is None else gray.to(device)


def _ncc_image(image, camera, dev, what: str):
    """Checks ``image`` against ``camera`` -> the ``device`` argument of ``gray_image`` that puts its grey image on ``dev``:
    a tensor must be there already, a camera's photograph is taken there."""
    H, W = int(camera.image_height), int(camera.image_width)
    is_tensor = isinstance(image, torch.Tensor)
    photo = image if is_tensor else getattr(image, "original_image", None)
    if not isinstance(photo, torch.Tensor):
        raise TypeError(f"multi_view_ncc_loss: {what} must be a torch.Tensor or a camera, got {type(image).__name__}")
    if photo.dtype != torch.float32:
        raise TypeError(f"multi_view_ncc_loss: {what} must be float32, got {photo.dtype}")
    if tuple(photo.shape) not in ((3, H, W), (1, H, W), (H, W)):
        raise ValueError(f"multi_view_ncc_loss: {what} must be [3,{H},{W}], [1,{H},{W}] or [{H},{W}] like its camera, got "
                         f"{tuple(photo.shape)}")
    if is_tensor and photo.device != dev:
        raise ValueError(f"multi_view_ncc_loss: depth is on {dev}, {what} on {photo.device}")
    return None if is_tensor else dev


class _MultiViewNcc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, normal, gray, src_depth, src_gray, pixels, H, W, fx, fy, row, radius, pix_max, ncc_max,
                min_cos, holder):
        lib = _lib.load()
        dev = depth.device
        need_d, need_n = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dc, nc, sc = depth.contiguous(), normal.contiguous(), src_depth.contiguous()
        row.depth = sc.data_ptr()
        n_pixels = 0 if pixels is None else int(pixels.numel())
        record = torch.empty(4, dtype=torch.float32, device=dev)
        ws = torch.empty(lib.gsr_mvs_ncc_loss_workspace_bytes(H, W, n_pixels), dtype=torch.uint8, device=dev)
        g_d = torch.empty((H, W), dtype=torch.float32, device=dev) if need_d else None
        g_n = torch.empty((3, H, W), dtype=torch.float32, device=dev) if need_n else None
        with torch.cuda.device(dev):
            table = torch.frombuffer(bytearray(bytes(row)), dtype=torch.uint8).to(dev)      # the one small upload
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.gsr_mvs_ncc_loss_fwd_bwd(dc.data_ptr(), nc.data_ptr(), gray.data_ptr(), H, W, fx, fy,
                                                    table.data_ptr(), src_gray.data_ptr(),
                                                    None if pixels is None else pixels.data_ptr(), n_pixels, radius,
                                                    pix_max, ncc_max, min_cos, record.data_ptr(),
                                                    None if g_d is None else g_d.data_ptr(),
                                                    None if g_n is None else g_n.data_ptr(), ws.data_ptr(), stream),
                       "gsr_mvs_ncc_loss_fwd_bwd")
        if need_d or need_n:
            inv_n = record.view(torch.int32)[1].clamp(min=1).to(torch.float32).reciprocal()
            ctx.save_for_backward(inv_n, *(g for g in (g_d, g_n) if g is not None))
        ctx.shapes = (depth.shape, normal.shape)
        holder.append(record)
        return record[0]

    @staticmethod
    def backward(ctx, g):
        inv_n, *units = ctx.saved_tensors
        k = g.to(torch.float32) * inv_n                              # a 0-dim device tensor: never .item()
        units = iter(units)
        out = [(next(units) * k).view(shape) if need else None
               for shape, need in zip(ctx.shapes, ctx.needs_input_grad[:2])]
        return (*out, *([None] * 14))


def multi_view_ncc_loss(depth: torch.Tensor, normal: torch.Tensor, image, camera, src_depth: torch.Tensor, src_image,
                        src_camera, *, patch_radius: int = 3, pix_max: float = 1.0, ncc_max: float = 0.9,
                        min_cos: float = 0.05, n_samples: Optional[int] = None, generator=None, pixels=None,
                        return_record: bool = False):
    """The multi-view photometric term of PGSR between a frame and one neighbouring frame, a 0-dim device tensor with
    gradients to ``depth`` and ``normal`` (each only where it requires one).  ``depth`` float32 ``[H,W]`` / ``[1,H,W]`` on
    a ROCm GPU, 0 where there is none; ``normal`` float32 ``[3,H,W]``, the view-space map ``render(return_normals=True)``
    gives (camera-facing, any magnitude: the term is of degree 0 in it, so it needs no normalisation and no division by
    alpha); ``image`` / ``src_image`` the two photographs, float32 ``[3,H,W]`` (turned to grey by ``gray_image``), grey
    ``[H,W]`` / ``[1,H,W]``, or the cameras themselves (``gray_image`` caches on them); ``src_depth`` the depth map of
    ``src_camera``, of that camera's size, which may differ.  Per reference pixel the plane through its point with its
    normal carries the ``(2 patch_radius + 1)^2`` patch about it into the source image (read bilinearly);
    ``ncc = clamp(1 - cross^2 / (var_r var_s + 1e-8), 0, 2)`` over the patch's centred sums.  The pixel counts when its
    patch lies inside the reference, the plane is not grazing (``|N . r| >= min_cos |N| |r|``), the round trip of
    ``depth_consistency`` passes with ``phi < pix_max``, every tap lands inside the source in front of it, and
    ``ncc < ncc_max``.  The loss is ``sum_counted exp(-phi) ncc / max(n_counted, 1)`` with ``exp(-phi)`` held constant;
    which pixels count is a decision without gradient; the photographs and the source depth receive none.
    n_samples: evaluate ``n_samples`` distinct pixels drawn uniformly from all ``H W`` on the device
    (``torch.randperm(H W, device=, generator=)[:n_samples]``, nothing read back; at least ``H W``: every pixel); drawn
    pixels that fail a gate simply do not count.  PGSR draws from the valid pixels instead, which needs a host
    synchronisation to learn how many there are; here the share of drawn pixels that count is the share of valid ones.
    pixels: an int32 tensor of distinct flat indices ``py W + px`` on the device instead (entries outside ``[0, H W)``
    are skipped; duplicates are the caller's error).  Neither: every pixel.
    One kernel call computes the value and the unit gradients; the backward multiplies them by ``upstream /
    max(n_counted, 1)`` on the device.  Value and gradients are the same bits from run to run.  The two
    ``world_view_transform``s are read on the host as in ``multi_view_geo_loss``.  No camera gradients.  No CPU path.
    return_record: also return the kernel's record, float32 ``[4]``: ``(loss, n_counted as uint32 bits, raw sum, 0)``."""
    name = "multi_view_ncc_loss"
    if isinstance(patch_radius, bool) or not isinstance(patch_radius, int) or not 1 <= patch_radius <= 4:
        raise ValueError(f"{name}: patch_radius must be an integer in 1..4, got {patch_radius!r}")
    pix_max, ncc_max, min_cos = float(pix_max), float(ncc_max), float(min_cos)
    if not pix_max > 0.0 or not math.isfinite(pix_max):
        raise ValueError(f"{name}: pix_max must be positive and finite, got {pix_max}")
    if not 0.0 < ncc_max <= 2.0:
        raise ValueError(f"{name}: ncc_max must lie in (0, 2], got {ncc_max}")
    if not 0.0 <= min_cos < 1.0:
        raise ValueError(f"{name}: min_cos must lie in [0, 1), got {min_cos}")
    if n_samples is not None and pixels is not None:
        raise ValueError(f"{name}: give n_samples or pixels, not both")
    if n_samples is not None and (isinstance(n_samples, bool) or not isinstance(n_samples, int) or n_samples < 1):
        raise ValueError(f"{name}: n_samples must be a positive integer, got {n_samples!r}")
    try:
        H, W, fx, fy = _loss_map(depth, camera, None, "depth")
        dev = depth.device
        Hs, Ws, fxs, fys = _loss_map(src_depth, src_camera, dev, "src_depth")
    except (TypeError, ValueError) as e:
        raise type(e)(str(e).replace("multi_view_geo_loss", name)) from None
    if not isinstance(normal, torch.Tensor):
        raise TypeError(f"{name}: normal must be a torch.Tensor, got {type(normal).__name__}")
    if normal.dtype != torch.float32:
        raise TypeError(f"{name}: normal must be float32, got {normal.dtype}")
    if tuple(normal.shape) != (3, H, W):
        raise ValueError(f"{name}: normal must be [3,{H},{W}] like its camera, got {tuple(normal.shape)}")
    if normal.device != dev:
        raise ValueError(f"{name}: depth is on {dev}, normal on {normal.device}")
    gray_dev, src_gray_dev = _ncc_image(image, camera, dev, "image"), _ncc_image(src_image, src_camera, dev, "src_image")
    if pixels is not None:
        if not isinstance(pixels, torch.Tensor) or pixels.dtype != torch.int32 or pixels.dim() != 1:
            raise TypeError(f"{name}: pixels must be a 1-d int32 tensor, got {getattr(pixels, 'dtype', type(pixels).__name__)} "
                            f"{tuple(getattr(pixels, 'shape', ()))}")
        if not 1 <= pixels.numel() <= H * W:
            raise ValueError(f"{name}: pixels must hold 1..{H * W} indices, got {pixels.numel()}")
        if pixels.device != dev:
            raise ValueError(f"{name}: depth is on {dev}, pixels on {pixels.device}")
        pixels = pixels.contiguous()
    if generator is not None and n_samples is None:
        raise ValueError(f"{name}: generator is read only with n_samples")
    M_ref, M_src = _view64(camera), _view64(src_camera)
    row = _lib.GsrMvsSource()
    row.width, row.height, row.fx, row.fy = Ws, Hs, fxs, fys
    A = (np.linalg.inv(M_ref) @ M_src).astype(np.float32).reshape(-1)
    B = (np.linalg.inv(M_src) @ M_ref).astype(np.float32).reshape(-1)
    for i in range(16):
        row.ref_to_src[i], row.src_to_ref[i] = float(A[i]), float(B[i])
    if not depth.is_cuda:
        raise _lib.GsrError(f"{name} needs the maps and the images on a ROCm GPU (no CPU path)")
    gray, src_gray = gray_image(image, gray_dev), gray_image(src_image, src_gray_dev)
    if n_samples is not None and n_samples < H * W:
        pixels = torch.randperm(H * W, device=dev, generator=generator)[:n_samples].to(torch.int32)
    holder = []
    loss = _MultiViewNcc.apply(depth, normal, gray, src_depth, src_gray, pixels, H, W, fx, fy, row, patch_radius, pix_max,
                               ncc_max, min_cos, holder)
    return (loss, holder[0]) if return_record else loss


__all__ = ["select_source_views", "depth_consistency", "backproject_depth", "fuse_depth_points",
           "multi_view_geo_loss", "multi_view_ncc_loss", "gray_image"]
