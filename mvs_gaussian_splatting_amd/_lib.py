"""ctypes binding of ``libgsr_hip.so`` (the C ABI declared in ``include/gsr.h``).

There is no CPU fallback: if the shared library is missing or does not load, importing the
operator raises, and every call on a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSR_LIB_PATH (read once, at import): lets the A/B tuning tools (tools/ab_*.sh) point the binding at a candidate build
# instead of copying it over the in-tree library
LIB_PATH = os.environ.get("GSR_LIB_PATH") or os.path.join(_HERE, "libgsr_hip.so")

ABI_VERSION = 47


class GsrParams(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("M", C.c_int32), ("D", C.c_int32),
        ("width", C.c_int32), ("height", C.c_int32),
        ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("scale_modifier", C.c_float),
        ("prefiltered", C.c_int32), ("debug", C.c_int32),
        ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("opacities", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p),
        ("cov3D_precomp", C.c_void_p), ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p),
        ("campos", C.c_void_p), ("bg", C.c_void_p), ("profile", C.c_void_p),
        ("shs_rest", C.c_void_p), ("act_flags", C.c_int32), ("binning_mode", C.c_int32),
        ("counts_pinned", C.c_void_p), ("forward_only", C.c_int32), ("debug_flags", C.c_int32),
        ("visible_out", C.c_void_p), ("depth_span_lt24", C.c_int32),
    ]


class GsrGrads(C.Structure):
    _fields_ = [
        ("dL_dmeans3D", C.c_void_p), ("dL_dmeans2D", C.c_void_p), ("dL_dshs", C.c_void_p),
        ("dL_dcolors", C.c_void_p), ("dL_dopacities", C.c_void_p), ("dL_dscales", C.c_void_p),
        ("dL_drotations", C.c_void_p), ("dL_dcov3D", C.c_void_p), ("dL_dshs_rest", C.c_void_p),
        ("stats_xyz_gradient_accum", C.c_void_p), ("stats_denom", C.c_void_p), ("stats_max_radii2D", C.c_void_p),
        # camera gradients: all three NULL or all three set, then camera_ws (gsr_camera_grad_bytes(P)) is required
        ("dL_dviewmatrix", C.c_void_p), ("dL_dprojmatrix", C.c_void_p), ("dL_dcampos", C.c_void_p),
        ("camera_ws", C.c_void_p),
    ]


class GsrAuxFrame(C.Structure):
    """The saved state of a rendered frame, as the depth / alpha map entry points take it (include/gsr.h)."""
    _fields_ = [("P", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("binning_mode", C.c_int32),
                ("num_rendered", C.c_uint32), ("num_visible", C.c_uint32),
                ("geom_ws", C.c_void_p), ("bin_ws", C.c_void_p), ("img_ws", C.c_void_p), ("radii", C.c_void_p)]


class GsrAuxGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacities", "dL_dscales", "dL_drotations",
                                          "dL_dcov3D")]


class GsrTsdfVolume(C.Structure):
    """A dense TSDF volume as the fusion / extraction entry points take it (include/gsr.h; tsdf.py)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("origin", C.c_float * 3),
                ("voxel_size", C.c_float), ("sdf_trunc", C.c_float),
                ("tsdf", C.c_void_p), ("weight", C.c_void_p), ("color", C.c_void_p)]


class GsrTsdfContraction(C.Structure):
    """The scene contraction of a contracted TSDF volume (include/gsr.h, ABI v33; tsdf.ContractedTSDFVolume)."""
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("q_max", C.c_float)]


class GsrTsdfView(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float),
                ("weight", C.c_float), ("max_depth", C.c_float), ("max_weight", C.c_float),
                ("viewmatrix", C.c_void_p), ("depth", C.c_void_p), ("color", C.c_void_p)]


MVS_MAX_SOURCES = 64


class GsrMvsSource(C.Structure):
    """One row of the source table of ``gsr_mvs_consistency`` (include/gsr.h, ABI v34; mvs.py): 152 bytes."""
    _fields_ = [("depth", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float),
                ("ref_to_src", C.c_float * 16), ("src_to_ref", C.c_float * 16)]


CULL_MAX_VIEWS = 65535
DILATE_MAX_RADIUS = 1024


class GsrCullView(C.Structure):
    """One row of the view table of ``gsr_cull_view_counts`` (include/gsr.h, ABI v41; mesh.py): 96 bytes."""
    _fields_ = [("mask", C.c_void_p), ("depth", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("world_to_view", C.c_float * 16)]


FILTER3D_MAX_VIEWS = 65535
FILTER3D_MIP_SPLATTING, FILTER3D_PAPER = 0, 1


class GsrFilterView(C.Structure):
    """One row of the view table of ``gsr_filter3d_sample`` (include/gsr.h, ABI v47; filter3d.py): 80 bytes."""
    _fields_ = [("world_to_view", C.c_float * 16), ("fx", C.c_float), ("fy", C.c_float), ("width", C.c_int32),
                ("height", C.c_int32)]


# the mesh rasterizer (include/gsr.h, ABI v42; mesh.py): image limits, the two launch constants and the flags
RASTER_MAX_SIDE = 16384
RASTER_LANE_PIXELS, RASTER_DRAIN_WAVES = 16, 256
RASTER_CLEAR, RASTER_CULL_BACKFACES, RASTER_NO_LOAD_SKIP = 1, 2, 4


class GsrGrow(C.Structure):
    _fields_ = [("P", C.c_int32), ("G", C.c_int32), ("mode", C.c_int32), ("num_dirs", C.c_int32), ("n_rest", C.c_int32)] + [
        (n, C.c_void_p) for n in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation", "dirs_prob", "dirs",
                                  "conti_dirs", "grow_dist", "split_distance", "split_scale", "noise", "vidx", "src")]


class GsrGrowGrads(C.Structure):
    _fields_ = [("in_", C.c_void_p * 7), ("out", C.c_void_p * 7)] + [
        (n, C.c_void_p) for n in ("d_dirs_prob", "d_conti_dirs", "d_grow_dist", "d_split_distance", "d_split_scale")]


GROW_DIR, GROW_CONTINUOUS, GROW_DISTANCE, SPLIT_DISTANCE, SPLIT_SCALE = 1, 2, 4, 8, 16


class GsrDensifyFork(C.Structure):
    _fields_ = [("P", C.c_int32), ("mode", C.c_int32), ("num_dirs", C.c_int32)] + [
        (n, C.c_void_p) for n in ("xyz", "scaling", "rotation", "dirs_prob", "dirs", "conti_dirs", "grow_dist",
                                  "split_distance", "split_scale", "noise", "dir_noise")]


# the fork's densify_and_prune (gsr_densify_fork_*): branch / split bits next to the GROW_* / SPLIT_* flags, and the
# value policy of one tensor's roles, ROW_POLICY(selected originals, clones / grown copies, children)
DENSIFY_GROW, DENSIFY_SYMMETRIC = 32, 64
ROW_COPY, ROW_CONST, ROW_SKIP = 0, 1, 2


def ROW_POLICY(orig_sel: int, extra: int, child: int) -> int:
    return orig_sel | (extra << 2) | (child << 4)
ACT_SCALE_EXP, ACT_ROT_NORMALIZE, ACT_OPACITY_SIGMOID = 1, 2, 4
BINNING_TWO_LEVEL, BINNING_KEYS64, BINNING_TWO_LEVEL_CULLED = 0, 1, 2
DSSIM_ONE_MINUS_MEAN, DSSIM_CLAMPED_HALF = 0, 1
MASKED_LOSS_NORM_IMAGE, MASKED_LOSS_NORM_MASK = 0, 1
ALPHA_MASK_L1, ALPHA_MASK_BCE = 0, 1
DEBUG_NO_MINIBLOCK_CULL = 1
BILAGRID_STAGE_AUTO, BILAGRID_STAGE_CACHE, BILAGRID_STAGE_LDS = 0, 1, 2
# gsr_eval_image flags and the floats of its per-view record (l1, psnr, ssim, 3 x sum|d|, 3 x sum d^2, 3 x psnr_c)
EVAL_CLAMP_X, EVAL_CLAMP_GT, EVAL_SSIM, EVAL_PSNR_WHOLE, EVAL_U8_TRUNCATE = 1, 2, 4, 8, 16
EVAL_VIEW_FLOATS = 12


ADAM_MAX_TENSORS = 16


class GsrAdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("numel", C.c_int64)] + [
        (n, C.c_float) for n in ("lerp_weight", "beta2", "sq_weight", "bc2_sqrt", "eps", "step_size")]


class GsrAdamBatch(C.Structure):
    _fields_ = [("count", C.c_int32), ("reserved", C.c_int32), ("t", GsrAdamTensor * ADAM_MAX_TENSORS)]


ADAM_VIS_U8, ADAM_VIS_I32 = 0, 1


class GsrAdamRowsBatch(C.Structure):
    _fields_ = [("visibility", C.c_void_p), ("rows", C.c_int64), ("visibility_kind", C.c_int32), ("count", C.c_int32),
                ("t", GsrAdamTensor * ADAM_MAX_TENSORS)]


# name -> (restype, argtypes); every symbol include/gsr.h declares
SYMBOLS = {
    "gsr_abi_version": (C.c_int, []),
    "gsr_last_error": (C.c_char_p, []),
    "gsr_build_info": (C.c_char_p, []),
    "gsr_geom_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_image_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_binning_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32]),
    "gsr_backward_bytes": (C.c_size_t, [C.c_int32, C.c_uint32]),
    "gsr_camera_grad_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_forward_preprocess": (C.c_int, [C.POINTER(GsrParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "gsr_forward_render": (C.c_int, [C.POINTER(GsrParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "gsr_forward": (C.c_int, [C.POINTER(GsrParams), C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_event_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "gsr_event_destroy": (C.c_int, [C.c_void_p]),
    "gsr_event_wait": (C.c_int, [C.c_void_p]),
    "gsr_event_query": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "gsr_enable_markers": (C.c_int, [C.c_int32]),
    "gsr_backward": (C.c_int, [C.POINTER(GsrParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                               C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(GsrGrads), C.c_void_p]),
    # depth / inverse-depth / alpha maps of a rendered frame and their gradients (csrc/depth.hip; rasterizer.py)
    "gsr_aux_maps_forward": (C.c_int, [C.POINTER(GsrAuxFrame), C.c_void_p, C.c_void_p]),
    "gsr_aux_maps_backward_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_aux_maps_backward": (C.c_int, [C.POINTER(GsrParams), C.POINTER(GsrAuxFrame), C.c_void_p, C.c_void_p, C.c_size_t,
                                        C.POINTER(GsrAuxGrads), C.c_void_p]),
    # per-Gaussian feature rows [P,C] composited to [C,H,W] maps of a rendered frame, and their gradients (csrc/features.hip)
    "gsr_feature_maps_forward": (C.c_int, [C.POINTER(GsrAuxFrame), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gsr_feature_maps_backward_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_feature_maps_backward": (C.c_int, [C.POINTER(GsrParams), C.POINTER(GsrAuxFrame), C.c_void_p, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(GsrAuxGrads), C.c_void_p]),
    # depth-distortion map [1,H,W] of a rendered frame, its per-pixel state [2,H,W] and its gradients (csrc/distortion.hip)
    "gsr_abs_grad_backward": (C.c_int, [C.POINTER(GsrParams), C.POINTER(GsrAuxFrame), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_distortion_forward": (C.c_int, [C.POINTER(GsrAuxFrame), C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "gsr_distortion_backward_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_distortion_backward": (C.c_int, [C.POINTER(GsrParams), C.POINTER(GsrAuxFrame), C.c_int32, C.c_float, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(GsrAuxGrads),
                                          C.c_void_p]),
    # median-depth map [1,H,W], Gaussian id map [H,W] (int32) and per-pixel state [H,W] (uint32) of a rendered frame, and
    # the map's gradient for means3D (csrc/median.hip)
    "gsr_median_depth_forward": (C.c_int, [C.POINTER(GsrAuxFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_median_depth_backward_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_median_depth_backward": (C.c_int, [C.POINTER(GsrParams), C.POINTER(GsrAuxFrame), C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    # per-Gaussian contribution statistics of a rendered frame, added into int64 [P,3] (csrc/contribution.hip)
    "gsr_contribution_accumulate": (C.c_int, [C.POINTER(GsrAuxFrame), C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_mark_visible": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_sort_scratch_bytes": (C.c_size_t, [C.c_uint32]),
    "gsr_sort_pairs_u64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    # the 32-bit-key sorts of the two-level binning, callable on their own (tests/test_gpu_sort.py)
    "gsr_sort_pairs_u32": (C.c_int, [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.POINTER(C.c_int32)]),
    "gsr_sort_extra_pass_u32": (C.c_int, [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                          C.c_void_p]),
    "gsr_sort_tile_runs_u32": (C.c_int, [C.c_void_p] * 4 + [C.c_uint32, C.c_void_p, C.c_int32, C.c_uint32] +
                               [C.c_void_p] * 4 + [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "gsr_debug_read_geom": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 9),
    "gsr_debug_read_binning": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_debug_read_counts": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_void_p]),
    "gsr_debug_read_image": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "gsr_l1_loss_workspace_bytes": (C.c_size_t, []),
    "gsr_l1_loss_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "gsr_debug_render_stats": (C.c_int, [C.POINTER(GsrParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_l1_dssim_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "gsr_l1_dssim_loss_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # per-view evaluation (metrics.py): L1 / PSNR / SSIM + 8-bit image in one pass, accumulated on the device
    "gsr_eval_workspace_bytes": (C.c_size_t, [C.c_int32] * 4),
    "gsr_eval_image": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 5),
    "gsr_image_to_u8": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p, C.c_void_p]),
    "gsr_splat2d_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "gsr_splat2d_forward": (C.c_int, [C.c_int32] * 4 + [C.c_void_p] * 7 + [C.c_size_t, C.c_void_p,
                                      C.POINTER(C.c_int32), C.c_void_p]),
    "gsr_splat2d_backward": (C.c_int, [C.c_int32] * 4 + [C.c_void_p] * 5 + [C.c_size_t] + [C.c_void_p] * 7),
    "gsr_knn3_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_dist2_knn3": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gsr_densify_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_densify_plan": (C.c_int, [C.c_int32] + [C.c_void_p] * 4 + [C.c_float] * 4 + [C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_uint32), C.c_void_p]),
    "gsr_densify_stats_abs": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_densify_plan_abs": (C.c_int, [C.c_int32] + [C.c_void_p] * 5 + [C.c_float] * 5 + [C.c_void_p, C.c_size_t,
                                       C.POINTER(C.c_uint32), C.c_void_p]),
    "gsr_densify_gather_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_int32,
                                          C.c_void_p, C.c_void_p]),
    "gsr_densify_split_children": (C.c_int, [C.c_int32] + [C.c_void_p] * 5 + [C.POINTER(C.c_uint32), C.c_void_p,
                                             C.c_void_p, C.c_void_p]),
    # scene/gaussian_model.py:751-773, the fork's branches (clone + split :509-610, grow :612-749): include/gsr.h
    "gsr_densify_fork_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_densify_fork_plan": (C.c_int, [C.c_int32] + [C.c_void_p] * 5 + [C.c_float] * 4 + [C.c_void_p, C.c_size_t,
                                        C.POINTER(C.c_uint32), C.c_void_p]),
    "gsr_densify_fork_gather_rows": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                               C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    "gsr_densify_fork_rows": (C.c_int, [C.POINTER(GsrDensifyFork), C.c_void_p, C.POINTER(C.c_uint32)] +
                              [C.c_void_p] * 4),
    "gsr_grow_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_grow_plan": (C.c_int, [C.c_int32] + [C.c_void_p] * 3 + [C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_size_t]
                      + [C.c_void_p] * 3 + [C.POINTER(C.c_uint32), C.c_void_p]),
    "gsr_grow_expand": (C.c_int, [C.POINTER(GsrGrow)] + [C.c_void_p] * 7),
    "gsr_grow_fold": (C.c_int, [C.POINTER(GsrGrow), C.POINTER(GsrGrowGrads), C.c_void_p]),
    "gsr_profile_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "gsr_profile_destroy": (C.c_int, [C.c_void_p]),
    "gsr_profile_collect": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "gsr_stage_name": (C.c_char_p, [C.c_int32]),
    "gsr_densify_stats": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    # torch.optim.Adam's foreach step over up to ADAM_MAX_TENSORS tensors in one launch (optim.py)
    "gsr_adam_step": (C.c_int, [C.POINTER(GsrAdamBatch), C.c_void_p]),
    # the same step for the rows a visibility array marks (optim.SparseGaussianAdam)
    "gsr_adam_step_rows": (C.c_int, [C.POINTER(GsrAdamRowsBatch), C.c_void_p]),
    # the opacity sparsity term of train.py:102-106 and the in-place reset_opacity (csrc/model.hip; losses.py, model.py)
    "gsr_opacity_sparsity_workspace_bytes": (C.c_size_t, []),
    "gsr_opacity_sparsity_fwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "gsr_opacity_sparsity_bwd": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "gsr_reset_opacity": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    # load-time image ingest on uint8 HWC images (csrc/image.hip; image_ingest.py)
    "gsr_image_composite_u8": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                         C.c_void_p, C.c_void_p]),
    "gsr_image_resize_u8": (C.c_int, [C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_void_p, C.c_int32] * 2 +
                            [C.c_void_p] * 3),
    "gsr_image_to_float_chw": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    # per-image exposure compensation: the 3x4 colour affine on the rendered image (csrc/exposure.hip; exposure.py)
    "gsr_exposure_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_exposure_apply_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gsr_exposure_apply_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 4),
    # MCMC densification on the raw model tensors: noise, priors, weighted sampler, relocation (csrc/mcmc.hip; mcmc.py)
    "gsr_mcmc_noise": (C.c_int, [C.c_int64] + [C.c_void_p] * 5 + [C.c_float, C.c_void_p]),
    "gsr_mcmc_reg_workspace_bytes": (C.c_size_t, []),
    "gsr_mcmc_reg_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "gsr_mcmc_reg_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 5),
    "gsr_mcmc_sample_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_mcmc_sample": (C.c_int, [C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "gsr_mcmc_relocation": (C.c_int, [C.c_int64] + [C.c_void_p] * 7),
    # depth-map fusion into a dense TSDF volume and marching-tetrahedra extraction (csrc/tsdf.hip; tsdf.py)
    "gsr_tsdf_integrate": (C.c_int, [C.POINTER(GsrTsdfVolume), C.POINTER(GsrTsdfView), C.c_void_p]),
    "gsr_tsdf_mesh_count": (C.c_int, [C.POINTER(GsrTsdfVolume), C.c_float] + [C.c_void_p] * 4),
    "gsr_tsdf_mesh_emit": (C.c_int, [C.POINTER(GsrTsdfVolume)] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64] +
                           [C.c_void_p] * 4),
    # the same on a volume in contracted space, and its vertices back to world space (csrc/tsdf.hip; tsdf.py)
    "gsr_tsdf_integrate_contracted": (C.c_int, [C.POINTER(GsrTsdfVolume), C.POINTER(GsrTsdfContraction),
                                                C.POINTER(GsrTsdfView), C.c_void_p]),
    "gsr_tsdf_uncontract_points": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(GsrTsdfContraction), C.c_void_p]),
    # depth-normal consistency loss of a rendered frame, value and unit gradients (csrc/normal_consistency.hip)
    "gsr_normal_consistency_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_normal_consistency_fwd_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_float] * 3 + [C.c_void_p] * 7),
    # connected components of an indexed triangle mesh (lock-free union-find) and compaction (csrc/mesh.hip; mesh.py)
    "gsr_mesh_cc_init": (C.c_int, [C.c_int64] + [C.c_void_p] * 3),
    "gsr_mesh_cc_hook_faces": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "gsr_mesh_edge_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "gsr_mesh_cc_hook_runs": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    "gsr_mesh_cc_flatten": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p]),
    "gsr_mesh_cc_mark": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 5),
    "gsr_mesh_cc_label": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 3),
    "gsr_mesh_mark_vertices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 3),
    "gsr_mesh_compact": (C.c_int, [C.c_void_p] * 7 + [C.c_int64] * 4 + [C.c_void_p] * 5),
    # cross-set nearest point on the Morton-box index of distCUDA2 (csrc/nearest.hip; geometry_eval.py)
    "gsr_nn_index_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_nn_build": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "gsr_nn_query_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_nn_query": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_size_t, C.c_void_p]),
    # point-to-point ICP between two nearest-point queries: transform by a float64 3x4, the 18 sums of the accepted pairs
    # (csrc/icp.hip; geometry_eval.icp_step); matrix and pivots are host arrays
    "gsr_icp_transform": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_icp_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_icp_accumulate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    # k-means vector quantisation: code norms, assignment on the matrix cores (and its vector-ALU cross-check for D <= 4),
    # atomic-free centre update (csrc/kmeans.hip; compress.py)
    "gsr_kmeans_code_norms": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gsr_kmeans_assign": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "gsr_kmeans_assign_valu": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "gsr_kmeans_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # depth-prior loss of a rendered inverse-depth map, value and unit gradient (csrc/depth_prior.hip; depth_prior.py)
    "gsr_depth_prior_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_depth_prior_fwd_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_double] * 2 + [C.c_void_p] * 3 +
                                [C.c_size_t, C.c_void_p]),
    # training under a per-image mask: fused masked L1 + D-SSIM and the alpha-versus-mask term, value and unit gradient
    # (csrc/masked_loss.hip; masked_loss.py)
    "gsr_masked_l1_dssim_workspace_bytes": (C.c_size_t, [C.c_int32] * 3),
    "gsr_masked_l1_dssim_loss_fwd_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_double, C.c_int32] +
                                         [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    "gsr_alpha_mask_workspace_bytes": (C.c_size_t, [C.c_int32] * 2),
    "gsr_alpha_mask_loss_fwd_bwd": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p] * 3 + [C.c_size_t, C.c_void_p]),
    # multi-view geometric consistency of depth maps and back-projection to points (csrc/mvs.hip; mvs.py)
    "gsr_mvs_consistency": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_int32,
                                      C.c_float, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_depth_backproject": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    # multi-view geometric consistency loss of a (reference, source) pair, value and unit gradients (csrc/mvs_loss.hip)
    "gsr_mvs_geo_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_mvs_geo_loss_fwd_bwd": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.c_float,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p]),
    # multi-view photometric (NCC) loss of a (reference, source) pair, value and unit gradients (csrc/mvs_ncc.hip)
    "gsr_mvs_ncc_loss_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "gsr_mvs_ncc_loss_fwd_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                           C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # per-Gaussian planes (view-space normal, camera-to-plane distance) and their gradients (csrc/planes.hip;
    # features.gaussian_planes); viewmatrix and campos are host arrays
    "gsr_gaussian_planes_fwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 4),
    "gsr_gaussian_planes_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 6),
    # PGSR's unbiased depth of a rendered frame, value and unit gradients, and their scaling by the upstream map
    # (csrc/plane_depth.hip; surface.plane_depth)
    "gsr_plane_depth_fwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_float] * 4 + [C.c_void_p] * 4),
    "gsr_plane_depth_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 3),
    # per-image bilateral grids: trilinear slice of a grid of 3x4 colour affines, its gradients and the TV term
    # (csrc/bilagrid.hip; bilagrid.py)
    "gsr_bilagrid_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "gsr_bilagrid_slice_fwd": (C.c_int, [C.c_void_p] * 2 + [C.c_int32] * 6 + [C.c_void_p] * 2),
    "gsr_bilagrid_slice_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 6 + [C.c_void_p] * 4),
    "gsr_bilagrid_tv_fwd_bwd": (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 4),
    # mesh simplification by vertex clustering on a uniform grid: the kernels around the sorts and scans of
    # mesh.simplify_mesh (csrc/mesh_simplify.hip)
    "gsr_simplify_default_origin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double] + [C.c_void_p] * 3),
    "gsr_simplify_cell_keys": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double] + [C.c_void_p] * 3),
    "gsr_simplify_run_heads": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "gsr_simplify_reduce": (C.c_int, [C.c_void_p] * 5 + [C.c_int64] * 2 + [C.c_void_p] * 6),
    "gsr_simplify_face_keys": (C.c_int, [C.c_void_p] * 2 + [C.c_int64] * 3 + [C.c_void_p] * 6),
    "gsr_simplify_face_unique": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3),
    "gsr_simplify_vertex_map": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] * 2 + [C.c_void_p] * 2),
    # culling a mesh by the views that saw it: per-vertex view counts, the face rule and mask dilation
    # (csrc/mesh_cull.hip; mesh.vertex_view_counts, mesh.cull_mesh_by_views, mesh.dilate_mask)
    "gsr_cull_view_counts": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32] +
                             [C.c_void_p] * 3),
    "gsr_cull_face_keep": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 3),
    "gsr_mask_dilate": (C.c_int, [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 3),
    # rasterizing a mesh from a camera: z-buffer of (depth, face) keys, its resolve, per-face view counts
    # (csrc/mesh_raster.hip; mesh.rasterize_mesh, mesh.face_view_counts, mesh.cull_invisible_faces)
    "gsr_raster_queue_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_raster_view": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(GsrCullView), C.c_float, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gsr_raster_resolve": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_raster_count_faces": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    # Mip-Splatting's 3D smoothing filter: the sampling pass over the training views, its finish, and the fused
    # application to raw scales and opacities with its gradient (csrc/filter3d.hip; filter3d.py)
    "gsr_filter3d_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_filter3d_sample": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32] +
                            [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "gsr_filter3d_finish": (C.c_int, [C.c_int64] + [C.c_void_p] * 3 + [C.c_int32, C.c_float, C.c_float, C.c_void_p,
                                                                       C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_filter3d_apply": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 3),
    "gsr_filter3d_apply_bwd": (C.c_int, [C.c_void_p] * 3 + [C.c_int64] + [C.c_void_p] * 5),
}

_lib = None
_lock = threading.Lock()


class GsrError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load (once) and type the library.  Raises ``GsrError`` if it is missing: build it with
    ``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C mvs_gaussian_splatting_amd/csrc``."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GsrError(f"HIP extension not built: {LIB_PATH} is missing (no CPU fallback exists); "
                           f"run `make -C {os.path.join(_HERE, 'csrc')}`")
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the machine
            raise GsrError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.gsr_abi_version() != ABI_VERSION:
            raise GsrError(f"ABI mismatch: library {lib.gsr_abi_version()} != binding {ABI_VERSION}")
        _lib = lib
    return _lib


def enable_markers(on: bool = True) -> None:
    """roctx ranges ("gsr:<stage>") around every stage, for ``rocprofv3 --marker-trace``; off by default."""
    check(load().gsr_enable_markers(1 if on else 0), "gsr_enable_markers")


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gsr_last_error().decode("utf-8", "replace")
        raise GsrError(f"{what} failed (code {rc}): {msg}")


STAGE_COUNT = 8
_active_profile = threading.local()


class StageProfile:
    """HIP-event stage timers of the C library (``gsr_profile_*``).  While active (``with prof:``) every
    rasterizer call made from this thread records an event pair around each stage on its stream."""

    def __init__(self):
        self._h = C.c_void_p()
        check(load().gsr_profile_create(C.byref(self._h)), "gsr_profile_create")

    def __enter__(self):
        _active_profile.obj = self
        return self

    def __exit__(self, *exc):
        _active_profile.obj = None

    def handle(self):
        """The native handle, or None once closed (a backward that outlives close() then runs untimed)."""
        return self._h if self._h else None

    def collect(self):
        """-> {stage name: (total ms, intervals)}; blocks on the recorded events and clears them."""
        lib = load()
        ms = (C.c_double * STAGE_COUNT)()
        cnt = (C.c_uint32 * STAGE_COUNT)()
        check(lib.gsr_profile_collect(self._h, ms, cnt), "gsr_profile_collect")
        return {lib.gsr_stage_name(i).decode(): (ms[i], cnt[i]) for i in range(STAGE_COUNT)}

    def close(self):
        if self._h:
            load().gsr_profile_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def active_profile():
    """The StageProfile active on this thread (autograd contexts hold on to the object, not the raw handle, so
    that the handle cannot be freed under a retained graph's backward)."""
    return getattr(_active_profile, "obj", None)


def active_profile_handle():
    obj = active_profile()
    return obj.handle() if obj is not None else None
