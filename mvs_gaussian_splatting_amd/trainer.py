"""One iteration of the reference's training loop (``train.py:72-142``) from this package's drop-ins, its
``OptimizationParams`` defaults (``arguments/__init__.py:82-108``) and the checkpoint file of ``train.py:41,159``.

    opt, pipe = OptimizationParams(), PipelineParams()
    gaussians.training_setup(opt)
    for iteration in range(first_iter + 1, opt.iterations + 1):
        loss = training_iteration(gaussians, camera, opt, pipe, background, iteration, dataset=dataset,
                                  cameras_extent=scene.cameras_extent)

``training_iteration`` reads nothing back from the device: the loss it returns is a device tensor and the caller
decides when to log it.  (Densification itself reads its row counts, as the reference's does.)
"""
from __future__ import annotations

import math

import torch

from .bilagrid import bilateral_grid_tv_loss, slice_bilateral_grid
from .densify import densify_and_prune, is_fork
from .depth_prior import depth_prior_loss
from .losses import add_densification_stats, l1_dssim_loss, opacity_sparsity_loss
from .masked_loss import alpha_mask_loss, masked_l1_dssim_loss
from .mcmc import add_new_gs, inject_noise, mcmc_regularizer, relocate_gs
from .mvs import multi_view_geo_loss, multi_view_ncc_loss
from .normal_consistency import normal_consistency_loss
from .optim import expon_lr_func
from .renderer import render
from .surface import blend_plane_depth, surface_depth
from .synthetic import PipelineParams  # noqa: F401  (the two parameter classes live side by side)


class OptimizationParams:
    """``arguments/__init__.py:82-108`` defaults."""
    iterations = 30_000
    position_lr_init = 0.00016
    position_lr_final = 0.0000016
    position_lr_delay_mult = 0.01
    position_lr_max_steps = 30_000
    feature_lr = 0.0025
    opacity_lr = 0.05
    scaling_lr = 0.005
    rotation_lr = 0.001
    percent_dense = 0.01
    growdirs_lr = 0.005
    growdistance_lr = 0.001
    lambda_dssim = 0.2
    densification_interval = 100
    opacity_reset_interval = 3000
    densify_from_iter = 500
    densify_until_iter = 15_000
    densify_grad_threshold = 0.0002
    min_opacity = 0.005
    random_background = False
    opacitysparse = 0.0
    splitdistance_lr = 0.005
    splitscale_lr = 0.005
    # this build's: "default" (optim.Adam, every row every step) or "sparse_adam" (optim.SparseGaussianAdam: the rows the
    # frame saw, as upstream 3DGS names its option)
    optimizer_type = "default"
    # upstream 3DGS's per-image exposure compensation (training_iteration(train_exposure=True)): its Adam's schedule
    exposure_lr_init = 0.01
    exposure_lr_final = 0.001
    exposure_lr_delay_steps = 0
    exposure_lr_delay_mult = 0.0
    # densification strategy: "default" (the reference's / the fork's densify_and_prune) or "mcmc" (mcmc.py: a budget of
    # cap_max Gaussians, relocation, 5 % growth, position noise at noise_lr * lr_xyz, L1 priors on opacity and scale;
    # opacity_reg / scale_reg are read only under "mcmc")
    strategy = "default"
    cap_max = -1
    noise_lr = 5e5
    opacity_reg = 0.01
    scale_reg = 0.01
    # depth-normal consistency (normal_consistency.py; 2DGS uses 0.05 from iteration 7000): 0 leaves the iteration as it is
    lambda_normal = 0.0
    normal_from_iter = 7000
    # which depth the normal term differentiates: (1 - depth_ratio) expected + depth_ratio median (2DGS: 0 for unbounded
    # scenes, 1 for bounded ones); read only while the normal term is on; 0 leaves the iteration as it is
    depth_ratio = 0.0
    # depth distortion (the rasterizer's distortion map; 2DGS uses 100 to 1000 from iteration 3000): 0 leaves the iteration
    # as it is
    lambda_dist = 0.0
    dist_from_iter = 3000
    # multi-view geometric consistency (mvs.multi_view_geo_loss; PGSR's multi-view term, from iteration 7000 there):
    # the forward-backward reprojection error between the frame and training_iteration(source_camera=), valid below
    # multi_view_pix_max pixels; reads depth_ratio for the surface depth of both frames; 0 leaves the iteration as it is
    lambda_multi_view_geo = 0.0
    multi_view_from_iter = 7000
    multi_view_pix_max = 1.0
    # multi-view photometric consistency (mvs.multi_view_ncc_loss; PGSR's NCC term, weight 0.15 there): one minus the
    # patch NCC between the frame's photograph and source_camera's under the homography of the rendered plane, at
    # multi_view_ncc_samples pixels drawn per iteration; shares multi_view_from_iter and multi_view_pix_max with the
    # geometric term; 0 leaves the iteration as it is, whatever the other three fields say
    lambda_multi_view_ncc = 0.0
    multi_view_ncc_samples = 102400
    multi_view_patch_radius = 3
    multi_view_ncc_max = 0.9
    # PGSR's unbiased depth (render(return_plane_depth=True); surface.plane_depth): while the normal term or a multi-view
    # term is on, the surface they see is the ray-plane depth of the blended plane instead of the expected depth; read
    # only then; False leaves the iteration as it is
    unbiased_depth = False
    # per-image bilateral grids (bilagrid.py; training_iteration(bilateral_grids=)): their Adam's exponential schedule
    # over `iterations` steps and the weight of their total-variation term; read only with grids
    bilateral_grid_lr_init = 2e-3
    bilateral_grid_lr_final = 2e-5
    lambda_tv = 10.0
    # absolute-gradient densification (AbsGS; PGSR's densify_abs_grad_threshold): the frame is rendered with
    # render(abs_grad=True) and a large Gaussian is also split when its accumulated absolute gradient reaches the second
    # threshold; read only under strategy "default"; False leaves the iteration as it is
    abs_grad = False
    densify_abs_grad_threshold = 0.0008
    # upstream 3DGS's depth-prior regularisation (depth_prior.py; scene.Camera.invdepthmap): the weight decays from init to
    # final over `iterations` (optim.expon_lr_func) and the term is `depth_prior_mode`, "l1" (upstream's, under the affine of
    # depth_params.json), "aligned_l1" or "pearson"; read only on a camera that carries a reliable prior
    depth_l1_weight_init = 1.0
    depth_l1_weight_final = 0.01
    depth_prior_mode = "l1"
    # training masks (masked_loss.py; scene.Camera.alpha_mask), read only on a camera that carries one:
    # mask_photometric puts the colour loss under the mask, normalised by the image ("image": upstream 3DGS's and gsplat's
    # rule) or by the mask's area ("mask"); lambda_alpha_mask > 0 adds that weight times the silhouette term of the
    # rendered opacity against the mask, alpha_mask_mode "bce" or "l1" (2DGS / NeuS / PGSR object captures)
    mask_photometric = True
    mask_normalize = "image"
    lambda_alpha_mask = 0.0
    alpha_mask_mode = "bce"
    # Mip-Splatting's 3D smoothing filter (filter3d.py; training_iteration(filter_cameras=)): the model is
    # rendered through model.filter_3D, recomputed from the training cameras after every densification step, at iteration 1
    # and every filter_3d_interval iterations once densification has ended; filter_3d_rule "mip_splatting" (the published
    # code's width) or "paper"; False leaves the iteration as it is
    filter_3d = False
    filter_3d_interval = 100
    filter_3d_rule = "mip_splatting"
    filter_3d_variance = 0.2

    def __init__(self, **overrides):
        for k, v in overrides.items():
            if not hasattr(type(self), k):
                raise TypeError(f"OptimizationParams has no field {k!r}")
            setattr(self, k, v)


def schedule(opt, iteration: int, white_background: bool = False) -> dict:
    """Which steps of ``train.py:72-142`` fire at ``iteration`` -- host arithmetic only:
    ``sh_up`` (:75), ``stats`` (:127), ``densify`` and its ``size_threshold`` (:132-133), ``reset`` (:136), ``step`` (:140)."""
    stats = iteration < opt.densify_until_iter
    densify = stats and iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0
    reset = stats and (iteration % opt.opacity_reset_interval == 0 or
                       (white_background and iteration == opt.densify_from_iter))
    return {"sh_up": iteration % 1000 == 0, "stats": stats, "densify": densify,
            "size_threshold": 20 if iteration > opt.opacity_reset_interval else None,
            "reset": reset, "step": iteration < opt.iterations}


def depth_prior_weight(opt, iteration: int) -> float:
    """The weight of the depth-prior term at ``iteration``: upstream's ``get_expon_lr_func(depth_l1_weight_init,
    depth_l1_weight_final, max_steps=iterations)`` -- ``init`` at iteration 0, ``final`` at ``opt.iterations``, log-linear
    in between; 0 when both are 0."""
    return float(expon_lr_func(float(getattr(opt, "depth_l1_weight_init", 0.0)),
                               float(getattr(opt, "depth_l1_weight_final", 0.0)),
                               max_steps=int(opt.iterations))(iteration))


def training_iteration(model, camera, opt, pipe, background, iteration, *, dataset=None, cameras_extent,
                       first_reset=None, gt_image=None, densify_kwargs=None, pose_optimizer=None, depth_loss=None,
                       train_exposure=False, mcmc_kwargs=None, source_camera=None, bilateral_grids=None,
                       filter_cameras=None):
    """``train.py:72-142`` for one camera, in the reference's order: learning rate, SH degree, background, ``render``
    with the fork's keyword arguments, L1 + D-SSIM against ``camera.original_image``, the opacity sparsity term
    (``opt.opacitysparse``), ``backward``; then, without gradients, the densification statistics, ``densify_and_prune``,
    ``reset_opacity``, and the optimizer step (with ``opt.optimizer_type == "sparse_adam"``: of the rows the frame saw,
    ``SparseGaussianAdam.step(visibility)``).  Returns the loss, a 0-dim device tensor.

    dataset: the reference's model namespace (``grow_dir``, ``continous_dir``, ``grow_distance``, the learned-split
    switches, ``white_background``); None is a plain model on a black background.
    first_reset: whether the extra opacity reset at ``densify_from_iter`` runs (``train.py:136``); default
    ``dataset.white_background``.
    gt_image: the target instead of ``camera.original_image``.  densify_kwargs: passed on to ``densify_and_prune``
    (``noise``, ``dir_noise``, ``spatial_order``).
    pose_optimizer: an optimizer over the parameters of ``camera`` when that is a ``scene.PoseCamera`` (the backward
    leaves dL/dpose in them); it is stepped and zeroed where the model's optimizer is.  None: the camera is not refined.
    depth_loss: None, or ``(target, weight)`` with ``target [1,H,W]`` an inverse-depth map (from multi-view stereo, say):
    the frame is rendered with ``return_depth=True`` and ``weight * mean|invdepth - target|`` joins the loss (plain torch
    ops on the map; the map and its gradients are the HIP path's).  Not on a frame of the open grow / learned-split
    branch.
    train_exposure: the frame is rendered with ``use_trained_exp=True`` -- the loss sees the image after the camera's
    3x4 exposure (``model.setup_exposures`` before ``training_setup``) -- and ``model.exposure_optimizer`` is stepped and
    zeroed where the model's optimizer is.
    mcmc_kwargs: under ``opt.strategy == "mcmc"`` (``mcmc.py``): ``generator``, ``draws`` (int64, for ``relocate_gs`` and
    ``add_new_gs``: each uses its first n, so the two steps of one iteration see the same numbers -- meant for tests; leave
    it out to have each step draw its own from ``generator``) and ``noise`` (``[>= P, 3]``, for ``inject_noise``), for reproducible runs.
    Under that strategy the L1 priors join the loss, ``relocate_gs`` then ``add_new_gs`` replace ``densify_and_prune`` on
    the schedule's densify iterations, there is no opacity reset and no densification statistics, ``inject_noise``
    follows the optimizer step, and a ``sparse_adam`` step takes ``opacity`` and ``scaling`` dense (the priors'
    gradients are).  ``ValueError`` for ``cap_max <= 0`` or a fork model.
    ``opt.lambda_normal > 0`` from ``opt.normal_from_iter`` on: the frame is rendered with ``return_depth=True,
    return_normals=True`` and ``lambda_normal * normal_consistency_loss(depth, alpha, normal, tan(FoVx / 2),
    tan(FoVy / 2))`` joins the loss; the densification statistics are read from ``viewspace_points.grad``, as on
    ``depth_loss`` frames.  Combines with ``depth_loss``, ``train_exposure``, ``sparse_adam`` and ``strategy="mcmc"``.
    ``ValueError`` with ``pose_optimizer`` (the maps carry no camera gradient) and on a fork grow / learned-split model
    (the maps are not rendered on its frames).  ``lambda_normal = 0``: exactly the calls made without it.
    ``opt.depth_ratio > 0`` while the normal term is on: the frame is also rendered with ``return_median_depth=True`` and
    the term is evaluated on the blend ``(1 - depth_ratio) depth / alpha + depth_ratio median`` (``median=``,
    ``depth_ratio=`` of ``normal_consistency_loss``); the refusals are the normal term's, and ``ValueError`` outside
    [0, 1].  ``depth_ratio = 0``, or the normal term off: exactly the calls made without it.
    ``opt.lambda_dist > 0`` from ``opt.dist_from_iter`` on: the frame is rendered with ``return_distortion=True`` and
    ``lambda_dist * distortion.mean()`` joins the loss; statistics, combinations and refusals as for ``lambda_normal``.
    ``lambda_dist = 0``: exactly the calls made without it.
    ``opt.lambda_multi_view_geo > 0`` from ``opt.multi_view_from_iter`` on: ``source_camera`` (one of the frame's
    ``mvs.select_source_views``) is required, ``ValueError`` without it.  The frame is rendered with ``return_depth=True``
    (and ``return_median_depth=True`` when ``opt.depth_ratio > 0``), the source camera once more with the same options and
    background -- its colour enters no loss term -- and ``lambda_multi_view_geo * multi_view_geo_loss(surface, camera,
    source surface, source_camera, pix_max=opt.multi_view_pix_max)`` joins the loss before the one ``backward``, both
    surfaces from ``surface.surface_depth(..., opt.depth_ratio)``.  Densification statistics come from the main frame
    only; a ``sparse_adam`` step takes the rows either frame saw.  Refusals as for ``lambda_normal``.  With the term off
    ``source_camera`` is ignored: exactly the calls made without it.
    ``opt.lambda_multi_view_ncc > 0`` from ``opt.multi_view_from_iter`` on: ``source_camera`` is required in the same way.
    The frame is rendered with ``return_depth=True, return_normals=True`` (and the median under ``opt.depth_ratio > 0``),
    the source camera once for its depth -- the one source render when both multi-view terms are on -- and
    ``lambda_multi_view_ncc * multi_view_ncc_loss(surface, normal, camera, camera, source surface, source_camera,
    source_camera, patch_radius=opt.multi_view_patch_radius, pix_max=opt.multi_view_pix_max,
    ncc_max=opt.multi_view_ncc_max, n_samples=opt.multi_view_ncc_samples)`` joins the loss before the one ``backward``:
    the photographs are the two cameras' ``original_image``, turned to grey once per camera (``mvs.gray_image``).
    Statistics, the ``sparse_adam`` union and the refusals are the geometric term's.  ``lambda_multi_view_ncc = 0``:
    exactly the calls made without it, whatever the other new fields say.
    ``opt.unbiased_depth`` while ``lambda_normal``, ``lambda_multi_view_geo`` or ``lambda_multi_view_ncc`` is active: the
    frame, and the source frame, are also rendered with ``return_plane_depth=True`` and the surface those terms see is
    ``"plane_depth"``, PGSR's unbiased depth, where it was ``depth / alpha``: the normal term is fed
    ``plane_depth * alpha`` (it divides by ``alpha`` itself) with ``alpha`` set to 0 on the pixels that have no plane
    depth, so that they are uncovered there as they are for the multi-view terms; the multi-view terms are fed
    ``plane_depth``; the median is blended in under ``opt.depth_ratio`` as before (``surface.blend_plane_depth``); the
    NCC term's normal map is the planes kernel's.
    The refusals are those terms' own.  ``unbiased_depth = False``, or none of the three terms active: exactly the calls
    made without it.
    bilateral_grids: a ``bilagrid.BilateralGrids`` after its ``training_setup``.  The frame's image is
    sliced through ``bilateral_grids.grid_for(camera.image_name)`` before the colour loss -- after the exposure when
    ``train_exposure`` is on too -- ``opt.lambda_tv * bilateral_grid_tv_loss(bilateral_grids.grids)`` joins the loss, its
    learning rate follows the iteration and its optimizer is stepped and zeroed where the model's is.  The source frame
    of the multi-view terms is not sliced: its colour enters no term.  ``KeyError`` for a camera without a grid and
    ``ValueError`` before ``training_setup``, both before anything is rendered.  None: exactly the calls made without
    it.
    ``opt.abs_grad`` (AbsGS / PGSR), on the iterations that take densification statistics
    (``iteration < opt.densify_until_iter``): the frame is rendered with ``abs_grad=True`` -- which, like the map
    losses, takes the densification statistics out of the backward for the frame (``pipe.fuse_densify_stats`` is not
    honoured on it) -- ``add_densification_stats`` is handed both leaves, and ``densify_and_prune`` gets
    ``abs_grad_threshold=opt.densify_abs_grad_threshold``.  The absolute gradient is that of the colour loss; with a
    multi-view term on, only the reference frame's is accumulated (the source frame is rendered without the switch).
    ``ValueError`` for a fork model, ``strategy="mcmc"`` and ``pose_optimizer``.  ``abs_grad = False``: exactly the calls
    made without it.
    A camera that carries a reliable depth prior (``getattr(camera, "depth_reliable", False)``: ``scene.Camera`` built with
    ``invdepthmap=``) while ``depth_prior_weight(opt, iteration) > 0``: the frame is rendered with
    ``return_depth=True`` and ``weight * depth_prior_loss(invdepth, camera.invdepthmap, camera.depth_mask,
    mode=opt.depth_prior_mode)`` joins the loss before the one ``backward``; combinations, statistics and refusals are
    those of ``depth_loss`` frames, and the term adds to ``depth_loss`` when both are given.  ``ValueError`` for an unknown
    ``opt.depth_prior_mode``, before anything is rendered.  A camera without a prior, or an unreliable one: exactly the
    calls made without it.
    A camera that carries a training mask (``getattr(camera, "alpha_mask", None)``: ``scene.Camera`` built with
    ``alpha_mask=``): with ``opt.mask_photometric`` the colour loss is ``masked_l1_dssim_loss(image, gt,
    mask, opt.lambda_dssim, normalize=opt.mask_normalize)`` where ``l1_dssim_loss`` stands otherwise, after the exposure and
    the bilateral-grid slice; with ``opt.lambda_alpha_mask > 0`` the frame is rendered with ``return_depth=True`` and
    ``lambda_alpha_mask * alpha_mask_loss(alpha, mask, mode=opt.alpha_mask_mode)`` joins the loss (statistics,
    combinations and refusals as on ``depth_loss`` frames); an active depth prior's ``depth_mask`` is multiplied by the
    mask.  The normal, distortion and multi-view terms do not see the mask.  ``ValueError`` for an unknown
    ``opt.mask_normalize`` or ``opt.alpha_mask_mode``, before anything is rendered.  A camera without a mask: exactly the
    calls made without it.
    ``opt.filter_3d`` (Mip-Splatting's 3D smoothing filter): ``filter_cameras``, the training cameras, is
    required (``ValueError`` without it, for an unknown ``opt.filter_3d_rule``, and for a fork grow / learned-split model,
    whose frames ``render`` refuses a filter on).  ``model.compute_3D_filter(filter_cameras, rule=opt.filter_3d_rule,
    variance=opt.filter_3d_variance)`` runs before the frame at iteration 1 (and whenever the model has no valid filter,
    as after a restart), after every ``densify_and_prune`` and after MCMC's relocate / add, and, once densification has
    ended (``iteration > opt.densify_until_iter``), every ``opt.filter_3d_interval`` iterations up to one interval before
    ``opt.iterations``; every frame is rendered through the filter and the gradients land on ``_scaling`` and
    ``_opacity``.  ``filter_3d = False``: ``filter_cameras`` is ignored, exactly the calls made without it."""
    filter_on = bool(getattr(opt, "filter_3d", False))
    if filter_on:
        if filter_cameras is None:
            raise ValueError("opt.filter_3d needs filter_cameras, the training cameras the filter is computed from")
        filter_kw = dict(rule=getattr(opt, "filter_3d_rule", "mip_splatting"),
                         variance=float(getattr(opt, "filter_3d_variance", 0.2)))
        if filter_kw["rule"] not in ("mip_splatting", "paper"):
            raise ValueError(f"opt.filter_3d_rule must be 'mip_splatting' or 'paper', got {filter_kw['rule']!r}")
        filter_interval = int(getattr(opt, "filter_3d_interval", 100))
        if filter_interval <= 0:
            raise ValueError(f"opt.filter_3d_interval must be positive, got {filter_interval}")
        if is_fork(model) or any(bool(getattr(dataset, n, False)) for n in (
                "grow_dir", "continous_dir", "learn_split_distance", "learn_split_scale")):
            raise ValueError("opt.filter_3d does not support the fork's grow / learned-split models: render refuses a 3D "
                             "filter on their frames (virtual rows appended)")
    prior_weight = depth_prior_weight(opt, iteration) if getattr(camera, "depth_reliable", False) else 0.0
    prior_on = prior_weight > 0.0
    if prior_on:
        prior_mode = getattr(opt, "depth_prior_mode", "l1")
        if prior_mode not in ("l1", "aligned_l1", "pearson"):
            raise ValueError(f"opt.depth_prior_mode must be 'l1', 'aligned_l1' or 'pearson', got {prior_mode!r}")
    mask = getattr(camera, "alpha_mask", None)
    mask_color = mask is not None and bool(getattr(opt, "mask_photometric", True))
    alpha_weight = float(getattr(opt, "lambda_alpha_mask", 0.0)) if mask is not None else 0.0
    alpha_on = alpha_weight > 0.0
    if mask_color and getattr(opt, "mask_normalize", "image") not in ("image", "mask"):
        raise ValueError(f"opt.mask_normalize must be 'image' or 'mask', got {opt.mask_normalize!r}")
    if alpha_on and getattr(opt, "alpha_mask_mode", "bce") not in ("bce", "l1"):
        raise ValueError(f"opt.alpha_mask_mode must be 'bce' or 'l1', got {opt.alpha_mask_mode!r}")
    strategy = getattr(opt, "strategy", "default")
    if strategy not in ("default", "mcmc"):
        raise ValueError(f"strategy must be 'default' or 'mcmc', got {strategy!r}")
    mcmc = strategy == "mcmc"
    if mcmc:
        if not int(getattr(opt, "cap_max", -1)) > 0:
            raise ValueError("strategy='mcmc' needs opt.cap_max > 0, the budget of Gaussians")
        if is_fork(model):
            raise ValueError("strategy='mcmc' does not support the fork's grow / learned-split models")
        mk = dict(mcmc_kwargs or {})
        unknown = set(mk) - {"generator", "draws", "noise"}
        if unknown:
            raise ValueError(f"mcmc_kwargs: unknown keys {sorted(unknown)}")
    elif mcmc_kwargs is not None:
        raise ValueError("mcmc_kwargs needs opt.strategy == 'mcmc'")
    abs_on = bool(getattr(opt, "abs_grad", False))
    if abs_on:
        if mcmc:
            raise ValueError("opt.abs_grad does not combine with strategy='mcmc': relocation reads no gradient statistics")
        if is_fork(model) or any(bool(getattr(dataset, n, False)) for n in (
                "grow_dir", "continous_dir", "grow_distance", "learn_split_distance", "learn_split_scale")):
            raise ValueError("opt.abs_grad does not support the fork's grow / learned-split models: their densification "
                             "plan has no absolute-gradient rule")
        if pose_optimizer is not None:
            raise ValueError("opt.abs_grad does not combine with pose_optimizer: the operator refuses abs_grad=True with "
                             "camera tensors that require grad")
        abs_on = iteration < opt.densify_until_iter      # the pass runs while statistics are taken (schedule's "stats")
    if train_exposure and getattr(model, "exposure_optimizer", None) is None:
        raise ValueError("train_exposure=True needs model.setup_exposures(image names) before training_setup")
    frame_grid = None
    if bilateral_grids is not None:
        if getattr(bilateral_grids, "optimizer", None) is None:
            raise ValueError("bilateral_grids needs its training_setup(opt) before the first iteration")
        frame_grid = bilateral_grids.grid_for(camera.image_name)
    flag = lambda name: bool(getattr(dataset, name, False))      # noqa: E731
    normal_on = float(getattr(opt, "lambda_normal", 0.0)) > 0.0 and iteration >= int(getattr(opt, "normal_from_iter", 0))
    if normal_on:
        if pose_optimizer is not None:
            raise ValueError("lambda_normal > 0 does not combine with pose_optimizer: the depth, alpha and normal maps "
                             "carry no camera gradient, so the pose would be refined against the colour loss alone")
        if is_fork(model) or any(flag(n) for n in ("grow_dir", "continous_dir", "learn_split_distance",
                                                   "learn_split_scale")):
            raise ValueError("lambda_normal > 0 does not support the fork's grow / learned-split models: render refuses "
                             "return_depth / return_normals on their frames (virtual rows appended)")
    mv_from = int(getattr(opt, "multi_view_from_iter", 0))
    geo_on = float(getattr(opt, "lambda_multi_view_geo", 0.0)) > 0.0 and iteration >= mv_from
    ncc_on = float(getattr(opt, "lambda_multi_view_ncc", 0.0)) > 0.0 and iteration >= mv_from
    mv_on = geo_on or ncc_on
    if mv_on:
        which = "lambda_multi_view_geo > 0" if geo_on else "lambda_multi_view_ncc > 0"
        if source_camera is None:
            raise ValueError(f"{which} needs source_camera, a neighbouring view of the frame (mvs.select_source_views)")
        if pose_optimizer is not None:
            raise ValueError(f"{which} does not combine with pose_optimizer: the depth maps and the multi-view term carry "
                             "no camera gradient")
        if is_fork(model) or any(flag(n) for n in ("grow_dir", "continous_dir", "learn_split_distance",
                                                   "learn_split_scale")):
            raise ValueError(f"{which} does not support the fork's grow / learned-split models: render refuses "
                             "return_depth on their frames (virtual rows appended)")
    depth_ratio = float(getattr(opt, "depth_ratio", 0.0)) if normal_on or mv_on else 0.0
    if not 0.0 <= depth_ratio <= 1.0:
        raise ValueError(f"opt.depth_ratio must lie in [0, 1], got {depth_ratio}")
    median_on = depth_ratio > 0.0
    unbiased = bool(getattr(opt, "unbiased_depth", False)) and (normal_on or mv_on)
    dist_on = float(getattr(opt, "lambda_dist", 0.0)) > 0.0 and iteration >= int(getattr(opt, "dist_from_iter", 0))
    if dist_on:
        if pose_optimizer is not None:
            raise ValueError("lambda_dist > 0 does not combine with pose_optimizer: the distortion map carries no camera "
                             "gradient, so the pose would be refined against the colour loss alone")
        if is_fork(model) or any(flag(n) for n in ("grow_dir", "continous_dir", "learn_split_distance",
                                                   "learn_split_scale")):
            raise ValueError("lambda_dist > 0 does not support the fork's grow / learned-split models: render refuses "
                             "return_distortion on their frames (virtual rows appended)")
    if first_reset is None:
        first_reset = flag("white_background")
    todo = schedule(opt, iteration, first_reset)
    model.update_learning_rate(iteration)                                                       # :72
    if bilateral_grids is not None:
        bilateral_grids.update_learning_rate(iteration)
    if todo["sh_up"]:                                                                           # :75-76
        model.oneupSHdegree()
    if filter_on and (iteration == 1 or getattr(model, "filter_3D", None) is None
                      or getattr(model, "_filter_3D_stale", False)):
        model.compute_3D_filter(filter_cameras, **filter_kw)
    bg = torch.rand((3), device=background.device) if opt.random_background else background    # :89
    render_kwargs = dict(grow_dir=flag("grow_dir"), densify_grad_threshold=opt.densify_grad_threshold,
                         iteration=iteration, opt=opt, continous_dir=flag("continous_dir"),
                         grow_distance=flag("grow_distance"), modelcg=dataset, cameras_extent=cameras_extent,
                         **({"return_depth": True} if depth_loss is not None or normal_on or mv_on or prior_on or alpha_on
                            else {}),
                         **({"return_normals": True} if normal_on or ncc_on else {}),
                         **({"return_distortion": True} if dist_on else {}),
                         **({"return_median_depth": True} if median_on else {}),
                         **({"return_plane_depth": True} if unbiased else {}),
                         **({"use_trained_exp": True} if train_exposure else {}))
    pkg = render(camera, model, pipe, bg, **render_kwargs, **({"abs_grad": True} if abs_on else {}))      # :91
    gt = camera.original_image if gt_image is None else gt_image
    image = pkg["render"] if frame_grid is None else slice_bilateral_grid(pkg["render"], frame_grid)
    if mask_color:
        loss = masked_l1_dssim_loss(image, gt.to(image.device), mask.to(image.device), opt.lambda_dssim,
                                    normalize=getattr(opt, "mask_normalize", "image"))
    else:
        loss = l1_dssim_loss(image, gt.to(image.device), opt.lambda_dssim)                      # :99-101
    if alpha_on:
        loss = loss + alpha_weight * alpha_mask_loss(pkg["alpha"], mask.to(pkg["alpha"].device),
                                                     mode=getattr(opt, "alpha_mask_mode", "bce"))
    if bilateral_grids is not None:
        loss = loss + float(getattr(opt, "lambda_tv", 10.0)) * bilateral_grid_tv_loss(bilateral_grids.grids)
    if opt.opacitysparse > 0:                                                                   # :102-106
        loss = loss + opacity_sparsity_loss(model._opacity, opt.opacitysparse)
    if mcmc:
        loss = loss + mcmc_regularizer(model._opacity, model._scaling, opt.opacity_reg, opt.scale_reg)
    if depth_loss is not None:
        depth_target, depth_weight = depth_loss
        loss = loss + float(depth_weight) * (pkg["invdepth"] - depth_target.to(pkg["invdepth"].device)).abs().mean()
    if prior_on:
        dev = pkg["invdepth"].device
        prior_mask = camera.depth_mask.to(dev) if mask is None else camera.depth_mask.to(dev) * mask.to(dev)
        loss = loss + prior_weight * depth_prior_loss(pkg["invdepth"], camera.invdepthmap.to(dev), prior_mask,
                                                      mode=prior_mode)
    if normal_on:
        n_depth, n_alpha = pkg["depth"], pkg["alpha"]
        if unbiased:
            # a pixel whose plane depth was refused has no surface: alpha 0 takes it out of the term's stencils, where
            # a depth of 0 under its real alpha would stand as a surface at the camera
            n_alpha = torch.where(pkg["plane_depth"] > 0, n_alpha, torch.zeros_like(n_alpha))
            n_depth = pkg["plane_depth"] * n_alpha
        loss = loss + float(opt.lambda_normal) * normal_consistency_loss(
            n_depth, n_alpha, pkg["normal"], math.tan(camera.FoVx * 0.5), math.tan(camera.FoVy * 0.5),
            **({"median": pkg["median_depth"], "depth_ratio": depth_ratio} if median_on else {}))
    if dist_on:
        loss = loss + float(opt.lambda_dist) * pkg["distortion"].mean()
    src_pkg = None
    if mv_on:
        src_pkg = render(source_camera, model, pipe, bg, **render_kwargs)        # for its depth: the colour enters no term
        if unbiased:
            surfaces = [blend_plane_depth(p["plane_depth"], p["median_depth"] if median_on else None, depth_ratio)
                        for p in (pkg, src_pkg)]
        else:
            surfaces = [surface_depth(p["depth"], p["alpha"], p["median_depth"] if median_on else None, depth_ratio)
                        for p in (pkg, src_pkg)]
        pix_max = float(getattr(opt, "multi_view_pix_max", 1.0))
        if geo_on:
            loss = loss + float(opt.lambda_multi_view_geo) * multi_view_geo_loss(
                surfaces[0], camera, surfaces[1], source_camera, pix_max=pix_max)
        if ncc_on:
            loss = loss + float(opt.lambda_multi_view_ncc) * multi_view_ncc_loss(
                surfaces[0], pkg["normal"], camera, camera, surfaces[1], source_camera, source_camera,
                patch_radius=int(getattr(opt, "multi_view_patch_radius", 3)), pix_max=pix_max,
                ncc_max=float(getattr(opt, "multi_view_ncc_max", 0.9)),
                n_samples=int(getattr(opt, "multi_view_ncc_samples", 102400)))
    loss.backward()                                                                             # :107
    with torch.no_grad():
        if mcmc:
            if todo["densify"]:
                relocate_gs(model, generator=mk.get("generator"), draws=mk.get("draws"))
                add_new_gs(model, opt.cap_max, generator=mk.get("generator"), draws=mk.get("draws"))
                if filter_on:
                    model.compute_3D_filter(filter_cameras, **filter_kw)
        elif todo["stats"]:                                                                     # :127-137
            add_densification_stats(model, pkg["viewspace_points"], pkg["radii"],
                                    **({"viewspace_abs": pkg["viewspace_points_abs"]} if abs_on else {}))
            if todo["densify"]:
                densify_and_prune(model, opt.densify_grad_threshold, opt.min_opacity, cameras_extent,
                                  todo["size_threshold"], opt=opt, iteration=iteration, **(densify_kwargs or {}),
                                  **({"abs_grad_threshold": opt.densify_abs_grad_threshold} if abs_on else {}))
                if filter_on:
                    model.compute_3D_filter(filter_cameras, **filter_kw)
            if todo["reset"]:
                model.reset_opacity()
        if filter_on and iteration > opt.densify_until_iter and iteration % filter_interval == 0 \
                and iteration < opt.iterations - filter_interval:
            model.compute_3D_filter(filter_cameras, **filter_kw)
        if todo["step"]:                                                                        # :140-142
            if getattr(opt, "optimizer_type", "default") == "sparse_adam":
                # the rows this frame produced a gradient for: the ones it saw, and on a grown / learned-split frame the
                # selected sources too (a source receives the folded gradient of its virtual copy even when it is off
                # screen itself).  The sparsity term's gradient lands on low-opacity rows seen or not: opacity goes dense.
                visibility = pkg["visibility_filter"]
                if pkg["selected_pts_mask"] is not None:
                    visibility = visibility | pkg["selected_pts_mask"]
                if src_pkg is not None:
                    visibility = visibility | src_pkg["visibility_filter"]       # the source frame's rows have gradients too
                dense = ("opacity", "scaling") if mcmc else (("opacity",) if opt.opacitysparse > 0 else ())
                model.optimizer.step(visibility, dense=dense)
            else:
                model.optimizer.step()
            model.optimizer.zero_grad(set_to_none=True)
            if mcmc:
                inject_noise(model, opt.noise_lr, generator=mk.get("generator"), noise=mk.get("noise"))
            if train_exposure:
                model.exposure_optimizer.step()
                model.exposure_optimizer.zero_grad(set_to_none=True)
            if bilateral_grids is not None:
                bilateral_grids.optimizer.step()
                bilateral_grids.optimizer.zero_grad(set_to_none=True)
            if pose_optimizer is not None:
                pose_optimizer.step()
                pose_optimizer.zero_grad(set_to_none=True)
    return loss.detach()


def save_checkpoint(model, iteration: int, path: str) -> None:
    """``torch.save((gaussians.capture(), iteration), path)`` (``train.py:159``)."""
    torch.save((model.capture(), iteration), path)


def load_checkpoint(model, path: str, opt, optimizer_cls=None) -> int:
    """``train.py:41-42``: restores ``model`` from the file and returns the iteration it was written at.  The file is
    a pickle of tensors, numbers and the optimizer's state dict: load only files you wrote."""
    model_params, first_iter = torch.load(path, weights_only=False)
    model.restore(model_params, opt, optimizer_cls)
    return int(first_iter)


__all__ = ["OptimizationParams", "PipelineParams", "schedule", "depth_prior_weight", "training_iteration", "save_checkpoint", "load_checkpoint"]
