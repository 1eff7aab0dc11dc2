"""Render host: the reference's ``gaussian_renderer.render`` (``gaussian_renderer/__init__.py:19-313``) on duck-typed
camera / model objects, with the fork's grow / learned-split branch (``:91-253``, ``grow.py``).

The branch opens when ``iteration`` and ``opt`` are given (``train.py:91`` passes both, ``training_report`` only ``opt``):
grow mode (``grow_dir`` / ``continous_dir`` inside the densification window, after the first opacity reset) or the
learned split (``modelcg.learn_split_distance`` / ``learn_split_scale``, every training frame).  An open frame renders
P + G Gaussians and returns ``radii`` / ``visibility_filter`` of the P originals and ``selected_pts_mask``; the gradient
of every virtual row lands on its source's parameters, the learned tensors (``_dirs_prob``, ``_conti_dirs``,
``_grow_dist``, ``_split_distance``, ``_split_scale``) and ``viewspace_points``.  A closed frame is the plain frame,
kernel for kernel.
"""
from __future__ import annotations

import math

import torch

from . import grow
from .exposure import apply_exposure
from .features import gaussian_normals, gaussian_planes
from .filter3d import apply_3d_filter, checked_filter_3D
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer, _grown_key, rasterize_gaussians_fused
from .sh import eval_sh
from .surface import plane_depth as _plane_depth


def _can_fuse(pc, pipe, override_color) -> bool:
    """The raw-parameter fast path applies when the model is the reference's parameterisation
    (``scene/gaussian_model.py:27-42``: exp / sigmoid / normalize activations, degree-3 SH storage split
    into ``_features_dc`` / ``_features_rest``) and no Python-side fallback was requested."""
    if override_color is not None or getattr(pipe, "convert_SHs_python", False) or \
            getattr(pipe, "compute_cov3D_python", False) or not getattr(pipe, "fuse_activations", True):
        return False
    need = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
    if not all(hasattr(pc, k) for k in need):
        return False
    if getattr(pc, "scaling_activation", None) is not torch.exp or \
            getattr(pc, "opacity_activation", None) is not torch.sigmoid or \
            getattr(pc, "rotation_activation", None) is not torch.nn.functional.normalize:
        return False
    fr = pc._features_rest
    # degree-3 storage (15 rest coefficients: split SH rows) or degree-0 storage (none: f_dc IS the SH tensor)
    return fr.dim() == 3 and fr.shape[1] in (0, 15) and pc._features_dc.shape[1] == 1 and pc._xyz.is_cuda


_ZEROS = {}


def _zero_leaf(like: torch.Tensor) -> torch.Tensor:
    """A leaf tensor of zeros shaped like ``like`` with ``requires_grad`` (its ``.grad`` is a fresh tensor per
    backward).  The zeros are cached per (shape, dtype, device) and shared read-only between the leaves."""
    key = (tuple(like.shape), like.dtype, like.device)
    z = _ZEROS.get(key)
    if z is None:
        if len(_ZEROS) > 8:
            _ZEROS.clear()
        z = _ZEROS[key] = torch.zeros(like.shape, dtype=like.dtype, device=like.device)
    return z.detach().requires_grad_(True)


def _fused_stats(pc, pipe, xyz):
    """(xyz_gradient_accum, denom, max_radii2D) when the caller asked for the densification statistics to be taken
    inside the backward (``pipe.fuse_densify_stats``) and the model carries float32 accumulators."""
    if not getattr(pipe, "fuse_densify_stats", False) or not (torch.is_grad_enabled() and xyz.requires_grad):
        return None
    trio = tuple(getattr(pc, k, None) for k in ("xyz_gradient_accum", "denom", "max_radii2D"))
    P = int(xyz.shape[0])
    if any(t is None or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P for t in trio):
        return None
    return trio


def _aux_entries(aux: torch.Tensor) -> dict:
    """The operator's ``[3,H,W]`` maps as the three ``[1,H,W]`` entries of the result dict."""
    return {"depth": aux[0:1], "invdepth": aux[1:2], "alpha": aux[2:3]}


def _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier):
    return GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height),
        image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5),
        tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
        bg=bg_color,
        scale_modifier=scaling_modifier,
        viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform,
        sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center,
        prefiltered=False,
        debug=bool(getattr(pipe, "debug", False)),
    )


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier: float = 1.0,
           override_color=None, grow_dir=False, densify_grad_threshold=0, iteration=None, opt=None,
           continous_dir=False, grow_distance=False, modelcg=None, cameras_extent=None, return_depth=False,
           use_trained_exp=False, contribution=None, contribution_mask=None, features=None, return_normals=False,
           return_distortion=False, distortion_kwargs=None, return_median_depth=False, return_plane_depth=False,
           abs_grad=False):
    """Render the scene; ``bg_color`` must be on the GPU.  Returns the reference's result dict
    (``gaussian_renderer/__init__.py:309-313``).  The keyword arguments after ``override_color`` are the reference's
    (``:19``) and drive the grow / learned-split branch (module docstring); the frame of a closed branch is unchanged.

    ``pipe.fuse_densify_stats = True`` (this build's extension) makes the backward of this frame also run
    ``add_densification_stats`` (``scene/gaussian_model.py:775-777``) and the ``max_radii2D`` update of ``train.py:130``
    on the model's accumulators; the ``add_densification_stats`` of this package then recognises the frame and does
    nothing, so the reference's call sequence (render, backward, add_densification_stats) stays as it is.

    ``return_depth=True`` (this build's extension): the dict gains ``"depth"`` (``sum w z``), ``"invdepth"``
    (``sum w / z``, upstream's inverse-depth map) and ``"alpha"`` (``sum w = 1 - T``), each ``[1,H,W]`` and
    differentiable; ``z`` is the view-space depth, there is no background term.  On such a frame the in-backward
    densification statistics are not taken (``viewspace_points.grad`` is the sum of the colour node's and the maps'
    node's gradients, which only exists after the backward): ``add_densification_stats`` reads it, as on grown frames.
    Not available on a frame of the open grow / learned-split branch.

    ``use_trained_exp=True`` (upstream 3DGS's name): ``"render"`` is the rasterizer's image after the camera's 3x4
    exposure, ``apply_exposure(image, pc.get_exposure_from_name(viewpoint_camera.image_name))`` (``exposure.py``), on
    every path; the maps of ``return_depth`` are untouched.  False leaves the frame exactly as it was.

    ``contribution=stats`` (a ``contribution.ContributionStats`` with one row per Gaussian): the frame's per-Gaussian
    blending-weight statistics are added into ``stats`` after the colour forward and ``stats.views`` counts the frame;
    ``contribution_mask`` (uint8 ``[H,W]``) leaves the pixels with value 0 out.  Not differentiable; the result dict is
    what it is without it.  Not available on a frame of the open grow / learned-split branch.

    ``features=F`` (float32 ``[P,C]``, C >= 1): the dict gains ``"features"`` ``[C,H,W]`` = ``sum w F[id]``, the rows of
    ``F`` composited with the colour pass's blending weights (no background term, no clamp), differentiable in ``F`` and
    the geometry.  ``return_normals=True``: the dict gains ``"normal"`` ``[3,H,W]`` = ``sum w n``, un-normalised, with
    ``n = features.gaussian_normals(pc.get_scaling, pc.get_rotation, ...)`` the view-space normals; with both, one
    concatenated call is split afterwards.  As with ``return_depth`` the in-backward densification statistics are not
    taken on such a frame, and it is refused on the open grow / learned-split branch.

    ``return_distortion=True``: the dict gains ``"distortion"`` ``[1,H,W]`` = ``sum_i sum_{j<i} w_i w_j (m_i - m_j)^2``, the
    depth-distortion map of 2DGS (``rasterizer`` module docstring), differentiable in the geometry;
    ``distortion_kwargs``: ``dict(mapping="linear" | "ndc", near=, far=)``, default ``"ndc"`` with near 0.2 and far 100.
    The same two conditions as for ``return_depth`` apply.

    ``return_median_depth=True``: the dict gains ``"median_depth"`` ``[1,H,W]``, the view depth of the last composited
    Gaussian in front of which the transmittance still exceeds one half (2DGS's median depth, what it meshes bounded scenes
    from; 0 where nothing was composited), differentiable in the positions alone, and ``"median_id"`` ``[H,W]`` (int32),
    the row of that Gaussian (-1 where nothing was composited) (``rasterizer`` module docstring).  The
    same two conditions as for ``return_depth`` apply.

    ``return_plane_depth=True`` (PGSR's unbiased depth): implies ``return_depth`` and ``return_normals``.
    The per-Gaussian rows ``(n_view, d) = features.gaussian_planes(pc.get_scaling, pc.get_rotation, ...)`` -- one HIP
    launch -- ride as four feature channels behind the caller's ``features``, so the dict gains ``"distance"`` ``[1,H,W]``
    = ``sum w d`` (``d`` the distance of the camera centre from the Gaussian's plane) next to ``"normal"``, and
    ``"plane_depth"`` ``[1,H,W]`` = ``surface.plane_depth(normal, distance, alpha, tan(FoVx / 2), tan(FoVy / 2))``: the
    depth at which the pixel's ray meets the blended plane, 0 where there is no surface.  Differentiable in the
    rotations, the positions and the blending weights.  On such a frame ``"normal"`` comes from the planes kernel and may
    differ from the torch path of ``return_normals`` alone in the last bits.  Combines with ``features=``,
    ``return_median_depth`` and ``return_distortion``; the same two conditions as for ``return_depth`` apply.

    ``abs_grad=True`` (AbsGS; PGSR's ``viewspace_point_tensor_abs``): the dict gains
    ``"viewspace_points_abs"``, a second zero leaf ``[P,3]`` whose ``.grad`` after the backward holds, per Gaussian and
    component, the sum over its pixels of ``|d L / d mean2D|`` of the COLOUR image (the maps' losses take no part), in
    ``viewspace_points.grad``'s scale, z = 0.  ``"render"``, ``"radii"`` and every other gradient are bit-identical to the
    frame without it.  The same two conditions as for ``return_depth`` apply; hand both leaves to
    ``add_densification_stats(model, viewspace_points, radii, viewspace_abs=viewspace_points_abs)``.

    ``pc.filter_3D`` set (Mip-Splatting's 3D smoothing filter; ``GaussianModel.compute_3D_filter``): the
    frame draws the filtered model.  The fused path hands the operator the effective raw tensors of
    ``filter3d.apply_3d_filter(pc._scaling, pc._opacity, pc.filter_3D)`` where ``_scaling`` and ``_opacity`` went (one more
    launch, and one in the backward; the gradients land on ``_scaling`` and ``_opacity``); the getter path hands it their
    activations.  ``gaussian_normals`` and ``gaussian_planes`` keep the unfiltered scales: adding the same ``f^2`` to all
    three squared axes does not change which axis is the flattest, so the normal is the same.  A filter that is stale
    (rows were removed, added or reordered since it was computed) or not ``[P]`` is refused with a ``ValueError`` that
    names ``compute_3D_filter``, before a GPU is asked for; so is a filter on a frame of the open grow / learned-split
    branch.  Without a filter the frame is issued exactly as before."""
    if distortion_kwargs is not None and not return_distortion:
        raise ValueError("distortion_kwargs needs return_distortion=True")
    pkg = _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, grow_dir,
                  densify_grad_threshold, iteration, opt, continous_dir, grow_distance, modelcg, cameras_extent,
                  return_depth, contribution, contribution_mask, features, return_normals,
                  (True if distortion_kwargs is None else dict(distortion_kwargs)) if return_distortion else None,
                  **({"median_depth": True} if return_median_depth else {}),
                  **({"plane_depth": True} if return_plane_depth else {}),
                  **({"abs_grad": True} if abs_grad else {}))
    if use_trained_exp:
        pkg["render"] = apply_exposure(pkg["render"], pc.get_exposure_from_name(viewpoint_camera.image_name))
    return pkg


def _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, grow_dir, densify_grad_threshold,
            iteration, opt, continous_dir, grow_distance, modelcg, cameras_extent, return_depth, contribution=None,
            contribution_mask=None, features=None, return_normals=False, distortion=None, median_depth=False,
            plane_depth=False, abs_grad=False):
    """The frame of ``render`` as the rasterizer leaves it.  ``abs_grad``: ``render``'s.  ``distortion``: None, or the operator's ``distortion=``;
    ``median_depth``: the operator's ``median_depth=``; ``plane_depth``: ``render``'s ``return_plane_depth``."""
    filt = checked_filter_3D(pc)                       # host checks only; None for a model without a filter
    which = grow.branch(iteration, opt, grow_dir, continous_dir, modelcg)
    if which is not None and filt is not None:
        raise ValueError("a 3D filter is not available on a frame of the open grow / learned-split branch (virtual rows "
                         "appended): set filter_3D = None, or call compute_3D_filter after the branch has closed")
    if filt is not None and not all(hasattr(pc, k) for k in ("_scaling", "_opacity")):
        raise ValueError("a 3D filter needs the model's raw _scaling and _opacity (exp / sigmoid activations)")
    if plane_depth:
        if which is not None:
            raise ValueError("return_plane_depth=True is not available on a frame of the open grow / learned-split branch "
                             "(virtual rows appended): render the maps in a frame of their own")
        return_depth = return_normals = True
    if which is not None and contribution is not None:
        raise ValueError("contribution statistics are not available on a frame of the open grow / learned-split branch "
                         "(virtual rows appended): measure in a frame of its own")
    # the statistics request travels only when the caller made one: a frame without it is issued exactly as before
    extra_stats = {} if contribution is None else {"contribution": contribution, "contribution_mask": contribution_mask}
    if which is not None and return_depth:
        raise ValueError("return_depth=True is not available on a frame of the open grow / learned-split branch "
                         "(virtual rows appended): render the maps in a frame of their own")
    want_feat = features is not None or return_normals
    if which is not None and want_feat:
        raise ValueError("features / return_normals are not available on a frame of the open grow / learned-split branch "
                         "(virtual rows appended): render the maps in a frame of their own")
    if which is not None and distortion is not None:
        raise ValueError("return_distortion=True is not available on a frame of the open grow / learned-split branch "
                         "(virtual rows appended): render the map in a frame of its own")
    if which is not None and median_depth:
        raise ValueError("return_median_depth=True is not available on a frame of the open grow / learned-split branch "
                         "(virtual rows appended): render the map in a frame of its own")
    if which is not None and abs_grad:
        raise ValueError("abs_grad=True is not available on a frame of the open grow / learned-split branch "
                         "(virtual rows appended)")
    if which is not None:
        return _render_grown(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, which, grow_dir,
                             densify_grad_threshold, continous_dir, grow_distance, modelcg, cameras_extent)
    xyz = pc.get_xyz
    # zero tensor whose .grad receives dL/d(mean2D) for the densification statistics.  The reference builds it as
    # `zeros_like(...) + 0` + retain_grad() (gaussian_renderer/__init__.py:32-36); a leaf with requires_grad gets
    # its .grad populated all the same and saves a 72 MB copy kernel per frame at 6 M Gaussians.
    # The operator never reads (or writes) its values, so every frame's leaf aliases one cached block of zeros: a
    # fresh 72 MB memset per frame is 20 us of the 6 M-Gaussian forward.
    screenspace_points = _zero_leaf(xyz)
    stats = None if return_depth or want_feat or distortion is not None or median_depth or abs_grad \
        else _fused_stats(pc, pipe, xyz)
    # the second leaf of an abs_grad frame travels only when the caller asked: a frame without it is issued exactly as before
    abs_kw = {"means2D_abs": _zero_leaf(xyz), "abs_grad": True} if abs_grad else {}
    abs_entry = {"viewspace_points_abs": abs_kw["means2D_abs"]} if abs_grad else {}
    if stats is not None:
        screenspace_points._gsr_stats_fused = True      # read by losses.add_densification_stats

    raster_settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    if want_feat:
        rows = [] if features is None else [features]
        if plane_depth:
            rows.append(gaussian_planes(pc.get_scaling, pc.get_rotation, xyz, raster_settings.viewmatrix,
                                        raster_settings.campos))
        elif return_normals:
            rows.append(gaussian_normals(pc.get_scaling, pc.get_rotation, xyz, raster_settings.viewmatrix,
                                         raster_settings.campos))
        extra_stats = dict(extra_stats, features=rows[0] if len(rows) == 1 else torch.cat(rows, dim=1))

    median_kw = {"median_depth": True} if median_depth else {}
    # the tensors the operator is handed where _scaling and _opacity go: the model's own, or with a 3D filter the
    # effective raw ones (their exp / sigmoid are the filtered values)
    raw_scaling, raw_opacity = (getattr(pc, "_scaling", None), getattr(pc, "_opacity", None)) if filt is None \
        else apply_3d_filter(pc._scaling, pc._opacity, filt)

    def feature_entries(out):
        """The operator's trailing ``feat`` / ``dist`` / ``median``, ``median_id`` as the dict's ``"features"`` /
        ``"normal"`` / ``"distortion"`` / ``"median_depth"``, ``"median_id"`` entries."""
        if median_depth:
            return {**_tail_entries(out[:-2]), "median_depth": out[-2], "median_id": out[-1]}
        return _tail_entries(out)

    def _tail_entries(out):
        if distortion is not None:
            return {**_feature_entries(out[-2]), "distortion": out[-1]}
        return _feature_entries(out[-1])

    def _feature_entries(feat):
        if not want_feat:
            return {}
        n_user = 0 if features is None else int(features.shape[1])
        out = {} if features is None else {"features": feat[:n_user]}
        if plane_depth:
            out["normal"], out["distance"] = feat[n_user:n_user + 3], feat[n_user + 3:]
        elif return_normals:
            out["normal"] = feat[n_user:]
        return out

    def with_plane_depth(pkg):
        if plane_depth:
            pkg["plane_depth"] = _plane_depth(pkg["normal"], pkg["distance"], pkg["alpha"], raster_settings.tanfovx,
                                              raster_settings.tanfovy)
        return pkg

    if _can_fuse(pc, pipe, override_color):
        # same result as the getter path below, without materialising cat(f_dc, f_rest), exp, normalize, sigmoid (and
        # without building an nn.Module per frame: the operator is called as a function)
        # visibility_filter (= radii > 0, gaussian_renderer/__init__.py:311) is stored by the preprocess kernel itself:
        # a torch compare over 6 M radii is a 9-us kernel per frame
        visible = torch.empty(xyz.shape[0], dtype=torch.bool, device=xyz.device)
        if return_depth or want_feat or distortion is not None or median_depth:
            out = rasterize_gaussians_fused(xyz, screenspace_points, pc._features_dc, pc._features_rest, raw_opacity,
                                            raw_scaling, pc._rotation, raster_settings, visible=visible,
                                            **({"aux_maps": True} if return_depth else {}), **extra_stats,
                                            **({} if distortion is None else {"distortion": distortion}), **median_kw,
                                            **abs_kw)
            return with_plane_depth({"render": out[0], "viewspace_points": screenspace_points, **abs_entry,
                                     "visibility_filter": visible, "radii": out[1], "selected_pts_mask": None,
                                     **(_aux_entries(out[2]) if return_depth else {}), **feature_entries(out)})
        rendered_image, radii = rasterize_gaussians_fused(xyz, screenspace_points, pc._features_dc, pc._features_rest,
                                                          raw_opacity, raw_scaling, pc._rotation, raster_settings,
                                                          densify_stats=stats, visible=visible, **extra_stats, **abs_kw)
        return {"render": rendered_image, "viewspace_points": screenspace_points, **abs_entry,
                "visibility_filter": visible, "radii": radii, "selected_pts_mask": None}

    feat_kw = {"features": extra_stats.pop("features")} if want_feat else {}
    rasterizer = GaussianRasterizer(raster_settings=raster_settings, **({"aux_maps": True} if return_depth else {}),
                                    **extra_stats, **({} if distortion is None else {"distortion": distortion}), **median_kw,
                                    **({"abs_grad": True} if abs_grad else {}))
    scales = rotations = cov3D_precomp = None
    if filt is not None:
        filtered_scales, filtered_opacity = torch.exp(raw_scaling), torch.sigmoid(raw_opacity)
    if getattr(pipe, "compute_cov3D_python", False):
        cov3D_precomp = pc.get_covariance(scaling_modifier) if filt is None else \
            pc.covariance_activation(filtered_scales, scaling_modifier, pc._rotation)
    else:
        scales, rotations = pc.get_scaling if filt is None else filtered_scales, pc.get_rotation

    shs = colors_precomp = None
    if override_color is None:
        if getattr(pipe, "convert_SHs_python", False):
            feats = pc.get_features
            shs_view = feats.transpose(1, 2).reshape(-1, 3, (pc.max_sh_degree + 1) ** 2)
            dir_pp = xyz - viewpoint_camera.camera_center.repeat(feats.shape[0], 1)
            dir_pp = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp) + 0.5, 0.0)
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color

    # exactly the reference's eight keyword arguments (gaussian_renderer/__init__.py:257-265); the statistics request of
    # this build travels as a ninth only when the caller asked for it
    extra = dict(feat_kw) if stats is None else {"densify_stats": stats}
    if abs_grad:
        extra["means2D_abs"] = abs_kw["means2D_abs"]
    out = rasterizer(means3D=xyz, means2D=screenspace_points, shs=shs,
                     colors_precomp=colors_precomp, opacities=pc.get_opacity if filt is None else filtered_opacity,
                     scales=scales,
                     rotations=rotations, cov3D_precomp=cov3D_precomp, **extra)
    rendered_image, radii = out[0], out[1]
    return with_plane_depth({"render": rendered_image,
                             "viewspace_points": screenspace_points, **abs_entry,
                             "visibility_filter": radii > 0,
                             "radii": radii,
                             "selected_pts_mask": None,
                             **(_aux_entries(out[2]) if return_depth else {}),
                             **feature_entries(out)})


def _render_grown(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, which, grow_dir,
                  densify_grad_threshold, continous_dir, grow_distance, modelcg, cameras_extent):
    """A frame of the open grow / learned-split branch (``gaussian_renderer/__init__.py:91-253``) on the fused
    raw-parameter path: plan (one count read-back), expansion to P + G rows, the fused operator, radii of the P originals.
    The in-backward densification statistics are not taken (their accumulators have P rows): the caller's
    ``add_densification_stats`` reads the folded ``viewspace_points.grad``."""
    if override_color is not None or getattr(pipe, "convert_SHs_python", False) or \
            getattr(pipe, "compute_cov3D_python", False):
        raise ValueError("the grow / learned-split branch exists for SH + scale / rotation inputs only: with "
                         "override_color, convert_SHs_python or compute_cov3D_python the reference's own branch fails "
                         "on torch.cat(None, ...) (gaussian_renderer/__init__.py:114-115, :246)")
    if not _can_fuse(pc, pipe, None):
        raise ValueError("the grow / learned-split branch runs on the fused raw-parameter path only: the model must be "
                         "the reference's parameterisation on the GPU with pipe.fuse_activations left on")
    mode = grow.mode_bits(which, grow_dir, continous_dir, grow_distance, modelcg)
    pde = grow.percent_dense_extent(pc, which, modelcg, cameras_extent)
    pl = grow.plan(pc, mode, densify_grad_threshold, pde)
    if which == grow.GROW and pde != math.inf and pl.n_big > 0:
        raise ValueError(grow._QUIRK.format(n=pl.n_big))
    xyz = pc.get_xyz
    P = int(xyz.shape[0])
    screenspace_points = _zero_leaf(xyz)
    raster_settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier)
    if which == grow.SPLIT and pl.G == 0:
        # :196 nothing to split: the plain frame (the learned split tensors take no part in it)
        visible = torch.empty(P, dtype=torch.bool, device=xyz.device)
        rendered_image, radii = rasterize_gaussians_fused(xyz, screenspace_points, pc._features_dc, pc._features_rest,
                                                          pc._opacity, pc._scaling, pc._rotation, raster_settings,
                                                          visible=visible)
        return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": visible,
                "radii": radii, "selected_pts_mask": pl.selected}
    _, ext = grow.expand(pc, screenspace_points, mode, densify_grad_threshold, pde, pl=pl)
    visible = torch.empty(P + pl.G, dtype=torch.bool, device=xyz.device)
    rendered_image, radii = rasterize_gaussians_fused(*ext, raster_settings, visible=visible, _state_key=_grown_key(P))
    return {"render": rendered_image, "viewspace_points": screenspace_points, "visibility_filter": visible[:P],
            "radii": radii[:P], "selected_pts_mask": pl.selected}
