"""MI355X-native differentiable Gaussian rasterizer: drop-in for the reference's
``diff_gaussian_rasterization`` operator and ``gaussian_renderer.render`` host.

    from mvs_gaussian_splatting_amd import GaussianRasterizationSettings, GaussianRasterizer, render
"""
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer, rasterize_gaussians,  # noqa: F401
                         rasterize_gaussians_fused)
from .renderer import render  # noqa: F401
from .losses import l1_loss, l1_dssim_loss, opacity_sparsity_loss, add_densification_stats  # noqa: F401
from .optim import Adam  # noqa: F401
from .exposure import apply_exposure, save_exposures, load_exposures  # noqa: F401
from .bilagrid import slice_bilateral_grid, bilateral_grid_tv_loss, BilateralGrids  # noqa: F401
from .model import GaussianModel  # noqa: F401
from .metrics import psnr, ssim, image_metrics, to_uint8_hwc, EvalAccumulator, evaluate_views  # noqa: F401
from .image_ingest import load_image, load_image_host  # noqa: F401
from .scene import Scene, Camera, MiniCam, PoseCamera, ModelParams  # noqa: F401
from .contribution import ContributionStats, measure, prune_points_, prune_by_contribution  # noqa: F401
from .features import gaussian_normals, gaussian_planes  # noqa: F401
from .tsdf import (TSDFVolume, ContractedTSDFVolume, fuse_views, volume_for_points,  # noqa: F401
                   contracted_volume_for_points, bounding_sphere, view_counts_for_views)
from .mcmc import mcmc_regularizer, inject_noise, relocate_gs, add_new_gs  # noqa: F401
from .normal_consistency import normal_consistency_loss, depth_to_normals  # noqa: F401
from .depth_prior import depth_prior_loss  # noqa: F401
from .masked_loss import alpha_mask_loss, masked_l1_dssim_loss  # noqa: F401
from .surface import surface_depth, plane_depth  # noqa: F401
from .mesh import (connected_components, clean_mesh, simplify_mesh, dilate_mask, vertex_view_counts,  # noqa: F401
                   cull_mesh_by_views, rasterize_mesh, face_normal_map, face_view_counts, cull_invisible_faces)
from .geometry_eval import NearestIndex, nearest_points, sample_surface, evaluate_points, evaluate_mesh  # noqa: F401
from .geometry_eval import (transform_points, voxel_down_sample, estimate_similarity, align_cameras,  # noqa: F401
                            icp_step, icp_registration, register_tnt, load_crop_volume, crop_points)
from .mvs import (select_source_views, depth_consistency, backproject_depth, fuse_depth_points,  # noqa: F401
                  multi_view_geo_loss, multi_view_ncc_loss, gray_image)
from .compress import (kmeans_assign, kmeans, compress_model, CompressedGaussians, save_compressed,  # noqa: F401
                       load_compressed)
from .filter3d import compute_3d_filter, apply_3d_filter, filtered_scaling_opacity  # noqa: F401

__all__ = ["Scene", "Camera", "MiniCam", "PoseCamera", "ModelParams", "load_image", "load_image_host",
           "GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "render", "l1_loss", "apply_exposure", "save_exposures", "load_exposures", "l1_dssim_loss",
           "opacity_sparsity_loss", "add_densification_stats", "Adam", "GaussianModel", "psnr", "ssim", "image_metrics", "to_uint8_hwc", "EvalAccumulator",
           "evaluate_views", "ContributionStats", "measure", "prune_points_", "prune_by_contribution",
           "mcmc_regularizer", "inject_noise", "relocate_gs", "add_new_gs", "gaussian_normals", "gaussian_planes",
           "TSDFVolume", "ContractedTSDFVolume", "fuse_views", "volume_for_points", "contracted_volume_for_points",
           "bounding_sphere", "normal_consistency_loss", "depth_to_normals",
           "surface_depth", "plane_depth", "connected_components", "clean_mesh", "simplify_mesh", "NearestIndex", "nearest_points", "sample_surface",
           "evaluate_points", "evaluate_mesh", "select_source_views", "depth_consistency", "backproject_depth",
           "fuse_depth_points", "multi_view_geo_loss", "multi_view_ncc_loss",
           "gray_image", "slice_bilateral_grid", "bilateral_grid_tv_loss", "BilateralGrids", "dilate_mask",
           "vertex_view_counts", "cull_mesh_by_views", "view_counts_for_views",
           "rasterize_mesh", "face_normal_map", "face_view_counts", "cull_invisible_faces",
           "transform_points", "voxel_down_sample", "estimate_similarity", "align_cameras", "icp_step", "icp_registration",
           "register_tnt", "load_crop_volume", "crop_points", "depth_prior_loss",
           "masked_l1_dssim_loss", "alpha_mask_loss",
           "kmeans_assign", "kmeans", "compress_model", "CompressedGaussians", "save_compressed", "load_compressed",
           "compute_3d_filter", "apply_3d_filter", "filtered_scaling_opacity"]
