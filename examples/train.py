"""The reference's training loop (``train.py:34-160``) on a synthetic scene, from this package's ``GaussianModel`` and
``trainer.training_iteration``: initialise from a point cloud, train with the reference's schedule (learning-rate decay,
SH degree steps, densification, opacity resets, the optional opacity sparsity term), checkpoint, resume, write a PLY.

    python examples/train.py [--iterations N] [--checkpoint_iterations N ...] [--start_checkpoint FILE] [--out DIR]
    python examples/train.py -s <COLMAP or Blender directory> -m <output directory> [-r 1|2|4|8|width] [--eval]
                             [--white_background] [--images DIR] [--data_device cuda|cpu] [--save_iterations N ...]
                             [--refine_poses [--pose_lr LR]]
                             [--train_exposure [--exposure_lr_init LR] [--exposure_lr_final LR]
                              [--exposure_lr_delay_steps N] [--exposure_lr_delay_mult M]]
                             [--bilateral_grid [--bilateral_grid_shape W H L]]
                             [--prune_iterations N [N ...] --prune_keep_ratio R [--prune_kind sum|max|count|mean]]
                             [--strategy mcmc --cap_max N [--noise_lr LR] [--opacity_reg W] [--scale_reg W]]
                             [--lambda_normal L [--normal_from_iter N] [--depth_ratio R]]
                             [--lambda_dist L [--dist_from_iter N]]
                             [--lambda_multi_view_geo L [--multi_view_sources K] [--multi_view_from_iter N]
                              [--multi_view_pix_max P]]
                             [--lambda_multi_view_ncc L [--multi_view_ncc_samples N] [--multi_view_patch_radius R]]
                             [-d DIR [--depth_prior_mode l1|aligned_l1|pearson] [--depth_l1_weight_init W]
                              [--depth_l1_weight_final W]]
                             [--masks DIR [--mask_normalize image|mask] [--no_mask_photometric] [--lambda_alpha_mask L]]

``--masks DIR`` (with ``-s``; off by default) trains under per-image masks: ``DIR/<image stem>.png`` or COLMAP's
``DIR/<image file name>.png`` for every training image, ``DIR`` under the scene or absolute, non-zero keeps the pixel.  The
colour loss then ignores what a mask hides (``masked_loss.py``), normalised by the image (``--mask_normalize image``,
upstream 3DGS's and gsplat's rule) or by the mask's area (``mask``); ``--no_mask_photometric`` leaves the colour loss
unmasked.  ``--lambda_alpha_mask L`` adds ``L`` times the binary cross-entropy of the rendered opacity against the mask: the
silhouette term of object captures, which keeps the background empty before meshing.

``-d DIR`` (with ``-s``; upstream 3DGS's option, off by default) regularises training with a per-image inverse-depth prior:
``<scene>/DIR/<image stem>.png``, 16-bit, for every training image, aligned by ``<scene>/sparse/0/depth_params.json`` when
upstream's ``make_depth_scale.py`` wrote one.  The term (``depth_prior.py``) is ``--depth_prior_mode``: ``l1``, upstream's,
which needs that file; ``aligned_l1`` or ``pearson``, which fit the alignment per frame and take raw monocular maps.  Its
weight decays from ``--depth_l1_weight_init`` to ``--depth_l1_weight_final`` over the run.
``--strategy mcmc --cap_max N`` (both forms) densifies the MCMC way (``mcmc.py``): a budget of N Gaussians, dead ones
relocated onto live ones, 5 % growth a round, position noise and L1 priors on opacity and scale.
``--lambda_normal L`` (both forms; off by default) adds the depth-normal consistency term of 2DGS from iteration
``--normal_from_iter`` on (``normal_consistency.py``): the normals composited from the Gaussians are pulled towards the
normals of the rendered depth surface.  2DGS uses 0.05 from iteration 7000.  ``--depth_ratio R`` (in [0, 1]) takes that
surface to be ``(1 - R) expected + R median`` depth: 2DGS uses 0 for unbounded scenes and 1 for bounded ones.
``--lambda_dist L`` (both forms; off by default) adds the depth-distortion term of 2DGS from iteration
``--dist_from_iter`` on: ``L`` times the mean of the rasterizer's distortion map, which pulls every ray's blending weights
together in depth.  2DGS uses 100 to 1000 from iteration 3000.
``--lambda_multi_view_geo L`` (both forms; off by default) adds the multi-view geometric term of PGSR from iteration
``--multi_view_from_iter`` on (``mvs.multi_view_geo_loss``): every view's ``--multi_view_sources`` nearest neighbours are
chosen once (``select_source_views``), each iteration draws one of the frame's at random, renders it too, and penalises
the forward-backward reprojection error between the two depth maps.  A view without neighbours trains without the term.
``--lambda_multi_view_ncc L`` (both forms; off by default; PGSR: 0.15) adds the multi-view photometric term of PGSR from
the same iteration on (``mvs.multi_view_ncc_loss``): at ``--multi_view_ncc_samples`` pixels drawn per iteration the
``(2R+1)^2`` patch (``--multi_view_patch_radius``) of the frame's photograph is carried into the source's by the homography
of the rendered plane, and one minus their normalised cross-correlation is penalised.  Sources are selected when either
multi-view weight is positive; the one source render serves both terms.
``--optimizer_type sparse_adam`` (both forms) steps only the Gaussians each frame saw (``optim.SparseGaussianAdam``).

With ``-s`` the example trains on a dataset through ``Scene`` (``scene.py``) and saves
``<output>/point_cloud/iteration_N/point_cloud.ply``, which ``examples/render.py -m <output>`` renders.
``--refine_poses`` (off by default) wraps every training camera in a ``PoseCamera`` and refines the poses with the model
(Adam at ``--pose_lr`` on the six pose parameters of each camera); the refined poses are written to
``<output>/refined_poses.json`` at the end.  ``--train_exposure`` (off by default; upstream 3DGS's option) gives every
training image a learnable 3x4 colour affine, trains it with the model and saves ``exposure.json`` next to each point
cloud; ``examples/render.py --use_trained_exp`` renders with it.  ``--bilateral_grid`` (off by default; gsplat's
``--use_bilateral_grid``) gives every training image a bilateral grid of ``--bilateral_grid_shape`` (default 16 16 8)
colour affines (``bilagrid.py``), trained with the model; the grids are saved as ``bilateral_grid_<iteration>.pt`` next to
each checkpoint and loaded with it on resume.  Evaluation and ``examples/render.py`` do not apply them: test views have
none.  ``--prune_iterations`` (both forms; off by default):
after each of those iterations the blending-weight statistics of every training camera are measured (``contribution.py``)
and the ``--prune_keep_ratio`` share of the Gaussians with the highest ``--prune_kind`` score is kept
(``examples/prune.py`` does the same to a saved scene).  Without ``-s``:

The scene: a ground-truth cloud rendered from orbit views gives the images; the model starts, as the reference's does
from a COLMAP cloud, from a jittered subsample of the ground truth's centres with their base colours.
"""
import argparse
import json
import math
import os
import random
import sys
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import (GaussianModel, measure, prune_by_contribution, render,  # noqa: E402
                                        select_source_views)
from mvs_gaussian_splatting_amd.sh import SH2RGB  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import PipelineParams, SyntheticGaussianModel, orbit_camera  # noqa: E402
from mvs_gaussian_splatting_amd.trainer import (OptimizationParams, load_checkpoint, save_checkpoint,  # noqa: E402
                                                training_iteration)

CAMERAS_EXTENT = 2.0


def make_problem(dev, P=4000, W=256, H=160, n_views=8, seed=0, keep_every=2):
    """(cameras with ``original_image``, background, point cloud ``(points, colors)`` on the device)."""
    gt = SyntheticGaussianModel(P, 3, seed=seed, log_scale_mean=math.log(0.06), extent=(1.6, 1.0, 0.8), centre=(0, 0, 4.0))
    gt._opacity += 1.0
    gt.to(dev)
    cams = [orbit_camera(v, n_views, W, H, 220.0, 220.0, centre=(0.0, 0.0, 4.0), device=dev) for v in range(n_views)]
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        for c in cams:
            c.original_image = render(c, gt, PipelineParams(), bg)["render"].clone()
    g = torch.Generator().manual_seed(seed + 7)
    points = gt._xyz[::keep_every] + 0.02 * torch.randn(gt._xyz[::keep_every].shape, generator=g).to(dev)
    colors = SH2RGB(gt._features_dc[::keep_every, 0, :]).clamp(0.0, 1.0)
    return cams, bg, (points.contiguous(), colors.contiguous())


def small_opt(iterations=60, **over):
    """The reference's defaults with the schedule shrunk to a run of tens of iterations."""
    kw = dict(iterations=iterations, position_lr_max_steps=iterations, densify_from_iter=10, densification_interval=10,
              opacity_reset_interval=30, densify_until_iter=50, densify_grad_threshold=0.0006)
    kw.update(over)
    return OptimizationParams(**kw)


def example_opt(iterations=200, **over):
    """This example's schedule: the reference's proportions at ``iterations`` -- densification every tenth of the run
    from the first tenth to three quarters, one opacity reset half-way."""
    n = iterations
    kw = dict(densify_from_iter=max(n // 10, 1), densification_interval=max(n // 10, 1),
              opacity_reset_interval=max(n // 2, 1), densify_until_iter=max(3 * n // 4, 2))
    kw.update(over)
    return small_opt(n, **kw)


def make_model(problem, opt, dataset=None, sh_degree=3, optimizer_cls=None, seed=0):
    _, _, (points, colors) = problem
    flag = lambda n: bool(getattr(dataset, n, False))   # noqa: E731
    model = GaussianModel(sh_degree, grow_dir=flag("grow_dir"), num_dirs=getattr(dataset, "num_dirs", 128),
                          continous_dir=flag("continous_dir"), grow_distance=flag("grow_distance"), modelcg=dataset)
    torch.manual_seed(seed)
    model.create_from_pcd(points, colors, CAMERAS_EXTENT)
    if optimizer_cls is None:
        model.training_setup(opt)
    else:
        model.training_setup(opt, optimizer_cls)
    return model


def prune_options(args):
    """``{"iterations", "keep_ratio", "kind"}`` of the ``--prune_*`` arguments, or None when pruning is off."""
    if not args.prune_iterations:
        return None
    if args.prune_keep_ratio is None:
        raise SystemExit("--prune_iterations needs --prune_keep_ratio")
    return {"iterations": set(args.prune_iterations), "keep_ratio": args.prune_keep_ratio, "kind": args.prune_kind}


def prune_step(model, cameras, pipe, bg, iteration, prune, log=print):
    """At the iterations of ``prune``: measure the contribution of every Gaussian over ``cameras`` and keep the best."""
    if not prune or iteration not in prune["iterations"]:
        return None
    out = prune_by_contribution(model, measure(model, cameras, pipe, bg), kind=prune["kind"],
                                keep_ratio=prune["keep_ratio"])
    if log:
        log(f"[ITER {iteration}] pruned by contribution ({prune['kind']}): {out['points'] + out['pruned']} -> "
            f"{out['points']} points")
    return out


def source_views(cameras, opt, n_sources):
    """Per view the indices of its ``n_sources`` source views, computed once; None while both multi-view terms are off."""
    if not (float(getattr(opt, "lambda_multi_view_geo", 0.0)) > 0.0 or float(getattr(opt, "lambda_multi_view_ncc", 0.0)) > 0.0):
        return None
    return select_source_views(cameras, n_sources)


def draw_source(cameras, sources, index, rng):
    """One of view ``index``'s source cameras at random; None when the term is off or the view has no source."""
    if not sources or not sources[index]:
        return None
    return cameras[rng.choice(sources[index])]


def train(model, problem, opt, first_iter=0, last_iter=None, dataset=None, pipe=None, seed=0, log=None, on_iteration=None,
          prune=None, multi_view_sources=4):
    """Iterations ``first_iter + 1 .. last_iter`` (default ``opt.iterations``), as ``train.py:54`` counts them.  The
    device generator is seeded from the iteration number before each one, so that the draws of a densification are the
    same in a resumed run as in an uninterrupted one.  ``prune``: ``prune_options``.  ``multi_view_sources``: how many
    source views each view gets while ``opt.lambda_multi_view_geo > 0`` or ``opt.lambda_multi_view_ncc > 0``.  Returns the losses as device tensors."""
    cams, bg, _ = problem
    pipe = pipe or PipelineParams()
    losses = []
    sources = source_views(cams, opt, multi_view_sources)
    for iteration in range(first_iter + 1, (last_iter or opt.iterations) + 1):
        torch.manual_seed(seed * 1_000_003 + iteration)
        index = (iteration * 3) % len(cams)
        source = draw_source(cams, sources, index, random.Random(seed * 1_000_003 + iteration))
        losses.append(training_iteration(model, cams[index], opt, pipe, bg, iteration, dataset=dataset,
                                         cameras_extent=CAMERAS_EXTENT,
                                         **({"filter_cameras": cams} if getattr(opt, "filter_3d", False) else {}),
                                         **({"source_camera": source} if source is not None else {})))
        prune_step(model, cams, pipe, bg, iteration, prune, log)
        if on_iteration:
            on_iteration(iteration, model)
        if log and iteration % 10 == 0:
            log(f"iteration {iteration}: loss {float(losses[-1]):.5f}  points {model._xyz.shape[0]}  "
                f"sh degree {model.active_sh_degree}")
    return losses


def strategy_options(args):
    """The ``OptimizationParams`` overrides of the ``--strategy`` arguments."""
    if args.strategy == "mcmc" and args.cap_max <= 0:
        raise SystemExit("--strategy mcmc needs --cap_max N, the budget of Gaussians")
    return dict(strategy=args.strategy, cap_max=args.cap_max, noise_lr=args.noise_lr, opacity_reg=args.opacity_reg,
                scale_reg=args.scale_reg, lambda_normal=args.lambda_normal, normal_from_iter=args.normal_from_iter,
                lambda_dist=args.lambda_dist, dist_from_iter=args.dist_from_iter, depth_ratio=args.depth_ratio,
                lambda_multi_view_geo=args.lambda_multi_view_geo, multi_view_from_iter=args.multi_view_from_iter,
                multi_view_pix_max=args.multi_view_pix_max, lambda_multi_view_ncc=args.lambda_multi_view_ncc,
                multi_view_ncc_samples=args.multi_view_ncc_samples, multi_view_patch_radius=args.multi_view_patch_radius,
                unbiased_depth=args.unbiased_depth, abs_grad=args.abs_grad,
                densify_abs_grad_threshold=args.densify_abs_grad_threshold,
                filter_3d=args.filter_3d, filter_3d_rule=args.filter_3d_rule)


def train_scene(args, dev):
    """``train.py:34-160`` on a dataset: ``Scene`` loads it, a random camera is popped from a copy of the training list
    that is refilled when it empties (:81-83), the model is saved at ``--save_iterations`` and at the end."""
    from mvs_gaussian_splatting_amd import ModelParams, Scene
    dataset = ModelParams(source_path=args.source_path, model_path=args.model_path, images=args.images,
                          resolution=args.resolution, white_background=args.white_background,
                          data_device=args.data_device, eval=args.eval, **({"depths": args.depths} if args.depths else {}),
                          **({"masks": args.masks} if args.masks else {}))
    n = args.iterations
    over = dict(opacitysparse=args.opacitysparse, optimizer_type=args.optimizer_type,
                depth_l1_weight_init=args.depth_l1_weight_init, depth_l1_weight_final=args.depth_l1_weight_final,
                depth_prior_mode=args.depth_prior_mode,
                mask_photometric=not args.no_mask_photometric, mask_normalize=args.mask_normalize,
                lambda_alpha_mask=args.lambda_alpha_mask,
                exposure_lr_init=args.exposure_lr_init, exposure_lr_final=args.exposure_lr_final,
                exposure_lr_delay_steps=args.exposure_lr_delay_steps, exposure_lr_delay_mult=args.exposure_lr_delay_mult,
                **strategy_options(args))
    opt = example_opt(n, **over) if n < 3000 else OptimizationParams(iterations=n, **over)
    model = GaussianModel(dataset.sh_degree)
    scene = Scene(dataset, model, **({"depth_prior_mode": opt.depth_prior_mode} if args.depths else {}))
    with open(os.path.join(args.model_path, "cfg_args.json"), "w") as f:         # what examples/render.py -m needs
        json.dump({k: getattr(dataset, k) for k in ("source_path", "images", "resolution", "white_background", "eval",
                                                    "sh_degree")}, f)
    if args.train_exposure:
        model.setup_exposures([c.image_name for c in scene.getTrainCameras()])
    model.training_setup(opt)
    first_iter = load_checkpoint(model, args.start_checkpoint, opt) if args.start_checkpoint else 0
    grids = None
    if args.bilateral_grid:
        from mvs_gaussian_splatting_amd import BilateralGrids
        grids = BilateralGrids([c.image_name for c in scene.getTrainCameras()], shape=tuple(args.bilateral_grid_shape),
                               device=dev)
        grids.training_setup(opt)
        if args.start_checkpoint:
            grids.load(os.path.join(os.path.dirname(os.path.abspath(args.start_checkpoint)),
                                    f"bilateral_grid_{first_iter}.pt"))
    bg = torch.tensor([1.0, 1.0, 1.0] if dataset.white_background else [0.0, 0.0, 0.0], device=dev)
    pipe, stack, loss = PipelineParams(), None, None
    prune = prune_options(args)
    train_cameras, pose_optimizer = scene.getTrainCameras(), None
    if args.refine_poses:
        from mvs_gaussian_splatting_amd import PoseCamera
        train_cameras = [PoseCamera(c) for c in train_cameras]
        pose_optimizer = torch.optim.Adam([p for c in train_cameras for p in c.parameters()], lr=args.pose_lr)
    sources = source_views(train_cameras, opt, args.multi_view_sources)
    for iteration in range(first_iter + 1, n + 1):
        if not stack:
            stack = list(range(len(train_cameras)))
        index = stack.pop(random.randint(0, len(stack) - 1))
        source = draw_source(train_cameras, sources, index, random)
        loss = training_iteration(model, train_cameras[index], opt, pipe, bg, iteration, dataset=dataset,
                                  cameras_extent=scene.cameras_extent, pose_optimizer=pose_optimizer,
                                  train_exposure=args.train_exposure,
                                  **({"bilateral_grids": grids} if grids is not None else {}),
                                  **({"filter_cameras": train_cameras} if args.filter_3d else {}),
                                  **({"source_camera": source} if source is not None else {}))
        prune_step(model, train_cameras, pipe, bg, iteration, prune)
        if iteration % 10 == 0:
            print(f"iteration {iteration}: loss {float(loss):.5f}  points {model._xyz.shape[0]}")
        if iteration in args.save_iterations or iteration == n:
            scene.save(iteration)
            print(f"[ITER {iteration}] saved the Gaussians under {args.model_path}")
        if iteration in args.checkpoint_iterations:
            save_checkpoint(model, iteration, os.path.join(args.model_path, f"chkpnt{iteration}.pth"))
            if grids is not None:
                grids.save(os.path.join(args.model_path, f"bilateral_grid_{iteration}.pt"))
    if args.refine_poses:
        poses = {c.image_name: dict(zip(("R", "T"), (a.tolist() for a in c.pose()))) for c in train_cameras}
        with open(os.path.join(args.model_path, "refined_poses.json"), "w") as f:
            json.dump(poses, f)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-s", "--source_path", default=None)
    ap.add_argument("-m", "--model_path", default=None)
    ap.add_argument("--images", default="images")
    ap.add_argument("-r", "--resolution", type=int, default=-1)
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--data_device", default="cuda")
    ap.add_argument("--save_iterations", type=int, nargs="*", default=[])
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--checkpoint_iterations", type=int, nargs="*", default=[])
    ap.add_argument("--start_checkpoint", default=None)
    ap.add_argument("--opacitysparse", type=float, default=0.0)
    ap.add_argument("--optimizer_type", choices=("default", "sparse_adam"), default="default",
                    help="sparse_adam: step only the Gaussians each frame saw (optim.SparseGaussianAdam)")
    ap.add_argument("--refine_poses", action="store_true", help="with -s: refine the training cameras' poses too")
    ap.add_argument("--pose_lr", type=float, default=1e-4)
    ap.add_argument("--train_exposure", action="store_true",
                    help="with -s: learn a 3x4 colour affine per training image (saved as exposure.json)")
    ap.add_argument("--exposure_lr_init", type=float, default=OptimizationParams.exposure_lr_init)
    ap.add_argument("--exposure_lr_final", type=float, default=OptimizationParams.exposure_lr_final)
    ap.add_argument("--exposure_lr_delay_steps", type=int, default=OptimizationParams.exposure_lr_delay_steps)
    ap.add_argument("--exposure_lr_delay_mult", type=float, default=OptimizationParams.exposure_lr_delay_mult)
    ap.add_argument("--bilateral_grid", action="store_true",
                    help="with -s: learn a bilateral grid of colour affines per training image (bilateral_grid_<N>.pt)")
    ap.add_argument("--bilateral_grid_shape", type=int, nargs=3, default=[16, 16, 8], metavar=("W", "H", "L"))
    ap.add_argument("--prune_iterations", type=int, nargs="*", default=[],
                    help="after these iterations: measure every training view and prune by contribution")
    ap.add_argument("--prune_keep_ratio", type=float, default=None, help="share of the Gaussians a pruning keeps")
    ap.add_argument("--prune_kind", choices=("sum", "max", "count", "mean"), default="sum")
    ap.add_argument("--strategy", choices=("default", "mcmc"), default="default",
                    help="mcmc: relocation, 5 %% growth up to --cap_max, position noise, opacity / scale priors (mcmc.py)")
    ap.add_argument("--cap_max", type=int, default=OptimizationParams.cap_max, help="with --strategy mcmc: the budget")
    ap.add_argument("--noise_lr", type=float, default=OptimizationParams.noise_lr)
    ap.add_argument("--opacity_reg", type=float, default=OptimizationParams.opacity_reg)
    ap.add_argument("--scale_reg", type=float, default=OptimizationParams.scale_reg)
    ap.add_argument("--lambda_normal", type=float, default=OptimizationParams.lambda_normal,
                    help="weight of the depth-normal consistency term (normal_consistency.py); 2DGS uses 0.05; 0: off")
    ap.add_argument("--normal_from_iter", type=int, default=OptimizationParams.normal_from_iter,
                    help="first iteration the term joins the loss at (2DGS: 7000)")
    ap.add_argument("--depth_ratio", type=float, default=OptimizationParams.depth_ratio,
                    help="with --lambda_normal: the share of the median depth in the surface the term differentiates "
                         "(2DGS: 0 unbounded, 1 bounded)")
    ap.add_argument("--lambda_dist", type=float, default=OptimizationParams.lambda_dist,
                    help="weight of the depth-distortion term (the rasterizer's distortion map); 2DGS uses 100 to 1000; 0: off")
    ap.add_argument("--dist_from_iter", type=int, default=OptimizationParams.dist_from_iter,
                    help="first iteration the term joins the loss at (2DGS: 3000)")
    ap.add_argument("--lambda_multi_view_geo", type=float, default=OptimizationParams.lambda_multi_view_geo,
                    help="weight of the multi-view geometric term (mvs.multi_view_geo_loss; PGSR's); 0: off")
    ap.add_argument("--multi_view_sources", type=int, default=4,
                    help="with --lambda_multi_view_geo: source views per view (select_source_views), one drawn an iteration")
    ap.add_argument("--multi_view_from_iter", type=int, default=OptimizationParams.multi_view_from_iter,
                    help="first iteration the term joins the loss at (PGSR: 7000)")
    ap.add_argument("--multi_view_pix_max", type=float, default=OptimizationParams.multi_view_pix_max,
                    help="reprojection error, in pixels, below which a pixel takes part in the term (PGSR: 1)")
    ap.add_argument("--lambda_multi_view_ncc", type=float, default=OptimizationParams.lambda_multi_view_ncc,
                    help="weight of the multi-view photometric (NCC) term (mvs.multi_view_ncc_loss; PGSR: 0.15); 0: off")
    ap.add_argument("--multi_view_ncc_samples", type=int, default=OptimizationParams.multi_view_ncc_samples,
                    help="with --lambda_multi_view_ncc: pixels drawn per iteration (PGSR: 102400)")
    ap.add_argument("--multi_view_patch_radius", type=int, default=OptimizationParams.multi_view_patch_radius,
                    help="with --lambda_multi_view_ncc: the patch is (2R+1)^2 pixels, R in 1..4 (PGSR: 3)")
    ap.add_argument("--unbiased_depth", action="store_true",
                    help="with --lambda_normal or a multi-view term: they see PGSR's unbiased plane depth "
                         "(render(return_plane_depth=True)) instead of the expected depth")
    ap.add_argument("--abs_grad", action="store_true",
                    help="absolute-gradient densification (AbsGS / PGSR): a large Gaussian is also split when its "
                         "accumulated absolute view-space gradient reaches --densify_abs_grad_threshold")
    ap.add_argument("--densify_abs_grad_threshold", type=float, default=0.0008, metavar="T")
    ap.add_argument("--filter_3d", action="store_true",
                    help="Mip-Splatting's 3D smoothing filter: band-limit every Gaussian by the training cameras' sampling "
                         "rate; the saved PLY carries a filter_3D property (examples/render.py --fuse_filter bakes it in)")
    ap.add_argument("--filter_3d_rule", choices=("mip_splatting", "paper"), default="mip_splatting",
                    help="the filter's width: the published code's (min depth / max focal) or the paper's (1 / max rate)")
    ap.add_argument("-d", "--depths", default="", metavar="DIR",
                    help="with -s: the folder of 16-bit inverse-depth PNGs under the scene, one per training image "
                         "(upstream 3DGS's -d); adds the depth-prior term (depth_prior.py)")
    ap.add_argument("--depth_l1_weight_init", type=float, default=OptimizationParams.depth_l1_weight_init)
    ap.add_argument("--depth_l1_weight_final", type=float, default=OptimizationParams.depth_l1_weight_final)
    ap.add_argument("--depth_prior_mode", choices=("l1", "aligned_l1", "pearson"),
                    default=OptimizationParams.depth_prior_mode,
                    help="with -d: l1 is upstream's term and needs sparse/0/depth_params.json; aligned_l1 and pearson fit "
                         "the scale and shift per frame")
    ap.add_argument("--masks", default="", metavar="DIR",
                    help="with -s: the folder of per-image mask PNGs (non-zero keeps the pixel), under the scene or "
                         "absolute; trains under them (masked_loss.py)")
    ap.add_argument("--mask_normalize", choices=("image", "mask"), default=OptimizationParams.mask_normalize,
                    help="with --masks: divide the masked colour loss by the image's size (upstream 3DGS, gsplat) or by "
                         "the mask's area")
    ap.add_argument("--no_mask_photometric", action="store_true",
                    help="with --masks: leave the colour loss unmasked (the masks then feed only --lambda_alpha_mask "
                         "and the depth prior)")
    ap.add_argument("--lambda_alpha_mask", type=float, default=OptimizationParams.lambda_alpha_mask, metavar="L",
                    help="with --masks: weight of the rendered opacity's cross-entropy against the mask; 0: off")
    ap.add_argument("--out", default=os.path.dirname(os.path.abspath(__file__)))
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if args.source_path:
        if not args.model_path:
            ap.error("-s needs -m, the directory the model is saved under")
        return train_scene(args, dev)
    n = args.iterations
    opt = example_opt(n, opacitysparse=args.opacitysparse, optimizer_type=args.optimizer_type, **strategy_options(args))
    dataset = types.SimpleNamespace(white_background=False)
    problem = make_problem(dev)
    model = make_model(problem, opt, dataset)
    first_iter = 0
    if args.start_checkpoint:
        first_iter = load_checkpoint(model, args.start_checkpoint, opt)
        print(f"resumed from {args.start_checkpoint} at iteration {first_iter}")
    os.makedirs(args.out, exist_ok=True)

    def on_iteration(iteration, m):
        if iteration in args.checkpoint_iterations:
            path = os.path.join(args.out, f"chkpnt{iteration}.pth")
            save_checkpoint(m, iteration, path)
            print(f"[ITER {iteration}] saved checkpoint {path}")

    losses = train(model, problem, opt, first_iter, dataset=dataset, log=print, on_iteration=on_iteration,
                   prune=prune_options(args), multi_view_sources=args.multi_view_sources)
    ply = os.path.join(args.out, "point_cloud.ply")
    model.save_ply(ply)
    if losses:
        print(f"loss {float(losses[0]):.5f} -> {float(losses[-1]):.5f}; {model._xyz.shape[0]} Gaussians; wrote {ply}")


if __name__ == "__main__":
    main()
