"""Make a trained scene smaller: measure how much every Gaussian contributes to the training views and drop the tail.

    python examples/prune.py -m <model directory> [--iteration I] (--keep_ratio R | --min_score S)
                             [--kind sum|max|count|mean] [--save_iteration J]
                             [-s <COLMAP or Blender directory>] [-r ...] [--white_background]

Loads the Gaussians ``examples/train.py -s ... -m ...`` saved (the latest iteration by default), renders every training
camera once with ``render(..., contribution=stats)`` (``contribution.measure``: the per-Gaussian sum, count and maximum of
the blending weights, accumulated on the device), keeps the ``--keep_ratio`` share with the highest ``--kind`` score --
or every Gaussian whose score reaches ``--min_score`` -- and saves the result as
``<model>/point_cloud/iteration_J/point_cloud.ply`` (default ``J = I + 1``, so that ``examples/render.py -m <model>``
renders the pruned cloud).  An ``exposure.json`` next to the loaded cloud is copied along.  Prints the points before and
after.  ``--kind count --min_score 1`` removes exactly the Gaussians no training view composites.
"""
import argparse
import json
import os
import shutil
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import GaussianModel, ModelParams, Scene, measure, prune_by_contribution  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import PipelineParams  # noqa: E402


def prune_scene(dataset, iteration, kind, keep_ratio=None, min_score=None, save_iteration=None):
    """-> (the scene, ``{"points", "pruned"}``, the iteration the pruned cloud was saved as)."""
    with torch.no_grad():
        gaussians = GaussianModel(dataset.sh_degree)
        scene = Scene(dataset, gaussians, load_iteration=iteration, shuffle=False)
        background = torch.tensor([1.0, 1.0, 1.0] if dataset.white_background else [0.0, 0.0, 0.0], device="cuda")
        stats = measure(gaussians, scene.getTrainCameras(), PipelineParams(), background)
        out = prune_by_contribution(gaussians, stats, kind=kind, keep_ratio=keep_ratio, min_score=min_score)
        target = scene.loaded_iter + 1 if save_iteration is None else save_iteration
        scene.save(target)
        loaded = os.path.join(dataset.model_path, "point_cloud", f"iteration_{scene.loaded_iter}", "exposure.json")
        if os.path.exists(loaded) and target != scene.loaded_iter:
            shutil.copy(loaded, os.path.join(dataset.model_path, "point_cloud", f"iteration_{target}", "exposure.json"))
    return scene, out, target


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-s", "--source_path", default=None)
    ap.add_argument("-m", "--model_path", required=True)
    ap.add_argument("--images", default=None)
    ap.add_argument("-r", "--resolution", type=int, default=None)
    ap.add_argument("--eval", action="store_true", default=None)
    ap.add_argument("--white_background", action="store_true", default=None)
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--save_iteration", type=int, default=None)
    ap.add_argument("--kind", choices=("sum", "max", "count", "mean"), default="sum")
    how = ap.add_mutually_exclusive_group(required=True)
    how.add_argument("--keep_ratio", type=float, default=None, help="share of the Gaussians to keep, best first")
    how.add_argument("--min_score", type=float, default=None, help="keep the Gaussians whose score is at least this")
    args = ap.parse_args(argv)
    fields = {}
    cfg = os.path.join(args.model_path, "cfg_args.json")
    if os.path.exists(cfg):
        with open(cfg) as f:
            fields = json.load(f)
    for k in ("source_path", "images", "resolution", "eval", "white_background"):
        if getattr(args, k) is not None:
            fields[k] = getattr(args, k)
    if not fields.get("source_path"):
        ap.error("no cfg_args.json in the model directory: give the dataset with -s")
    dataset = ModelParams(model_path=args.model_path, **fields)
    scene, out, target = prune_scene(dataset, args.iteration, args.kind, args.keep_ratio, args.min_score,
                                     args.save_iteration)
    print(f"iteration {scene.loaded_iter}: {out['points'] + out['pruned']} points -> {out['points']} points "
          f"({out['pruned']} pruned by {args.kind}); saved as iteration {target}")


if __name__ == "__main__":
    main()
