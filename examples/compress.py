"""Make a trained scene's file smaller: vector-quantise the Gaussians' attributes against k-means codebooks.

    python examples/compress.py -m <model directory> [--iteration N] [--codebook_size K] [--iters I] [--importance]
                                [--xyz_half] [-s <COLMAP or Blender directory>] [-r ...] [--eval] [--white_background]

Loads ``<model>/point_cloud/iteration_N/point_cloud.ply`` (the latest iteration by default), runs
``compress.compress_model`` (one codebook of ``K`` rows each for f_dc, f_rest, scaling and rotation; positions float32, or
float16 with ``--xyz_half``; opacity float16) and writes ``point_cloud_vq.npz`` beside the PLY.  With ``--importance``
every Gaussian is weighted by the sum of its blending weights over the training views (``contribution.measure``:
LightGaussian's weighting), which needs the scene's cameras.  Prints both file sizes and, when the cameras are there, the
PSNR / SSIM of the original and of the decoded model over the test views (the training views if the scene has no test
split).  ``examples/render.py -m <model> --point_cloud <...>/point_cloud_vq.npz`` renders the compressed file.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import GaussianModel, ModelParams, Scene, evaluate_views, measure  # noqa: E402
from mvs_gaussian_splatting_amd.compress import compress_model, save_compressed  # noqa: E402
from mvs_gaussian_splatting_amd.scene import searchForMaxIteration  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import PipelineParams  # noqa: E402


def compress_scene(model_path, iteration=-1, codebook_size=4096, iters=10, importance=False, xyz_half=False, dataset=None):
    """-> ``{"ply_bytes", "npz_bytes", "payload_bytes", "points", "path", "original", "decoded"}``; the last two are the
    ``evaluate_views`` results (None without ``dataset``, a ``ModelParams``)."""
    if iteration == -1:
        iteration = searchForMaxIteration(os.path.join(model_path, "point_cloud"))
    folder = os.path.join(model_path, "point_cloud", f"iteration_{iteration}")
    ply, out = os.path.join(folder, "point_cloud.ply"), os.path.join(folder, "point_cloud_vq.npz")
    if importance and dataset is None:
        raise ValueError("--importance measures the training views: give the dataset")
    with torch.no_grad():
        sh_degree = dataset.sh_degree if dataset is not None else 3
        gaussians = GaussianModel(sh_degree)
        scene = None
        if dataset is not None:
            scene = Scene(dataset, gaussians, load_iteration=iteration, shuffle=False)
        else:
            gaussians.load_ply(ply)
        background = torch.tensor([1.0, 1.0, 1.0] if dataset is not None and dataset.white_background else [0.0, 0.0, 0.0],
                                  device="cuda")
        weights = None
        if importance:
            stats = measure(gaussians, scene.getTrainCameras(), PipelineParams(), background)
            weights = stats.score("sum").to(torch.float32)
        cg = compress_model(gaussians, codebook_size=codebook_size, iters=iters, weights=weights,
                            xyz_dtype="float16" if xyz_half else "float32")
        save_compressed(out, cg)
        res = {"ply_bytes": os.path.getsize(ply), "npz_bytes": os.path.getsize(out), "payload_bytes": cg.nbytes(),
               "points": cg.num_points, "path": out, "original": None, "decoded": None}
        if scene is not None:
            views = scene.getTestCameras() or scene.getTrainCameras()
            res["original"] = evaluate_views(views, gaussians, PipelineParams(), background, with_ssim=True)
            decoded = GaussianModel(sh_degree)
            decoded.load_compressed(out)
            res["decoded"] = evaluate_views(views, decoded, PipelineParams(), background, with_ssim=True)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-s", "--source_path", default=None)
    ap.add_argument("-m", "--model_path", required=True)
    ap.add_argument("--images", default=None)
    ap.add_argument("-r", "--resolution", type=int, default=None)
    ap.add_argument("--eval", action="store_true", default=None)
    ap.add_argument("--white_background", action="store_true", default=None)
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--codebook_size", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--importance", action="store_true", help="weight every Gaussian by its contribution to the training views")
    ap.add_argument("--xyz_half", action="store_true", help="store positions as float16")
    args = ap.parse_args(argv)
    fields = {}
    cfg = os.path.join(args.model_path, "cfg_args.json")
    if os.path.exists(cfg):
        with open(cfg) as f:
            fields = json.load(f)
    for k in ("source_path", "images", "resolution", "eval", "white_background"):
        if getattr(args, k) is not None:
            fields[k] = getattr(args, k)
    dataset = ModelParams(model_path=args.model_path, **fields) if fields.get("source_path") else None
    if dataset is None and args.importance:
        ap.error("--importance needs the scene's cameras: no cfg_args.json in the model directory, give the dataset with -s")
    res = compress_scene(args.model_path, args.iteration, args.codebook_size, args.iters, args.importance, args.xyz_half,
                         dataset)
    print(f"{res['points']} Gaussians: {res['ply_bytes']} bytes (PLY) -> {res['npz_bytes']} bytes ({res['path']}; payload "
          f"{res['payload_bytes']}): {res['ply_bytes'] / res['npz_bytes']:.1f} x smaller")
    for name in ("original", "decoded"):
        if res[name] is not None:
            r = res[name]
            print(f"  {name}: PSNR {r['psnr']:.3f} dB, SSIM {r['ssim']:.4f} over {r['n']} views")
    if dataset is None:
        print("  (no cameras: give the dataset with -s to compare image quality)")
    return res


if __name__ == "__main__":
    main()
