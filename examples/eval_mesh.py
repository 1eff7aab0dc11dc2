"""Score a mesh against ground-truth points: DTU's Chamfer distance (accuracy, completeness, their mean) and the
Tanks-and-Temples precision / recall / F-score, on the HIP path (``mvs_gaussian_splatting_amd/geometry_eval.py``;
DESIGN.md §7.19).

    python examples/eval_mesh.py --mesh M.ply --gt G.ply [--samples N] [--tau T ...] [--max_dist D] [--seed S]
                                 [--align T.txt] [--crop crop.json] [--icp --dtau D] [--down_sample V]

``M.ply`` is a triangle mesh as ``examples/extract_mesh.py`` writes it (``tsdf_mesh.ply`` / ``tsdf_mesh_post.ply``); ``G.ply``
is a point cloud with x, y, z (a scanner's cloud, or a ``points3D.ply``).  The mesh is sampled at ``--samples`` points
(default 1 000 000; area-weighted, stratified, seeded by ``--seed``), every sample finds its exact nearest ground-truth
point and every ground-truth point its nearest sample.  ``--max_dist`` leaves larger distances out of the means, as DTU's
script does (20 there, in mm).  The result is printed and written as ``results_mesh.json`` next to the mesh.

What the protocols do before they measure, each on request; with none of these flags the output is what
it always was.  ``--align T.txt``: a 4x4 similarity (16 numbers, row-major) applied to the mesh first, e.g. the trajectory
alignment.  ``--crop crop.json``: the scene's crop volume (Open3D's ``SelectionPolygonVolume`` JSON); the samples and the
ground truth are cropped by it.  ``--icp --dtau D``: the alignment is refined by the staged point-to-point ICP with scale
of the Tanks-and-Temples protocol for the scene's ``dTau`` (``geometry_eval.register_tnt``; its default stages are written
down from memory of the toolbox) and the JSON also carries the final transformation, fitness and RMSE.
``--down_sample V``: both clouds are voxel-down-sampled to ``V`` before scoring (TnT: ``dTau / 2``).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd.geometry_eval import (crop_points, evaluate_mesh, evaluate_points,  # noqa: E402
                                                      load_crop_volume, register_tnt, sample_surface, transform_points)
from mvs_gaussian_splatting_amd.ply_io import read_ply_mesh, read_ply_vertices  # noqa: E402


def evaluate(mesh_path, gt_path, samples=1_000_000, taus=(), max_dist=None, seed=0, device="cuda"):
    vertices, faces, _ = read_ply_mesh(mesh_path)
    gt, _ = read_ply_vertices(gt_path)
    gt = np.stack([np.asarray(gt[n], dtype=np.float32) for n in ("x", "y", "z")], axis=1)
    generator = torch.Generator(device="cpu").manual_seed(seed)
    res = evaluate_mesh(torch.from_numpy(np.ascontiguousarray(vertices)).to(device),
                        torch.from_numpy(np.ascontiguousarray(faces)).to(device), torch.from_numpy(gt).to(device), samples,
                        thresholds=taus, max_dist=max_dist, generator=generator)
    res.update({"mesh": os.path.abspath(mesh_path), "gt": os.path.abspath(gt_path), "seed": seed,
                "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0])})
    return res


def evaluate_registered(mesh_path, gt_path, samples=1_000_000, taus=(), max_dist=None, seed=0, device="cuda", align=None,
                        crop=None, icp=False, dtau=None, down_sample=None):
    """``evaluate`` with the steps of the protocols in front: align, crop, refine by ICP, down-sample."""
    vertices, faces, _ = read_ply_mesh(mesh_path)
    gt, _ = read_ply_vertices(gt_path)
    gt = torch.from_numpy(np.stack([np.asarray(gt[n], dtype=np.float32) for n in ("x", "y", "z")], axis=1)).to(device)
    generator = torch.Generator(device="cpu").manual_seed(seed)
    points, _ = sample_surface(torch.from_numpy(np.ascontiguousarray(vertices)).to(device),
                               torch.from_numpy(np.ascontiguousarray(faces)).to(device), samples, generator)
    T = np.eye(4) if align is None else np.loadtxt(align, dtype=np.float64).reshape(4, 4)
    volume = None if crop is None else load_crop_volume(crop)
    extra = {}
    if icp:
        reg = register_tnt(points, gt, T, volume, dtau)
        T = reg.transformation
        extra["icp"] = {"fitness": reg.fitness, "inlier_rmse": reg.inlier_rmse, "iterations": reg.iterations,
                        "converged": bool(reg.converged), "dtau": dtau}
    if align is not None or icp:
        points = transform_points(points, T)
        extra["transformation"] = [[float(x) for x in row] for row in T]
    if volume is not None:
        points, gt = crop_points(points, volume), crop_points(gt, volume)
    res = evaluate_points(points, gt, taus, max_dist, down_sample=down_sample)
    res.update({"n_samples": int(samples), "mesh": os.path.abspath(mesh_path), "gt": os.path.abspath(gt_path), "seed": seed,
                "vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]), "align": align, "crop": crop,
                "down_sample": down_sample})
    res.update(extra)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mesh", required=True, help="triangle mesh (PLY)")
    ap.add_argument("--gt", required=True, help="ground-truth point cloud (PLY with x, y, z)")
    ap.add_argument("--samples", type=int, default=1_000_000, help="points sampled on the mesh")
    ap.add_argument("--tau", type=float, nargs="*", default=[], help="distance thresholds of precision / recall / F-score")
    ap.add_argument("--max_dist", type=float, default=None, help="leave larger distances out of the means (DTU: 20)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--align", default=None, help="text file with a 4x4 similarity applied to the mesh first")
    ap.add_argument("--crop", default=None, help="crop volume (SelectionPolygonVolume JSON) applied to both clouds")
    ap.add_argument("--icp", action="store_true", help="refine the alignment by staged ICP with scale (needs --dtau)")
    ap.add_argument("--dtau", type=float, default=None, help="the scene's dTau, which sizes the ICP stages")
    ap.add_argument("--down_sample", type=float, default=None, help="voxel size both clouds are down-sampled to")
    args = ap.parse_args(argv)
    if args.samples < 1:
        ap.error("--samples must be positive")
    if any(not (t > 0 and np.isfinite(t)) for t in args.tau) or len(set(args.tau)) != len(args.tau):
        ap.error("--tau takes distinct finite positive distances")
    if args.max_dist is not None and not (args.max_dist > 0 and np.isfinite(args.max_dist)):
        ap.error("--max_dist must be finite and positive")
    if args.icp != (args.dtau is not None):
        ap.error("--icp and --dtau come together")
    for name in ("dtau", "down_sample"):
        v = getattr(args, name)
        if v is not None and not (v > 0 and np.isfinite(v)):
            ap.error(f"--{name} must be finite and positive")
    for path in (args.mesh, args.gt, args.align, args.crop):
        if path is not None and not os.path.isfile(path):
            ap.error(f"{path}: no such file")
    if args.align is None and args.crop is None and not args.icp and args.down_sample is None:
        res = evaluate(args.mesh, args.gt, args.samples, tuple(args.tau), args.max_dist, args.seed)
    else:
        res = evaluate_registered(args.mesh, args.gt, args.samples, tuple(args.tau), args.max_dist, args.seed,
                                  align=args.align, crop=args.crop, icp=args.icp, dtau=args.dtau,
                                  down_sample=args.down_sample)
        if "icp" in res:
            print(f"ICP: {res['icp']['iterations']} iterations, fitness {res['icp']['fitness']:.4f}, "
                  f"inlier RMSE {res['icp']['inlier_rmse']:.6g}")
    print(f"{res['n_pred']} samples of {res['faces']} faces against {res['n_gt']} ground-truth points")
    print(f"accuracy {res['accuracy']:.6g}  completeness {res['completeness']:.6g}  chamfer {res['chamfer']:.6g}"
          + (f"  (beyond {args.max_dist:g}: {100 * res['dropped_pred']:.2f} % of the samples, "
             f"{100 * res['dropped_gt']:.2f} % of the ground truth)" if args.max_dist is not None else ""))
    for t in res["thresholds"]:
        print(f"tau {t['tau']:g}: precision {t['precision']:.4f}  recall {t['recall']:.4f}  F-score {t['fscore']:.4f}")
    out = os.path.join(os.path.dirname(os.path.abspath(args.mesh)), "results_mesh.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=2)
    print("-> " + out)
    return res


if __name__ == "__main__":
    main()
