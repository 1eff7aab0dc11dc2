"""Score a mesh against ground-truth points: DTU's Chamfer distance (accuracy, completeness, their mean) and the
Tanks-and-Temples precision / recall / F-score, on the HIP path (``mvs_gaussian_splatting_amd/geometry_eval.py``;
DESIGN.md §7.19).

    python examples/eval_mesh.py --mesh M.ply --gt G.ply [--samples N] [--tau T ...] [--max_dist D] [--seed S]

``M.ply`` is a triangle mesh as ``examples/extract_mesh.py`` writes it (``tsdf_mesh.ply`` / ``tsdf_mesh_post.ply``); ``G.ply``
is a point cloud with x, y, z (a scanner's cloud, or a ``points3D.ply``).  The mesh is sampled at ``--samples`` points
(default 1 000 000; area-weighted, stratified, seeded by ``--seed``), every sample finds its exact nearest ground-truth
point and every ground-truth point its nearest sample.  ``--max_dist`` leaves larger distances out of the means, as DTU's
script does (20 there, in mm).  The result is printed and written as ``results_mesh.json`` next to the mesh.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd.geometry_eval import evaluate_mesh  # noqa: E402
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mesh", required=True, help="triangle mesh (PLY)")
    ap.add_argument("--gt", required=True, help="ground-truth point cloud (PLY with x, y, z)")
    ap.add_argument("--samples", type=int, default=1_000_000, help="points sampled on the mesh")
    ap.add_argument("--tau", type=float, nargs="*", default=[], help="distance thresholds of precision / recall / F-score")
    ap.add_argument("--max_dist", type=float, default=None, help="leave larger distances out of the means (DTU: 20)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.samples < 1:
        ap.error("--samples must be positive")
    if any(not (t > 0 and np.isfinite(t)) for t in args.tau) or len(set(args.tau)) != len(args.tau):
        ap.error("--tau takes distinct finite positive distances")
    if args.max_dist is not None and not (args.max_dist > 0 and np.isfinite(args.max_dist)):
        ap.error("--max_dist must be finite and positive")
    for path in (args.mesh, args.gt):
        if not os.path.isfile(path):
            ap.error(f"{path}: no such file")
    res = evaluate(args.mesh, args.gt, args.samples, tuple(args.tau), args.max_dist, args.seed)
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
