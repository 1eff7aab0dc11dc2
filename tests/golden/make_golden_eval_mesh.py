"""Writes the fixtures of the examples/eval_mesh.py regression (tests/test_gpu_icp.py):

    eval_mesh_mesh.ply, eval_mesh_gt.ply    a squashed octahedron and 400 points near its surface (no GPU needed)
    eval_mesh_results.json                  the bytes of results_mesh.json that examples/eval_mesh.py writes for the pair
                                            with ARGS below (needs the GPU), the two absolute paths replaced by @MESH@ / @GT@

    python tests/golden/make_golden_eval_mesh.py [out_dir]      (default: this folder)

The JSON was recorded on the commit before the registration flags were added: without those flags the script must go on
writing exactly these bytes."""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ARGS = ["--samples", "3000", "--tau", "0.05", "0.2", "--max_dist", "0.5", "--seed", "3"]


def write_pair(folder):
    from mvs_gaussian_splatting_amd.ply_io import write_ply_mesh, write_ply_vertices
    v = np.array([[1.5, 0, 0], [-1.5, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 0.5], [0, 0, -0.5]], dtype=np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)
    rng = np.random.default_rng(11)
    tri = v[f[rng.integers(0, 8, size=400)]].astype(np.float64)
    w = rng.dirichlet((1.0, 1.0, 1.0), size=400)
    p = (w[:, :, None] * tri).sum(axis=1) + rng.normal(0.0, 0.03, size=(400, 3))
    gt = np.zeros(400, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
    gt["x"], gt["y"], gt["z"] = p[:, 0], p[:, 1], p[:, 2]
    write_ply_mesh(os.path.join(folder, "eval_mesh_mesh.ply"), v, f)
    write_ply_vertices(os.path.join(folder, "eval_mesh_gt.ply"), gt)


def results_bytes(folder):
    """Run examples/eval_mesh.py on a copy of the pair in a folder of its own -> the bytes of its results_mesh.json with
    the two paths replaced."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("example_eval_mesh", os.path.join(ROOT, "examples", "eval_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as tmp:
        mesh, gt = (shutil.copy(os.path.join(folder, n), tmp) for n in ("eval_mesh_mesh.ply", "eval_mesh_gt.ply"))
        mod.main(["--mesh", mesh, "--gt", gt] + ARGS)
        with open(os.path.join(tmp, "results_mesh.json"), "rb") as fh:
            raw = fh.read()
    for path, tag in ((mesh, "@MESH@"), (gt, "@GT@")):
        quoted = json.dumps(os.path.abspath(path)).encode()
        assert raw.count(quoted) == 1
        raw = raw.replace(quoted, json.dumps(tag).encode())
    return raw


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    os.makedirs(out, exist_ok=True)
    write_pair(out)
    import torch
    if torch.cuda.is_available():
        with open(os.path.join(out, "eval_mesh_results.json"), "wb") as fh:
            fh.write(results_bytes(out))
