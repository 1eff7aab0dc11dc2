"""Device time of the per-Gaussian planes kernel (csrc/planes.hip) and the plane-depth kernel (csrc/plane_depth.hip;
DESIGN.md §7.24), forward plus backward, beside the same quantities written in torch ops in the same run, from HIP events.

    PYTHONPATH=.:tools python tools/bench_planes.py [--iters 20] [--rounds 3] [--points 6000000] [--parent DIR]

``gaussian_planes`` at P rows (default 6 M, the bench frame's) against ``features.gaussian_normals`` plus the distance
``n_world . (campos - mean)`` in torch ops, both under a random upstream gradient; ``surface.plane_depth`` at 1920 x 1080
against its torch-op form (rays, the dot product, the validity mask, ``torch.where``) under autograd.  Reported: ms per
forward + backward, the bytes each kernel must move (forward 56 and backward 84 per row; forward 40 and backward 32 per
pixel) and the rate that is of the best round, and how far the two sides agree.

``--parent DIR`` (a checkout of the parent commit with its library built: ``git worktree add DIR HEAD~1 && make -C
DIR/mvs_gaussian_splatting_amd/csrc``) first runs ``bench.py --gpus 1 --steps 20 --warmup 3`` in DIR and in this tree,
alternating ``--ab-runs`` (3) times, each run a process of its own started before this one touches the GPU, and reports
every run's Mpixels/s and train-step ms: no existing kernel moved if this tree sits within the parent's own spread.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

from mvs_gaussian_splatting_amd import gaussian_planes, plane_depth
from mvs_gaussian_splatting_amd.features import _rotation_matrices

from bench_mvs import timed


def torch_planes(scales, rotations, means3D, viewmatrix, campos):
    """``gaussian_normals`` and the distance channel in torch ops -> [P,4]."""
    R = _rotation_matrices(rotations)
    axis = torch.argmin(scales.detach(), dim=1)
    n = torch.gather(R, 2, axis.view(-1, 1, 1).expand(-1, 3, 1)).squeeze(2)
    to_cam = campos.view(1, 3) - means3D
    facing = (n.detach() * to_cam.detach()).sum(dim=1)
    n = n * torch.where(facing < 0, -1.0, 1.0).to(n.dtype).unsqueeze(1)
    return torch.cat([n @ viewmatrix[:3, :3], (n * to_cam).sum(dim=1, keepdim=True)], dim=1)


def torch_plane_depth(normal, distance, alpha, tanfovx, tanfovy, alpha_min=0.5, min_cos=0.05):
    H, W = distance.shape[-2:]
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    ys, xs = torch.meshgrid(torch.arange(H, device=normal.device, dtype=torch.float32),
                            torch.arange(W, device=normal.device, dtype=torch.float32), indexing="ij")
    rx, ry = (xs - (W - 1) * 0.5) / fx, (ys - (H - 1) * 0.5) / fy
    c = -(normal[0] * rx + normal[1] * ry + normal[2])
    D, A = distance.view(H, W), alpha.view(H, W)
    bound = min_cos * normal.detach().norm(dim=0) * torch.sqrt(rx * rx + ry * ry + 1.0)
    valid = (A >= alpha_min) & (D.detach() > 0) & (c.detach() > 0) & (c.detach() >= bound)
    return torch.where(valid, D / torch.where(valid, c, torch.ones_like(c)), torch.zeros_like(c))[None]


def bench(iters, rounds, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    scales = torch.exp(torch.randn(P, 3, device=dev, generator=g) * 0.7 - 3.0)
    rot = torch.randn(P, 4, device=dev, generator=g)
    means = torch.randn(P, 3, device=dev, generator=g) * 2.0 + torch.tensor([0.0, 0.0, 5.0], device=dev)
    vm = torch.eye(4, device=dev)
    campos = torch.tensor([0.3, -0.2, -1.0], device=dev)
    up = torch.randn(P, 4, device=dev, generator=g)
    out = {"points": P}

    def run(fn):
        def step():
            q, m = rot.detach().requires_grad_(True), means.detach().requires_grad_(True)
            fn(scales, q, m, vm, campos).backward(up)
            return q.grad, m.grad
        return step
    results = {}
    for name, fn in (("kernel", gaussian_planes), ("torch", torch_planes)):
        step = run(fn)
        timed(step, 2)
        ms = [timed(step, iters) for _ in range(rounds)]
        results[name] = step()
        out[f"planes_fwd_bwd_ms ({name})"] = [round(x, 4) for x in ms]
        print(f"planes forward + backward, {name}, P = {P}: {min(ms):.4f} ms" +
              (f", {P * 140 / min(ms) / 1e6:.0f} GB/s on {P * 140 / 1e6:.0f} MB" if name == "kernel" else ""))
        torch.cuda.empty_cache()
    rel = lambda a, b: float((a - b).double().norm() / b.double().norm())      # noqa: E731
    out["planes agreement (rel l2 of dL/drotations, dL/dmeans3D)"] = [rel(a, b) for a, b in zip(results["kernel"], results["torch"])]
    del results

    H, W, tan = 1080, 1920, (0.8, 0.45)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    n = torch.stack([0.45 + 0.05 * torch.sin(xs / 90.0), 0.2 + 0.05 * torch.cos(ys / 70.0), -torch.ones_like(xs)])
    alpha = (0.75 + 0.2 * torch.sin(xs / 50.0 + ys / 40.0))[None].contiguous()
    normal = (n / n.norm(dim=0, keepdim=True) * alpha).contiguous()
    distance = ((3.0 + 0.1 * torch.sin(xs / 120.0)) * alpha[0])[None].contiguous()
    upz = torch.randn(1, H, W, device=dev, generator=g)
    results = {}
    for name, fn in (("kernel", plane_depth), ("torch", torch_plane_depth)):
        def step():
            nm, d = normal.detach().requires_grad_(True), distance.detach().requires_grad_(True)
            z = fn(nm, d, alpha, *tan)
            z.backward(upz)
            return z.detach(), nm.grad, d.grad
        timed(step, 2)
        ms = [timed(step, iters) for _ in range(rounds)]
        results[name] = step()
        out[f"plane_depth_fwd_bwd_ms ({name})"] = [round(x, 4) for x in ms]
        print(f"plane depth forward + backward, {name}, {W} x {H}: {min(ms):.4f} ms" +
              (f", {H * W * 72 / min(ms) / 1e6:.0f} GB/s on {H * W * 72 / 1e6:.0f} MB" if name == "kernel" else ""))
    out["plane_depth agreement (rel l2 of z, dL/dnormal, dL/ddistance)"] = [rel(a, b) for a, b in
                                                                           zip(results["kernel"], results["torch"])]
    return out


def headline_ab(parent, runs):
    """``bench.py``'s headline frame in ``parent`` and in this tree, alternating: -> {"parent": [...], "this": [...]} of
    (Mpixels/s, train-step ms, first timed forward step ms) per run."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {"parent": [], "this": []}
    for i in range(runs):
        for name, tree in (("parent", os.path.abspath(parent)), ("this", here)):
            env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "GSR_LIB_PATH")}
            done = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], cwd=tree,
                                  env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=600,
                                  check=True)
            line = json.loads(done.stdout.strip().splitlines()[-1])
            out[name].append((line["value"], line["ms_per_step"], line["fwd_step_ms_in_order"][0]))
            print(f"bench.py, {name}, run {i + 1}: {line['value']} Mpixels/s, {line['ms_per_step']} ms per train step, "
                  f"first timed forward step {line['fwd_step_ms_in_order'][0]} ms", flush=True)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--points", type=int, default=6_000_000)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: also run bench.py there and here")
    ap.add_argument("--ab-runs", type=int, default=3)
    args = ap.parse_args(argv)
    ab = None
    if args.parent is not None:                            # before this process opens the GPU
        if not os.path.exists(os.path.join(args.parent, "bench.py")):
            raise SystemExit(f"--parent: no bench.py under {args.parent}")
        ab = headline_ab(args.parent, args.ab_runs)
    if not torch.cuda.is_available():
        raise SystemExit("bench_planes needs a GPU: a CPU run measures nothing")
    out = bench(args.iters, args.rounds, args.points, torch.device("cuda:0"))
    if ab is not None:
        out["bench.py (Mpixels/s, train ms, first forward ms)"] = ab
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
