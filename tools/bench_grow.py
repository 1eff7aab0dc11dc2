"""Cost of the fork's grow / learned-split branch at C4 (6 M Gaussians, 1920x1080): forward and train step with the gate
open (about 2 % and 10 % of the rows selected, so G ~ 0.12 M / 0.6 M virtual rows) against the same frame with the gate
closed, and the expand / fold passes alone.  Prints one JSON line per measurement.

    python tools/bench_grow.py [--steps 20] [--warmup 5] [--gaussians 6000000]
"""
import argparse
import json
import math
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvs_gaussian_splatting_amd import grow, l1_loss, render  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene  # noqa: E402

OPT = types.SimpleNamespace(densify_from_iter=500, densification_interval=100, densify_until_iter=15000,
                            opacity_reset_interval=3000)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--gaussians", type=int, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model, cam, bg, target = make_scene(CONFIGS["C4"], seed=0, device=dev, P=args.gaussians)
    P = model._xyz.shape[0]
    g = torch.Generator(device=dev).manual_seed(1)
    model._dirs_prob = torch.full((P, 128), 1.0 / 128, device=dev)
    model._grow_dist = torch.zeros(P, 1, device=dev)
    n = torch.arange(128, dtype=torch.float64)
    zz = 1 - (2 * n + 1) / 128
    th = math.pi * (3 - math.sqrt(5)) * n
    r = torch.sqrt(1 - zz * zz)
    model.dirs = torch.stack([r * torch.cos(th), r * torch.sin(th), zz], 1).float().to(dev)
    model.denom = torch.ones(P, 1, device=dev)
    u = torch.rand(P, 1, device=dev, generator=g)
    leaves = model.parameters() + [model._dirs_prob, model._grow_dist]
    for t in leaves:
        t.requires_grad_(True)
    target, bg = target.to(dev), bg.to(dev)
    pipe = PipelineParams()
    kw = dict(grow_dir=True, grow_distance=True, densify_grad_threshold=0.5, iteration=4000, opt=OPT)
    closed = dict(kw, iteration=3000)
    out = []
    for frac in (0.02, 0.10):
        model.xyz_gradient_accum = (u < frac).float()          # |accum / denom| >= 0.5 on ~frac of the rows
        G = int(model.xyz_gradient_accum.sum())
        for gate, args_ in (("closed", closed), ("open", kw)):
            def fwd():
                with torch.no_grad():
                    render(cam, model, pipe, bg, **args_)

            def step():
                for t in leaves:
                    t.grad = None
                l1_loss(render(cam, model, pipe, bg, **args_)["render"], target).backward()
            out.append({"frac": frac, "G": G, "gate": gate, "fwd_ms": round(timed(fwd, args.steps, args.warmup), 4),
                        "step_ms": round(timed(step, args.steps, args.warmup), 4)})
            print(json.dumps(out[-1]), flush=True)
        # expand alone and expand + fold alone (no rasterizer)
        m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
        pl = grow.plan(model, grow.mode_bits("grow", grow_dir=True, grow_distance=True), 0.5, math.inf)
        mode = pl.mode

        def expand():
            with torch.no_grad():
                grow.expand(model, m2, mode, 0.5, math.inf, pl=pl)

        def expand_fold():
            _, ext = grow.expand(model, m2, mode, 0.5, math.inf, pl=pl)
            torch.autograd.backward([ext[0], ext[2], ext[3]], [torch.ones_like(ext[0]), torch.ones_like(ext[2]),
                                                              torch.ones_like(ext[3])])
        e_ms = timed(expand, args.steps, args.warmup)
        ef_ms = timed(expand_fold, args.steps, args.warmup)
        moved = 2 * (P + G) * 59 * 4                            # every extended raw float read once and written once
        print(json.dumps({"frac": frac, "G": G, "plan_expand_ms": round(e_ms, 4), "expand_fold_ms": round(ef_ms, 4),
                          "expand_bytes": moved, "expand_GBps": round(moved / e_ms / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
