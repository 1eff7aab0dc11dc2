"""Times one optimizer step at C4 (6 M Gaussians) for the reference's group sets: the six plain groups (SH 3, 59 floats
per Gaussian) and the fork's 128-direction model (+ dirs_prob, grow_dist, split_distance, split_scale: 192 floats).

Three optimizers over the same tensors: mvs_gaussian_splatting_amd.optim.Adam (csrc/adam.hip), torch.optim.Adam's default
(foreach) and torch.optim.Adam(fused=True).  Device events around each step after warm-up; the median is reported with
the achieved rate on the least-traffic model of 28 B per element (read grad, param, exp_avg, exp_avg_sq; write the last
three) against 6.3 TB/s achievable and 8 TB/s peak HBM.

    python tools/bench_adam.py [--points 6000000] [--steps 20] [--warmup 5] [--sets plain,fork] [--only hip,foreach,fused]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import optim  # noqa: E402

BYTES_PER_ELEMENT = 28
ACHIEVABLE_TBS, PEAK_TBS = 6.3, 8.0
WIDTHS = {
    "plain": {"xyz": 3, "f_dc": 3, "f_rest": 45, "opacity": 1, "scaling": 3, "rotation": 4},
}
WIDTHS["fork"] = dict(WIDTHS["plain"], dirs_prob=128, grow_dist=1, split_distance=3, split_scale=1)
LRS = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 1.25e-4, "opacity": 0.05, "scaling": 5e-3, "rotation": 1e-3,
       "dirs_prob": 5e-3, "grow_dist": 1e-3, "split_distance": 5e-3, "split_scale": 5e-3}


def make(kind, params):
    groups = [{"params": [p], "lr": LRS[k], "name": k} for k, p in params.items()]
    if kind == "hip":
        return optim.Adam(groups, lr=0.0, eps=1e-15)
    if kind == "foreach":
        return torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    return torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True)


def time_steps(opt, steps, warmup):
    for _ in range(warmup):
        opt.step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        opt.step()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=6_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", default="plain,fork")
    ap.add_argument("--only", default="hip,foreach,fused")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.sets.split(","):
        widths = WIDTHS[name]
        params = {k: torch.nn.Parameter(torch.randn(args.points, w, device=dev, generator=g)) for k, w in widths.items()}
        for p in params.values():
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
        elements = sum(p.numel() for p in params.values())
        gb = BYTES_PER_ELEMENT * elements / 1e9
        for kind in args.only.split(","):
            opt = make(kind, params)
            ms = time_steps(opt, args.steps, args.warmup)
            med = statistics.median(ms)
            tbs = gb / med                                   # GB / ms = TB/s
            print(json.dumps({"set": name, "optimizer": kind, "points": args.points, "floats_per_row": sum(widths.values()),
                              "elements": elements, "model_GB": round(gb, 3), "median_ms": round(med, 4),
                              "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "TBps_28B": round(tbs, 3),
                              "of_achievable": round(tbs / ACHIEVABLE_TBS, 3), "of_peak": round(tbs / PEAK_TBS, 3)}),
                  flush=True)
            del opt
            torch.cuda.empty_cache()
        del params
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
