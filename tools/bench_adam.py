"""Times one optimizer step at C4 (6 M Gaussians) for the reference's group sets: the six plain groups (SH 3, 59 floats
per Gaussian) and the fork's 128-direction model (+ dirs_prob, grow_dist, split_distance, split_scale: 192 floats).

Three optimizers over the same tensors: mvs_gaussian_splatting_amd.optim.Adam (csrc/adam.hip), torch.optim.Adam's default
(foreach) and torch.optim.Adam(fused=True).  Device events around each step after warm-up; the median is reported with
the achieved rate on the least-traffic model of 28 B per element (read grad, param, exp_avg, exp_avg_sq; write the last
three) against 6.3 TB/s achievable and 8 TB/s peak HBM.

The `sparse` kind is optim.SparseGaussianAdam.step(visibility) (gsr_adam_step_rows) over the same tensors, once per
visibility pattern: all rows; the C4 bench camera's own `radii` from one render() of the bench cloud, as stored and
in Morton order (layout.morton_permutation); seeded random masks and contiguous blocks at 25 % and 5 %.  Its byte
model is 28 B per element of a visible row plus the visibility entry of every row, per tensor; the dense `hip` step of
the same process is the comparison.

    python tools/bench_adam.py [--points 6000000] [--steps 20] [--warmup 5] [--sets plain,fork]
                               [--only hip,foreach,fused,sparse] [--patterns all,camera,...]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import optim  # noqa: E402
from mvs_gaussian_splatting_amd.layout import morton_permutation  # noqa: E402
from mvs_gaussian_splatting_amd.renderer import render  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene  # noqa: E402

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
    if kind == "sparse":
        return optim.SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
    if kind == "foreach":
        return torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    return torch.optim.Adam(groups, lr=0.0, eps=1e-15, fused=True)


PATTERNS = ("all", "camera", "camera_morton", "random25", "random5", "block25", "block5")


def visibility_patterns(points, dev, wanted):
    """name -> visibility tensor [points]: int32 radii for the camera patterns (as render() hands them out), bool masks
    for the others."""
    out = {}
    if "all" in wanted:
        out["all"] = torch.ones(points, dtype=torch.bool, device=dev)
    if "camera" in wanted or "camera_morton" in wanted:
        model, cam, bg, _ = make_scene(CONFIGS["C4"], P=points, device=dev)
        with torch.no_grad():
            radii = render(cam, model, PipelineParams(), bg)["radii"].to(torch.int32).contiguous()
        if "camera" in wanted:
            out["camera"] = radii
        if "camera_morton" in wanted:
            out["camera_morton"] = radii[morton_permutation(model._xyz)].contiguous()
        del model
    g = torch.Generator(device=dev).manual_seed(1)
    for pct in (25, 5):
        if f"random{pct}" in wanted:
            out[f"random{pct}"] = torch.rand(points, device=dev, generator=g) < pct / 100
        if f"block{pct}" in wanted:
            m = torch.zeros(points, dtype=torch.bool, device=dev)
            m[points // 3:points // 3 + points * pct // 100] = True
            out[f"block{pct}"] = m
    return {k: out[k] for k in PATTERNS if k in out}


def time_steps(opt, steps, warmup, visibility=None):
    step = opt.step if visibility is None else (lambda: opt.step(visibility))
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        step()
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
    ap.add_argument("--patterns", default=",".join(PATTERNS), help="visibility patterns of the sparse kind")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam needs a GPU")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    patterns = visibility_patterns(args.points, dev, args.patterns.split(",")) if "sparse" in args.only.split(",") else {}
    for name in args.sets.split(","):
        widths = WIDTHS[name]
        params = {k: torch.nn.Parameter(torch.randn(args.points, w, device=dev, generator=g)) for k, w in widths.items()}
        for p in params.values():
            p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-3
        elements = sum(p.numel() for p in params.values())
        gb = BYTES_PER_ELEMENT * elements / 1e9
        for kind in args.only.split(","):
            opt = make(kind, params)
            if kind == "sparse":
                for pattern, vis in patterns.items():
                    ms = time_steps(opt, args.steps, args.warmup, vis)
                    med = statistics.median(ms)
                    visible = int((vis > 0).sum())
                    sgb = (BYTES_PER_ELEMENT * sum(widths.values()) * visible
                           + vis.element_size() * args.points * len(widths)) / 1e9
                    print(json.dumps({"set": name, "optimizer": kind, "pattern": pattern, "visibility": str(vis.dtype),
                                      "points": args.points, "visible_rows": visible,
                                      "visible_fraction": round(visible / args.points, 4), "model_GB": round(sgb, 4),
                                      "median_ms": round(med, 4), "min_ms": round(min(ms), 4),
                                      "max_ms": round(max(ms), 4), "TBps_model": round(sgb / med, 3),
                                      "of_achievable": round(sgb / med / ACHIEVABLE_TBS, 3)}), flush=True)
                del opt
                torch.cuda.empty_cache()
                continue
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
