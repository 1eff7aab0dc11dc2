"""Cost of the fork's densify_and_prune at C4 size (6 M Gaussians, 128 directions, grow_dir + grow_distance, the grow
branch of scene/gaussian_model.py:755) with about 2 % and 10 % of the rows selected: the HIP path
(mvs_gaussian_splatting_amd.densify) against the float32 torch restatement of tests/densify_fork_restate.py on the same
GPU, which runs the reference's op sequence (boolean-mask gathers, cat, repeat, in-place re-init).  Every timed call
starts from the same model (restored outside the timed region).  Prints one JSON line per measurement.

    python tools/bench_densify_fork.py [--steps 5] [--warmup 1] [--gaussians 6000000] [--hip-only]
"""
import argparse
import json
import math
import os
import sys
import types

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mvs_gaussian_splatting_amd.densify import densify_and_prune  # noqa: E402
from densify_fork_restate import FLAG_NAMES, densify_and_prune as restate  # noqa: E402

ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity",
        "scaling": "_scaling", "rotation": "_rotation", "dirs_prob": "_dirs_prob", "grow_dist": "_grow_dist"}
OPT = types.SimpleNamespace(opacity_reset_interval=3000)
ND = 128


def make(P, frac, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)          # noqa: E731
    params = {"xyz": r(P, 3) * 2.0, "f_dc": r(P, 1, 3), "f_rest": 0.1 * r(P, 15, 3),
              "opacity": 2.5 * r(P, 1) - 1.0, "scaling": math.log(0.01) + 1.2 * r(P, 3), "rotation": r(P, 4),
              "dirs_prob": r(P, ND), "grow_dist": r(P, 1)}
    moments = {k: (r(*t.shape), r(*t.shape).abs()) for k, t in params.items()}
    denom = torch.ones(P, 1, device=dev)
    accum = (torch.rand(P, 1, generator=g, device=dev) < frac).float() * 0.001      # selected: g = 0.001 >= 0.0002
    i = torch.arange(ND, dtype=torch.float64)
    zz = torch.linspace(1 - 1.0 / ND, 1.0 / ND - 1, ND, dtype=torch.float64)
    rr = torch.sqrt(1 - zz * zz)
    th = math.pi * (3 - math.sqrt(5)) * i
    dirs = torch.stack([rr * torch.cos(th), rr * torch.sin(th), zz], 1).float().to(dev)
    return params, moments, accum, denom, dirs


def load_model(m, params, moments, accum, denom, dirs):
    for k, t in params.items():
        setattr(m, ATTR[k], nn.Parameter(t.clone()))
    m.optimizer = torch.optim.Adam([{"params": [getattr(m, ATTR[k])], "lr": 1e-3, "name": k} for k in params],
                                   lr=0.0, eps=1e-15)
    for k in params:
        m.optimizer.state[getattr(m, ATTR[k])] = {"step": torch.tensor(1.0), "exp_avg": moments[k][0].clone(),
                                                   "exp_avg_sq": moments[k][1].clone()}
    m.xyz_gradient_accum, m.denom = accum.clone(), denom.clone()
    m.max_radii2D = torch.zeros(accum.shape[0], device=accum.device)
    m.dirs = dirs


def timed(setup, fn, steps, warmup):
    ms = []
    for s in range(warmup + steps):
        args = setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args)
        b.record()
        b.synchronize()
        if s >= warmup:
            ms.append(a.elapsed_time(b))
        del args
    ms.sort()
    return ms[len(ms) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--gaussians", type=int, default=6_000_000)
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    P = a.gaussians
    flags = dict.fromkeys(FLAG_NAMES, False)
    flags.update(grow_dir=True, grow_distance=True)
    for frac in (0.02, 0.10):
        params, moments, accum, denom, dirs = make(P, frac, dev)
        m = types.SimpleNamespace(percent_dense=0.01, num_dirs=ND, modelcg=types.SimpleNamespace(),
                                  **{f: flags[f] for f in FLAG_NAMES[:5]})

        def setup():
            load_model(m, params, moments, accum, denom, dirs)
            return (m,)

        hip_ms, info = timed(setup, lambda mm: densify_and_prune(mm, 0.0002, 0.005, 5.0, 20, opt=OPT,
                                                                 iteration=3100), a.steps, a.warmup)
        # bytes: every parameter / moment row read once (the rows that reach an output) and every output row written
        w = sum(t.numel() for t in params.values()) // P
        n_out = info["points"]
        bytes_moved = 3 * 4 * w * (P + n_out)
        line = {"what": "densify_fork_hip", "P": P, "num_dirs": ND, "selected_frac": frac, "ms": round(hip_ms, 3),
                "points_out": n_out, "selected": info["selected"], "split_selected": info["split_selected"],
                "gb_moved": round(bytes_moved / 1e9, 3), "tb_per_s": round(bytes_moved / hip_ms / 1e9, 3)}
        if not a.hip_only:
            ns = 2 * 2 * info["split_selected"]
            noise = torch.randn(ns, 3, device=dev)
            t_ms, out = timed(lambda: (), lambda: restate(params, moments, accum, denom, flags, 0.01, 0.0002, 0.005,
                                                          5.0, 20, 3100, 3000, dirs=dirs, noise=noise),
                              max(2, a.steps // 2), a.warmup)
            line.update(torch_ms=round(t_ms, 3), speedup=round(t_ms / hip_ms, 2),
                        torch_points_out=int(out[0]["xyz"].shape[0]))
            del out
        print(json.dumps(line), flush=True)
        del params, moments, accum, denom, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
