"""Times the model-lifecycle kernels of csrc/model.hip against their torch restatements on the same device, one JSON
line per measurement.  Run each part as its own process under its own time limit:

    timeout -k 10 300 python tools/bench_model.py sparsity [--points 6000000]   # the term alone, forward + backward
    timeout -k 10 600 python tools/bench_model.py step     [--points 6000000]   # a train step with the term switched on
    timeout -k 10 300 python tools/bench_model.py reset    [--points 6000000]   # reset_opacity (for the record)
    timeout -k 10 300 python tools/bench_model.py pcd      [--points 1000000]   # create_from_pcd (for the record)

"torch" is train.py:102-106 (and scene/gaussian_model.py:312-315, :386-399) restated in torch ops.  Device time is
taken with events around the calls, wall time with a host clock around a window that ends in a synchronise; the two
versions alternate inside one process so that they share the box's conditions.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import GaussianModel, l1_dssim_loss, opacity_sparsity_loss, render  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene  # noqa: E402


def torch_term(raw, w):
    """train.py:102-106: two host synchronisations (the `if` on a device sum, the boolean-mask gather)."""
    o = torch.sigmoid(raw)
    prune_mask = (o < 0.005).squeeze()
    if w > 0 and torch.sum(prune_mask) > 0:
        return w * torch.abs(o[prune_mask] - 1).mean()
    return None


def hip_term(raw, w):
    return opacity_sparsity_loss(raw, w)


def timed(fn, steps, warmup):
    """-> (median device ms per call, wall ms per call over the whole window)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    return statistics.median(a.elapsed_time(b) for a, b in ev), wall


def emit(**kw):
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in kw.items()}), flush=True)


def raw_opacity(points, dev, low_share=0.2):
    g = torch.Generator(device=dev).manual_seed(0)
    raw = torch.randn(points, 1, device=dev, generator=g) * 1.5
    low = torch.rand(points, 1, device=dev, generator=g) < low_share
    return torch.where(low, raw - 8.0, raw)                       # about a fifth of the rows below sigmoid = 0.005


def bench_sparsity(args, dev):
    raw = raw_opacity(args.points, dev).requires_grad_(True)

    def run(term):
        def fn():
            raw.grad = None
            loss = term(raw, 0.05)
            if loss is not None:
                loss.backward()
        return fn

    for rnd in range(args.rounds):
        for name, term in (("hip", hip_term), ("torch", torch_term)):
            dev_ms, wall_ms = timed(run(term), args.steps, args.warmup)
            emit(what="sparsity_fwd_bwd", impl=name, round=rnd, points=args.points, device_ms=dev_ms, wall_ms=wall_ms)


def bench_step(args, dev):
    cfg = CONFIGS["C4"]
    model, cam, bg, target = make_scene(cfg, seed=0, device=dev, P=args.points)
    with torch.no_grad():
        model._opacity.copy_(raw_opacity(args.points, dev))
    for p in model.parameters():
        p.requires_grad_(True)
    pipe = PipelineParams()

    def run(term):
        def fn():
            for p in model.parameters():
                p.grad = None
            loss = l1_dssim_loss(render(cam, model, pipe, bg)["render"], target, 0.2)
            if term is not None:
                extra = term(model._opacity, 0.05)
                if extra is not None:
                    loss = loss + extra
            loss.backward()
        return fn

    for rnd in range(args.rounds):
        for name, term in (("off", None), ("hip", hip_term), ("torch", torch_term)):
            dev_ms, wall_ms = timed(run(term), args.steps, args.warmup)
            emit(what="train_step_fwd_bwd", term=name, round=rnd, points=args.points, width=cfg.width, height=cfg.height,
                 device_ms=dev_ms, wall_ms=wall_ms)


def bench_reset(args, dev):
    start = raw_opacity(args.points, dev)
    m = GaussianModel(0)
    m._opacity = torch.nn.Parameter(start.clone().requires_grad_(True))
    mom = [torch.ones_like(start), torch.ones_like(start)]
    m.optimizer = torch.optim.Adam([{"params": [m._opacity], "lr": 0.05, "name": "opacity"}], lr=0.0, eps=1e-15)
    m.optimizer.state[m._opacity] = {"step": torch.tensor(1.0), "exp_avg": mom[0], "exp_avg_sq": mom[1]}
    holder = {"p": torch.nn.Parameter(start.clone())}

    def torch_reset():
        o = torch.sigmoid(holder["p"])
        new = torch.min(o, torch.ones_like(o) * 0.01)
        new = torch.log(new / (1 - new))
        mom[0], mom[1] = torch.zeros_like(new), torch.zeros_like(new)
        holder["p"] = torch.nn.Parameter(new.requires_grad_(True))

    for rnd in range(args.rounds):
        for name, fn in (("hip", m.reset_opacity), ("torch", torch_reset)):
            dev_ms, wall_ms = timed(fn, args.steps, args.warmup)
            emit(what="reset_opacity", impl=name, round=rnd, points=args.points, device_ms=dev_ms, wall_ms=wall_ms)


def bench_pcd(args, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    pts = torch.randn(args.points, 3, device=dev, generator=g) * torch.tensor([4.0, 2.0, 3.0], device=dev)
    cols = torch.rand(args.points, 3, device=dev, generator=g)
    for rnd in range(args.rounds):
        dev_ms, wall_ms = timed(lambda: GaussianModel(3).create_from_pcd(pts, cols, 1.0), max(args.steps // 10, 2), 1)
        emit(what="create_from_pcd", round=rnd, points=args.points, device_ms=dev_ms, wall_ms=wall_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sparsity", "step", "reset", "pcd"])
    ap.add_argument("--points", type=int, default=None)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_model needs a GPU")
    if args.points is None:
        args.points = 1_000_000 if args.what == "pcd" else 6_000_000
    dev = torch.device("cuda:0")
    emit(what="box", device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=str(torch.version.hip))
    {"sparsity": bench_sparsity, "step": bench_step, "reset": bench_reset, "pcd": bench_pcd}[args.what](args, dev)


if __name__ == "__main__":
    main()
