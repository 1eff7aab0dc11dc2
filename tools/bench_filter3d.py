"""Device time of the 3D smoothing filter (csrc/filter3d.hip; filter3d.py) on a synthetic bench cloud.

    PYTHONPATH=. python tools/bench_filter3d.py [--config C4] [--views 64 300] [--iters 20] [--warmup 5] [--rounds 3]

Timed, HIP events around the call, median / min / max over ``--iters`` calls after ``--warmup`` (warm clocks), the whole
set repeated ``--rounds`` times so the spread between rounds shows:

* ``compute_3d_filter`` for V orbit views (the whole call: table build, its one small copy, sample, finish) and the
  sampling kernel alone through its entry point with the table already on the device;
* ``apply_3d_filter`` forward plus backward against the same maths in torch float32 ops, with the bytes each moves and
  the rate that makes -- the float64 arithmetic inside the lane is free while the kernel runs at memory speed;
* one frame, forward plus backward of the L1 loss, with ``filter_3D`` set beside the same frame without it (the path of a
  model that has no filter), interleaved in one session.
"""
import argparse
import json
import statistics
import sys

import torch

from mvs_gaussian_splatting_amd import _lib, apply_3d_filter, compute_3d_filter, filter3d, l1_loss, render
from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene, orbit_camera


def call_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return [round(x, 4) for x in (statistics.median(out), min(out), max(out))]


def torch_apply(s, o, f):
    """The closed form of csrc/filter3d_math.h in torch float32 ops."""
    t = (f * f)[:, None] * torch.exp(-2.0 * s)
    l = 0.5 * torch.log1p(t)
    L = l.sum(dim=1, keepdim=True)
    omc = -torch.expm1(-L)
    neg = (o - L) - torch.log1p(omc * torch.exp(o.clamp(max=0.0)))
    pos = -L - torch.log(omc + torch.exp(-o.clamp(min=0.0)))
    return s + l, torch.where(o <= 0, neg, pos)


def sample_only(xyz, cameras, near=0.2, margin=0.15):
    """-> a closure that launches gsr_filter3d_sample with the table already on the device."""
    rows, _ = filter3d.view_table(cameras)
    dev, P = xyz.device, int(xyz.shape[0])
    table = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).to(dev)
    lib = _lib.load()
    min_depth, max_rate = torch.empty(P, device=dev), torch.empty(P, device=dev)
    seen = torch.empty(P, dtype=torch.uint8, device=dev)
    ws_bytes = int(lib.gsr_filter3d_workspace_bytes(P))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        _lib.check(lib.gsr_filter3d_sample(xyz.data_ptr(), P, table.data_ptr(), len(cameras), near, margin, 0,
                                           min_depth.data_ptr(), max_rate.data_ptr(), seen.data_ptr(), ws.data_ptr(), ws_bytes,
                                           stream), "gsr_filter3d_sample")
    launch.keep = (table, min_depth, max_rate, seen, ws)
    return launch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--views", type=int, nargs="+", default=[64, 300])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter3d needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    model, cam, bg, target = make_scene(cfg, seed=0, device=dev)
    for p in model.parameters():
        p.requires_grad_(True)
    target = target.to(dev)
    P = int(model._xyz.shape[0])
    xyz = model._xyz.detach().contiguous()
    res = {"config": args.config, "P": P, "image": [cfg.width, cfg.height], "iters": args.iters, "rounds": []}
    print(f"cloud: {P} Gaussians; views of {cfg.width} x {cfg.height}")
    pipe = PipelineParams()

    def frame():
        for p in model.parameters():
            p.grad = None
        l1_loss(render(cam, model, pipe, bg)["render"], target).backward()

    for r in range(args.rounds):
        row = {}
        for V in args.views:
            cameras = [orbit_camera(v, V, cfg.width, cfg.height, cfg.fx, cfg.fy) for v in range(V)]
            launch = sample_only(xyz, cameras)
            for rule in ("mip_splatting", "paper"):
                row[f"V{V} compute_3d_filter {rule}"] = call_ms(lambda: compute_3d_filter(xyz, cameras, rule=rule), args.iters,
                                                                args.warmup)
            k = row[f"V{V} sample kernel"] = call_ms(launch, args.iters, args.warmup)
            row[f"V{V} pairs_per_us"] = round(P * V / (k[0] * 1e3), 1)
            filt, flag = compute_3d_filter(xyz, cameras)
            row[f"V{V} seen_none"] = int(flag)
        s, o = model._scaling, model._opacity
        g_s, g_o = torch.randn_like(s), torch.randn_like(o)

        def hip_step():
            s.grad = o.grad = None
            torch.autograd.backward(apply_3d_filter(s, o, filt), [g_s, g_o])

        def torch_step():
            s.grad = o.grad = None
            torch.autograd.backward(torch_apply(s, o, filt), [g_s, g_o])

        with torch.no_grad():
            row["apply fwd"] = call_ms(lambda: apply_3d_filter(s, o, filt), args.iters, args.warmup)
            row["torch fwd"] = call_ms(lambda: torch_apply(s, o, filt), args.iters, args.warmup)
        row["apply fwd+bwd"] = call_ms(hip_step, args.iters, args.warmup)
        row["torch fwd+bwd"] = call_ms(torch_step, args.iters, args.warmup)
        s.grad = o.grad = None
        # forward: 20 bytes in, 16 out per Gaussian; backward: 36 in, 16 out
        row["apply fwd GB/s"] = round(36 * P / (row["apply fwd"][0] * 1e6), 1)
        model.filter_3D = None
        row["frame fwd+bwd, no filter"] = call_ms(frame, args.iters, args.warmup)
        model.filter_3D = filt
        row["frame fwd+bwd, filter"] = call_ms(frame, args.iters, args.warmup)
        model.filter_3D = None
        row["frame fwd+bwd, no filter (again)"] = call_ms(frame, args.iters, args.warmup)
        res["rounds"].append(row)
        print(f"[round {r}] " + "; ".join(f"{k}: {v}" for k, v in row.items()))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
