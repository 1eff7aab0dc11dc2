"""Device time of the depth-prior loss at 1920 x 1080, value and backward, per mode: the fused call
(``gsr_depth_prior_fwd_bwd`` with the unit gradient; 2, 4 or 3 launches) against the same mode written as float32 torch
ops with autograd on the GPU, from HIP events around batches of calls on one stream.

    PYTHONPATH=. python tools/bench_depth_prior.py [--height 1080] [--width 1920] [--iters 100] [--rounds 5] [--ring 8]

The calls of a batch walk a ring of ``ring`` map sets (render, prior, weight and the gradient: 33 MB a set at the default
size), so that no call finds its maps in the caches the call before it filled.  Rounds alternate fused and torch batches
on one box.  Prints every round's mean per call in microseconds, the ratio per mode, the bytes a fused call has to move
(3 floats read per pass over the maps, 1 written) and one JSON line with the raw numbers.  The torch forms are float32
sums: they are the comparison for time, not for bits.
"""
import argparse
import json
import sys

import torch

from mvs_gaussian_splatting_amd import _lib
from mvs_gaussian_splatting_amd.depth_prior import MODES


def torch_loss(x, y, w, mode, scale=0.4, offset=0.1):
    """The definitions of DESIGN.md §7.31 as whole-image float32 torch ops."""
    valid = (w > 0) & torch.isfinite(y) & torch.isfinite(x.detach())
    wv = torch.where(valid, w, torch.zeros_like(w))
    yv = torch.where(valid, y, torch.zeros_like(y))
    xv = torch.where(valid, x, torch.zeros_like(x))
    if mode == "l1":
        return (wv * (xv - (scale * yv + offset)).abs()).sum() / x.numel()
    Sw = wv.sum()
    mx, my = (wv * xv).sum() / Sw, (wv * yv).sum() / Sw
    dx, dy = xv - mx, yv - my
    cov, vx, vy = (wv * dx * dy).sum() / Sw, (wv * dx * dx).sum() / Sw, (wv * dy * dy).sum() / Sw
    if mode == "aligned_l1":
        s = (cov / vy).detach()
        t = (mx - s * my).detach()
        return (wv * (xv - (s * yv + t)).abs()).sum() / Sw
    return 1.0 - cov / torch.sqrt(vx * vy)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=8)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_depth_prior needs a ROCm GPU", file=sys.stderr)
        return 1
    lib, dev = _lib.load(), torch.device("cuda:0")
    H, W = args.height, args.width
    torch.manual_seed(0)
    u = torch.linspace(0, 1, W, device=dev).view(1, W)
    v = torch.linspace(0, 1, H, device=dev).view(H, 1)
    sets = []
    for k in range(args.ring):
        y = (0.2 + 1.8 * (0.375 * (u + v) + 0.125 * (1.0 + torch.sin(7.0 * u + 3.0 * v + k)))).contiguous()
        x = (0.4 * y + 0.1 + 0.05 * torch.randn(H, W, device=dev)).contiguous()
        w = torch.tensor([0.0, 0.5, 1.0], device=dev)[torch.randint(0, 5, (H, W), device=dev).clamp(max=2)].contiguous()
        sets.append((x, y, w, torch.empty(H, W, device=dev)))
    record = torch.empty(8, dtype=torch.float64, device=dev)
    nbytes = lib.gsr_depth_prior_workspace_bytes(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fused(mode):
        def call(i):
            x, y, w, g = sets[i % args.ring]
            _lib.check(lib.gsr_depth_prior_fwd_bwd(x.data_ptr(), y.data_ptr(), w.data_ptr(), H, W, MODES[mode], 0.4, 0.1,
                                                   record.data_ptr(), g.data_ptr(), ws.data_ptr(), nbytes, stream), "fused")
        return call

    def as_torch(mode):
        def call(i):
            x, y, w, _ = sets[i % args.ring]
            leaf = x.detach().requires_grad_(True)
            torch_loss(leaf, y, w, mode).backward()
            return leaf
        return call

    def run(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(n):
            fn(i)
        stop.record()
        torch.cuda.synchronize(dev)
        return 1000.0 * start.elapsed_time(stop) / n

    out = {"height": H, "width": W, "iters": args.iters, "ring": args.ring, "lib": _lib.LIB_PATH, "modes": {}}
    passes = {"l1": 1, "aligned_l1": 2, "pearson": 2}
    for mode in MODES:
        f, t = fused(mode), as_torch(mode)
        f(0)                                                         # the two compute the same thing
        leaf = t(0)
        ref = float(torch_loss(*sets[0][:3], mode))
        g_err = float((sets[0][3] - leaf.grad).abs().max() / leaf.grad.abs().max())
        print(f"{mode}: loss fused {float(record[0]):.7f} torch {ref:.7f}; dL/dinvdepth max-norm difference {g_err:.2e}")
        for fn in (f, t):
            run(fn, 2 * args.ring)
        rows = {"fused": [], "torch": []}
        for r in range(args.rounds):
            for kind, fn, n in (("fused", f, args.iters), ("torch", t, max(args.iters // 5, 1))):
                us = run(fn, n)
                rows[kind].append(round(us, 2))
                print(f"{mode} round {r} {kind}: {us:.1f} us per call")
        med = sorted(rows["fused"])[len(rows["fused"]) // 2]
        med_t = sorted(rows["torch"])[len(rows["torch"]) // 2]
        need = (3 * passes[mode] + 1) * H * W * 4
        print(f"{mode}: median fused {med:.1f} us (best {min(rows['fused']):.1f}), median torch {med_t:.1f} us, ratio "
              f"{med_t / med:.1f}x; the fused call moves {need / 1e6:.1f} MB: {need / med / 1e6:.2f} TB/s")
        out["modes"][mode] = {"call_us": rows, "median_us": {"fused": med, "torch": med_t}, "ratio": round(med_t / med, 2),
                              "bytes": need}
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
