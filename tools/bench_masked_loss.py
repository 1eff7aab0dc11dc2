"""Stream time per call, through the wrappers, of the masked colour loss at 1920 x 1080 with C = 3, value and backward: the
span between two HIP events around a batch of calls on one stream, divided by the calls.  It holds the kernels, the
wrappers' allocations and small torch ops and any gap in which the stream waits for the host; it is not kernel time.

    fused image     masked_l1_dssim_loss(x, gt, m, normalize="image") and its backward
    fused mask      the same with normalize="mask" (no composition of shipped ops gives it)
    composition     l1_dssim_loss(m * x, m * gt) with autograd, forward plus backward: what "image" replaces
    unmasked        l1_dssim_loss(x, gt) and its backward

    PYTHONPATH=. python tools/bench_masked_loss.py [--height 1080] [--width 1920] [--iters 50] [--rounds 5] [--ring 6]

Every variant goes through the public autograd wrappers, allocations included, as the trainer calls them.  The calls of a
batch walk a ring of ``ring`` image sets (x, gt and the mask: 58 MB a set at the default size), so that no call finds its
images in the caches the call before it filled.  Rounds alternate the four variants on one box.  Prints every round's mean
per call in microseconds, the medians, and one JSON line with the raw numbers."""
import argparse
import json
import sys

import torch

from mvs_gaussian_splatting_amd import _lib, l1_dssim_loss, masked_l1_dssim_loss


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=6)
    ap.add_argument("--lambda_dssim", type=float, default=0.2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_masked_loss needs a ROCm GPU", file=sys.stderr)
        return 1
    _lib.load()
    dev = torch.device("cuda:0")
    H, W, lam = args.height, args.width, args.lambda_dssim
    torch.manual_seed(0)
    u = torch.linspace(0, 1, W, device=dev).view(1, 1, W)
    v = torch.linspace(0, 1, H, device=dev).view(1, H, 1)
    sets = []
    for k in range(args.ring):
        gt = (0.5 + 0.3 * torch.sin(9.0 * u + 5.0 * v + k) + 0.1 * torch.rand(3, H, W, device=dev)).clamp(0, 1).contiguous()
        x = (gt + 0.05 * torch.randn(3, H, W, device=dev)).clamp(0, 1).contiguous()
        m = ((u[0] - 0.5) ** 2 + (v[0] - 0.5) ** 2 < 0.16).to(torch.float32).contiguous()          # a disc: 50 % of the frame
        sets.append((x, gt, m))

    def variant(kind):
        def call(i):
            x, gt, m = sets[i % args.ring]
            leaf = x.detach().requires_grad_(True)
            if kind == "fused image":
                loss = masked_l1_dssim_loss(leaf, gt, m, lam, "image")
            elif kind == "fused mask":
                loss = masked_l1_dssim_loss(leaf, gt, m, lam, "mask")
            elif kind == "composition":
                loss = l1_dssim_loss(m[None] * leaf, m[None] * gt, lam)
            else:
                loss = l1_dssim_loss(leaf, gt, lam)
            loss.backward()
            return loss, leaf
        return call

    def run(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(n):
            fn(i)
        stop.record()
        torch.cuda.synchronize(dev)
        return 1000.0 * start.elapsed_time(stop) / n

    kinds = ("fused image", "fused mask", "composition", "unmasked")
    calls = {k: variant(k) for k in kinds}
    first = {k: calls[k](0) for k in kinds}                              # image mode and the composition compute the same thing
    gap = float((first["fused image"][1].grad - first["composition"][1].grad).abs().max() / first["composition"][1].grad.abs().max())
    print("loss: " + ", ".join(f"{k} {float(first[k][0].detach()):.7f}" for k in kinds) + f"; gradient, fused image against composition: "
          f"max-norm difference {gap:.2e}")
    for k in kinds:
        run(calls[k], 2 * args.ring)
    rows = {k: [] for k in kinds}
    for r in range(args.rounds):
        for k in kinds:
            us = run(calls[k], args.iters)
            rows[k].append(round(us, 2))
            print(f"round {r} {k}: {us:.1f} us per call")
    med = {k: sorted(rows[k])[len(rows[k]) // 2] for k in kinds}
    print("; ".join(f"median {k} {med[k]:.1f} us" for k in kinds) +
          f"; composition / fused image {med['composition'] / med['fused image']:.2f}x")
    print(json.dumps({"height": H, "width": W, "iters": args.iters, "ring": args.ring, "lambda_dssim": lam, "lib": _lib.LIB_PATH,
                      "call_us": rows, "median_us": med}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
