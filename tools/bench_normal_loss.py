"""Device time of the depth-normal consistency loss at 1920 x 1080, value and backward: the fused call
(``gsr_normal_consistency_fwd_bwd`` with the three gradients, finish kernel included) against the same loss written as
float32 torch ops with autograd on the GPU, from HIP events around batches of calls on one stream.

    PYTHONPATH=. python tools/bench_normal_loss.py [--height 1080] [--width 1920] [--iters 100] [--rounds 5] [--ring 8]

The calls of a batch walk a ring of ``ring`` map sets (depth, alpha, normal and the three gradients: 100 MB a set at the
default size), so that no call finds its maps in the caches the call before it filled.  Rounds alternate fused and torch
batches on one box.  Prints every round's mean per call in microseconds, the ratio, the bytes the fused call has to move
(5 floats read -- depth, alpha, normal -- and 5 written -- their gradients -- per pixel, 40 B; the round figure of
6 and 6, 48 B or 100 MB a frame, is listed next to it) with the share of ``--stream-tbps`` (default 6.29 TB/s, the
project's measured streaming rate, ``profiles/r03/hbm_stream_rates.txt``) those bytes reach, and one JSON line with the
raw numbers.
"""
import argparse
import json
import sys

import torch

from mvs_gaussian_splatting_amd import _lib


def torch_loss(depth, alpha, normal, fx, fy, alpha_min):
    """The definition of DESIGN.md §7.15 as whole-image float32 torch ops; depth, alpha [H,W], normal [3,H,W]."""
    H, W = depth.shape
    covered = alpha.detach() >= alpha_min
    d = torch.where(covered, depth / torch.where(covered, alpha, torch.ones_like(alpha)), torch.zeros_like(depth))
    xs = (torch.arange(W, dtype=torch.float32, device=depth.device) - (W - 1) / 2.0).view(1, W)
    ys = (torch.arange(H, dtype=torch.float32, device=depth.device) - (H - 1) / 2.0).view(H, 1)
    P = torch.stack((d * xs / fx, d * ys / fy, d))
    tx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    ty = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(ty, tx, dim=0)
    s = (c * c).sum(dim=0)
    ok = covered[1:-1, 1:-1] & covered[1:-1, 2:] & covered[1:-1, :-2] & covered[2:, 1:-1] & covered[:-2, 1:-1] & \
        torch.isfinite(s.detach()) & (s.detach() > 1e-20)
    n_d = c / torch.sqrt(torch.where(ok, s, torch.ones_like(s)))
    e = alpha[1:-1, 1:-1] - (normal[:, 1:-1, 1:-1] * n_d).sum(dim=0)
    return torch.where(ok, e, torch.zeros_like(e)).sum() / (H * W)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--stream-tbps", type=float, default=6.29)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_normal_loss needs a ROCm GPU", file=sys.stderr)
        return 1
    lib, dev = _lib.load(), torch.device("cuda:0")
    H, W = args.height, args.width
    tanx, tany = 0.8, 0.45
    fx, fy = W / (2 * tanx), H / (2 * tany)
    torch.manual_seed(0)
    u = torch.linspace(0, 1, W, device=dev).view(1, W)
    v = torch.linspace(0, 1, H, device=dev).view(H, 1)
    sets = []
    for k in range(args.ring):
        alpha = (0.75 + 0.25 * torch.sin(7.0 * u + k) * torch.cos(5.0 * v)).contiguous()
        alpha[(u - 0.5) ** 2 + (v - 0.5) ** 2 > 0.2] = 0.0                         # an uncovered surround, as a scene has
        z = 4.0 + 0.5 * torch.sin(9.0 * u + 0.3 * k) + 0.4 * torch.cos(6.0 * v) + 0.001 * torch.rand(H, W, device=dev)
        normal = torch.nn.functional.normalize(torch.randn(3, H, W, device=dev), dim=0) * alpha
        sets.append(((z * alpha).contiguous(), alpha, normal.contiguous(),
                     torch.empty(H, W, device=dev), torch.empty(H, W, device=dev), torch.empty(3, H, W, device=dev)))
    record = torch.empty(4, device=dev)
    ws = torch.empty(lib.gsr_normal_consistency_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fused(i):
        d, a, n, gd, ga, gn = sets[i % args.ring]
        _lib.check(lib.gsr_normal_consistency_fwd_bwd(d.data_ptr(), a.data_ptr(), n.data_ptr(), H, W, tanx, tany, 0.5,
                                                      record.data_ptr(), gd.data_ptr(), ga.data_ptr(), gn.data_ptr(), None,
                                                      ws.data_ptr(), stream), "fused")

    def as_torch(i):
        leaves = [t.detach().requires_grad_(True) for t in sets[i % args.ring][:3]]
        torch_loss(*leaves, fx, fy, 0.5).backward()
        return leaves

    def run(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(n):
            fn(i)
        stop.record()
        torch.cuda.synchronize(dev)
        return 1000.0 * start.elapsed_time(stop) / n

    # the two compute the same thing
    fused(0)
    leaves = as_torch(0)
    ref = float(torch_loss(*sets[0][:3], fx, fy, 0.5))
    gd_err = float((sets[0][3] - leaves[0].grad).abs().max() / leaves[0].grad.abs().max())
    print(f"loss fused {float(record[0]):.7f} torch {ref:.7f}; n_valid {int(record.view(torch.int32)[1])} of {H * W}; "
          f"dL/ddepth max-norm difference {gd_err:.2e}")
    for fn in (fused, as_torch):
        run(fn, 2 * args.ring)
    rows = {"fused": [], "torch": []}
    for r in range(args.rounds):
        for kind, fn, n in (("fused", fused, args.iters), ("torch", as_torch, max(args.iters // 5, 1))):
            us = run(fn, n)
            rows[kind].append(round(us, 2))
            print(f"round {r} {kind}: {us:.1f} us per call")
    need = {"training_call": 10 * H * W * 4, "six_and_six": 12 * H * W * 4}
    best = min(rows["fused"])
    med = sorted(rows["fused"])[len(rows["fused"]) // 2]
    med_t = sorted(rows["torch"])[len(rows["torch"]) // 2]
    frac = {k: round(b / (med * 1e6) / args.stream_tbps, 3) for k, b in need.items()}
    print(f"median fused {med:.1f} us (best {best:.1f}), median torch {med_t:.1f} us, ratio {med_t / med:.1f}x")
    print(f"the training call moves {need['training_call'] / 1e6:.1f} MB: {need['training_call'] / med / 1e6:.2f} TB/s, "
          f"{frac['training_call']:.2f} of {args.stream_tbps} TB/s")
    print(json.dumps({"height": H, "width": W, "iters": args.iters, "ring": args.ring, "lib": _lib.LIB_PATH,
                      "bytes": need, "call_us": rows, "median_us": {"fused": med, "torch": med_t},
                      "ratio": round(med_t / med, 2), "stream_fraction": frac}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
