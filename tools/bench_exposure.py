"""Device time of the two exposure kernels' calls (``gsr_exposure_apply_fwd``; ``gsr_exposure_apply_bwd`` with dx and dA,
finish kernel included) at 1920 x 1080, from HIP events around batches of calls on one stream.

    PYTHONPATH=. python tools/bench_exposure.py [--height 1080] [--width 1920] [--iters 200] [--rounds 5] [--ring 12]

The calls of a batch walk a ring of ``ring`` image sets (x, g, y, dx: 100 MB a set at the default size), so that no call
finds its images in the caches the call before it filled.  Rounds alternate forward and backward batches; prints every
round's mean per call in microseconds, the bytes each call has to move (forward: 25 MB read, x, and 25 MB written, y;
backward: 50 MB read, x and g, and 25 MB written, dx) with the time those bytes take at ``--stream-tbps`` (default
4.5 TB/s: what a copy kernel of a few thousand blocks reaches on this card, ``profiles/r03/hbm_stream_rates.txt``), and
one JSON line with the raw numbers.
"""
import argparse
import json
import sys

import torch

from mvs_gaussian_splatting_amd import _lib


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=12)
    ap.add_argument("--stream-tbps", type=float, default=4.5)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_exposure needs a ROCm GPU", file=sys.stderr)
        return 1
    lib, dev = _lib.load(), torch.device("cuda:0")
    H, W = args.height, args.width
    torch.manual_seed(0)
    sets = [(torch.rand(3, H, W, device=dev), torch.randn(3, H, W, device=dev) / (3 * H * W),
             torch.empty(3, H, W, device=dev), torch.empty(3, H, W, device=dev)) for _ in range(args.ring)]
    A = (torch.eye(3, 4) + 0.01).to(dev)
    dA = torch.empty(3, 4, device=dev)
    ws = torch.empty(lib.gsr_exposure_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def forward(i):
        x, _, y, _ = sets[i % args.ring]
        _lib.check(lib.gsr_exposure_apply_fwd(x.data_ptr(), A.data_ptr(), H, W, y.data_ptr(), stream), "fwd")

    def backward(i):
        x, g, _, dx = sets[i % args.ring]
        _lib.check(lib.gsr_exposure_apply_bwd(x.data_ptr(), A.data_ptr(), g.data_ptr(), H, W, dx.data_ptr(),
                                              dA.data_ptr(), ws.data_ptr(), stream), "bwd")

    def run(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for i in range(n):
            fn(i)
        stop.record()
        torch.cuda.synchronize(dev)
        return 1000.0 * start.elapsed_time(stop) / n

    image_bytes = 3 * H * W * 4
    need = {"fwd": 2 * image_bytes, "bwd": 3 * image_bytes}
    for fn in (forward, backward):
        run(fn, 2 * args.ring)
    rows = {"fwd": [], "bwd": []}
    for r in range(args.rounds):
        for kind, fn in (("fwd", forward), ("bwd", backward)):
            us = run(fn, args.iters)
            rows[kind].append(round(us, 2))
            print(f"round {r} {kind}: {us:.1f} us per call, {need[kind] / us / 1e6:.2f} TB/s of its {need[kind] / 1e6:.1f} MB")
    floor = {k: round(v / (args.stream_tbps * 1e6), 2) for k, v in need.items()}
    print(f"streaming time of the bytes at {args.stream_tbps} TB/s: fwd {floor['fwd']} us, bwd {floor['bwd']} us")
    print("dA:", dA.cpu().tolist()[0])
    print(json.dumps({"height": H, "width": W, "iters": args.iters, "ring": args.ring, "lib": _lib.LIB_PATH,
                      "bytes": need, "stream_floor_us": floor, "call_us": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
