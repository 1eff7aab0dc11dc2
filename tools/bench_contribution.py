"""Device time of ``gsr_contribution_accumulate`` next to ``gsr_aux_maps_forward`` on the same frame, from HIP events
around batches of calls.

    PYTHONPATH=.:tools python tools/bench_contribution.py [C4] [--iters 20] [--rounds 5] [--mask]

One forward of the scene (1920 x 1080 for C3 / C4), then ``rounds`` rounds that alternate ``iters`` calls of the maps'
forward and ``iters`` calls of the statistics (so that clock drift hits both); prints every round's mean per call in
microseconds and one JSON line with the raw numbers, the frame's instance count and the number of Gaussians the
statistics found composited.  ``--mask`` passes an all-ones pixel mask (the cost of reading it).  Repeated calls add into
one buffer: 2^63 / 2^30 weight units leave room for millions of calls of a frame.
"""
import argparse
import ctypes as C
import json
import sys

import torch

from mvs_gaussian_splatting_amd import _lib


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mask", action="store_true")
    args = ap.parse_args(argv)
    from scene_gpu import GpuScene
    sc = GpuScene(args.config, fused=True)
    lib, dev, P = sc.lib, sc.dev, sc.P
    sc.forward()
    torch.cuda.synchronize(dev)
    frame = _lib.GsrAuxFrame()
    frame.P, frame.width, frame.height, frame.binning_mode = P, sc.W, sc.H, int(sc.params.binning_mode)
    frame.num_rendered, frame.num_visible = sc.R, sc.V
    frame.geom_ws, frame.bin_ws, frame.img_ws, frame.radii = (sc.geom.data_ptr(), sc.binning.data_ptr(), sc.img.data_ptr(),
                                                              sc.radii.data_ptr())
    maps = torch.empty(3, sc.H, sc.W, device=dev)
    stats = torch.zeros(P, 3, dtype=torch.int64, device=dev)
    mask = torch.ones(sc.H, sc.W, dtype=torch.uint8, device=dev) if args.mask else None
    calls = {
        "aux_maps_forward": lambda: _lib.check(lib.gsr_aux_maps_forward(C.byref(frame), maps.data_ptr(), sc.stream), "maps"),
        "contribution": lambda: _lib.check(lib.gsr_contribution_accumulate(
            C.byref(frame), None if mask is None else mask.data_ptr(), stats.data_ptr(), sc.stream), "contribution"),
    }

    def run(kind, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            calls[kind]()
        stop.record()
        stop.synchronize()
        return 1000.0 * start.elapsed_time(stop) / n

    for kind in calls:
        run(kind, 3)
    rows = {kind: [] for kind in calls}
    for r in range(args.rounds):
        for kind in calls:
            us = run(kind, args.iters)
            rows[kind].append(round(us, 2))
            print(f"round {r} {kind}: {us:.1f} us per call")
    composited = int((stats[:, 1] > 0).sum())
    print(json.dumps({"config": args.config, "P": P, "W": sc.W, "H": sc.H, "num_rendered": sc.R, "num_visible": sc.V,
                      "composited": composited, "mask": bool(args.mask), "iters": args.iters, "lib": _lib.LIB_PATH,
                      "call_us": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
