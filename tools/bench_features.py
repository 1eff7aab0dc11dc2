"""Device time of the feature-map kernels (csrc/features.hip: forward; backward = compositing backward + the per-Gaussian
geometry kernel) for several channel counts, next to the depth / alpha maps of csrc/depth.hip (three fixed channels) as
the yardstick, on one frame of a bench scene, from HIP events around each call.

    PYTHONPATH=.:tools python tools/bench_features.py [C4] [--channels 3 8 32] [--iters 20] [--rounds 5]

One colour forward of the scene (two-call path), then ``rounds`` rounds that alternate the calls (so that clock drift hits
all of them), ``iters`` calls each; prints every round's mean per call in microseconds and one JSON line with the raw
numbers.  The frame's saved state is only read, so every call sees the same lists.
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
    ap.add_argument("--channels", type=int, nargs="+", default=[3, 8, 32])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args(argv)
    from scene_gpu import GpuScene
    sc = GpuScene(args.config, fused=True)
    lib, dev, P, W, H = sc.lib, sc.dev, sc.P, sc.W, sc.H
    sc.forward()
    frame = _lib.GsrAuxFrame()
    frame.P, frame.width, frame.height, frame.binning_mode = P, W, H, int(sc.params.binning_mode)
    frame.num_rendered, frame.num_visible = sc.R, sc.V
    frame.geom_ws, frame.bin_ws, frame.img_ws, frame.radii = (sc.geom.data_ptr(), sc.binning.data_ptr(), sc.img.data_ptr(),
                                                              sc.radii.data_ptr())
    new = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    g = [new(P, 3), new(P, 3), new(P, 1), new(P, 3), new(P, 4)]
    grads = _lib.GsrAuxGrads(*[t.data_ptr() for t in g], None)
    nbytes = lib.gsr_feature_maps_backward_bytes(P)
    acc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    gen = torch.Generator(device="cpu").manual_seed(7)
    calls = {}

    def add_aux():
        maps, dL = new(3, H, W), (torch.rand(3, H, W, generator=gen) / (3 * H * W)).to(dev)
        calls["aux fwd"] = lambda: _lib.check(lib.gsr_aux_maps_forward(C.byref(frame), maps.data_ptr(), sc.stream), "aux fwd")
        calls["aux bwd"] = lambda: _lib.check(lib.gsr_aux_maps_backward(
            C.byref(sc.params), C.byref(frame), dL.data_ptr(), acc.data_ptr(), nbytes, C.byref(grads), sc.stream), "aux bwd")

    def add_features(n_ch):
        F = torch.randn(P, n_ch, generator=gen).to(dev)
        maps, dL, dF = new(n_ch, H, W), (torch.rand(n_ch, H, W, generator=gen) / (n_ch * H * W)).to(dev), new(P, n_ch)
        calls[f"C={n_ch} fwd"] = lambda: _lib.check(lib.gsr_feature_maps_forward(
            C.byref(frame), F.data_ptr(), n_ch, maps.data_ptr(), sc.stream), "feature fwd")
        calls[f"C={n_ch} bwd"] = lambda: _lib.check(lib.gsr_feature_maps_backward(
            C.byref(sc.params), C.byref(frame), F.data_ptr(), n_ch, dL.data_ptr(), dF.data_ptr(), acc.data_ptr(), nbytes,
            C.byref(grads), sc.stream), "feature bwd")

    add_aux()
    for n_ch in args.channels:
        add_features(n_ch)

    def run(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return 1000.0 * a.elapsed_time(b) / n

    for fn in calls.values():
        run(fn, 3)
    rows = {k: [] for k in calls}
    for r in range(args.rounds):
        for k, fn in calls.items():
            us = run(fn, args.iters)
            rows[k].append(round(us, 1))
            print(f"round {r} {k}: {us:.1f} us per call")
    print(json.dumps({"config": args.config, "P": P, "W": W, "H": H, "num_rendered": sc.R, "iters": args.iters,
                      "us_per_call": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
