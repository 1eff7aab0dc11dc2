"""Device time of the median-depth map (csrc/median.hip: forward; backward = the per-tile scatter + the per-Gaussian
finish kernel) against its nearest sibling, the depth / inverse-depth / alpha maps (csrc/depth.hip: forward; backward =
compositing backward + the per-Gaussian geometry kernel), on one frame of a bench scene at 1920x1080, from HIP events
around each route.

    PYTHONPATH=.:tools python tools/bench_median_depth.py [C4] [--iters 20] [--rounds 5]

One colour forward of the scene (two-call path), then ``rounds`` rounds that alternate the four calls (so that clock drift
hits all of them), ``iters`` calls each; prints every round's mean per call in microseconds and one JSON line with the raw
numbers.  The frame's saved state is only read, so every call sees the same lists.  The question the figures answer is
whether the early exit -- a pixel's walk ends where its transmittance reaches one half, a tile's where all its pixels'
have -- makes the forward cheaper than the three-map forward, which walks every pixel to its last contributor.  Also
printed: how far the pixels walk (mean list position of the median against the mean contributor count).
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
    fref = C.byref(frame)

    median, g_median = new(1, H, W), torch.full((1, H, W), 1.0 / (H * W), device=dev)
    median_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    state = torch.empty(H, W, dtype=torch.int32, device=dev)
    g_xyz = new(P, 3)
    med_bytes = lib.gsr_median_depth_backward_bytes(P)
    med_acc = torch.empty(med_bytes, dtype=torch.uint8, device=dev)

    def median_fwd():
        _lib.check(lib.gsr_median_depth_forward(fref, median.data_ptr(), median_id.data_ptr(), state.data_ptr(), sc.stream),
                   "median fwd")

    def median_fwd_bwd():
        median_fwd()
        _lib.check(lib.gsr_median_depth_backward(C.byref(sc.params), fref, state.data_ptr(), g_median.data_ptr(),
                                                 med_acc.data_ptr(), med_bytes, g_xyz.data_ptr(), sc.stream), "median bwd")

    maps, g_maps = new(3, H, W), torch.full((3, H, W), 1.0 / (3 * H * W), device=dev)
    g = [new(P, 3), new(P, 3), new(P, 1), new(P, 3), new(P, 4)]
    grads = _lib.GsrAuxGrads(*[t.data_ptr() for t in g], None)
    aux_bytes = lib.gsr_aux_maps_backward_bytes(P)
    aux_acc = torch.empty(aux_bytes, dtype=torch.uint8, device=dev)

    def aux_fwd():
        _lib.check(lib.gsr_aux_maps_forward(fref, maps.data_ptr(), sc.stream), "aux fwd")

    def aux_fwd_bwd():
        aux_fwd()
        _lib.check(lib.gsr_aux_maps_backward(C.byref(sc.params), fref, g_maps.data_ptr(), aux_acc.data_ptr(), aux_bytes,
                                             C.byref(grads), sc.stream), "aux bwd")

    calls = {"median fwd": median_fwd, "aux_maps fwd": aux_fwd, "median fwd+bwd": median_fwd_bwd,
             "aux_maps fwd+bwd": aux_fwd_bwd}

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
    n_contrib = torch.empty(H, W, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_debug_read_image(sc.img.data_ptr(), W, H, None, n_contrib.data_ptr(), None, sc.stream), "read_image")
    torch.cuda.synchronize(dev)
    has = median_id >= 0
    walk = {"pixels_with_a_median": int(has.sum()), "mean_median_position": float(state[has].float().mean()) if bool(has.any()) else 0.0,
            "mean_n_contrib": float(n_contrib[has].float().mean()) if bool(has.any()) else 0.0,
            "gaussians_chosen": int(torch.unique(median_id[has]).numel()),
            "grad_rows_nonzero": int((g_xyz.abs().sum(dim=1) > 0).sum())}
    print(f"walk: {walk}")
    print(json.dumps({"config": args.config, "P": P, "W": W, "H": H, "num_rendered": sc.R, "iters": args.iters,
                      "us_per_call": rows, "walk": walk, "finite": bool(torch.isfinite(median).all())}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
