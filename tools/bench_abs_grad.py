"""Cost of the absolute-gradient pass (csrc/abs_grad.hip) on one frame of a bench scene, from HIP events.

    PYTHONPATH=.:tools python tools/bench_abs_grad.py [C4] [--iters 20] [--rounds 5] [--steps 20]

1. Calls: ``gsr_abs_grad_backward`` (zero-fill of [P,3] + the kernel) next to its yardstick, the feature maps' backward at
   C = 3, geometry only (``gsr_feature_maps_backward`` with ``dL_dfeatures = NULL``: zero-fill of [P,8], the same walk
   with six sums, and the per-Gaussian geometry kernel), on the saved state of one colour forward.  ``rounds`` rounds
   alternate the two, ``iters`` calls each.
2. Train step: ``render`` + L1 + ``backward`` + ``add_densification_stats`` with and without ``abs_grad``, alternating,
   ``steps`` steps per round.

Prints every round and one JSON line with the raw numbers (microseconds).
"""
import argparse
import ctypes as C
import json
import sys

import torch

from mvs_gaussian_splatting_amd import _lib


def _timed(dev, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return 1000.0 * a.elapsed_time(b) / n


def bench_calls(args):
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
    dL = ((torch.rand(3, H, W, generator=gen) * 2 - 1) / (3 * H * W)).to(dev)
    F = torch.randn(P, 3, generator=gen).to(dev)
    out_abs = new(P, 3)
    calls = {
        "abs_grad bwd": lambda: _lib.check(lib.gsr_abs_grad_backward(
            C.byref(sc.params), C.byref(frame), dL.data_ptr(), out_abs.data_ptr(), sc.stream), "abs bwd"),
        "features C=3 bwd, geometry only": lambda: _lib.check(lib.gsr_feature_maps_backward(
            C.byref(sc.params), C.byref(frame), F.data_ptr(), 3, dL.data_ptr(), None, acc.data_ptr(), nbytes,
            C.byref(grads), sc.stream), "feature bwd"),
    }
    for fn in calls.values():
        _timed(dev, fn, 3)
    rows = {k: [] for k in calls}
    for r in range(args.rounds):
        for k, fn in calls.items():
            us = _timed(dev, fn, args.iters)
            rows[k].append(round(us, 1))
            print(f"round {r} {k}: {us:.1f} us per call")
    return {"P": P, "W": W, "H": H, "num_rendered": sc.R, "us_per_call": rows}


def bench_steps(args):
    from mvs_gaussian_splatting_amd import add_densification_stats, l1_loss, render
    from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene
    dev = torch.device("cuda:0")
    model, cam, bg, target = make_scene(CONFIGS[args.config])
    model.to(dev)
    cam.to(dev)
    bg, target = bg.to(dev), target.to(dev)
    for p in model.parameters():
        p.requires_grad_(True)
    pipe = PipelineParams()

    def step(abs_grad):
        pkg = render(cam, model, pipe, bg, **({"abs_grad": True} if abs_grad else {}))
        l1_loss(pkg["render"], target).backward()
        add_densification_stats(model, pkg["viewspace_points"], pkg["radii"],
                                **({"viewspace_abs": pkg["viewspace_points_abs"]} if abs_grad else {}))
        for p in model.parameters():
            p.grad = None

    kinds = {"step": False, "step, abs_grad": True}
    for flag in kinds.values():
        _timed(dev, lambda: step(flag), 3)
    rows = {k: [] for k in kinds}
    for r in range(args.rounds):
        for k, flag in kinds.items():
            us = _timed(dev, lambda: step(flag), args.steps)
            rows[k].append(round(us, 1))
            print(f"round {r} {k}: {us:.1f} us per step")
    return {"us_per_step": rows}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args(argv)
    out = {"config": args.config, "iters": args.iters, "steps": args.steps}
    out.update(bench_calls(args))
    torch.cuda.empty_cache()
    out.update(bench_steps(args))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
