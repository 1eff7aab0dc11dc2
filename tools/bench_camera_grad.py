"""Device time of the per-Gaussian backward stage (sum_big_rows + preprocess_bwd, and the camera finish kernel when it
runs) with and without camera gradients, from the library's own stage timers (HIP events around the stage).

    PYTHONPATH=.:tools python tools/bench_camera_grad.py [C4] [--iters 20] [--rounds 5] [--plain-only]

One forward of the scene, then ``rounds`` rounds that alternate ``iters`` plain backwards and ``iters`` camera backwards
(so that clock drift hits both); prints every round's mean per backward in microseconds and one JSON line with the raw
numbers.

A/B against a library built from the commit before the camera gradients (ABI 19): point ``GSR_LIB_PATH`` at it and pass
``--plain-only --base-abi 19``.  That ABI differs by the four members appended to ``GsrGrads`` (which such a library
never reads) and by ``gsr_camera_grad_bytes``; the tool then binds without that symbol.  Run it several times to get the
noise band of the base build, then run this build with ``--plain-only`` the same way.
"""
import argparse
import json
import sys

import torch

from mvs_gaussian_splatting_amd import _lib


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--base-abi", type=int, default=None)
    args = ap.parse_args(argv)
    if args.base_abi is not None and args.base_abi != _lib.ABI_VERSION:
        if not args.plain_only:
            ap.error("--base-abi needs --plain-only")
        _lib.ABI_VERSION = args.base_abi
        _lib.SYMBOLS.pop("gsr_camera_grad_bytes")
    from scene_gpu import GpuScene
    sc = GpuScene(args.config, fused=True)
    lib, dev, P = sc.lib, sc.dev, sc.P
    prof = _lib.StageProfile()
    sc.forward()
    dL = torch.rand(3, sc.H, sc.W, device=dev) / (3 * sc.H * sc.W)
    sc.backward(dL)                         # builds sc.grads (plain)
    cam_out = ws = None
    if not args.plain_only:
        cam_out = [torch.empty(16, device=dev), torch.empty(16, device=dev), torch.empty(3, device=dev)]
        ws = torch.empty(lib.gsr_camera_grad_bytes(P), dtype=torch.uint8, device=dev)

    def set_camera(on):
        g = sc.grads
        g.dL_dviewmatrix, g.dL_dprojmatrix, g.dL_dcampos = [t.data_ptr() for t in cam_out] if on else [None] * 3
        g.camera_ws = ws.data_ptr() if on else None

    def run(n):
        sc.params.profile = prof.handle()
        for _ in range(n):
            sc.backward(dL)
        torch.cuda.synchronize(dev)
        sc.params.profile = None
        ms, cnt = prof.collect()["preprocess_bwd"]
        return 1000.0 * ms / cnt

    run(3)
    rows = {"plain": [], "camera": []}
    for r in range(args.rounds):
        for kind in ("plain",) if args.plain_only else ("plain", "camera"):
            if not args.plain_only:
                set_camera(kind == "camera")
            us = run(args.iters)
            rows[kind].append(round(us, 2))
            print(f"round {r} {kind}: preprocess_bwd stage {us:.1f} us per backward")
    if cam_out is not None:
        print("camera gradients:", [t.cpu().tolist() for t in cam_out][2])
    print(json.dumps({"config": args.config, "P": P, "iters": args.iters, "lib": _lib.LIB_PATH, "stage_us": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
