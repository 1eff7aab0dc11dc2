"""Device time of the bilateral-grid calls against their torch-op forms on the same card, from HIP events around batches
of calls on one stream.

    PYTHONPATH=. python tools/bench_bilagrid.py [--height 1080] [--width 1920] [--shape 16 16 8] [--images 300]
                                                [--iters 20] [--rounds 3]

  * slice forward + backward (dX and dG) through ``slice_bilateral_grid``, against ``F.grid_sample`` on the 5-D grid, the
    affine as torch ops, and autograd;
  * the forward alone with the cells read through the caches and with the whole grid staged in LDS
    (``GSR_BILAGRID_STAGE_CACHE`` / ``_LDS``);
  * the TV term over ``--images`` grids, value and gradient, against its torch-op form.

Prints every round's mean per call in microseconds, the agreement of the two sides as a relative L2, and one JSON line.
"""
import argparse
import json
import sys

import torch
import torch.nn.functional as F

from mvs_gaussian_splatting_amd import _lib, bilateral_grid_tv_loss, slice_bilateral_grid


def torch_slice(x, grid):
    H, W = x.shape[1:]
    xs = (torch.arange(W, device=x.device, dtype=x.dtype) + 0.5) / W
    ys = (torch.arange(H, device=x.device, dtype=x.dtype) + 0.5) / H
    gray = 0.299 * x[0] + 0.587 * x[1] + 0.114 * x[2]
    coords = torch.stack([xs[None, :].expand(H, W), ys[:, None].expand(H, W), gray], dim=-1)
    A = F.grid_sample(grid[None], (coords * 2.0 - 1.0)[None, None], mode="bilinear", padding_mode="border",
                      align_corners=True)[0, :, 0].reshape(3, 4, H, W)
    xt = torch.cat([x, torch.ones_like(x[:1])], dim=0)
    return (A * xt[None]).sum(dim=1)


def torch_tv(g):
    return (((g[:, :, 1:] - g[:, :, :-1]) ** 2).mean(dim=(1, 2, 3, 4)) +
            ((g[:, :, :, 1:] - g[:, :, :, :-1]) ** 2).mean(dim=(1, 2, 3, 4)) +
            ((g[:, :, :, :, 1:] - g[:, :, :, :, :-1]) ** 2).mean(dim=(1, 2, 3, 4))).mean()


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--shape", type=int, nargs=3, default=[16, 16, 8], metavar=("W", "H", "L"))
    ap.add_argument("--images", type=int, default=300)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_bilagrid needs a ROCm GPU", file=sys.stderr)
        return 1
    lib, dev = _lib.load(), torch.device("cuda:0")
    H, W = args.height, args.width
    Wg, Hg, L = args.shape
    torch.manual_seed(0)
    x = torch.rand(3, H, W, device=dev)
    up = torch.randn(3, H, W, device=dev) / (3 * H * W)
    eye = torch.eye(3, 4, device=dev).reshape(12, 1, 1, 1)
    grid = (eye + 0.1 * torch.randn(12, L, Hg, Wg, device=dev)).contiguous()
    grids = (eye[None] + 0.1 * torch.randn(args.images, 12, L, Hg, Wg, device=dev)).contiguous()
    y = torch.empty_like(x)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def fwd_bwd(op):
        def step():
            xi, gi = x.detach().requires_grad_(True), grid.detach().requires_grad_(True)
            op(xi, gi).backward(up)
            return xi.grad, gi.grad
        return step

    def tv_step(op):
        def step():
            gi = grids.detach().requires_grad_(True)
            v = op(gi)
            v.backward()
            return v.detach(), gi.grad
        return step

    def staged(kind):
        def step():
            _lib.check(lib.gsr_bilagrid_slice_fwd(x.data_ptr(), grid.data_ptr(), H, W, Wg, Hg, L, kind, y.data_ptr(),
                                                  stream), "fwd")
        return step

    sides = {"slice fwd+bwd hip": fwd_bwd(slice_bilateral_grid), "slice fwd+bwd torch": fwd_bwd(torch_slice),
             "fwd cache": staged(_lib.BILAGRID_STAGE_CACHE), "tv hip": tv_step(bilateral_grid_tv_loss),
             "tv torch": tv_step(torch_tv)}
    if 12 * L * Hg * Wg <= 24576:
        sides["fwd lds"] = staged(_lib.BILAGRID_STAGE_LDS)

    def run(fn, n):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        torch.cuda.synchronize(dev)
        return 1000.0 * start.elapsed_time(stop) / n

    a, b = sides["slice fwd+bwd hip"](), sides["slice fwd+bwd torch"]()
    agree = {"dX": rel_l2(a[0], b[0]), "dG": rel_l2(a[1], b[1]),
             "Y": rel_l2(slice_bilateral_grid(x, grid), torch_slice(x, grid))}
    a, b = sides["tv hip"](), sides["tv torch"]()
    agree.update({"tv": rel_l2(a[0], b[0]), "dtv": rel_l2(a[1], b[1])})
    print("relative L2 between the two sides:", ", ".join(f"{k} {v:.2e}" for k, v in agree.items()))
    for fn in sides.values():
        run(fn, 3)
    rows = {k: [] for k in sides}
    for r in range(args.rounds):
        for kind, fn in sides.items():
            us = run(fn, args.iters)
            rows[kind].append(round(us, 1))
            print(f"round {r} {kind}: {us:.1f} us per call")
    print(json.dumps({"height": H, "width": W, "shape": [Wg, Hg, L], "images": args.images, "iters": args.iters,
                      "lib": _lib.LIB_PATH, "agreement": agree, "call_us": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
