"""Times the per-view evaluation of a report (train.py:217-235, metrics.py:71-78) at 1920x1080: the fused HIP passes of
mvs_gaussian_splatting_amd.metrics against the same arithmetic as torch ops on the device.

  1  report arithmetic (two clamps, l1_loss, psnr, the two .double() running sums)  vs  image_metrics(accumulate=acc)
  2  the same with SSIM (11x11 grouped convolutions)                                vs  image_metrics(with_ssim=True, ...)
  3  the 8-bit chain + permute().contiguous()  vs  to_uint8_hwc  vs  the byte image fused into pass 1
  4  (--views) evaluate_views over the eight C5 views at C4 vs the torch loop around the same render()

One process, the variants of a part alternate, every shape warmed up; a window of --calls back-to-back calls between two
device events (a single call lasts tens of microseconds), --windows windows per variant: median, min and max per call.
Byte model of the fused pass: 2 * 12 * H*W bytes in (+ 3 * H*W out with the byte image), against the 6.3 TB/s streaming
rate measured elsewhere in this project (profiles/adam/NOTES.md).  One JSON line per result.

    python tools/bench_eval.py [--calls 50] [--windows 9] [--views] [--launches N]

--launches N: no timing; run every variant N times after one warm-up call each, printing marker lines, for a kernel
trace taken in a run of its own (the launch count of a torch chain = its kernel calls / N).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import EvalAccumulator, evaluate_views, image_metrics, render, to_uint8_hwc  # noqa: E402

ACHIEVABLE_TBS = 6.3


def torch_psnr(a, b):
    mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def make_window(dev):
    w1 = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], device=dev)
    w1 = (w1 / w1.sum()).unsqueeze(1)
    return (w1 @ w1.t()).expand(3, 1, 11, 11).contiguous()


def torch_ssim(p, q, win):
    p, q = p[None], q[None]
    m1, m2 = F.conv2d(p, win, padding=5, groups=3), F.conv2d(q, win, padding=5, groups=3)
    s1 = F.conv2d(p * p, win, padding=5, groups=3) - m1 * m1
    s2 = F.conv2d(q * q, win, padding=5, groups=3) - m2 * m2
    s12 = F.conv2d(p * q, win, padding=5, groups=3) - m1 * m2
    return (((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (s1 + s2 + 9e-4))).mean()


def windows(variants, calls, nwin, warmup=3):
    """variants: {name: callable}.  -> {name: [us per call of each window]}, the variants alternating."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(nwin):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / calls)
    return out


def report(part, times, extra=None):
    for name, us in times.items():
        row = {"part": part, "variant": name, "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2),
               "max_us": round(max(us), 2), "windows": len(us)}
        row.update((extra or {}).get(name, {}))
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--views", action="store_true", help="part 4: eight C5 views at C4 (6 M Gaussians)")
    ap.add_argument("--launches", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval needs a GPU")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.rand(3, H, W, device=dev, generator=g)
    img = gt + 0.05 * torch.randn(3, H, W, device=dev, generator=g) + 0.02
    win = make_window(dev)
    acc = EvalAccumulator(dev)
    sums = torch.zeros(3, dtype=torch.float64, device=dev)
    u8 = torch.empty(H, W, 3, dtype=torch.uint8, device=dev)

    def torch_report(with_ssim=False):
        a, b = torch.clamp(img, 0.0, 1.0), torch.clamp(gt, 0.0, 1.0)
        sums[0] += (a - b).abs().mean().mean().double()
        sums[1] += torch_psnr(a, b).mean().double()
        if with_ssim:
            sums[2] += torch_ssim(a, b, win).double()

    parts = {
        "1 report": {"torch": torch_report, "hip": lambda: image_metrics(img, gt, accumulate=acc)},
        "2 report+ssim": {"torch": lambda: torch_report(True),
                          "hip": lambda: image_metrics(img, gt, with_ssim=True, accumulate=acc)},
        "3 uint8": {"torch": lambda: (img.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).contiguous(),
                    "hip": lambda: to_uint8_hwc(img),
                    "hip fused with 1": lambda: image_metrics(img, gt, out_u8=u8, accumulate=acc)},
    }
    if args.launches:
        for part, variants in parts.items():
            for name, fn in variants.items():
                fn()
                torch.cuda.synchronize()
                print(f"launches: {part} / {name} x {args.launches}", flush=True)
                for _ in range(args.launches):
                    fn()
                torch.cuda.synchronize()
        return
    px = H * W
    model_b = {"hip": 24 * px, "hip fused with 1": 27 * px}
    for part, variants in parts.items():
        t = windows(variants, args.calls, args.windows)
        extra = {}
        if part != "2 report+ssim":
            for name in variants:
                if name.startswith("hip"):
                    b = 15 * px if part == "3 uint8" and name == "hip" else model_b[name]
                    tbs = b / (statistics.median(t[name]) * 1e-6) / 1e12
                    extra[name] = {"model_MB": round(b / 1e6, 1), "TBps": round(tbs, 3), "of_achievable": round(tbs / ACHIEVABLE_TBS, 3)}
        report(part, t, extra)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = max(max(v) - min(v) for v in t.values())
        print(json.dumps({"part": part, "speedup_vs_torch": {k: round(med["torch"] / v, 2) for k, v in med.items() if k != "torch"},
                          "largest_window_spread_us": round(spread, 2)}), flush=True)
    if args.views:
        from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene, orbit_camera
        cfg = CONFIGS["C4"]
        model, _, bg, _ = make_scene(cfg)
        model.to(dev)
        bg, pipe = bg.to(dev), PipelineParams()
        cams = [orbit_camera(v, 8, cfg.width, cfg.height, cfg.fx, cfg.fy, device=dev) for v in range(8)]
        gts = [torch.rand(3, cfg.height, cfg.width, device=dev, generator=g) for _ in cams]

        def torch_loop():
            l1_test = torch.zeros((), dtype=torch.float64, device=dev)
            psnr_test = torch.zeros((), dtype=torch.float64, device=dev)
            with torch.no_grad():
                for cam, t in zip(cams, gts):
                    image = torch.clamp(render(cam, model, pipe, bg)["render"], 0.0, 1.0)
                    gt_image = torch.clamp(t, 0.0, 1.0)
                    l1_test += (image - gt_image).abs().mean().mean().double()
                    psnr_test += torch_psnr(image, gt_image).mean().double()
            return float(l1_test / len(cams)), float(psnr_test / len(cams))

        def render_only():
            with torch.no_grad():
                for cam in cams:
                    render(cam, model, pipe, bg)
            torch.cuda.synchronize()

        variants = {"render only": render_only, "torch loop": torch_loop,
                    "evaluate_views": lambda: evaluate_views(cams, model, pipe, bg, gt_images=gts)}
        t = windows(variants, 1, max(3, args.windows // 2), warmup=2)
        t = {k: [u / 8 for u in v] for k, v in t.items()}                 # per view
        report(f"4 eight C5 views at C4 ({cfg.width}x{cfg.height}), us per view", t)
        med = {k: statistics.median(v) for k, v in t.items()}
        print(json.dumps({"part": "4", "metrics_share_of_a_view": {
            "torch loop": round(1 - med["render only"] / med["torch loop"], 4),
            "evaluate_views": round(1 - med["render only"] / med["evaluate_views"], 4)}}), flush=True)


if __name__ == "__main__":
    main()
