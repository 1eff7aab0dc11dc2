"""Device time of the TSDF kernels (csrc/tsdf.hip): integration of one view into a dense volume, with and without
colour, from HIP events, as milliseconds and as the share of the streaming rate the bytes actually touched would allow;
and the extraction of a volume fused from the eight orbit views of a synthetic bench scene.

    PYTHONPATH=. python tools/bench_tsdf.py [--dim 512] [--config C4] [--resolution 256] [--iters 10] [--rounds 3]

Integration inputs: a 1920 x 1080 depth map of a slanted plane through the volume (every pixel valid), the camera
at the origin looking down +z, the volume in front of it so that the whole grid projects into the image.  Bytes touched
are counted from the result, not from the shape: 16 B per updated point (tsdf and weight, read and written) -- a point's
fields are read only after it passed the depth tests, so a skipped point moves no field bytes -- plus 24 B per updated
point with colour.  STREAM_TBPS is the measured float4-copy rate of the MI355X (6.29 TB/s).
"""
import argparse
import json
import math
import sys
import time

import torch

from mvs_gaussian_splatting_amd import TSDFVolume, fuse_views, render
from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene, orbit_camera

STREAM_TBPS = 6.29


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def bench_integrate(dim, iters, rounds, dev):
    W, H, f = 1920, 1080, 1200.0
    cam = orbit_camera(0, 8, W, H, f, f, device=dev)
    extent = 3.0                                                   # the grid spans 3 units at depth 4.5 .. 7.5
    voxel = extent / (dim - 1)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    depth = (6.0 + 0.3 * (xs - W / 2) / W + 0.2 * (ys - H / 2) / H).float().contiguous()
    color = torch.rand(3, H, W, device=dev)
    out = {}
    for with_color in (False, True):
        vol = TSDFVolume((-extent / 2, -extent / 2, 4.5), voxel, (dim, dim, dim), 4 * voxel, with_color=with_color,
                         device=dev)
        call = lambda: vol.integrate(depth, cam, color=color if with_color else None)      # noqa: E731
        timed(call, 2)
        updated = int((vol.weight > 0).sum())
        moved = updated * (16 + (24 if with_color else 0))
        ms = [timed(call, iters) for _ in range(rounds)]
        best = min(ms)
        out["color" if with_color else "plain"] = {
            "ms_per_view": [round(m, 4) for m in ms], "updated_points": updated, "points": dim ** 3,
            "bytes_touched": moved, "share_of_stream_rate": round(moved / (best * 1e-3) / (STREAM_TBPS * 1e12), 4)}
        print(f"integrate {dim}^3 colour={with_color}: {best:.3f} ms per view, {updated} of {dim ** 3} points updated, "
              f"{moved / 1e9:.2f} GB touched, {out['color' if with_color else 'plain']['share_of_stream_rate']:.3f} of "
              f"{STREAM_TBPS} TB/s")
        del vol
    return out


def bench_extract(config, resolution, rounds, dev):
    cfg = CONFIGS[config]
    model, _, bg, _ = make_scene(cfg, seed=0, device=dev)
    cams = [orbit_camera(v, 8, cfg.width, cfg.height, cfg.fx, cfg.fy, device=dev) for v in range(8)]
    extent = 6.0
    voxel = extent / (resolution - 1)
    vol = TSDFVolume((-3.0, -3.0, 3.0), voxel, (resolution,) * 3, 4 * voxel, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fuse_views(cams, model, PipelineParams(), bg, vol, renderer=render)
    torch.cuda.synchronize()
    fuse_ms = 1e3 * (time.perf_counter() - t0)
    vol.extract_mesh()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v, f, _ = vol.extract_mesh()
        torch.cuda.synchronize()
        ms.append(round(1e3 * (time.perf_counter() - t0), 3))
    print(f"extract {config} {resolution}^3: {min(ms):.2f} ms, {v.shape[0]} vertices, {f.shape[0]} faces "
          f"(fusing the 8 views, first frames included: {fuse_ms:.0f} ms)")
    return {"config": config, "resolution": resolution, "extract_ms": ms, "vertices": int(v.shape[0]),
            "faces": int(f.shape[0]), "fuse_8_views_ms_cold": round(fuse_ms, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--config", default="C4")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    res = {"integrate": bench_integrate(args.dim, args.iters, args.rounds, dev),
           "extract": bench_extract(args.config, args.resolution, args.rounds, dev)}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
