"""Device time of the multi-view depth consistency check (csrc/mvs.hip, ``mvs_consistency_kernel``)
beside a torch implementation of the same check (matrix ops and ``grid_sample``) in the same run, from HIP events.

    PYTHONPATH=. python tools/bench_mvs.py [--iters 20] [--rounds 3] [--alt-lib tools/ab/mvs_tile16.so]

One 1920 x 1080 reference against 4 and 8 sources of the same size: cameras 5 degrees apart on an orbit about a slanted
plane at depth 6 (``synthetic.orbit_camera`` of 72 views), analytic depth maps, every pixel valid.  Reported per case:
ms per call of the kernel and of the torch yardstick, their agreement (share of pixels with the same count), and the
bytes / s on the compulsory traffic -- the reference depth in (4 bytes a pixel), the two outputs out (1 + 4), and four
gathered floats per pixel and source (16 S): ``H W (9 + 16 S)`` bytes.  ``--alt-lib``: a second build of the library
(``tools/build_variant.sh mvs_tile16 mvs_gaussian_splatting_amd/csrc/mvs.hip -DMVS_TILE_X=16``: 16 x 16 pixel tiles
instead of 64 x 4) timed through the same raw call on the same inputs.
"""
import argparse
import ctypes as C
import json
import math
import sys

import numpy as np
import torch
import torch.nn.functional as F

from mvs_gaussian_splatting_amd import _lib, depth_consistency
from mvs_gaussian_splatting_amd.mvs import _focal, _view64
from mvs_gaussian_splatting_amd.synthetic import orbit_camera

PLANE_N, PLANE_C = (0.05, 0.03, 1.0), 6.0


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def plane_depth(cam, dev):
    H, W, fx, fy = _focal(cam)
    c2w = torch.from_numpy(np.linalg.inv(_view64(cam))).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    ray = torch.stack(((xs - (W - 1) / 2) / fx, (ys - (H - 1) / 2) / fy, torch.ones_like(xs)), dim=-1) @ c2w[:3, :3]
    n = torch.tensor(PLANE_N, dtype=torch.float64, device=dev)
    t = (PLANE_C - c2w[3, :3] @ n) / (ray @ n)
    return torch.where(t > 0, t, torch.zeros_like(t)).to(torch.float32).contiguous()


def torch_check(depth, cam, src_depths, src_cams, pix_thresh, depth_thresh, min_views):
    """The same check in torch ops: one grid_sample of the depth and one of its validity mask per source."""
    dev = depth.device
    H, W, fx, fy = _focal(cam)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    p = torch.stack(((xs - cx) * depth / fx, (ys - cy) * depth / fy, depth, torch.ones_like(depth)), dim=-1)
    has = depth > 0
    n = torch.zeros((H, W), dtype=torch.int32, device=dev)
    total = torch.zeros((H, W), device=dev)
    Mr = _view64(cam)
    for sd, sc in zip(src_depths, src_cams):
        Hs, Ws, fxs, fys = _focal(sc)
        Ms = _view64(sc)
        A = torch.from_numpy((np.linalg.inv(Mr) @ Ms).astype(np.float32)).to(dev)
        B = torch.from_numpy((np.linalg.inv(Ms) @ Mr).astype(np.float32)).to(dev)
        q = p @ A
        zs = q[..., 2]
        us, vs = fxs * q[..., 0] / zs + (Ws - 1) * 0.5, fys * q[..., 1] / zs + (Hs - 1) * 0.5
        inside = (zs > 0.2) & (us >= 0) & (us < Ws - 1) & (vs >= 0) & (vs < Hs - 1)
        grid = torch.stack((2 * us / (Ws - 1) - 1, 2 * vs / (Hs - 1) - 1), dim=-1)[None]
        both = torch.stack((sd, (sd > 0).to(torch.float32)))[None]
        ds, mask = F.grid_sample(both, grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0]
        back = torch.stack(((us - (Ws - 1) * 0.5) * ds / fxs, (vs - (Hs - 1) * 0.5) * ds / fys, ds, torch.ones_like(ds)), dim=-1) @ B
        zb = back[..., 2]
        du, dv = fx * back[..., 0] / zb + cx - xs, fy * back[..., 1] / zb + cy - ys
        ok = has & inside & (mask > 0.9999) & (zb > 0.2) & (du * du + dv * dv < pix_thresh ** 2) \
            & ((zb - depth).abs() < depth_thresh * depth)
        n += ok
        total += torch.where(ok, zb, torch.zeros_like(zb))
    fused = torch.where(has & (n >= min_views), (depth + total) / (n + 1), torch.zeros_like(depth))
    return n.to(torch.uint8), fused


def raw_call(lib, depth, cam, src_depths, src_cams, pix_thresh, depth_thresh, min_views):
    """A closure that launches ``lib``'s kernel on a table built once -> (call, count, fused)."""
    dev = depth.device
    H, W, fx, fy = _focal(cam)
    table = (_lib.GsrMvsSource * len(src_cams))()
    Mr = _view64(cam)
    for row, sd, sc in zip(table, src_depths, src_cams):
        Hs, Ws, fxs, fys = _focal(sc)
        Ms = _view64(sc)
        row.depth, row.width, row.height, row.fx, row.fy = sd.data_ptr(), Ws, Hs, fxs, fys
        A, B = (np.linalg.inv(Mr) @ Ms).astype(np.float32).reshape(-1), (np.linalg.inv(Ms) @ Mr).astype(np.float32).reshape(-1)
        for i in range(16):
            row.ref_to_src[i], row.src_to_ref[i] = float(A[i]), float(B[i])
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    count = torch.empty((H, W), dtype=torch.uint8, device=dev)
    fused = torch.empty((H, W), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    fn = lib.gsr_mvs_consistency
    fn.restype, fn.argtypes = _lib.SYMBOLS["gsr_mvs_consistency"]

    def call():
        rc = fn(depth.data_ptr(), H, W, fx, fy, table_dev.data_ptr(), len(src_cams), pix_thresh, depth_thresh, min_views,
                count.data_ptr(), fused.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"gsr_mvs_consistency failed: {rc}")
    return call, count, fused, table_dev


def bench(iters, rounds, alt_lib, dev):
    W, H, f = 1920, 1080, 1200.0
    cams = [orbit_camera(v % 72, 72, W, H, f, f, device=dev) for v in (0, 1, -1, 2, -2, 3, -3, 4, -4)]
    depths = [plane_depth(c, dev) for c in cams]
    libs = {"tile 64x4 (in-tree)": _lib.load()}
    if alt_lib:
        libs[f"alt ({alt_lib})"] = C.CDLL(alt_lib)
    out = {}
    for S in (4, 8):
        sd, sc = depths[1:1 + S], cams[1:1 + S]
        traffic = H * W * (9 + 16 * S)
        row = {"sources": S, "compulsory_bytes": traffic}
        want_n, want_f = torch_check(depths[0], cams[0], sd, sc, 1.0, 0.01, 2)
        for name, lib in libs.items():
            call, count, fused, keep = raw_call(lib, depths[0], cams[0], sd, sc, 1.0, 0.01, 2)
            timed(call, 3)
            ms = [timed(call, iters) for _ in range(rounds)]
            same = float((count == want_n).float().mean())
            row[name] = {"ms": [round(m, 4) for m in ms], "GB_per_s": round(traffic / min(ms) / 1e6, 1),
                         "count_equal_to_torch": round(same, 6), "mean_count": round(float(count.float().mean()), 4)}
            print(f"S={S} {name}: {min(ms):.4f} ms, {traffic / min(ms) / 1e6:.0f} GB/s on {traffic / 1e6:.1f} MB; "
                  f"count equals torch's on {same:.4%} of the pixels, mean count {float(count.float().mean()):.3f}")
            del keep
        wrapper = lambda: depth_consistency(depths[0], cams[0], sd, sc)      # noqa: E731,B023
        timed(wrapper, 3)
        row["wrapper_ms"] = round(min(timed(wrapper, iters) for _ in range(rounds)), 4)
        ref = lambda: torch_check(depths[0], cams[0], sd, sc, 1.0, 0.01, 2)      # noqa: E731,B023
        timed(ref, 2)
        ms = [timed(ref, max(2, iters // 4)) for _ in range(rounds)]
        row["torch"] = {"ms": [round(m, 4) for m in ms]}
        print(f"S={S} torch (matrix ops + grid_sample): {min(ms):.3f} ms; the wrapper with its table upload {row['wrapper_ms']:.4f} ms")
        out[f"S{S}"] = row
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--alt-lib", default=None, help="a second build of libgsr_hip.so to time through the same raw call")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvs needs a GPU: a CPU run measures nothing")
    print(json.dumps(bench(args.iters, args.rounds, args.alt_lib, torch.device("cuda:0"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
