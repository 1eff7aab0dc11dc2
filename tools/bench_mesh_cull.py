"""Device time of the per-vertex view counts (csrc/mesh_cull.hip; ``mesh.vertex_view_counts``) on the mesh of
tools/bench_mesh_clean.py (fused from the eight orbit views of a synthetic bench scene), against the same rule written
in torch ops on the same GPU: per view one matmul, the rounding, one index gather per map, and two accumulations.

    PYTHONPATH=. python tools/bench_mesh_cull.py [--config C4] [--resolution 256] [--views 64 300] [--iters 20] [--warmup 3]

The views are orbit cameras of the scene's size; each view's depth map is its own rendered surface and its mask is where
that surface exists.  Timed: S = 64 (DTU) and S = 300, each without maps, with masks, with depths and with both, in the
order marching tetrahedra emits the vertices (grid order: neighbouring lanes gather neighbouring pixels) and in a
shuffled order.  Whole calls, HIP events around the call (the host's table build and its one small copy included),
median over ``--iters`` calls after ``--warmup``; the kernel alone is the same call through the entry point with the table
already on the device.  The torch formulation's matmul contracts differently, so its counts may differ on pairs that sit
on a pixel or depth boundary: the share of vertices on which they do is printed and must stay below 0.1 %.
"""
import argparse
import json
import statistics
import sys

import torch

from mvs_gaussian_splatting_amd import TSDFVolume, _lib, fuse_views, render, vertex_view_counts
from mvs_gaussian_splatting_amd.mvs import _focal
from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene, orbit_camera
from mvs_gaussian_splatting_amd.tsdf import render_surface


def call_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return [round(x, 4) for x in (statistics.median(out), min(out), max(out))]


def torch_counts(vertices, views, masks, depths, near, depth_tol):
    """The rule of vertex_view_counts in torch ops; ``views[k] = (world_to_view [4,4] on the device, W, H, fx, fy)``."""
    V = vertices.shape[0]
    hom = torch.cat((vertices, torch.ones((V, 1), dtype=vertices.dtype, device=vertices.device)), dim=1)
    in_view = torch.zeros(V, dtype=torch.int32, device=vertices.device)
    visible = torch.zeros(V, dtype=torch.int32, device=vertices.device)
    for (M, W, H, fx, fy), mask, depth in zip(views, masks, depths):
        p = hom @ M
        zv = p[:, 2]
        ix = torch.floor((fx * p[:, 0]) / zv + (W - 1) * 0.5 + 0.5)
        iy = torch.floor((fy * p[:, 1]) / zv + (H - 1) * 0.5 + 0.5)
        inside = (zv > near) & (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
        seen = inside
        if mask is not None or depth is not None:
            idx = torch.where(inside, iy * W + ix, torch.zeros_like(ix)).long()
            if mask is not None:
                seen = seen & (mask.reshape(-1)[idx] != 0)
            if depth is not None:
                ds = depth.reshape(-1)[idx]
                seen = seen & (ds > 0) & (zv - ds <= depth_tol * ds)
        in_view += inside
        visible += seen
    return in_view, visible


def kernel_only(vertices, cameras, masks, depths, near, depth_tol):
    """-> a closure that launches gsr_cull_view_counts with the table already on the device."""
    table = (_lib.GsrCullView * len(cameras))()
    for k, cam in enumerate(cameras):
        H, W, fx, fy = _focal(cam)
        row = table[k]
        row.width, row.height, row.fx, row.fy = W, H, fx, fy
        row.world_to_view[:] = cam.world_view_transform.detach().cpu().float().reshape(-1).tolist()
        row.mask = None if masks[k] is None else masks[k].data_ptr()
        row.depth = None if depths[k] is None else depths[k].data_ptr()
    dev = vertices.device
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
    V = int(vertices.shape[0])
    in_view = torch.empty(V, dtype=torch.int32, device=dev)
    visible = torch.empty(V, dtype=torch.int32, device=dev)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        _lib.check(lib.gsr_cull_view_counts(vertices.data_ptr(), V, table_dev.data_ptr(), len(cameras), near, depth_tol, 0,
                                            in_view.data_ptr(), visible.data_ptr(), stream), "gsr_cull_view_counts")
    launch.keep = (table_dev, in_view, visible)
    return launch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, nargs="+", default=[64, 300])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--near", type=float, default=0.2)
    ap.add_argument("--depth_tol", type=float, default=0.01)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_cull needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    model, _, bg, _ = make_scene(cfg, seed=0, device=dev)
    pipe = PipelineParams()
    cams = [orbit_camera(v, 8, cfg.width, cfg.height, cfg.fx, cfg.fy, device=dev) for v in range(8)]
    voxel = 6.0 / (args.resolution - 1)
    vol = TSDFVolume((-3.0, -3.0, 3.0), voxel, (args.resolution,) * 3, 4 * voxel, device=dev)
    fuse_views(cams, model, pipe, bg, vol, renderer=render)
    vertices, faces, _ = vol.extract_mesh()
    del vol
    V = int(vertices.shape[0])
    shuffled = vertices[torch.randperm(V, device=dev, generator=torch.Generator(device=dev).manual_seed(0))].contiguous()
    res = {"config": args.config, "resolution": args.resolution, "vertices": V, "faces": int(faces.shape[0]),
           "image": [cfg.width, cfg.height], "iters": args.iters}
    print(f"mesh: {V} vertices, {faces.shape[0]} faces; views of {cfg.width} x {cfg.height}")
    for S in args.views:
        cameras = [orbit_camera(v, S, cfg.width, cfg.height, cfg.fx, cfg.fy, device=dev) for v in range(S)]
        with torch.no_grad():
            all_depths = [render_surface(render, cam, model, pipe, bg, 0.5, 0.0)[0].reshape(cfg.height, cfg.width).contiguous()
                          for cam in cameras]
        all_masks = [(d > 0).to(torch.uint8) for d in all_depths]
        views = [(cam.world_view_transform.detach().to(dev).float(), *(_focal(cam)[k] for k in (1, 0, 2, 3))) for cam in cameras]
        none = [None] * S
        for label, masks, depths in (("no maps", none, none), ("masks", all_masks, none), ("depths", none, all_depths),
                                     ("masks and depths", all_masks, all_depths)):
            out = res[f"S{S} {label}"] = {}
            for order, pts in (("grid order", vertices), ("shuffled", shuffled)):
                kw = dict(masks=masks, depths=depths, near=args.near, depth_tol=args.depth_tol)
                got = vertex_view_counts(pts, cameras, **kw)
                ref = torch_counts(pts, views, masks, depths, args.near, args.depth_tol)
                off = max(int((got[0] != ref[0]).sum()), int((got[1] != ref[1]).sum())) / V
                assert off < 1e-3, f"the torch formulation differs on {off:.2%} of the vertices"
                launch = kernel_only(pts, cameras, masks, depths, args.near, args.depth_tol)
                row = out[order] = {
                    "vertex_view_counts_ms": call_ms(lambda: vertex_view_counts(pts, cameras, **kw), args.iters, args.warmup),
                    "kernel_ms": call_ms(launch, args.iters, args.warmup),
                    "torch_ops_ms": call_ms(lambda: torch_counts(pts, views, masks, depths, args.near, args.depth_tol),
                                            args.iters, args.warmup),
                    "torch_differs_on": off, "visible_somewhere": int((got[1] > 0).sum()),
                }
                row["pairs_per_us_kernel"] = round(V * S / (row["kernel_ms"][0] * 1e3), 1)
                print(f"[S={S}, {label}, {order}] vertex_view_counts {row['vertex_view_counts_ms'][0]:.3f} ms (kernel "
                      f"{row['kernel_ms'][0]:.3f} ms, {row['pairs_per_us_kernel']} pairs/us), torch ops "
                      f"{row['torch_ops_ms'][0]:.3f} ms ({row['torch_ops_ms'][0] / row['vertex_view_counts_ms'][0]:.1f} x); "
                      f"torch differs on {100 * off:.4f} % of the vertices; {row['visible_somewhere']} visible somewhere")
        del all_depths, all_masks
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
