"""Device time of the mesh rasterizer (csrc/mesh_raster.hip; ``mesh.rasterize_mesh``, ``mesh.face_view_counts``) on the
mesh of tools/bench_mesh_cull.py (fused from the eight orbit views of a synthetic bench scene), rendered from orbit
cameras of the scene's size.

    PYTHONPATH=. python tools/bench_mesh_raster.py [--config C4] [--resolution 256] [--views 64 300] [--iters 20] [--warmup 3]

Reported, HIP events around the calls, median over ``--iters`` after ``--warmup``:

* one view's rasterize plus resolve through the entry points, workspaces allocated once (and ``rasterize_mesh``, the whole
  call with its allocations);
* the same rasterize with the load in front of the atomicMin disabled (GSR_RASTER_NO_LOAD_SKIP): the A/B of that skip;
* the same with the vertices taken to view space once per view into a scratch ``[V,3]`` (``view_scratch``) instead of per
  face on the fly: the A/B behind the default;
* ``face_view_counts`` over S views, and ``vertex_view_counts`` (no maps) on the same mesh and views, for scale.

All three rasterize variants must give the same keys; that is checked before anything is timed.
"""
import argparse
import ctypes as C
import json
import statistics
import sys

import torch

from mvs_gaussian_splatting_amd import (TSDFVolume, _lib, face_view_counts, fuse_views, rasterize_mesh, render,
                                        vertex_view_counts)
from mvs_gaussian_splatting_amd.mesh import _raster_rows
from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene, orbit_camera


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, nargs="+", default=[64, 300])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--near", type=float, default=0.2)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_raster needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    model, _, bg, _ = make_scene(cfg, seed=0, device=dev)
    cams = [orbit_camera(v, 8, cfg.width, cfg.height, cfg.fx, cfg.fy, device=dev) for v in range(8)]
    voxel = 6.0 / (args.resolution - 1)
    vol = TSDFVolume((-3.0, -3.0, 3.0), voxel, (args.resolution,) * 3, 4 * voxel, device=dev)
    fuse_views(cams, model, PipelineParams(), bg, vol, renderer=render)
    vertices, faces, _ = vol.extract_mesh()
    del vol, model
    V, F, W, H = int(vertices.shape[0]), int(faces.shape[0]), cfg.width, cfg.height
    res = {"config": args.config, "resolution": args.resolution, "vertices": V, "faces": F, "image": [W, H], "iters": args.iters,
           "lane_pixels": _lib.RASTER_LANE_PIXELS, "drain_waves": _lib.RASTER_DRAIN_WAVES}
    print(f"mesh: {V} vertices, {F} faces; views of {W} x {H}")

    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    row, = _raster_rows([cams[0]])
    keys = torch.empty(H * W, dtype=torch.int64, device=dev)
    qbytes = lib.gsr_raster_queue_bytes(F)
    queue = torch.empty(qbytes, dtype=torch.uint8, device=dev)
    scratch = torch.empty((V, 3), dtype=torch.float32, device=dev)
    depth = torch.empty((H, W), dtype=torch.float32, device=dev)
    face_id = torch.empty((H, W), dtype=torch.int32, device=dev)

    def view(flags=0, view_scratch=None, into=keys):
        _lib.check(lib.gsr_raster_view(vertices.data_ptr(), V, faces.data_ptr(), F, C.byref(row), args.near,
                                       _lib.RASTER_CLEAR | flags, into.data_ptr(), queue.data_ptr(), qbytes,
                                       None if view_scratch is None else view_scratch.data_ptr(), stream), "gsr_raster_view")

    def resolve():
        _lib.check(lib.gsr_raster_resolve(keys.data_ptr(), H, W, depth.data_ptr(), face_id.data_ptr(), stream),
                   "gsr_raster_resolve")

    view()
    head = queue[:12].view(torch.int32).tolist()
    other = torch.empty_like(keys)
    for kw in ({"flags": _lib.RASTER_NO_LOAD_SKIP}, {"view_scratch": scratch}):
        view(into=other, **kw)
        assert torch.equal(other, keys), f"{kw} changes the keys"
    resolve()
    res["one_view"] = one = {
        "queued_pieces": head[0], "dropped": head[1], "covered_pixels": int((face_id >= 0).sum()),
        "faces_owning_a_pixel": int(face_id[face_id >= 0].unique().numel()),
        "rasterize_ms": call_ms(view, args.iters, args.warmup),
        "resolve_ms": call_ms(resolve, args.iters, args.warmup),
        "rasterize_plus_resolve_ms": call_ms(lambda: (view(), resolve()), args.iters, args.warmup),
        "rasterize_no_load_skip_ms": call_ms(lambda: view(flags=_lib.RASTER_NO_LOAD_SKIP), args.iters, args.warmup),
        "rasterize_view_scratch_ms": call_ms(lambda: view(view_scratch=scratch), args.iters, args.warmup),
        "rasterize_mesh_call_ms": call_ms(lambda: rasterize_mesh(vertices, faces, cams[0], near=args.near), args.iters, args.warmup),
    }
    one["faces_per_us"] = round(F / (one["rasterize_ms"][0] * 1e3), 1)
    print(f"[one view] rasterize {one['rasterize_ms'][0]:.3f} ms ({one['faces_per_us']} faces/us), resolve "
          f"{one['resolve_ms'][0]:.3f} ms, both {one['rasterize_plus_resolve_ms'][0]:.3f} ms; without the load-before-atomic skip "
          f"{one['rasterize_no_load_skip_ms'][0]:.3f} ms; vertices to view space once per view {one['rasterize_view_scratch_ms'][0]:.3f} "
          f"ms; rasterize_mesh, whole call {one['rasterize_mesh_call_ms'][0]:.3f} ms; {head[0]} queued pieces, "
          f"{one['covered_pixels']} covered pixels, {one['faces_owning_a_pixel']} faces own one")
    for S in args.views:
        cameras = [orbit_camera(v, S, W, H, cfg.fx, cfg.fy, device=dev) for v in range(S)]
        counts = face_view_counts(vertices, faces, cameras, near=args.near)
        iters = max(3, args.iters // 4)
        out = res[f"S{S}"] = {
            "faces_seen_somewhere": int((counts > 0).sum()),
            "face_view_counts_ms": call_ms(lambda: face_view_counts(vertices, faces, cameras, near=args.near), iters, 1),
            "vertex_view_counts_ms": call_ms(lambda: vertex_view_counts(vertices, cameras, near=args.near), iters, 1),
        }
        print(f"[S={S}] face_view_counts {out['face_view_counts_ms'][0]:.3f} ms ({out['face_view_counts_ms'][0] / S:.3f} ms a view), "
              f"vertex_view_counts (no maps) {out['vertex_view_counts_ms'][0]:.3f} ms; {out['faces_seen_somewhere']} of {F} faces "
              f"seen somewhere")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
