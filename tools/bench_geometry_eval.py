"""Device time of the cross-set nearest point (csrc/nearest.hip on the index of csrc/knn.hip; geometry_eval.py): the index
build and the query at ``--n`` x ``--n`` points on a uniform and on a clustered cloud, and ``evaluate_points`` on a mesh
sampled at ``--samples`` points against itself shifted by a third of a voxel, each against ``scipy.spatial.cKDTree`` on
the host for the same inputs.

    PYTHONPATH=. python tools/bench_geometry_eval.py [--n 1000000] [--resolution 256] [--samples 2000000]
                                                     [--iters 20] [--warmup 3] [--no_host]

HIP events around the native call (buffers allocated outside), median over ``--iters`` calls after ``--warmup``.  The mesh
is the one of tools/bench_tsdf.py / profiles/tsdf/NOTES.md: the volume fused from the eight orbit views of a synthetic
bench scene.  The host figure is the tree's build and its ``query(k=1)`` with all workers; its distances must agree with
the device's to 8 * 2^-24 relative.
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

from mvs_gaussian_splatting_amd import _lib, evaluate_points, sample_surface


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
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def clouds(kind, n, rng):
    if kind == "uniform":
        return rng.random((n, 3), dtype=np.float32), rng.random((n, 3), dtype=np.float32)
    # clustered: 200 Gaussian blobs of very different widths, as an SfM cloud is anything but uniform
    centres = rng.random((200, 3))
    widths = 10.0 ** rng.uniform(-4.0, -1.0, size=200)
    pick = lambda: rng.integers(0, 200, size=n)                                                   # noqa: E731
    make = lambda c: (centres[c] + rng.standard_normal((n, 3)) * widths[c, None]).astype(np.float32)   # noqa: E731
    return make(pick()), make(pick())


def bench_pair(ref, query, args, host):
    lib, dev = _lib.load(), torch.device("cuda:0")
    R, Q = len(ref), len(query)
    r, q = torch.from_numpy(ref).to(dev), torch.from_numpy(query).to(dev)
    ib, wb = lib.gsr_nn_index_bytes(R), lib.gsr_nn_query_workspace_bytes(Q)
    index = torch.empty(ib, dtype=torch.uint8, device=dev)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    d2 = torch.empty(Q, dtype=torch.float32, device=dev)
    nn = torch.empty(Q, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    build = lambda: _lib.check(lib.gsr_nn_build(r.data_ptr(), R, index.data_ptr(), ib, s), "build")          # noqa: E731
    query_fn = lambda: _lib.check(lib.gsr_nn_query(index.data_ptr(), ib, R, q.data_ptr(), Q, d2.data_ptr(),  # noqa: E731
                                                   nn.data_ptr(), ws.data_ptr(), wb, s), "query")
    out = {"R": R, "Q": Q, "index_bytes": ib, "workspace_bytes": wb,
           "build_ms": call_ms(build, args.iters, args.warmup), "query_ms": call_ms(query_fn, args.iters, args.warmup)}
    if host:
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        tree = cKDTree(ref.astype(np.float64))
        t1 = time.perf_counter()
        dist, _ = tree.query(query.astype(np.float64), k=1, workers=16)
        t2 = time.perf_counter()
        out["host_build_ms"], out["host_query_ms"] = round(1e3 * (t1 - t0), 1), round(1e3 * (t2 - t1), 1)
        got, want = d2.cpu().numpy().astype(np.float64), dist ** 2
        err = np.abs(got - want)[want > 0] / want[want > 0]
        out["worst_relative_error_vs_host"] = float(err.max()) if err.size else 0.0
        assert out["worst_relative_error_vs_host"] <= 8 * 2.0 ** -24 + 1e-12, out["worst_relative_error_vs_host"]
    return out


def bench_mesh(args, host):
    from mvs_gaussian_splatting_amd import TSDFVolume, fuse_views, render
    from mvs_gaussian_splatting_amd.synthetic import CONFIGS, PipelineParams, make_scene, orbit_camera
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    model, _, bg, _ = make_scene(cfg, seed=0, device=dev)
    cams = [orbit_camera(v, 8, cfg.width, cfg.height, cfg.fx, cfg.fy, device=dev) for v in range(8)]
    voxel = 6.0 / (args.resolution - 1)
    vol = TSDFVolume((-3.0, -3.0, 3.0), voxel, (args.resolution,) * 3, 4 * voxel, device=dev)
    fuse_views(cams, model, PipelineParams(), bg, vol, renderer=render)
    vertices, faces, _ = vol.extract_mesh()
    gen = torch.Generator().manual_seed(0)
    pred, _ = sample_surface(vertices, faces, args.samples, generator=gen)
    gt, _ = sample_surface(vertices + torch.tensor([voxel / 3, 0.0, 0.0], device=dev), faces, args.samples, generator=gen)
    taus = (voxel, 2 * voxel)
    out = {"vertices": int(vertices.shape[0]), "faces": int(faces.shape[0]), "samples": args.samples, "voxel": voxel,
           "sample_surface_ms": call_ms(lambda: sample_surface(vertices, faces, args.samples, generator=gen), args.iters,
                                        args.warmup),
           "evaluate_points_ms": call_ms(lambda: evaluate_points(pred, gt, thresholds=taus), args.iters, args.warmup),
           "result": evaluate_points(pred, gt, thresholds=taus)}
    if host:
        from scipy.spatial import cKDTree
        p, g = pred.cpu().numpy().astype(np.float64), gt.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        a = cKDTree(g).query(p, k=1, workers=16)[0].mean()
        c = cKDTree(p).query(g, k=1, workers=16)[0].mean()
        out["host_evaluate_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["host_chamfer"] = 0.5 * (a + c)
        assert abs(out["host_chamfer"] - out["result"]["chamfer"]) <= 1e-6 * out["host_chamfer"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--config", default="C4")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--samples", type=int, default=2_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no_host", action="store_true", help="skip the cKDTree figures")
    ap.add_argument("--no_mesh", action="store_true", help="skip the sampled-mesh evaluation")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry_eval needs a GPU: a CPU run measures nothing")
    res = {"n": args.n, "iters": args.iters}
    rng = np.random.default_rng(0)
    for kind in ("uniform", "clustered"):
        ref, query = clouds(kind, args.n, rng)
        res[kind] = bench_pair(ref, query, args, not args.no_host)
        o = res[kind]
        print(f"[{kind}] {o['R']} x {o['Q']}: build {o['build_ms'][0]:.3f} ms, query {o['query_ms'][0]:.3f} ms (median; min, max: "
              f"{o['build_ms'][1:]}, {o['query_ms'][1:]})" +
              ("" if args.no_host else f"; cKDTree build {o['host_build_ms']} ms, query {o['host_query_ms']} ms"), flush=True)
    if not args.no_mesh:
        res["mesh"] = o = bench_mesh(args, not args.no_host)
        print(f"[mesh] {o['faces']} faces, {o['samples']} samples each side: sample_surface {o['sample_surface_ms'][0]:.3f} ms, "
              f"evaluate_points {o['evaluate_points_ms'][0]:.3f} ms" +
              ("" if args.no_host else f"; two cKDTrees on the host {o['host_evaluate_ms']} ms"), flush=True)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
