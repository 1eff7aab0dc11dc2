"""Device time of the mesh simplification (csrc/mesh_simplify.hip; ``mesh.simplify_mesh``) on the mesh of
tools/bench_mesh_clean.py (fused from the eight orbit views of a synthetic bench scene), at cells of 2 and 4 TSDF voxels,
against the same rule written in torch ops: ``torch.unique(return_inverse=True)`` for the clusters, ``index_add_`` in
float64 for the means, a sort-unique over the rotated face triples and boolean indexing for the compaction.

    PYTHONPATH=. python tools/bench_mesh_simplify.py [--config C4] [--resolution 256] [--iters 20] [--warmup 3]

Whole calls: HIP events around the call (its host read-backs included), median over ``--iters`` calls after ``--warmup``.
Per stage: the same sequence of native calls and torch ops that ``simplify_mesh`` issues, with a HIP event between the
stages, median per stage; the read-backs are stages of their own, and the share of the three torch sorts is printed.
Run lengths: how many vertices the cells hold (mean, 99th percentile, longest), which is what the one-lane-per-cluster
reduce kernel walks.  The torch formulation must give the same faces and the same vertices (to one float32 spacing).
"""
import argparse
import json
import statistics
import sys

import torch

from mvs_gaussian_splatting_amd import TSDFVolume, _lib, fuse_views, render, simplify_mesh
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


class Stages:
    """Runs a list of (name, fn) on the current stream with an event between each; median ms per stage."""

    def __init__(self):
        self.ms = {}

    def run(self, stages):
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
        marks[0].record()
        for n, (_, fn) in enumerate(stages):
            fn()
            marks[n + 1].record()
        torch.cuda.synchronize()
        for n, (name, _) in enumerate(stages):
            self.ms.setdefault(name, []).append(marks[n].elapsed_time(marks[n + 1]))

    def medians(self, skip):
        return {k: round(statistics.median(v[skip:]), 4) for k, v in self.ms.items()}


def simplify_stages(vertices, faces, colors, h, timer):
    """The calls of simplify_mesh (default origin, colours, no map), one stage each."""
    lib, dev = _lib.load(), vertices.device
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    s = torch.cuda.current_stream(dev).cuda_stream
    ck, p, st = _lib.check, (lambda t: t.data_ptr()), {}
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def mark():
        st["every"] = torch.ones(F, dtype=torch.uint8, device=dev)
        st["vmark"] = torch.zeros(V, dtype=torch.uint8, device=dev)
        ck(lib.gsr_mesh_mark_vertices(p(faces), p(st["every"]), F, V, p(st["vmark"]), p(status), s), "mark")

    def origin():
        st["origin"] = torch.empty(3, dtype=torch.float64, device=dev)
        st["lowest"] = torch.empty(3, dtype=torch.int32, device=dev)
        ck(lib.gsr_simplify_default_origin(p(vertices), p(st["vmark"]), V, h, p(st["lowest"]), p(st["origin"]), s), "origin")

    def keys():
        st["keys"] = torch.empty(V, dtype=torch.int64, device=dev)
        ck(lib.gsr_simplify_cell_keys(p(vertices), p(st["vmark"]), V, p(st["origin"]), h, p(st["keys"]), p(status), s), "keys")

    def sort_keys():
        st["sorted"], st["order"] = torch.sort(st["keys"], stable=True)

    def heads():
        st["head"] = torch.empty(V, dtype=torch.uint8, device=dev)
        ck(lib.gsr_simplify_run_heads(p(st["sorted"]), V, p(st["head"]), s), "heads")
        st["ends"] = torch.cumsum(st["head"], dim=0, dtype=torch.int64)

    def read_k():
        st["K"] = int(torch.stack((st["ends"][-1], status[0].to(torch.int64))).tolist()[0])

    def reduce():
        K = st["K"]
        st["start"] = torch.empty(K + 1, dtype=torch.int32, device=dev)
        st["means"], st["mcol"] = torch.empty((K, 3), device=dev), torch.empty((K, 3), device=dev)
        st["cov"] = torch.empty(V, dtype=torch.int32, device=dev)
        ck(lib.gsr_simplify_reduce(p(vertices), p(colors), p(st["sorted"]), p(st["order"]), p(st["ends"]), V, K, p(st["start"]),
                                   p(st["means"]), p(st["mcol"]), p(st["cov"]), p(status), s), "reduce")

    def face_keys():
        st["tri"] = torch.empty((F, 3), dtype=torch.int32, device=dev)
        st["keep"] = torch.empty(F, dtype=torch.uint8, device=dev)
        st["kf"], st["kt"] = torch.empty(F, dtype=torch.int64, device=dev), torch.empty(F, dtype=torch.int32, device=dev)
        ck(lib.gsr_simplify_face_keys(p(faces), p(st["cov"]), F, V, st["K"], p(st["tri"]), p(st["keep"]), p(st["kf"]),
                                      p(st["kt"]), p(status), s), "face_keys")

    def sort_third():
        st["by_third"] = torch.sort(st["kt"], stable=True).indices

    def sort_first():
        st["fs"], by_first = torch.sort(st["kf"][st["by_third"]], stable=True)
        st["perm"] = st["by_third"][by_first]

    def unique():
        ck(lib.gsr_simplify_face_unique(p(st["fs"]), p(st["perm"]), p(st["kt"]), F, p(st["keep"]), p(status), s), "unique")

    def mark_clusters():
        st["cmark"] = torch.zeros(st["K"], dtype=torch.uint8, device=dev)
        ck(lib.gsr_mesh_mark_vertices(p(st["tri"]), p(st["keep"]), F, st["K"], p(st["cmark"]), p(status), s), "mark clusters")

    def scans():
        st["ve"] = torch.cumsum(st["cmark"], dim=0, dtype=torch.int64)
        st["fe"] = torch.cumsum(st["keep"], dim=0, dtype=torch.int64)
        st["Vk"], st["Fk"], _ = (int(v) for v in torch.stack((st["ve"][-1], st["fe"][-1], status[0].to(torch.int64))).tolist())

    def compact():
        K, Vk, Fk = st["K"], st["Vk"], st["Fk"]
        ov, oc = torch.empty((Vk, 3), device=dev), torch.empty((Vk, 3), device=dev)
        of = torch.empty((Fk, 3), dtype=torch.int32, device=dev)
        vo, fo = st["ve"] - st["cmark"], st["fe"] - st["keep"]
        ck(lib.gsr_mesh_compact(p(st["means"]), p(st["mcol"]), p(st["tri"]), p(st["keep"]), p(st["cmark"]), p(vo), p(fo), K, F,
                                Vk, Fk, p(ov), p(oc), p(of), p(status), s), "compact")

    timer.run([("mark_vertices (every face)", mark), ("default_origin", origin), ("cell_keys", keys),
               ("torch.sort(cell keys, stable)", sort_keys), ("run_heads + torch.cumsum", heads), ("read-back of K", read_k),
               ("reduce (starts + means)", reduce), ("face_keys", face_keys), ("torch.sort(third, stable)", sort_third),
               ("gather + torch.sort(first two, stable) + gather", sort_first), ("face_unique", unique),
               ("mark_vertices (clusters)", mark_clusters), ("two cumsums + read-back", scans), ("compact", compact)])
    return st


def torch_simplify(vertices, faces, colors, h):
    """The rule of simplify_mesh in torch ops (default origin); every vertex of the bench mesh is referenced and finite."""
    V = vertices.shape[0]
    f = faces.long()
    origin = vertices.amin(dim=0).double() - h / 2
    cell = torch.floor((vertices.double() - origin) / h).long()
    key = (cell[:, 0] << 42) | (cell[:, 1] << 21) | cell[:, 2]
    uniq, inverse = torch.unique(key, return_inverse=True)
    K = uniq.shape[0]
    count = torch.zeros(K, dtype=torch.float64, device=vertices.device).index_add_(0, inverse, torch.ones(V, dtype=torch.float64,
                                                                                                           device=vertices.device))
    mean = lambda rows: (torch.zeros((K, 3), dtype=torch.float64, device=rows.device).index_add_(0, inverse, rows.double())  # noqa: E731
                         / count[:, None]).float()
    means, mean_colors = mean(vertices), mean(colors)
    tri = inverse[f]
    alive = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    tri = tri[alive]
    shift = tri.argmin(dim=1, keepdim=True)
    rotated = torch.gather(tri, 1, (shift + torch.arange(3, device=tri.device)) % 3)
    _, which = torch.unique(rotated, dim=0, return_inverse=True)                       # a sort-unique over the triples
    first = torch.full((int(which.max()) + 1,), tri.shape[0], dtype=torch.int64, device=tri.device)
    first.scatter_reduce_(0, which, torch.arange(tri.shape[0], device=tri.device), reduce="amin")
    tri = tri[torch.sort(first).values]
    used = torch.zeros(K, dtype=torch.bool, device=tri.device)
    used[tri.reshape(-1)] = True
    renumber = torch.cumsum(used, dim=0) - 1
    return means[used], renumber[tri].to(torch.int32), mean_colors[used]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0], help="cell sizes in TSDF voxels")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_simplify needs a GPU: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    cfg = CONFIGS[args.config]
    model, _, bg, _ = make_scene(cfg, seed=0, device=dev)
    cams = [orbit_camera(v, 8, cfg.width, cfg.height, cfg.fx, cfg.fy, device=dev) for v in range(8)]
    voxel = 6.0 / (args.resolution - 1)
    vol = TSDFVolume((-3.0, -3.0, 3.0), voxel, (args.resolution,) * 3, 4 * voxel, device=dev)
    fuse_views(cams, model, PipelineParams(), bg, vol, renderer=render)
    vertices, faces, colors = vol.extract_mesh()
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    res = {"config": args.config, "resolution": args.resolution, "vertices": V, "faces": F, "iters": args.iters}
    print(f"mesh: {V} vertices, {F} faces, TSDF voxel {voxel:.5g}")
    for cell in args.cells:
        h = cell * voxel
        out = res[f"cell_{cell:g}_voxels"] = {"voxel_size": h}
        got = simplify_mesh(vertices, faces, colors, voxel_size=h, return_map=True)
        ref = torch_simplify(vertices, faces, colors, h)
        assert torch.equal(got[1], ref[1]), "the torch formulation gives other faces"
        spacing = 2.0 ** -23 * vertices.abs().max()
        assert float((got[0] - ref[0]).abs().max()) <= spacing and float((got[2] - ref[2]).abs().max()) <= 2.0 ** -23
        out["vertices_out"], out["faces_out"] = int(got[0].shape[0]), int(got[1].shape[0])
        runs = torch.bincount(got[3][got[3] >= 0].long()).double()                     # members of the kept clusters
        out["run_mean"], out["run_p99"], out["run_max"] = (round(float(runs.mean()), 2), float(torch.quantile(runs, 0.99)),
                                                           int(runs.max()))
        out["simplify_mesh_ms"] = call_ms(lambda: simplify_mesh(vertices, faces, colors, voxel_size=h), args.iters, args.warmup)
        out["torch_ops_ms"] = call_ms(lambda: torch_simplify(vertices, faces, colors, h), args.iters, args.warmup)
        timer = Stages()
        for _ in range(args.warmup + args.iters):
            simplify_stages(vertices, faces, colors, h, timer)
        out["stage_ms"] = timer.medians(args.warmup)
        total = sum(out["stage_ms"].values())
        sorts = sum(ms for name, ms in out["stage_ms"].items() if "torch.sort" in name)
        out["sort_share_of_stages"] = round(sorts / total, 4)
        print(f"[{cell:g} voxels] {out['vertices_out']} of {V} vertices, {out['faces_out']} of {F} faces; members per cluster: "
              f"mean {out['run_mean']}, p99 {out['run_p99']:g}, longest {out['run_max']}; simplify_mesh "
              f"{out['simplify_mesh_ms'][0]:.3f} ms, torch ops {out['torch_ops_ms'][0]:.3f} ms "
              f"({out['torch_ops_ms'][0] / out['simplify_mesh_ms'][0]:.1f} x); the sorts are {100 * sorts / total:.1f} % of the stages")
        for name, ms in out["stage_ms"].items():
            print(f"    {name:50s} {ms:8.4f} ms  {100 * ms / total:5.1f} %")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
