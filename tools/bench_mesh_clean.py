"""Device time of the mesh cleaning (csrc/mesh.hip; mesh.py): ``connected_components`` and ``clean_mesh`` in both
connectivities on the mesh extracted from a volume fused from the eight orbit views of a synthetic bench scene (the
input of tools/bench_tsdf.py), against the extraction measured in the same run and against scipy on the host.

    PYTHONPATH=. python tools/bench_mesh_clean.py [--config C4] [--resolution 256] [--iters 20] [--warmup 3]

Whole calls: HIP events around the call (its host read-backs included), median over ``--iters`` calls after ``--warmup``.
Per launch: the same sequence of native calls and torch ops that ``mesh._label`` / ``clean_mesh`` issue, with a HIP event
between the stages, median per stage; the read-back of K is a stage of its own.  Hook statistics: the find steps and
retries (an atomicMin that found its node linked already) the hook kernels count when given a ``stats`` array.  The host
figure is ``scipy.sparse.csgraph.connected_components`` on the same faces, the copy to the host timed separately; its
labels, renumbered by smallest face, must equal the device's.
"""
import argparse
import json
import statistics
import sys
import time

import numpy as np
import torch

from mvs_gaussian_splatting_amd import TSDFVolume, _lib, clean_mesh, connected_components, fuse_views, render
from mvs_gaussian_splatting_amd import mesh as mesh_mod
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
    return statistics.median(out), min(out), max(out)


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

    def medians(self):
        return {k: round(statistics.median(v), 4) for k, v in self.ms.items()}


def label_stages(faces, V, connectivity, keep_largest, min_faces, vertices, colors, timer):
    """The calls of mesh._label and clean_mesh, one stage each."""
    lib, dev = _lib.load(), faces.device
    F = int(faces.shape[0])
    s = torch.cuda.current_stream(dev).cuda_stream
    ck = _lib.check
    st = {}
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mark = torch.empty(F, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()                                                                   # noqa: E731
    if connectivity == "vertex":
        parent = torch.empty(V, dtype=torch.int32, device=dev)
        first = torch.empty(V, dtype=torch.int32, device=dev)
        root = torch.empty(F, dtype=torch.int32, device=dev)
        stages = [
            ("init", lambda: ck(lib.gsr_mesh_cc_init(V, p(parent), p(first), s), "init")),
            ("hook_faces", lambda: ck(lib.gsr_mesh_cc_hook_faces(p(faces), F, V, p(parent), p(status), None, s), "hook")),
            ("flatten", lambda: ck(lib.gsr_mesh_cc_flatten(V, p(parent), s), "flatten")),
            ("mark (face_min + mark)", lambda: ck(lib.gsr_mesh_cc_mark(p(faces), F, V, p(parent), p(first), p(root), p(mark), s),
                                                  "mark")),
        ]
    else:
        parent = torch.empty(F, dtype=torch.int32, device=dev)
        keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        owner = torch.empty(3 * F, dtype=torch.int32, device=dev)
        root = parent

        def sort():
            st["sorted"], st["order"] = torch.sort(keys)
        stages = [
            ("init", lambda: ck(lib.gsr_mesh_cc_init(F, p(parent), None, s), "init")),
            ("edge_keys", lambda: ck(lib.gsr_mesh_edge_keys(p(faces), F, V, p(keys), p(owner), p(status), s), "keys")),
            ("torch.sort", sort),
            ("hook_runs", lambda: ck(lib.gsr_mesh_cc_hook_runs(p(st["sorted"]), p(st["order"]), p(owner), 3 * F, F, p(parent),
                                                               p(status), None, s), "hook")),
            ("flatten", lambda: ck(lib.gsr_mesh_cc_flatten(F, p(parent), s), "flatten")),
            ("mark", lambda: ck(lib.gsr_mesh_cc_mark(None, F, 0, p(parent), None, None, p(mark), s), "mark")),
        ]

    def scan():
        st["ends"] = torch.cumsum(mark, dim=0, dtype=torch.int64)

    def read_k():
        st["K"] = int(torch.stack((st["ends"][-1], status[0].to(torch.int64))).tolist()[0])

    def label():
        st["ids"] = st["ends"] - mark
        st["fc"] = torch.empty(F, dtype=torch.int32, device=dev)
        st["cf"] = torch.zeros(st["K"], dtype=torch.int64, device=dev)
        ck(lib.gsr_mesh_cc_label(p(root), p(st["ids"]), F, st["K"], p(st["fc"]), p(st["cf"]), s), "label")

    def threshold():
        thr = torch.full((), min_faces, dtype=torch.int64, device=dev)
        if keep_largest < st["K"]:
            thr = torch.maximum(thr, torch.topk(st["cf"], keep_largest).values[-1])
        st["keep"] = (st["cf"][st["fc"].to(torch.int64)] >= thr).to(torch.uint8)
        st["vmark"] = torch.zeros(V, dtype=torch.uint8, device=dev)

    def scans():
        st["ve"] = torch.cumsum(st["vmark"], dim=0, dtype=torch.int64)
        st["fe"] = torch.cumsum(st["keep"], dim=0, dtype=torch.int64)
        st["Vk"], st["Fk"] = (int(v) for v in torch.stack((st["ve"][-1], st["fe"][-1])).tolist())

    def compact():
        Vk, Fk = st["Vk"], st["Fk"]
        ov, of = torch.empty((Vk, 3), device=dev), torch.empty((Fk, 3), dtype=torch.int32, device=dev)
        oc = torch.empty((Vk, 3), device=dev)
        vo, fo = st["ve"] - st["vmark"], st["fe"] - st["keep"]
        ck(lib.gsr_mesh_compact(p(vertices), p(colors), p(faces), p(st["keep"]), p(st["vmark"]), p(vo), p(fo), V, F, Vk, Fk,
                                p(ov), p(oc), p(of), p(status), s), "compact")

    stages += [("torch.cumsum(mark)", scan), ("read-back of K", read_k), ("label", label),
               ("clean: threshold + keep flags (torch)", threshold),
               ("clean: mark_vertices", lambda: ck(lib.gsr_mesh_mark_vertices(p(faces), p(st["keep"]), F, V, p(st["vmark"]),
                                                                              p(status), s), "mark_vertices")),
               ("clean: two cumsums + read-back", scans), ("clean: compact", compact)]
    timer.run(stages)
    return st


def scipy_labels(faces_np, V, connectivity):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components as cc
    F = len(faces_np)
    f = faces_np.astype(np.int64)
    if connectivity == "vertex":
        rows, cols = np.concatenate((f[:, 0], f[:, 0])), np.concatenate((f[:, 1], f[:, 2]))
        _, lab = cc(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)), directed=False)
        lab = lab[f[:, 0]]
    else:
        a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
        keys = np.minimum(a, b) * V + np.maximum(a, b)
        order = np.argsort(keys, kind="stable")
        owner = order // 3
        same = keys[order][1:] == keys[order][:-1]
        _, lab = cc(coo_matrix((np.ones(int(same.sum()), np.int8), (owner[:-1][same], owner[1:][same])), shape=(F, F)),
                    directed=False)
    _, first, inverse = np.unique(lab, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[inverse]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--keep_largest", type=int, default=50)
    ap.add_argument("--min_faces", type=int, default=50)
    ap.add_argument("--no_host", action="store_true", help="skip the scipy figure")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_clean needs a GPU: a CPU run measures nothing")
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
    res["extract_mesh_ms"] = [round(x, 4) for x in call_ms(vol.extract_mesh, args.iters, args.warmup)]
    print(f"mesh: {V} vertices, {F} faces; extract_mesh {res['extract_mesh_ms'][0]:.3f} ms (median, min, max: "
          f"{res['extract_mesh_ms']})")
    faces_np = None
    for connectivity in ("edge", "vertex"):
        out = res[connectivity] = {}
        out["connected_components_ms"] = [round(x, 4) for x in call_ms(
            lambda: connected_components(faces, V, connectivity), args.iters, args.warmup)]
        out["clean_mesh_ms"] = [round(x, 4) for x in call_ms(
            lambda: clean_mesh(vertices, faces, colors, keep_largest=args.keep_largest, min_faces=args.min_faces,
                               connectivity=connectivity), args.iters, args.warmup)]
        fc, cf = connected_components(faces, V, connectivity)
        kept = clean_mesh(vertices, faces, colors, keep_largest=args.keep_largest, min_faces=args.min_faces,
                          connectivity=connectivity)
        out["components"], out["largest"] = int(cf.shape[0]), int(cf.max())
        out["kept_vertices"], out["kept_faces"] = int(kept[0].shape[0]), int(kept[1].shape[0])
        stats = torch.zeros(2, dtype=torch.int64, device=dev)
        fc2, _ = mesh_mod._label(faces, V, connectivity, stats=stats)
        assert torch.equal(fc, fc2), "the labelling changed between two runs"
        out["hook_find_steps"], out["hook_retries"] = (int(v) for v in stats.tolist())
        out["hook_pairs"] = 2 * F if connectivity == "vertex" else None
        timer = Stages()
        for _ in range(args.warmup + args.iters):
            label_stages(faces, V, connectivity, args.keep_largest, args.min_faces, vertices, colors, timer)
        timer.ms = {k: v[args.warmup:] for k, v in timer.ms.items()}
        out["stage_ms"] = timer.medians()
        total = sum(out["stage_ms"].values())
        if "torch.sort" in out["stage_ms"]:
            out["sort_share_of_clean_mesh_stages"] = round(out["stage_ms"]["torch.sort"] / total, 4)
        print(f"[{connectivity}] connected_components {out['connected_components_ms'][0]:.3f} ms, clean_mesh "
              f"{out['clean_mesh_ms'][0]:.3f} ms ({out['clean_mesh_ms'][0] / res['extract_mesh_ms'][0]:.1f} x the extraction); "
              f"{out['components']} components, largest {out['largest']} faces; kept {out['kept_faces']} faces; hooks: "
              f"{out['hook_find_steps']} find steps, {out['hook_retries']} retries")
        for name, ms in out["stage_ms"].items():
            print(f"    {name:42s} {ms:8.4f} ms  {100 * ms / total:5.1f} %")
        if not args.no_host:
            t0 = time.perf_counter()
            faces_np = faces.cpu().numpy()
            t1 = time.perf_counter()
            lab = scipy_labels(faces_np, V, connectivity)
            t2 = time.perf_counter()
            assert np.array_equal(lab, fc.cpu().numpy().astype(np.int64)), "scipy's components differ from the device's"
            out["host_copy_ms"], out["host_scipy_ms"] = round(1e3 * (t1 - t0), 2), round(1e3 * (t2 - t1), 1)
            print(f"    host: copy {out['host_copy_ms']} ms, numpy + scipy {out['host_scipy_ms']} ms; labels equal the device's")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
