"""Device time of the registration layer (csrc/icp.hip; geometry_eval.py) at ``--n`` source points on
``--n`` target points:

  * one ICP iteration, ``icp_step``: transform + nearest-point query + accumulate + the read-back of the 18 values (host
    wall clock around the call, which ends in that read-back), and its parts by HIP events;
  * the accumulate entry alone (both launches) against the same sums in torch ops -- the index gather, float64
    subtraction of the pivots, ``einsum`` for a b^T -- which is what the host layer would have used without the kernel and
    what runs unchanged on the commit before it; the two must agree to the bound of tests/icp_restate.py;
  * ``voxel_down_sample`` at ``--n`` points.

    PYTHONPATH=. python tools/bench_icp.py [--n 1000000] [--iters 20] [--warmup 3]

The accumulate kernel's time is set against its bytes -- 20 per source point streamed (q, dist2, nearest) and 12 gathered
per accepted pair -- at the 6.29 TB/s a float4 copy reaches on this GPU (8.0 TB/s is the data sheet's figure).  Event
timings include the launch boundary between the two kernels; a kernel trace would be needed to separate them.
"""
import argparse
import json
import statistics
import time

import numpy as np
import torch

from mvs_gaussian_splatting_amd import _lib
from mvs_gaussian_splatting_amd.geometry_eval import IcpTarget, icp_step, voxel_down_sample

HBM_COPY_TBS = 6.29


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


def wall_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()                                      # ends in a read-back: the device is idle again
        out.append(1e3 * (time.perf_counter() - t0))
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def torch_sums(q, dist2, nearest, target, thr2, cq, cr):
    """The 18 values in torch ops, on the device."""
    ok = (dist2 <= thr2) & (nearest >= 0)
    j = nearest.clamp(min=0).to(torch.int64)
    w = ok.to(torch.float64)
    a = (q.double() - cq) * w[:, None]
    b = (target[j].double() - cr) * w[:, None]
    return torch.cat([ok.sum().double()[None], a.sum(dim=0), b.sum(dim=0), torch.einsum("ni,nj->ij", a, b).reshape(-1),
                      (a * a).sum()[None], (dist2.double() * w).sum()[None]])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_icp needs a GPU: a CPU run measures nothing")
    lib, dev, n = _lib.load(), torch.device("cuda:0"), args.n
    rng = np.random.default_rng(0)
    tgt_h = rng.random((n, 3), dtype=np.float32)
    c, s = np.cos(np.radians(1.0)), np.sin(np.radians(1.0))
    T = np.eye(4)
    T[:3, :3] = 1.01 * np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    T[:3, 3] = [0.004, -0.003, 0.002]
    src_h = ((rng.random((n, 3), dtype=np.float32).astype(np.float64) - T[:3, 3]) @ np.linalg.inv(T[:3, :3]).T).astype(np.float32)
    src, tgt = torch.from_numpy(src_h).to(dev), torch.from_numpy(tgt_h).to(dev)
    target = IcpTarget(tgt)
    max_dist = 0.008                               # about the mean spacing of 1 M points in the unit cube (0.01)
    piv = (np.full(3, 0.5), np.full(3, 0.5))
    res = {"n": n, "iters": args.iters, "max_dist": max_dist}

    step = icp_step(src, target, T, max_dist, pivots=piv)
    res["accepted"] = step.count
    res["icp_step_wall_ms"] = wall_ms(lambda: icp_step(src, target, T, max_dist, pivots=piv), args.iters, args.warmup)

    stream = torch.cuda.current_stream(dev).cuda_stream
    m = np.ascontiguousarray(T[:3])
    q = torch.empty_like(src)
    transform = lambda: _lib.check(lib.gsr_icp_transform(src.data_ptr(), n, m.ctypes.data, q.data_ptr(), stream), "t")   # noqa: E731
    res["transform_ms"] = call_ms(transform, args.iters, args.warmup)
    dist2, nearest = target.index.query(q)
    res["query_ms"] = call_ms(lambda: target.index.query(q), args.iters, args.warmup)
    wb = int(lib.gsr_icp_workspace_bytes(n))
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    out = torch.empty(18, dtype=torch.int64, device=dev)
    pv = np.concatenate(piv)
    thr2 = float(np.float32(max_dist * max_dist))
    accumulate = lambda: _lib.check(lib.gsr_icp_accumulate(q.data_ptr(), dist2.data_ptr(), nearest.data_ptr(), n,   # noqa: E731
                                                           tgt.data_ptr(), n, thr2, pv.ctypes.data, ws.data_ptr(), wb,
                                                           out.data_ptr(), stream), "a")
    res["accumulate_ms"] = call_ms(accumulate, args.iters, args.warmup)
    cq, cr = (torch.from_numpy(p).to(dev) for p in piv)
    res["accumulate_torch_ops_ms"] = call_ms(lambda: torch_sums(q, dist2, nearest, tgt, thr2, cq, cr), args.iters, args.warmup)
    words = out.cpu().numpy()
    mine = np.concatenate([[float(words[0])], words[1:].view(np.float64)])
    theirs = torch_sums(q, dist2, nearest, tgt, thr2, cq, cr).cpu().numpy()
    assert mine[0] == theirs[0] == step.count
    scale = np.abs(mine[1:]).max()
    assert np.abs(mine[1:] - theirs[1:]).max() <= 1e-9 * max(scale, 1.0), (mine, theirs)
    nbytes = 20 * n + 12 * step.count
    floor_ms = nbytes / (HBM_COPY_TBS * 1e12) * 1e3
    res["accumulate_bytes"] = nbytes
    res["accumulate_floor_ms_at_6.29TBs"] = round(floor_ms, 4)
    res["accumulate_share_of_copy_bandwidth"] = round(floor_ms / res["accumulate_ms"][0], 3)
    res["voxel_down_sample_ms"] = wall_ms(lambda: voxel_down_sample(tgt, 0.02), args.iters, args.warmup)
    res["voxel_cells"] = int(voxel_down_sample(tgt, 0.02).shape[0])

    print(f"icp_step at {n} x {n} ({step.count} pairs accepted): {res['icp_step_wall_ms'][0]:.3f} ms wall (median; min, max "
          f"{res['icp_step_wall_ms'][1:]})")
    print(f"  transform {res['transform_ms'][0]:.4f} ms, query {res['query_ms'][0]:.3f} ms, accumulate "
          f"{res['accumulate_ms'][0]:.4f} ms (torch ops: {res['accumulate_torch_ops_ms'][0]:.3f} ms)")
    print(f"  accumulate: {nbytes / 1e6:.1f} MB -> {floor_ms:.4f} ms at {HBM_COPY_TBS} TB/s: "
          f"{100 * res['accumulate_share_of_copy_bandwidth']:.1f} % of the copy bandwidth (memory-bound; both launches timed)")
    print(f"voxel_down_sample at {n} points, {res['voxel_cells']} cells: {res['voxel_down_sample_ms'][0]:.3f} ms wall")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
