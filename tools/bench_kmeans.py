"""Device time of the k-means layer (csrc/kmeans.hip; compress.py) at ``--n`` points against ``--k`` codes,
for every ``--d`` (default 48 = f_rest padded, 4 = rotation, 3 = f_dc / scaling):

  * one assign (code norms + the assignment kernel) by HIP events on the stream, the matrix-core kernel and, for D <= 4,
    the vector-ALU kernel too;
  * the same step in torch ops on the same card in the same session: chunked ``x @ c.T``, add the norms, ``argmin`` -- what
    the host layer would have used without the kernel.  Its indices are compared with the kernel's and the number that differ
    is reported: the two forms round differently, so they may differ where two codes are within rounding of each other;
  * one full iteration (assign, the stable sort, run heads, update) by host wall clock around a device synchronise;
  * the achieved FLOP/s of the assign, counted as 2 N K D' with D' the dims the kernel multiplies (D rounded up to its
    instantiation: 4, 16, 32, 48, 64), and as 2 N K D useful, set against the 122 TF of an untuned float32 MFMA GEMM and the
    52 TF of a float32 VALU GEMM on this GPU (cdna_hip_programming.md §3).

    PYTHONPATH=. python tools/bench_kmeans.py [--n 6000000] [--k 4096] [--d 48 4 3] [--iters 5] [--warmup 2]
"""
import argparse
import json
import statistics
import time

import torch

from mvs_gaussian_splatting_amd import _lib, compress

MFMA_GEMM_TF, VALU_GEMM_TF = 122.0, 52.0


def padded_dims(d):
    return next(p for p in (4, 16, 32, 48, 64) if d <= p)


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
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def torch_assign(x, codebook, chunk):
    """score = |c|^2 - 2 x c^T in chunks of rows (an [N,K] float32 matrix of 6 M x 4096 would be 98 GB), argmin."""
    cn = (codebook * codebook).sum(dim=1)
    ct = codebook.t().contiguous()
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    for lo in range(0, x.shape[0], chunk):
        out[lo:lo + chunk] = torch.argmin(torch.addmm(cn, x[lo:lo + chunk], ct, alpha=-2.0), dim=1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=6_000_000)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--d", type=int, nargs="+", default=[48, 4, 3])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=131072)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans needs a GPU: a CPU run measures nothing")
    lib, dev, n, k = _lib.load(), torch.device("cuda:0"), args.n, args.k
    stream = torch.cuda.current_stream(dev).cuda_stream
    results = []
    for d in args.d:
        g = torch.Generator(device=dev).manual_seed(d)
        centres = torch.randn(k, d, generator=g, device=dev)
        x = centres[torch.randint(0, k, (n,), generator=g, device=dev)] + 0.3 * torch.randn(n, d, generator=g, device=dev)
        codebook = x[torch.randperm(n, generator=g, device=dev)[:k]].contiguous()
        res = {"n": n, "k": k, "d": d, "d_multiplied": padded_dims(d), "iters": args.iters}
        res["assign_ms"] = call_ms(lambda: compress._assign(lib, x, codebook, stream), args.iters, args.warmup)
        if d <= 4:
            res["assign_valu_ms"] = call_ms(lambda: compress._assign(lib, x, codebook, stream, "valu"), args.iters, args.warmup)
        res["assign_torch_ops_ms"] = call_ms(lambda: torch_assign(x, codebook, args.chunk), args.iters, args.warmup)
        index, _ = compress._assign(lib, x, codebook, stream)
        theirs = torch_assign(x, codebook, args.chunk)
        res["indices_differing_from_torch_ops"] = int((index.long() != theirs).sum())
        counters = torch.zeros(2, dtype=torch.int32, device=dev)

        def iteration():
            cb = codebook.clone()
            idx, _ = compress._assign(lib, x, cb, stream)
            compress._update(lib, x, None, idx, cb, counters, stream)
        res["iteration_wall_ms"] = wall_ms(iteration, args.iters, args.warmup)
        s = res["assign_ms"][0] * 1e-3
        res["assign_tflops_multiplied"] = round(2.0 * n * k * padded_dims(d) / s / 1e12, 2)
        res["assign_tflops_useful"] = round(2.0 * n * k * d / s / 1e12, 2)
        res["share_of_mfma_gemm_122tf"] = round(res["assign_tflops_multiplied"] / MFMA_GEMM_TF, 3)
        res["share_of_valu_gemm_52tf"] = round(res["assign_tflops_multiplied"] / VALU_GEMM_TF, 3)
        print(f"D = {d}: assign {res['assign_ms'][0]:.3f} ms (min, max {res['assign_ms'][1:]}), torch ops "
              f"{res['assign_torch_ops_ms'][0]:.3f} ms, " + (f"VALU kernel {res['assign_valu_ms'][0]:.3f} ms, " if d <= 4 else "")
              + f"one iteration {res['iteration_wall_ms'][0]:.3f} ms wall; {res['assign_tflops_multiplied']} TF multiplied "
              f"({res['assign_tflops_useful']} useful): {100 * res['share_of_mfma_gemm_122tf']:.0f} % of the MFMA GEMM figure; "
              f"{res['indices_differing_from_torch_ops']} of {n} indices differ from the torch-ops form")
        results.append(res)
        del x, codebook, index, theirs
    print(json.dumps(results))
    return results


if __name__ == "__main__":
    main()
