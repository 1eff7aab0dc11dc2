"""Device time of the contracted TSDF integration (csrc/tsdf.hip, ``tsdf_integrate_kernel<*, true>``)
beside the bounded kernel on the same dims and the same view, from HIP events in one run, and of the uncontraction of a
mesh's vertices.

    PYTHONPATH=. python tools/bench_tsdf_unbounded.py [--dim 512] [--iters 10] [--rounds 3]

Inputs: the 1920 x 1080 view of tools/bench_tsdf.py (camera at the origin looking down +z, a slanted plane at depth 6,
every pixel valid).  The contracted volume is the cube [-1.9, 1.9]^3 of contracted space with ``dim`` samples per side,
centre (0, 0, 6), radius 1, q_max 1.9, truncation 5 world voxels: its unit ball holds the plane's middle, its shell
everything out to 10 units.  The bounded volume is a world-space box of the same dims and voxel size about the same
centre (z from 4.1 to 7.9), truncation 5 voxels: the yardstick.  The share of lanes that leave at the q_max test is
counted from the grid, the updated points from the result.
"""
import argparse
import json
import sys

import torch

from mvs_gaussian_splatting_amd import ContractedTSDFVolume, TSDFVolume
from mvs_gaussian_splatting_amd.synthetic import orbit_camera


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def leaving_share(vol):
    """Share of the grid points with |q|^2 >= q_max^2, in float32 as the kernel forms it."""
    nx, ny, nz = vol.dims
    dev = vol.tsdf.device
    ax = [torch.tensor(vol.origin[a], dtype=torch.float32, device=dev) + torch.tensor(vol.voxel_size, dtype=torch.float32,
          device=dev) * torch.arange(n, dtype=torch.float32, device=dev) for a, n in enumerate((nx, ny, nz))]
    bound = torch.tensor(vol.q_max, dtype=torch.float32, device=dev) ** 2
    left = 0
    for k in range(nz):
        m2 = (ax[0][None, :] ** 2 + ax[1][:, None] ** 2) + ax[2][k] ** 2
        left += int((~(m2 < bound)).sum())
    return left / float(nx * ny * nz)


def bench(dim, iters, rounds, dev):
    W, H, f = 1920, 1080, 1200.0
    cam = orbit_camera(0, 8, W, H, f, f, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    depth = (6.0 + 0.3 * (xs - W / 2) / W + 0.2 * (ys - H / 2) / H).float().contiguous()
    color = torch.rand(3, H, W, device=dev)
    R, centre, radius = 1.9, (0.0, 0.0, 6.0), 1.0
    voxel = 2.0 * R / (dim - 1)
    out = {}
    for with_color in (False, True):
        bounded = TSDFVolume(tuple(c - R for c in centre), voxel, (dim,) * 3, 5 * voxel, with_color=with_color, device=dev)
        contracted = ContractedTSDFVolume((-R,) * 3, voxel, (dim,) * 3, 5 * radius * voxel, centre, radius, q_max=1.9,
                                          with_color=with_color, device=dev)
        row = {}
        for name, vol in (("bounded", bounded), ("contracted", contracted)):
            call = lambda: vol.integrate(depth, cam, color=color if with_color else None)      # noqa: E731,B023
            timed(call, 2)
            ms = [timed(call, iters) for _ in range(rounds)]
            row[name] = {"ms_per_view": [round(m, 4) for m in ms], "updated_points": int((vol.weight > 0).sum())}
        row["points"] = dim ** 3
        row["leave_at_q_max"] = round(leaving_share(contracted), 4)
        row["ratio_contracted_over_bounded"] = round(min(row["contracted"]["ms_per_view"]) / min(row["bounded"]["ms_per_view"]), 3)
        print(f"integrate {dim}^3 colour={with_color}: bounded {min(row['bounded']['ms_per_view']):.3f} ms "
              f"({row['bounded']['updated_points']} updated), contracted {min(row['contracted']['ms_per_view']):.3f} ms "
              f"({row['contracted']['updated_points']} updated, {row['leave_at_q_max']:.3f} of the lanes leave at q_max): "
              f"ratio {row['ratio_contracted_over_bounded']:.3f}")
        out["color" if with_color else "plain"] = row
        del bounded, contracted
    # the uncontraction of a mesh's vertices: 4 M rows inside q_max
    g = torch.Generator(device=dev).manual_seed(0)
    d = torch.randn(4_000_000, 3, device=dev, generator=g)
    q = d / d.norm(dim=1, keepdim=True) * (1.85 * torch.rand(4_000_000, 1, device=dev, generator=g))
    vol = ContractedTSDFVolume((-R,) * 3, 1.0, (2, 2, 2), 1.0, centre, radius, device=dev)
    from mvs_gaussian_splatting_amd import _lib
    import ctypes as C
    con, lib = vol._native_contraction(), _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    work = q.clone()

    def call():
        work.copy_(q)
        _lib.check(lib.gsr_tsdf_uncontract_points(work.data_ptr(), work.shape[0], C.byref(con), stream), "uncontract")
    timed(call, 2)
    both = min(timed(call, iters) for _ in range(rounds))
    copy = min(timed(lambda: work.copy_(q), iters) for _ in range(rounds))
    out["uncontract"] = {"rows": int(q.shape[0]), "ms_with_copy": round(both, 4), "ms_copy_alone": round(copy, 4)}
    print(f"uncontract {q.shape[0]} rows: {both - copy:.4f} ms (with the restoring copy {both:.4f}, the copy alone {copy:.4f})")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_unbounded needs a GPU: a CPU run measures nothing")
    print(json.dumps(bench(args.dim, args.iters, args.rounds, torch.device("cuda:0"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
