"""Device time of the MCMC strategy's steps (``mcmc.py``, ``csrc/mcmc.hip``) at P = 6 M and P = 1 M Gaussians, in one
process:

  * ``inject_noise`` (one launch) against the torch chain it replaces (the covariance built per Gaussian, ``bmm``, gate);
  * ``mcmc_regularizer`` forward + backward against its torch composition;
  * one ``relocate_gs`` + ``add_new_gs`` round on a model with Adam state and 5 % dead rows.

    PYTHONPATH=. python tools/bench_mcmc.py [--points 6000000 1000000] [--iters 50] [--warmup 10]

Every number is the median of ``--iters`` timed iterations after ``--warmup`` untimed ones, each iteration between its own
pair of HIP events.  The noise kernel's rate is given against the 56 bytes it reads per Gaussian (44 B of state, 12 B of
noise) and the 68 it moves in all (12 B written back).  The densification round is restored from a copy before every
iteration, outside the timed span; its span includes the host's one read-back.  Prints one JSON line at the end.
"""
import argparse
import json
import statistics
import sys

import torch
from torch import nn

from mvs_gaussian_splatting_amd import add_new_gs, inject_noise, mcmc_regularizer, optim, relocate_gs
from mvs_gaussian_splatting_amd.densify import GROUP_ATTR
from mvs_gaussian_splatting_amd.synthetic import SyntheticGaussianModel
from mvs_gaussian_splatting_amd.trainer import OptimizationParams


def timed(fn, iters, warmup, before=None):
    """Median milliseconds of fn() over iters runs; before() runs untimed ahead of each."""
    out = []
    for i in range(warmup + iters):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def torch_noise(xyz, scaling_raw, rotation_raw, opacity_raw, noise, step):
    """The original strategy's noise step in torch ops."""
    s = torch.exp(scaling_raw)
    q = torch.nn.functional.normalize(rotation_raw)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    L = R * s[:, None, :]
    cov = L @ L.transpose(1, 2)
    gate = torch.sigmoid(100.0 * ((1.0 - torch.sigmoid(opacity_raw)) - 0.995))
    v = noise * gate * step
    xyz.add_(torch.bmm(cov, v.unsqueeze(-1)).squeeze(-1))


def bench_points(P, iters, warmup, dev):
    model = SyntheticGaussianModel(P, 3, seed=0)
    model._opacity = (model._opacity - 1.0).contiguous()
    model.to(dev)
    model.spatial_lr_scale = 1.0
    for a in GROUP_ATTR.values():
        setattr(model, a, nn.Parameter(getattr(model, a).contiguous()))
    opt = OptimizationParams()
    optim.training_setup(model, opt)
    noise = torch.randn(P, 3, device=dev)
    out = {"points": P}

    # noise
    for group in model.optimizer.param_groups:               # training_setup leaves lr = 0 until the first iteration
        if group["name"] == "xyz":
            group["lr"] = opt.position_lr_init
    step = opt.noise_lr * opt.position_lr_init
    with torch.no_grad():
        out["noise_hip_ms"] = timed(lambda: inject_noise(model, opt.noise_lr, noise=noise), iters, warmup)
        xyz = model._xyz.detach().clone()
        out["noise_torch_ms"] = timed(lambda: torch_noise(xyz, model._scaling.detach(), model._rotation.detach(),
                                                          model._opacity.detach(), noise, step), iters, warmup)
    out["noise_read_tbps"] = 56.0 * P / (out["noise_hip_ms"] * 1e-3) / 1e12
    out["noise_moved_tbps"] = 68.0 * P / (out["noise_hip_ms"] * 1e-3) / 1e12

    # priors, forward + backward
    def reg_hip():
        model._opacity.grad = model._scaling.grad = None
        mcmc_regularizer(model._opacity, model._scaling, opt.opacity_reg, opt.scale_reg).backward()

    def reg_torch():
        model._opacity.grad = model._scaling.grad = None
        (opt.opacity_reg * torch.sigmoid(model._opacity).mean() + opt.scale_reg * torch.exp(model._scaling).mean()).backward()

    out["reg_hip_ms"] = timed(reg_hip, iters, warmup)
    out["reg_torch_ms"] = timed(reg_torch, iters, warmup)
    model._opacity.grad = model._scaling.grad = None

    # one relocation + growth round with 5 % dead rows, on a model with Adam moments
    base = {a: getattr(model, a).detach().clone() for a in GROUP_ATTR.values()}
    g = torch.Generator(device=dev).manual_seed(1)
    dead = torch.randperm(P, device=dev, generator=g)[:P // 20]
    base["_opacity"][dead] = -7.0
    stats = {a: getattr(model, a).clone() for a in ("xyz_gradient_accum", "denom", "max_radii2D")}
    draws = torch.randint(0, 2 ** 63 - 1, (P // 10,), dtype=torch.int64, device=dev)

    def restore():
        for group in model.optimizer.param_groups:
            old = group["params"][0]
            model.optimizer.state.pop(old, None)
            p = nn.Parameter(base[GROUP_ATTR[group["name"]]].clone())
            group["params"][0] = p
            setattr(model, GROUP_ATTR[group["name"]], p)
            model.optimizer.state[p] = {"step": torch.tensor(5.0), "exp_avg": torch.full_like(p, 1e-3),
                                        "exp_avg_sq": torch.full_like(p, 1e-6)}
        for a, t in stats.items():
            setattr(model, a, t.clone())

    moved = {}

    def round_():
        moved["relocated"] = relocate_gs(model, draws=draws)
        moved["added"] = add_new_gs(model, int(1.05 * P), draws=draws)

    out["round_ms"] = timed(round_, iters, warmup, before=restore)
    out.update(moved)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="*", default=[6_000_000, 1_000_000])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("bench_mcmc needs a ROCm GPU", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    rows = []
    for P in args.points:
        r = bench_points(P, args.iters, args.warmup, dev)
        rows.append(r)
        print(f"P = {P}: inject_noise {r['noise_hip_ms']:.3f} ms (reads {r['noise_read_tbps']:.2f} TB/s of 56 B/Gaussian, "
              f"moves {r['noise_moved_tbps']:.2f} TB/s) vs torch chain {r['noise_torch_ms']:.3f} ms "
              f"({r['noise_torch_ms'] / r['noise_hip_ms']:.1f}x); regularizer fwd+bwd {r['reg_hip_ms']:.3f} ms vs torch "
              f"{r['reg_torch_ms']:.3f} ms ({r['reg_torch_ms'] / r['reg_hip_ms']:.1f}x); relocate {r['relocated']} + add "
              f"{r['added']}: {r['round_ms']:.2f} ms", flush=True)
    print(json.dumps({"iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "rows": rows}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
