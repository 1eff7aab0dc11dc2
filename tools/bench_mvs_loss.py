"""Device time of the multi-view geometric consistency loss (csrc/mvs_loss.hip, ``mvs_geo_loss_kernel``; DESIGN.md
§7.22), value plus both gradients, beside the same loss written in torch ops (matrix products, ``grid_sample``, autograd)
in the same run, from HIP events.

    PYTHONPATH=.:tools python tools/bench_mvs_loss.py [--iters 20] [--rounds 3]

One 1920 x 1080 pair: two cameras 5 degrees apart on an orbit about a slanted plane at depth 6 (``synthetic.orbit_camera``
of 72 views), analytic depth maps, the source's scaled by a smooth field so that phi spreads over (0, pix_max).  Reported:
ms per call of the raw entry point (memset, kernel, finish) with both gradients, with ``grad_ref`` only and forward only;
of the wrapper's forward + backward; of the torch yardstick's forward + backward; how far the two agree (value, and the
gradients: max-norm where both took the same decisions and phi >= 0.01, and relative L2 over all); and the bytes / s on the compulsory traffic -- the reference depth in and
``grad_ref`` out (4 + 4 bytes a pixel), four gathered floats and four atomic adds per valid pixel (16 + 16).
"""
import argparse
import json
import sys

import numpy as np
import torch
import torch.nn.functional as F

from mvs_gaussian_splatting_amd import _lib, multi_view_geo_loss
from mvs_gaussian_splatting_amd.mvs import _focal, _view64
from mvs_gaussian_splatting_amd.synthetic import orbit_camera

from bench_mvs import plane_depth, timed


def torch_loss(depth, cam, sd, sc, pix_max):
    """The same loss in torch ops; the bilinear read (and its two gradients) is ``grid_sample``'s."""
    dev = depth.device
    H, W, fx, fy = _focal(cam)
    Hs, Ws, fxs, fys = _focal(sc)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    cx, cy = (W - 1) * 0.5, (H - 1) * 0.5
    Mr, Ms = _view64(cam), _view64(sc)
    A = torch.from_numpy((np.linalg.inv(Mr) @ Ms).astype(np.float32)).to(dev)
    B = torch.from_numpy((np.linalg.inv(Ms) @ Mr).astype(np.float32)).to(dev)
    p = torch.stack(((xs - cx) * depth / fx, (ys - cy) * depth / fy, depth, torch.ones_like(depth)), dim=-1)
    q = p @ A
    zs = q[..., 2]
    us, vs = fxs * q[..., 0] / zs + (Ws - 1) * 0.5, fys * q[..., 1] / zs + (Hs - 1) * 0.5
    inside = (zs > 0.2) & (us >= 0) & (us < Ws - 1) & (vs >= 0) & (vs < Hs - 1)
    grid = torch.stack((2 * us / (Ws - 1) - 1, 2 * vs / (Hs - 1) - 1), dim=-1)[None]
    ds = F.grid_sample(sd[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
    with torch.no_grad():
        mask = F.grid_sample((sd.detach() > 0).to(torch.float32)[None, None], grid, mode="bilinear", padding_mode="zeros",
                             align_corners=True)[0, 0]
    back = torch.stack(((us - (Ws - 1) * 0.5) * ds / fxs, (vs - (Hs - 1) * 0.5) * ds / fys, ds, torch.ones_like(ds)), dim=-1) @ B
    zb = back[..., 2]
    du, dv = fx * back[..., 0] / zb + cx - xs, fy * back[..., 1] / zb + cy - ys
    e2 = du * du + dv * dv
    valid = (depth.detach() > 0) & inside & (mask > 0.9999) & (zb.detach() > 0.2) & (e2.detach() < pix_max ** 2) & (e2.detach() > 0)
    phi = torch.sqrt(torch.where(valid, e2, torch.ones_like(e2)))
    w = torch.exp(-phi).detach()
    n = valid.sum().clamp(min=1)
    return torch.where(valid, w * phi, torch.zeros_like(phi)).sum() / n, n, phi.detach()


def raw_call(lib, depth, cam, sd, sc, pix_max, want_ref, want_src):
    dev = depth.device
    H, W, fx, fy = _focal(cam)
    Hs, Ws, fxs, fys = _focal(sc)
    row = _lib.GsrMvsSource()
    Mr, Ms = _view64(cam), _view64(sc)
    row.depth, row.width, row.height, row.fx, row.fy = sd.data_ptr(), Ws, Hs, fxs, fys
    A, B = (np.linalg.inv(Mr) @ Ms).astype(np.float32).reshape(-1), (np.linalg.inv(Ms) @ Mr).astype(np.float32).reshape(-1)
    for i in range(16):
        row.ref_to_src[i], row.src_to_ref[i] = float(A[i]), float(B[i])
    table = torch.frombuffer(bytearray(bytes(row)), dtype=torch.uint8).to(dev)
    record = torch.empty(4, device=dev)
    g_ref = torch.empty((H, W), device=dev) if want_ref else None
    g_src = torch.empty((Hs, Ws), device=dev) if want_src else None
    ws = torch.empty(lib.gsr_mvs_geo_loss_workspace_bytes(H, W), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call():
        rc = lib.gsr_mvs_geo_loss_fwd_bwd(depth.data_ptr(), H, W, fx, fy, table.data_ptr(), pix_max, 0.0, record.data_ptr(),
                                          None if g_ref is None else g_ref.data_ptr(),
                                          None if g_src is None else g_src.data_ptr(), Hs, Ws, ws.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"gsr_mvs_geo_loss_fwd_bwd failed: {rc}")
    return call, record, g_ref, g_src, (table, ws)


def bench(iters, rounds, dev):
    W, H, f = 1920, 1080, 1200.0
    cam, sc = (orbit_camera(v, 72, W, H, f, f, device=dev) for v in (0, 1))
    depth, sd = plane_depth(cam, dev), plane_depth(sc, dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    sd = (sd * (1.0 + 0.004 * torch.sin(xs / 90.0) * torch.sin(ys / 70.0 + 0.5))).contiguous()
    lib = _lib.load()
    out = {"shape": [H, W]}
    for name, want in (("value + both gradients", (True, True)), ("value + grad_ref", (True, False)), ("value only", (False, False))):
        call, record, g_ref, g_src, keep = raw_call(lib, depth, cam, sd, sc, 1.0, *want)
        timed(call, 3)
        ms = [timed(call, iters) for _ in range(rounds)]
        n = int(record.view(torch.int32)[1])
        traffic = H * W * (4 + (4 if want[0] else 0)) + n * (16 + (16 if want[1] else 0))
        out[name] = {"ms": [round(m, 4) for m in ms], "n_valid": n, "compulsory_bytes": traffic,
                     "GB_per_s": round(traffic / min(ms) / 1e6, 1)}
        print(f"raw, {name}: {min(ms):.4f} ms, n_valid {n} of {H * W}, {traffic / min(ms) / 1e6:.0f} GB/s on {traffic / 1e6:.1f} MB")
        if want == (True, True):
            value, unit_ref, unit_src = float(record[0]), g_ref.clone(), g_src.clone()
        del keep

    def wrapper():
        d, s = depth.clone().requires_grad_(True), sd.clone().requires_grad_(True)
        multi_view_geo_loss(d, cam, s, sc).backward()
        return d.grad, s.grad

    def yardstick():
        d, s = depth.clone().requires_grad_(True), sd.clone().requires_grad_(True)
        loss, n, phi = torch_loss(d, cam, s, sc, 1.0)
        loss.backward()
        return loss.detach(), n, d.grad, s.grad, phi
    timed(wrapper, 3)
    out["wrapper_fwd_bwd_ms"] = [round(timed(wrapper, iters), 4) for _ in range(rounds)]
    timed(yardstick, 2)
    out["torch_fwd_bwd_ms"] = [round(timed(yardstick, max(2, iters // 4)), 4) for _ in range(rounds)]
    loss_t, n_t, gr_t, gs_t, phi_t = yardstick()
    scale = 1.0 / max(out["value + both gradients"]["n_valid"], 1)
    # the two float32 evaluation orders take another decision at a few pixels (phi next to pix_max, a footprint next to
    # the border), and where phi is next to 0 the direction (du, dv) / phi is rounding noise in both: those pixels carry a
    # whole gradient of difference, so grad_ref is compared where both decided alike and phi >= 0.01
    mine = unit_ref * scale
    same = ((unit_ref != 0) == (gr_t != 0)) & (phi_t >= 0.01)
    rel_l2 = lambda a, b: float((a - b).double().norm() / b.double().norm())      # noqa: E731
    out["agreement"] = {"value": value, "torch_value": float(loss_t), "torch_n_valid": int(n_t),
                        "pixels_set_aside": int((~same).sum()),
                        "grad_ref_max_rel_elsewhere": float((mine - gr_t)[same].abs().max() / gr_t.abs().max()),
                        "grad_ref_rel_l2": rel_l2(mine, gr_t), "grad_src_rel_l2": rel_l2(unit_src * scale, gs_t)}
    print(f"wrapper forward + backward {min(out['wrapper_fwd_bwd_ms']):.4f} ms; torch forward + backward "
          f"{min(out['torch_fwd_bwd_ms']):.3f} ms; agreement {out['agreement']}")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvs_loss needs a GPU: a CPU run measures nothing")
    print(json.dumps(bench(args.iters, args.rounds, torch.device("cuda:0"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
