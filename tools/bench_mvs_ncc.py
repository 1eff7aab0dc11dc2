"""Device time of the multi-view photometric (NCC) loss (csrc/mvs_ncc.hip, ``mvs_ncc_loss_kernel``),
dense and at 102400 sampled pixels, value only and value plus both gradients, beside the same loss written in torch ops
(a matrix product per tap, a 49-tap ``grid_sample``, sums over the tap axis, autograd) in the same run, from HIP events.

    PYTHONPATH=.:tools python tools/bench_mvs_ncc.py [--iters 20] [--rounds 3]

One 1920 x 1080 pair: two cameras 5 degrees apart on an orbit about a slanted plane at depth 6 (``synthetic.orbit_camera``
of 72 views) that carries a sinusoidal texture; analytic depth maps, the reference's 0.5 % off so that the gradients are
not near zero, the plane's normal in the reference's view space times a smooth positive field.  Reported: ms per call of
the raw entry point (memsets, kernel, finish); of the wrapper's forward + backward; of the torch yardstick's forward +
backward on the same pixels; how far the two agree; taps per second (lanes that reach the tap loop x 50 taps) and bytes
per second on the compulsory traffic: per lane the depth, three normal components and the grey value in (20 bytes) and,
with gradients, four floats out (16), plus 4 bytes per listed index; the reference and source taps are served by caches
that neighbouring lanes share and are not counted.
"""
import argparse
import json
import sys

import numpy as np
import torch
import torch.nn.functional as F

from mvs_gaussian_splatting_amd import _lib, multi_view_ncc_loss
from mvs_gaussian_splatting_amd.mvs import _focal, _view64
from mvs_gaussian_splatting_amd.synthetic import orbit_camera

from bench_mvs import PLANE_C, PLANE_N, plane_depth, timed

RADIUS, PIX_MAX, NCC_MAX, MIN_COS = 3, 1.0, 0.9, 0.05


def plane_image(cam, depth, dev):
    """The texture of the plane's world points seen through ``cam`` -> grey float32 [H,W]."""
    H, W, fx, fy = _focal(cam)
    c2w = torch.from_numpy(np.linalg.inv(_view64(cam))).to(dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    d = depth.double()
    X = torch.stack(((xs - (W - 1) / 2) / fx * d, (ys - (H - 1) / 2) / fy * d, d, torch.ones_like(d)), dim=-1) @ c2w
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    tex = 0.5 + 0.2 * torch.sin(9.0 * x + 0.4) + 0.15 * torch.sin(7.0 * y - 1.0) + 0.1 * torch.sin(13.0 * (x + z))
    return tex.to(torch.float32).contiguous()


def torch_loss(depth, normal, gray, cam, sd, sg, sc, pixels):
    """The same loss in torch ops over ``pixels`` (flat indices whose patch lies inside the reference)."""
    dev = depth.device
    H, W, fx, fy = _focal(cam)
    Hs, Ws, fxs, fys = _focal(sc)
    cx, cy, cxs, cys = (W - 1) * 0.5, (H - 1) * 0.5, (Ws - 1) * 0.5, (Hs - 1) * 0.5
    Mr, Ms = _view64(cam), _view64(sc)
    A = torch.from_numpy((np.linalg.inv(Mr) @ Ms).astype(np.float32)).to(dev)
    B = torch.from_numpy((np.linalg.inv(Ms) @ Mr).astype(np.float32)).to(dev)
    py, px = (pixels // W).to(torch.float32), (pixels % W).to(torch.float32)
    d = depth.reshape(-1)[pixels]
    N = normal.reshape(3, -1)[:, pixels].t()
    r = torch.stack(((px - cx) / fx, (py - cy) / fy, torch.ones_like(px)), dim=-1)
    sample = lambda img, u, v: F.grid_sample(img[None, None], torch.stack((2 * u / (Ws - 1) - 1, 2 * v / (Hs - 1) - 1), dim=-1)[None],      # noqa: E731
                                             mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0]
    with torch.no_grad():                                                  # the round trip: the weight and its gate
        q = torch.cat((r * d[:, None], torch.ones_like(d)[:, None]), dim=-1) @ A
        us, vs = fxs * q[:, 0] / q[:, 2] + cxs, fys * q[:, 1] / q[:, 2] + cys
        inside = (q[:, 2] > 0.2) & (us >= 0) & (us < Ws - 1) & (vs >= 0) & (vs < Hs - 1)
        ds = sample(sd, us[:, None], vs[:, None])[:, 0]
        back = torch.stack(((us - cxs) * ds / fxs, (vs - cys) * ds / fys, ds, torch.ones_like(ds)), dim=-1) @ B
        du, dv = fx * back[:, 0] / back[:, 2] + cx - px, fy * back[:, 1] / back[:, 2] + cy - py
        phi = torch.sqrt(du * du + dv * dv)
        gate = (d > 0) & inside & (ds > 0) & (back[:, 2] > 0.2) & (phi < PIX_MAX)
        w = torch.exp(-phi)
    s = (N * r).sum(-1)
    gate = gate & (s.detach().abs() >= MIN_COS * N.detach().norm(dim=-1) * r.norm(dim=-1))
    m = N / (d * s)[:, None]
    off = torch.arange(-RADIUS, RADIUS + 1, device=dev)
    oy, ox = (o.reshape(-1) for o in torch.meshgrid(off, off, indexing="ij"))
    qx, qy = px[:, None] + ox[None], py[:, None] + oy[None]                # [n, 49]
    rq = torch.stack(((qx - cx) / fx, (qy - cy) / fy, torch.ones_like(qx)), dim=-1)
    k = (rq * m[:, None, :]).sum(-1)
    Y = rq @ A[:3, :3] + k[..., None] * A[3, :3]
    u, v = fxs * Y[..., 0] / Y[..., 2] + cxs, fys * Y[..., 1] / Y[..., 2] + cys
    ok = ((k.detach() > 0) & (Y[..., 2].detach() > 0) & (u.detach() >= 0) & (u.detach() < Ws - 1) & (v.detach() >= 0)
          & (v.detach() < Hs - 1)).all(dim=-1)
    S = sample(sg, u, v)
    Rq = gray.reshape(-1)[(pixels[:, None] + oy[None] * W + ox[None])]
    S0, R0 = S - S.mean(dim=-1, keepdim=True), Rq - Rq.mean(dim=-1, keepdim=True)
    cross, vr, vs_ = (R0 * S0).sum(-1), (R0 * R0).sum(-1), (S0 * S0).sum(-1)
    ncc = (1 - cross * cross / (vr * vs_ + 1e-8)).clamp(0.0, 2.0)
    counted = gate & ok & (ncc.detach() < NCC_MAX)
    n = counted.sum().clamp(min=1)
    return torch.where(counted, w * ncc, torch.zeros_like(ncc)).sum() / n, n


def raw_call(lib, depth, normal, gray, cam, sd, sg, sc, pixels, want):
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
    n_px = 0 if pixels is None else int(pixels.numel())
    record = torch.empty(4, device=dev)
    g_d = torch.empty((H, W), device=dev) if want else None
    g_n = torch.empty((3, H, W), device=dev) if want else None
    ws = torch.empty(lib.gsr_mvs_ncc_loss_workspace_bytes(H, W, n_px), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def call():
        rc = lib.gsr_mvs_ncc_loss_fwd_bwd(depth.data_ptr(), normal.data_ptr(), gray.data_ptr(), H, W, fx, fy, table.data_ptr(),
                                          sg.data_ptr(), None if pixels is None else pixels.data_ptr(), n_px, RADIUS, PIX_MAX,
                                          NCC_MAX, MIN_COS, record.data_ptr(), None if g_d is None else g_d.data_ptr(),
                                          None if g_n is None else g_n.data_ptr(), ws.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f"gsr_mvs_ncc_loss_fwd_bwd failed: {rc}")
    return call, record, g_d, g_n, (table, ws)


def bench(iters, rounds, dev, n_samples=102400):
    W, H, f = 1920, 1080, 1200.0
    cam, sc = (orbit_camera(v, 72, W, H, f, f, device=dev) for v in (0, 1))
    true_depth, sd = plane_depth(cam, dev), plane_depth(sc, dev)
    gray, sg = plane_image(cam, true_depth, dev), plane_image(sc, sd, dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    depth = (true_depth * (1.005 + 0.002 * torch.sin(xs / 90.0) * torch.sin(ys / 70.0 + 0.5))).contiguous()
    n_view = torch.tensor(PLANE_N, dtype=torch.float64) @ torch.from_numpy(_view64(cam))[:3, :3]      # world normal -> view space
    n_view = -n_view / n_view.norm()                                       # camera-facing
    normal = (n_view.to(torch.float32).to(dev)[:, None, None] * (0.6 + 0.3 * torch.sin(xs / 50.0) * torch.cos(ys / 40.0))[None]).contiguous()
    assert PLANE_C > 0
    lib = _lib.load()
    sampled = torch.randperm(H * W, device=dev, generator=torch.Generator(device=dev).manual_seed(0))[:n_samples].to(torch.int32)
    out = {"shape": [H, W], "patch_radius": RADIUS, "n_samples": n_samples}
    units = {}
    for mode, pixels in (("dense", None), (f"{n_samples} samples", sampled)):
        lanes = H * W if pixels is None else n_samples
        for name, want in (("value + gradients", True), ("value only", False)):
            call, record, g_d, g_n, keep = raw_call(lib, depth, normal, gray, cam, sd, sg, sc, pixels, want)
            timed(call, 3)
            ms = [timed(call, iters) for _ in range(rounds)]
            n = int(record.view(torch.int32)[1])
            interior = (H - 2 * RADIUS) * (W - 2 * RADIUS) / (H * W)
            taps = lanes * interior * ((2 * RADIUS + 1) ** 2 + 1)
            traffic = lanes * (20 + (16 if want else 0) + (4 if pixels is not None else 0))
            out[f"{mode}, {name}"] = {"ms": [round(m, 4) for m in ms], "n_counted": n, "taps": int(taps),
                                      "Gtaps_per_s": round(taps / min(ms) / 1e6, 2), "compulsory_bytes": traffic,
                                      "GB_per_s": round(traffic / min(ms) / 1e6, 1)}
            print(f"raw, {mode}, {name}: {min(ms):.4f} ms, n {n} of {lanes}, {taps / min(ms) / 1e6:.1f} Gtaps/s, "
                  f"{traffic / min(ms) / 1e6:.0f} GB/s on {traffic / 1e6:.1f} MB")
            if want:
                units[mode] = (float(record[0]), n, g_d.clone(), g_n.clone())
            del keep

    def wrapper():
        d, nm = depth.clone().requires_grad_(True), normal.clone().requires_grad_(True)
        multi_view_ncc_loss(d, nm, gray, cam, sd, sg, sc, pixels=sampled).backward()
        return d.grad, nm.grad
    timed(wrapper, 3)
    out["wrapper_fwd_bwd_ms (samples)"] = [round(timed(wrapper, iters), 4) for _ in range(rounds)]

    # the yardstick needs whole patches: the same pixels without those next to the border (the kernel gates them out)
    def interior_of(p):
        py, px = p // W, p % W
        return p[(px >= RADIUS) & (px < W - RADIUS) & (py >= RADIUS) & (py < H - RADIUS)].long()
    everything = torch.arange(H * W, device=dev)
    for mode, pixels, reps in ((f"{n_samples} samples", interior_of(sampled), max(2, iters // 4)), ("dense", interior_of(everything), 2)):
        def yardstick():
            d, nm = depth.clone().requires_grad_(True), normal.clone().requires_grad_(True)
            loss, n = torch_loss(d, nm, gray, cam, sd, sg, sc, pixels)
            loss.backward()
            return loss.detach(), n, d.grad, nm.grad
        timed(yardstick, 1)
        out[f"torch_fwd_bwd_ms ({mode})"] = [round(timed(yardstick, reps), 3) for _ in range(rounds)]
        loss_t, n_t, gd_t, gn_t = yardstick()
        value, n, g_d, g_n = units[mode]
        rel_l2 = lambda a, b: float((a - b).double().norm() / b.double().norm())      # noqa: E731
        out[f"agreement ({mode})"] = {"value": value, "torch_value": float(loss_t), "n_counted": n, "torch_n_counted": int(n_t),
                                      "grad_depth_rel_l2": rel_l2(g_d / max(n, 1), gd_t),
                                      "grad_normal_rel_l2": rel_l2(g_n / max(n, 1), gn_t)}
        print(f"torch forward + backward, {mode}: {min(out[f'torch_fwd_bwd_ms ({mode})']):.3f} ms; agreement "
              f"{out[f'agreement ({mode})']}")
        del yardstick
        torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvs_ncc needs a GPU: a CPU run measures nothing")
    print(json.dumps(bench(args.iters, args.rounds, torch.device("cuda:0"))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
