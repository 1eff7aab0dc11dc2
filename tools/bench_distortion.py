"""Device time of the fused depth-distortion map (csrc/distortion.hip: forward, backward = compositing backward + the
per-Gaussian geometry kernel) against the moments route that existed before it -- the depth / alpha maps for A, a
2-channel feature map of [m, m^2] for M1 and M2, ``A M2 - M1^2`` in torch, and the three backwards -- on one frame of a
bench scene at 1920x1080, from HIP events around each route; and the two routes' value errors on a thin-slab scene.

    PYTHONPATH=.:tools python tools/bench_distortion.py [C4] [--iters 20] [--rounds 5] [--mapping ndc|linear]

One colour forward of the scene (two-call path), then ``rounds`` rounds that alternate the two routes (so that clock drift
hits both), ``iters`` calls each; prints every round's mean per call in microseconds and one JSON line with the raw
numbers.  The frame's saved state is only read, so every call sees the same lists.  The moments route is timed WITHOUT the
step from dL/d[m, m^2] to dL/dz (a per-Gaussian chain rule and a second geometry pass it would still need): the
comparison favours it.

The value check runs the operator on the `slab` scene of tests/test_gpu_distortion.py (P = 400 at 72x40, every view depth
in 5 +- 0.005, mapping "linear") and prints, relative to the largest value of the float64 restatement
(tests/distortion_restate.py), the error of the fused map and of ``A M2 - M1^2`` formed from the operator's own float32
depth / alpha and feature maps.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

from mvs_gaussian_splatting_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR, FAR = 0.2, 100.0


def mapped(z, mapping):
    return z if mapping == "linear" else FAR / (FAR - NEAR) * (1.0 - NEAR / z)


def slab_errors(dev):
    """-> {route: max error / max of the float64 map} on the thin-slab scene, on the pixels the oracle is robust on."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import make_settings, small_scene
    from distortion_restate import distortion_ref, slab_model
    from grad_util import MARGIN, oracle_operator_inputs
    from mvs_gaussian_splatting_amd import GaussianRasterizer
    from mvs_gaussian_splatting_amd.rasterizer import GaussianRasterizationSettings
    model, cam, bg, _ = small_scene(P=400, sh_degree=3, width=72, height=40, focal=40.0, scale=0.25, seed=2)
    slab_model(model)
    with torch.no_grad():
        _, xyz, m2, op, kw = oracle_operator_inputs(model, torch.float64)
        truth, _, _, aux = distortion_ref(xyz, m2, op, make_settings(cam, bg, 3), "linear", **kw)
        robust = aux["margin"] > MARGIN
        cam.to(dev)
        st = make_settings(cam, bg.to(dev), 3, cls=GaussianRasterizationSettings)
        z = model._xyz[:, 2:3].to(dev)          # the identity camera: the view depth is the z coordinate
        _, _, maps, feat, dist = GaussianRasterizer(st, aux_maps=True, distortion=dict(mapping="linear"))(
            means3D=model._xyz.to(dev), means2D=None, opacities=model.get_opacity.to(dev), shs=model.get_features.to(dev),
            scales=model.get_scaling.to(dev), rotations=model.get_rotation.to(dev), features=torch.cat((z, z * z), dim=1))
        moments = maps[2] * feat[1] - feat[0] * feat[0]
    scale = float(truth[0][robust].max())
    err = lambda t: float((t.double().cpu() - truth[0])[robust].abs().max()) / scale  # noqa: E731
    return {"fused": err(dist[0]), "moments": err(moments)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mapping", choices=("ndc", "linear"), default="ndc")
    args = ap.parse_args(argv)
    from scene_gpu import GpuScene
    sc = GpuScene(args.config, fused=True)
    lib, dev, P, W, H = sc.lib, sc.dev, sc.P, sc.W, sc.H
    sc.forward()
    frame = _lib.GsrAuxFrame()
    frame.P, frame.width, frame.height, frame.binning_mode = P, W, H, int(sc.params.binning_mode)
    frame.num_rendered, frame.num_visible = sc.R, sc.V
    frame.geom_ws, frame.bin_ws, frame.img_ws, frame.radii = (sc.geom.data_ptr(), sc.binning.data_ptr(), sc.img.data_ptr(),
                                                              sc.radii.data_ptr())
    new = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    g = [new(P, 3), new(P, 3), new(P, 1), new(P, 3), new(P, 4)]
    grads = _lib.GsrAuxGrads(*[t.data_ptr() for t in g], None)
    nbytes = lib.gsr_distortion_backward_bytes(P)
    acc = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mapping = {"linear": 0, "ndc": 1}[args.mapping]
    fref = C.byref(frame)

    dist, state = new(1, H, W), new(2, H, W)
    g_dist = torch.full((1, H, W), 1.0 / (H * W), device=dev)

    def fused():
        _lib.check(lib.gsr_distortion_forward(fref, mapping, NEAR, FAR, dist.data_ptr(), state.data_ptr(), sc.stream), "fwd")
        _lib.check(lib.gsr_distortion_backward(C.byref(sc.params), fref, mapping, NEAR, FAR, state.data_ptr(),
                                               g_dist.data_ptr(), acc.data_ptr(), nbytes, C.byref(grads), sc.stream), "bwd")

    view = sc.cam.world_view_transform.to(dev)
    z = (sc.model._xyz.to(dev) @ view[:3, 2:3] + view[3, 2]).clamp_min(NEAR)
    m = mapped(z, args.mapping)
    F = torch.cat((m, m * m), dim=1).contiguous()
    maps, feat, dF = new(3, H, W), new(2, H, W), new(P, 2)
    g_maps, g_feat = torch.zeros(3, H, W, device=dev), new(2, H, W)

    def moments():
        _lib.check(lib.gsr_aux_maps_forward(fref, maps.data_ptr(), sc.stream), "aux fwd")
        _lib.check(lib.gsr_feature_maps_forward(fref, F.data_ptr(), 2, feat.data_ptr(), sc.stream), "feature fwd")
        value = maps[2] * feat[1] - feat[0] * feat[0]
        # d (A M2 - M1^2): dA = M2, dM1 = -2 M1, dM2 = A, each times the incoming gradient
        torch.mul(feat[1], g_dist[0], out=g_maps[2])
        torch.mul(feat[0], g_dist[0], out=g_feat[0]).mul_(-2.0)
        torch.mul(maps[2], g_dist[0], out=g_feat[1])
        _lib.check(lib.gsr_aux_maps_backward(C.byref(sc.params), fref, g_maps.data_ptr(), acc.data_ptr(), nbytes,
                                             C.byref(grads), sc.stream), "aux bwd")
        _lib.check(lib.gsr_feature_maps_backward(C.byref(sc.params), fref, F.data_ptr(), 2, g_feat.data_ptr(), dF.data_ptr(),
                                                 acc.data_ptr(), nbytes, C.byref(grads), sc.stream), "feature bwd")
        return value

    calls = {"fused fwd+bwd": fused, "moments fwd+bwd": moments}

    def run(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize(dev)
        return 1000.0 * a.elapsed_time(b) / n

    for fn in calls.values():
        run(fn, 3)
    rows = {k: [] for k in calls}
    for r in range(args.rounds):
        for k, fn in calls.items():
            us = run(fn, args.iters)
            rows[k].append(round(us, 1))
            print(f"round {r} {k}: {us:.1f} us per call")
    covered = maps[2] > 0
    agree = float((moments() - dist[0])[covered].abs().max() / dist.max())
    errors = slab_errors(dev)
    print(f"thin slab (z in 5 +- 0.005, linear): fused {errors['fused']:.2e}, float32 moments {errors['moments']:.2e} "
          f"of the float64 map's maximum")
    print(json.dumps({"config": args.config, "P": P, "W": W, "H": H, "num_rendered": sc.R, "iters": args.iters,
                      "mapping": args.mapping, "us_per_call": rows, "bench_scene_routes_differ_by": agree,
                      "slab_value_error": errors, "finite": bool(math.isfinite(float(dist.sum())))}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
