"""Recover a perturbed camera pose against a fixed Gaussian cloud with the rasterizer's camera gradients.

    python examples/refine_pose.py [iterations]

A synthetic cloud is rendered from a known camera; a copy of that camera is rotated and shifted a little, wrapped in a
``PoseCamera`` and optimised (Adam on its six pose parameters, fused L1 + D-SSIM loss) until its image matches again.  The
cloud is frozen: the only gradients the frame's backward is asked for are ``dL/dviewmatrix``, ``dL/dprojmatrix`` and
``dL/dcampos``, which autograd carries on to ``rot_delta`` / ``trans_delta``.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mvs_gaussian_splatting_amd import PoseCamera, l1_dssim_loss, render  # noqa: E402
from mvs_gaussian_splatting_amd.synthetic import (PipelineParams, SyntheticCamera, SyntheticGaussianModel,  # noqa: E402
                                                  orbit_camera)


def rotation_about(axis, degrees: float) -> np.ndarray:
    """Rotation matrix of ``degrees`` about ``axis`` (Rodrigues, float64)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = math.radians(degrees)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def pose_errors(R, T, R_true, T_true):
    """(rotation error in degrees, translation error) between two poses in ``Camera``'s (R, T) convention."""
    c = (np.trace(np.asarray(R).T @ np.asarray(R_true)) - 1.0) * 0.5
    return math.degrees(math.acos(max(-1.0, min(1.0, c)))), float(np.linalg.norm(np.asarray(T) - np.asarray(T_true)))


def make_problem(dev, P=3000, W=192, H=128, seed=0, rot_degrees=1.0, shift=(0.02, -0.015, 0.03)):
    """(frozen cloud, true camera, perturbed camera, target image, background)."""
    cloud = SyntheticGaussianModel(P, 3, seed=seed, log_scale_mean=math.log(0.06), extent=(1.6, 1.0, 0.8), centre=(0, 0, 4.0))
    cloud._opacity += 1.0
    cloud.to(dev)
    true_cam = orbit_camera(1, 8, W, H, 220.0, 220.0, centre=(0.0, 0.0, 4.0), device=dev)
    bg = torch.zeros(3, device=dev)
    with torch.no_grad():
        target = render(true_cam, cloud, PipelineParams(), bg)["render"].clone()
    # world-to-camera = [R^T | T]: rotate the camera frame a little and shift it
    dR = rotation_about((0.3, 1.0, 0.2), rot_degrees)
    R = true_cam.R @ dR.T
    T = dR @ true_cam.T + np.asarray(shift, dtype=np.float64)
    start = SyntheticCamera(W, H, 220.0, 220.0, R=R, T=T, device=dev)
    return cloud, true_cam, start, target, bg


def refine(dev, iterations=300, lr=1e-3, log=None, **problem):
    """Runs the refinement; returns {"loss": [...], "rot_err": (start, end) degrees, "trans_err": (start, end),
    "camera": the PoseCamera}."""
    cloud, true_cam, start, target, bg = make_problem(dev, **problem)
    cam = PoseCamera(start)
    optimizer = torch.optim.Adam(cam.parameters(), lr=lr)
    pipe = PipelineParams()
    err0 = pose_errors(*cam.pose(), true_cam.R, true_cam.T)
    losses = []
    for it in range(1, iterations + 1):
        pkg = render(cam, cloud, pipe, bg)
        loss = l1_dssim_loss(pkg["render"], target, 0.2)
        loss.backward()
        optimizer.step()
        optimizer.zero_grad(set_to_none=True)
        losses.append(float(loss.detach()))
        if log and it % 25 == 0:
            r, t = pose_errors(*cam.pose(), true_cam.R, true_cam.T)
            log(f"iteration {it}: loss {losses[-1]:.6f}  rotation error {r:.4f} deg  translation error {t:.5f}")
    err1 = pose_errors(*cam.pose(), true_cam.R, true_cam.T)
    return {"loss": losses, "rot_err": (err0[0], err1[0]), "trans_err": (err0[1], err1[1]), "camera": cam}


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    out = refine(torch.device("cuda:0"), iterations=n, log=print)
    print(f"loss {out['loss'][0]:.6f} -> {out['loss'][-1]:.6f}; rotation error {out['rot_err'][0]:.4f} -> "
          f"{out['rot_err'][1]:.4f} deg; translation error {out['trans_err'][0]:.5f} -> {out['trans_err'][1]:.5f}")
