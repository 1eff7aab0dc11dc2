"""Generates tests/golden/eval_metrics.npz from the reference's own importable Python (run ONLY in the build
container, where /root/reference exists; the fixture -- plain input/output arrays and scalars -- is committed):
utils/loss_utils.py (l1_loss, ssim) and utils/image_utils.py (psnr), evaluated the way train.py:222-229
(training_report: both images clamped, [3,H,W]) and metrics.py:75-76 ([1,3,H,W]) call them.

Per case ``<name>``: ``<name>_img``, ``<name>_gt`` float32 [3,H,W] with some values outside [0, 1]; on the clamped pair
``<name>_l1``, ``<name>_psnr3`` (the [3,1] per-channel values), ``<name>_psnr_mean`` (their mean: the report's term),
``<name>_psnr1`` (the [1,3,H,W] form), ``<name>_ssim`` and the six raw sums ``<name>_sums`` -- each in float32 (``_f32``)
and on ``.double()`` inputs (``_f64``).  ``seq_*``: five views and the report's running sums in double.  ``same_*``:
a pair with one identical channel (mse = 0 -> inf).
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def pair(g, H, W):
    gt = torch.rand(3, H, W, generator=g)
    img = gt + 0.05 * torch.randn(3, H, W, generator=g) + 0.02
    return img, gt


def main():
    sys.path.insert(0, REF)
    from utils.image_utils import psnr
    from utils.loss_utils import l1_loss, ssim
    g = torch.Generator().manual_seed(20240611)
    out = {}

    def case(name, img, gt):
        out[f"{name}_img"], out[f"{name}_gt"] = img.numpy(), gt.numpy()
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            a, b = img.to(dt).clamp(0.0, 1.0), gt.to(dt).clamp(0.0, 1.0)
            p3 = psnr(a, b)
            out[f"{name}_l1_{tag}"] = l1_loss(a, b).numpy()
            out[f"{name}_psnr3_{tag}"] = p3.numpy()
            out[f"{name}_psnr_mean_{tag}"] = p3.mean().numpy()
            out[f"{name}_psnr1_{tag}"] = psnr(a[None], b[None]).numpy()
            out[f"{name}_ssim_{tag}"] = ssim(a, b).numpy()
            out[f"{name}_ssim4_{tag}"] = ssim(a[None], b[None]).numpy()
            d = a - b
            out[f"{name}_sums_{tag}"] = torch.cat((d.abs().sum(dim=(1, 2)), (d * d).sum(dim=(1, 2)))).numpy()
        outside = float(((img < 0) | (img > 1)).float().mean())
        out[f"{name}_outside"] = np.float64(outside)
        return outside

    for name, (H, W) in (("a", (48, 64)), ("b", (131, 77))):
        img, gt = pair(g, H, W)
        print(name, "outside [0,1]:", case(name, img, gt), "psnr", float(out[f"{name}_psnr_mean_f64"]))

    # training_report's running sums over five views (train.py:219-231), float32 per view then .double(), and the same
    # loop on double inputs
    views = [pair(g, 24, 32) for _ in range(5)]
    out["seq_img"] = torch.stack([v[0] for v in views]).numpy()
    out["seq_gt"] = torch.stack([v[1] for v in views]).numpy()
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        l1_test, psnr_test, steps = 0.0, 0.0, []
        for img, gt in views:
            a, b = torch.clamp(img.to(dt), 0.0, 1.0), torch.clamp(gt.to(dt), 0.0, 1.0)
            l1_test += l1_loss(a, b).mean().double()
            psnr_test += psnr(a, b).mean().double()
            steps.append((float(l1_test), float(psnr_test)))
        out[f"seq_running_{tag}"] = np.array(steps, dtype=np.float64)
        out[f"seq_mean_{tag}"] = np.array([float(l1_test / len(views)), float(psnr_test / len(views))], dtype=np.float64)

    img, gt = pair(g, 16, 20)
    img = img.clamp(0.0, 1.0)
    gt = gt.clamp(0.0, 1.0)
    img[1] = gt[1]
    out["same_img"], out["same_gt"] = img.numpy(), gt.numpy()
    out["same_psnr3_f32"] = psnr(img, gt).numpy()
    out["same_psnr1_f32"] = psnr(img[None], gt[None]).numpy()
    out["same_l1_f64"] = l1_loss(img.double(), gt.double()).numpy()
    assert np.isinf(out["same_psnr3_f32"][1, 0]) and np.isfinite(out["same_psnr1_f32"]).all()

    np.savez_compressed(os.path.join(OUT, "eval_metrics.npz"), **out)
    print("wrote eval_metrics.npz", os.path.getsize(os.path.join(OUT, "eval_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
