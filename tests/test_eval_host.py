"""The evaluation path (csrc/metrics.hip, mvs_gaussian_splatting_amd/metrics.py) without a GPU: the C ABI exports and
types its entry points, refuses bad arguments before any launch, the Python functions have no CPU path, and a float32
restatement of the kernels' arithmetic meets the GPU tests' bars against the reference's float64 values."""
import os
import re

import numpy as np
import pytest
import torch

from eval_restate import ABS_PSNR_DB, REL_L1, REL_SSIM, record, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_metrics.npz")
EVAL_SYMBOLS = ("gsr_eval_workspace_bytes", "gsr_eval_image", "gsr_image_to_u8")


def test_eval_entry_points_are_declared_exported_and_typed():
    from mvs_gaussian_splatting_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", src))
    lib = _lib.load()
    for n in EVAL_SYMBOLS:
        assert n in declared, f"{n} is not declared in include/gsr.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in _lib.SYMBOLS, f"{n} has no ctypes signature"
    assert int(re.search(r"#define GSR_ABI_VERSION (\d+)", src).group(1)) == _lib.ABI_VERSION == lib.gsr_abi_version() >= 17
    for name in ("CLAMP_X", "CLAMP_GT", "SSIM", "PSNR_WHOLE", "U8_TRUNCATE", "VIEW_FLOATS"):
        assert int(re.search(rf"#define GSR_EVAL_{name} (\d+)", src).group(1)) == getattr(_lib, f"EVAL_{name}")


def test_eval_workspace_size():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    plain = lib.gsr_eval_workspace_bytes(3, 1080, 1920, 0)
    with_ssim = lib.gsr_eval_workspace_bytes(3, 1080, 1920, _lib.EVAL_SSIM)
    assert 0 < plain <= 1 << 16                                     # block partials only: no image-sized scratch
    assert with_ssim - plain == 4 * 3 * 120 * 68                    # one float per 16x16 tile and channel, no maps
    assert with_ssim < lib.gsr_l1_dssim_workspace_bytes(3, 1080, 1920) // 100
    assert lib.gsr_eval_workspace_bytes(3, 0, 8, 0) == 0 and lib.gsr_eval_workspace_bytes(4, 8, 8, 0) == 0
    assert lib.gsr_eval_workspace_bytes(3, 8, 8, 1 << 9) == 0


def test_eval_bad_arguments_are_rejected_before_any_launch():
    from mvs_gaussian_splatting_amd import _lib
    lib = _lib.load()
    p = 4096                                   # a non-NULL, aligned pointer value; refused calls never touch it
    ok = dict(x=p, gt=p, C=3, H=8, W=8, flags=0, view=p, acc=None, u8=None, ws=p)

    def call(**over):
        a = dict(ok, **over)
        return lib.gsr_eval_image(a["x"], a["gt"], a["C"], a["H"], a["W"], a["flags"], a["view"], a["acc"], a["u8"],
                                  a["ws"], None)

    for over, msg in ((dict(x=None), b"NULL image"), (dict(gt=None), b"NULL image"), (dict(ws=None), b"workspace"),
                      (dict(view=None), b"no output"), (dict(H=0), b"shape"), (dict(W=-3), b"shape"),
                      (dict(C=4, u8=p), b"3-channel"), (dict(C=1), b"3-channel"), (dict(flags=32), b"flag"),
                      (dict(flags=-1), b"flag")):
        assert call(**over) == -1, over
        assert msg in lib.gsr_last_error(), (over, lib.gsr_last_error())
    assert call(x=p + 2) == -3 and call(acc=p + 4) == -3            # GSR_E_ALIGN
    with pytest.raises(_lib.GsrError, match="3-channel"):
        _lib.check(call(C=2), "gsr_eval_image")
    for args, msg in (((None, 3, 8, 8, 0, p), b"NULL"), ((p, 3, 8, 8, 0, None), b"NULL"), ((p, 3, 0, 8, 0, p), b"shape"),
                      ((p, 1, 8, 8, 0, p), b"3-channel"), ((p, 3, 8, 8, _lib.EVAL_SSIM, p), b"flag")):
        assert lib.gsr_image_to_u8(*args, None) == -1, args
        assert msg in lib.gsr_last_error()


def test_metrics_have_no_cpu_path():
    from mvs_gaussian_splatting_amd import _lib, psnr, ssim, image_metrics, to_uint8_hwc, EvalAccumulator, evaluate_views
    a, b = torch.rand(3, 8, 8), torch.rand(3, 8, 8)
    for fn in (psnr, ssim, image_metrics):
        with pytest.raises(_lib.GsrError, match="no CPU path"):
            fn(a, b)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        psnr(a[None], b[None])
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        to_uint8_hwc(a)
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        EvalAccumulator("cpu")
    with pytest.raises(_lib.GsrError, match="no CPU path"):
        evaluate_views([], None, None, torch.zeros(3))
    with pytest.raises(RuntimeError, match="l1_dssim_loss"):
        ssim(a.clone().requires_grad_(True), b)
    with pytest.raises(ValueError):
        ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="rounding"):
        to_uint8_hwc(a, rounding="floor")


@pytest.mark.parametrize("name", ["a", "b"])
def test_float32_restatement_of_the_kernels_meets_the_bars(name):
    """Block partials in float32 -> double sums -> float32 record, against the reference evaluated in float64; and the
    reference's own float32 values against the same bars (what float32 arithmetic alone can reach)."""
    g = np.load(GOLDEN)
    assert 0.03 < float(g[f"{name}_outside"]) < 0.06                # the clamp matters in these cases
    x, gt = torch.tensor(g[f"{name}_img"]), torch.tensor(g[f"{name}_gt"])
    r3 = record(x, gt, with_ssim=True)
    r1 = record(x, gt, whole=True)
    print(name, "l1", rel(r3["l1"], g[f"{name}_l1_f64"]), "sums", rel(r3["sums"], g[f"{name}_sums_f64"]),
          "ssim", rel(r3["ssim"], g[f"{name}_ssim_f64"]),
          "psnr3", float(np.abs(r3["psnr3"].numpy() - g[f"{name}_psnr3_f64"][:, 0]).max()),
          "psnr_mean", abs(float(r3["psnr"]) - float(g[f"{name}_psnr_mean_f64"])),
          "psnr1", abs(float(r1["psnr"]) - float(g[f"{name}_psnr1_f64"].item())))
    assert rel(r3["l1"], g[f"{name}_l1_f64"]) <= REL_L1
    assert rel(r3["sums"], g[f"{name}_sums_f64"]) <= REL_L1
    assert rel(r3["ssim"], g[f"{name}_ssim_f64"]) <= REL_SSIM
    assert float(np.abs(r3["psnr3"].double().numpy() - g[f"{name}_psnr3_f64"][:, 0]).max()) <= ABS_PSNR_DB
    assert abs(float(r3["psnr"]) - float(g[f"{name}_psnr_mean_f64"])) <= ABS_PSNR_DB
    assert abs(float(r1["psnr"]) - float(g[f"{name}_psnr1_f64"].item())) <= ABS_PSNR_DB
    # the reference's float32 results alone
    assert rel(g[f"{name}_l1_f32"], g[f"{name}_l1_f64"]) <= REL_L1
    assert rel(g[f"{name}_ssim_f32"], g[f"{name}_ssim_f64"]) <= REL_SSIM
    assert abs(float(g[f"{name}_psnr_mean_f32"]) - float(g[f"{name}_psnr_mean_f64"])) <= ABS_PSNR_DB
    assert abs(float(g[f"{name}_psnr1_f32"].item()) - float(g[f"{name}_psnr1_f64"].item())) <= ABS_PSNR_DB
    assert float(g[f"{name}_ssim4_f64"]) == float(g[f"{name}_ssim_f64"])      # [3,H,W] and [1,3,H,W]: the same mean


def test_fixture_sequence_and_inf_case_are_consistent():
    g = np.load(GOLDEN)
    run = g["seq_running_f64"]
    assert run.shape == (5, 2) and np.all(np.diff(run[:, 0]) > 0)
    assert np.allclose(g["seq_mean_f64"], run[-1] / 5, rtol=1e-15)
    tot_l1 = tot_psnr = 0.0
    for i in range(5):
        r = record(torch.tensor(g["seq_img"][i]), torch.tensor(g["seq_gt"][i]))
        tot_l1 += float(r["l1"])
        tot_psnr += float(r["psnr"])
        assert abs(tot_l1 - run[i, 0]) <= (i + 1) * REL_L1 * run[i, 0] and abs(tot_psnr - run[i, 1]) <= (i + 1) * ABS_PSNR_DB
    same = record(torch.tensor(g["same_img"]), torch.tensor(g["same_gt"]), whole=True)
    assert torch.isinf(same["psnr3"][1]) and same["psnr3"][1] > 0 and torch.isfinite(same["psnr"])
    assert np.isinf(g["same_psnr3_f32"][1, 0]) and np.isfinite(g["same_psnr1_f32"]).all()
