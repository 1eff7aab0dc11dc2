"""Float32 torch restatement of what csrc/metrics.hip computes for one view, in the kernels' order: per-lane running
sums over the lane's pixels, the wave butterfly, the walk over a block's waves -> block partials (float32) -> their sum
in double -> the float32 record.  SSIM: float32 per-pixel map (grouped convolution, as tests/test_gpu_parity.py) ->
16x16 tile partials in float32 -> double.  Shared by the host test (which shows the bars of the GPU test are reachable
in this arithmetic) and the GPU tests (expressions to compare against)."""
import math

import torch
import torch.nn.functional as F

EV_THREADS, EVAL_MAX_BLOCKS, WAVE = 256, 2048, 64
# the bars of the evaluation tests, against float64 values: L1 and the raw sums (tests/test_gpu_parity.py:375), SSIM
# (:382), PSNR in dB (4.3 dB per unit relative error of the mse, plus the rounding of a float32 near 16-32 dB)
REL_L1, REL_SSIM, ABS_PSNR_DB = 1e-6, 1e-5, 1e-5


def _lane_sums(vals: torch.Tensor, per_item: int) -> torch.Tensor:
    """vals: float32 [n] in pixel order; a lane owns per_item consecutive values per grid-stride step.  -> [blocks]"""
    items = vals.numel() // per_item
    blocks = max(1, min((items + EV_THREADS - 1) // EV_THREADS, EVAL_MAX_BLOCKS))
    stride = blocks * EV_THREADS
    K = (items + stride - 1) // stride
    v = torch.zeros(K * stride * per_item, dtype=torch.float32)
    v[:items * per_item] = vals[:items * per_item]
    v = v.reshape(K, stride, per_item).permute(1, 0, 2).reshape(stride, K * per_item)
    acc = torch.zeros(stride, dtype=torch.float32)
    for j in range(K * per_item):                      # the lane's running sum, one rounded add per pixel
        acc = acc + v[:, j]
    acc = acc.reshape(blocks, EV_THREADS // WAVE, WAVE)
    lane = torch.arange(WAVE)
    d = WAVE // 2
    while d:                                            # v += shfl_xor(v, d)
        acc = acc + acc[..., lane ^ d]
        d //= 2
    waves = acc[..., 0]
    out = torch.zeros(blocks, dtype=torch.float32)
    for w in range(waves.shape[1]):
        out = out + waves[:, w]
    return out


def stream_sums(x: torch.Tensor, gt: torch.Tensor, clamp_x=True, clamp_gt=True) -> torch.Tensor:
    """-> double[6]: sum|d| per channel, sum d^2 per channel (block partials in float32, summed in double)."""
    x, gt = x.float().reshape(3, -1), gt.float().reshape(3, -1)
    if clamp_x:
        x = x.clamp(0.0, 1.0)
    if clamp_gt:
        gt = gt.clamp(0.0, 1.0)
    d = x - gt
    per_item = 4 if x.shape[1] % 4 == 0 else 1
    parts = [_lane_sums(v[c], per_item) for v in (d.abs(), d * d) for c in range(3)]
    return torch.stack([p.double().sum() for p in parts])


def window(device="cpu", dtype=torch.float32):
    w1 = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    w1 = (w1 / w1.sum()).unsqueeze(1)
    return (w1 @ w1.t()).expand(3, 1, 11, 11).contiguous().to(device=device, dtype=dtype)


def ssim_map(p: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """per-pixel SSIM [3,H,W] in the inputs' dtype (utils/loss_utils.py:43-58 restated)"""
    win = window(p.device, p.dtype)
    p, q = p[None], q[None]
    m1, m2 = F.conv2d(p, win, padding=5, groups=3), F.conv2d(q, win, padding=5, groups=3)
    s1 = F.conv2d(p * p, win, padding=5, groups=3) - m1 * m1
    s2 = F.conv2d(q * q, win, padding=5, groups=3) - m2 * m2
    s12 = F.conv2d(p * q, win, padding=5, groups=3) - m1 * m2
    return (((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (s1 + s2 + 9e-4)))[0]


def ssim_sum(x: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """double: float32 map -> float32 sums of 16x16 tiles -> double"""
    m = ssim_map(x.float().clamp(0.0, 1.0), gt.float().clamp(0.0, 1.0))
    H, W = m.shape[1:]
    m = F.pad(m, (0, (-W) % 16, 0, (-H) % 16))
    tiles = m.reshape(3, m.shape[1] // 16, 16, m.shape[2] // 16, 16).permute(0, 1, 3, 2, 4).reshape(-1, 256)
    part = torch.zeros(tiles.shape[0], dtype=torch.float32)
    for j in range(256):
        part = part + tiles[:, j]
    return part.double().sum()


def psnr_db(mse: torch.Tensor) -> torch.Tensor:
    return 20.0 * torch.log10(1.0 / torch.sqrt(mse))


def record(x, gt, clamp_x=True, clamp_gt=True, whole=False, with_ssim=False) -> dict:
    """The float32 record eval_finish_kernel writes, from the restated sums."""
    hw = float(x.shape[-1] * x.shape[-2])
    t = stream_sums(x, gt, clamp_x, clamp_gt)
    pc = psnr_db(t[3:] / hw)
    out = {"l1": (t[:3].sum() / (3.0 * hw)).float(), "sums": t.float(), "psnr3": pc.float(),
           "psnr": (psnr_db(t[3:].sum() / (3.0 * hw)) if whole else pc.mean()).float()}
    if with_ssim:
        out["ssim"] = (ssim_sum(x, gt) / (3.0 * hw)).float()
    return out


def rel(got, want) -> float:
    got, want = (torch.as_tensor(v, dtype=torch.float64).cpu() for v in (got, want))
    return float(((got - want).abs() / want.abs()).max())


def ssim_mean_f64(x: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """mean SSIM in float64 with the float32 taps applied separably by shifted adds (element-wise ops only, so it runs in
    double on any device; differs from the 2D float32 window of create_window by the rounding of the tap products, 6e-8)."""
    w = window()[0, 0].sum(dim=0).double().to(x.device)          # rows of the outer product sum to the 1D taps
    w = w / w.sum()

    def blur(t):
        H, W = t.shape[-2:]
        p = F.pad(t, (5, 5, 5, 5))
        h = sum(w[k] * p[..., :, k:k + W] for k in range(11))
        return sum(w[k] * h[..., k:k + H, :] for k in range(11))

    p, q = x.double(), gt.double()
    m1, m2 = blur(p), blur(q)
    s1, s2, s12 = blur(p * p) - m1 * m1, blur(q * q) - m2 * m2, blur(p * q) - m1 * m2
    return (((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (s1 + s2 + 9e-4))).mean()


def expected_f64(x: torch.Tensor, gt: torch.Tensor, clamp_x=True, clamp_gt=True, with_ssim=False) -> dict:
    """The reference's expressions (utils/loss_utils.py:17-18, utils/image_utils.py:17-19) on .double() inputs."""
    a, b = x.double(), gt.double()
    a = a.clamp(0.0, 1.0) if clamp_x else a
    b = b.clamp(0.0, 1.0) if clamp_gt else b
    d = a - b
    sq = d * d
    out = {"l1": d.abs().mean(), "sums": torch.cat((d.abs().sum(dim=(1, 2)), sq.sum(dim=(1, 2)))),
           "psnr3": psnr_db(sq.reshape(3, -1).mean(1)), "psnr1": psnr_db(sq.mean())}
    out["psnr"] = out["psnr3"].mean()
    if with_ssim:
        out["ssim"] = ssim_mean_f64(a, b)
    return out
