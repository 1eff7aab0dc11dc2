// Fused training loss of the reference's step (train.py:99-101): (1-lambda) * L1 + lambda * (1 - SSIM), forward and
// gradient.  dssim_mode 1 is the 2D script's variant (2d_gaussian_splatting.py:196-202):
// (1-lambda) * L1 + lambda * mean(clamp((1 - SSIM)/2, 0, 1)).  SSIM as utils/loss_utils.py:23-63: 11x11 Gaussian window (sigma 1.5), depthwise,
// zero padding, C1 = 0.01^2, C2 = 0.03^2, mean over all pixels and channels.  The window is separable
// (create_window builds it as an outer product), so every 16x16 output tile stages a 26x26 halo in LDS and
// runs a horizontal then a vertical 11-tap pass: the tile core of ssim_tile.h, shared with masked_loss.hip.  The
// kernels here keep their halo loader (zero padding, the metric's clamp) and their epilogue.  Sums: ordered_sum.h.
//   forward : per pixel the five windowed moments -> SSIM, its sum, and the three derivative maps
//             A = dL/dmu1, B = dL/dE[x^2], Cm = dL/dE[xy]  (the loss depends on x only through them)
//   backward: dL/dx = w * A + 2 x (w * B) + y (w * Cm) + (1-lambda) sign(x-y)/n      (w symmetric)
#include "gsr_common.h"
#include "gsr_entry.h"
#include "gsr_launch.h"
#include "ordered_sum.h"
#include "ssim_tile.h"

namespace gsr {

// METRIC = false: the training loss (value partials + the three derivative maps).  METRIC = true: SSIM as a metric
// (metrics.py:75, csrc/metrics.hip): no derivative maps and no workspace for them, one SSIM partial per block, and the
// optional clamp of either image to [0, 1] on load (clamp_flags: GSR_EVAL_CLAMP_X | GSR_EVAL_CLAMP_GT; the zero padding
// is unchanged by it).
template <bool METRIC>
__global__ __launch_bounds__(SS_T * SS_T) void ssim_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                int W, int H, Win11 win, float lambda, float inv_n,
                                                                int dssim_mode, float* __restrict__ partials,
                                                                float* __restrict__ maps, int clamp_flags) {
  __shared__ float sx[SS_H][SS_H + 1];
  __shared__ float sy[SS_H][SS_H + 1];
  __shared__ float hz[5][SS_H][SS_T + 1];   // horizontally filtered x, y, xx, yy, xy
  __shared__ float red[SS_T * SS_T / WAVE][2];
  const int tx = threadIdx.x & (SS_T - 1), ty = threadIdx.x / SS_T;
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const size_t plane = (size_t)W * H;
  const float* __restrict__ xc = X + plane * blockIdx.z;
  const float* __restrict__ yc = Y + plane * blockIdx.z;
  const SsimMoments m = ssim_tile_moments(sx, sy, hz, win, x0, y0, [&](int gx, int gy, float& xv, float& yv) {
    xv = halo_load(xc, W, H, gx, gy);
    yv = halo_load(yc, W, H, gx, gy);
    if constexpr (METRIC) {
      if (clamp_flags & GSR_EVAL_CLAMP_X) xv = fminf(fmaxf(xv, 0.0f), 1.0f);
      if (clamp_flags & GSR_EVAL_CLAMP_GT) yv = fminf(fmaxf(yv, 0.0f), 1.0f);
    }
  });
  const int px = x0 + tx, py = y0 + ty;
  float v[2] = {0.f, 0.f};                  // the lane's |x - y| and its SSIM term
  if (px < W && py < H) {
    const SsimTerms t = ssim_terms(m);
    const float s = t.N1 * t.N2 * t.inv;
    if constexpr (METRIC) {
      v[1] = s;
    } else {
      float dLds = -lambda * inv_n;                                     // d/ds of lambda * (1 - mean s)
      if (dssim_mode == GSR_DSSIM_CLAMPED_HALF) {                       // lambda * mean(clamp((1 - s)/2, 0, 1))
        const float d = (1.0f - s) * 0.5f;
        dLds = (d >= 0.0f && d <= 1.0f) ? 0.5f * dLds : 0.0f;
        v[1] = fminf(fmaxf(d, 0.0f), 1.0f);
      } else {
        v[1] = s;
      }
      const SsimDerivs ds = ssim_derivs(m, t, s);
      const size_t o = plane * blockIdx.z + (size_t)py * W + px;
      const size_t total = plane * gridDim.z;
      maps[o] = dLds * ds.dm1;
      maps[total + o] = dLds * ds.dexx;
      maps[2 * total + o] = dLds * ds.dexy;
      v[0] = fabsf(sx[ty + SS_R][tx + SS_R] - sy[ty + SS_R][tx + SS_R]);
    }
  }
  // one partial (pair) per block, summed in block order by ssim_sum_kernel: tens of thousands of atomics on two
  // addresses serialise (0.6 ms at 1080p) and would make the loss value depend on the arrival order
  const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if constexpr (METRIC) {
    const float s_sum = ordered_block_sum<SS_T * SS_T / WAVE, FROM_ZERO>(v[1], &red[0][0]);
    if (threadIdx.x == 0) partials[blk] = s_sum;
  } else {
    ordered_block_sum<SS_T * SS_T / WAVE, FROM_ZERO>(v, red);
    if (threadIdx.x == 0) {
      partials[2 * blk] = v[0];
      partials[2 * blk + 1] = v[1];
    }
  }
}

// sums[0] += sum of the blocks' L1 partials, sums[1] += sum of their SSIM partials (fixed order: deterministic)
__global__ __launch_bounds__(1024) void ssim_sum_kernel(size_t nblocks, const float* __restrict__ partials,
                                                        float* __restrict__ sums) {
  __shared__ float red[1024 / WAVE][2];
  float v[2] = {0.f, 0.f};
  for (size_t i = threadIdx.x; i < nblocks; i += 1024) { v[0] += partials[2 * i]; v[1] += partials[2 * i + 1]; }
  ordered_block_sum<1024 / WAVE, FROM_ZERO>(v, red);
  if (threadIdx.x == 0) {
    sums[0] += v[0];
    sums[1] += v[1];
  }
}

__global__ __launch_bounds__(SS_T * SS_T) void ssim_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                int W, int H, Win11 win, float l1_scale,
                                                                const float* __restrict__ maps,
                                                                float* __restrict__ dL_dx) {
  __shared__ float sm[3][SS_H][SS_H + 1];
  __shared__ float hz[3][SS_H][SS_T + 1];
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const size_t plane = (size_t)W * H, total = plane * gridDim.z;
  const SsimMapGrads g = ssim_convolve_maps(sm, hz, win, maps + plane * blockIdx.z, total, W, H, x0, y0);
  const int px = x0 + (threadIdx.x & (SS_T - 1)), py = y0 + threadIdx.x / SS_T;
  if (px < W && py < H) {
    const size_t o = plane * blockIdx.z + (size_t)py * W + px;
    const float xv = X[o], yv = Y[o], d = xv - yv;
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    dL_dx[o] = g.ga + 2.0f * xv * g.gb + yv * g.gc + l1_scale * sg;
  }
}

static void launch_l1_dssim(const float* x, const float* gt, int C, int H, int W, float lambda, int dssim_mode,
                            float* sums, float* dL_dx, float* maps, hipStream_t s) {
  const Win11 win = make_window();
  const dim3 grid((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, C);
  const float inv_n = 1.0f / ((float)C * (float)H * (float)W);
  float* partials = maps + 3 * (size_t)C * H * W;      // behind the three derivative maps
  const size_t nblocks = ssim_tiles(C, H, W);
  hipLaunchKernelGGL(ssim_fwd_kernel<false>, grid, dim3(SS_T * SS_T), 0, s, x, gt, W, H, win, lambda, inv_n, dssim_mode,
                     partials, maps, 0);
  hipLaunchKernelGGL(ssim_sum_kernel, dim3(1), dim3(1024), 0, s, nblocks, partials, sums);
  hipLaunchKernelGGL(ssim_bwd_kernel, grid, dim3(SS_T * SS_T), 0, s, x, gt, W, H, win, (1.0f - lambda) * inv_n, maps, dL_dx);
}

// partials[block] = sum of the block's per-pixel SSIM, blocks in (channel, tile row, tile column) order; summed by
// metrics.hip's eval_finish_kernel
void launch_ssim_metric(const float* x, const float* gt, int C, int H, int W, int clamp_flags, float* partials,
                        hipStream_t s) {
  const dim3 grid((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, C);
  hipLaunchKernelGGL(ssim_fwd_kernel<true>, grid, dim3(SS_T * SS_T), 0, s, x, gt, W, H, make_window(), 0.0f, 0.0f,
                     GSR_DSSIM_ONE_MINUS_MEAN, partials, nullptr, clamp_flags);
}

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_l1_dssim_workspace_bytes(int32_t C, int32_t H, int32_t W) {
  if (C <= 0 || H <= 0 || W <= 0) return 0;
  return sizeof(float) * (3 * (size_t)C * (size_t)H * (size_t)W + 2 * ssim_tiles(C, H, W));
}
int gsr_l1_dssim_loss_fwd_bwd(const float* x, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                              int32_t dssim_mode, float* sums, float* dL_dx, void* workspace, void* stream) {
  if (!x || !gt || !sums || !dL_dx || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  if (C <= 0 || H <= 0 || W <= 0 || C > 65535) return fail(GSR_E_BADARG, "bad image shape");
  if (dssim_mode != GSR_DSSIM_ONE_MINUS_MEAN && dssim_mode != GSR_DSSIM_CLAMPED_HALF)
    return fail(GSR_E_BADARG, "unknown dssim_mode");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_l1_dssim(x, gt, C, H, W, lambda_dssim, dssim_mode, sums, dL_dx, static_cast<float*>(workspace), s);
  return check(false, s, "l1_dssim");
}

}  // extern "C"
