// Training under a per-image mask (include/gsr.h, ABI v45; masked_loss.py): the fused L1 + D-SSIM loss
// of the masked images x' = m x, y' = m gt with its gradient for x, and the silhouette term of a rendered alpha map
// against the mask.  The SSIM is the one of csrc/loss.hip -- the tile core of ssim_tile.h, but s by a true division -- on x', y':
//
//   * ml_mask_sum_kernel      mask mode only.  At most ML_MAX_BLOCKS workgroups of 256 lanes; lane t of workgroup g adds
//                             the pixels g 256 + t, + gridDim 256, ... of the mask in ascending order in float64; the
//                             workgroup's sum goes to mask_partials[g].
//   * ml_mask_total_kernel    mask mode only, ONE workgroup: adds the partials, lane t taking t, t + 256, ..., and stores
//                             sum m and Z = C sum m in the header block.  The later kernels read Z from there: the host
//                             never sees it.
//   * masked_ssim_fwd_kernel  one workgroup per 16x16 output tile and channel.  Stages the 26x26 halo of x' and y' in LDS
//                             (each a float32 product, +0 where m is 0 or outside the image), runs the horizontal and the
//                             vertical 11-tap pass, and per pixel writes the three derivative maps A = dL/dmu1,
//                             B = dL/dE[x'^2], Cm = dL/dE[x'y'] scaled by dL/dS: -lambda / (C H W) in image mode,
//                             -lambda m_p / Z in mask mode.  One partial pair per workgroup: sum |x' - y'| and
//                             sum S (image) or sum m_p (1 - S) (mask).
//   * masked_finish_kernel    ONE workgroup of 1024 lanes: adds the partial pairs in float64, lane t taking t, t + 1024,
//                             ..., and writes the record (loss, L1 term, D-SSIM term, Z, sum m, degenerate, 0, 0).
//   * masked_ssim_bwd_kernel  the same grid: convolves the three maps and writes
//                             dL/dx = m (w*A + 2 x' (w*B) + y' (w*Cm) + (1 - lambda) sign(x' - y') / Z), +0 where m is 0.
//   * alpha_mask_kernel / alpha_mask_finish_kernel: the silhouette term, one elementwise walk of the mask sum's shape that
//                             writes the unit gradient and a float64 partial per workgroup, and the one-workgroup sum.
//
// image mode is 3 launches, mask mode 5, the silhouette term 2, all on the caller's stream.  No atomics: a kernel reads
// only what an earlier launch on the stream wrote, every sum has a fixed order, so value and gradient are the same bits
// from run to run and whatever the workspace held.
//
// LDS: the layout of csrc/loss.hip (ssim_tile.h).  Reductions: ordered_sum.h.
//
// Safety.  Every global read and write of the tile kernels is under 0 <= x < W, 0 <= y < H; the walks are under i < N.
// Every barrier is reached by every lane: none sits under a lane-dependent branch.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "ordered_sum.h"
#include "ssim_tile.h"

namespace gsr {

namespace {

constexpr int ML_BLOCK = 256;
constexpr int ML_WAVES = ML_BLOCK / WAVE;
constexpr int ML_MAX_BLOCKS = 1024;
constexpr int ML_FINISH = 1024;          // lanes of the one-workgroup sum of the tile partials
constexpr int ML_HDR_WORDS = 32;         // the header block at the head of the workspace, in 8-byte words: sum m, Z
constexpr int ML_RECORD_WORDS = 8;

static_assert(GSR_MASKED_LOSS_RECORD_WORDS == ML_RECORD_WORDS && GSR_MASKED_LOSS_MAX_BLOCKS == ML_MAX_BLOCKS,
              "constants of include/gsr.h");

inline int ml_blocks(int64_t N) {
  const int64_t nb = (N + ML_BLOCK - 1) / ML_BLOCK;
  return (int)(nb < ML_MAX_BLOCKS ? nb : ML_MAX_BLOCKS);
}

__global__ void __launch_bounds__(ML_BLOCK) ml_mask_sum_kernel(const float* __restrict__ mask, int64_t N,
                                                               double* __restrict__ mask_partials) {
  __shared__ double part[ML_WAVES][1];
  double v[1] = {0.0};
  const int64_t stride = (int64_t)gridDim.x * ML_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ML_BLOCK + threadIdx.x; i < N; i += stride) v[0] += (double)mask[i];
  ordered_block_sum<ML_WAVES, FROM_WAVE0>(v, part);
  if (threadIdx.x == 0) mask_partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(ML_BLOCK) ml_mask_total_kernel(const double* __restrict__ mask_partials, int nb, int C,
                                                                 double* __restrict__ hdr) {
  __shared__ double part[ML_WAVES][1];
  double v[1] = {0.0};
  for (int g = threadIdx.x; g < nb; g += ML_BLOCK) v[0] += mask_partials[g];
  ordered_block_sum<ML_WAVES, FROM_WAVE0>(v, part);
  if (threadIdx.x == 0) {
    hdr[0] = v[0];
    hdr[1] = (double)C * v[0];
  }
}

// 1 / Z as the tile kernels use it: the host's 1 / (C H W) in image mode, the header's Z in mask mode (0 when Z is not
// positive: every map and every gradient is then 0)
template <bool BY_MASK>
__device__ inline float ml_inv_z(float inv_n, const double* __restrict__ hdr) {
  if constexpr (BY_MASK) {
    const double Z = hdr[1];                     // one address for every lane
    return Z > 0.0 ? (float)(1.0 / Z) : 0.0f;
  } else {
    return inv_n;
  }
}

template <bool BY_MASK>
__global__ __launch_bounds__(SS_T * SS_T) void masked_ssim_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                       const float* __restrict__ M, int W, int H, Win11 win,
                                                                       float lambda, float inv_n,
                                                                       const double* __restrict__ hdr,
                                                                       float* __restrict__ partials,
                                                                       float* __restrict__ maps) {
  __shared__ float sx[SS_H][SS_H + 1];
  __shared__ float sy[SS_H][SS_H + 1];
  __shared__ float hz[5][SS_H][SS_T + 1];   // horizontally filtered x', y', x'x', y'y', x'y'
  __shared__ float red[SS_T * SS_T / WAVE][2];
  const int tx = threadIdx.x & (SS_T - 1), ty = threadIdx.x / SS_T;
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const size_t plane = (size_t)W * H;
  const float* __restrict__ xc = X + plane * blockIdx.z;
  const float* __restrict__ yc = Y + plane * blockIdx.z;
  const float inv_z = ml_inv_z<BY_MASK>(inv_n, hdr);
  const SsimMoments m = ssim_tile_moments(sx, sy, hz, win, x0, y0, [&](int gx, int gy, float& xv, float& yv) {
    xv = yv = 0.0f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t o = (size_t)gy * W + gx;
      const float mo = M[o];
      if (mo != 0.0f) {                         // a masked-out pixel is +0 whatever the images hold there
        xv = mo * xc[o];
        yv = mo * yc[o];
      }
    }
  });
  const int px = x0 + tx, py = y0 + ty;
  float v[2] = {0.f, 0.f};                      // the lane's |x' - y'| and its SSIM term
  if (px < W && py < H) {
    const SsimTerms t = ssim_terms(m);
    const float s = (t.N1 * t.N2) / t.den;      // a true division: exactly 1 where the two images agree on the window
    float dLds = -lambda * inv_z;               // d/ds of lambda (1 - mean s)
    if constexpr (BY_MASK) {
      const float mp = M[(size_t)py * W + px];
      dLds *= mp;                               // d/ds of lambda sum m (1 - s) / Z
      v[1] = mp * (1.0f - s);
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
  ordered_block_sum<SS_T * SS_T / WAVE, FROM_ZERO>(v, red);
  if (threadIdx.x == 0) {
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[2 * blk] = v[0];
    partials[2 * blk + 1] = v[1];
  }
}

__global__ __launch_bounds__(ML_FINISH) void masked_finish_kernel(size_t nblocks, const float* __restrict__ partials,
                                                                  double lambda, int by_mask, double n,
                                                                  const double* __restrict__ hdr,
                                                                  double* __restrict__ record) {
  __shared__ double part[ML_FINISH / WAVE][2];
  double v[2] = {0.0, 0.0};
  for (size_t i = threadIdx.x; i < nblocks; i += ML_FINISH) {
    v[0] += (double)partials[2 * i];
    v[1] += (double)partials[2 * i + 1];
  }
  ordered_block_sum<ML_FINISH / WAVE, FROM_WAVE0>(v, part);
  if (threadIdx.x == 0) {
    const double Z = by_mask ? hdr[1] : n;
    const bool live = Z > 0.0;
    const double l1 = live ? v[0] / Z : 0.0;
    const double ds = live ? (by_mask ? v[1] / Z : 1.0 - v[1] / Z) : 0.0;
    record[0] = (1.0 - lambda) * l1 + lambda * ds;
    record[1] = l1;
    record[2] = ds;
    record[3] = Z;
    record[4] = by_mask ? hdr[0] : 0.0;
    record[5] = live ? 0.0 : 1.0;
    record[6] = 0.0;
    record[7] = 0.0;
  }
}

template <bool BY_MASK>
__global__ __launch_bounds__(SS_T * SS_T) void masked_ssim_bwd_kernel(const float* __restrict__ X, const float* __restrict__ Y,
                                                                       const float* __restrict__ M, int W, int H, Win11 win,
                                                                       float lambda, float inv_n,
                                                                       const double* __restrict__ hdr,
                                                                       const float* __restrict__ maps,
                                                                       float* __restrict__ dL_dx) {
  __shared__ float sm[3][SS_H][SS_H + 1];
  __shared__ float hz[3][SS_H][SS_T + 1];
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const size_t plane = (size_t)W * H, total = plane * gridDim.z;
  const float l1_scale = (1.0f - lambda) * ml_inv_z<BY_MASK>(inv_n, hdr);
  const SsimMapGrads c = ssim_convolve_maps(sm, hz, win, maps + plane * blockIdx.z, total, W, H, x0, y0);
  const int px = x0 + (threadIdx.x & (SS_T - 1)), py = y0 + threadIdx.x / SS_T;
  if (px < W && py < H) {
    const size_t p = (size_t)py * W + px, o = plane * blockIdx.z + p;
    const float m = M[p];
    float g = 0.0f;                             // +0 on a masked-out pixel, whatever the images hold there
    if (m != 0.0f) {
      const float xv = m * X[o], yv = m * Y[o], d = xv - yv;
      const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
      g = m * (c.ga + 2.0f * xv * c.gb + yv * c.gc + l1_scale * sg);
    }
    dL_dx[o] = g;
  }
}

// the clamp of the bce mode, float32 constants: a is clamped to [lo, hi] and has gradient 0 outside
constexpr float AM_LO = 1e-6f;
constexpr float AM_HI = 1.0f - 1e-6f;

__global__ void __launch_bounds__(ML_BLOCK) alpha_mask_kernel(const float* __restrict__ A, const float* __restrict__ M,
                                                              int64_t N, int mode, double inv_n, float* __restrict__ grad,
                                                              double* __restrict__ partials) {
  __shared__ double part[ML_WAVES][1];
  double v[1] = {0.0};
  const int64_t stride = (int64_t)gridDim.x * ML_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ML_BLOCK + threadIdx.x; i < N; i += stride) {
    const float af = A[i];
    const double a = (double)af, m = (double)M[i];
    double term, g;
    if (mode == GSR_ALPHA_MASK_L1) {            // a kernel argument: every lane takes the same side
      const double d = a - m;
      term = fabs(d);
      g = d > 0.0 ? inv_n : (d < 0.0 ? -inv_n : 0.0);
    } else {
      const double ah = fmin(fmax(a, (double)AM_LO), (double)AM_HI);
      term = -(m * log(ah) + (1.0 - m) * log1p(-ah));
      g = (af < AM_LO || af > AM_HI) ? 0.0 : (ah - m) / (ah * (1.0 - ah)) * inv_n;
    }
    v[0] += term;
    if (grad) grad[i] = (float)g;
  }
  ordered_block_sum<ML_WAVES, FROM_WAVE0>(v, part);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(ML_BLOCK) alpha_mask_finish_kernel(const double* __restrict__ partials, int nb, int mode,
                                                                     double n, double* __restrict__ record) {
  __shared__ double part[ML_WAVES][1];
  double v[1] = {0.0};
  for (int g = threadIdx.x; g < nb; g += ML_BLOCK) v[0] += partials[g];
  ordered_block_sum<ML_WAVES, FROM_WAVE0>(v, part);
  if (threadIdx.x == 0) {
    record[0] = v[0] / n;
    record[1] = n;
    record[2] = (double)mode;
    record[3] = 0.0;
  }
}

// the workspace of the masked loss in bytes: the header block, the mask sum's partials, the three derivative maps, one
// partial pair per tile
struct MlLayout {
  size_t mask_partials, maps, partials, bytes, nblocks;
  MlLayout(int C, int H, int W) {
    nblocks = ssim_tiles(C, H, W);
    mask_partials = 8 * (size_t)ML_HDR_WORDS;
    maps = mask_partials + 8 * (size_t)ML_MAX_BLOCKS;
    partials = maps + sizeof(float) * 3 * (size_t)C * (size_t)H * (size_t)W;
    bytes = align_up(partials + sizeof(float) * 2 * nblocks, 256);
  }
};

inline bool ml_shape_ok(int32_t C, int32_t H, int32_t W) {
  return image_shape_ok(H, W) && C > 0 && C <= 65535 && (H + SS_T - 1) / SS_T <= 65535;
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_masked_l1_dssim_workspace_bytes(int32_t C, int32_t H, int32_t W) {
  if (!ml_shape_ok(C, H, W)) return 0;
  return MlLayout(C, H, W).bytes;
}

int gsr_masked_l1_dssim_loss_fwd_bwd(const float* x, const float* gt, const float* mask, int32_t C, int32_t H, int32_t W,
                                     double lambda_dssim, int32_t normalize, double* record, float* dL_dx, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!ml_shape_ok(C, H, W))
    return fail(GSR_E_BADARG, "the images must be [C,H,W] with 1 <= C <= 65535, 1 <= H W <= 2^28 and H <= 16 * 65535");
  if (normalize != GSR_MASKED_LOSS_NORM_IMAGE && normalize != GSR_MASKED_LOSS_NORM_MASK)
    return fail(GSR_E_BADARG, "normalize must be GSR_MASKED_LOSS_NORM_IMAGE or _NORM_MASK");
  if (!(lambda_dssim >= 0.0 && lambda_dssim <= 1.0)) return fail(GSR_E_BADARG, "lambda_dssim must lie in [0, 1]");
  if (!x || !gt || !mask || !record || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  const MlLayout L(C, H, W);
  if (workspace_bytes < L.bytes) return fail(GSR_E_CAPACITY, "masked loss workspace too small");
  if (!aligned({x, gt, mask, dL_dx}, 3u)) return fail(GSR_E_ALIGN, "x / gt / mask / dL_dx must be 4-byte aligned");
  if (!aligned({record}, 7u)) return fail(GSR_E_ALIGN, "record must be 8-byte aligned");
  if (!aligned({workspace}, 255u)) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  double* hdr = reinterpret_cast<double*>(ws);
  double* mask_partials = reinterpret_cast<double*>(ws + L.mask_partials);
  float* maps = reinterpret_cast<float*>(ws + L.maps);
  float* partials = reinterpret_cast<float*>(ws + L.partials);
  const Win11 win = make_window();
  const dim3 grid((W + SS_T - 1) / SS_T, (H + SS_T - 1) / SS_T, C), block(SS_T * SS_T);
  const float lambda = (float)lambda_dssim;
  const float inv_n = 1.0f / ((float)C * (float)H * (float)W);
  const double n = (double)C * (double)H * (double)W;
  const bool by_mask = normalize == GSR_MASKED_LOSS_NORM_MASK;
  if (by_mask) {
    const int64_t N = (int64_t)H * W;
    const int nb = ml_blocks(N);
    hipLaunchKernelGGL(ml_mask_sum_kernel, dim3(nb), dim3(ML_BLOCK), 0, s, mask, N, mask_partials);
    hipLaunchKernelGGL(ml_mask_total_kernel, dim3(1), dim3(ML_BLOCK), 0, s, mask_partials, nb, (int)C, hdr);
    hipLaunchKernelGGL(masked_ssim_fwd_kernel<true>, grid, block, 0, s, x, gt, mask, W, H, win, lambda, inv_n, hdr, partials,
                       maps);
  } else {
    hipLaunchKernelGGL(masked_ssim_fwd_kernel<false>, grid, block, 0, s, x, gt, mask, W, H, win, lambda, inv_n, hdr, partials,
                       maps);
  }
  hipLaunchKernelGGL(masked_finish_kernel, dim3(1), dim3(ML_FINISH), 0, s, L.nblocks, partials, lambda_dssim, by_mask ? 1 : 0,
                     n, hdr, record);
  if (dL_dx) {
    if (by_mask)
      hipLaunchKernelGGL(masked_ssim_bwd_kernel<true>, grid, block, 0, s, x, gt, mask, W, H, win, lambda, inv_n, hdr, maps,
                         dL_dx);
    else
      hipLaunchKernelGGL(masked_ssim_bwd_kernel<false>, grid, block, 0, s, x, gt, mask, W, H, win, lambda, inv_n, hdr, maps,
                         dL_dx);
  }
  return check(false, s, "masked_l1_dssim");
}

size_t gsr_alpha_mask_workspace_bytes(int32_t H, int32_t W) {
  const int64_t N = image_shape_ok(H, W) ? (int64_t)H * W : 1;
  return align_up(8 * (size_t)ml_blocks(N), 256);
}

int gsr_alpha_mask_loss_fwd_bwd(const float* alpha, const float* mask, int32_t H, int32_t W, int32_t mode, double* record,
                                float* dL_dalpha, void* workspace, size_t workspace_bytes, void* stream) {
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "the maps must hold between 1 and 2^28 pixels");
  if (mode != GSR_ALPHA_MASK_L1 && mode != GSR_ALPHA_MASK_BCE)
    return fail(GSR_E_BADARG, "mode must be GSR_ALPHA_MASK_L1 or GSR_ALPHA_MASK_BCE");
  if (!alpha || !mask || !record || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  if (workspace_bytes < gsr_alpha_mask_workspace_bytes(H, W)) return fail(GSR_E_CAPACITY, "alpha mask workspace too small");
  if (!aligned({alpha, mask, dL_dalpha}, 3u)) return fail(GSR_E_ALIGN, "alpha / mask / dL_dalpha must be 4-byte aligned");
  if (!aligned({record, workspace}, 7u)) return fail(GSR_E_ALIGN, "record and workspace must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t N = (int64_t)H * W;
  const int nb = ml_blocks(N);
  double* partials = static_cast<double*>(workspace);
  hipLaunchKernelGGL(alpha_mask_kernel, dim3(nb), dim3(ML_BLOCK), 0, s, alpha, mask, N, (int)mode, 1.0 / (double)N, dL_dalpha,
                     partials);
  hipLaunchKernelGGL(alpha_mask_finish_kernel, dim3(1), dim3(ML_BLOCK), 0, s, partials, nb, (int)mode, (double)N, record);
  return check(false, s, "alpha_mask_loss");
}

}  // extern "C"
