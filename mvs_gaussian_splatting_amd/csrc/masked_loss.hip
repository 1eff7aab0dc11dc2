// Training under a per-image mask (include/gsr.h, ABI v45; masked_loss.py): the fused L1 + D-SSIM loss
// of the masked images x' = m x, y' = m gt with its gradient for x, and the silhouette term of a rendered alpha map
// against the mask.  The SSIM is the one of csrc/loss.hip -- same window, tile and passes (ssim_window.h) -- on x', y':
//
//   * ml_mask_sum_kernel      mask mode only.  At most ML_MAX_BLOCKS workgroups of 256 lanes; lane t of workgroup g adds
//                             the pixels g 256 + t, + gridDim 256, ... of the mask in ascending order in float64; the
//                             workgroup's sum (ml_block_sum) goes to mask_partials[g].
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
// LDS: the layout of csrc/loss.hip -- rows of 27 and 17 dwords, odd strides, so that the 16 lanes of a tile row and the
// rows under them fall on different banks in both passes.  Reductions: the xor butterfly over the 64 lanes, one word per
// wave in LDS, thread 0 adds the waves in order.
//
// Safety.  Every global read and write of the tile kernels is under 0 <= x < W, 0 <= y < H; the walks are under i < N.
// Every barrier is reached by every lane: none sits under a lane-dependent branch.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "ssim_window.h"

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

// The sums of the workgroup's NV-vectors, valid in thread 0.  Every lane of the workgroup must call it.
template <int NV, int WAVES>
__device__ inline void ml_block_sum(double (&v)[NV], double (*part)[NV]) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += __shfl_xor(v[k], d, WAVE);
  }
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) part[wave][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      double s = part[0][k];
      for (int w = 1; w < WAVES; ++w) s += part[w][k];
      v[k] = s;
    }
  }
}

__global__ void __launch_bounds__(ML_BLOCK) ml_mask_sum_kernel(const float* __restrict__ mask, int64_t N,
                                                               double* __restrict__ mask_partials) {
  __shared__ double part[ML_WAVES][1];
  double v[1] = {0.0};
  const int64_t stride = (int64_t)gridDim.x * ML_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ML_BLOCK + threadIdx.x; i < N; i += stride) v[0] += (double)mask[i];
  ml_block_sum<1, ML_WAVES>(v, part);
  if (threadIdx.x == 0) mask_partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(ML_BLOCK) ml_mask_total_kernel(const double* __restrict__ mask_partials, int nb, int C,
                                                                 double* __restrict__ hdr) {
  __shared__ double part[ML_WAVES][1];
  double v[1] = {0.0};
  for (int g = threadIdx.x; g < nb; g += ML_BLOCK) v[0] += mask_partials[g];
  ml_block_sum<1, ML_WAVES>(v, part);
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
  __shared__ float red[2][SS_T * SS_T / WAVE];
  const int tx = threadIdx.x & (SS_T - 1), ty = threadIdx.x / SS_T;
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const size_t plane = (size_t)W * H;
  const float* __restrict__ xc = X + plane * blockIdx.z;
  const float* __restrict__ yc = Y + plane * blockIdx.z;
  const float inv_z = ml_inv_z<BY_MASK>(inv_n, hdr);
  for (int i = threadIdx.x; i < SS_H * SS_H; i += SS_T * SS_T) {
    const int hy = i / SS_H, hx = i - hy * SS_H;
    const int gx = x0 + hx - SS_R, gy = y0 + hy - SS_R;
    float xv = 0.0f, yv = 0.0f;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      const size_t o = (size_t)gy * W + gx;
      const float m = M[o];
      if (m != 0.0f) {                          // a masked-out pixel is +0 whatever the images hold there
        xv = m * xc[o];
        yv = m * yc[o];
      }
    }
    sx[hy][hx] = xv;
    sy[hy][hx] = yv;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SS_H * SS_T; i += SS_T * SS_T) {
    const int hy = i / SS_T, ox = i - hy * SS_T;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float xv = sx[hy][ox + k], yv = sy[hy][ox + k], wk = win.w[k];
      a += wk * xv; b += wk * yv; aa += wk * xv * xv; bb += wk * yv * yv; ab += wk * xv * yv;
    }
    hz[0][hy][ox] = a; hz[1][hy][ox] = b; hz[2][hy][ox] = aa; hz[3][hy][ox] = bb; hz[4][hy][ox] = ab;
  }
  __syncthreads();
  float m1 = 0.f, m2 = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    const float wk = win.w[k];
    m1 += wk * hz[0][ty + k][tx]; m2 += wk * hz[1][ty + k][tx]; exx += wk * hz[2][ty + k][tx];
    eyy += wk * hz[3][ty + k][tx]; exy += wk * hz[4][ty + k][tx];
  }
  const int px = x0 + tx, py = y0 + ty;
  float s_acc = 0.f, l1 = 0.f;
  if (px < W && py < H) {
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float mu1_sq = m1 * m1, mu2_sq = m2 * m2, mu12 = m1 * m2;
    const float s1 = exx - mu1_sq, s2 = eyy - mu2_sq, s12 = exy - mu12;
    const float N1 = 2.0f * mu12 + C1, N2 = 2.0f * s12 + C2, D1 = mu1_sq + mu2_sq + C1, D2 = s1 + s2 + C2;
    const float num = N1 * N2, den = D1 * D2;
    const float inv = 1.0f / den;
    const float s = num / den;                  // a true division: exactly 1 where the two images agree on the window
    float dLds = -lambda * inv_z;               // d/ds of lambda (1 - mean s)
    if constexpr (BY_MASK) {
      const float mp = M[(size_t)py * W + px];
      dLds *= mp;                               // d/ds of lambda sum m (1 - s) / Z
      s_acc = mp * (1.0f - s);
    } else {
      s_acc = s;
    }
    const float ds_dm1 = 2.0f * m2 * (N2 - N1) * inv - s * 2.0f * m1 * (D2 - D1) * inv;
    const size_t o = plane * blockIdx.z + (size_t)py * W + px;
    const size_t total = plane * gridDim.z;
    maps[o] = dLds * ds_dm1;
    maps[total + o] = dLds * (-s / D2);
    maps[2 * total + o] = dLds * (2.0f * N1 * inv);
    l1 = fabsf(sx[ty + SS_R][tx + SS_R] - sy[ty + SS_R][tx + SS_R]);
  }
  s_acc = wave_reduce_add_f32(s_acc);
  l1 = wave_reduce_add_f32(l1);
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  if (lane == 0) { red[0][wid] = l1; red[1][wid] = s_acc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < SS_T * SS_T / WAVE; ++w) { a += red[0][w]; b += red[1][w]; }
    const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[2 * blk] = a;
    partials[2 * blk + 1] = b;
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
  ml_block_sum<2, ML_FINISH / WAVE>(v, part);
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
  const int tx = threadIdx.x & (SS_T - 1), ty = threadIdx.x / SS_T;
  const int x0 = blockIdx.x * SS_T, y0 = blockIdx.y * SS_T;
  const size_t plane = (size_t)W * H, total = plane * gridDim.z;
  const float l1_scale = (1.0f - lambda) * ml_inv_z<BY_MASK>(inv_n, hdr);
  for (int i = threadIdx.x; i < SS_H * SS_H; i += SS_T * SS_T) {
    const int hy = i / SS_H, hx = i - hy * SS_H;
#pragma unroll
    for (int m = 0; m < 3; ++m)
      sm[m][hy][hx] = halo_load(maps + m * total + plane * blockIdx.z, W, H, x0 + hx - SS_R, y0 + hy - SS_R);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SS_H * SS_T; i += SS_T * SS_T) {
    const int hy = i / SS_T, ox = i - hy * SS_T;
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = win.w[k];
      a += wk * sm[0][hy][ox + k]; b += wk * sm[1][hy][ox + k]; c += wk * sm[2][hy][ox + k];
    }
    hz[0][hy][ox] = a; hz[1][hy][ox] = b; hz[2][hy][ox] = c;
  }
  __syncthreads();
  const int px = x0 + tx, py = y0 + ty;
  if (px < W && py < H) {
    float ga = 0.f, gb = 0.f, gc = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = win.w[k];
      ga += wk * hz[0][ty + k][tx]; gb += wk * hz[1][ty + k][tx]; gc += wk * hz[2][ty + k][tx];
    }
    const size_t p = (size_t)py * W + px, o = plane * blockIdx.z + p;
    const float m = M[p];
    float g = 0.0f;                             // +0 on a masked-out pixel, whatever the images hold there
    if (m != 0.0f) {
      const float xv = m * X[o], yv = m * Y[o], d = xv - yv;
      const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
      g = m * (ga + 2.0f * xv * gb + yv * gc + l1_scale * sg);
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
  ml_block_sum<1, ML_WAVES>(v, part);
  if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(ML_BLOCK) alpha_mask_finish_kernel(const double* __restrict__ partials, int nb, int mode,
                                                                     double n, double* __restrict__ record) {
  __shared__ double part[ML_WAVES][1];
  double v[1] = {0.0};
  for (int g = threadIdx.x; g < nb; g += ML_BLOCK) v[0] += partials[g];
  ml_block_sum<1, ML_WAVES>(v, part);
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
    nblocks = (size_t)((W + SS_T - 1) / SS_T) * (size_t)((H + SS_T - 1) / SS_T) * (size_t)C;
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
