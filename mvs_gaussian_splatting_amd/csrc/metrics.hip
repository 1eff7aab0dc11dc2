// Per-view evaluation of the reference's report loop (train.py:217-235, metrics.py:71-78) and its 8-bit image output
// (render.py / train.py:63): one streaming read of a rendered image and its ground truth gives the per-channel
// sum|d| and sum d^2 (L1, PSNR) and, optionally, the [H,W,3] byte image; eval_finish_kernel adds the block partials
// (and the SSIM partials of loss.hip's forward-only tile kernel) in a fixed order in double, writes the view's
// float32 record and adds the view into a device-side double[4] running sum, so that a report over any number of
// views needs one read-back.
// Built with -ffp-contract=off: the byte image is torch's clamp, mul, (add,) truncate, each rounded on its own.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "gsr_launch.h"
#include "ssim_tile.h"       // ssim_tiles: the SSIM partials of loss.hip's forward-only tile kernel

namespace gsr {

constexpr int EVAL_MAX_BLOCKS = 2048;      // the streaming grid's cap: the workspace holds 6 floats for each
constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / WAVE;
constexpr int FIN_THREADS = 512;      // one block; the double-precision log10 wants more than 128 registers

__device__ inline float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// torch: (clamp(x, 0, 1) * 255 [+ 0.5]).to(uint8) -- the value is in [0, 255.5], so the truncation is exact
__device__ inline uint32_t to_byte(float v, float bias) { return (uint32_t)(int)(clamp01(v) * 255.0f + bias); }

struct EvalAcc {
  float ab[3], sq[3];
  __device__ void add(int c, float x, float g) {
    const float d = x - g;
    ab[c] += fabsf(d);
    sq[c] += d * d;
  }
};

// VEC: a lane owns 4 consecutive pixels (six 16-byte loads, 12 output bytes as three dwords); needs H*W % 4 == 0 and
// 16-byte aligned images so that every plane base is aligned.  Otherwise a lane owns one pixel (three byte stores).
// METRICS = false: conversion only, gt is not read and nothing is summed.
template <bool VEC, bool METRICS>
__global__ __launch_bounds__(EV_THREADS) void eval_image_kernel(const float* __restrict__ x, const float* __restrict__ gt,
                                                                size_t hw, int flags, float* __restrict__ partials,
                                                                uint8_t* __restrict__ u8) {
  __shared__ float red[6][EV_WAVES];
  const bool cx = (flags & GSR_EVAL_CLAMP_X) != 0, cg = (flags & GSR_EVAL_CLAMP_GT) != 0;
  const float bias = (flags & GSR_EVAL_U8_TRUNCATE) ? 0.0f : 0.5f;
  const size_t items = VEC ? hw / 4 : hw;
  const size_t stride = (size_t)gridDim.x * EV_THREADS;
  EvalAcc a = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  for (size_t i = (size_t)blockIdx.x * EV_THREADS + threadIdx.x; i < items; i += stride) {
    if constexpr (VEC) {
      float4 v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = reinterpret_cast<const float4*>(x + c * hw)[i];
      if constexpr (METRICS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float4 g = reinterpret_cast<const float4*>(gt + c * hw)[i];
          float4 m = v[c];
          if (cx) m = make_float4(clamp01(m.x), clamp01(m.y), clamp01(m.z), clamp01(m.w));
          if (cg) g = make_float4(clamp01(g.x), clamp01(g.y), clamp01(g.z), clamp01(g.w));
          a.add(c, m.x, g.x); a.add(c, m.y, g.y); a.add(c, m.z, g.z); a.add(c, m.w, g.w);
        }
      }
      if (u8) {
        uint32_t b[12];   // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          b[c] = to_byte(v[c].x, bias); b[3 + c] = to_byte(v[c].y, bias);
          b[6 + c] = to_byte(v[c].z, bias); b[9 + c] = to_byte(v[c].w, bias);
        }
        uint32_t* o = reinterpret_cast<uint32_t*>(u8 + 12 * i);
#pragma unroll
        for (int w = 0; w < 3; ++w) o[w] = b[4 * w] | (b[4 * w + 1] << 8) | (b[4 * w + 2] << 16) | (b[4 * w + 3] << 24);
      }
    } else {
      float v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = x[c * hw + i];
      if constexpr (METRICS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float g = gt[c * hw + i];
          a.add(c, cx ? clamp01(v[c]) : v[c], cg ? clamp01(g) : g);
        }
      }
      if (u8) {
#pragma unroll
        for (int c = 0; c < 3; ++c) u8[3 * i + c] = (uint8_t)to_byte(v[c], bias);
      }
    }
  }
  if constexpr (METRICS) {
    const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float s0 = wave_reduce_add_f32(a.ab[c]), s1 = wave_reduce_add_f32(a.sq[c]);
      if (lane == 0) { red[c][wid] = s0; red[3 + c][wid] = s1; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
      float s = 0.0f;
#pragma unroll
      for (int w = 0; w < EV_WAVES; ++w) s += red[threadIdx.x][w];
      partials[6 * (size_t)blockIdx.x + threadIdx.x] = s;     // one sextet per block: no atomics, see loss.hip
    }
  }
}

// utils/image_utils.py:17-19 (mse == 0 gives +inf there too)
__device__ inline double psnr_of(double mse) { return 20.0 * log10(1.0 / sqrt(mse)); }

// One block.  sums 0..5 = the stream partials' columns, sum 6 = the SSIM tile partials; lane t adds entries t, t + 512,
// ... in order, then a fixed butterfly and a fixed walk over the waves: the result does not depend on arrival order.
__global__ __launch_bounds__(FIN_THREADS) void eval_finish_kernel(const float* __restrict__ partials, int nblocks,
                                                                  const float* __restrict__ ssim_partials,
                                                                  size_t ssim_blocks, double hw, int flags,
                                                                  float* __restrict__ view, double* __restrict__ acc) {
  __shared__ double red[7][FIN_THREADS / WAVE];
  double s[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < nblocks; i += FIN_THREADS) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] += (double)partials[6 * (size_t)i + k];
  }
  if (ssim_partials)
    for (size_t i = threadIdx.x; i < ssim_blocks; i += FIN_THREADS) s[6] += (double)ssim_partials[i];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const double r = wave_reduce_add_f64(s[k]);
    if (lane == 0) red[k][wid] = r;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    t[k] = 0.0;
    for (int w = 0; w < FIN_THREADS / WAVE; ++w) t[k] += red[k][w];
  }
  const double l1 = (t[0] + t[1] + t[2]) / (3.0 * hw);
  const double pc[3] = {psnr_of(t[3] / hw), psnr_of(t[4] / hw), psnr_of(t[5] / hw)};
  // the rows of the reference's view(img.shape[0], -1): one per channel of a [3,H,W] image, one for a [1,3,H,W] batch
  const double psnr = (flags & GSR_EVAL_PSNR_WHOLE) ? psnr_of((t[3] + t[4] + t[5]) / (3.0 * hw))
                                                    : (pc[0] + pc[1] + pc[2]) / 3.0;
  const double ssim = ssim_partials ? t[6] / (3.0 * hw) : 0.0;
  if (view) {
    view[0] = (float)l1; view[1] = (float)psnr; view[2] = (float)ssim;
#pragma unroll
    for (int k = 0; k < 6; ++k) view[3 + k] = (float)t[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) view[9 + c] = (float)pc[c];
  }
  if (acc) {   // calls on one stream are ordered: plain read-modify-write
    acc[0] += l1; acc[1] += psnr; acc[2] += ssim; acc[3] += 1.0;
  }
}

static int eval_blocks(size_t hw, bool vec) {
  const size_t items = vec ? hw / 4 : hw;
  const size_t b = (items + EV_THREADS - 1) / EV_THREADS;
  return (int)(b < (size_t)EVAL_MAX_BLOCKS ? (b ? b : 1) : (size_t)EVAL_MAX_BLOCKS);
}

static size_t eval_ssim_blocks(int H, int W) { return ssim_tiles(3, H, W); }

// gt == nullptr converts only.  workspace: 6 floats per streaming block, then eval_ssim_blocks floats
static void launch_eval_image(const float* x, const float* gt, int H, int W, int flags, float* view, double* acc,
                              uint8_t* u8, float* workspace, hipStream_t s) {
  const size_t hw = (size_t)H * W;
  const bool vec = hw % 4 == 0 && (((uintptr_t)x | (uintptr_t)gt) & 15u) == 0 && ((uintptr_t)u8 & 3u) == 0;
  const int blocks = eval_blocks(hw, vec);
  if (!gt) {
    if (vec) hipLaunchKernelGGL((eval_image_kernel<true, false>), dim3(blocks), dim3(EV_THREADS), 0, s, x, gt, hw, flags, nullptr, u8);
    else hipLaunchKernelGGL((eval_image_kernel<false, false>), dim3(blocks), dim3(EV_THREADS), 0, s, x, gt, hw, flags, nullptr, u8);
    return;
  }
  float* partials = workspace;                               // [EVAL_MAX_BLOCKS][6], then one float per SSIM tile
  float* ssim_partials = (flags & GSR_EVAL_SSIM) ? workspace + 6 * (size_t)EVAL_MAX_BLOCKS : nullptr;
  if (vec) hipLaunchKernelGGL((eval_image_kernel<true, true>), dim3(blocks), dim3(EV_THREADS), 0, s, x, gt, hw, flags, partials, u8);
  else hipLaunchKernelGGL((eval_image_kernel<false, true>), dim3(blocks), dim3(EV_THREADS), 0, s, x, gt, hw, flags, partials, u8);
  if (ssim_partials) launch_ssim_metric(x, gt, 3, H, W, flags, ssim_partials, s);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(FIN_THREADS), 0, s, partials, blocks, ssim_partials,
                     eval_ssim_blocks(H, W), (double)hw, flags, view, acc);
}

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

static const int32_t kEvalFlags = GSR_EVAL_CLAMP_X | GSR_EVAL_CLAMP_GT | GSR_EVAL_SSIM | GSR_EVAL_PSNR_WHOLE |
                                  GSR_EVAL_U8_TRUNCATE;
size_t gsr_eval_workspace_bytes(int32_t C, int32_t H, int32_t W, int32_t flags) {
  if (C != 3 || H <= 0 || W <= 0 || (flags & ~kEvalFlags)) return 0;
  return sizeof(float) * (6 * (size_t)EVAL_MAX_BLOCKS + ((flags & GSR_EVAL_SSIM) ? eval_ssim_blocks(H, W) : 0));
}
int gsr_eval_image(const float* x, const float* gt, int32_t C, int32_t H, int32_t W, int32_t flags, float* view_out,
                   double* acc, uint8_t* u8_out, void* workspace, void* stream) {
  if (!x || !gt) return fail(GSR_E_BADARG, "NULL image");
  if (!workspace) return fail(GSR_E_BADARG, "NULL workspace");
  if (!view_out && !acc && !u8_out) return fail(GSR_E_BADARG, "no output: view_out, acc and u8_out are all NULL");
  if (H <= 0 || W <= 0) return fail(GSR_E_BADARG, "bad image shape");
  if (C != 3) return fail(GSR_E_BADARG, "evaluation needs a 3-channel image");
  if (flags & ~kEvalFlags) return fail(GSR_E_BADARG, "unknown evaluation flag bits");
  if (!aligned({x, gt, view_out, workspace}, 3u) || !aligned({acc}, 7u))
    return fail(GSR_E_ALIGN, "images, view_out and workspace must be 4-byte aligned, acc 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_eval_image(x, gt, H, W, flags, view_out, acc, u8_out, static_cast<float*>(workspace), s);
  return check(false, s, "eval_image");
}
int gsr_image_to_u8(const float* x, int32_t C, int32_t H, int32_t W, int32_t flags, uint8_t* u8_out, void* stream) {
  if (!x || !u8_out) return fail(GSR_E_BADARG, "NULL image");
  if (H <= 0 || W <= 0) return fail(GSR_E_BADARG, "bad image shape");
  if (C != 3) return fail(GSR_E_BADARG, "the 8-bit output needs a 3-channel image");
  if (flags & ~GSR_EVAL_U8_TRUNCATE) return fail(GSR_E_BADARG, "unknown conversion flag bits");
  if (!aligned({x}, 3u)) return fail(GSR_E_ALIGN, "image must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_eval_image(x, nullptr, H, W, flags, nullptr, nullptr, u8_out, nullptr, s);
  return check(false, s, "image_to_u8");
}

}  // extern "C"
