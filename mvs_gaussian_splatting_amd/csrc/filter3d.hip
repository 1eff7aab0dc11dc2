// Mip-Splatting's 3D smoothing filter (include/gsr.h, ABI v47; filter3d.py): a per-Gaussian scalar from
// the training cameras, folded into the raw scales and opacities before the rasterizer sees them.
//
// filter3d_sample_kernel: one lane per Gaussian, 256-lane workgroups, no grid-stride loop, no LDS, no atomics, nothing
// waits on another workgroup.  The loop over the V views runs inside the kernel; the 80-byte table row of trip v is the
// same for every lane, so it arrives through scalar loads (as mesh_cull.hip's), and what a lane reads from memory is its
// own 12 bytes of xyz.  The pair's float32 arithmetic is csrc/filter3d_math.h (the unit is built with
// -ffp-contract=off): three divisions per counted view.  min_depth, max_rate and seen live in registers and are written
// once.  Each wave then reduces (max of min_depth, min of max_rate) over its seen lanes with shuffles and lane 0 writes the
// pair to the workspace: the "block maximum" of the finish, without a launch of its own.  Lanes past P stay in the wave
// for the shuffles and write nothing.
//
// filter3d_reduce_kernel: one workgroup over the ceil(P / 64) pairs -> (D, R) and the none-seen flag.  A maximum and a
// minimum do not depend on the order: the same bits from run to run.
// filter3d_write_kernel: one lane per Gaussian, filter3d_width.
//
// filter3d_apply_kernel / filter3d_apply_bwd_kernel: one lane per Gaussian, float64 inside the lane (the precedent is
// plane_depth.hip), 20 bytes in and 16 out (forward), 36 in and 16 out (backward); the closed forms are the header's.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "filter3d_math.h"

namespace gsr {

namespace {

constexpr int F3D_BLOCK = 256;
constexpr int F3D_REDUCE_BLOCK = 1024;

inline size_t f3d_waves(int64_t P) { return (size_t)((P + WAVE - 1) / WAVE); }
inline size_t f3d_result_offset(int64_t P) { return align_up(2 * f3d_waves(P) * sizeof(float), 16); }

struct F3dResult {
  float max_depth, min_rate;
  int32_t any_seen, pad;
};

__device__ inline float wave_max(float v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}
__device__ inline float wave_min(float v) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, WAVE));
  return v;
}

__global__ __launch_bounds__(F3D_BLOCK) void filter3d_sample_kernel(const float* __restrict__ xyz, int64_t P,
                                                                    const GsrFilterView* __restrict__ views, int V,
                                                                    float near, float margin, int accumulate,
                                                                    float* min_depth, float* max_rate, uint8_t* seen,
                                                                    float* __restrict__ pairs) {
  const int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x;
  const bool live = i < P;
  float d = INFINITY, r = 0.0f;
  int hit = 0;
  if (live) {
    const float* __restrict__ p = xyz + 3 * (size_t)i;
    const float x = p[0], y = p[1], z = p[2];
    if (accumulate) {
      d = min_depth[i];
      r = max_rate[i];
      hit = seen[i] != 0;
    }
    for (int v = 0; v < V; ++v)       // views[v]: uniform across the wave, scalar loads
      hit |= (int)filter3d_view_sample(views[v], x, y, z, near, margin, d, r);
    min_depth[i] = d;
    max_rate[i] = r;
    seen[i] = (uint8_t)hit;
  }
  // a wave's first row is a multiple of 64 (F3D_BLOCK is): the pair of rows 64 k .. 64 k + 63 goes to slot k
  const float wd = wave_max(hit ? d : -INFINITY), wr = wave_min(hit ? r : INFINITY);
  if ((threadIdx.x & (WAVE - 1)) == 0 && live) {
    const size_t k = (size_t)(i / WAVE);
    pairs[2 * k] = wd;
    pairs[2 * k + 1] = wr;
  }
}

__global__ __launch_bounds__(F3D_REDUCE_BLOCK) void filter3d_reduce_kernel(const float* __restrict__ pairs, size_t n,
                                                                           F3dResult* __restrict__ result,
                                                                           int32_t* __restrict__ none_seen) {
  __shared__ float sd[F3D_REDUCE_BLOCK / WAVE], sr[F3D_REDUCE_BLOCK / WAVE];
  float d = -INFINITY, r = INFINITY;
  for (size_t k = threadIdx.x; k < n; k += F3D_REDUCE_BLOCK) {
    d = fmaxf(d, pairs[2 * k]);
    r = fminf(r, pairs[2 * k + 1]);
  }
  d = wave_max(d);
  r = wave_min(r);
  const int wave = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    sd[wave] = d;
    sr[wave] = r;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < F3D_REDUCE_BLOCK / WAVE; ++w) {
      d = fmaxf(d, sd[w]);
      r = fminf(r, sr[w]);
    }
    const int any = d > -INFINITY;          // a seen row has a finite min_depth above near
    result->max_depth = d;
    result->min_rate = r;
    result->any_seen = any;
    result->pad = 0;
    *none_seen = !any;
  }
}

__global__ __launch_bounds__(F3D_BLOCK) void filter3d_write_kernel(int64_t P, const float* __restrict__ min_depth,
                                                                   const float* __restrict__ max_rate,
                                                                   const uint8_t* __restrict__ seen, int rule,
                                                                   float focal_max, float variance,
                                                                   const F3dResult* __restrict__ result,
                                                                   float* __restrict__ filter) {
  const int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x;
  if (i >= P) return;
  if (!result->any_seen) {
    filter[i] = 0.0f;
    return;
  }
  const bool paper = rule == GSR_FILTER3D_PAPER;
  filter[i] = filter3d_width(rule, seen[i] != 0, paper ? max_rate[i] : min_depth[i],
                             paper ? result->min_rate : result->max_depth, focal_max, variance);
}

__global__ __launch_bounds__(F3D_BLOCK) void filter3d_apply_kernel(const float* __restrict__ scaling,
                                                                   const float* __restrict__ opacity,
                                                                   const float* __restrict__ filter, int64_t P,
                                                                   float* __restrict__ scaling_out,
                                                                   float* __restrict__ opacity_out) {
  const int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x;
  if (i >= P) return;
  const float* __restrict__ sp = scaling + 3 * (size_t)i;
  const float s[3] = {sp[0], sp[1], sp[2]};
  float so[3], oo;
  filter3d_apply_row(s, opacity[i], filter[i], so, &oo);
  float* __restrict__ dp = scaling_out + 3 * (size_t)i;
  dp[0] = so[0];
  dp[1] = so[1];
  dp[2] = so[2];
  opacity_out[i] = oo;
}

__global__ __launch_bounds__(F3D_BLOCK) void filter3d_apply_bwd_kernel(const float* __restrict__ scaling,
                                                                       const float* __restrict__ opacity,
                                                                       const float* __restrict__ filter, int64_t P,
                                                                       const float* __restrict__ g_scaling,
                                                                       const float* __restrict__ g_opacity,
                                                                       float* __restrict__ d_scaling,
                                                                       float* __restrict__ d_opacity) {
  const int64_t i = (int64_t)blockIdx.x * F3D_BLOCK + threadIdx.x;
  if (i >= P) return;
  const float* __restrict__ sp = scaling + 3 * (size_t)i;
  const float* __restrict__ gp = g_scaling + 3 * (size_t)i;
  const float s[3] = {sp[0], sp[1], sp[2]}, g[3] = {gp[0], gp[1], gp[2]};
  float ds[3], dop;
  filter3d_apply_bwd_row(s, opacity[i], filter[i], g, g_opacity[i], ds, &dop);
  float* __restrict__ dp = d_scaling + 3 * (size_t)i;
  dp[0] = ds[0];
  dp[1] = ds[1];
  dp[2] = ds[2];
  d_opacity[i] = dop;
}

inline dim3 f3d_grid(int64_t n) { return dim3((unsigned)((n + F3D_BLOCK - 1) / F3D_BLOCK)); }
inline bool finite(float v) { return v - v == 0.0f; }                     // false for NaN and +-inf
inline bool rows_ok(int64_t P) { return P >= 0 && P <= (int64_t)INT32_MAX; }

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_filter3d_workspace_bytes(int64_t P) {
  if (!rows_ok(P)) return 0;
  return f3d_result_offset(P) + sizeof(F3dResult);
}

int gsr_filter3d_sample(const float* xyz, int64_t P, const GsrFilterView* views, int32_t V, float near_plane, float margin,
                        int32_t accumulate, float* min_depth, float* max_rate, uint8_t* seen, void* ws, size_t ws_bytes,
                        void* stream) {
  if (!rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (V < 0 || V > GSR_FILTER3D_MAX_VIEWS) return fail(GSR_E_BADARG, "V must lie in 0..65535");
  if (V > 0 && !views) return fail(GSR_E_BADARG, "the view table is NULL");
  if (!(near_plane > 0.0f) || !finite(near_plane)) return fail(GSR_E_BADARG, "near must be positive and finite");
  if (!(margin >= 0.0f) || !finite(margin)) return fail(GSR_E_BADARG, "margin must be finite and not negative");
  if (P > 0 && (!xyz || !min_depth || !max_rate || !seen || !ws))
    return fail(GSR_E_BADARG, "xyz / min_depth / max_rate / seen / ws is NULL");
  if (!aligned({xyz, min_depth, max_rate}, 3u)) return fail(GSR_E_ALIGN, "xyz, min_depth and max_rate must be 4-byte aligned");
  if (!aligned({views}, 7u)) return fail(GSR_E_ALIGN, "the view table must be 8-byte aligned");
  if (!aligned({ws}, 15u)) return fail(GSR_E_ALIGN, "ws must be 16-byte aligned");
  if (P > 0 && ws_bytes < gsr_filter3d_workspace_bytes(P)) return fail(GSR_E_CAPACITY, "ws is smaller than gsr_filter3d_workspace_bytes(P)");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(filter3d_sample_kernel, f3d_grid(P), dim3(F3D_BLOCK), 0, s, xyz, P, views, (int)V, near_plane, margin,
                     (int)accumulate, min_depth, max_rate, seen, static_cast<float*>(ws));
  return check(false, s, "filter3d_sample");
}

int gsr_filter3d_finish(int64_t P, const float* min_depth, const float* max_rate, const uint8_t* seen, int32_t rule,
                        float focal_max, float variance, void* ws, size_t ws_bytes, float* filter, int32_t* none_seen,
                        void* stream) {
  if (!rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (rule != GSR_FILTER3D_MIP_SPLATTING && rule != GSR_FILTER3D_PAPER) return fail(GSR_E_BADARG, "unknown rule");
  if (!(focal_max > 0.0f) || !finite(focal_max)) return fail(GSR_E_BADARG, "focal_max must be positive and finite");
  if (!(variance > 0.0f) || !finite(variance)) return fail(GSR_E_BADARG, "variance must be positive and finite");
  if (!none_seen || !ws) return fail(GSR_E_BADARG, "none_seen / ws is NULL");
  if (P > 0 && (!min_depth || !max_rate || !seen || !filter))
    return fail(GSR_E_BADARG, "min_depth / max_rate / seen / filter is NULL");
  if (!aligned({min_depth, max_rate, filter, none_seen}, 3u))
    return fail(GSR_E_ALIGN, "min_depth, max_rate, filter and none_seen must be 4-byte aligned");
  if (!aligned({ws}, 15u)) return fail(GSR_E_ALIGN, "ws must be 16-byte aligned");
  if (ws_bytes < gsr_filter3d_workspace_bytes(P)) return fail(GSR_E_CAPACITY, "ws is smaller than gsr_filter3d_workspace_bytes(P)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  F3dResult* result = reinterpret_cast<F3dResult*>(static_cast<char*>(ws) + f3d_result_offset(P));
  hipLaunchKernelGGL(filter3d_reduce_kernel, dim3(1), dim3(F3D_REDUCE_BLOCK), 0, s, static_cast<const float*>(ws),
                     f3d_waves(P), result, none_seen);
  if (P > 0)
    hipLaunchKernelGGL(filter3d_write_kernel, f3d_grid(P), dim3(F3D_BLOCK), 0, s, P, min_depth, max_rate, seen, (int)rule,
                       focal_max, variance, (const F3dResult*)result, filter);
  return check(false, s, "filter3d_finish");
}

int gsr_filter3d_apply(const float* scaling, const float* opacity, const float* filter, int64_t P, float* scaling_out,
                       float* opacity_out, void* stream) {
  if (!rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (P > 0 && (!scaling || !opacity || !filter || !scaling_out || !opacity_out)) return fail(GSR_E_BADARG, "NULL argument");
  if (P > 0 && (scaling_out == scaling || opacity_out == opacity)) return fail(GSR_E_BADARG, "the outputs may not alias the inputs");
  if (!aligned({scaling, opacity, filter, scaling_out, opacity_out}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(filter3d_apply_kernel, f3d_grid(P), dim3(F3D_BLOCK), 0, s, scaling, opacity, filter, P, scaling_out,
                     opacity_out);
  return check(false, s, "filter3d_apply");
}

int gsr_filter3d_apply_bwd(const float* scaling, const float* opacity, const float* filter, int64_t P,
                           const float* dL_dscaling_out, const float* dL_dopacity_out, float* dL_dscaling,
                           float* dL_dopacity, void* stream) {
  if (!rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (P > 0 && (!scaling || !opacity || !filter || !dL_dscaling_out || !dL_dopacity_out || !dL_dscaling || !dL_dopacity))
    return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({scaling, opacity, filter, dL_dscaling_out, dL_dopacity_out, dL_dscaling, dL_dopacity}, 3u))
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(filter3d_apply_bwd_kernel, f3d_grid(P), dim3(F3D_BLOCK), 0, s, scaling, opacity, filter, P,
                     dL_dscaling_out, dL_dopacity_out, dL_dscaling, dL_dopacity);
  return check(false, s, "filter3d_apply_bwd");
}

}  // extern "C"
