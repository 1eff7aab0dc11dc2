// The per-Gaussian steps of the "3DGS as Markov-chain Monte Carlo" strategy (include/gsr.h, ABI v25).
// Inputs are the model's RAW tensors; the activations are preprocess's (preprocess_geom.h, GSR_ACT_*), in float32:
//   o = 1 / (1 + expf(-raw)),   s = expf(raw),   q = raw / fmaxf(sqrtf(((x x + y y) + z z) + w w), 1e-12f)
//
//   * mcmc_noise_kernel: xyz += Sigma v with Sigma = R diag(s^2) R^T, never formed.  One row per lane, a capped grid
//     that strides: 44 B of state and 12 B of noise read, 12 B written per row.  Float32, no contraction, in this order:
//       gate = 1 / (1 + expf(-100 * ((1 - o) - 0.995f)))            v_k = (noise_k * gate) * step_scale
//       R    = cov3d_from_scale_rot's matrix of q (r, x, y, z = q.x, q.y, q.z, q.w)
//       u_j  = (R_0j v_0 + R_1j v_1) + R_2j v_2      w_j = (s_j s_j) u_j      d_i = (R_i0 w_0 + R_i1 w_1) + R_i2 w_2
//       xyz_i = xyz_i + d_i
//     For o >= 0.9 the exponent passes 88.8, expf is +inf and gate is exactly 0: the row keeps its bits.
//   * mcmc_reg_kernel / mcmc_reg_finish_kernel / mcmc_reg_bwd_kernel: opacity_reg mean(o) + scale_reg mean(s).  A lane
//     adds its float32 activations in double; wave butterfly, waves in order, one (sum o, sum s) slot per block; one
//     block adds the slots in a fixed order and writes the 16-byte record {value, opacity_reg / P, scale_reg / (3P), 0},
//     each rounded once from double.  No atomics: the same bits from run to run.
//   * the sampler: w_i = rint(o_i 2^30) as int64 where o_i > alive_threshold, else 0 (contribution.hip's fixed point);
//     C = inclusive prefix sum of w in three launches (block sums, one block scans them, blocks write C); a draw r in
//     [0, 2^63) becomes t = floor(r T / 2^63) through the 128-bit product, and the sample is the smallest i with
//     C_i > t (binary search).  Integers only: the result does not depend on the launch shape.  No kernel waits on
//     another workgroup.
//   * mcmc_relocation_kernel: the opacity / scale correction of a Gaussian that stands for N copies of itself, in double
//     from the float32 activations to the one final rounding.
//
// Built with -ffp-contract=off: the noise step's order above is the contract.
#include "gsr_common.h"
#include "gsr_entry.h"

namespace gsr {

namespace {

constexpr int MCMC_MAX_BLOCKS = 2048;                                // streaming kernels cap their grid here and stride
constexpr int MC_THREADS = 256;
constexpr int MC_WAVES = MC_THREADS / WAVE;
constexpr int MC_RELOC_THREADS = 64;
constexpr int MC_NMAX = 51;                                      // the correction's binomials stop at C(50, k)
constexpr float MC_FX_ONE = 1073741824.0f;                       // 2^30

__device__ __forceinline__ float act_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ double wave_add_f64(double v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

int capped_blocks(size_t n, int per_block, int cap) {
  const size_t b = (n + per_block - 1) / per_block;
  return (int)(b < (size_t)cap ? (b ? b : 1) : (size_t)cap);
}

// ---- noise ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mcmc_noise_kernel(size_t P, float* __restrict__ xyz,
                                                                const float* __restrict__ scaling,
                                                                const float4* __restrict__ rotation,
                                                                const float* __restrict__ opacity,
                                                                const float* __restrict__ noise, float step_scale) {
  const size_t stride = (size_t)gridDim.x * MC_THREADS;
  for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < P; i += stride) {
    float4 q = rotation[i];
    const float raw_o = opacity[i];
    const float n0 = noise[3 * i], n1 = noise[3 * i + 1], n2 = noise[3 * i + 2];
    const float s0 = expf(scaling[3 * i]), s1 = expf(scaling[3 * i + 1]), s2 = expf(scaling[3 * i + 2]);
    const float o = act_sigmoid(raw_o);
    const float gate = 1.0f / (1.0f + expf(-100.0f * ((1.0f - o) - 0.995f)));
    const float v0 = (n0 * gate) * step_scale, v1 = (n1 * gate) * step_scale, v2 = (n2 * gate) * step_scale;
    const float qn = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
    q.x = q.x / qn; q.y = q.y / qn; q.z = q.z / qn; q.w = q.w / qn;
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    const float R00 = 1.0f - 2.0f * (y * y + z * z), R01 = 2.0f * (x * y - r * z), R02 = 2.0f * (x * z + r * y);
    const float R10 = 2.0f * (x * y + r * z), R11 = 1.0f - 2.0f * (x * x + z * z), R12 = 2.0f * (y * z - r * x);
    const float R20 = 2.0f * (x * z - r * y), R21 = 2.0f * (y * z + r * x), R22 = 1.0f - 2.0f * (x * x + y * y);
    const float w0 = (s0 * s0) * (R00 * v0 + R10 * v1 + R20 * v2);
    const float w1 = (s1 * s1) * (R01 * v0 + R11 * v1 + R21 * v2);
    const float w2 = (s2 * s2) * (R02 * v0 + R12 * v1 + R22 * v2);
    xyz[3 * i] = xyz[3 * i] + (R00 * w0 + R01 * w1 + R02 * w2);
    xyz[3 * i + 1] = xyz[3 * i + 1] + (R10 * w0 + R11 * w1 + R12 * w2);
    xyz[3 * i + 2] = xyz[3 * i + 2] + (R20 * w0 + R21 * w1 + R22 * w2);
  }
}

// ---- priors --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mcmc_reg_kernel(size_t P, const float* __restrict__ opacity,
                                                              const float* __restrict__ scaling,
                                                              double* __restrict__ slots) {
  __shared__ double red[MC_WAVES][2];
  double so = 0.0, ss = 0.0;
  const size_t stride = (size_t)gridDim.x * MC_THREADS;
  for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < P; i += stride) {
    so += (double)act_sigmoid(opacity[i]);
    ss += (double)expf(scaling[3 * i]);
    ss += (double)expf(scaling[3 * i + 1]);
    ss += (double)expf(scaling[3 * i + 2]);
  }
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  so = wave_add_f64(so);
  ss = wave_add_f64(ss);
  if (lane == 0) { red[wid][0] = so; red[wid][1] = ss; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double d = red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < MC_WAVES; ++w) d += red[w][threadIdx.x];
    slots[2 * (size_t)blockIdx.x + threadIdx.x] = d;
  }
}

// One block.  Lane t adds slots t, t + 256, ... in order, then the butterfly and the waves in order.
__global__ __launch_bounds__(MC_THREADS) void mcmc_reg_finish_kernel(const double* __restrict__ slots, int nslots,
                                                                     double P, float opacity_reg, float scale_reg,
                                                                     float* __restrict__ record) {
  __shared__ double red[MC_WAVES][2];
  double so = 0.0, ss = 0.0;
  for (int b = threadIdx.x; b < nslots; b += MC_THREADS) {
    so += slots[2 * (size_t)b];
    ss += slots[2 * (size_t)b + 1];
  }
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  so = wave_add_f64(so);
  ss = wave_add_f64(ss);
  if (lane == 0) { red[wid][0] = so; red[wid][1] = ss; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double to = 0.0, ts = 0.0;
  for (int w = 0; w < MC_WAVES; ++w) { to += red[w][0]; ts += red[w][1]; }
  const double fo = (double)opacity_reg / P, fs = (double)scale_reg / (3.0 * P);
  record[0] = (float)(fo * to + fs * ts);
  record[1] = (float)fo;
  record[2] = (float)fs;
  record[3] = 0.0f;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_reg_bwd_kernel(size_t P, const float* __restrict__ opacity,
                                                                  const float* __restrict__ scaling,
                                                                  const float* __restrict__ record,
                                                                  const float* __restrict__ grad_out,
                                                                  float* __restrict__ grad_opacity,
                                                                  float* __restrict__ grad_scaling) {
  const float g = grad_out[0];                                   // device memory: no host read-back
  const float go = g * record[1], gs = g * record[2];
  const size_t stride = (size_t)gridDim.x * MC_THREADS;
  for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < P; i += stride) {
    const float o = act_sigmoid(opacity[i]);
    grad_opacity[i] = go * (o * (1.0f - o));
#pragma unroll
    for (int k = 0; k < 3; ++k) grad_scaling[3 * i + k] = gs * expf(scaling[3 * i + k]);
  }
}

// ---- sampler -------------------------------------------------------------------------------------------------------
constexpr int MC_SCAN_ITEMS = 4;
constexpr int MC_SCAN_BLOCK = MC_THREADS * MC_SCAN_ITEMS;        // rows per scan block

__device__ __forceinline__ long long sample_weight(float raw, float alive_threshold) {
  const float o = act_sigmoid(raw);
  // o 2^30 is exact in float32 and at most 2^30; a NaN opacity compares false and weighs nothing
  return (alive_threshold < 0.0f ? o >= 0.0f : o > alive_threshold) ? (long long)__builtin_rintf(o * MC_FX_ONE) : 0ll;
}

__device__ __forceinline__ long long wave_incl_scan_i64(long long v, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long o = __shfl_up(v, d, WAVE);
    if (lane >= d) v += o;
  }
  return v;
}

// inclusive scan of one value per lane over the block; every lane of the block calls it.  *total: the block's sum.
__device__ __forceinline__ long long block_incl_scan_i64(long long v, long long* total) {
  __shared__ long long wave_tot[MC_WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wid = threadIdx.x / WAVE;
  v = wave_incl_scan_i64(v, lane);
  __syncthreads();                                               // the previous call's readers are done
  if (lane == WAVE - 1) wave_tot[wid] = v;
  __syncthreads();
  long long before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < MC_WAVES; ++w) {
    const long long t = wave_tot[w];
    if (w < wid) before += t;
    all += t;
  }
  *total = all;
  return v + before;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_weight_sums_kernel(size_t P, const float* __restrict__ opacity,
                                                                      float alive_threshold,
                                                                      long long* __restrict__ block_sums) {
  const size_t first = (size_t)blockIdx.x * MC_SCAN_BLOCK + (size_t)threadIdx.x * MC_SCAN_ITEMS;
  long long s = 0;
#pragma unroll
  for (int k = 0; k < MC_SCAN_ITEMS; ++k)
    if (first + k < P) s += sample_weight(opacity[first + k], alive_threshold);
  long long total;
  (void)block_incl_scan_i64(s, &total);
  if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// One block: block_sums[0 .. nb) -> exclusive prefix sums in place, block_sums[nb] = T.
__global__ __launch_bounds__(MC_THREADS) void mcmc_scan_sums_kernel(long long* __restrict__ block_sums, size_t nb) {
  long long carry = 0;
  for (size_t base = 0; base < nb; base += MC_THREADS) {
    const size_t i = base + threadIdx.x;
    const long long v = i < nb ? block_sums[i] : 0ll;
    long long total;
    const long long incl = block_incl_scan_i64(v, &total);
    if (i < nb) block_sums[i] = carry + incl - v;
    carry += total;
  }
  if (threadIdx.x == 0) block_sums[nb] = carry;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_prefix_kernel(size_t P, const float* __restrict__ opacity,
                                                                 float alive_threshold,
                                                                 const long long* __restrict__ block_offs,
                                                                 long long* __restrict__ C) {
  const size_t first = (size_t)blockIdx.x * MC_SCAN_BLOCK + (size_t)threadIdx.x * MC_SCAN_ITEMS;
  long long w[MC_SCAN_ITEMS], s = 0;
#pragma unroll
  for (int k = 0; k < MC_SCAN_ITEMS; ++k) {
    w[k] = first + k < P ? sample_weight(opacity[first + k], alive_threshold) : 0ll;
    s += w[k];
  }
  long long total;
  long long run = block_offs[blockIdx.x] + block_incl_scan_i64(s, &total) - s;
#pragma unroll
  for (int k = 0; k < MC_SCAN_ITEMS; ++k) {
    run += w[k];
    if (first + k < P) C[first + k] = run;
  }
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_zero_i32_kernel(int32_t* __restrict__ p, size_t n) {
  const size_t stride = (size_t)gridDim.x * MC_THREADS;
  for (size_t i = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; i < n; i += stride) p[i] = 0;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_sample_kernel(size_t P, const long long* __restrict__ C,
                                                                 const long long* __restrict__ total,
                                                                 const long long* __restrict__ draws, size_t n,
                                                                 int32_t* __restrict__ idx_out,
                                                                 int32_t* __restrict__ count_out) {
  const unsigned long long T = (unsigned long long)total[0];
  const size_t stride = (size_t)gridDim.x * MC_THREADS;
  for (size_t j = (size_t)blockIdx.x * MC_THREADS + threadIdx.x; j < n; j += stride) {
    if (T == 0ull) {
      idx_out[j] = -1;
      continue;
    }
    // r in [0, 2^63) (the sign bit is masked off: an out-of-contract draw cannot leave the table), T < 2^62:
    // floor(r T / 2^63) from the 128-bit product, always below T
    const unsigned long long r = (unsigned long long)draws[j] & 0x7fffffffffffffffull;
    const long long t = (long long)((__umul64hi(r, T) << 1) | ((r * T) >> 63));
    size_t lo = 0, hi = P - 1;                                   // C[P-1] = T > t: the answer exists
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (C[mid] > t) hi = mid; else lo = mid + 1;
    }
    idx_out[j] = (int32_t)lo;
    atomicAdd(count_out + lo, 1);
  }
}

// ---- relocation ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_RELOC_THREADS) void mcmc_relocation_kernel(size_t n, const int32_t* __restrict__ idx,
                                                                           const int32_t* __restrict__ count,
                                                                           const float* __restrict__ opacity,
                                                                           const float* __restrict__ scaling,
                                                                           float* __restrict__ new_opacity,
                                                                           float* __restrict__ new_scaling) {
  __shared__ double inv_sqrt[MC_NMAX];                           // 1 / sqrt(k + 1)
  if (threadIdx.x < MC_NMAX) inv_sqrt[threadIdx.x] = 1.0 / sqrt((double)(threadIdx.x + 1));
  __syncthreads();
  const size_t j = (size_t)blockIdx.x * MC_RELOC_THREADS + threadIdx.x;
  if (j >= n) return;
  const int32_t i = idx[j];
  if (i < 0) {                                                   // the sampler found no weight: nothing to correct
    new_opacity[j] = 0.0f;
    new_scaling[3 * j] = new_scaling[3 * j + 1] = new_scaling[3 * j + 2] = 0.0f;
    return;
  }
  const int32_t c = count[i];
  const int N = c >= MC_NMAX - 1 ? MC_NMAX : (c < 0 ? 1 : c + 1);
  const double o = (double)act_sigmoid(opacity[i]);
  const double op = 1.0 - pow(1.0 - o, 1.0 / (double)N);
  double D = 0.0;
  for (int m = 1; m <= N; ++m) {
    double binom = 1.0, pw = op, sign = 1.0;                     // C(m-1, k), o'^(k+1), (-1)^k
    for (int k = 0; k < m; ++k) {
      D += binom * (sign * inv_sqrt[k]) * pw;
      binom = binom * (double)(m - 1 - k) / (double)(k + 1);     // exact: below 2^53 up to C(50, 25) * 25
      pw *= op;
      sign = -sign;
    }
  }
  const double ratio = o / D;
#pragma unroll
  for (int k = 0; k < 3; ++k) new_scaling[3 * j + k] = (float)log(ratio * (double)expf(scaling[3 * (size_t)i + k]));
  const double hi = 1.0 - 1.1920928955078125e-07;                // 1 - 2^-23
  const double oc = op < 0.005 ? 0.005 : (op > hi ? hi : op);
  new_opacity[j] = (float)log(oc / (1.0 - oc));
}

size_t scan_blocks(size_t P) { return (P + MC_SCAN_BLOCK - 1) / MC_SCAN_BLOCK; }

// the priors leave one (sum o, sum s) pair of doubles per block in their workspace
size_t mcmc_reg_workspace_bytes() { return (size_t)MCMC_MAX_BLOCKS * 2 * sizeof(double); }

// the sampler's workspace: the int64 prefix sums [P], then the scan-block offsets and the total
size_t mcmc_sample_workspace_bytes(size_t P) {
  return align_up(P * sizeof(long long), 256) + align_up((scan_blocks(P) + 1) * sizeof(long long), 256);
}

void launch_mcmc_reg_fwd(size_t P, const float* opacity, const float* scaling, float opacity_reg, float scale_reg,
                         float* record, void* workspace, hipStream_t s) {
  const int blocks = capped_blocks(P, MC_THREADS, MCMC_MAX_BLOCKS);
  double* slots = static_cast<double*>(workspace);
  hipLaunchKernelGGL(mcmc_reg_kernel, dim3(blocks), dim3(MC_THREADS), 0, s, P, opacity, scaling, slots);
  hipLaunchKernelGGL(mcmc_reg_finish_kernel, dim3(1), dim3(MC_THREADS), 0, s, slots, blocks, (double)P, opacity_reg,
                     scale_reg, record);
}

void launch_mcmc_sample(size_t P, const float* opacity, float alive_threshold, const int64_t* draws, size_t n,
                        int32_t* idx_out, int32_t* count_out, void* workspace, hipStream_t s) {
  long long* C = static_cast<long long*>(workspace);
  long long* sums = reinterpret_cast<long long*>(static_cast<char*>(workspace) + align_up(P * sizeof(long long), 256));
  const size_t nb = scan_blocks(P);
  hipLaunchKernelGGL(mcmc_zero_i32_kernel, dim3(capped_blocks(P, MC_THREADS, MCMC_MAX_BLOCKS)), dim3(MC_THREADS), 0, s,
                     count_out, P);
  hipLaunchKernelGGL(mcmc_weight_sums_kernel, dim3((unsigned)nb), dim3(MC_THREADS), 0, s, P, opacity, alive_threshold, sums);
  hipLaunchKernelGGL(mcmc_scan_sums_kernel, dim3(1), dim3(MC_THREADS), 0, s, sums, nb);
  hipLaunchKernelGGL(mcmc_prefix_kernel, dim3((unsigned)nb), dim3(MC_THREADS), 0, s, P, opacity, alive_threshold, sums, C);
  if (n > 0)
    hipLaunchKernelGGL(mcmc_sample_kernel, dim3(capped_blocks(n, MC_THREADS, MCMC_MAX_BLOCKS)), dim3(MC_THREADS), 0, s, P,
                       C, sums + nb, reinterpret_cast<const long long*>(draws), n, idx_out, count_out);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

static int mcmc_rows_ok(int64_t P) { return P >= 0 && P <= (int64_t)INT32_MAX; }
int gsr_mcmc_noise(int64_t P, float* xyz, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                   const float* noise, float step_scale, void* stream) {
  if (!mcmc_rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (P > 0 && (!xyz || !scaling_raw || !rotation_raw || !opacity_raw || !noise)) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({xyz, scaling_raw, opacity_raw, noise}, 3u) || !aligned({rotation_raw}, 15u))
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned, rotations 16-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mcmc_noise_kernel, dim3(capped_blocks((size_t)P, MC_THREADS, MCMC_MAX_BLOCKS)), dim3(MC_THREADS), 0, s,
                     (size_t)P, xyz, scaling_raw, reinterpret_cast<const float4*>(rotation_raw), opacity_raw, noise,
                     step_scale);
  return check(false, s, "mcmc_noise");
}
size_t gsr_mcmc_reg_workspace_bytes(void) { return mcmc_reg_workspace_bytes(); }
int gsr_mcmc_reg_fwd(const float* opacity_raw, const float* scaling_raw, int64_t P, float opacity_reg, float scale_reg,
                     float* record, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mcmc_rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (!record || !workspace || (P > 0 && (!opacity_raw || !scaling_raw))) return fail(GSR_E_BADARG, "NULL argument");
  if (workspace_bytes < mcmc_reg_workspace_bytes()) return fail(GSR_E_BADARG, "workspace smaller than gsr_mcmc_reg_workspace_bytes()");
  if (!aligned({opacity_raw, scaling_raw}, 3u) || !aligned({workspace}, 7u) || !aligned({record}, 15u))
    return fail(GSR_E_ALIGN, "arrays must be 4-byte, the workspace 8-byte and the record 16-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mcmc_reg_fwd((size_t)P, opacity_raw, scaling_raw, opacity_reg, scale_reg, record, workspace, s);
  return check(false, s, "mcmc_reg_fwd");
}
int gsr_mcmc_reg_bwd(const float* opacity_raw, const float* scaling_raw, int64_t P, const float* record,
                     const float* grad_out, float* grad_opacity, float* grad_scaling, void* stream) {
  if (!mcmc_rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (!record || !grad_out || (P > 0 && (!opacity_raw || !scaling_raw || !grad_opacity || !grad_scaling)))
    return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({opacity_raw, scaling_raw, record, grad_out, grad_opacity, grad_scaling}, 3u))
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mcmc_reg_bwd_kernel, dim3(capped_blocks((size_t)P, MC_THREADS, MCMC_MAX_BLOCKS)), dim3(MC_THREADS), 0,
                     s, (size_t)P, opacity_raw, scaling_raw, record, grad_out, grad_opacity, grad_scaling);
  return check(false, s, "mcmc_reg_bwd");
}
size_t gsr_mcmc_sample_workspace_bytes(int64_t P) { return mcmc_rows_ok(P) ? mcmc_sample_workspace_bytes((size_t)P) : 0; }
int gsr_mcmc_sample(int64_t P, const float* opacity_raw, float alive_threshold, const int64_t* draws, int64_t n,
                    int32_t* idx_out, int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mcmc_rows_ok(P) || !mcmc_rows_ok(n)) return fail(GSR_E_BADARG, "P and n must lie in 0..2^31-1");
  if ((P > 0 && (!opacity_raw || !count_out || !workspace)) || (n > 0 && (!draws || !idx_out)))
    return fail(GSR_E_BADARG, "NULL argument");
  if (n > 0 && P == 0) return fail(GSR_E_BADARG, "samples asked of an empty model");
  if (P > 0 && workspace_bytes < mcmc_sample_workspace_bytes((size_t)P))
    return fail(GSR_E_BADARG, "workspace smaller than gsr_mcmc_sample_workspace_bytes(P)");
  if (!aligned({opacity_raw, idx_out, count_out}, 3u) || !aligned({draws, workspace}, 7u))
    return fail(GSR_E_ALIGN, "float / int32 arrays must be 4-byte, draws and workspace 8-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mcmc_sample((size_t)P, opacity_raw, alive_threshold, draws, (size_t)n, idx_out, count_out, workspace, s);
  return check(false, s, "mcmc_sample");
}
int gsr_mcmc_relocation(int64_t n, const int32_t* idx, const int32_t* count, const float* opacity_raw,
                        const float* scaling_raw, float* new_opacity_raw, float* new_scaling_raw, void* stream) {
  if (!mcmc_rows_ok(n)) return fail(GSR_E_BADARG, "n must lie in 0..2^31-1");
  if (n > 0 && (!idx || !count || !opacity_raw || !scaling_raw || !new_opacity_raw || !new_scaling_raw))
    return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({idx, count, opacity_raw, scaling_raw, new_opacity_raw, new_scaling_raw}, 3u))
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (n == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t blocks = ((size_t)n + MC_RELOC_THREADS - 1) / MC_RELOC_THREADS;
  hipLaunchKernelGGL(mcmc_relocation_kernel, dim3((unsigned)blocks), dim3(MC_RELOC_THREADS), 0, s, (size_t)n, idx, count,
                     opacity_raw, scaling_raw, new_opacity_raw, new_scaling_raw);
  return check(false, s, "mcmc_relocation");
}

}  // extern "C"
