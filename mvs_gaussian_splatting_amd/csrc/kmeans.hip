// k-means vector quantisation of per-Gaussian attribute rows (include/gsr.h, ABI v46; compress.py): the
// code norms, the assignment on the matrix cores and the atomic-free centre update.  The rule is csrc/kmeans_math.h.
//
//   * kmeans_code_norms_kernel   one lane per code: cnorm[c] = the fmaf chain of the row with itself.
//   * kmeans_assign_mfma_kernel  the hot path, score = |c|^2 - 2 x.c over N x K x D, x.c on v_mfma_f32_32x32x2_f32.
//       Workgroup: 256 lanes = 4 waves, 256 points; a wave owns 64 points as two 32-point tiles.  Its rows are read once
//       into registers in the instruction's B layout (lane l holds x[point l & 31][2 s + (l >> 5)] for step s), 2 STEPS
//       registers.  The codebook streams through LDS in stages of KM_STAGE = 128 codes, stored transposed ([dim][code],
//       row pitch 129 floats): the A operand of step s is one ds_read_b32 whose 32-lane halves read 32 consecutive floats
//       (no bank conflict; lanes l and l + 32 never conflict), and the staging writes of 32 consecutive lanes, which walk
//       the dims of a code, land 129 floats apart, on 32 different banks.  The next stage's rows are fetched into
//       registers while the current stage is multiplied.  Per 32-code tile the wave runs STEPS steps into two independent
//       accumulator tiles (one per point tile: the A operand is shared, and the 64-cycle dependent latency of one tile is
//       the issue slot of the other), both started at 0, so an accumulator is bit for bit kmeans_chain.
//       Epilogue: the accumulator of lane l holds point l & 31 against codes 8 (reg >> 2) + 4 (l >> 5) + (reg & 3) of the
//       tile, ascending in reg: each lane folds its 16 registers into a running (score, index) with '<', tiles and stages
//       arrive in ascending code order, and at the end lanes l and l + 32 merge (smaller score, then smaller index).
//       Codes past K sit in LDS as zero rows with cnorm = +inf, so their score is +inf and '<' never takes them; points
//       past N are computed on zeros and not stored.  No atomics, no inter-workgroup waiting: every (point, code) score is
//       a fixed expression and the minimum is order-free, so the bits repeat.
//       LDS: 2 STEPS x 129 + 128 floats (at most 33.5 KB at D = 64); VGPRs: 2 STEPS (x) + 32 (acc) + STEPS (prefetch) are
//       what the algorithm needs; two workgroups per CU by the launch bound (profiles/kmeans/NOTES.md).
//       STEPS is instantiated for 2, 8, 16, 24, 32 (D <= 4, 16, 32, 48, 64); steps past D multiply zeros, fmaf(0, 0, a) = a.
//   * kmeans_assign_valu_kernel  the same rule on the vector ALU for D <= 4, one lane per point, the codes broadcast from
//       LDS: the on-device cross-check of the matrix-core path (gsr_kmeans_assign_valu).
//   * kmeans_runs_kernel         from the stably sorted indices and their run heads: runs[c] = (first slot, end slot).
//   * kmeans_update_kernel       one 64-lane workgroup per code, lane d owns dim d and walks the run in slot order (rows
//       of a code in ascending row index): the float64 sum of w x (exact products) from the first member on, divided by
//       the float64 sum of w (or the count) and rounded to float32 once.  A code without rows or with sum w = 0 keeps its
//       centre and adds one to an integer counter (the only atomic here, an order-free integer add).
#include <float.h>

#include "gsr_common.h"
#include "gsr_entry.h"
#include "kmeans_math.h"

namespace gsr {

namespace {

constexpr int KM_BLOCK = 256;
constexpr int KM_POINTS = 256;                 // points per workgroup: 64 per wave
constexpr int KM_STAGE = 128;                  // codes per LDS stage: 4 tiles of 32
constexpr int KM_PITCH = KM_STAGE + 1;         // floats between the rows of two dims
constexpr int KM_VALU_STAGE = 1024;            // codes per LDS stage of the vector-ALU kernel

static_assert(KMEANS_MAX_D == GSR_KMEANS_MAX_D && KMEANS_MAX_K == GSR_KMEANS_MAX_K, "limits of include/gsr.h");

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void __launch_bounds__(KM_BLOCK) kmeans_code_norms_kernel(const float* codebook, int32_t K, int32_t D,
                                                                     float* cnorm) {
  const int32_t c = blockIdx.x * KM_BLOCK + threadIdx.x;
  if (c >= K) return;
  const float* row = codebook + (int64_t)c * D;
  cnorm[c] = kmeans_chain(row, row, D);
}

// the fold of one accumulator tile into a lane's running minimum; `cn` is the stage's cnorm in LDS, first the
// index of the tile's first code within the stage, code0 the stage's first code
__device__ __forceinline__ void fold_tile(const f32x16& acc, const float* cn, int first, int half, int32_t code0,
                                          float* best, int32_t* best_index) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int row = first + 8 * g + 4 * half;
    const float4 n4 = *reinterpret_cast<const float4*>(cn + row);
    const float n[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) kmeans_take(kmeans_score(acc[4 * g + j], n[j]), code0 + row + j, best, best_index);
  }
}

template <int STEPS>
__global__ void __launch_bounds__(KM_BLOCK, 2)           // two workgroups per CU: at most 256 registers a lane
    kmeans_assign_mfma_kernel(const float* __restrict__ x, int32_t N, int32_t D, const float* __restrict__ codebook,
                              const float* __restrict__ cnorm, int32_t K, int32_t* __restrict__ index_out,
                              float* __restrict__ dist2_out) {
  constexpr int DP = 2 * STEPS;
  constexpr int PER_LANE = KM_STAGE * DP / KM_BLOCK;           // staged floats per lane = STEPS
  __shared__ float codes[DP * KM_PITCH];
  __shared__ __attribute__((aligned(16))) float norms[KM_STAGE];

  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int r = lane & 31, half = lane >> 5;
  const int64_t base = (int64_t)blockIdx.x * KM_POINTS + wave * 64;

  // this lane's share of both point tiles, in the B layout
  float xb0[STEPS], xb1[STEPS];
  {
    const int64_t p0 = base + r, p1 = base + 32 + r;
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
      const int k = 2 * s + half;
      xb0[s] = (k < D && p0 < N) ? x[p0 * D + k] : 0.0f;
      xb1[s] = (k < D && p1 < N) ? x[p1 * D + k] : 0.0f;
    }
  }

  float best0 = __builtin_inff(), best1 = __builtin_inff();
  int32_t bi0 = 0, bi1 = 0;

  // staging: element e = threadIdx.x + KM_BLOCK * q of the stage's [KM_STAGE][DP] image is dim e % DP of code e / DP
  float pre[PER_LANE];
  auto fetch = [&](int32_t code0) {
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
      const int e = threadIdx.x + KM_BLOCK * q;
      const int i = e / DP, k = e % DP;
      const int32_t c = code0 + i;
      pre[q] = (c < K && k < D) ? codebook[(int64_t)c * D + k] : 0.0f;
    }
  };
  fetch(0);
  for (int32_t code0 = 0; code0 < K; code0 += KM_STAGE) {
    __syncthreads();                                   // every wave is done with the stage before
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q) {
      const int e = threadIdx.x + KM_BLOCK * q;
      codes[(e % DP) * KM_PITCH + e / DP] = pre[q];
    }
    if (threadIdx.x < KM_STAGE) {
      const int32_t c = code0 + (int32_t)threadIdx.x;
      norms[threadIdx.x] = c < K ? cnorm[c] : __builtin_inff();
    }
    __syncthreads();
    if (code0 + KM_STAGE < K) fetch(code0 + KM_STAGE);   // in flight under the products below

    const int tiles = min(KM_STAGE / 32, (K - code0 + 31) / 32);   // wave-uniform
#pragma unroll 1
    for (int t = 0; t < tiles; ++t) {
      f32x16 acc0 = {0}, acc1 = {0};
      const float* a_col = codes + half * KM_PITCH + 32 * t + r;
#pragma unroll
      for (int s = 0; s < STEPS; ++s) {
        const float a = a_col[2 * s * KM_PITCH];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb0[s], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, xb1[s], acc1, 0, 0, 0);
      }
      fold_tile(acc0, norms, 32 * t, half, code0, &best0, &bi0);
      fold_tile(acc1, norms, 32 * t, half, code0, &best1, &bi1);
    }
  }

  // lanes l and l + 32 share a point and hold disjoint codes
  kmeans_merge(__shfl_xor(best0, 32, WAVE), __shfl_xor(bi0, 32, WAVE), &best0, &bi0);
  kmeans_merge(__shfl_xor(best1, 32, WAVE), __shfl_xor(bi1, 32, WAVE), &best1, &bi1);
  const int64_t p = base + lane;                       // lanes 0..31 store tile 0, lanes 32..63 tile 1
  if (p >= N) return;
  const float best = half ? best1 : best0;
  index_out[p] = half ? bi1 : bi0;
  if (dist2_out) {
    const float* row = x + p * D;
    dist2_out[p] = kmeans_dist2(kmeans_chain(row, row, D), best);
  }
}

template <int D>
__global__ void __launch_bounds__(KM_BLOCK) kmeans_assign_valu_kernel(const float* __restrict__ x, int32_t N,
                                                                      const float* __restrict__ codebook,
                                                                      const float* __restrict__ cnorm, int32_t K,
                                                                      int32_t* __restrict__ index_out,
                                                                      float* __restrict__ dist2_out) {
  __shared__ float codes[KM_VALU_STAGE * D];
  __shared__ float norms[KM_VALU_STAGE];
  const int64_t p = (int64_t)blockIdx.x * KM_BLOCK + threadIdx.x;
  float row[D];
#pragma unroll
  for (int k = 0; k < D; ++k) row[k] = p < N ? x[p * D + k] : 0.0f;
  float best = __builtin_inff();
  int32_t bi = 0;
  for (int32_t code0 = 0; code0 < K; code0 += KM_VALU_STAGE) {
    const int32_t n = min(KM_VALU_STAGE, K - code0);
    __syncthreads();
    for (int e = threadIdx.x; e < n * D; e += KM_BLOCK) codes[e] = codebook[(int64_t)code0 * D + e];
    for (int e = threadIdx.x; e < n; e += KM_BLOCK) norms[e] = cnorm[code0 + e];
    __syncthreads();
    for (int32_t c = 0; c < n; ++c)
      kmeans_take(kmeans_score(kmeans_chain(row, codes + c * D, D), norms[c]), code0 + c, &best, &bi);
  }
  if (p >= N) return;
  index_out[p] = bi;
  if (dist2_out) dist2_out[p] = kmeans_dist2(kmeans_chain(row, row, D), best);
}

__global__ void __launch_bounds__(KM_BLOCK) kmeans_runs_kernel(const int64_t* keys_sorted, const uint8_t* head, int32_t N,
                                                               int32_t K, int32_t* runs, int32_t* counters) {
  const int32_t i = blockIdx.x * KM_BLOCK + threadIdx.x;
  if (i >= N) return;
  const int64_t c = keys_sorted[i];
  if ((uint64_t)c >= (uint64_t)K) {
    atomicOr(counters + 1, 1);
    return;
  }
  if (head[i]) runs[2 * c] = i;
  if (i == N - 1 || head[i + 1]) runs[2 * c + 1] = i + 1;
}

__global__ void __launch_bounds__(WAVE) kmeans_update_kernel(const float* x, const float* weights, const int64_t* order,
                                                             const int32_t* runs, int32_t N, int32_t D, float* codebook,
                                                             int32_t* counters) {
  const int32_t c = blockIdx.x;
  const int d = threadIdx.x;
  const int32_t lo = runs[2 * c], hi = runs[2 * c + 1];
  if (lo < 0 || hi > N) {
    if (d == 0) atomicOr(counters + 1, 1);
    return;
  }
  double sum = 0.0, wsum = 0.0;
  for (int32_t i = lo; i < hi; ++i) {                   // the rows of code c in ascending row index
    const int64_t row = order[i];
    if ((uint64_t)row >= (uint64_t)N) {
      if (d == 0) atomicOr(counters + 1, 1);
      return;
    }
    const double w = weights ? (double)weights[row] : 1.0;
    const double term = d < D ? w * (double)x[row * D + d] : 0.0;   // exact: 24 + 24 significant bits
    sum = i == lo ? term : sum + term;
    wsum = i == lo ? w : wsum + w;
  }
  if (hi <= lo || !(wsum > 0.0)) {                      // no row, or no weight: the centre stays
    if (d == 0) atomicAdd(counters, 1);
    return;
  }
  if (d < D) codebook[(int64_t)c * D + d] = (float)(sum / wsum);
}

inline bool kmeans_shape_ok(int64_t N, int32_t D, int32_t K) {
  return N >= 1 && N <= (int64_t)INT32_MAX && D >= 1 && D <= KMEANS_MAX_D && K >= 1 && K <= KMEANS_MAX_K;
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h): every argument is checked before any HIP call
using namespace gsr;

extern "C" {

int gsr_kmeans_code_norms(const float* codebook, int32_t K, int32_t D, float* cnorm, void* stream) {
  if (!kmeans_shape_ok(1, D, K)) return fail(GSR_E_BADARG, "K must lie in 1..65536 and D in 1..64");
  if (!codebook || !cnorm) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({codebook, cnorm}, 3u)) return fail(GSR_E_ALIGN, "codebook / cnorm must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kmeans_code_norms_kernel, dim3((unsigned)((K + KM_BLOCK - 1) / KM_BLOCK)), dim3(KM_BLOCK), 0, s,
                     codebook, K, D, cnorm);
  return check(false, s, "kmeans_code_norms");
}

static int kmeans_assign_args(const float* x, int64_t N, int32_t D, const float* codebook, const float* cnorm, int32_t K,
                              const int32_t* index_out, const float* dist2_out) {
  if (!kmeans_shape_ok(N, D, K)) return fail(GSR_E_BADARG, "N must lie in 1..2^31-1, K in 1..65536 and D in 1..64");
  if (!x || !codebook || !cnorm || !index_out) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({x, codebook, cnorm, index_out, dist2_out}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  return 0;
}

int gsr_kmeans_assign(const float* x, int64_t N, int32_t D, const float* codebook, const float* cnorm, int32_t K,
                      int32_t* index_out, float* dist2_out, void* stream) {
  if (const int rc = kmeans_assign_args(x, N, D, codebook, cnorm, K, index_out, dist2_out)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + KM_POINTS - 1) / KM_POINTS)), block(KM_BLOCK);
#define GSR_KMEANS_LAUNCH(STEPS)                                                                                          \
  hipLaunchKernelGGL(kmeans_assign_mfma_kernel<STEPS>, grid, block, 0, s, x, (int32_t)N, D, codebook, cnorm, K, index_out, \
                     dist2_out)
  if (D <= 4) GSR_KMEANS_LAUNCH(2);
  else if (D <= 16) GSR_KMEANS_LAUNCH(8);
  else if (D <= 32) GSR_KMEANS_LAUNCH(16);
  else if (D <= 48) GSR_KMEANS_LAUNCH(24);
  else GSR_KMEANS_LAUNCH(32);
#undef GSR_KMEANS_LAUNCH
  return check(false, s, "kmeans_assign");
}

int gsr_kmeans_assign_valu(const float* x, int64_t N, int32_t D, const float* codebook, const float* cnorm, int32_t K,
                           int32_t* index_out, float* dist2_out, void* stream) {
  if (const int rc = kmeans_assign_args(x, N, D, codebook, cnorm, K, index_out, dist2_out)) return rc;
  if (D > 4) return fail(GSR_E_BADARG, "the vector-ALU assignment takes D in 1..4");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((N + KM_BLOCK - 1) / KM_BLOCK)), block(KM_BLOCK);
#define GSR_KMEANS_LAUNCH(DIM)                                                                                       \
  hipLaunchKernelGGL(kmeans_assign_valu_kernel<DIM>, grid, block, 0, s, x, (int32_t)N, codebook, cnorm, K, index_out, \
                     dist2_out)
  if (D == 1) GSR_KMEANS_LAUNCH(1);
  else if (D == 2) GSR_KMEANS_LAUNCH(2);
  else if (D == 3) GSR_KMEANS_LAUNCH(3);
  else GSR_KMEANS_LAUNCH(4);
#undef GSR_KMEANS_LAUNCH
  return check(false, s, "kmeans_assign_valu");
}

int gsr_kmeans_update(const float* x, const float* weights, int64_t N, int32_t D, const int64_t* keys_sorted,
                      const int64_t* order, const uint8_t* head, int32_t K, int32_t* runs, float* codebook,
                      int32_t* counters, void* stream) {
  if (!kmeans_shape_ok(N, D, K)) return fail(GSR_E_BADARG, "N must lie in 1..2^31-1, K in 1..65536 and D in 1..64");
  if (!x || !keys_sorted || !order || !head || !runs || !codebook || !counters) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({x, weights, runs, codebook, counters}, 3u))
    return fail(GSR_E_ALIGN, "float and int32 arrays must be 4-byte aligned");
  if (!aligned({keys_sorted, order}, 7u)) return fail(GSR_E_ALIGN, "keys_sorted / order must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  GSR_HIP(hipMemsetAsync(runs, 0, sizeof(int32_t) * 2 * (size_t)K, s));
  hipLaunchKernelGGL(kmeans_runs_kernel, dim3((unsigned)((N + KM_BLOCK - 1) / KM_BLOCK)), dim3(KM_BLOCK), 0, s,
                     keys_sorted, head, (int32_t)N, K, runs, counters);
  hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)K), dim3(WAVE), 0, s, x, weights, order, runs, (int32_t)N, D,
                     codebook, counters);
  return check(false, s, "kmeans_update");
}

}  // extern "C"
