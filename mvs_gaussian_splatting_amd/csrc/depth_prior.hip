// Depth-prior loss of a rendered inverse-depth map against a per-image prior (include/gsr.h, ABI v44; depth_prior.py;
// DESIGN.md §7.31): upstream 3DGS's L1 term under a given affine, the same term under the weighted least-squares fit of
// the render on the prior, and one minus their weighted Pearson correlation.  The arithmetic of a pixel and of the fit is
// depth_prior_math.h, float64 with no fused multiply-add (this file is compiled with -ffp-contract=off), as
// tests/depth_prior_host_check.cpp builds it on the host.  The reduction is the word form of ordered_sum.h.
//
//   * depth_prior_sums_kernel    at most DEPTH_PRIOR_MAX_BLOCKS workgroups of 256 lanes.  Lane t of workgroup g takes the
//                                pixels g 256 + t, + gridDim 256, ... in ascending order and adds the six terms of every
//                                valid pixel to its own float64 sums, and 1 to its count.  Lanes 0..6 store the
//                                workgroup's 7 words (ordered_block_words) at partials[word][g].
//   * depth_prior_fit_kernel     ONE workgroup.  Per word, lane t adds partials[word][t], [t + 256], ... in ascending
//                                order (ordered_read_words), then the same block sum; lane 0 computes the fit
//                                (depth_prior_fit), stores it and the sums in the workspace's fit block and writes the
//                                record (for pearson with its loss 1 - r).  Not launched in the l1 mode.
//   * depth_prior_apply_kernel   the same grid and walk.  The affine and the moments are uniform: kernel arguments in the
//                                l1 mode, loads from the fit block at addresses every lane shares otherwise.  A lane
//                                writes the unit gradient of its pixel -- float64 in the lane, rounded once; +0 on an
//                                invalid pixel and under a degenerate fit; no store at all with a NULL gradient -- and, in
//                                the two L1 modes, adds 1, w and w |e| to its count and two sums, reduced to
//                                partials[word][g] as above (3 words).
//   * depth_prior_finish_kernel  ONE workgroup, the L1 modes only: adds the 3-word partials in the same fixed order and
//                                writes the loss: sum / (H W) with the count and Sw of its own walk (l1), or sum / Sw of
//                                the fit, 0 under a degenerate one (aligned_l1).
//
// l1 is 2 launches, aligned_l1 4, pearson 3, all on the caller's stream.  No atomics of any kind and no ticket: which
// workgroup finishes first changes nothing, a kernel reads only what an EARLIER launch on the stream wrote (word < its
// words, g < gridDim), so a call gives the same bits from run to run and whatever the workspace held before.
//
// Bandwidth: 8 (12 with a weight map) bytes a pixel read by the sums kernel, the same again plus a 4-byte store by the
// apply kernel.  LDS: the reduction words only (4 waves x 7 words, and 8 words of the finished sums in the one-workgroup
// kernels).  No local array is indexed dynamically: every loop over words has constant bounds and unrolls.
//
// Safety.  i < N bounds every read and the one store; N = H W <= 2^28, so i + stride stays far inside int64.  The loops
// are bounded at launch: ceil(N / (gridDim 256)) trips of the lane loop, ceil(gridDim / 256) <= 4 trips of the
// one-workgroup kernels.  Every barrier is reached by every lane of its workgroup: none sits under a lane-dependent
// branch, and the one under `mode` is under a kernel argument.  The fit block is read by the apply and finish kernels
// only in the modes in which the fit kernel wrote it.
#include <float.h>

#include "depth_prior_math.h"
#include "gsr_common.h"
#include "gsr_entry.h"
#include "ordered_sum.h"

namespace gsr {

namespace {

constexpr int DP_BLOCK = 256;
constexpr int DP_WAVES = DP_BLOCK / WAVE;
constexpr int DP_MAX_BLOCKS = 1024;  // 4 workgroups = 16 waves a CU on 256 CUs; the one-workgroup kernels make 4 trips at most
constexpr int DP_TRIP = DP_BLOCK;    // partials of one word that a one-workgroup kernel reads in one trip
constexpr int DP_APPLY_SUMS = 2;     // Sw and sum w |e| behind the count
constexpr int DP_APPLY_WORDS = 1 + DP_APPLY_SUMS;
// the fit block at the head of the workspace, in 8-byte words: DepthPriorFit, then the count (int64) and the six sums
constexpr int DP_FIT_BLOCK_WORDS = 32;
constexpr int DP_FIT_COUNT = 16;

static_assert(DEPTH_PRIOR_SUM_WORDS == 1 + DEPTH_PRIOR_SUMS, "the count and the sums");
static_assert(sizeof(DepthPriorFit) == 8 * DEPTH_PRIOR_FIT_WORDS && DEPTH_PRIOR_FIT_WORDS <= DP_FIT_COUNT &&
                  DP_FIT_COUNT + DEPTH_PRIOR_SUM_WORDS <= DP_FIT_BLOCK_WORDS,
              "layout of the fit block");
static_assert(GSR_DEPTH_PRIOR_BLOCK == DP_BLOCK && GSR_DEPTH_PRIOR_MAX_BLOCKS == DP_MAX_BLOCKS &&
                  GSR_DEPTH_PRIOR_SUM_WORDS == DEPTH_PRIOR_SUM_WORDS && GSR_DEPTH_PRIOR_FIT_COUNT_WORD == DP_FIT_COUNT &&
                  GSR_DEPTH_PRIOR_L1 == DEPTH_PRIOR_L1 && GSR_DEPTH_PRIOR_ALIGNED_L1 == DEPTH_PRIOR_ALIGNED_L1 &&
                  GSR_DEPTH_PRIOR_PEARSON == DEPTH_PRIOR_PEARSON,
              "constants of include/gsr.h");

inline int dp_blocks(int64_t N) {
  const int64_t nb = (N + DP_BLOCK - 1) / DP_BLOCK;
  return (int)(nb < DP_MAX_BLOCKS ? nb : DP_MAX_BLOCKS);
}
inline int dp_stride_words(int nb) { return (int)align_up((size_t)(nb > 0 ? nb : 1), 32); }

__global__ void __launch_bounds__(DP_BLOCK) depth_prior_sums_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                    const float* __restrict__ w, int64_t N,
                                                                    unsigned long long* __restrict__ partials,
                                                                    int stride_words) {
  __shared__ unsigned long long part[DP_WAVES][DEPTH_PRIOR_SUM_WORDS];
  CountSums<DEPTH_PRIOR_SUMS> acc;
  acc.zero();
  const int64_t stride = (int64_t)gridDim.x * DP_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * DP_BLOCK + threadIdx.x; i < N; i += stride) {
    const float xi = x[i], yi = y[i];
    const float wi = w ? w[i] : 1.0f;
    if (!depth_prior_valid(xi, yi, wi)) continue;
    double t[DEPTH_PRIOR_SUMS];
    depth_prior_terms(xi, yi, wi, t);
    acc.n += 1;
    for (int k = 0; k < DEPTH_PRIOR_SUMS; ++k) acc.s[k] += t[k];
  }
  const unsigned long long word = ordered_block_words<DP_WAVES>(acc, part);
  if (threadIdx.x < DEPTH_PRIOR_SUM_WORDS) partials[(size_t)threadIdx.x * stride_words + blockIdx.x] = word;
}

__global__ void __launch_bounds__(DP_BLOCK) depth_prior_fit_kernel(const unsigned long long* __restrict__ partials, int nb,
                                                                   int stride_words, int mode,
                                                                   unsigned long long* __restrict__ fit_block,
                                                                   double* __restrict__ record) {
  __shared__ unsigned long long part[DP_WAVES][DEPTH_PRIOR_SUM_WORDS];
  __shared__ unsigned long long total[DEPTH_PRIOR_SUM_WORDS + 1];
  CountSums<DEPTH_PRIOR_SUMS> acc;
  ordered_read_words<DP_TRIP>(acc, partials, nb, stride_words);
  const unsigned long long word = ordered_block_words<DP_WAVES>(acc, part);
  if (threadIdx.x < DEPTH_PRIOR_SUM_WORDS) total[threadIdx.x] = word;
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long n = (long long)total[0];
    double S[DEPTH_PRIOR_SUMS];
    for (int k = 0; k < DEPTH_PRIOR_SUMS; ++k) S[k] = __longlong_as_double((long long)total[1 + k]);
    DepthPriorFit f;
    depth_prior_fit(n, S, f);
    double* fb = reinterpret_cast<double*>(fit_block);
    fb[0] = f.n;
    fb[1] = f.Sw;
    fb[2] = f.mx;
    fb[3] = f.my;
    fb[4] = f.vx;
    fb[5] = f.vy;
    fb[6] = f.cov;
    fb[7] = f.sd;
    fb[8] = f.s;
    fb[9] = f.t;
    fb[10] = f.r;
    fb[11] = f.degenerate;
    fit_block[DP_FIT_COUNT] = (unsigned long long)n;
    for (int k = 0; k < DEPTH_PRIOR_SUMS; ++k) fb[DP_FIT_COUNT + 1 + k] = S[k];
    // aligned_l1: the finish kernel writes the loss behind the apply kernel
    record[0] = (mode == DEPTH_PRIOR_PEARSON && f.degenerate == 0.0) ? 1.0 - f.r : 0.0;
    record[1] = f.n;
    record[2] = f.Sw;
    record[3] = f.s;
    record[4] = f.t;
    record[5] = f.r;
    record[6] = f.degenerate;
    record[7] = 0.0;
  }
}

__global__ void __launch_bounds__(DP_BLOCK) depth_prior_apply_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                     const float* __restrict__ w, int64_t N, int mode,
                                                                     double scale, double offset, double pixels,
                                                                     const double* __restrict__ fit_block,
                                                                     float* __restrict__ grad,
                                                                     unsigned long long* __restrict__ partials,
                                                                     int stride_words) {
  __shared__ unsigned long long part[DP_WAVES][DP_APPLY_WORDS];
  DepthPriorFit f;
  f.n = f.Sw = f.mx = f.my = f.vx = f.vy = f.cov = f.sd = f.r = f.degenerate = 0.0;
  f.s = scale;
  f.t = offset;
  double denom = pixels;
  if (mode != DEPTH_PRIOR_L1) {  // uniform addresses: every lane reads the same words
    f.n = fit_block[0];
    f.Sw = fit_block[1];
    f.mx = fit_block[2];
    f.my = fit_block[3];
    f.vx = fit_block[4];
    f.vy = fit_block[5];
    f.cov = fit_block[6];
    f.sd = fit_block[7];
    f.s = fit_block[8];
    f.t = fit_block[9];
    f.r = fit_block[10];
    f.degenerate = fit_block[11];
    denom = f.Sw;
  }
  const bool live = f.degenerate == 0.0;
  CountSums<DP_APPLY_SUMS> acc;
  acc.zero();
  const int64_t stride = (int64_t)gridDim.x * DP_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * DP_BLOCK + threadIdx.x; i < N; i += stride) {
    const float xi = x[i], yi = y[i];
    const float wi = w ? w[i] : 1.0f;
    float g = 0.0f;
    if (live && depth_prior_valid(xi, yi, wi)) {
      if (mode == DEPTH_PRIOR_PEARSON) {
        g = depth_prior_grad_pearson(xi, yi, wi, f);
      } else {
        const double e = depth_prior_residual(xi, yi, f.s, f.t);
        g = depth_prior_grad_l1(e, wi, denom);
        acc.n += 1;
        acc.s[0] += (double)wi;
        acc.s[1] += (double)wi * fabs(e);
      }
    }
    if (grad) grad[i] = g;
  }
  if (mode != DEPTH_PRIOR_PEARSON) {  // a kernel argument: every lane of every workgroup takes the same side
    const unsigned long long word = ordered_block_words<DP_WAVES>(acc, part);
    if (threadIdx.x < DP_APPLY_WORDS) partials[(size_t)threadIdx.x * stride_words + blockIdx.x] = word;
  }
}

__global__ void __launch_bounds__(DP_BLOCK) depth_prior_finish_kernel(const unsigned long long* __restrict__ partials, int nb,
                                                                      int stride_words, int mode, double scale,
                                                                      double offset, double pixels,
                                                                      const double* __restrict__ fit_block,
                                                                      double* __restrict__ record) {
  __shared__ unsigned long long part[DP_WAVES][DP_APPLY_WORDS];
  __shared__ unsigned long long total[DP_APPLY_WORDS + 1];
  CountSums<DP_APPLY_SUMS> acc;
  ordered_read_words<DP_TRIP>(acc, partials, nb, stride_words);
  const unsigned long long word = ordered_block_words<DP_WAVES>(acc, part);
  if (threadIdx.x < DP_APPLY_WORDS) total[threadIdx.x] = word;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double sum = __longlong_as_double((long long)total[2]);
    if (mode == DEPTH_PRIOR_L1) {
      record[0] = sum / pixels;
      record[1] = (double)(long long)total[0];
      record[2] = __longlong_as_double((long long)total[1]);
      record[3] = scale;
      record[4] = offset;
      record[5] = 0.0;
      record[6] = 0.0;
      record[7] = 0.0;
    } else {
      record[0] = fit_block[11] == 0.0 ? sum / fit_block[1] : 0.0;
    }
  }
}

// the workspace in 8-byte words: the fit block, the sums kernel's partials, the apply kernel's partials
struct DpLayout {
  int nb, stride_words;
  size_t sums, apply, words;
  explicit DpLayout(int64_t N) {
    nb = dp_blocks(N);
    stride_words = dp_stride_words(nb);
    sums = DP_FIT_BLOCK_WORDS;
    apply = sums + (size_t)DEPTH_PRIOR_SUM_WORDS * stride_words;
    words = apply + (size_t)DP_APPLY_WORDS * stride_words;
  }
};

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_depth_prior_workspace_bytes(int32_t H, int32_t W) {
  const int64_t N = image_shape_ok(H, W) ? (int64_t)H * W : 1;
  return align_up(DpLayout(N).words * 8, 256);
}

int gsr_depth_prior_fwd_bwd(const float* invdepth, const float* prior, const float* weight, int32_t H, int32_t W,
                            int32_t mode, double scale, double offset, double* record, float* grad, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "the maps must hold between 1 and 2^28 pixels");
  if (mode != DEPTH_PRIOR_L1 && mode != DEPTH_PRIOR_ALIGNED_L1 && mode != DEPTH_PRIOR_PEARSON)
    return fail(GSR_E_BADARG, "mode must be GSR_DEPTH_PRIOR_L1, _ALIGNED_L1 or _PEARSON");
  if (!(scale >= -DBL_MAX && scale <= DBL_MAX) || !(offset >= -DBL_MAX && offset <= DBL_MAX))
    return fail(GSR_E_BADARG, "scale and offset must be finite");
  if (!invdepth || !prior || !record || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  if (workspace_bytes < gsr_depth_prior_workspace_bytes(H, W)) return fail(GSR_E_CAPACITY, "depth prior workspace too small");
  if (!aligned({invdepth, prior, weight, grad}, 3u))
    return fail(GSR_E_ALIGN, "invdepth / prior / weight / grad must be 4-byte aligned");
  if (!aligned({record}, 7u)) return fail(GSR_E_ALIGN, "record must be 8-byte aligned");
  if (!aligned({workspace}, 255u)) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  const int64_t N = (int64_t)H * W;
  const DpLayout L(N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* ws = static_cast<unsigned long long*>(workspace);
  const double* fit_block = reinterpret_cast<const double*>(ws);
  const double pixels = (double)N;
  if (mode != DEPTH_PRIOR_L1) {
    hipLaunchKernelGGL(depth_prior_sums_kernel, dim3(L.nb), dim3(DP_BLOCK), 0, s, invdepth, prior, weight, N, ws + L.sums,
                       L.stride_words);
    hipLaunchKernelGGL(depth_prior_fit_kernel, dim3(1), dim3(DP_BLOCK), 0, s, ws + L.sums, L.nb, L.stride_words, (int)mode,
                       ws, record);
  }
  hipLaunchKernelGGL(depth_prior_apply_kernel, dim3(L.nb), dim3(DP_BLOCK), 0, s, invdepth, prior, weight, N, (int)mode,
                     scale, offset, pixels, fit_block, grad, ws + L.apply, L.stride_words);
  if (mode != DEPTH_PRIOR_PEARSON)
    hipLaunchKernelGGL(depth_prior_finish_kernel, dim3(1), dim3(DP_BLOCK), 0, s, ws + L.apply, L.nb, L.stride_words,
                       (int)mode, scale, offset, pixels, fit_block, record);
  return check(false, s, "depth_prior_fwd_bwd");
}

}  // extern "C"
