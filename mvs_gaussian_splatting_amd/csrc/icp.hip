// Point-to-point ICP, the hot path between two nearest-point queries (include/gsr.h, ABI v43; geometry_eval.icp_step /
// icp_registration).  The arithmetic of a point and of a pair is icp_math.h, float64 with no fused
// multiply-add (this file is compiled with -ffp-contract=off), as tests/icp_host_check.cpp builds it on the host.
//
//   * icp_transform_kernel    out[i] = float32(M p_i): one lane per point, the 3x4 float64 matrix by value (kernel
//                             arguments: uniform loads), one rounding to float32 per coordinate.  The caller always
//                             transforms the ORIGINAL source by the CUMULATIVE matrix, so nothing accumulates.
//   * icp_accumulate_kernel   at most ICP_MAX_BLOCKS workgroups of 256 lanes.  Lane t of workgroup g takes the points
//                             g 256 + t, + gridDim 256, ... in ascending order and adds the 17 terms of every accepted
//                             pair (dist2 <= thr2, 0 <= nearest < R) to its own float64 sums, and 1 to its count.  The
//                             workgroup's 18 words are the word form of ordered_sum.h (576 bytes of LDS, the only
//                             LDS); lanes 0..17 store them at partials[word][g].
//   * icp_finish_kernel       ONE workgroup of 256 lanes, a launch of its own behind the first on the stream.  Per
//                             word, lane t adds partials[word][t], [t + 256], ... in ascending order (a trip reads
//                             ICP_FINISH_TRIP = 256 partials, coalesced), then the same block sum.
//
// No atomics of any kind and no ticket: which workgroup finishes first changes nothing.  The order of every addition is
// a function of Q alone (through the grid size), so a call gives the same bits from run to run and whatever the
// workspace held before: every partial that the finish reads, word < 18 and g < gridDim, was written by the launch
// before it.  A partial read by nobody is written by nobody.
//
// Bandwidth: 12 + 4 + 4 = 20 bytes of q, dist2 and nearest per source point, streamed once, and a 12-byte gather of the
// target row for an accepted pair.  Nothing else is read; the partials are 144 bytes a workgroup.
//
// Safety.  A neighbour index is used only after 0 <= nearest < R was tested; i < Q bounds every other read.  The loops
// are bounded at launch: ceil(Q / (gridDim 256)) trips of the lane loop, ceil(gridDim / 256) <= ICP_MAX_BLOCKS / 256
// trips of the finish.  Every barrier is reached by every lane of its workgroup (no return above one).  Q and R are at
// most GSR_NN_MAX_POINTS = 2^31 - 256, so i + stride stays inside int64 and 3 i is formed in size_t.
#include <float.h>

#include "gsr_common.h"
#include "gsr_entry.h"
#include "icp_math.h"
#include "ordered_sum.h"

namespace gsr {

namespace {

constexpr int ICP_BLOCK = 256;
constexpr int ICP_WAVES = ICP_BLOCK / WAVE;
constexpr int ICP_MAX_BLOCKS = 1024;        // 4 workgroups = 16 waves a CU on 256 CUs; the finish makes 4 trips at most
constexpr int ICP_FINISH_TRIP = ICP_BLOCK;  // partials of one word that the finish reads in one trip

static_assert(ICP_WORDS <= WAVE, "lanes 0..ICP_WORDS-1 of the first wave fold the waves' words");
static_assert(GSR_ICP_WORDS == ICP_WORDS && GSR_ICP_MAX_BLOCKS == ICP_MAX_BLOCKS && GSR_ICP_BLOCK == ICP_BLOCK,
              "constants of include/gsr.h");

inline int icp_blocks(int64_t Q) {
  const int64_t nb = (Q + ICP_BLOCK - 1) / ICP_BLOCK;
  return (int)(nb < ICP_MAX_BLOCKS ? nb : ICP_MAX_BLOCKS);
}

using IcpAcc = CountSums<ICP_SUMS>;         // one result or partial in registers (ordered_sum.h): word 0 is the count
static_assert(ICP_WORDS == 1 + ICP_SUMS, "the count and the sums");

__global__ void __launch_bounds__(ICP_BLOCK) icp_transform_kernel(const float* __restrict__ points, int Q, IcpMatrix M,
                                                                  float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x;
  if (i >= Q) return;
  const float p[3] = {points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2]};
  float o[3];
  icp_transform_point(M, p, o);
  for (int a = 0; a < 3; ++a) out[3 * (size_t)i + a] = o[a];
}

__global__ void __launch_bounds__(ICP_BLOCK) icp_accumulate_kernel(const float* __restrict__ q,
                                                                   const float* __restrict__ dist2,
                                                                   const int32_t* __restrict__ nearest, int Q,
                                                                   const float* __restrict__ target, int R, float thr2,
                                                                   IcpPivots c, unsigned long long* __restrict__ partials,
                                                                   int stride_words) {
  __shared__ unsigned long long part[ICP_WAVES][ICP_WORDS];
  IcpAcc acc;
  acc.zero();
  const int64_t stride = (int64_t)gridDim.x * ICP_BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * ICP_BLOCK + threadIdx.x; i < Q; i += stride) {
    const float d = dist2[i];
    const int32_t j = nearest[i];
    if (!icp_pair_accepted(d, thr2, j, R)) continue;
    const float qp[3] = {q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2]};
    const float rp[3] = {target[3 * (size_t)j], target[3 * (size_t)j + 1], target[3 * (size_t)j + 2]};
    double t[ICP_SUMS];
    icp_pair_terms(qp, rp, d, c, t);
    acc.n += 1;
    for (int k = 0; k < ICP_SUMS; ++k) acc.s[k] += t[k];
  }
  const unsigned long long word = ordered_block_words<ICP_WAVES>(acc, part);
  if (threadIdx.x < ICP_WORDS) partials[(size_t)threadIdx.x * stride_words + blockIdx.x] = word;
}

__global__ void __launch_bounds__(ICP_BLOCK) icp_finish_kernel(const unsigned long long* __restrict__ partials, int nb,
                                                               int stride_words, unsigned long long* __restrict__ out) {
  __shared__ unsigned long long part[ICP_WAVES][ICP_WORDS];
  IcpAcc acc;
  ordered_read_words<ICP_FINISH_TRIP>(acc, partials, nb, stride_words);
  const unsigned long long word = ordered_block_words<ICP_WAVES>(acc, part);
  if (threadIdx.x < ICP_WORDS) out[threadIdx.x] = word;
}

inline int icp_stride_words(int nb) { return (int)align_up((size_t)(nb > 0 ? nb : 1), 32); }

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_icp_transform(const float* points, int32_t Q, const double* matrix, float* out, void* stream) {
  if (Q < 0 || Q > GSR_NN_MAX_POINTS) return fail(GSR_E_BADARG, "Q must lie in 0..2^31-256");
  if (!matrix) return fail(GSR_E_BADARG, "NULL matrix");
  IcpMatrix M;
  for (int k = 0; k < 12; ++k) {
    if (!(matrix[k] >= -DBL_MAX && matrix[k] <= DBL_MAX)) return fail(GSR_E_BADARG, "the matrix must be finite");
    M.m[k] = matrix[k];
  }
  if (Q == 0) return 0;
  if (!points || !out) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({points, out}, 3u)) return fail(GSR_E_ALIGN, "points / out must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(icp_transform_kernel, dim3((unsigned)(((int64_t)Q + ICP_BLOCK - 1) / ICP_BLOCK)), dim3(ICP_BLOCK), 0, s,
                     points, Q, M, out);
  return check(false, s, "icp_transform");
}

size_t gsr_icp_workspace_bytes(int32_t Q) {
  return align_up((size_t)ICP_WORDS * icp_stride_words(icp_blocks(Q > 0 ? Q : 0)) * 8, 256);
}

int gsr_icp_accumulate(const float* q, const float* dist2, const int32_t* nearest, int32_t Q, const float* target,
                       int32_t R, float thr2, const double* pivots, void* workspace, size_t workspace_bytes, void* out,
                       void* stream) {
  if (R < 0 || Q < 0 || R > GSR_NN_MAX_POINTS || Q > GSR_NN_MAX_POINTS)
    return fail(GSR_E_BADARG, "R and Q must lie in 0..2^31-256");
  if (!pivots || !out) return fail(GSR_E_BADARG, "NULL pivots / out");
  if (!(thr2 >= 0.0f)) return fail(GSR_E_BADARG, "thr2 must be a non-negative number");
  IcpPivots c;
  for (int k = 0; k < 6; ++k) {
    if (!(pivots[k] >= -DBL_MAX && pivots[k] <= DBL_MAX)) return fail(GSR_E_BADARG, "the pivots must be finite");
    (k < 3 ? c.cq[k] : c.cr[k - 3]) = pivots[k];
  }
  if (!aligned({out}, 7u)) return fail(GSR_E_ALIGN, "out must be 8-byte aligned");
  const int nb = icp_blocks(Q);
  const int stride_words = icp_stride_words(nb);
  if (Q > 0) {
    if (!q || !dist2 || !nearest || !workspace) return fail(GSR_E_BADARG, "NULL argument");
    if (R > 0 && !target) return fail(GSR_E_BADARG, "NULL target");
    if (workspace_bytes < gsr_icp_workspace_bytes(Q)) return fail(GSR_E_CAPACITY, "icp workspace too small");
    if (!aligned({q, dist2, nearest, target}, 3u)) return fail(GSR_E_ALIGN, "q / dist2 / nearest / target must be 4-byte aligned");
    if (!aligned({workspace}, 255u)) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned long long* partials = static_cast<unsigned long long*>(workspace);
  if (nb > 0)
    hipLaunchKernelGGL(icp_accumulate_kernel, dim3(nb), dim3(ICP_BLOCK), 0, s, q, dist2, nearest, Q, target, R, thr2, c,
                       partials, stride_words);
  hipLaunchKernelGGL(icp_finish_kernel, dim3(1), dim3(ICP_BLOCK), 0, s, partials, nb, stride_words,
                     static_cast<unsigned long long*>(out));
  return check(false, s, "icp_accumulate");
}

}  // extern "C"
