// Two steps of the model's lifecycle that touch every opacity (include/gsr.h, ABI v18):
//
//   * the fork's opacity sparsity term of train.py:102-106, `w * mean(|o - 1|)` over the rows with o = sigmoid(raw)
//     below 0.005: opacity_sparsity_kernel streams the [P,1] tensor once and leaves one (sum, count) pair per block,
//     opacity_sparsity_finish_kernel adds the pairs in a fixed order in double (ordered_sum.h) and writes the record the backward reads
//     from device memory (loss, n, w / n), opacity_sparsity_bwd_kernel writes the dense gradient.  No atomics: the
//     value does not depend on arrival order.  The host never sees n, so a train step keeps its queue full.
//   * reset_opacity (scene/gaussian_model.py:312-315 with replace_tensor_to_optimizer :386-399) in place:
//     raw <- log(c / (1 - c)) with c = min(sigmoid(raw), cap), and the two Adam moments zero-filled, in one launch.
//
// Built with -ffp-contract=off: sigmoid, min, sub, div, log are torch's ops, each rounded to float32 on its own.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "ordered_sum.h"

namespace gsr {

namespace {

constexpr int OPACITY_MAX_BLOCKS = 2048;      // the streaming grid's cap: one float sum and one uint32 count for each
constexpr int OS_THREADS = 256;
constexpr int OS_WAVES = OS_THREADS / WAVE;
constexpr int OS_FIN_THREADS = 256;

// torch's sigmoid kernel: 1 / (1 + exp(-x)) in float
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

struct SparsityAcc {
  float sum;
  uint32_t n;
  __device__ __forceinline__ void add(float raw, float thr) {
    const float o = sigmoid_f32(raw);
    if (o < thr) {
      sum += fabsf(o - 1.0f);
      n += 1u;
    }
  }
};

// VEC: a lane owns 4 consecutive rows (one 16-byte load); the P % 4 tail rows go to the first lanes of block 0.
template <bool VEC>
__global__ __launch_bounds__(OS_THREADS) void opacity_sparsity_kernel(const float* __restrict__ raw, size_t P, float thr,
                                                                      float* __restrict__ part_sum,
                                                                      uint32_t* __restrict__ part_n) {
  __shared__ PairSlots<float, OS_WAVES> red;
  SparsityAcc a = {0.0f, 0u};
  const size_t stride = (size_t)gridDim.x * OS_THREADS;
  const size_t first = (size_t)blockIdx.x * OS_THREADS + threadIdx.x;
  if constexpr (VEC) {
    const size_t items = P / 4;
    for (size_t i = first; i < items; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(raw)[i];
      a.add(v.x, thr); a.add(v.y, thr); a.add(v.z, thr); a.add(v.w, thr);
    }
    const size_t tail = 4 * items + first;                       // first < 4 only in block 0
    if (first < 4 && tail < P) a.add(raw[tail], thr);
  } else {
    for (size_t i = first; i < P; i += stride) a.add(raw[i], thr);
  }
  ordered_pair_sum(a.sum, a.n, red);
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = a.sum;                                // one pair per block: no atomics, see ordered_sum.h
    part_n[blockIdx.x] = a.n;
  }
}

// One block: the pairs in the fixed order of ordered_pair_finish, the float partials widened to double as they are added.
// record = {float loss, uint32 n, float weight / n, 0}; n == 0 gives loss = factor = 0 (train.py:104 skips the term).
__global__ __launch_bounds__(OS_FIN_THREADS) void opacity_sparsity_finish_kernel(const float* __restrict__ part_sum,
                                                                                 const uint32_t* __restrict__ part_n,
                                                                                 int nblocks, float weight,
                                                                                 float* __restrict__ record) {
  __shared__ PairSlots<double, OS_FIN_THREADS / WAVE> red;
  double ts;
  uint32_t tn;
  ordered_pair_finish(part_sum, part_n, nblocks, ts, tn, red);
  if (threadIdx.x != 0) return;
  const double factor = tn ? (double)weight / (double)tn : 0.0;
  record[0] = (float)(factor * ts);
  reinterpret_cast<uint32_t*>(record)[1] = tn;
  record[2] = (float)factor;
  record[3] = 0.0f;
}

// d/d raw of w/n * |o - 1| on the selected rows: g * (w/n) * sign(o - 1) * o * (1 - o); 0 elsewhere
__device__ __forceinline__ float sparsity_grad(float raw, float thr, float scale) {
  const float o = sigmoid_f32(raw);
  if (!(o < thr)) return 0.0f;
  const float d = o - 1.0f;
  const float sgn = (float)((d > 0.0f) - (d < 0.0f));
  return (scale * sgn) * ((1.0f - o) * o);
}

template <bool VEC>
__global__ __launch_bounds__(OS_THREADS) void opacity_sparsity_bwd_kernel(const float* __restrict__ raw, size_t P,
                                                                          float thr, const float* __restrict__ record,
                                                                          const float* __restrict__ grad_out,
                                                                          float* __restrict__ grad_raw) {
  const float scale = grad_out[0] * record[2];                   // both live in device memory: no host read-back
  const size_t stride = (size_t)gridDim.x * OS_THREADS;
  const size_t first = (size_t)blockIdx.x * OS_THREADS + threadIdx.x;
  if constexpr (VEC) {
    const size_t items = P / 4;
    for (size_t i = first; i < items; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(raw)[i];
      reinterpret_cast<float4*>(grad_raw)[i] = make_float4(sparsity_grad(v.x, thr, scale), sparsity_grad(v.y, thr, scale),
                                                           sparsity_grad(v.z, thr, scale), sparsity_grad(v.w, thr, scale));
    }
    const size_t tail = 4 * items + first;
    if (first < 4 && tail < P) grad_raw[tail] = sparsity_grad(raw[tail], thr, scale);
  } else {
    for (size_t i = first; i < P; i += stride) grad_raw[i] = sparsity_grad(raw[i], thr, scale);
  }
}

// inverse_sigmoid(torch.min(sigmoid(raw), cap)) as the reference evaluates it: the uncapped rows make the round trip
// too.  `o > cap ? cap : o` keeps a NaN, as torch.min does.
__device__ __forceinline__ float reset_value(float raw, float cap) {
  const float o = sigmoid_f32(raw);
  const float c = o > cap ? cap : o;
  return logf(c / (1.0f - c));
}

template <bool VEC>
__global__ __launch_bounds__(OS_THREADS) void reset_opacity_kernel(float* __restrict__ raw, size_t P, float cap,
                                                                   float* __restrict__ exp_avg,
                                                                   float* __restrict__ exp_avg_sq) {
  const size_t stride = (size_t)gridDim.x * OS_THREADS;
  const size_t first = (size_t)blockIdx.x * OS_THREADS + threadIdx.x;
  if constexpr (VEC) {
    const size_t items = P / 4;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (size_t i = first; i < items; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(raw)[i];
      reinterpret_cast<float4*>(raw)[i] = make_float4(reset_value(v.x, cap), reset_value(v.y, cap),
                                                      reset_value(v.z, cap), reset_value(v.w, cap));
      if (exp_avg) reinterpret_cast<float4*>(exp_avg)[i] = zero;
      if (exp_avg_sq) reinterpret_cast<float4*>(exp_avg_sq)[i] = zero;
    }
    const size_t tail = 4 * items + first;
    if (first < 4 && tail < P) {
      raw[tail] = reset_value(raw[tail], cap);
      if (exp_avg) exp_avg[tail] = 0.0f;
      if (exp_avg_sq) exp_avg_sq[tail] = 0.0f;
    }
  } else {
    for (size_t i = first; i < P; i += stride) {
      raw[i] = reset_value(raw[i], cap);
      if (exp_avg) exp_avg[i] = 0.0f;
      if (exp_avg_sq) exp_avg_sq[i] = 0.0f;
    }
  }
}

int stream_blocks(size_t P, bool vec) {
  const size_t items = vec ? P / 4 : P;
  const size_t b = (items + OS_THREADS - 1) / OS_THREADS;
  return (int)(b < (size_t)OPACITY_MAX_BLOCKS ? (b ? b : 1) : (size_t)OPACITY_MAX_BLOCKS);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// record: {float loss, uint32 n, float weight / n, 0}
void launch_opacity_sparsity_fwd(const float* raw, size_t P, float weight, float thr, float* record, void* workspace,
                                 hipStream_t s) {
  float* part_sum = static_cast<float*>(workspace);              // [OPACITY_MAX_BLOCKS] sums, then as many counts
  uint32_t* part_n = reinterpret_cast<uint32_t*>(part_sum + OPACITY_MAX_BLOCKS);
  const bool vec = aligned16(raw);
  const int blocks = stream_blocks(P, vec);
  if (vec) hipLaunchKernelGGL((opacity_sparsity_kernel<true>), dim3(blocks), dim3(OS_THREADS), 0, s, raw, P, thr, part_sum, part_n);
  else hipLaunchKernelGGL((opacity_sparsity_kernel<false>), dim3(blocks), dim3(OS_THREADS), 0, s, raw, P, thr, part_sum, part_n);
  hipLaunchKernelGGL(opacity_sparsity_finish_kernel, dim3(1), dim3(OS_FIN_THREADS), 0, s, part_sum, part_n, blocks, weight,
                     record);
}

void launch_opacity_sparsity_bwd(const float* raw, size_t P, float thr, const float* record, const float* grad_out,
                                 float* grad_raw, hipStream_t s) {
  const bool vec = aligned16(raw) && aligned16(grad_raw);
  const int blocks = stream_blocks(P, vec);
  if (vec) hipLaunchKernelGGL((opacity_sparsity_bwd_kernel<true>), dim3(blocks), dim3(OS_THREADS), 0, s, raw, P, thr, record, grad_out, grad_raw);
  else hipLaunchKernelGGL((opacity_sparsity_bwd_kernel<false>), dim3(blocks), dim3(OS_THREADS), 0, s, raw, P, thr, record, grad_out, grad_raw);
}

void launch_reset_opacity(float* raw, size_t P, float cap, float* exp_avg, float* exp_avg_sq, hipStream_t s) {
  const bool vec = aligned16(raw) && aligned16(exp_avg) && aligned16(exp_avg_sq);      // NULL counts as aligned
  const int blocks = stream_blocks(P, vec);
  if (vec) hipLaunchKernelGGL((reset_opacity_kernel<true>), dim3(blocks), dim3(OS_THREADS), 0, s, raw, P, cap, exp_avg, exp_avg_sq);
  else hipLaunchKernelGGL((reset_opacity_kernel<false>), dim3(blocks), dim3(OS_THREADS), 0, s, raw, P, cap, exp_avg, exp_avg_sq);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_opacity_sparsity_workspace_bytes(void) { return (size_t)OPACITY_MAX_BLOCKS * (sizeof(float) + sizeof(uint32_t)); }
int gsr_opacity_sparsity_fwd(const float* opacity_raw, int64_t P, float weight, float threshold, float* record,
                             void* workspace, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "negative P");
  if (!record || !workspace || (P > 0 && !opacity_raw)) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({opacity_raw, workspace}, 3u) || !aligned({record}, 15u))
    return fail(GSR_E_ALIGN, "opacity and workspace must be 4-byte aligned, the record 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_opacity_sparsity_fwd(opacity_raw, (size_t)P, weight, threshold, record, workspace, s);
  return check(false, s, "opacity_sparsity_fwd");
}
int gsr_opacity_sparsity_bwd(const float* opacity_raw, int64_t P, float threshold, const float* record,
                             const float* grad_out, float* grad_raw, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "negative P");
  if (!record || !grad_out || (P > 0 && (!opacity_raw || !grad_raw))) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({opacity_raw, grad_raw, record, grad_out}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_opacity_sparsity_bwd(opacity_raw, (size_t)P, threshold, record, grad_out, grad_raw, s);
  return check(false, s, "opacity_sparsity_bwd");
}
int gsr_reset_opacity(float* opacity_raw, int64_t P, float cap, float* exp_avg, float* exp_avg_sq, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "negative P");
  if (P > 0 && !opacity_raw) return fail(GSR_E_BADARG, "NULL opacity");
  if (!(cap > 0.0f && cap < 1.0f)) return fail(GSR_E_BADARG, "cap must lie in (0, 1)");
  if (!aligned({opacity_raw, exp_avg, exp_avg_sq}, 3u)) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_reset_opacity(opacity_raw, (size_t)P, cap, exp_avg, exp_avg_sq, s);
  return check(false, s, "reset_opacity");
}

}  // extern "C"
