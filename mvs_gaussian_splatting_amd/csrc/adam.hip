// One Adam step for every parameter group of the Gaussian model in one launch (gsr_adam_step, include/gsr.h), and the
// same step for the rows a frame saw only (gsr_adam_step_rows, below).
//
// The reference steps its optimizer with torch.optim.Adam(l, lr=0.0, eps=1e-15) (scene/gaussian_model.py:264), which
// torch runs as `_multi_tensor_adam`: about eight `_foreach_*` passes over every parameter and moment tensor.  Here
// each element is read once and written once: 28 bytes (grad, param, exp_avg, exp_avg_sq in; the last three out).
//
//   grid   : fixed chunks of ADAM_CHUNK elements, the chunks of tensor 0 first; a block finds its tensor by a uniform
//            scan of the chunk prefixes held in the kernel argument (<= GSR_ADAM_MAX_TENSORS entries, no table in
//            memory)
//   access : full chunks of a tensor whose four arrays are 16-byte aligned take 16-byte loads / stores (the gradient
//            with a non-temporal load: it is read once); the last, partial chunk and unaligned tensors go per element
//   values : torch's foreach ops one by one, each rounded to float32 (see adam_update); no LDS, no atomics
#include "gsr_common.h"
#include "gsr_entry.h"

namespace gsr {

namespace {

constexpr int ADAM_BLOCK = 256;
constexpr int ADAM_VECS = 4;                                     // float4 per thread per chunk
constexpr int64_t ADAM_CHUNK = (int64_t)ADAM_BLOCK * ADAM_VECS * 4;  // 4096 elements

typedef float f4 __attribute__((ext_vector_type(4)));

struct AdamLaunch {
  GsrAdamTensor t[GSR_ADAM_MAX_TENSORS];
  uint32_t first_chunk[GSR_ADAM_MAX_TENSORS];                    // exclusive prefix of the tensors' chunk counts
  uint32_t vec_mask;                                             // bit k: tensor k's four arrays are 16-byte aligned
  int32_t count;
};

struct AdamScalars {
  float w, one_minus_w, beta2, sq_w, bc2_sqrt, eps, step_size;
  bool small;
};

__device__ __forceinline__ AdamScalars adam_scalars(const GsrAdamTensor& t) {
  AdamScalars s;
  s.w = t.lerp_weight;
  s.one_minus_w = 1.0f - t.lerp_weight;                          // Lerp.h: opmath_t(1) - weight, in float
  s.small = fabsf(t.lerp_weight) < 0.5f;                         // is_lerp_weight_small
  s.beta2 = t.beta2;
  s.sq_w = t.sq_weight;
  s.bc2_sqrt = t.bc2_sqrt;
  s.eps = t.eps;
  s.step_size = t.step_size;
  return s;
}

// torch's foreach functors (ATen/native/hip/ForeachFunctors.cuh, Lerp.h) evaluate `a + s * x` and the lerp's
// `self + w * (end - self)` / `end - (end - self) * (1 - w)` in float, and torch's kernels contract each of them into one
// fused multiply-add: against torch.optim.Adam on the MI355X these three lines as FMAs give equal bits for params and
// both moments, and as a rounded multiply then add they differ (exp_avg on ~27 % of the elements from the second step
// on; profiles/adam/NOTES.md).  Every other op is its own rounded float op: this file is compiled with
// -ffp-contract=off, so only the explicit __builtin_fmaf calls fuse.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamScalars& s) {
  const float diff = g - m;                                      // _foreach_lerp_(exp_avgs, grads, 1 - beta1)
  m = s.small ? __builtin_fmaf(s.w, diff, m) : __builtin_fmaf(-diff, s.one_minus_w, g);
  v = v * s.beta2;                                               // _foreach_mul_(exp_avg_sqs, beta2)
  v = __builtin_fmaf(s.sq_w, g * g, v);                          // _foreach_addcmul_(.., grads, grads, 1 - beta2)
  float d = __builtin_sqrtf(v);                                  // _foreach_sqrt (correctly rounded)
  d = d / s.bc2_sqrt;                                            // _foreach_div_(.., bias_correction2_sqrt)
  d = d + s.eps;                                                 // _foreach_add_(.., eps)
  p = __builtin_fmaf(s.step_size, m / d, p);                     // _foreach_addcdiv_(params, exp_avgs, d, step_size)
}

__global__ __launch_bounds__(ADAM_BLOCK) void adam_step_kernel(const AdamLaunch L) {
  const uint32_t b = blockIdx.x;
  int k = 0;
#pragma unroll
  for (int i = 1; i < GSR_ADAM_MAX_TENSORS; ++i)
    if (i < L.count && b >= L.first_chunk[i]) k = i;             // uniform: the last tensor whose chunks start <= b
  const GsrAdamTensor& T = L.t[k];
  const AdamScalars s = adam_scalars(T);
  const int64_t base = (int64_t)(b - L.first_chunk[k]) * ADAM_CHUNK;
  const int64_t len = T.numel - base < ADAM_CHUNK ? T.numel - base : ADAM_CHUNK;
  float* __restrict__ P = T.param + base;
  const float* __restrict__ G = T.grad + base;
  float* __restrict__ M = T.exp_avg + base;
  float* __restrict__ V = T.exp_avg_sq + base;
  if (len == ADAM_CHUNK && ((L.vec_mask >> k) & 1u)) {
    f4 p[ADAM_VECS], g[ADAM_VECS], m[ADAM_VECS], v[ADAM_VECS];
#pragma unroll
    for (int j = 0; j < ADAM_VECS; ++j) {
      const int i = threadIdx.x + j * ADAM_BLOCK;
      g[j] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(G) + i);
      p[j] = reinterpret_cast<const f4*>(P)[i];
      m[j] = reinterpret_cast<const f4*>(M)[i];
      v[j] = reinterpret_cast<const f4*>(V)[i];
    }
#pragma unroll
    for (int j = 0; j < ADAM_VECS; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float pe = p[j][e], me = m[j][e], ve = v[j][e];
        adam_update(pe, g[j][e], me, ve, s);
        p[j][e] = pe;
        m[j][e] = me;
        v[j][e] = ve;
      }
      const int i = threadIdx.x + j * ADAM_BLOCK;
      reinterpret_cast<f4*>(P)[i] = p[j];
      reinterpret_cast<f4*>(M)[i] = m[j];
      reinterpret_cast<f4*>(V)[i] = v[j];
    }
  } else {
    for (int i = threadIdx.x; i < len; i += ADAM_BLOCK) {
      float p = P[i], m = M[i], v = V[i];
      adam_update(p, __builtin_nontemporal_load(G + i), m, v, s);
      P[i] = p;
      M[i] = m;
      V[i] = v;
    }
  }
}

// ---- the row-masked step (gsr_adam_step_rows) ----------------------------------------------------------------------
// The same grid, chunks and access shapes as adam_step_kernel; a tensor is [rows, row_floats] and only the elements of
// rows the visibility array marks get adam_update.  The point is bytes: a lane whose 16-byte piece (or element) lies in
// invisible rows only issues no load or store, so whole 128-byte stretches of invisible rows never leave HBM.  A piece
// that straddles a visible and an invisible row is loaded and written back whole, the invisible elements with the bits
// they came with.
struct AdamRowsLaunch {
  AdamLaunch a;
  int64_t row_floats[GSR_ADAM_MAX_TENSORS];
  const void* visibility;                                        // [rows]: uint8 (non-zero) or int32 (> 0) = visible
};

// Where the elements of one chunk lie in their tensor's rows.  The chunk's first element is divided once, in 64 bits
// and uniformly; an element `off` (< ADAM_CHUNK) further on then needs a 32-bit division at most, of a value below
// 2 * ADAM_CHUNK.  Rows longer than a chunk meet a chunk in at most two rows: a compare.  Exact for every row_floats.
struct RowCursor {
  int64_t row0;                                                  // row of the chunk's first element
  uint64_t rem0;                                                 // its offset in that row
  uint64_t rf;
  bool wide;                                                     // rf > ADAM_CHUNK

  __device__ __forceinline__ RowCursor(int64_t base, int64_t row_floats) {
    rf = (uint64_t)row_floats;
    row0 = (int64_t)((uint64_t)base / rf);
    rem0 = (uint64_t)base - (uint64_t)row0 * rf;
    wide = rf > (uint64_t)ADAM_CHUNK;
  }
  __device__ __forceinline__ void locate(uint32_t off, int64_t& row, uint64_t& rem) const {
    if (wide) {
      const uint64_t q = rem0 + off;                             // < 2 * rf
      const bool next = q >= rf;
      row = row0 + (next ? 1 : 0);
      rem = next ? q - rf : q;
    } else {
      const uint32_t q = (uint32_t)rem0 + off, d = q / (uint32_t)rf;
      row = row0 + d;
      rem = q - d * (uint32_t)rf;
    }
  }
};

template <typename VisT>
__global__ __launch_bounds__(ADAM_BLOCK) void adam_step_rows_kernel(const AdamRowsLaunch R) {
  const AdamLaunch& L = R.a;
  const uint32_t b = blockIdx.x;
  int k = 0;
#pragma unroll
  for (int i = 1; i < GSR_ADAM_MAX_TENSORS; ++i)
    if (i < L.count && b >= L.first_chunk[i]) k = i;             // uniform: the last tensor whose chunks start <= b
  const GsrAdamTensor& T = L.t[k];
  const AdamScalars s = adam_scalars(T);
  const int64_t base = (int64_t)(b - L.first_chunk[k]) * ADAM_CHUNK;
  const int64_t len = T.numel - base < ADAM_CHUNK ? T.numel - base : ADAM_CHUNK;
  const RowCursor cur(base, R.row_floats[k]);
  const VisT* __restrict__ vis = static_cast<const VisT*>(R.visibility);
  float* __restrict__ P = T.param + base;
  const float* __restrict__ G = T.grad + base;
  float* __restrict__ M = T.exp_avg + base;
  float* __restrict__ V = T.exp_avg_sq + base;
  if (len == ADAM_CHUNK && ((L.vec_mask >> k) & 1u)) {
    uint32_t seen = 0;                                           // bit 4 j + e: element e of piece j is in a visible row
#pragma unroll
    for (int j = 0; j < ADAM_VECS; ++j) {
      int64_t row;
      uint64_t rem;
      cur.locate(4u * (threadIdx.x + j * ADAM_BLOCK), row, rem);
      int64_t at = -1;
      bool on = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {                              // rem + e < rf + 3 <= 4 rf: at most three row ends
        const uint64_t q = rem + e;
        const int64_t r = row + (q >= cur.rf ? 1 : 0) + (q >= 2 * cur.rf ? 1 : 0) + (q >= 3 * cur.rf ? 1 : 0);
        if (r != at) {                                           // one visibility read per row the piece meets
          on = vis[r] > 0;
          at = r;
        }
        seen |= (on ? 1u : 0u) << (4 * j + e);
      }
    }
    f4 p[ADAM_VECS] = {}, g[ADAM_VECS] = {}, m[ADAM_VECS] = {}, v[ADAM_VECS] = {};
#pragma unroll
    for (int j = 0; j < ADAM_VECS; ++j) {
      if ((seen >> (4 * j)) & 15u) {
        const int i = threadIdx.x + j * ADAM_BLOCK;
        g[j] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(G) + i);
        p[j] = reinterpret_cast<const f4*>(P)[i];
        m[j] = reinterpret_cast<const f4*>(M)[i];
        v[j] = reinterpret_cast<const f4*>(V)[i];
      }
    }
#pragma unroll
    for (int j = 0; j < ADAM_VECS; ++j) {
      if ((seen >> (4 * j)) & 15u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float pe = p[j][e], me = m[j][e], ve = v[j][e];
          adam_update(pe, g[j][e], me, ve, s);
          const bool on = (seen >> (4 * j + e)) & 1u;            // a select moves bits: the elements of an invisible
          p[j][e] = on ? pe : p[j][e];                           // row go back as they came, whatever the update made
          m[j][e] = on ? me : m[j][e];                           // of their gradient
          v[j][e] = on ? ve : v[j][e];
        }
        const int i = threadIdx.x + j * ADAM_BLOCK;
        reinterpret_cast<f4*>(P)[i] = p[j];
        reinterpret_cast<f4*>(M)[i] = m[j];
        reinterpret_cast<f4*>(V)[i] = v[j];
      }
    }
  } else {
    for (int i = threadIdx.x; i < len; i += ADAM_BLOCK) {
      int64_t row;
      uint64_t rem;
      cur.locate((uint32_t)i, row, rem);
      if (vis[row] > 0) {
        float p = P[i], m = M[i], v = V[i];
        adam_update(p, __builtin_nontemporal_load(G + i), m, v, s);
        P[i] = p;
        M[i] = m;
        V[i] = v;
      }
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// one launch over the batch's tensors; returns nonzero (nothing enqueued) if the grid would exceed 2^32 work-items
int launch_adam_step(const GsrAdamBatch& batch, hipStream_t s) {
  AdamLaunch L = {};
  L.count = batch.count;
  uint64_t chunks = 0;
  for (int k = 0; k < batch.count; ++k) {
    const GsrAdamTensor& t = batch.t[k];
    L.t[k] = t;
    L.first_chunk[k] = (uint32_t)chunks;
    chunks += (uint64_t)((t.numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
    if (chunks * ADAM_BLOCK > 0xffffffffull) return 1;          // grid of more than 2^32 work-items
    if (aligned16(t.param) && aligned16(t.grad) && aligned16(t.exp_avg) && aligned16(t.exp_avg_sq))
      L.vec_mask |= 1u << k;
  }
  if (chunks == 0) return 0;
  adam_step_kernel<<<dim3((uint32_t)chunks), dim3(ADAM_BLOCK), 0, s>>>(L);
  return 0;
}

// the row-masked step; the caller has checked that rows > 0 divides the numel of every non-empty entry
int launch_adam_step_rows(const GsrAdamRowsBatch& batch, hipStream_t s) {
  AdamRowsLaunch R = {};
  AdamLaunch& L = R.a;
  L.count = batch.count;
  R.visibility = batch.visibility;
  uint64_t chunks = 0;
  for (int k = 0; k < batch.count; ++k) {
    const GsrAdamTensor& t = batch.t[k];
    L.t[k] = t;
    R.row_floats[k] = t.numel > 0 ? t.numel / batch.rows : 1;   // the caller has checked rows > 0 and the remainder
    L.first_chunk[k] = (uint32_t)chunks;
    chunks += (uint64_t)((t.numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
    if (chunks * ADAM_BLOCK > 0xffffffffull) return 1;          // grid of more than 2^32 work-items
    if (aligned16(t.param) && aligned16(t.grad) && aligned16(t.exp_avg) && aligned16(t.exp_avg_sq))
      L.vec_mask |= 1u << k;
  }
  if (chunks == 0) return 0;
  if (batch.visibility_kind == GSR_ADAM_VIS_I32)
    adam_step_rows_kernel<int32_t><<<dim3((uint32_t)chunks), dim3(ADAM_BLOCK), 0, s>>>(R);
  else
    adam_step_rows_kernel<uint8_t><<<dim3((uint32_t)chunks), dim3(ADAM_BLOCK), 0, s>>>(R);
  return 0;
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_adam_step(const GsrAdamBatch* batch, void* stream) {
  if (!batch) return fail(GSR_E_BADARG, "NULL batch");
  if (batch->count < 0 || batch->count > GSR_ADAM_MAX_TENSORS)
    return fail(GSR_E_BADARG, "count must be 0..GSR_ADAM_MAX_TENSORS");
  for (int k = 0; k < batch->count; ++k) {
    const GsrAdamTensor& t = batch->t[k];
    if (t.numel < 0) return fail(GSR_E_BADARG, "negative numel");
    if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))
      return fail(GSR_E_BADARG, "NULL param / grad / exp_avg / exp_avg_sq");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (launch_adam_step(*batch, s)) return fail(GSR_E_BADARG, "batch too large for one launch (more than 2^32 work-items)");
  return check(false, s, "adam_step");
}

int gsr_adam_step_rows(const GsrAdamRowsBatch* batch, void* stream) {
  if (!batch) return fail(GSR_E_BADARG, "NULL batch");
  if (batch->count < 0 || batch->count > GSR_ADAM_MAX_TENSORS)
    return fail(GSR_E_BADARG, "count must be 0..GSR_ADAM_MAX_TENSORS");
  if (batch->visibility_kind != GSR_ADAM_VIS_U8 && batch->visibility_kind != GSR_ADAM_VIS_I32)
    return fail(GSR_E_BADARG, "unknown visibility_kind");
  if (batch->rows < 0) return fail(GSR_E_BADARG, "negative rows");
  for (int k = 0; k < batch->count; ++k) {
    const GsrAdamTensor& t = batch->t[k];
    if (t.numel < 0) return fail(GSR_E_BADARG, "negative numel");
    if (t.numel == 0) continue;
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)
      return fail(GSR_E_BADARG, "NULL param / grad / exp_avg / exp_avg_sq");
    if (!batch->visibility) return fail(GSR_E_BADARG, "NULL visibility with a non-empty tensor");
    if (batch->rows == 0 || t.numel % batch->rows != 0) return fail(GSR_E_BADARG, "numel is not a multiple of rows");
  }
  if (batch->visibility_kind == GSR_ADAM_VIS_I32 && !aligned({batch->visibility}, 3u))
    return fail(GSR_E_ALIGN, "an int32 visibility must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (launch_adam_step_rows(*batch, s))
    return fail(GSR_E_BADARG, "batch too large for one launch (more than 2^32 work-items)");
  return check(false, s, "adam_step_rows");
}

}  // extern "C"
