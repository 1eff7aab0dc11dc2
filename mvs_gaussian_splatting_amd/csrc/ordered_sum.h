// The one deterministic workgroup sum of the loss and statistic kernels (loss.hip, masked_loss.hip, mvs_loss.hip,
// mvs_ncc.hip, normal_consistency.hip, model.hip, icp.hip, depth_prior.hip, exposure.hip, bilagrid.hip, aux.hip).
//
// The rule, owned HERE: every wave adds its 64 lanes with the xor butterfly, distance WAVE/2 down to 1 (a lane's
// partners are fixed); lane 0 of every wave leaves the wave's sum in the wave's slot in LDS; after ONE barrier a fixed
// lane adds the slots in ascending wave order.  No atomics.  The order of every addition is a function of the launch
// shape alone, so a sum is the same bits from run to run.  The header holds additions only and no pragma about
// contraction: it gives the same bits in a unit built with -ffp-contract=off and in one built without.
//
// Every lane of the workgroup must reach a call (none may sit under a lane-dependent branch): the butterfly reads all 64
// lanes and the one-call forms hold a __syncthreads().  The slots are the caller's LDS, WAVES = workgroup lanes / 64.
//
// Split form.  ordered_stage* is the part before the barrier, ordered_fold* the part behind it, for a kernel that has
// more to put into LDS before its own barrier (normal_consistency_kernel); the one-call forms are stage, barrier, fold.
//
// Where the walk over the slots starts.  FROM_ZERO: s = +0, then += every slot.  FROM_WAVE0: s = wave 0's slot, then +=
// the others.  The two differ only when every slot is -0.0 (+0 + -0 is +0).  An accumulator that starts at +0.0 and is
// only added to never becomes -0.0, but some sites reduce a value a lane computed directly (the SSIM tile kernels'
// s and m (1 - s): a -0.0 mask gives -0.0 in every lane), so each site keeps the start it always had.  The pair form is
// FROM_ZERO throughout; normal_consistency_kernel's e = alpha - dot is loaded with alpha >= alpha_min > 0 and so is
// never -0.0 either way.
#pragma once
#include "gsr_common.h"

namespace gsr {

enum OrderedStart { FROM_ZERO, FROM_WAVE0 };

template <typename T>
__device__ inline T wave_butterfly_add(T v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, WAVE);
  return v;
}

// slot[0] + slot[stride] + ... over WAVES slots, in that order
template <int WAVES, OrderedStart START, typename T>
__device__ inline T ordered_walk(const T* slot, int stride) {
  T s = START == FROM_ZERO ? T(0) : slot[0];
#pragma unroll
  for (int w = START == FROM_ZERO ? 0 : 1; w < WAVES; ++w) s += slot[w * stride];
  return s;
}

// ---- a vector of NV values of type T (float or double): the sums are valid in thread 0 ------------------------------
template <int NV, typename T>
__device__ inline void ordered_stage(T (&v)[NV], T (*slot)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = wave_butterfly_add(v[k]);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) slot[threadIdx.x / WAVE][k] = v[k];
  }
}

template <int WAVES, OrderedStart START, int NV, typename T>
__device__ inline void ordered_block_sum(T (&v)[NV], T (*slot)[NV]) {
  ordered_stage(v, slot);
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = ordered_walk<WAVES, START>(&slot[0][k], NV);
  }
}

// one value
template <int WAVES, OrderedStart START, typename T>
__device__ inline T ordered_block_sum(T value, T* slot) {
  T v[1] = {value};
  ordered_block_sum<WAVES, START>(v, reinterpret_cast<T(*)[1]>(slot));
  return v[0];
}

// the same vector with value k folded by lane k: returns the sum of value threadIdx.x in lanes 0..NV-1, T(0) elsewhere
template <int WAVES, int NV, typename T>
__device__ inline T ordered_block_sum_by_lane(T (&v)[NV], T (*slot)[NV]) {
  static_assert(NV <= WAVE, "lanes 0..NV-1 of the first wave fold the values");
  ordered_stage(v, slot);
  __syncthreads();
  return threadIdx.x < NV ? ordered_walk<WAVES, FROM_WAVE0>(&slot[0][threadIdx.x], NV) : T(0);
}

// ---- a (sum, count) pair: valid in thread 0 -------------------------------------------------------------------------
template <typename T, int WAVES>
struct PairSlots {
  T s[WAVES];
  uint32_t n[WAVES];
};

template <typename T, int WAVES>
__device__ inline void ordered_pair_stage(T s, uint32_t n, PairSlots<T, WAVES>& slot) {
  s = wave_butterfly_add(s);
  n = wave_butterfly_add(n);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    slot.s[threadIdx.x / WAVE] = s;
    slot.n[threadIdx.x / WAVE] = n;
  }
}

// behind the barrier, in thread 0
template <typename T, int WAVES>
__device__ inline void ordered_pair_fold(const PairSlots<T, WAVES>& slot, T& s, uint32_t& n) {
  s = ordered_walk<WAVES, FROM_ZERO>(slot.s, 1);
  n = ordered_walk<WAVES, FROM_ZERO>(slot.n, 1);
}

template <typename T, int WAVES>
__device__ inline void ordered_pair_sum(T& s, uint32_t& n, PairSlots<T, WAVES>& slot) {
  ordered_pair_stage(s, n, slot);
  __syncthreads();
  if (threadIdx.x == 0) ordered_pair_fold(slot, s, n);
}

// The finish side, ONE workgroup of 64 WAVES lanes: lane t adds the pairs t, t + 64 WAVES, ... in ascending order, a
// partial of type P widened to double as it is added, then the block sum.
template <typename P, typename I, int WAVES>
__device__ inline void ordered_pair_finish(const P* __restrict__ part_sum, const uint32_t* __restrict__ part_n, I nblocks,
                                           double& s, uint32_t& n, PairSlots<double, WAVES>& slot) {
  s = 0.0;
  n = 0u;
  for (I i = threadIdx.x; i < nblocks; i += WAVES * WAVE) {
    s += (double)part_sum[i];
    n += part_n[i];
  }
  ordered_pair_sum(s, n, slot);
}

// ---- words: an int64 count and NS doubles, word k (the count is word 0) folded by lane k ----------------------------
template <int NS>
struct CountSums {
  long long n;
  double s[NS];
  __device__ inline void zero() {
    n = 0;
    for (int k = 0; k < NS; ++k) s[k] = 0.0;
  }
};

// Returns word threadIdx.x of the workgroup's sum in lanes 0..NS (the count as the bits of an int64, a sum as the bits of
// a double), 0 elsewhere.
template <int WAVES, int NS>
__device__ inline unsigned long long ordered_block_words(CountSums<NS>& acc, unsigned long long (*slot)[1 + NS]) {
  static_assert(1 + NS <= WAVE, "lanes 0..NS of the first wave fold the words");
  for (int d = WAVE / 2; d > 0; d >>= 1) {      // all words a distance at a time: word by word costs 16 more VGPRs at NS = 17
    acc.n += __shfl_xor(acc.n, d, WAVE);
    for (int k = 0; k < NS; ++k) acc.s[k] += __shfl_xor(acc.s[k], d, WAVE);
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    const int wave = threadIdx.x / WAVE;
    slot[wave][0] = (unsigned long long)acc.n;
    for (int k = 0; k < NS; ++k) slot[wave][1 + k] = (unsigned long long)__double_as_longlong(acc.s[k]);
  }
  __syncthreads();
  unsigned long long word = 0;
  if (threadIdx.x == 0) {                       // FROM_WAVE0, on the words' own types
    long long n = (long long)slot[0][0];
    for (int w = 1; w < WAVES; ++w) n += (long long)slot[w][0];
    word = (unsigned long long)n;
  } else if (threadIdx.x < 1 + NS) {
    double v = __longlong_as_double((long long)slot[0][threadIdx.x]);
    for (int w = 1; w < WAVES; ++w) v += __longlong_as_double((long long)slot[w][threadIdx.x]);
    word = (unsigned long long)__double_as_longlong(v);
  }
  return word;
}

// The finish side: the partials of `nb` workgroups, laid out partials[word * stride_words + g], added per word, lane t
// taking g = t, t + TRIP, ... in ascending order.
template <int TRIP, int NS>
__device__ inline void ordered_read_words(CountSums<NS>& acc, const unsigned long long* __restrict__ partials, int nb,
                                          int stride_words) {
  acc.zero();
  for (int g = threadIdx.x; g < nb; g += TRIP) {
    acc.n += (long long)partials[g];
    for (int k = 0; k < NS; ++k) acc.s[k] += __longlong_as_double((long long)partials[(size_t)(1 + k) * stride_words + g]);
  }
}

}  // namespace gsr
