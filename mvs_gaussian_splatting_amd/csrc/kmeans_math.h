// The assignment rule of csrc/kmeans.hip (compress.kmeans_assign / kmeans), written once for device and
// host: tests/kmeans_host_check.cpp builds it with the host compiler and the kernel's -ffp-contract=off, so the chosen
// index and dist2 are checked against the numpy restatement (tests/kmeans_restate.py) without a GPU.
//
// For a point x[D] and a code c[D], both padded to an even D by zeros (a padded step is fmaf(0, 0, acc) = acc):
//   dot   = fmaf(x[D-1], c[D-1], ... fmaf(x[1], c[1], fmaf(x[0], c[0], 0.0f)) ...)
//   cnorm = the same chain of c with itself
//   score = fmaf(-2.0f, dot, cnorm)
// The assignment of x is the code with the smallest score; of equal scores the smallest index wins (a code is taken only
// when its score is < the best so far, walking the codes in ascending index from (+inf, 0)).  |x|^2 is left out: it does
// not change the argmin.  dist2 = max(0, xnorm + score), xnorm the chain of x with itself and the sum one float32 add:
// a diagnostic, not part of the rule.
//
// The matrix-core path forms `dot` with v_mfma_f32_32x32x2_f32, whose accumulator is bit for bit this k-ordered chain
// (two steps of it per instruction), so the bits do not depend on the path.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif

namespace gsr {

constexpr int KMEANS_MAX_D = 64;
constexpr int KMEANS_MAX_K = 65536;

// fmaf(a[n-1], b[n-1], ... fmaf(a[0], b[0], 0.0f))
GSR_HD float kmeans_chain(const float* a, const float* b, int n) {
  float acc = 0.0f;
  for (int k = 0; k < n; ++k) acc = __builtin_fmaf(a[k], b[k], acc);
  return acc;
}

GSR_HD float kmeans_score(float dot, float cnorm) { return __builtin_fmaf(-2.0f, dot, cnorm); }

// one step of the running minimum: codes arrive in ascending index, so '<' keeps the smallest index of equal scores
GSR_HD void kmeans_take(float score, int32_t index, float* best, int32_t* best_index) {
  if (score < *best) {
    *best = score;
    *best_index = index;
  }
}

// the merge of two running minima over disjoint sets of codes
GSR_HD void kmeans_merge(float score, int32_t index, float* best, int32_t* best_index) {
  if (score < *best || (score == *best && index < *best_index)) {
    *best = score;
    *best_index = index;
  }
}

GSR_HD float kmeans_dist2(float xnorm, float score) {
  const float d = xnorm + score;
  return d > 0.0f ? d : 0.0f;         // a NaN (inf - inf) gives 0 as well
}

// the whole rule for one point, the way a single lane walks it
GSR_HD int32_t kmeans_assign_point(const float* x, const float* codebook, const float* cnorm, int32_t K, int D,
                                   float* best_score) {
  float best = __builtin_inff();
  int32_t bi = 0;
  for (int32_t c = 0; c < K; ++c)
    kmeans_take(kmeans_score(kmeans_chain(x, codebook + (int64_t)c * D, D), cnorm[c]), c, &best, &bi);
  *best_score = best;
  return bi;
}

}  // namespace gsr
