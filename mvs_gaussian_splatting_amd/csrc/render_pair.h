// The (instance, pixel) alpha of the compositing kernels: the staged record, its LDS image and the evaluation.  One
// definition for every translation unit that must take the colour pass's alpha >= 1/255 decisions bit for bit
// (render.hip; depth.hip, whose maps are sums of the same weights).
#pragma once
#include "gsr_common.h"

namespace gsr {

constexpr float LOG2E = 1.4426950408889634f;

// What one lane fetches for the instance it stages (GeomRec words 0..10, 14..15 and, for the backward, 11..13).
struct Staged {
  float4 q0, q1, q2;
  float kk, isyy;
  uint32_t rect_min, rect_wh, slot_base;
};

// LDS image of a staged instance.  The quadratic form is kept as a completed square, pre-scaled by log2(e) so that
// the exponential is a bare v_exp_f32:
//    log2(e) * power = nka * u^2 + nkd * dy^2,   u = dx + kk * dy,   (dx, dy) = mean - pixel,
//    nka = -0.5 log2e cxx,  kk = cxy / cxx,  nkd = -0.5 log2e / cov_yy.
// Both terms are <= 0 in float32 whatever the rounding, so the reference's "power > 0 -> skip" guard (Appendix A.4)
// can never fire -- it only ever fired on rounding noise of the expanded form -- and costs no compare here.
// The opacity rides in the exponent: alpha = opacity * exp(power) = exp2(log2(opacity) + log2e * power) -- the addend
// of a multiply that becomes an fma, one instruction less per pair than the product (v_log_f32 is good to an ulp, the
// sum is at most ~8 in magnitude: alpha moves by < 5e-7 relative).
// Whether an instance can reach the 0.99 clamp (opacity > 0.99; alpha <= opacity otherwise, to the ulp of v_log / v_exp)
// rides in the SIGN of the stored nkd: the evaluation takes -|nkd| (source modifiers: free), the clamped copies of the
// walks read the sign.  The clamp is thus a property of the INSTANCE: which copy of a walk runs depends on what else
// shares the round (256 instances in the forward, 64 in the backward), and an instance must get the same alpha in both
// kernels whatever its neighbours are.
struct LdsRec {
  float4 A;   // x, y, nka, kk
  float4 B;   // +-|nkd| (+: opacity > 0.99), log2(opacity), r, g
};
__device__ inline void make_lds(const Staged& st, LdsRec& o) {
  // -|cxx|: a covariance whose float32 determinant came out negative (a needle thousands of pixels long) yields a
  // negative conic; upstream's power > 0 guard drops most pairs of such a splat, here it composes with |cxx| instead.
  // What matters is that alpha stays <= opacity: an alpha above 1 would un-park a saturated pixel (T (1 - alpha) > 0)
  o.A = make_float4(st.q0.x, st.q0.y, (-0.5f * LOG2E) * fabsf(st.q0.z), st.kk);
  const float nkd_abs = (0.5f * LOG2E) * fabsf(st.isyy);
  o.B = make_float4(st.q1.y > ALPHA_MAX ? nkd_abs : -nkd_abs, __builtin_amdgcn_logf(st.q1.y), st.q1.z, st.q1.w);
}
__device__ __forceinline__ float clamp_alpha(float alpha, float nkd_signed) {
  return nkd_signed > 0.0f ? fminf(ALPHA_MAX, alpha) : alpha;
}
// log2(alpha before the clamp).  The same five operations in the forward and in the backward: both must take the same
// alpha >= 1/255 decisions
__device__ __forceinline__ float pair_p2(float dx, float dy, float nka, float kk, float nkd_signed, float lo) {
#pragma clang fp contract(off)
  const float u = __builtin_fmaf(kk, dy, dx);
  const float s = nka * u;
  const float v = __builtin_fmaf(-fabsf(nkd_signed) * dy, dy, lo);
  return __builtin_fmaf(s, u, v);
}

}  // namespace gsr
