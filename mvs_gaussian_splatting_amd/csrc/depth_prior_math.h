// The per-pixel arithmetic and the fit of csrc/depth_prior.hip (depth_prior.py), written once for device
// and host: tests/depth_prior_host_check.cpp builds it with the host compiler and the kernel's -ffp-contract=off, so the
// fit from given sums and the per-pixel gradients are checked against numpy's float64 (tests/depth_prior_restate.py)
// without a GPU.  Everything is float64 from the float32 values widened exactly, every operation rounded on its own (no
// fused multiply-add), and a gradient is rounded ONCE to float32.
//
// A pixel (x rendered, y prior, w weight; w = 1 without a weight map) is VALID when w > 0, w is finite, and x and y are
// finite.  An invalid pixel has no term anywhere and gradient +0.
//
// Terms of a valid pixel, in the order of the sums Sw, Sx, Sy, Sxx, Sxy, Syy: w, wx = w x, wy = w y, wx x, wx y, wy y.
//
// Fit from the count n and the six sums:
//   mx = Sx / Sw, my = Sy / Sw, ex = Sxx / Sw, ey = Syy / Sw, vx = ex - mx mx, vy = ey - my my, cov = Sxy / Sw - mx my
//   degenerate when n < 2, or not Sw > 0, or not vx > 2^-40 ex, or not vy > 2^-40 ey (a NaN anywhere lands here too)
//   sd = sqrt(vx vy), s = cov / vy, t = mx - s my, r = cov / sd;  degenerate: s = 1, t = 0, r = 0, sd = 0
//
// Gradients (the unit gradient dL/dx of a valid pixel):
//   the L1 modes   e = x - (a y + b), g = (w sign(e)) / D with sign(0) = 0; (a, b, D) = (scale, offset, H W) or (s, t, Sw)
//   pearson        A = (w / Sw) ((y - my) / sd), B = (w / Sw) ((r (x - mx)) / vx), g = -(A - B)
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif

namespace gsr {

constexpr int DEPTH_PRIOR_SUMS = 6;                         // doubles behind the int64 count: Sw, Sx, Sy, Sxx, Sxy, Syy
constexpr int DEPTH_PRIOR_SUM_WORDS = 1 + DEPTH_PRIOR_SUMS;  // 8-byte words of a partial of the sums kernel
constexpr int DEPTH_PRIOR_FIT_WORDS = 12;                   // doubles of DepthPriorFit
constexpr double DEPTH_PRIOR_DEGENERATE = 1.0 / 1099511627776.0;  // 2^-40: below it the moments form has no digits left

enum { DEPTH_PRIOR_L1 = 0, DEPTH_PRIOR_ALIGNED_L1 = 1, DEPTH_PRIOR_PEARSON = 2 };

struct DepthPriorFit {
  double n, Sw, mx, my, vx, vy, cov, sd, s, t, r, degenerate;
};

GSR_HD bool depth_prior_finite(float v) { return fabsf(v) <= FLT_MAX; }   // false for a NaN and for an infinity

GSR_HD bool depth_prior_valid(float x, float y, float w) {
  return w > 0.0f && w <= FLT_MAX && depth_prior_finite(x) && depth_prior_finite(y);
}

GSR_HD void depth_prior_terms(float x, float y, float w, double t[DEPTH_PRIOR_SUMS]) {
  const double wx = (double)w * (double)x;
  const double wy = (double)w * (double)y;
  t[0] = (double)w;
  t[1] = wx;
  t[2] = wy;
  t[3] = wx * (double)x;
  t[4] = wx * (double)y;
  t[5] = wy * (double)y;
}

GSR_HD void depth_prior_fit(long long n, const double S[DEPTH_PRIOR_SUMS], DepthPriorFit& f) {
  const double Sw = S[0];
  f.n = (double)n;
  f.Sw = Sw;
  f.mx = S[1] / Sw;
  f.my = S[2] / Sw;
  const double ex = S[3] / Sw;
  const double ey = S[5] / Sw;
  f.vx = ex - f.mx * f.mx;
  f.vy = ey - f.my * f.my;
  f.cov = S[4] / Sw - f.mx * f.my;
  const bool ok = n >= 2 && Sw > 0.0 && f.vx > DEPTH_PRIOR_DEGENERATE * ex && f.vy > DEPTH_PRIOR_DEGENERATE * ey;
  if (ok) {
    f.sd = sqrt(f.vx * f.vy);
    f.s = f.cov / f.vy;
    f.t = f.mx - f.s * f.my;
    f.r = f.cov / f.sd;
    f.degenerate = 0.0;
  } else {
    f.sd = 0.0;
    f.s = 1.0;
    f.t = 0.0;
    f.r = 0.0;
    f.degenerate = 1.0;
  }
}

// the residual of the two L1 modes
GSR_HD double depth_prior_residual(float x, float y, double a, double b) { return (double)x - (a * (double)y + b); }

// the L1 modes' gradient of a VALID pixel from its residual e
GSR_HD float depth_prior_grad_l1(double e, float w, double denom) {
  const double sign = e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0);
  return (float)(((double)w * sign) / denom);
}

// the two terms of the pearson gradient of a VALID pixel under a fit that is not degenerate
GSR_HD void depth_prior_pearson_terms(float x, float y, float w, const DepthPriorFit& f, double* A, double* B) {
  const double k = (double)w / f.Sw;
  *A = k * (((double)y - f.my) / f.sd);
  *B = k * ((f.r * ((double)x - f.mx)) / f.vx);
}

GSR_HD float depth_prior_grad_pearson(float x, float y, float w, const DepthPriorFit& f) {
  double A, B;
  depth_prior_pearson_terms(x, y, w, f, &A, &B);
  return (float)(-(A - B));
}

}  // namespace gsr
