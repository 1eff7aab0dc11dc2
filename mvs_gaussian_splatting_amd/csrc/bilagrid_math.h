// The per-pixel arithmetic of csrc/bilagrid.hip (include/gsr.h, ABI v38), as functions a host compiler
// takes too: tests/bilagrid_host_check.cpp is the host build, which tests/test_bilagrid_host.py holds to the GPU test's
// bar.  Inputs and outputs are float32; every intermediate is a double and each output is rounded once, on its store,
// as in planes_math.h.  The unit is built with -ffp-contract=off; the sums are written left to right.
//
// Grid G [12, L, Hg, Wg]: channel 4 c + k is A[c,k] (c the output colour, k the input colour, k = 3 the offset).
// Pixel (x, y) of a [3,H,W] image X:  u = (x + 0.5) / W (Wg - 1),  v = (y + 0.5) / H (Hg - 1),
// gray = 0.299 X0 + 0.587 X1 + 0.114 X2,  z = clamp(gray, 0, 1) (L - 1);  dz/dgray = L - 1 for 0 < gray < 1, else 0 (a
// gray that is not finite included: a NaN clamps to 0).  Cell i0 = min(floor(u), Wg - 2), tu = u - i0, likewise v, z.
// Each coefficient: nested lerps a + t (b - a) along x, then y, then z -- a grid that is constant over the pixel's cell
// returns the cell's value bit for bit, so the identity grid gives Y = X and dX = g bit for bit on finite input.
#pragma once
#include <math.h>
#include <stddef.h>

#ifndef GSR_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif
#endif

namespace gsr {

constexpr int BG_TERMS = 12;
constexpr int BG_MIN_SIZE = 2, BG_MAX_XY = 64, BG_MAX_L = 16;

struct BilagridShape {
  int H, W, Wg, Hg, L;
};

GSR_HD bool bilagrid_shape_ok(int Wg, int Hg, int L) {
  return Wg >= BG_MIN_SIZE && Wg <= BG_MAX_XY && Hg >= BG_MIN_SIZE && Hg <= BG_MAX_XY && L >= BG_MIN_SIZE && L <= BG_MAX_L;
}

// What a pixel decides: its cell and the three fractions, and the slope of z in gray (0 where the clamp acts).
struct BilagridPixel {
  int i0, j0, l0;
  double tu, tv, tz;
  double dz_dgray;
};

// coordinate c in [0, n - 1] of an axis with n vertices -> cell and fraction
GSR_HD void bg_cell(double c, int n, int& i0, double& t) {
  int i = (int)floor(c);
  if (i > n - 2) i = n - 2;
  if (i < 0) i = 0;
  i0 = i;
  t = c - (double)i;
}

// pixel centre p of n_px along an axis with n_v vertices
GSR_HD double bg_axis_coord(int p, int n_px, int n_v) { return ((double)p + 0.5) / (double)n_px * (double)(n_v - 1); }

GSR_HD void bg_pixel(const float X[3], int x, int y, const BilagridShape& s, BilagridPixel& o) {
  bg_cell(bg_axis_coord(x, s.W, s.Wg), s.Wg, o.i0, o.tu);
  bg_cell(bg_axis_coord(y, s.H, s.Hg), s.Hg, o.j0, o.tv);
  const double gray = (0.299 * (double)X[0] + 0.587 * (double)X[1]) + 0.114 * (double)X[2];
  const double lm1 = (double)(s.L - 1);
  const bool inside = gray > 0.0 && gray < 1.0;                 // false for a NaN
  const double clamped = inside ? gray : (gray >= 1.0 ? 1.0 : 0.0);
  o.dz_dgray = inside ? lm1 : 0.0;
  bg_cell(clamped * lm1, s.L, o.l0, o.tz);
}

// The 12 coefficients at the pixel and their slope in z: the difference of the two z slabs after the x and y lerps.
GSR_HD void bg_slice(const float* G, const BilagridShape& s, const BilagridPixel& p, double A[BG_TERMS],
                     double dA_dz[BG_TERMS]) {
  const size_t sy = (size_t)s.Wg, sz = sy * (size_t)s.Hg, sc = sz * (size_t)s.L;
  const float* base = G + ((size_t)p.l0 * sz + (size_t)p.j0 * sy + (size_t)p.i0);
  for (int t = 0; t < BG_TERMS; ++t) {
    const float* q = base + (size_t)t * sc;
    const double a00 = q[0], a01 = q[1], a10 = q[sy], a11 = q[sy + 1];
    const double b00 = q[sz], b01 = q[sz + 1], b10 = q[sz + sy], b11 = q[sz + sy + 1];
    const double a0 = a00 + p.tu * (a01 - a00), a1 = a10 + p.tu * (a11 - a10);
    const double b0 = b00 + p.tu * (b01 - b00), b1 = b10 + p.tu * (b11 - b10);
    const double a = a0 + p.tv * (a1 - a0), b = b0 + p.tv * (b1 - b0);
    dA_dz[t] = b - a;
    A[t] = a + p.tz * (b - a);
  }
}

// Y[c] = A[c,0] X0 + A[c,1] X1 + A[c,2] X2 + A[c,3], no clamp
GSR_HD void bg_apply(const double A[BG_TERMS], const float X[3], float Y[3]) {
  const double x0 = X[0], x1 = X[1], x2 = X[2];
  for (int c = 0; c < 3; ++c) Y[c] = (float)(((A[4 * c] * x0 + A[4 * c + 1] * x1) + A[4 * c + 2] * x2) + A[4 * c + 3]);
}

// dL/dX[k] = sum_c A[c,k] g[c] + coef_k dz/dgray sum_c g[c] sum_k' dA[c,k']/dz Xt[k'],  Xt = (X0, X1, X2, 1)
GSR_HD void bg_image_grad(const double A[BG_TERMS], const double dA_dz[BG_TERMS], const float X[3], const float g[3],
                          double dz_dgray, float dX[3]) {
  const double x0 = X[0], x1 = X[1], x2 = X[2], g0 = g[0], g1 = g[1], g2 = g[2];
  double through_z = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double dy_dz = ((dA_dz[4 * c] * x0 + dA_dz[4 * c + 1] * x1) + dA_dz[4 * c + 2] * x2) + dA_dz[4 * c + 3];
    through_z += (double)g[c] * dy_dz;
  }
  const double coef[3] = {0.299, 0.587, 0.114};
  for (int k = 0; k < 3; ++k)
    dX[k] = (float)(((A[k] * g0 + A[4 + k] * g1) + A[8 + k] * g2) + coef[k] * dz_dgray * through_z);
}

// The weight a pixel with cell i0 and fraction t puts on vertex i of that axis: what the lerp a + t (b - a) gives a and
// b.  Along z this is the hat max(0, 1 - |z - l|) of level l.
GSR_HD double bg_axis_weight(int i0, double t, int i) { return i == i0 ? 1.0 - t : (i == i0 + 1 ? t : 0.0); }

// A range [lo, hi] of pixels that holds every pixel of an axis with a weight on vertex i (cells i - 1 and i: coordinate
// in [i - 1, i + 1)), with a pixel of slack on either side: the weight is evaluated per pixel and is exactly 0 outside.
GSR_HD void bg_vertex_range(int i, int n_px, int n_v, int& lo, int& hi) {
  const double scale = (double)n_px / (double)(n_v - 1);
  double l = floor((double)(i - 1) * scale - 0.5) - 1.0, h = ceil((double)(i + 1) * scale - 0.5) + 1.0;
  if (l < 0.0) l = 0.0;
  if (h > (double)(n_px - 1)) h = (double)(n_px - 1);
  lo = (int)l;
  hi = (int)h;
}

// The 12 terms g[c] Xt[k] of dL/dG at 4 c + k that a pixel adds, under its weight, to a vertex
GSR_HD void bg_grid_terms(const float X[3], const float g[3], double w, double acc[BG_TERMS]) {
  const double xt[4] = {(double)X[0], (double)X[1], (double)X[2], 1.0};
  for (int c = 0; c < 3; ++c)
    for (int k = 0; k < 4; ++k) acc[4 * c + k] += w * ((double)g[c] * xt[k]);
}

}  // namespace gsr
