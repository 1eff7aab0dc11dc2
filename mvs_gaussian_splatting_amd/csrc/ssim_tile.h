// The SSIM tile core that csrc/loss.hip and csrc/masked_loss.hip share: the 11-tap Gaussian of
// utils/loss_utils.py:23-25, the 16x16 output tile with its 26x26 halo, the staging and the two separable passes of the
// forward (ssim_tile_moments), the per-pixel terms of utils/loss_utils.py:39-63 and their derivatives (ssim_terms,
// ssim_derivs), the convolution of the three derivative maps of the backward (ssim_convolve_maps), and the tile count.
// A kernel keeps what is its own: how a halo pixel is loaded (zero padding, clamp, mask) and its epilogue.
//
// LDS is the caller's: rows of 27 and 17 dwords, odd strides, so that the 16 lanes of a tile row and the rows under
// them fall on different banks in both passes.  Every lane of the 256-lane workgroup must call ssim_tile_moments and
// ssim_convolve_maps: each holds two barriers.  Every global read is the loader's, under 0 <= x < W, 0 <= y < H.
//
// The one deliberate difference between the two losses is the SSIM value s itself and stays with the caller:
// loss.hip forms s = N1 N2 inv with inv = 1 / (D1 D2); masked_loss.hip forms s = (N1 N2) / (D1 D2), a true division
// that is exactly 1 where the two images agree on the window.  The two round differently; merging them would change
// the bits of one of the losses.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace gsr {

constexpr int SS_T = 16;                 // output tile edge
constexpr int SS_R = 5;                  // window radius (11 taps)
constexpr int SS_H = SS_T + 2 * SS_R;    // halo edge (26)

struct Win11 { float w[11]; };

// one workgroup per 16x16 output tile and channel
inline size_t ssim_tiles(int C, int H, int W) {
  return (size_t)((W + SS_T - 1) / SS_T) * (size_t)((H + SS_T - 1) / SS_T) * (size_t)C;
}

__device__ inline float halo_load(const float* __restrict__ img, int W, int H, int x, int y) {
  return (x >= 0 && x < W && y >= 0 && y < H) ? img[(size_t)y * W + x] : 0.0f;
}

inline Win11 make_window() {
  Win11 win;
  double g[11];
  for (int i = 0; i < 11; ++i) g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
  // utils/loss_utils.py:23-25 builds the window in float32: exp() per tap, then a float32 normalisation
  float gf[11], totf = 0.f;
  for (int i = 0; i < 11; ++i) { gf[i] = (float)g[i]; totf += gf[i]; }
  for (int i = 0; i < 11; ++i) win.w[i] = gf[i] / totf;
  return win;
}

// ---- forward --------------------------------------------------------------------------------------------------------
// the five windowed moments of the lane's pixel: E[x], E[y], E[x^2], E[y^2], E[xy]
struct SsimMoments { float m1, m2, exx, eyy, exy; };

// Stages the halo of the tile at (x0, y0) through load(gx, gy, xv, yv) -- which applies the padding, clamp or mask --
// and runs the horizontal and the vertical 11-tap pass.  sx, sy keep the staged halo: the lane's own pixel is
// sx[ty + SS_R][tx + SS_R].
template <typename Load>
__device__ inline SsimMoments ssim_tile_moments(float (&sx)[SS_H][SS_H + 1], float (&sy)[SS_H][SS_H + 1],
                                                float (&hz)[5][SS_H][SS_T + 1], const Win11& win, int x0, int y0,
                                                Load load) {
  const int tx = threadIdx.x & (SS_T - 1), ty = threadIdx.x / SS_T;
  for (int i = threadIdx.x; i < SS_H * SS_H; i += SS_T * SS_T) {
    const int hy = i / SS_H, hx = i - hy * SS_H;
    float xv, yv;
    load(x0 + hx - SS_R, y0 + hy - SS_R, xv, yv);
    sx[hy][hx] = xv;
    sy[hy][hx] = yv;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SS_H * SS_T; i += SS_T * SS_T) {
    const int hy = i / SS_T, ox = i - hy * SS_T;
    float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float xv = sx[hy][ox + k], yv = sy[hy][ox + k], wk = win.w[k];
      a += wk * xv; b += wk * yv; aa += wk * xv * xv; bb += wk * yv * yv; ab += wk * xv * yv;
    }
    hz[0][hy][ox] = a; hz[1][hy][ox] = b; hz[2][hy][ox] = aa; hz[3][hy][ox] = bb; hz[4][hy][ox] = ab;
  }
  __syncthreads();
  SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 11; ++k) {
    const float wk = win.w[k];
    m.m1 += wk * hz[0][ty + k][tx]; m.m2 += wk * hz[1][ty + k][tx]; m.exx += wk * hz[2][ty + k][tx];
    m.eyy += wk * hz[3][ty + k][tx]; m.exy += wk * hz[4][ty + k][tx];
  }
  return m;
}

// SSIM = (N1 N2) / (D1 D2); den = D1 D2, inv = 1 / den.  The value s is the caller's (see the head of the file).
struct SsimTerms { float N1, N2, D1, D2, den, inv; };

__device__ inline SsimTerms ssim_terms(const SsimMoments& m) {
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  const float mu1_sq = m.m1 * m.m1, mu2_sq = m.m2 * m.m2, mu12 = m.m1 * m.m2;
  const float s1 = m.exx - mu1_sq, s2 = m.eyy - mu2_sq, s12 = m.exy - mu12;
  SsimTerms t;
  t.N1 = 2.0f * mu12 + C1;
  t.N2 = 2.0f * s12 + C2;
  t.D1 = mu1_sq + mu2_sq + C1;
  t.D2 = s1 + s2 + C2;
  t.den = t.D1 * t.D2;
  t.inv = 1.0f / t.den;
  return t;
}

// the unscaled derivatives of s through the moments of x: d s / d mu1, d s / d E[x^2], d s / d E[xy]
struct SsimDerivs { float dm1, dexx, dexy; };

__device__ inline SsimDerivs ssim_derivs(const SsimMoments& m, const SsimTerms& t, float s) {
  SsimDerivs d;
  d.dm1 = 2.0f * m.m2 * (t.N2 - t.N1) * t.inv - s * 2.0f * m.m1 * (t.D2 - t.D1) * t.inv;
  d.dexx = -s / t.D2;
  d.dexy = 2.0f * t.N1 * t.inv;
  return d;
}

// ---- backward -------------------------------------------------------------------------------------------------------
// w * A, w * B, w * Cm at the lane's pixel (w symmetric), zero for a lane outside the image
struct SsimMapGrads { float ga, gb, gc; };

// maps: the three derivative maps of this channel, `total` floats apart; zero padding
__device__ inline SsimMapGrads ssim_convolve_maps(float (&sm)[3][SS_H][SS_H + 1], float (&hz)[3][SS_H][SS_T + 1],
                                                  const Win11& win, const float* __restrict__ maps, size_t total, int W,
                                                  int H, int x0, int y0) {
  const int tx = threadIdx.x & (SS_T - 1), ty = threadIdx.x / SS_T;
  for (int i = threadIdx.x; i < SS_H * SS_H; i += SS_T * SS_T) {
    const int hy = i / SS_H, hx = i - hy * SS_H;
#pragma unroll
    for (int m = 0; m < 3; ++m) sm[m][hy][hx] = halo_load(maps + m * total, W, H, x0 + hx - SS_R, y0 + hy - SS_R);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SS_H * SS_T; i += SS_T * SS_T) {
    const int hy = i / SS_T, ox = i - hy * SS_T;
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = win.w[k];
      a += wk * sm[0][hy][ox + k]; b += wk * sm[1][hy][ox + k]; c += wk * sm[2][hy][ox + k];
    }
    hz[0][hy][ox] = a; hz[1][hy][ox] = b; hz[2][hy][ox] = c;
  }
  __syncthreads();
  SsimMapGrads g = {0.f, 0.f, 0.f};
  if (x0 + tx < W && y0 + ty < H) {
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float wk = win.w[k];
      g.ga += wk * hz[0][ty + k][tx]; g.gb += wk * hz[1][ty + k][tx]; g.gc += wk * hz[2][ty + k][tx];
    }
  }
  return g;
}

}  // namespace gsr
