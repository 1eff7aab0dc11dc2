// The SSIM window and tile shape that csrc/loss.hip and csrc/masked_loss.hip share: the 11-tap Gaussian of
// utils/loss_utils.py:23-25, the 16x16 output tile with its 26x26 halo, and the zero-padded halo load.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

namespace gsr {

constexpr int SS_T = 16;                 // output tile edge
constexpr int SS_R = 5;                  // window radius (11 taps)
constexpr int SS_H = SS_T + 2 * SS_R;    // halo edge (26)

struct Win11 { float w[11]; };

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

}  // namespace gsr
