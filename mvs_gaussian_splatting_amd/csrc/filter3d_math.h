// Mip-Splatting's 3D smoothing filter (csrc/filter3d.hip; filter3d.py), written once for device and
// host: tests/filter3d_host_check.cpp builds it with the host compiler, so the float32 operation order of the sampling
// pass is checked against the numpy restatement (tests/filter3d_restate.py) bit for bit without a GPU, and the float64
// closed forms of the application to the last place of a float32.
//
// Sampling, one (Gaussian, view) pair; float32, every operation rounded on its own (both builds pass -ffp-contract=off):
//     (xv, yv, zv) = (x, y, z, 1) through world_to_view, the association of mesh_cull_math.h's cull_transform
//     out unless zv > near                                              (a NaN fails)
//     W = (float)width, H = (float)height                               (at most 2^24: exact)
//     u = (xv / zv) * fx + W * 0.5f         w = (yv / zv) * fy + H * 0.5f
//     out unless -margin * W <= u <= (1 + margin) * W  and  -margin * H <= w <= (1 + margin) * H     (inclusive; a NaN fails)
//     min_depth = fminf(min_depth, zv)      max_rate = fmaxf(max_rate, fx / zv)       seen
//
// Width, one Gaussian; D = the largest min_depth and R = the smallest max_rate over the seen rows (an unseen Gaussian
// takes them: it is filtered as the farthest / most coarsely sampled seen one):
//     mip_splatting   filter = ((seen ? min_depth : D) / focal_max) * sqrtf(variance)
//     paper           filter = sqrtf(variance) / (seen ? max_rate : R)
//
// Application, one Gaussian, float64 from float32 inputs, each output rounded to float32 once.  With f the filter,
// t_i = f^2 exp(-2 s_i), l_i = log1p(t_i) / 2 and L = l_0 + l_1 + l_2 (so that c = exp(-L) and 1 - c = -expm1(-L)):
//     s'_i = s_i + l_i
//     o'   = o                                        when 1 - c == 0          (f = 0 lands here: s and o bit for bit)
//          = (o - L) - log1p((1 - c) exp(o))          when o <= 0
//          = -L - log((1 - c) + exp(-o))              when o > 0
// which is logit(sigmoid(o) c) = log c - log((1 - c) + exp(-o)) with the large exponential factored out.  Gradients:
//     ds'_i/ds_i = 1 / (1 + t_i)      dL/ds_i = -t_i / (1 + t_i)
//     do'/do = 1 / (1 + (1 - c) exp(o)) = exp(-o) / ((1 - c) + exp(-o))
//     do'/dL = -(1 + exp(o)) / (1 + (1 - c) exp(o)) = -(1 + exp(-o)) / ((1 - c) + exp(-o))
// each in the form whose exponential is at most 1.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gsr.h"

#ifndef GSR_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif
#endif

namespace gsr {

// one view of the sampling pass -> whether it counts; min_depth and max_rate are updated when it does
GSR_HD bool filter3d_view_sample(const GsrFilterView& view, float x, float y, float z, float near, float margin,
                                 float& min_depth, float& max_rate) {
  const float* M = view.world_to_view;
  const float xv = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
  const float yv = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
  const float zv = ((x * M[2] + y * M[6]) + z * M[10]) + M[14];
  if (!(zv > near)) return false;
  const float W = (float)view.width, H = (float)view.height;
  const float u = (xv / zv) * view.fx + W * 0.5f, w = (yv / zv) * view.fy + H * 0.5f;
  const float hi = 1.0f + margin;
  if (!(u >= -margin * W && u <= hi * W && w >= -margin * H && w <= hi * H)) return false;      // a NaN fails
  min_depth = fminf(min_depth, zv);
  max_rate = fmaxf(max_rate, view.fx / zv);
  return true;
}

// own: the row's min_depth (mip_splatting) or max_rate (paper); global: D or R of the seen rows
GSR_HD float filter3d_width(int rule, bool seen, float own, float global, float focal_max, float variance) {
  const float v = seen ? own : global;
  const float sd = sqrtf(variance);
  return rule == GSR_FILTER3D_PAPER ? sd / v : (v / focal_max) * sd;
}

struct Filter3dTerms {
  double t[3];      // f^2 exp(-2 s_i)
  double L;         // sum log1p(t_i) / 2 = -log c
  double omc;       // 1 - c
};

GSR_HD Filter3dTerms filter3d_terms(const float s[3], float f, double l[3]) {
  Filter3dTerms q;
  const double f2 = (double)f * (double)f;
  for (int i = 0; i < 3; ++i) {
    q.t[i] = f2 * exp(-2.0 * (double)s[i]);
    l[i] = 0.5 * log1p(q.t[i]);
  }
  q.L = (l[0] + l[1]) + l[2];
  q.omc = -expm1(-q.L);
  return q;
}

GSR_HD void filter3d_apply_row(const float s[3], float o, float f, float s_out[3], float* o_out) {
  double l[3];
  const Filter3dTerms q = filter3d_terms(s, f, l);
  for (int i = 0; i < 3; ++i) s_out[i] = (float)((double)s[i] + l[i]);
  const double od = (double)o;
  double r;
  if (q.omc == 0.0) r = od;
  else if (od <= 0.0) r = (od - q.L) - log1p(q.omc * exp(od));
  else r = -q.L - log(q.omc + exp(-od));
  *o_out = (float)r;
}

GSR_HD void filter3d_apply_bwd_row(const float s[3], float o, float f, const float g_s[3], float g_o, float d_s[3],
                                   float* d_o) {
  double l[3];
  const Filter3dTerms q = filter3d_terms(s, f, l);
  const double od = (double)o;
  double do_do, do_dL;
  if (od <= 0.0) {
    const double e = exp(od), den = 1.0 + q.omc * e;
    do_do = 1.0 / den;
    do_dL = -(1.0 + e) / den;
  } else {
    const double e = exp(-od), den = q.omc + e;
    do_do = den > 0.0 ? e / den : 1.0;
    do_dL = den > 0.0 ? -(1.0 + e) / den : 0.0;
  }
  *d_o = (float)((double)g_o * do_do);
  const double gL = (double)g_o * do_dL;
  for (int i = 0; i < 3; ++i) {
    const double w = 1.0 / (1.0 + q.t[i]);                   // t = inf: w = 0 and the second factor below is -1
    const double u = q.t[i] > 1.0e300 ? 1.0 : q.t[i] * w;
    d_s[i] = (float)((double)g_s[i] * w - gL * u);
  }
}

}  // namespace gsr
