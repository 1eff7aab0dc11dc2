// The forward-backward reprojection round trip that mvs.hip (the consistency filter) and mvs_loss.hip (the training
// loss) share: one reference pixel into one source view at its depth, the source's depth read there (bilinear), and back.
// The float32 operation order is the header comment of mvs.hip; both units are built with -ffp-contract=off, so the two
// kernels form the same bits up to (ub, vb, zb).
#pragma once
#include "gsr_common.h"
#include "../../include/gsr.h"

#ifndef MVS_TILE_X
#define MVS_TILE_X 64
#endif

namespace gsr {

constexpr int MVS_BLOCK = 256;
constexpr int MVS_TILE_Y = MVS_BLOCK / MVS_TILE_X;
static_assert(MVS_TILE_X * MVS_TILE_Y == MVS_BLOCK && MVS_TILE_X >= 1, "a tile is one 256-lane workgroup");

// (x, y, z, 1) through M, row-vector convention, the association of mvs.hip's header comment
__device__ inline void mvs_transform(const float* __restrict__ M, float x, float y, float z, float& ox, float& oy,
                                     float& oz) {
  ox = ((x * M[0] + y * M[4]) + z * M[8]) + M[12];
  oy = ((x * M[1] + y * M[5]) + z * M[9]) + M[13];
  oz = ((x * M[2] + y * M[6]) + z * M[10]) + M[14];
}

// What one round trip leaves behind.  The consistency filter reads zb, du, dv; the loss reads all of it.
struct MvsTrip {
  float xs, ys, zs;              // the reference point in the source's frame
  float cxs, cys, us, vs;        // the source's principal point and where the point lands
  float ax, ay;                  // us - floor(us), vs - floor(vs)
  size_t tap;                    // index of (x0, y0) in the source's depth; the other taps are +1, +width, +width + 1
  float d00, d10, d01, d11, ds;  // the four taps and their bilinear value
  float xb0, yb0;                // (us, vs, ds) back-projected in the source's frame
  float xb, yb, zb;              // ... and in the reference's
  float du, dv;                  // ub - px, vb - py
};

// The trip of reference pixel (fpx, fpy) at depth d > 0 with (xr, yr) = (((px - cx) d) / fx, ((py - cy) d) / fy).
// false as soon as a gate fails: zs > 0.2, the 2 x 2 footprint inside the source (a NaN fails), four taps > 0, zb > 0.2.
// Every gather is behind the footprint test, formed in float32 from the row's own width and height.
__device__ inline bool mvs_round_trip(const GsrMvsSource& src, float fpx, float fpy, float cx, float cy, float fx, float fy,
                                      float xr, float yr, float d, MvsTrip& t) {
  mvs_transform(src.ref_to_src, xr, yr, d, t.xs, t.ys, t.zs);
  if (!(t.zs > 0.2f)) return false;
  const float Ws = (float)src.width, Hs = (float)src.height;
  t.cxs = (Ws - 1.0f) * 0.5f;
  t.cys = (Hs - 1.0f) * 0.5f;
  t.us = (src.fx * t.xs) / t.zs + t.cxs;
  t.vs = (src.fy * t.ys) / t.zs + t.cys;
  const float x0 = floorf(t.us), y0 = floorf(t.vs);
  if (!(x0 >= 0.0f && x0 + 1.0f <= Ws - 1.0f && y0 >= 0.0f && y0 + 1.0f <= Hs - 1.0f)) return false;   // a NaN fails
  t.ax = t.us - x0;
  t.ay = t.vs - y0;
  t.tap = (size_t)(int)y0 * (size_t)src.width + (size_t)(int)x0;
  const float* __restrict__ row0 = src.depth + t.tap;
  const float* __restrict__ row1 = row0 + src.width;
  t.d00 = row0[0];
  t.d10 = row0[1];
  t.d01 = row1[0];
  t.d11 = row1[1];
  if (!(t.d00 > 0.0f && t.d10 > 0.0f && t.d01 > 0.0f && t.d11 > 0.0f)) return false;
  t.ds = (t.d00 * (1.0f - t.ax) + t.d10 * t.ax) * (1.0f - t.ay) + (t.d01 * (1.0f - t.ax) + t.d11 * t.ax) * t.ay;
  t.xb0 = ((t.us - t.cxs) * t.ds) / src.fx;
  t.yb0 = ((t.vs - t.cys) * t.ds) / src.fy;
  mvs_transform(src.src_to_ref, t.xb0, t.yb0, t.ds, t.xb, t.yb, t.zb);
  if (!(t.zb > 0.2f)) return false;
  const float ub = (fx * t.xb) / t.zb + cx, vb = (fy * t.yb) / t.zb + cy;
  t.du = ub - fpx;
  t.dv = vb - fpy;
  return true;
}

inline bool mvs_positive_finite(float v) { return v > 0.0f && v - v == 0.0f; }   // false for NaN and +-inf

}  // namespace gsr
