// Per-Gaussian geometry shared by the translation units that project a Gaussian (preprocess.hip; depth.hip): the
// matrices, cov3D from scale / rotation, the EWA projection and the fused input activations.  A unit that includes
// this is built with -ffp-contract=off, so that all of them form the same float32 values.
#pragma once
#include "gsr_common.h"

namespace gsr {

struct Mat4 { float m[16]; };   // m[4*row + col] of the row-vector-convention tensor

__device__ inline void load_mat(const float* __restrict__ src, Mat4& d) {
#pragma unroll
  for (int i = 0; i < 16; ++i) d.m[i] = src[i];
}

// cov3D (xx,xy,xz,yy,yz,zz) = R diag(s^2) R^T, quaternion used as passed (A.2)
__device__ inline void cov3d_from_scale_rot(float sx, float sy, float sz, float mod, float r, float x, float y,
                                            float z, float* cov) {
  const float s0 = mod * sx, s1 = mod * sy, s2 = mod * sz;
  const float R00 = 1.0f - 2.0f * (y * y + z * z), R01 = 2.0f * (x * y - r * z), R02 = 2.0f * (x * z + r * y);
  const float R10 = 2.0f * (x * y + r * z), R11 = 1.0f - 2.0f * (x * x + z * z), R12 = 2.0f * (y * z - r * x);
  const float R20 = 2.0f * (x * z - r * y), R21 = 2.0f * (y * z + r * x), R22 = 1.0f - 2.0f * (x * x + y * y);
  const float L00 = R00 * s0, L01 = R01 * s1, L02 = R02 * s2;
  const float L10 = R10 * s0, L11 = R11 * s1, L12 = R12 * s2;
  const float L20 = R20 * s0, L21 = R21 * s1, L22 = R22 * s2;
  cov[0] = L00 * L00 + L01 * L01 + L02 * L02;
  cov[1] = L00 * L10 + L01 * L11 + L02 * L12;
  cov[2] = L00 * L20 + L01 * L21 + L02 * L22;
  cov[3] = L10 * L10 + L11 * L11 + L12 * L12;
  cov[4] = L10 * L20 + L11 * L21 + L12 * L22;
  cov[5] = L20 * L20 + L21 * L21 + L22 * L22;
}

// EWA projection intermediates shared by forward and backward.
struct Proj {
  float tx, ty, tz;        // clamped view-space point
  float txtz, tytz;        // unclamped ratios
  float j00, j02, j11, j12;
  float A0[3], A1[3];      // rows of J * Wv
  float a, b, c;           // dilated cov2D
};

__device__ inline void project_cov(const Mat4& V, float vx, float vy, float vz, const float* cov, float fx,
                                   float fy, float limx, float limy, Proj& o) {
  o.tz = vz;
  o.txtz = vx / vz;
  o.tytz = vy / vz;
  o.tx = fminf(limx, fmaxf(-limx, o.txtz)) * vz;
  o.ty = fminf(limy, fmaxf(-limy, o.tytz)) * vz;
  o.j00 = fx / vz;
  o.j02 = -(fx * o.tx) / (vz * vz);
  o.j11 = fy / vz;
  o.j12 = -(fy * o.ty) / (vz * vz);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    o.A0[j] = o.j00 * V.m[4 * j + 0] + o.j02 * V.m[4 * j + 2];
    o.A1[j] = o.j11 * V.m[4 * j + 1] + o.j12 * V.m[4 * j + 2];
  }
  const float S[3][3] = {{cov[0], cov[1], cov[2]}, {cov[1], cov[3], cov[4]}, {cov[2], cov[4], cov[5]}};
  float B0[3], B1[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    B0[j] = o.A0[0] * S[0][j] + o.A0[1] * S[1][j] + o.A0[2] * S[2][j];
    B1[j] = o.A1[0] * S[0][j] + o.A1[1] * S[1][j] + o.A1[2] * S[2][j];
  }
  o.a = (B0[0] * o.A0[0] + B0[1] * o.A0[1] + B0[2] * o.A0[2]) + DILATION;
  o.b = B0[0] * o.A1[0] + B0[1] * o.A1[1] + B0[2] * o.A1[2];
  o.c = (B1[0] * o.A1[0] + B1[1] * o.A1[1] + B1[2] * o.A1[2]) + DILATION;
}

// ---- fused input activations: the raw parameters of scene/gaussian_model.py:151-183 -------
struct Activated {
  float sc[3];      // activated scales
  float4 q;         // activated (normalised) quaternion
  float qn;         // norm used for the normalisation (1 when not normalising)
  float op;         // activated opacity
};
// the raw values are read first (all of a Gaussian's small loads are issued together, ahead of the arithmetic that
// decides whether they are needed), activated later
__device__ inline void load_scale_rot_raw(const GsrParams& p, int idx, Activated& a) {
  a.sc[0] = p.scales[3 * (size_t)idx];
  a.sc[1] = p.scales[3 * (size_t)idx + 1];
  a.sc[2] = p.scales[3 * (size_t)idx + 2];
  a.q = reinterpret_cast<const float4*>(p.rotations)[idx];
}
__device__ inline void activate_scale_rot(const GsrParams& p, Activated& a) {
  if (p.act_flags & GSR_ACT_SCALE_EXP) {
#pragma unroll
    for (int k = 0; k < 3; ++k) a.sc[k] = expf(a.sc[k]);
  }
  a.qn = 1.0f;
  if (p.act_flags & GSR_ACT_ROT_NORMALIZE) {
    a.qn = fmaxf(sqrtf(a.q.x * a.q.x + a.q.y * a.q.y + a.q.z * a.q.z + a.q.w * a.q.w), 1e-12f);
    a.q.x = a.q.x / a.qn; a.q.y = a.q.y / a.qn; a.q.z = a.q.z / a.qn; a.q.w = a.q.w / a.qn;
  }
}
__device__ inline void load_scale_rot(const GsrParams& p, int idx, Activated& a) {
  load_scale_rot_raw(p, idx, a);
  activate_scale_rot(p, a);
}

}  // namespace gsr
