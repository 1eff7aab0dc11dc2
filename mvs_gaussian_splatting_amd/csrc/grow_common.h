// Per-Gaussian helpers shared by the fork's render-side expansion (grow.hip) and its densification
// (densify_fork.hip): the same direction rule and rotation in both, so a Gaussian grows where the frame drew it.
#pragma once
#include "gsr_common.h"

namespace gsr {

__device__ inline float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

struct Rot {
  float w, x, y, z, norm;   // normalised quaternion and the norm it was divided by
  float R[9];
};

// utils/general_utils.py:78-99 build_rotation
__device__ inline void build_rotation(const float* __restrict__ q, Rot& r) {
  const float qr = q[0], qx = q[1], qy = q[2], qz = q[3];
  r.norm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);
  const float w = qr / r.norm, x = qx / r.norm, y = qy / r.norm, z = qz / r.norm;
  r.w = w; r.x = x; r.y = y; r.z = z;
  r.R[0] = 1.f - 2.f * (y * y + z * z); r.R[1] = 2.f * (x * y - w * z); r.R[2] = 2.f * (x * z + w * y);
  r.R[3] = 2.f * (x * y + w * z); r.R[4] = 1.f - 2.f * (x * x + z * z); r.R[5] = 2.f * (y * z - w * x);
  r.R[6] = 2.f * (x * z - w * y); r.R[7] = 2.f * (y * z + w * x); r.R[8] = 1.f - 2.f * (x * x + y * y);
}

// argmax of softmax(logits) over one row, in every lane: the largest logit, the lowest index on ties (:361-363).  A row
// without any ordered value yields index 0 and max -inf.
__device__ inline void wave_argmax(const float* __restrict__ row, int nd, int lane, float& best, int& bi) {
  best = -INFINITY;
  bi = nd;
  for (int n = lane; n < nd; n += WAVE) {
    const float v = row[n];
    if (v > best || (bi == nd && v == best)) { best = v; bi = n; }
  }
#pragma unroll
  for (int k = WAVE / 2; k > 0; k >>= 1) {
    const float ob = __shfl_xor(best, k, WAVE);
    const int oi = __shfl_xor(bi, k, WAVE);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if (bi >= nd) bi = 0;
}

}  // namespace gsr
