// Per-Gaussian planes (n_view, d) for PGSR's unbiased depth, forward and backward (include/gsr.h, ABI v37;
// features.gaussian_planes).  Per row, with q = rot / max(|rot|, 1e-12) and R the matrix of
// features._rotation_matrices:
//     axis = the index of the smallest scale, the smallest index among equals
//     n_w  = R[:, axis], times -1 when n_w . (campos - mean) < 0 (exactly 0 keeps +1)
//     planes = (n_w @ viewmatrix[:3,:3], n_w . (campos - mean))
// Backward, axis and sign decisions without gradient: G = sign (V g[0:3] + g[3] (campos - mean)) is dL/dR[:, axis],
// dL/dq follows from the column's entries, dL/drot = (dL/dq - q (q . dL/dq)) / |rot| (dL/dq / 1e-12 under the clamp),
// dL/dmean = -g[3] n_w.  The arithmetic is planes_math.h's: float32 in and out, doubles in between.
//
// One lane per row, 256-lane workgroups.  The quaternion, the plane row and their gradients move as one 16-byte access
// per lane; scales and means are three 4-byte loads each (12-byte rows).  The camera is a kernel argument.  No LDS, no
// atomics, nothing that depends on the order lanes run in: the same bits from run to run.  Forward 56 bytes per row,
// backward 84.
#include "gsr_common.h"
#include "gsr_entry.h"
#include "planes_math.h"

namespace gsr {

namespace {

constexpr int PL_THREADS = 256;

__device__ inline void load3(const float* __restrict__ p, int64_t row, float out[3]) {
  out[0] = p[3 * row];
  out[1] = p[3 * row + 1];
  out[2] = p[3 * row + 2];
}

__global__ __launch_bounds__(PL_THREADS) void planes_fwd_kernel(const float* __restrict__ scales,
                                                                const float4* __restrict__ rotations,
                                                                const float* __restrict__ means3D, int32_t P,
                                                                PlaneCamera cam, float4* __restrict__ planes) {
  const int64_t row = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
  if (row >= P) return;
  float s[3], m[3], out[4];
  load3(scales, row, s);
  load3(means3D, row, m);
  const float4 q4 = rotations[row];
  const float rot[4] = {q4.x, q4.y, q4.z, q4.w};
  plane_forward(s, rot, m, cam, out);
  planes[row] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(PL_THREADS) void planes_bwd_kernel(const float* __restrict__ scales,
                                                                const float4* __restrict__ rotations,
                                                                const float* __restrict__ means3D, int32_t P,
                                                                PlaneCamera cam, const float4* __restrict__ dL_dplanes,
                                                                float4* __restrict__ dL_drotations,
                                                                float* __restrict__ dL_dmeans3D) {
  const int64_t row = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x;
  if (row >= P) return;
  float s[3], m[3], d_rot[4], d_mean[3];
  load3(scales, row, s);
  load3(means3D, row, m);
  const float4 q4 = rotations[row], g4 = dL_dplanes[row];
  const float rot[4] = {q4.x, q4.y, q4.z, q4.w}, g[4] = {g4.x, g4.y, g4.z, g4.w};
  plane_backward(s, rot, m, cam, g, d_rot, d_mean);
  dL_drotations[row] = make_float4(d_rot[0], d_rot[1], d_rot[2], d_rot[3]);
  dL_dmeans3D[3 * row] = d_mean[0];
  dL_dmeans3D[3 * row + 1] = d_mean[1];
  dL_dmeans3D[3 * row + 2] = d_mean[2];
}

PlaneCamera plane_camera(const float* viewmatrix, const float* campos) {
  PlaneCamera cam;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) cam.v[3 * i + j] = viewmatrix[4 * i + j];
    cam.campos[i] = campos[i];
  }
  return cam;
}

// the checks the two entry points share; 0 when the call may go on
int planes_args(const float* scales, const float* rotations, const float* means3D, int32_t P, const float* viewmatrix,
                const float* campos) {
  if (P < 0) return fail(GSR_E_BADARG, "P must not be negative");
  if (!viewmatrix || !campos) return fail(GSR_E_BADARG, "NULL viewmatrix or campos");
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      if (!(fabsf(viewmatrix[4 * i + j]) <= 3.402823466e38f)) return fail(GSR_E_BADARG, "viewmatrix must be finite");
    if (!(fabsf(campos[i]) <= 3.402823466e38f)) return fail(GSR_E_BADARG, "campos must be finite");
  }
  if (P == 0) return 0;
  if (!scales || !rotations || !means3D) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({scales, means3D}, 3u)) return fail(GSR_E_ALIGN, "scales and means3D must be 4-byte aligned");
  if (!aligned({rotations}, 15u)) return fail(GSR_E_ALIGN, "rotations must be 16-byte aligned");
  return 0;
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

int gsr_gaussian_planes_fwd(const float* scales, const float* rotations, const float* means3D, int32_t P,
                            const float* viewmatrix, const float* campos, float* planes, void* stream) {
  if (const int rc = planes_args(scales, rotations, means3D, P, viewmatrix, campos)) return rc;
  if (P == 0) return 0;
  if (!planes) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({planes}, 15u)) return fail(GSR_E_ALIGN, "planes must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)(((int64_t)P + PL_THREADS - 1) / PL_THREADS);
  hipLaunchKernelGGL(planes_fwd_kernel, dim3(blocks), dim3(PL_THREADS), 0, s, scales,
                     reinterpret_cast<const float4*>(rotations), means3D, P, plane_camera(viewmatrix, campos),
                     reinterpret_cast<float4*>(planes));
  return check(false, s, "gaussian_planes_fwd");
}

int gsr_gaussian_planes_bwd(const float* scales, const float* rotations, const float* means3D, int32_t P,
                            const float* viewmatrix, const float* campos, const float* dL_dplanes, float* dL_drotations,
                            float* dL_dmeans3D, void* stream) {
  if (const int rc = planes_args(scales, rotations, means3D, P, viewmatrix, campos)) return rc;
  if (P == 0) return 0;
  if (!dL_dplanes || !dL_drotations || !dL_dmeans3D) return fail(GSR_E_BADARG, "NULL argument");
  if (!aligned({dL_dplanes, dL_drotations}, 15u))
    return fail(GSR_E_ALIGN, "dL_dplanes and dL_drotations must be 16-byte aligned");
  if (!aligned({dL_dmeans3D}, 3u)) return fail(GSR_E_ALIGN, "dL_dmeans3D must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned blocks = (unsigned)(((int64_t)P + PL_THREADS - 1) / PL_THREADS);
  hipLaunchKernelGGL(planes_bwd_kernel, dim3(blocks), dim3(PL_THREADS), 0, s, scales,
                     reinterpret_cast<const float4*>(rotations), means3D, P, plane_camera(viewmatrix, campos),
                     reinterpret_cast<const float4*>(dL_dplanes), reinterpret_cast<float4*>(dL_drotations), dL_dmeans3D);
  return check(false, s, "gaussian_planes_bwd");
}

}  // extern "C"
