// The per-row arithmetic of csrc/planes.hip and the per-pixel arithmetic of csrc/plane_depth.hip (include/gsr.h, ABI v37;
// DESIGN.md §7.24), as functions a host compiler takes too: tests/planes_host_check.cpp is the host build, which
// tests/test_planes_host.py holds to the GPU test's bar.  Inputs and outputs are float32; every intermediate is a
// double and each output is rounded once, on its store.  Both kernels move 50 to 70 bytes per lane for a few dozen
// flops, so the double arithmetic is hidden behind the memory traffic, and the outputs are the float64 restatement's
// (tests/planes_restate.py) rounded to float32.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSR_HD __host__ __device__ inline
#else
#define GSR_HD inline
#endif

namespace gsr {

// viewmatrix[:3,:3] (row-vector convention: n_view = n_world @ V, row-major) and the camera centre
struct PlaneCamera {
  float v[9];
  float campos[3];
};

// What both directions decide and build from one row: the unit quaternion, 1 / max(|rot|, 1e-12) and whether the
// clamp acted, the flattest axis, the facing sign and the signed world-space normal.
struct PlaneRow {
  double q[4];      // r, x, y, z
  double inv_norm;
  bool clamped;
  int axis;
  double sign;
  double n[3];      // sign * R[:, axis]
  double to_cam[3]; // campos - mean
};

GSR_HD void plane_row(const float s[3], const float rot[4], const float mean[3], const PlaneCamera& cam, PlaneRow& o) {
  const double r0 = rot[0], r1 = rot[1], r2 = rot[2], r3 = rot[3];
  const double norm = sqrt(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3);
  o.clamped = norm < 1e-12;
  o.inv_norm = 1.0 / (o.clamped ? 1e-12 : norm);
  const double r = r0 * o.inv_norm, x = r1 * o.inv_norm, y = r2 * o.inv_norm, z = r3 * o.inv_norm;
  o.q[0] = r; o.q[1] = x; o.q[2] = y; o.q[3] = z;
  int a = 0;                                       // torch.argmin: the smallest index among equals
  if (s[1] < s[a]) a = 1;
  if (s[2] < s[a]) a = 2;
  o.axis = a;
  double c0, c1, c2;                               // R[:, a] of features._rotation_matrices
  if (a == 0) {
    c0 = 1.0 - 2.0 * (y * y + z * z); c1 = 2.0 * (x * y + r * z); c2 = 2.0 * (x * z - r * y);
  } else if (a == 1) {
    c0 = 2.0 * (x * y - r * z); c1 = 1.0 - 2.0 * (x * x + z * z); c2 = 2.0 * (y * z + r * x);
  } else {
    c0 = 2.0 * (x * z + r * y); c1 = 2.0 * (y * z - r * x); c2 = 1.0 - 2.0 * (x * x + y * y);
  }
  for (int i = 0; i < 3; ++i) o.to_cam[i] = (double)cam.campos[i] - (double)mean[i];
  const double facing = (c0 * o.to_cam[0] + c1 * o.to_cam[1]) + c2 * o.to_cam[2];
  o.sign = facing < 0.0 ? -1.0 : 1.0;              // exactly 0 keeps +1
  o.n[0] = o.sign * c0; o.n[1] = o.sign * c1; o.n[2] = o.sign * c2;
}

// planes row = (n_w @ V, n_w . (campos - mean))
GSR_HD void plane_forward(const float s[3], const float rot[4], const float mean[3], const PlaneCamera& cam,
                          float out[4]) {
  PlaneRow p;
  plane_row(s, rot, mean, cam, p);
  for (int j = 0; j < 3; ++j)
    out[j] = (float)((p.n[0] * (double)cam.v[j] + p.n[1] * (double)cam.v[3 + j]) + p.n[2] * (double)cam.v[6 + j]);
  out[3] = (float)((p.n[0] * p.to_cam[0] + p.n[1] * p.to_cam[1]) + p.n[2] * p.to_cam[2]);
}

// g = dL/dplanes row -> dL/drotations row (through the matrix column and the normalisation) and dL/dmeans3D row
GSR_HD void plane_backward(const float s[3], const float rot[4], const float mean[3], const PlaneCamera& cam,
                           const float g[4], float d_rot[4], float d_mean[3]) {
  PlaneRow p;
  plane_row(s, rot, mean, cam, p);
  const double gd = g[3];
  double G[3];                                     // dL/dR[:, axis]
  for (int i = 0; i < 3; ++i) {
    const double gn = ((double)cam.v[3 * i] * (double)g[0] + (double)cam.v[3 * i + 1] * (double)g[1]) +
                      (double)cam.v[3 * i + 2] * (double)g[2];
    G[i] = p.sign * (gn + gd * p.to_cam[i]);
    d_mean[i] = (float)(-(gd * p.n[i]));
  }
  const double r = p.q[0], x = p.q[1], y = p.q[2], z = p.q[3];
  double dq[4];
  if (p.axis == 0) {
    dq[0] = 2.0 * (z * G[1] - y * G[2]);
    dq[1] = 2.0 * (y * G[1] + z * G[2]);
    dq[2] = 2.0 * (x * G[1] - r * G[2]) - 4.0 * y * G[0];
    dq[3] = 2.0 * (r * G[1] + x * G[2]) - 4.0 * z * G[0];
  } else if (p.axis == 1) {
    dq[0] = 2.0 * (x * G[2] - z * G[0]);
    dq[1] = 2.0 * (y * G[0] + r * G[2]) - 4.0 * x * G[1];
    dq[2] = 2.0 * (x * G[0] + z * G[2]);
    dq[3] = 2.0 * (y * G[2] - r * G[0]) - 4.0 * z * G[1];
  } else {
    dq[0] = 2.0 * (y * G[0] - x * G[1]);
    dq[1] = 2.0 * (z * G[0] - r * G[1]) - 4.0 * x * G[2];
    dq[2] = 2.0 * (r * G[0] + z * G[1]) - 4.0 * y * G[2];
    dq[3] = 2.0 * (x * G[0] + y * G[1]);
  }
  // q = rot / max(|rot|, 1e-12): under the clamp the divisor is a constant
  const double qdq = p.clamped ? 0.0 : ((r * dq[0] + x * dq[1]) + y * dq[2]) + z * dq[3];
  for (int k = 0; k < 4; ++k) d_rot[k] = (float)((dq[k] - p.q[k] * qdq) * p.inv_norm);
}

struct PlaneDepthCamera {
  float fx, fy, cx, cy, alpha_min, min_cos;
};

// One pixel: z = D / c with c = -(N . r), r = ((x - cx) / fx, (y - cy) / fy, 1), on a valid pixel, and the unit
// gradients dz/dD = 1 / c, dz/dN = (D / c^2) r.  Returns false, and zeros, on a pixel that is not valid: alpha <
// alpha_min, D <= 0, c <= 0 or c < min_cos |N| |r|, an input that is not finite, or a result float32 cannot hold.
GSR_HD bool plane_depth_pixel(const float N[3], float D, float alpha, int px, int py, const PlaneDepthCamera& cam,
                              float* z, float* dz_dD, float dz_dN[3]) {
  *z = 0.0f;
  *dz_dD = 0.0f;
  dz_dN[0] = dz_dN[1] = dz_dN[2] = 0.0f;
  const double FMAX = 3.4028234663852886e38;
  const double n0 = N[0], n1 = N[1], n2 = N[2], d = D, a = alpha;
  // NaN fails every comparison; +-inf fails the bound
  if (!(fabs(n0) <= FMAX && fabs(n1) <= FMAX && fabs(n2) <= FMAX && fabs(d) <= FMAX && fabs(a) <= FMAX)) return false;
  if (!(a >= (double)cam.alpha_min) || !(d > 0.0)) return false;
  const double rx = ((double)px - (double)cam.cx) / (double)cam.fx, ry = ((double)py - (double)cam.cy) / (double)cam.fy;
  const double c = -((n0 * rx + n1 * ry) + n2);
  const double nn = (n0 * n0 + n1 * n1) + n2 * n2, rr = (rx * rx + ry * ry) + 1.0;
  if (!(c > 0.0) || !(c >= (double)cam.min_cos * sqrt(nn * rr))) return false;
  const double inv = 1.0 / c, zz = d * inv, k = zz * inv;
  const double rmax = fmax(1.0, fmax(fabs(rx), fabs(ry)));
  if (!(zz <= FMAX && inv <= FMAX && k * rmax <= FMAX)) return false;
  *z = (float)zz;
  *dz_dD = (float)inv;
  dz_dN[0] = (float)(k * rx);
  dz_dN[1] = (float)(k * ry);
  dz_dN[2] = (float)k;
  return true;
}

}  // namespace gsr
