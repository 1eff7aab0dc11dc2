// csrc/planes_math.h built by a host compiler: the loops tests/test_planes_host.py calls through ctypes, so that the
// arithmetic of csrc/planes.hip and csrc/plane_depth.hip is checked against the restatement without a GPU.
#include "planes_math.h"
#include <stddef.h>

using namespace gsr;

static PlaneCamera camera(const float* viewmatrix, const float* campos) {
  PlaneCamera cam;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) cam.v[3 * i + j] = viewmatrix[4 * i + j];
    cam.campos[i] = campos[i];
  }
  return cam;
}

extern "C" {

void planes_fwd(const float* scales, const float* rot, const float* means, int P, const float* viewmatrix,
                const float* campos, float* planes) {
  const PlaneCamera cam = camera(viewmatrix, campos);
  for (int i = 0; i < P; ++i) plane_forward(scales + 3 * i, rot + 4 * i, means + 3 * i, cam, planes + 4 * i);
}

void planes_bwd(const float* scales, const float* rot, const float* means, int P, const float* viewmatrix,
                const float* campos, const float* g, float* d_rot, float* d_mean) {
  const PlaneCamera cam = camera(viewmatrix, campos);
  for (int i = 0; i < P; ++i)
    plane_backward(scales + 3 * i, rot + 4 * i, means + 3 * i, cam, g + 4 * i, d_rot + 4 * i, d_mean + 3 * i);
}

void plane_depth(const float* normal, const float* distance, const float* alpha, int H, int W, float fx, float fy,
                 float alpha_min, float min_cos, float* z, float* dz_dD, float* dz_dN) {
  const PlaneDepthCamera cam = {fx, fy, (float)((W - 1.0) * 0.5), (float)((H - 1.0) * 0.5), alpha_min, min_cos};
  const size_t plane = (size_t)H * (size_t)W;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * (size_t)W + (size_t)x;
      const float N[3] = {normal[p], normal[plane + p], normal[2 * plane + p]};
      float g[3];
      plane_depth_pixel(N, distance[p], alpha[p], x, y, cam, z + p, dz_dD + p, g);
      for (int a = 0; a < 3; ++a) dz_dN[a * plane + p] = g[a];
    }
}

}  // extern "C"
