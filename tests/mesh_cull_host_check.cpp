// csrc/mesh_cull_math.h -- the body of mesh_view_counts_kernel -- built by the host compiler and run over a scene that
// tests/test_mesh_cull_host.py writes: the counts must be those of the float32 restatement (tests/mesh_cull_restate.py)
// bit for bit.  Stand-alone: it may be built with -fsanitize=address,undefined and run directly.
//
//   mesh_cull_host_check <scene file>  ->  one line "in_view visible" per vertex
//
// The file, little endian: int32 V, S; float near, depth_tol; per view int32 width, height, has_mask, has_depth, float fx,
// fy, float[16] world_to_view, then width height mask bytes if has_mask, then width height depth floats if has_depth;
// then V rows of three floats.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mesh_cull_math.h"

namespace {

template <typename T>
bool get(FILE* f, T* out, size_t n) {
  return fread(out, sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t VS[2];
  float scalars[2];
  if (!get(f, VS, 2) || !get(f, scalars, 2) || VS[0] < 0 || VS[1] < 0) return 4;
  const int32_t V = VS[0], S = VS[1];
  std::vector<GsrCullView> views((size_t)S);
  std::vector<std::vector<uint8_t>> masks((size_t)S);
  std::vector<std::vector<float>> depths((size_t)S);
  for (int32_t s = 0; s < S; ++s) {
    int32_t head[4];
    float focal[2];
    GsrCullView& view = views[(size_t)s];
    if (!get(f, head, 4) || !get(f, focal, 2) || !get(f, view.world_to_view, 16) || head[0] < 1 || head[1] < 1) return 5;
    view.width = head[0];
    view.height = head[1];
    view.fx = focal[0];
    view.fy = focal[1];
    const size_t n = (size_t)head[0] * (size_t)head[1];
    view.mask = nullptr;
    view.depth = nullptr;
    if (head[2]) {
      masks[(size_t)s].resize(n);
      if (!get(f, masks[(size_t)s].data(), n)) return 6;
      view.mask = masks[(size_t)s].data();
    }
    if (head[3]) {
      depths[(size_t)s].resize(n);
      if (!get(f, depths[(size_t)s].data(), n)) return 7;
      view.depth = depths[(size_t)s].data();
    }
  }
  std::vector<float> vertices(3 * (size_t)V);
  if (!get(f, vertices.data(), vertices.size())) return 8;
  fclose(f);
  for (int32_t i = 0; i < V; ++i) {
    const float* p = &vertices[3 * (size_t)i];
    int n_in = 0, n_vis = 0;
    for (int32_t s = 0; s < S; ++s) {
      const int r = gsr::cull_view_test(views[(size_t)s], p[0], p[1], p[2], scalars[0], scalars[1]);
      n_in += r & gsr::CULL_IN_VIEW;
      n_vis += (r & gsr::CULL_VISIBLE) >> 1;
    }
    printf("%d %d\n", n_in, n_vis);
  }
  return 0;
}
