// csrc/filter3d_math.h -- the bodies of the kernels of csrc/filter3d.hip -- built by the host compiler and run over a case
// that tests/test_filter3d_host.py writes: the sampling pass and the width must be those of the float32 restatement
// (tests/filter3d_restate.py) bit for bit, the application and its gradient within one float32 place of the float64 one.
// Stand-alone: it may be built with -fsanitize=address,undefined and run directly.
//
//   filter3d_host_check <case file>  ->  line 1: none_seen; then per Gaussian one line of 12 hex words
//       min_depth max_rate seen filter  s'_0 s'_1 s'_2 o'  ds_0 ds_1 ds_2 do
//
// The file, little endian: int32 P, V, rule; float near, margin, variance, focal_max; per view int32 width, height, float
// fx, fy, float[16] world_to_view; then P rows of three floats (xyz); then P rows of nine floats: s[3], o, f, g_s[3], g_o
// (f < 0: use the filter the sampling pass computed for the row).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "filter3d_math.h"

namespace {

template <typename T>
bool get(FILE* f, T* out, size_t n) {
  return fread(out, sizeof(T), n, f) == n;
}

uint32_t bits(float v) {
  uint32_t u;
  memcpy(&u, &v, sizeof u);
  return u;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t head[3];
  float scalars[4];
  if (!get(f, head, 3) || !get(f, scalars, 4) || head[0] < 0 || head[1] < 0) return 4;
  const int32_t P = head[0], V = head[1], rule = head[2];
  const float near = scalars[0], margin = scalars[1], variance = scalars[2], focal_max = scalars[3];
  std::vector<GsrFilterView> views((size_t)V);
  for (int32_t v = 0; v < V; ++v) {
    int32_t wh[2];
    float focal[2];
    GsrFilterView& view = views[(size_t)v];
    if (!get(f, wh, 2) || !get(f, focal, 2) || !get(f, view.world_to_view, 16)) return 5;
    view.width = wh[0];
    view.height = wh[1];
    view.fx = focal[0];
    view.fy = focal[1];
  }
  std::vector<float> xyz(3 * (size_t)P), rows(9 * (size_t)P);
  if (!get(f, xyz.data(), xyz.size()) || !get(f, rows.data(), rows.size())) return 6;
  fclose(f);
  std::vector<float> min_depth((size_t)P), max_rate((size_t)P);
  std::vector<int> seen((size_t)P);
  float D = -INFINITY, R = INFINITY;
  for (int32_t i = 0; i < P; ++i) {
    const float* p = &xyz[3 * (size_t)i];
    float d = INFINITY, r = 0.0f;
    int hit = 0;
    for (int32_t v = 0; v < V; ++v) hit |= (int)gsr::filter3d_view_sample(views[(size_t)v], p[0], p[1], p[2], near, margin, d, r);
    min_depth[(size_t)i] = d;
    max_rate[(size_t)i] = r;
    seen[(size_t)i] = hit;
    if (hit) {
      D = fmaxf(D, d);
      R = fminf(R, r);
    }
  }
  const bool any = D > -INFINITY, paper = rule == GSR_FILTER3D_PAPER;
  printf("%d\n", any ? 0 : 1);
  for (int32_t i = 0; i < P; ++i) {
    const size_t k = (size_t)i;
    const float filter = !any ? 0.0f
                              : gsr::filter3d_width(rule, seen[k] != 0, paper ? max_rate[k] : min_depth[k], paper ? R : D,
                                                    focal_max, variance);
    const float* row = &rows[9 * k];
    const float fa = row[4] < 0.0f ? filter : row[4];
    float so[3], oo, ds[3], dop;
    gsr::filter3d_apply_row(row, row[3], fa, so, &oo);
    gsr::filter3d_apply_bwd_row(row, row[3], fa, row + 5, row[8], ds, &dop);
    printf("%08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x %08x\n", bits(min_depth[k]), bits(max_rate[k]),
           (unsigned)seen[k], bits(filter), bits(so[0]), bits(so[1]), bits(so[2]), bits(oo), bits(ds[0]), bits(ds[1]),
           bits(ds[2]), bits(dop));
  }
  return 0;
}
