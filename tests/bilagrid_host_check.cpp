// csrc/bilagrid_math.h built by a host compiler, as a program of its own: tests/test_bilagrid_host.py writes an input
// file, runs it and reads the results, so that the arithmetic of csrc/bilagrid.hip is checked against the restatement
// without a GPU (and once under the address and undefined-behaviour sanitizers).
//
//   bilagrid_host_check IN OUT
//   IN:  int32 H, W, Wg, Hg, L; float32 x[3 H W], grid[12 L Hg Wg], g[3 H W]
//   OUT: float32 y[3 H W], dx[3 H W], dgrid[12 L Hg Wg]
//
// y and dx are the per-pixel functions the kernels call; dgrid is gathered by grid vertex over bg_vertex_range with the
// weights the kernel uses, in double, rounded once (the order of the sum is the program's own).
#include "bilagrid_math.h"
#include <stdint.h>
#include <stdio.h>
#include <vector>

using namespace gsr;

static bool read_all(FILE* f, void* p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 3;
  int32_t head[5];
  if (!read_all(in, head, sizeof head)) return 4;
  const BilagridShape s = {head[0], head[1], head[2], head[3], head[4]};
  if (s.H < 1 || s.W < 1 || (int64_t)s.H * s.W > (1 << 24) || !bilagrid_shape_ok(s.Wg, s.Hg, s.L)) return 5;
  const size_t pixels = (size_t)s.H * (size_t)s.W, cells = (size_t)s.L * s.Hg * s.Wg;
  std::vector<float> x(3 * pixels), grid(BG_TERMS * cells), g(3 * pixels);
  if (!read_all(in, x.data(), 4 * x.size()) || !read_all(in, grid.data(), 4 * grid.size()) ||
      !read_all(in, g.data(), 4 * g.size()))
    return 6;
  fclose(in);
  std::vector<float> y(3 * pixels), dx(3 * pixels), dgrid(BG_TERMS * cells);
  for (int py = 0; py < s.H; ++py)
    for (int px = 0; px < s.W; ++px) {
      const size_t p = (size_t)py * s.W + px;
      const float X[3] = {x[p], x[pixels + p], x[2 * pixels + p]}, gv[3] = {g[p], g[pixels + p], g[2 * pixels + p]};
      BilagridPixel pix;
      bg_pixel(X, px, py, s, pix);
      double A[BG_TERMS], dA_dz[BG_TERMS];
      bg_slice(grid.data(), s, pix, A, dA_dz);
      float Y[3], dX[3];
      bg_apply(A, X, Y);
      bg_image_grad(A, dA_dz, X, gv, pix.dz_dgray, dX);
      for (int c = 0; c < 3; ++c) {
        y[c * pixels + p] = Y[c];
        dx[c * pixels + p] = dX[c];
      }
    }
  for (int vj = 0; vj < s.Hg; ++vj)
    for (int vi = 0; vi < s.Wg; ++vi) {
      int x_lo, x_hi, y_lo, y_hi;
      bg_vertex_range(vi, s.W, s.Wg, x_lo, x_hi);
      bg_vertex_range(vj, s.H, s.Hg, y_lo, y_hi);
      std::vector<double> acc((size_t)s.L * BG_TERMS, 0.0);
      for (int py = y_lo; py <= y_hi; ++py) {
        int j0;
        double tv;
        bg_cell(bg_axis_coord(py, s.H, s.Hg), s.Hg, j0, tv);
        const double wy = bg_axis_weight(j0, tv, vj);
        if (wy == 0.0) continue;
        for (int px = x_lo; px <= x_hi; ++px) {
          const size_t p = (size_t)py * s.W + px;
          const float X[3] = {x[p], x[pixels + p], x[2 * pixels + p]}, gv[3] = {g[p], g[pixels + p], g[2 * pixels + p]};
          BilagridPixel pix;
          bg_pixel(X, px, py, s, pix);
          for (int level = 0; level < s.L; ++level) {
            const double w = (bg_axis_weight(pix.i0, pix.tu, vi) * wy) * bg_axis_weight(pix.l0, pix.tz, level);
            if (w != 0.0) bg_grid_terms(X, gv, w, &acc[(size_t)level * BG_TERMS]);
          }
        }
      }
      for (int level = 0; level < s.L; ++level)
        for (int t = 0; t < BG_TERMS; ++t)
          dgrid[(size_t)t * cells + ((size_t)level * s.Hg + vj) * s.Wg + vi] = (float)acc[(size_t)level * BG_TERMS + t];
    }
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 7;
  const bool ok = fwrite(y.data(), 4, y.size(), out) == y.size() && fwrite(dx.data(), 4, dx.size(), out) == dx.size() &&
                  fwrite(dgrid.data(), 4, dgrid.size(), out) == dgrid.size();
  return fclose(out) == 0 && ok ? 0 : 8;
}
