// csrc/mesh_raster_math.h -- the rule of the rasterizing kernels -- built by the host compiler and run over a scene that
// tests/test_mesh_raster_host.py writes: snapped coordinates, coverage and depth bits must be those of the numpy
// restatement (tests/mesh_raster_restate.py) bit for bit.  Stand-alone: it may be built with -fsanitize=address,undefined
// and run directly.
//
//   mesh_raster_host_check <scene file>
//     -> per piece, in face order   "P face status X0 Y0 X1 Y1 X2 Y2 covered keysum"
//        (status 1 ok, 0 no area or culled, -1 dropped; the coordinates after the orientation is normalised, 0 unless ok;
//         covered: the centres it covers; keysum: the sum of their keys modulo 2^64, in hex)
//        then per pixel, row-major  "K key" (hex; all ones where nothing landed)
//
// The file, little endian: int32 V, F, width, height, cull_backfaces; float near, fx, fy; float[16] world_to_view; V rows of
// three floats; F rows of three int32.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mesh_raster_math.h"

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
  int32_t head[5];
  float scalars[3];
  GsrCullView view;
  if (!get(f, head, 5) || !get(f, scalars, 3) || !get(f, view.world_to_view, 16)) return 4;
  const int32_t V = head[0], F = head[1];
  if (V < 0 || F < 0 || head[2] < 1 || head[3] < 1 || head[2] > 16384 || head[3] > 16384) return 5;
  view.mask = nullptr;
  view.depth = nullptr;
  view.width = head[2];
  view.height = head[3];
  view.fx = scalars[1];
  view.fy = scalars[2];
  const bool cull = head[4] != 0;
  const float near = scalars[0];
  std::vector<float> vertices(3 * (size_t)V);
  std::vector<int32_t> faces(3 * (size_t)F);
  if (!get(f, vertices.data(), vertices.size()) || !get(f, faces.data(), faces.size())) return 6;
  fclose(f);
  std::vector<uint64_t> keys((size_t)view.width * (size_t)view.height, ~(uint64_t)0);
  for (int32_t i = 0; i < F; ++i) {
    const int32_t* row = &faces[3 * (size_t)i];
    if (row[0] < 0 || row[0] >= V || row[1] < 0 || row[1] >= V || row[2] < 0 || row[2] >= V) return 7;
    gsr::RasterVert o[4];
    const int n = gsr::raster_face(view, &vertices[3 * (size_t)row[0]], &vertices[3 * (size_t)row[1]],
                                   &vertices[3 * (size_t)row[2]], near, o);
    for (int k = 0; k + 3 <= n; ++k) {
      gsr::RasterPiece p;
      const int status = gsr::raster_setup(view, o[0], o[1 + k], o[2 + k], cull, p);
      long covered = 0;
      uint64_t keysum = 0;
      if (status == gsr::RASTER_PIECE_OK) {
        for (int32_t iy = p.y0; iy <= p.y1; ++iy)
          for (int32_t ix = p.x0; ix <= p.x1; ++ix) {
            float z;
            if (!gsr::raster_cover(p, ix, iy, z)) continue;
            const uint64_t key = gsr::raster_key(z, (uint32_t)i);
            uint64_t& slot = keys[(size_t)iy * (size_t)view.width + (size_t)ix];
            slot = key < slot ? key : slot;
            ++covered;
            keysum += key;
          }
        printf("P %d 1 %d %d %d %d %d %d %ld %llx\n", i, p.X[0], p.Y[0], p.X[1], p.Y[1], p.X[2], p.Y[2], covered,
               (unsigned long long)keysum);
      } else {
        printf("P %d %d 0 0 0 0 0 0 0 0\n", i, status);
      }
    }
  }
  for (uint64_t key : keys) printf("K %llx\n", (unsigned long long)key);
  return 0;
}
