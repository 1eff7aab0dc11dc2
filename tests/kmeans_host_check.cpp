// csrc/kmeans_math.h -- the rule that kmeans_assign_mfma_kernel / kmeans_assign_valu_kernel compute -- built by the host
// compiler with the kernel's -ffp-contract=off and run over points and codes that tests/test_kmeans_host.py writes: the
// chosen index, the best score and dist2 must be those of the numpy restatement (tests/kmeans_restate.py) bit for bit,
// walked three ways: code by code (the vector-ALU kernel's order), with every row padded by zeros to an even D (what the
// matrix-core kernel multiplies), and as two interleaved halves merged at the end (its lanes l and l + 32).
// Stand-alone: it may be built with -fsanitize=address,undefined and run directly.
//
//   kmeans_host_check <file>  ->  per point one line: index, padded index, merged index (decimal), then the float32 bits
//                                 of the best score, of the padded best score and of dist2 (hex)
//
// The file, little endian: int32 N, int32 K, int32 D, float x[N][D], float codebook[K][D].
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kmeans_math.h"

namespace {

uint32_t bits_of(float v) {
  uint32_t b;
  memcpy(&b, &v, 4);
  return b;
}

std::vector<float> padded(const std::vector<float>& a, int n, int D, int DP) {
  std::vector<float> out((size_t)n * DP, 0.0f);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < D; ++k) out[(size_t)i * DP + k] = a[(size_t)i * D + k];
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t h[3];
  if (fread(h, 4, 3, f) != 3 || h[0] < 0 || h[1] < 1 || h[2] < 1 || h[2] > gsr::KMEANS_MAX_D) return 4;
  const int N = h[0], K = h[1], D = h[2], DP = (D + 1) / 2 * 2;
  std::vector<float> x((size_t)N * D), cb((size_t)K * D);
  if (fread(x.data(), 4, x.size(), f) != x.size() || fread(cb.data(), 4, cb.size(), f) != cb.size()) return 5;
  fclose(f);
  const std::vector<float> xp = padded(x, N, D, DP), cbp = padded(cb, K, D, DP);
  std::vector<float> cnorm(K), cnorm_p(K);
  for (int c = 0; c < K; ++c) {
    cnorm[c] = gsr::kmeans_chain(&cb[(size_t)c * D], &cb[(size_t)c * D], D);
    cnorm_p[c] = gsr::kmeans_chain(&cbp[(size_t)c * DP], &cbp[(size_t)c * DP], DP);
  }
  for (int i = 0; i < N; ++i) {
    const float* row = &x[(size_t)i * D];
    float best, best_p;
    const int32_t a = gsr::kmeans_assign_point(row, cb.data(), cnorm.data(), K, D, &best);
    const int32_t b = gsr::kmeans_assign_point(&xp[(size_t)i * DP], cbp.data(), cnorm_p.data(), K, DP, &best_p);
    // codes 8 g + 4 h + j of every 32 belong to half h, as in the accumulator tile
    float part[2] = {__builtin_inff(), __builtin_inff()};
    int32_t part_i[2] = {0, 0};
    for (int32_t c = 0; c < K; ++c) {
      const int half = (c >> 2) & 1;
      gsr::kmeans_take(gsr::kmeans_score(gsr::kmeans_chain(row, &cb[(size_t)c * D], D), cnorm[c]), c, &part[half],
                       &part_i[half]);
    }
    gsr::kmeans_merge(part[1], part_i[1], &part[0], &part_i[0]);
    const float d2 = gsr::kmeans_dist2(gsr::kmeans_chain(row, row, D), best);
    printf("%d %d %d %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", a, b, part_i[0], bits_of(best), bits_of(best_p),
           bits_of(d2));
  }
  return 0;
}
