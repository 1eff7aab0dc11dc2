// csrc/depth_prior_math.h -- the fit of depth_prior_fit_kernel and the per-pixel bodies of depth_prior_sums_kernel and
// depth_prior_apply_kernel -- built by the host compiler with the kernel's -ffp-contract=off and run over pixels that
// tests/test_depth_prior_host.py writes: the fit from the given sums, the six terms and the three gradients of every pixel
// must be those of the numpy restatement (tests/depth_prior_restate.py) bit for bit.
// Stand-alone: it may be built with -fsanitize=address,undefined and run directly.
//
//   depth_prior_host_check <file>  ->  line 1: 12 hex words, the float64 bits of DepthPriorFit from the file's sums;
//                                      then per pixel one line: valid (0 / 1), 6 hex words (the float64 bits of the terms,
//                                      zeros on an invalid pixel) and 3 hex words (the float32 bits of the l1, aligned_l1
//                                      and pearson gradients; the fitted ones +0 under a degenerate fit)
//
// The file, little endian: int64 n, double[6] the sums, double scale, double offset, double pixels (the l1 mode's
// denominator), int64 count, then `count` records of float x, y, w.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "depth_prior_math.h"

namespace {

template <typename T>
bool get(FILE* f, T* out, size_t n) {
  return fread(out, sizeof(T), n, f) == n;
}

struct Record {
  float x, y, w;
};
static_assert(sizeof(Record) == 12, "packed as the test writes it");

void put64(double v) {
  uint64_t bits;
  memcpy(&bits, &v, 8);
  printf(" %016" PRIx64, bits);
}

void put32(float v) {
  uint32_t bits;
  memcpy(&bits, &v, 4);
  printf(" %08" PRIx32, bits);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int64_t n, count;
  double S[gsr::DEPTH_PRIOR_SUMS], affine[3];
  if (!get(f, &n, 1) || !get(f, S, gsr::DEPTH_PRIOR_SUMS) || !get(f, affine, 3) || !get(f, &count, 1) || count < 0) return 4;
  std::vector<Record> records((size_t)count);
  if (!get(f, records.data(), records.size())) return 5;
  fclose(f);
  gsr::DepthPriorFit fit;
  gsr::depth_prior_fit((long long)n, S, fit);
  const double words[gsr::DEPTH_PRIOR_FIT_WORDS] = {fit.n,  fit.Sw, fit.mx, fit.my, fit.vx, fit.vy,
                                                    fit.cov, fit.sd, fit.s,  fit.t,  fit.r,  fit.degenerate};
  printf("fit");
  for (int k = 0; k < gsr::DEPTH_PRIOR_FIT_WORDS; ++k) put64(words[k]);
  printf("\n");
  const bool live = fit.degenerate == 0.0;
  for (const Record& p : records) {
    const bool valid = gsr::depth_prior_valid(p.x, p.y, p.w);
    double t[gsr::DEPTH_PRIOR_SUMS] = {0, 0, 0, 0, 0, 0};
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (valid) {
      gsr::depth_prior_terms(p.x, p.y, p.w, t);
      g[0] = gsr::depth_prior_grad_l1(gsr::depth_prior_residual(p.x, p.y, affine[0], affine[1]), p.w, affine[2]);
      if (live) {
        g[1] = gsr::depth_prior_grad_l1(gsr::depth_prior_residual(p.x, p.y, fit.s, fit.t), p.w, fit.Sw);
        g[2] = gsr::depth_prior_grad_pearson(p.x, p.y, p.w, fit);
      }
    }
    printf("%d", valid ? 1 : 0);
    for (int k = 0; k < gsr::DEPTH_PRIOR_SUMS; ++k) put64(t[k]);
    for (int k = 0; k < 3; ++k) put32(g[k]);
    printf("\n");
  }
  return 0;
}
