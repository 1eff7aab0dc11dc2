// Per-Gaussian feature vectors F[P,C] composited to C-channel maps of a rendered frame, with gradients.
//
//   feat[c] = sum_i w_i F[id_i, c],   w_i = alpha_i T_i,   c = 0 .. C-1      (no background term, no clamp)
//
// over the list entries the colour pass composited at the pixel -- the entries of depth.hip (§7.9): the first
// n_contrib[pixel] entries of the tile's list whose alpha passes the 1/255 test, alpha evaluated with the colour pass's own
// functions (render_pair.h) and T updated with its single fma, so the decisions and the running T come out bit for bit.
//
// Channels are processed in groups of FEAT_GROUP in the grid's second dimension: a workgroup composites its tile for its
// group's slice of the rows of F.  The last group is predicated (no read past a row's end, no write past channel C-1).
// Nothing of the colour path or of depth.hip is read-modified; the backward's geometry sums go into a zeroed [P,8]
// accumulator in the layout aux_geom_bwd_kernel reads (word 6, d z, stays 0: a feature does not depend on the depth).
//
// Built with the flags of depth.o; the compositing arithmetic that has to match the colour pass is explicit fma.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "render_pair.h"

namespace gsr {

constexpr int FEAT_CHUNK = 256;     // list entries staged per round: one per lane of the workgroup
constexpr int FEAT_GROUP = 8;       // channels per workgroup: two float4 of LDS per staged entry
constexpr int FEAT_GEOM = 6;        // per-entry geometry sums of the backward

struct FeatEntry {
  LdsRec lr;
  float cxx, cxy, cyy, opacity;
  uint32_t id;
};

// the words of a list entry's Gaussian that the maps need, and the colour pass's LDS image of them
__device__ inline void feat_load_entry(const GeomRec* __restrict__ rec, uint32_t id, FeatEntry& e) {
  const GeomRec* r = rec + id;
  Staged st;
  st.q0 = make_float4(r->x, r->y, r->cxx, 0.0f);
  st.q1 = make_float4(0.0f, r->opacity, 0.0f, 0.0f);
  st.q2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  st.kk = r->kk;
  st.isyy = r->isyy;
  make_lds(st, e.lr);
  e.cxx = r->cxx; e.cxy = r->cxy; e.cyy = r->cyy; e.opacity = r->opacity;
  e.id = id;
}

// channels [c0, c0 + FEAT_GROUP) of row id of F, zero past the row's end
__device__ inline void feat_load_row(const float* __restrict__ F, int C, int c0, uint32_t id, float (&f)[FEAT_GROUP]) {
  const float* row = F + (size_t)id * (size_t)C;
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; ++j) f[j] = c0 + j < C ? row[c0 + j] : 0.0f;
}

// largest value of v over the workgroup's 256 lanes (every lane calls it)
__device__ inline uint32_t feat_block_max_u32(uint32_t v, uint32_t* s4) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0) s4[threadIdx.x / WAVE] = v;
  __syncthreads();
  return max(max(s4[0], s4[1]), max(s4[2], s4[3]));
}

// ------------------------------------------------------------------------------------------------------------------
// Forward: grid (tiles, channel groups).  One 256-lane workgroup per tile in the colour pass's tile order, one lane per
// pixel; a round stages up to 256 entries (the colour pass's LDS image and the group's slice of the F row); every lane
// walks the round's entries in list order up to ITS n_contrib.  No atomics: the map is the same bits from run to run.
// T is updated with the colour pass's single fma, so 1 - T at the end is 1 - final_T of the frame bit for bit.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FEAT_CHUNK) void feature_maps_fwd_kernel(int W, int H, int grid_x,
                                                                      const uint32_t* __restrict__ tile_order,
                                                                      const uint2* __restrict__ ranges,
                                                                      const uint32_t* __restrict__ point_list,
                                                                      const GeomRec* __restrict__ rec,
                                                                      const uint32_t* __restrict__ n_contrib,
                                                                      const float* __restrict__ F, int C,
                                                                      float* __restrict__ out) {
  __shared__ float4 sA[FEAT_CHUNK];
  __shared__ float4 sB[FEAT_CHUNK];
  __shared__ float4 sF0[FEAT_CHUNK];      // channels c0 .. c0 + 3 of the entry's row
  __shared__ float4 sF1[FEAT_CHUNK];      // channels c0 + 4 .. c0 + 7
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int c0 = (int)blockIdx.y * FEAT_GROUP;
  const int tile = __builtin_amdgcn_readfirstlane((int)tile_order[blockIdx.x]);
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const int px = tile_x * TILE + (tid & (TILE - 1)), py = tile_y * TILE + tid / TILE;
  const bool inside = px < W && py < H;
  const size_t pix = (size_t)py * W + px, HW = (size_t)W * H;
  const float pxf = (float)px, pyf = (float)py;
  const uint2 range = ranges[tile];
  const uint32_t start = range.x, len = range.y - range.x;
  const uint32_t last = inside ? min(n_contrib[pix], len) : 0u;
  const uint32_t tmax = feat_block_max_u32(last, sMax);

  // The sum is taken about the row of the pixel's FIRST composited entry, R:
  //    feat[c] = R[c] (1 - T_final) + sum_i w_i (F[id_i, c] - R[c]),
  // which is sum_i w_i F[id_i, c] because sum_i w_i = 1 - T_final.  The rounding error is that of the plain sum (every
  // term is bounded by w_i times twice the largest |F|), and a field that is constant over the pixel's contributors
  // comes out as that constant times 1 - T_final rounded once: the channel of F = ones is the alpha map bit for bit.
  float T = 1.0f;
  bool first = true;
  float S[FEAT_GROUP], R[FEAT_GROUP];
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; ++j) S[j] = R[j] = 0.0f;
  for (uint32_t base = 0; base < tmax; base += FEAT_CHUNK) {
    const uint32_t n = min((uint32_t)FEAT_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      FeatEntry e;
      feat_load_entry(rec, point_list[start + base + tid], e);
      float f[FEAT_GROUP];
      feat_load_row(F, C, c0, e.id, f);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sF0[tid] = make_float4(f[0], f[1], f[2], f[3]);
      sF1[tid] = make_float4(f[4], f[5], f[6], f[7]);
    }
    __syncthreads();
    const uint32_t mine = last > base ? min(n, last - base) : 0u;
    for (uint32_t k = 0; k < mine; ++k) {
      const float4 a = sA[k], b = sB[k];
      const float alpha = clamp_alpha(__builtin_amdgcn_exp2f(pair_p2(a.x - pxf, a.y - pyf, a.z, a.w, b.x, b.y)), b.x);
      if (alpha >= ALPHA_MIN) {
        const float4 f0 = sF0[k], f1 = sF1[k];
        const float f[FEAT_GROUP] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
        const float w = alpha * T;
#pragma unroll
        for (int j = 0; j < FEAT_GROUP; ++j) {
          R[j] = first ? f[j] : R[j];
          S[j] = __builtin_fmaf(f[j] - R[j], w, S[j]);
        }
        first = false;
        T = __builtin_fmaf(-alpha, T, T);      // T (1 - alpha), rounded once: the colour pass's update
      }
    }
    __syncthreads();
  }
  if (inside) {
    const float cover = 1.0f - T;      // the alpha map of depth.hip: T is the colour pass's final T
#pragma unroll
    for (int j = 0; j < FEAT_GROUP; ++j)
      if (c0 + j < C) out[(size_t)(c0 + j) * HW + pix] = __builtin_fmaf(R[j], cover, S[j]);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward: same grid and staging, back to front from the pixel's final T (final_T of the frame).  The recurrence of
// aux_maps_bwd_kernel with the entry's channel values c_i = F[id_i, c0 .. c0 + 7] and g the incoming gradient of the
// pixel's channels of this group:  U = (sum over the entries behind of (c . g) w) / T,
//    D = c_i . g - U,   dL/dalpha_i = T_i D,   U <- U + alpha_i D.
// dL/dalpha_i is LINEAR in c . g = sum_c F[id_i, c] g[c]: the recurrence run on a subset of the channels gives that
// subset's share of dL/dalpha_i, and the shares of disjoint subsets add up to the whole.  So every channel group runs
// the recurrence on its own channels and adds its six geometry sums
//    sum h dx, sum h dy, sum h dx^2, sum h dx dy, sum h dy^2, sum h      (h = opacity G dL/dalpha, d = mean - pixel)
// into the SAME [P,8] accumulator: that is what makes the grouping legal.  (Word 6, d z, is never written.)
// Per entry and channel, sum over the tile's pixels of w_i g[c] is dL/dF[id_i, c]: one float atomic per
// (entry, tile, channel) into dL_dF [P,C].  All sums are added across the wave with shuffles and across the four waves
// in LDS; the lane that staged the entry issues the global atomics.  A wave none of whose pixels the entry reaches
// skips the entry.  GEOM / FEAT: which of the two sides the caller wants.
// ------------------------------------------------------------------------------------------------------------------
template <bool GEOM, bool FEAT>
__global__ __launch_bounds__(FEAT_CHUNK) void feature_maps_bwd_kernel(int W, int H, int grid_x,
                                                                      const uint32_t* __restrict__ tile_order,
                                                                      const uint2* __restrict__ ranges,
                                                                      const uint32_t* __restrict__ point_list,
                                                                      const GeomRec* __restrict__ rec,
                                                                      const uint32_t* __restrict__ n_contrib,
                                                                      const float* __restrict__ final_T,
                                                                      const float* __restrict__ F, int C,
                                                                      const float* __restrict__ dL_dmaps,
                                                                      float* __restrict__ acc, float* __restrict__ dL_dF) {
  constexpr int NSUM = (GEOM ? FEAT_GEOM : 0) + (FEAT ? FEAT_GROUP : 0);
  constexpr int FEAT0 = GEOM ? FEAT_GEOM : 0;      // first channel sum
  __shared__ float4 sA[FEAT_CHUNK];
  __shared__ float4 sB[FEAT_CHUNK];
  __shared__ float4 sF0[FEAT_CHUNK];
  __shared__ float4 sF1[FEAT_CHUNK];
  __shared__ float sSum[NSUM][FEAT_CHUNK];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int c0 = (int)blockIdx.y * FEAT_GROUP;
  const int nch = min(FEAT_GROUP, C - c0);      // channels of this group that exist
  const int tile = __builtin_amdgcn_readfirstlane((int)tile_order[blockIdx.x]);
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const int px = tile_x * TILE + (tid & (TILE - 1)), py = tile_y * TILE + tid / TILE;
  const bool inside = px < W && py < H;
  const size_t pix = (size_t)py * W + px, HW = (size_t)W * H;
  const float pxf = (float)px, pyf = (float)py;
  const uint2 range = ranges[tile];
  const uint32_t start = range.x, len = range.y - range.x;
  const uint32_t last = inside ? min(n_contrib[pix], len) : 0u;
  const uint32_t tmax = feat_block_max_u32(last, sMax);
  float T = inside ? final_T[pix] : 0.0f;
  float g[FEAT_GROUP];
#pragma unroll
  for (int j = 0; j < FEAT_GROUP; ++j) g[j] = (inside && j < nch) ? dL_dmaps[(size_t)(c0 + j) * HW + pix] : 0.0f;
  float U = 0.0f;

  uint32_t hi = tmax;
  while (hi > 0) {
    const uint32_t lo = hi > (uint32_t)FEAT_CHUNK ? hi - FEAT_CHUNK : 0u;
    const uint32_t n = hi - lo;
    FeatEntry e;
    e.cxx = e.cxy = e.cyy = e.opacity = 0.0f;
    e.id = 0u;
    if ((uint32_t)tid < n) {
      feat_load_entry(rec, point_list[start + lo + tid], e);
      float f[FEAT_GROUP];
      feat_load_row(F, C, c0, e.id, f);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sF0[tid] = make_float4(f[0], f[1], f[2], f[3]);
      sF1[tid] = make_float4(f[4], f[5], f[6], f[7]);
    }
#pragma unroll
    for (int q = 0; q < NSUM; ++q) sSum[q][tid] = 0.0f;
    __syncthreads();
    for (uint32_t k = n; k-- > 0;) {
      const float4 a = sA[k], b = sB[k];
      const float dx = a.x - pxf, dy = a.y - pyf;
      const float ar = __builtin_amdgcn_exp2f(pair_p2(dx, dy, a.z, a.w, b.x, b.y));      // opacity * G
      const bool ok = lo + k < last && ar >= ALPHA_MIN;      // (the clamp is above the threshold: same test on either)
      if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;      // uniform over the wave
      // lanes the entry does not reach run the same instructions on alpha = 0: T and U stay, every sum gets zero
      const float arm = ok ? ar : 0.0f;
      const float am = clamp_alpha(arm, b.x);
      T = T / (1.0f - am);                                   // transmittance in front of this entry
      if (GEOM) {
        const float4 f0 = sF0[k], f1 = sF1[k];
        float cg = f0.x * g[0];
        cg = __builtin_fmaf(f0.y, g[1], cg);
        cg = __builtin_fmaf(f0.z, g[2], cg);
        cg = __builtin_fmaf(f0.w, g[3], cg);
        cg = __builtin_fmaf(f1.x, g[4], cg);
        cg = __builtin_fmaf(f1.y, g[5], cg);
        cg = __builtin_fmaf(f1.z, g[6], cg);
        cg = __builtin_fmaf(f1.w, g[7], cg);
        const float Dv = cg - U;
        const float h = arm * T * Dv;                        // the clamp passes the gradient on, as in the colour backward
        U = __builtin_fmaf(am, Dv, U);
        float v[FEAT_GEOM];
        v[0] = h * dx; v[1] = h * dy; v[2] = v[0] * dx; v[3] = v[0] * dy; v[4] = v[1] * dy; v[5] = h;
#pragma unroll
        for (int q = 0; q < FEAT_GEOM; ++q) {
          const float s = wave_reduce_add_f32(v[q]);
          if (lane == 0) atomicAdd(&sSum[q][k], s);
        }
      }
      if (FEAT) {
        const float w = am * T;
#pragma unroll
        for (int j = 0; j < FEAT_GROUP; ++j) {
          if (j < nch) {      // uniform over the workgroup
            const float s = wave_reduce_add_f32(w * g[j]);
            if (lane == 0) atomicAdd(&sSum[FEAT0 + j][k], s);
          }
        }
      }
    }
    __syncthreads();
    if ((uint32_t)tid < n) {
      if (GEOM) {
        float s[FEAT_GEOM];
        uint32_t bits = 0u;
#pragma unroll
        for (int q = 0; q < FEAT_GEOM; ++q) { s[q] = sSum[q][tid]; bits |= __float_as_uint(s[q]); }
        if ((bits << 1) != 0u) {
          float* row = acc + 8 * (size_t)e.id;
          atomicAdd(row + 0, -(e.cxx * s[0] + e.cxy * s[1]));      // d mean2D, pixel units
          atomicAdd(row + 1, -(e.cxy * s[0] + e.cyy * s[1]));
          atomicAdd(row + 2, -0.5f * s[2]);                        // d conic xx, xy (true derivative), yy
          atomicAdd(row + 3, -s[3]);
          atomicAdd(row + 4, -0.5f * s[4]);
          atomicAdd(row + 5, s[5] / e.opacity);                    // d opacity
        }
      }
      if (FEAT) {
        float* row = dL_dF + (size_t)e.id * (size_t)C + c0;
#pragma unroll
        for (int j = 0; j < FEAT_GROUP; ++j) {
          if (j < nch) {
            const float s = sSum[FEAT0 + j][tid];
            if ((__float_as_uint(s) << 1) != 0u) atomicAdd(row + j, s);
          }
        }
      }
    }
    __syncthreads();
    hi = lo;
  }
}

static inline dim3 feat_grid(int W, int H, int C) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  return dim3(gx * gy, (C + FEAT_GROUP - 1) / FEAT_GROUP);
}

void launch_feature_maps_fwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const GeomRec* rec,
                             const uint32_t* n_contrib, const uint32_t* tile_order, const float* features, int C,
                             float* out, hipStream_t s) {
  const int gx = (W + TILE - 1) / TILE;
  hipLaunchKernelGGL(feature_maps_fwd_kernel, feat_grid(W, H, C), dim3(FEAT_CHUNK), 0, s, W, H, gx, tile_order, ranges,
                     point_list, rec, n_contrib, features, C, out);
}

void launch_feature_maps_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const GeomRec* rec,
                             const uint32_t* n_contrib, const float* final_T, const uint32_t* tile_order,
                             const float* features, int C, const float* dL_dmaps, float* acc, float* dL_dfeatures,
                             hipStream_t s) {
  const int gx = (W + TILE - 1) / TILE;
  const dim3 grid = feat_grid(W, H, C), block(FEAT_CHUNK);
  if (acc && dL_dfeatures)
    hipLaunchKernelGGL((feature_maps_bwd_kernel<true, true>), grid, block, 0, s, W, H, gx, tile_order, ranges, point_list,
                       rec, n_contrib, final_T, features, C, dL_dmaps, acc, dL_dfeatures);
  else if (acc)
    hipLaunchKernelGGL((feature_maps_bwd_kernel<true, false>), grid, block, 0, s, W, H, gx, tile_order, ranges, point_list,
                       rec, n_contrib, final_T, features, C, dL_dmaps, acc, dL_dfeatures);
  else if (dL_dfeatures)
    hipLaunchKernelGGL((feature_maps_bwd_kernel<false, true>), grid, block, 0, s, W, H, gx, tile_order, ranges, point_list,
                       rec, n_contrib, final_T, features, C, dL_dmaps, acc, dL_dfeatures);
}

}  // namespace gsr
