// The walk the map kernels of a rendered frame share (depth.hip, features.hip, distortion.hip, median.hip,
// contribution.hip): one 256-lane workgroup per tile in the colour pass's tile order, one lane per pixel, the tile's
// list staged in LDS in rounds of MAP_CHUNK entries, every lane walking up to ITS n_contrib.
//
// Every map must take the colour pass's alpha >= 1/255 decisions and its running T bit for bit.  That property lives
// HERE, once: the staging of an entry (load_entry), the forward alpha (map_alpha), the back-to-front step
// (map_bwd_test, map_bwd_advance, map_bwd_dalpha), the geometry terms and the flush into acc[P][8].  The alpha itself is the colour
// pass's (render_pair.h, which render.hip includes alone).  The loops stay in the .hip files: they differ (median leaves
// early, contribution walks to a per-wave bound and honours a mask, features has a second grid dimension).
#pragma once
#include "gsr_common.h"
#include "render_pair.h"

namespace gsr {

constexpr int MAP_CHUNK = 256;      // list entries staged per round: one per lane of the workgroup
constexpr int MAP_GEOM = 6;         // per-entry geometry sums of a backward (geom_terms); a seventh, where present, is d z

// ---- the lane's pixel and its tile's list ---------------------------------------------------------------------------
struct MapPixel {
  int tile, px, py;
  bool inside;              // the pixel lies in the image
  size_t pix;               // py * W + px
  uint32_t start, len;      // the tile's list: point_list[start .. start + len)
};

__device__ __forceinline__ MapPixel map_pixel(int W, int H, int grid_x, const uint32_t* tile_order, const uint2* ranges) {
  MapPixel m;
  const int tid = threadIdx.x;
  m.tile = __builtin_amdgcn_readfirstlane((int)tile_order[blockIdx.x]);
  const int tile_x = m.tile % grid_x, tile_y = m.tile / grid_x;
  m.px = tile_x * TILE + (tid & (TILE - 1));
  m.py = tile_y * TILE + tid / TILE;
  m.inside = m.px < W && m.py < H;
  m.pix = (size_t)m.py * W + m.px;
  const uint2 range = ranges[m.tile];
  m.start = range.x;
  m.len = range.y - range.x;
  return m;
}

// how far the pixel walks: the prefix the colour pass composited (takes_part: the kernel's own say, m.inside at least)
__device__ __forceinline__ uint32_t map_last(const MapPixel& m, const uint32_t* n_contrib, bool takes_part) {
  return takes_part ? min(n_contrib[m.pix], m.len) : 0u;
}

// largest of the four waves' values over the workgroup.  v must be uniform over the wave (a wave_reduce_* result); every
// lane calls it (it holds a barrier), and s4 must not be written again before the workgroup's next barrier
__device__ inline uint32_t block_max_of_waves(uint32_t v, uint32_t* s4) {
  if ((threadIdx.x & (WAVE - 1)) == 0) s4[threadIdx.x / WAVE] = v;
  __syncthreads();
  return max(max(s4[0], s4[1]), max(s4[2], s4[3]));
}
// largest value of v over the workgroup's 256 lanes (every lane calls it)
__device__ inline uint32_t block_max_u32(uint32_t v, uint32_t* s4) { return block_max_of_waves(wave_reduce_max_u32(v), s4); }

// ---- a staged list entry ---------------------------------------------------------------------------------------------
// the words of a list entry's Gaussian that the maps need, and the colour pass's LDS image of them.  A lane that stages
// nothing in a round keeps the zeros (and never flushes)
struct MapEntry {
  LdsRec lr;
  float cxx = 0.0f, cxy = 0.0f, cyy = 0.0f, opacity = 0.0f;
  uint32_t id = 0u;
};

__device__ inline MapEntry load_entry(const GeomRec* __restrict__ rec, uint32_t id) {
  const GeomRec* r = rec + id;
  Staged st;
  st.q0 = make_float4(r->x, r->y, r->cxx, 0.0f);
  st.q1 = make_float4(0.0f, r->opacity, 0.0f, 0.0f);
  st.q2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  st.kk = r->kk;
  st.isyy = r->isyy;
  MapEntry e;
  make_lds(st, e.lr);
  e.cxx = r->cxx; e.cxy = r->cxy; e.cyy = r->cyy; e.opacity = r->opacity;
  e.id = id;
  return e;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
// the colour pass's alpha of (entry, pixel) from the entry's LDS image; the caller tests alpha >= ALPHA_MIN and updates
// T with the colour pass's single fma, T = fma(-alpha, T, T)
__device__ __forceinline__ float map_alpha(const float4 a, const float4 b, float pxf, float pyf) {
  return clamp_alpha(__builtin_amdgcn_exp2f(pair_p2(a.x - pxf, a.y - pyf, a.z, a.w, b.x, b.y)), b.x);
}

// ---- backward: back to front from the pixel's final T -----------------------------------------------------------------
// Upstream's recurrence with the entry's channel values c and no background: with g the incoming gradient of the
// pixel's channels, U = (sum over the entries behind of (c . g) w) / T,
//    D = c . g - U,   dL/dalpha = T D,   U <- U + alpha D.
struct MapStep {
  bool ok;             // the pixel composited the entry
  float dx, dy;        // mean - pixel
  float arm, am;       // opacity * G and the clamped alpha; both 0 where !ok
};

// One entry, one pixel, in two halves around the caller's skip.  map_bwd_test: reached = the entry lies inside the
// pixel's prefix; leaves opacity * G in arm.  The caller then skips an entry none of its wave's pixels composited,
//    if (__builtin_amdgcn_ballot_w64(st.ok) == 0ull) continue;
// (the skip is the caller's: it is control flow of ITS loop), and map_bwd_advance takes T to the transmittance in front of
// the entry.  Lanes the entry does not reach run the same instructions on alpha = 0: T stays, every sum gets zero.
__device__ __forceinline__ MapStep map_bwd_test(const float4 a, const float4 b, float pxf, float pyf, bool reached) {
  const float dx = a.x - pxf, dy = a.y - pyf;
  const float ar = __builtin_amdgcn_exp2f(pair_p2(dx, dy, a.z, a.w, b.x, b.y));      // opacity * G
  return MapStep{reached && ar >= ALPHA_MIN, dx, dy, ar, 0.0f};      // (the clamp is above the threshold: same test on either)
}
__device__ __forceinline__ void map_bwd_advance(MapStep& s, const float4 b, float& T) {
  s.arm = s.ok ? s.arm : 0.0f;
  s.am = clamp_alpha(s.arm, b.x);
  T = T / (1.0f - s.am);
}

// h = opacity G dL/dalpha of the entry whose channel values give cg = c . g; steps U
__device__ __forceinline__ float map_bwd_dalpha(const MapStep& s, float T, float cg, float& U) {
  const float Dv = cg - U;
  const float h = s.arm * T * Dv;      // the clamp passes the gradient on, as in the colour backward
  U = __builtin_fmaf(s.am, Dv, U);
  return h;
}

// the pixel's terms of  sum h dx, sum h dy, sum h dx^2, sum h dx dy, sum h dy^2, sum h      (d = mean - pixel)
__device__ __forceinline__ void geom_terms(float h, float dx, float dy, float* v) {
  v[0] = h * dx; v[1] = h * dy; v[2] = v[0] * dx; v[3] = v[0] * dy; v[4] = v[1] * dy; v[5] = h;
}

// one sum of entry k over the tile's pixels: across the wave with shuffles, across the four waves in LDS
__device__ __forceinline__ void map_add_sum(float v, float* slot, int lane) {
  const float s = wave_reduce_add_f32(v);
  if (lane == 0) atomicAdd(slot, s);
}
template <int N>
__device__ __forceinline__ void map_add_sums(const float (&v)[N], float (*sSum)[MAP_CHUNK], uint32_t k, int lane) {
#pragma unroll
  for (int q = 0; q < N; ++q) map_add_sum(v[q], &sSum[q][k], lane);
}

// The lane that staged entry e turns its N (6, or 7 with d z) sums into d mean2D (pixels), d conic, d opacity (and d z)
// and issues one float atomic add per quantity into the entry's row of acc[P][8], the layout aux_geom_bwd_kernel reads.
// An entry whose sums are all zero (either sign) costs no atomic.
template <int N>
__device__ __forceinline__ void map_flush_acc(const float (*sSum)[MAP_CHUNK], int tid, const MapEntry& e, float* acc) {
  static_assert(N == MAP_GEOM || N == MAP_GEOM + 1, "six geometry sums, and d z or not");
  float s[N];
  uint32_t bits = 0u;
#pragma unroll
  for (int q = 0; q < N; ++q) { s[q] = sSum[q][tid]; bits |= __float_as_uint(s[q]); }
  if ((bits << 1) != 0u) {
    float* row = acc + 8 * (size_t)e.id;
    atomicAdd(row + 0, -(e.cxx * s[0] + e.cxy * s[1]));      // d mean2D, pixel units
    atomicAdd(row + 1, -(e.cxy * s[0] + e.cyy * s[1]));
    atomicAdd(row + 2, -0.5f * s[2]);                        // d conic xx, xy (true derivative), yy
    atomicAdd(row + 3, -s[3]);
    atomicAdd(row + 4, -0.5f * s[4]);
    atomicAdd(row + 5, s[5] / e.opacity);                    // d opacity
    if (N > MAP_GEOM) atomicAdd(row + 6, s[N - 1]);          // d z
  }
}

}  // namespace gsr
