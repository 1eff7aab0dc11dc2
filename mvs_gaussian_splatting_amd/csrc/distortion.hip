// Depth-distortion map of a rendered frame (the regulariser of 2DGS), with gradients.
//
//   dist = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2,   w_i = alpha_i T_i,   m_i = m(z_i)
//   m(z) = z                                 mapping 0 ("linear")
//   m(z) = far / (far - near) (1 - near / z)  mapping 1 (the NDC depth 2DGS uses)
//
// over the list entries the colour pass composited at the pixel -- the entries of depth.hip (§7.9): the first
// n_contrib[pixel] entries of the tile's list whose alpha passes the 1/255 test, alpha evaluated with the colour pass's own
// functions (render_pair.h) and T updated with its single fma, so the decisions and the running T come out bit for bit.
// z_i is BinInfo::depth.  No background term; a pixel with zero or one contributor is exactly 0.
//
// In exact arithmetic dist = A M2 - M1^2 (A = sum w, M1 = sum w m, M2 = sum w m^2), but in float32 that subtraction cancels
// whenever the pixel's contributors lie in a thin slab -- the state the loss drives towards.  Both kernels therefore
// carry differences of m only.  Forward, per composited entry, with d = m_i - m_prev (0 at the first entry):
//     Q += d (2 S + d A);   S += d A;   dist += w_i Q;   A += w_i
// where S_i = sum_{j<i} w_j (m_i - m_j) and Q_i = sum_{j<i} w_j (m_i - m_j)^2; the identities hold for either sign of d.
//
// state [2,H,W], written by the forward for the backward (opaque to the caller), with cover = 1 - T_final:
//     state[0] = S_end / cover = m_last - mbar      (mbar = M1 / A; 0 without a contributor)
//     state[1] = dist / cover                       (0 without a contributor)
// Backward, back to front: r_k = m_k - mbar starts at state[0] and steps by r <- r - (m_next - m_k);
//     d dist / d w_k = E_k = A r_k^2 + dist / A,      d dist / d m_k = 2 w_k A r_k,
// and dL/dalpha_k is the recurrence of aux_maps_bwd_kernel with g E_k as the entry's channel value.  Every quantity
// is of the order of the contributors' spread, never of m itself.
//
// Nothing of the colour path or of depth.hip is read-modified; the backward's sums go into a zeroed [P,8] accumulator in
// the layout aux_geom_bwd_kernel reads (word 6 is d z).  Nothing waits on another workgroup.
//
// Built with the flags of depth.o; the arithmetic that has to match the colour pass, and the recurrences, are explicit fma.
#include "gsr_common.h"
#include "gsr_launch.h"
#include "render_pair.h"

namespace gsr {

constexpr int DIST_CHUNK = 256;     // list entries staged per round: one per lane of the workgroup
constexpr int DIST_SUMS = 7;        // per-entry sums of the backward (those of aux_maps_bwd_kernel)

struct DistEntry {
  LdsRec lr;
  float m, dm, cxx, cxy, cyy, opacity;      // m(z) and m'(z)
  uint32_t id;
};

// the words of a list entry's Gaussian that the map needs, and the colour pass's LDS image of them
__device__ inline void dist_load_entry(const GeomRec* __restrict__ rec, const BinInfo* __restrict__ bin, uint32_t id,
                                       int mapping, float near, float scale, DistEntry& e) {
  const GeomRec* r = rec + id;
  Staged st;
  st.q0 = make_float4(r->x, r->y, r->cxx, 0.0f);
  st.q1 = make_float4(0.0f, r->opacity, 0.0f, 0.0f);
  st.q2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  st.kk = r->kk;
  st.isyy = r->isyy;
  make_lds(st, e.lr);
  e.cxx = r->cxx; e.cxy = r->cxy; e.cyy = r->cyy; e.opacity = r->opacity;
  const float z = bin[id].depth;
  if (mapping == 0) {
    e.m = z;
    e.dm = 1.0f;
  } else {      // scale = far / (far - near)
    const float iz = 1.0f / z;
    e.m = scale * (1.0f - near * iz);
    e.dm = scale * near * iz * iz;
  }
  e.id = id;
}

// largest value of v over the workgroup's 256 lanes (every lane calls it)
__device__ inline uint32_t dist_block_max_u32(uint32_t v, uint32_t* s4) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0) s4[threadIdx.x / WAVE] = v;
  __syncthreads();
  return max(max(s4[0], s4[1]), max(s4[2], s4[3]));
}

// ------------------------------------------------------------------------------------------------------------------
// Forward: one 256-lane workgroup per tile (the colour pass's tile order), one lane per pixel.  A round stages up to 256
// entries in LDS; every lane then walks the round's entries in list order up to ITS n_contrib.  No atomics: the map is
// the same bits from run to run.  A tile with an empty list writes zeros.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DIST_CHUNK) void distortion_fwd_kernel(int W, int H, int grid_x,
                                                                    const uint32_t* __restrict__ tile_order,
                                                                    const uint2* __restrict__ ranges,
                                                                    const uint32_t* __restrict__ point_list,
                                                                    const GeomRec* __restrict__ rec,
                                                                    const BinInfo* __restrict__ bin,
                                                                    const uint32_t* __restrict__ n_contrib, int mapping,
                                                                    float near, float scale, float* __restrict__ dist,
                                                                    float* __restrict__ state) {
  __shared__ float4 sA[DIST_CHUNK];
  __shared__ float4 sB[DIST_CHUNK];
  __shared__ float sM[DIST_CHUNK];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int tile = __builtin_amdgcn_readfirstlane((int)tile_order[blockIdx.x]);
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const int px = tile_x * TILE + (tid & (TILE - 1)), py = tile_y * TILE + tid / TILE;
  const bool inside = px < W && py < H;
  const size_t pix = (size_t)py * W + px, HW = (size_t)W * H;
  const float pxf = (float)px, pyf = (float)py;
  const uint2 range = ranges[tile];
  const uint32_t start = range.x, len = range.y - range.x;
  const uint32_t last = inside ? min(n_contrib[pix], len) : 0u;
  const uint32_t tmax = dist_block_max_u32(last, sMax);

  float T = 1.0f, A = 0.0f, S = 0.0f, Q = 0.0f, D = 0.0f, mp = 0.0f;
  bool first = true;
  for (uint32_t base = 0; base < tmax; base += DIST_CHUNK) {
    const uint32_t n = min((uint32_t)DIST_CHUNK, tmax - base);
    if ((uint32_t)tid < n) {
      DistEntry e;
      dist_load_entry(rec, bin, point_list[start + base + tid], mapping, near, scale, e);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sM[tid] = e.m;
    }
    __syncthreads();
    const uint32_t mine = last > base ? min(n, last - base) : 0u;
    for (uint32_t k = 0; k < mine; ++k) {
      const float4 a = sA[k], b = sB[k];
      const float alpha = clamp_alpha(__builtin_amdgcn_exp2f(pair_p2(a.x - pxf, a.y - pyf, a.z, a.w, b.x, b.y)), b.x);
      if (alpha >= ALPHA_MIN) {
        const float m = sM[k];
        const float w = alpha * T;
        const float d = first ? 0.0f : m - mp;
        Q = __builtin_fmaf(d, __builtin_fmaf(d, A, 2.0f * S), Q);      // Q += d (2 S + d A), with the S and A of j < i
        S = __builtin_fmaf(d, A, S);
        D = __builtin_fmaf(w, Q, D);
        A += w;
        mp = m;
        first = false;
        T = __builtin_fmaf(-alpha, T, T);      // T (1 - alpha), rounded once: the colour pass's update
      }
    }
    __syncthreads();
  }
  if (inside) {
    const float cover = 1.0f - T;      // the alpha map of depth.hip; the backward forms the same number from final_T
    const bool any = cover > 0.0f;
    dist[pix] = D;
    state[pix] = any ? S / cover : 0.0f;
    state[HW + pix] = any ? D / cover : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Backward: same grid and staging, back to front from the pixel's final T (final_T of the frame).  With g the incoming
// gradient of the pixel, A = 1 - final_T and r_k = m_k - mbar (header comment), the entry's "channel value" is
//    c_k = g E_k = g (A r_k^2 + dist / A),   U = (sum over the entries behind of c w) / T,
//    D = c_k - U,   dL/dalpha_k = T_k D,   U <- U + alpha_k D,
// and dL/dz_k = g 2 w_k A r_k m'(z_k).  Per entry the seven sums over the tile's pixels
//    sum h dx, sum h dy, sum h dx^2, sum h dx dy, sum h dy^2, sum h, sum dL/dz      (h = opacity G dL/dalpha, d = mean - pixel)
// are added across the wave with shuffles and across the four waves in LDS; the lane that staged the entry turns them into
// d mean2D (pixels), d conic, d opacity and d z and issues one float atomic add per quantity into acc[P][8].  A wave none
// of whose pixels the entry reaches skips the entry.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DIST_CHUNK) void distortion_bwd_kernel(int W, int H, int grid_x,
                                                                    const uint32_t* __restrict__ tile_order,
                                                                    const uint2* __restrict__ ranges,
                                                                    const uint32_t* __restrict__ point_list,
                                                                    const GeomRec* __restrict__ rec,
                                                                    const BinInfo* __restrict__ bin,
                                                                    const uint32_t* __restrict__ n_contrib,
                                                                    const float* __restrict__ final_T, int mapping,
                                                                    float near, float scale,
                                                                    const float* __restrict__ state,
                                                                    const float* __restrict__ dL_ddist,
                                                                    float* __restrict__ acc) {
  __shared__ float4 sA[DIST_CHUNK];
  __shared__ float4 sB[DIST_CHUNK];
  __shared__ float2 sM[DIST_CHUNK];      // m, m'
  __shared__ float sSum[DIST_SUMS][DIST_CHUNK];
  __shared__ uint32_t sMax[4];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int tile = __builtin_amdgcn_readfirstlane((int)tile_order[blockIdx.x]);
  const int tile_x = tile % grid_x, tile_y = tile / grid_x;
  const int px = tile_x * TILE + (tid & (TILE - 1)), py = tile_y * TILE + tid / TILE;
  const bool inside = px < W && py < H;
  const size_t pix = (size_t)py * W + px, HW = (size_t)W * H;
  const float pxf = (float)px, pyf = (float)py;
  const uint2 range = ranges[tile];
  const uint32_t start = range.x, len = range.y - range.x;
  const uint32_t last = inside ? min(n_contrib[pix], len) : 0u;
  const uint32_t tmax = dist_block_max_u32(last, sMax);
  float T = inside ? final_T[pix] : 0.0f;
  const float A = inside ? 1.0f - T : 0.0f;
  const float g = inside ? dL_ddist[pix] : 0.0f;
  const float E0 = inside ? state[HW + pix] : 0.0f;      // dist / A
  float r = inside ? state[pix] : 0.0f;                  // m_k - mbar of the entry last visited
  float mn = 0.0f;                                       // its m
  bool seen = false;
  float U = 0.0f;

  uint32_t hi = tmax;
  while (hi > 0) {
    const uint32_t lo = hi > (uint32_t)DIST_CHUNK ? hi - DIST_CHUNK : 0u;
    const uint32_t n = hi - lo;
    DistEntry e;
    e.cxx = e.cxy = e.cyy = e.opacity = 0.0f;
    e.id = 0u;
    if ((uint32_t)tid < n) {
      dist_load_entry(rec, bin, point_list[start + lo + tid], mapping, near, scale, e);
      sA[tid] = e.lr.A;
      sB[tid] = e.lr.B;
      sM[tid] = make_float2(e.m, e.dm);
    }
#pragma unroll
    for (int q = 0; q < DIST_SUMS; ++q) sSum[q][tid] = 0.0f;
    __syncthreads();
    for (uint32_t k = n; k-- > 0;) {
      const float4 a = sA[k], b = sB[k];
      const float dx = a.x - pxf, dy = a.y - pyf;
      const float ar = __builtin_amdgcn_exp2f(pair_p2(dx, dy, a.z, a.w, b.x, b.y));      // opacity * G
      const bool ok = lo + k < last && ar >= ALPHA_MIN;      // (the clamp is above the threshold: same test on either)
      if (__builtin_amdgcn_ballot_w64(ok) == 0ull) continue;      // uniform over the wave
      const float2 mz = sM[k];
      // lanes the entry does not reach run the same instructions on alpha = 0: T, U and r stay, every sum gets zero
      const float arm = ok ? ar : 0.0f;
      const float am = clamp_alpha(arm, b.x);
      r -= (ok && seen) ? mn - mz.x : 0.0f;                  // the first entry visited is the last composited: r = state[0]
      mn = ok ? mz.x : mn;
      seen = seen || ok;
      T = T / (1.0f - am);                                   // transmittance in front of this entry
      const float Ar = A * r;
      const float cg = g * __builtin_fmaf(Ar, r, E0);
      const float Dv = cg - U;
      const float h = arm * T * Dv;                          // the clamp passes the gradient on, as in the colour backward
      U = __builtin_fmaf(am, Dv, U);
      float v[DIST_SUMS];
      v[0] = h * dx; v[1] = h * dy; v[2] = v[0] * dx; v[3] = v[0] * dy; v[4] = v[1] * dy; v[5] = h;
      v[6] = am * T * (2.0f * g * Ar * mz.y);
#pragma unroll
      for (int q = 0; q < DIST_SUMS; ++q) {
        const float s = wave_reduce_add_f32(v[q]);
        if (lane == 0) atomicAdd(&sSum[q][k], s);
      }
    }
    __syncthreads();
    if ((uint32_t)tid < n) {
      float s[DIST_SUMS];
      uint32_t bits = 0u;
#pragma unroll
      for (int q = 0; q < DIST_SUMS; ++q) { s[q] = sSum[q][tid]; bits |= __float_as_uint(s[q]); }
      if ((bits << 1) != 0u) {
        float* row = acc + 8 * (size_t)e.id;
        atomicAdd(row + 0, -(e.cxx * s[0] + e.cxy * s[1]));      // d mean2D, pixel units
        atomicAdd(row + 1, -(e.cxy * s[0] + e.cyy * s[1]));
        atomicAdd(row + 2, -0.5f * s[2]);                        // d conic xx, xy (true derivative), yy
        atomicAdd(row + 3, -s[3]);
        atomicAdd(row + 4, -0.5f * s[4]);
        atomicAdd(row + 5, s[5] / e.opacity);                    // d opacity
        atomicAdd(row + 6, s[6]);                                // d z
      }
    }
    __syncthreads();
    hi = lo;
  }
}

void launch_distortion_fwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const GeomRec* rec,
                           const BinInfo* bin, const uint32_t* n_contrib, const uint32_t* tile_order, int mapping,
                           float near, float far, float* dist, float* state, hipStream_t s) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const float scale = mapping ? far / (far - near) : 1.0f;
  hipLaunchKernelGGL(distortion_fwd_kernel, dim3(gx * gy), dim3(DIST_CHUNK), 0, s, W, H, gx, tile_order, ranges, point_list,
                     rec, bin, n_contrib, mapping, near, scale, dist, state);
}

void launch_distortion_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const GeomRec* rec,
                           const BinInfo* bin, const uint32_t* n_contrib, const float* final_T, const uint32_t* tile_order,
                           int mapping, float near, float far, const float* state, const float* dL_ddist, float* acc,
                           hipStream_t s) {
  const int gx = (W + TILE - 1) / TILE, gy = (H + TILE - 1) / TILE;
  const float scale = mapping ? far / (far - near) : 1.0f;
  hipLaunchKernelGGL(distortion_bwd_kernel, dim3(gx * gy), dim3(DIST_CHUNK), 0, s, W, H, gx, tile_order, ranges, point_list,
                     rec, bin, n_contrib, final_T, mapping, near, scale, state, dL_ddist, acc);
}

}  // namespace gsr
