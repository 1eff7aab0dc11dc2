// TSDF fusion of depth maps into a dense volume and marching-tetrahedra mesh extraction (include/gsr.h, ABI v27;
// DESIGN.md §7.14).  Grid point (i, j, k) is the sample at origin + voxel_size * (i, j, k); linear index
// (k * ny + j) * nx + i, x fastest; fields tsdf / weight [nz,ny,nx] and colour [nz,ny,nx,3].
//
// Launch shape of every kernel here: 256-lane workgroups of 64 x-neighbours times 4 consecutive (j, k) rows, a
// one-dimensional grid of ceil(nx / 64) * ceil(ny nz / 4) workgroups.  A wave reads and writes 256 consecutive bytes of
// a scalar field.  No grid-stride loop and no persistence: a lane that skips its point returns, so a workgroup whose
// points all lie outside the frustum (or hold no surface) ends after a few instructions and the dispatcher balances the
// rest.  No LDS, no atomics, nothing waits on another workgroup.
//
// tsdf_integrate_kernel, per grid point, float32, every operation rounded on its own (the unit is built with
// -ffp-contract=off), M = viewmatrix in the row-vector convention, M[4 * row + col]:
//     p    = (origin.x + voxel_size * i,  origin.y + voxel_size * j,  origin.z + voxel_size * k)
//     x    = ((p.x M[0] + p.y M[4]) + p.z M[8]) + M[12]        y: M[1], M[5], M[9], M[13]      z: M[2], M[6], M[10], M[14]
//     skip unless z > 0.2
//     u    = (fx x) / z + cx,  v = (fy y) / z + cy             cx = (W - 1) / 2, cy = (H - 1) / 2, fx, fy from the host
//     px   = floorf(u + 0.5),  py = floorf(v + 0.5)            skip unless 0 <= px < W and 0 <= py < H
//     d    = depth[py, px]                                     skip unless d > 0; skip if d > max_depth
//     sdf  = d - z                                             skip if sdf < -sdf_trunc
//     t    = min(1, sdf / sdf_trunc)
//     tsdf = (tsdf w_old + t w) / (w_old + w)                  colour channel c with image[c, py, px] the same way
//     weight = min(w_old + w, max_weight)
// A skipped point is not written.  A missing max_depth / max_weight arrives as +inf.
//
// Contracted volumes (unbounded scenes; ABI v33).  The Mip-NeRF 360 contraction of a normalised point
// x = (p - center) / radius keeps the unit ball and squeezes the rest of space into the shell 1 < |q| < 2:
//     contract(x) = x for |x| <= 1,   (2 - 1 / |x|) x / |x| otherwise.
// Its inverse on |q| < 2, m = |q|:   m <= 1: s = 1, g = 1;   m > 1: s = 1 / ((2 - m) m), g = 1 / (2 - m);
//     p = center + radius * (q * s).
// A contracted volume is the same GsrTsdfVolume with its grid in contracted space, q = origin + voxel_size * (i, j, k),
// and a GsrTsdfContraction { center, radius > 0, 1 < q_max < 2 }; sdf_trunc is in world units, as it applies inside the
// unit ball.  tsdf_integrate_kernel<*, true> puts in front of the sequence above, per grid point:
//     q    = origin + voxel_size * (i, j, k)                   (multiply, then add, per axis)
//     m2   = (q.x q.x + q.y q.y) + q.z q.z                     skip unless m2 < q_max q_max: the first test, before any load
//     m    = sqrtf(m2);  s, g as above                         (m <= 1 is the identity branch: q = 0 divides by nothing)
//     p    = center + radius * (q * s)                         (per axis: q s, times radius, plus center)
//     trunc = sdf_trunc * g                                    (2DGS: the truncation grows as 1 / (2 - m))
// and goes on from p with trunc in the place of sdf_trunc.  With center 0, radius 1 and every |q| <= 1 it is the plain
// kernel bit for bit.  The mesh is extracted on the grid by the kernels below, which cannot tell the difference;
// contract_points_inverse_kernel then maps every vertex row q -> center + radius * (q * s) in place, one lane per row,
// with the same s, so a vertex that coincides with a grid point lands on the point the integration projected.
//
// Mesh extraction, marching tetrahedra on the Kuhn decomposition.  Cube corner c = x + 2 y + 4 z.  The six tetrahedra
// around the diagonal 0 -- 7, in the order of the axis permutations xyz, xzy, yxz, yzx, zxy, zyx, each written
// positively oriented (det [v1 - v0, v2 - v0, v3 - v0] > 0; the odd permutations have their middle corners swapped):
//     (0,1,3,7) (0,5,1,7) (0,3,2,7) (0,2,6,7) (0,4,5,7) (0,6,4,7)
// Every edge of a tetrahedron runs from a corner to a componentwise larger one, so it is one of the seven directions
// (1,0,0) (0,1,0) (0,0,1) (1,1,0) (0,1,1) (1,0,1) (1,1,1) of the grid point at its lower end, which owns it.
// Case table (local vertex n of the tetrahedron inside <=> bit n; an edge is the pair of its local ends), derived by
// hand from one rule.  One vertex A on its own side: the others (B, C, D) with B the lowest and (A, B, C, D) an even
// permutation of (0,1,2,3); the triangle is (AB, AC, AD) when A is inside and (AB, AD, AC) when A is outside.  Two
// inside, P < Q, and (R, S) the outside pair ordered so that (P, Q, R, S) is even: (PR, PS, QS), (PR, QS, QR).  With a
// positively oriented tetrahedron the normals then point from inside to outside.
//   * tsdf_cube_kernel: triangles of the cube based at each grid point (0 unless all eight weights >= min_weight).
//   * tsdf_edge_kernel: the 7-bit mask of owned edges that carry a vertex -- crossed (exactly one end has tsdf < 0) and
//     inside at least one cube that emits triangles -- and its population count.
//   * exclusive scans of both counts by the caller (plumbing), then
//   * tsdf_emit_vertices_kernel: p_a + (p_b - p_a) * (t_a / (t_a - t_b)), a the owner, colours with the same factor, at
//     vertex_offset[point] + rank of the direction in the mask;
//   * tsdf_emit_faces_kernel: the triangles of cube, tetrahedron, case order at tri_offset[cube], each corner the index
//     of its edge's vertex.  Plain stores to slots fixed by the scans: the same bits from run to run.
#include "gsr_common.h"
#include "gsr_entry.h"

namespace gsr {

namespace {

constexpr int TSDF_X = 64, TSDF_ROWS = 4;

struct TsdfPoint {
  int i, j, k, idx;
};

// the lane's grid point; false: the lane has none
__device__ inline bool tsdf_point(int nx, int ny, int nz, unsigned xchunks, TsdfPoint& p) {
  const unsigned xc = blockIdx.x % xchunks, rb = blockIdx.x / xchunks;
  const long long row = (long long)rb * TSDF_ROWS + threadIdx.y;
  p.i = (int)(xc * TSDF_X + threadIdx.x);
  if (p.i >= nx || row >= (long long)ny * nz) return false;
  p.k = (int)(row / ny);
  p.j = (int)(row - (long long)p.k * ny);
  p.idx = (int)row * nx + p.i;
  return true;
}

// the inverse contraction's scale s and the growth g of the truncation at |q|^2 = m2 (header comment)
__device__ inline void uncontract_scale(float m2, float& s, float& g) {
  const float m = sqrtf(m2);
  if (m <= 1.0f) {
    s = 1.0f;
    g = 1.0f;
  } else {
    s = 1.0f / ((2.0f - m) * m);
    g = 1.0f / (2.0f - m);
  }
}

// CONTRACTED: the grid lives in contracted space (con); otherwise con is not read
template <bool COLOR, bool CONTRACTED>
__global__ __launch_bounds__(TSDF_X* TSDF_ROWS) void tsdf_integrate_kernel(GsrTsdfVolume vol, GsrTsdfContraction con,
                                                                            GsrTsdfView view, unsigned xchunks) {
  TsdfPoint p;
  if (!tsdf_point(vol.nx, vol.ny, vol.nz, xchunks, p)) return;
  const float* __restrict__ M = view.viewmatrix;
  float wx = vol.origin[0] + vol.voxel_size * (float)p.i;
  float wy = vol.origin[1] + vol.voxel_size * (float)p.j;
  float wz = vol.origin[2] + vol.voxel_size * (float)p.k;
  float trunc = vol.sdf_trunc;
  if constexpr (CONTRACTED) {
    const float m2 = (wx * wx + wy * wy) + wz * wz;
    if (!(m2 < con.q_max * con.q_max)) return;
    float s, g;
    uncontract_scale(m2, s, g);
    wx = con.center[0] + con.radius * (wx * s);
    wy = con.center[1] + con.radius * (wy * s);
    wz = con.center[2] + con.radius * (wz * s);
    trunc = vol.sdf_trunc * g;
  }
  const float z = ((wx * M[2] + wy * M[6]) + wz * M[10]) + M[14];
  if (!(z > 0.2f)) return;
  const float x = ((wx * M[0] + wy * M[4]) + wz * M[8]) + M[12];
  const float y = ((wx * M[1] + wy * M[5]) + wz * M[9]) + M[13];
  const float W = (float)view.width, H = (float)view.height;
  const float u = (view.fx * x) / z + (W - 1.0f) * 0.5f;
  const float v = (view.fy * y) / z + (H - 1.0f) * 0.5f;
  const float fpx = floorf(u + 0.5f), fpy = floorf(v + 0.5f);
  if (!(fpx >= 0.0f && fpx < W && fpy >= 0.0f && fpy < H)) return;      // a NaN fails the test
  const size_t pix = (size_t)(int)fpy * (size_t)view.width + (size_t)(int)fpx;
  const float d = view.depth[pix];
  if (!(d > 0.0f) || d > view.max_depth) return;
  const float sdf = d - z;
  if (sdf < -trunc) return;
  const float t = fminf(1.0f, sdf / trunc);
  const float w = view.weight, w_old = vol.weight[p.idx], w_sum = w_old + w;
  vol.tsdf[p.idx] = (vol.tsdf[p.idx] * w_old + t * w) / w_sum;
  if constexpr (COLOR) {
    const size_t plane = (size_t)view.width * (size_t)view.height;
    float* c = vol.color + 3 * (size_t)p.idx;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) c[ch] = (c[ch] * w_old + view.color[ch * plane + pix] * w) / w_sum;
  }
  vol.weight[p.idx] = fminf(w_sum, view.max_weight);
}

constexpr int POINTS_BLOCK = 256;

__global__ __launch_bounds__(POINTS_BLOCK) void contract_points_inverse_kernel(float* __restrict__ xyz, int64_t n,
                                                                               GsrTsdfContraction con) {
  const int64_t row = (int64_t)blockIdx.x * POINTS_BLOCK + threadIdx.x;
  if (row >= n) return;
  float* q = xyz + 3 * row;
  const float qx = q[0], qy = q[1], qz = q[2];
  float s, g;
  uncontract_scale((qx * qx + qy * qy) + qz * qz, s, g);
  q[0] = con.center[0] + con.radius * (qx * s);
  q[1] = con.center[1] + con.radius * (qy * s);
  q[2] = con.center[2] + con.radius * (qz * s);
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------------
__constant__ uint8_t TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 5, 1, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 6, 4, 7}};
__constant__ uint8_t CASE_TRIS[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
// an edge between local vertices a and b is the byte 4 a + b
#define E(a, b) (uint8_t)(4 * (a) + (b))
__constant__ uint8_t CASE_EDGE[16][6] = {
    {0, 0, 0, 0, 0, 0},                                              // 0000
    {E(0, 1), E(0, 2), E(0, 3), 0, 0, 0},                            // 0001  A = 0 inside
    {E(1, 0), E(1, 3), E(1, 2), 0, 0, 0},                            // 0010  A = 1 inside
    {E(0, 2), E(0, 3), E(1, 3), E(0, 2), E(1, 3), E(1, 2)},          // 0011  P, Q, R, S = 0, 1, 2, 3
    {E(2, 0), E(2, 1), E(2, 3), 0, 0, 0},                            // 0100  A = 2 inside
    {E(0, 3), E(0, 1), E(2, 1), E(0, 3), E(2, 1), E(2, 3)},          // 0101  0, 2, 3, 1
    {E(1, 0), E(1, 3), E(2, 3), E(1, 0), E(2, 3), E(2, 0)},          // 0110  1, 2, 0, 3
    {E(3, 0), E(3, 1), E(3, 2), 0, 0, 0},                            // 0111  A = 3 outside
    {E(3, 0), E(3, 2), E(3, 1), 0, 0, 0},                            // 1000  A = 3 inside
    {E(0, 1), E(0, 2), E(3, 2), E(0, 1), E(3, 2), E(3, 1)},          // 1001  0, 3, 1, 2
    {E(1, 2), E(1, 0), E(3, 0), E(1, 2), E(3, 0), E(3, 2)},          // 1010  1, 3, 2, 0
    {E(2, 0), E(2, 3), E(2, 1), 0, 0, 0},                            // 1011  A = 2 outside
    {E(2, 0), E(2, 1), E(3, 1), E(2, 0), E(3, 1), E(3, 0)},          // 1100  2, 3, 0, 1
    {E(1, 0), E(1, 2), E(1, 3), 0, 0, 0},                            // 1101  A = 1 outside
    {E(0, 1), E(0, 3), E(0, 2), 0, 0, 0},                            // 1110  A = 0 outside
    {0, 0, 0, 0, 0, 0}};                                             // 1111
#undef E
// direction index of an edge from the corner difference (bits x, y, z): (1,0,0) (0,1,0) (0,0,1) (1,1,0) (0,1,1) (1,0,1) (1,1,1)
__constant__ uint8_t DIR_OF_BITS[8] = {0, 0, 1, 3, 2, 5, 4, 6};
__constant__ uint8_t BITS_OF_DIR[7] = {1, 2, 4, 3, 6, 5, 7};

__device__ inline int corner_offset(int c, int nx, int ny) {
  return (c & 1) + ((c >> 1) & 1) * nx + ((c >> 2) & 1) * nx * ny;
}

// inside bits of the cube's eight corners; false: the cube is not processed
__device__ inline bool cube_inside_bits(const GsrTsdfVolume& vol, const TsdfPoint& p, float min_weight, unsigned& bits) {
  if (p.i + 1 >= vol.nx || p.j + 1 >= vol.ny || p.k + 1 >= vol.nz) return false;
  bool all = true;
  bits = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int q = p.idx + corner_offset(c, vol.nx, vol.ny);
    all = all && (vol.weight[q] >= min_weight);
    bits |= (vol.tsdf[q] < 0.0f ? 1u : 0u) << c;
  }
  return all;
}

__device__ inline unsigned tet_case(unsigned bits, int t) {
  unsigned m = 0;
#pragma unroll
  for (int n = 0; n < 4; ++n) m |= ((bits >> TET_CORNER[t][n]) & 1u) << n;
  return m;
}

__global__ __launch_bounds__(TSDF_X* TSDF_ROWS) void tsdf_cube_kernel(GsrTsdfVolume vol, float min_weight,
                                                                      unsigned xchunks, uint8_t* __restrict__ tri_count) {
  TsdfPoint p;
  if (!tsdf_point(vol.nx, vol.ny, vol.nz, xchunks, p)) return;
  unsigned bits, n = 0;
  if (cube_inside_bits(vol, p, min_weight, bits) && bits != 0u && bits != 255u) {
#pragma unroll
    for (int t = 0; t < 6; ++t) n += CASE_TRIS[tet_case(bits, t)];
  }
  tri_count[p.idx] = (uint8_t)n;
}

__global__ __launch_bounds__(TSDF_X* TSDF_ROWS) void tsdf_edge_kernel(GsrTsdfVolume vol, unsigned xchunks,
                                                                      const uint8_t* __restrict__ tri_count,
                                                                      uint8_t* __restrict__ edge_mask,
                                                                      uint8_t* __restrict__ vert_count) {
  TsdfPoint p;
  if (!tsdf_point(vol.nx, vol.ny, vol.nz, xchunks, p)) return;
  // emits[o]: the cube based at p - o emits triangles (o = bits x, y, z; p - (1,1,1) shares no owned edge with p)
  unsigned emits = 0;
#pragma unroll
  for (int o = 0; o < 7; ++o) {
    const int ox = o & 1, oy = (o >> 1) & 1, oz = (o >> 2) & 1;
    if (p.i - ox >= 0 && p.j - oy >= 0 && p.k - oz >= 0)
      emits |= (tri_count[p.idx - corner_offset(o, vol.nx, vol.ny)] != 0 ? 1u : 0u) << o;
  }
  unsigned mask = 0;
  if (emits != 0u) {
    const bool in_a = vol.tsdf[p.idx] < 0.0f;
#pragma unroll
    for (int d = 0; d < 7; ++d) {
      const int b = BITS_OF_DIR[d];
      if (p.i + (b & 1) >= vol.nx || p.j + ((b >> 1) & 1) >= vol.ny || p.k + ((b >> 2) & 1) >= vol.nz) continue;
      bool used = false;                       // a cube based at p - o holds the edge when o and the direction share no axis
#pragma unroll
      for (int o = 0; o < 7; ++o) used = used || ((o & b) == 0 && ((emits >> o) & 1u));
      const bool in_b = vol.tsdf[p.idx + corner_offset(b, vol.nx, vol.ny)] < 0.0f;
      if (used && in_a != in_b) mask |= 1u << d;
    }
  }
  edge_mask[p.idx] = (uint8_t)mask;
  vert_count[p.idx] = (uint8_t)__popc(mask);
}

__global__ __launch_bounds__(TSDF_X* TSDF_ROWS) void tsdf_emit_vertices_kernel(GsrTsdfVolume vol, unsigned xchunks,
                                                                               const uint8_t* __restrict__ edge_mask,
                                                                               const int64_t* __restrict__ vert_offs,
                                                                               int64_t V, float* __restrict__ vertices,
                                                                               float* __restrict__ vcolors) {
  TsdfPoint p;
  if (!tsdf_point(vol.nx, vol.ny, vol.nz, xchunks, p)) return;
  const unsigned mask = edge_mask[p.idx];
  if (mask == 0u) return;
  int64_t at = vert_offs[p.idx];
  const float ta = vol.tsdf[p.idx];
  const int ijk[3] = {p.i, p.j, p.k};
  float pa[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) pa[a] = vol.origin[a] + vol.voxel_size * (float)ijk[a];
  for (int d = 0; d < 7; ++d) {
    if (!((mask >> d) & 1u)) continue;
    if (at >= V) return;                       // offsets that do not belong to this mask: never write past the buffer
    const int b = BITS_OF_DIR[d];
    const int q = p.idx + corner_offset(b, vol.nx, vol.ny);
    const float tb = vol.tsdf[q];
    const float s = ta / (ta - tb);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float pb = vol.origin[a] + vol.voxel_size * (float)(ijk[a] + ((b >> a) & 1));
      vertices[3 * at + a] = pa[a] + (pb - pa[a]) * s;
    }
    if (vcolors) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float ca = vol.color[3 * (size_t)p.idx + ch], cb = vol.color[3 * (size_t)q + ch];
        vcolors[3 * at + ch] = ca + (cb - ca) * s;
      }
    }
    ++at;
  }
}

__global__ __launch_bounds__(TSDF_X* TSDF_ROWS) void tsdf_emit_faces_kernel(GsrTsdfVolume vol, unsigned xchunks,
                                                                            const uint8_t* __restrict__ tri_count,
                                                                            const uint8_t* __restrict__ edge_mask,
                                                                            const int64_t* __restrict__ vert_offs,
                                                                            const int64_t* __restrict__ tri_offs,
                                                                            int64_t F, int32_t* __restrict__ faces) {
  TsdfPoint p;
  if (!tsdf_point(vol.nx, vol.ny, vol.nz, xchunks, p)) return;
  if (p.i + 1 >= vol.nx || p.j + 1 >= vol.ny || p.k + 1 >= vol.nz || tri_count[p.idx] == 0) return;
  unsigned bits = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) bits |= (vol.tsdf[p.idx + corner_offset(c, vol.nx, vol.ny)] < 0.0f ? 1u : 0u) << c;
  int64_t at = tri_offs[p.idx];
  for (int t = 0; t < 6; ++t) {
    const unsigned m = tet_case(bits, t);
    const int ntri = CASE_TRIS[m];
    for (int n = 0; n < ntri; ++n, ++at) {
      if (at >= F) return;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int code = CASE_EDGE[m][3 * n + e];
        const int ca = TET_CORNER[t][code >> 2], cb = TET_CORNER[t][code & 3];
        const int lo = ca < cb ? ca : cb, hi = ca < cb ? cb : ca;
        const int q = p.idx + corner_offset(lo, vol.nx, vol.ny);
        const unsigned below = (1u << DIR_OF_BITS[hi - lo]) - 1u;
        faces[3 * at + e] = (int32_t)(vert_offs[q] + __popc((unsigned)edge_mask[q] & below));
      }
    }
  }
}

// All kernels share one launch shape; false when it would exceed 2^32 work-items (then nothing is launched)
bool tsdf_grid_blocks(int nx, int ny, int nz, unsigned* xchunks, unsigned* blocks) {
  const unsigned long long xc = ((unsigned long long)nx + TSDF_X - 1) / TSDF_X;
  const unsigned long long rb = ((unsigned long long)ny * (unsigned long long)nz + TSDF_ROWS - 1) / TSDF_ROWS;
  const unsigned long long b = xc * rb;
  if (b * (TSDF_X * TSDF_ROWS) >= (1ull << 32)) return false;            // HIP's bound on the work-items of a launch
  *xchunks = (unsigned)xc;
  *blocks = (unsigned)b;
  return true;
}

// con: NULL for a world-space volume
void launch_tsdf_integrate(const GsrTsdfVolume& vol, const GsrTsdfContraction* con, const GsrTsdfView& view,
                           hipStream_t s) {
  unsigned xchunks, blocks;
  if (!tsdf_grid_blocks(vol.nx, vol.ny, vol.nz, &xchunks, &blocks)) return;
  const dim3 grid(blocks), block(TSDF_X, TSDF_ROWS);
  const bool color = vol.color && view.color;
  const GsrTsdfContraction c = con ? *con : GsrTsdfContraction{};
  auto kernel = con ? (color ? tsdf_integrate_kernel<true, true> : tsdf_integrate_kernel<false, true>)
                    : (color ? tsdf_integrate_kernel<true, false> : tsdf_integrate_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, s, vol, c, view, xchunks);
}

void launch_contract_points_inverse(float* xyz, int64_t n, const GsrTsdfContraction& con, hipStream_t s) {
  const dim3 grid((unsigned)((n + POINTS_BLOCK - 1) / POINTS_BLOCK)), block(POINTS_BLOCK);
  hipLaunchKernelGGL(contract_points_inverse_kernel, grid, block, 0, s, xyz, n, con);
}

void launch_tsdf_mesh_count(const GsrTsdfVolume& vol, float min_weight, uint8_t* tri_count, uint8_t* edge_mask,
                            uint8_t* vert_count, hipStream_t s) {
  unsigned xchunks, blocks;
  if (!tsdf_grid_blocks(vol.nx, vol.ny, vol.nz, &xchunks, &blocks)) return;
  const dim3 grid(blocks), block(TSDF_X, TSDF_ROWS);
  hipLaunchKernelGGL(tsdf_cube_kernel, grid, block, 0, s, vol, min_weight, xchunks, tri_count);
  hipLaunchKernelGGL(tsdf_edge_kernel, grid, block, 0, s, vol, xchunks, tri_count, edge_mask, vert_count);
}

void launch_tsdf_mesh_emit(const GsrTsdfVolume& vol, const uint8_t* tri_count, const uint8_t* edge_mask,
                           const int64_t* vert_offs, const int64_t* tri_offs, int64_t V, int64_t F, float* vertices,
                           float* vcolors, int32_t* faces, hipStream_t s) {
  unsigned xchunks, blocks;
  if (!tsdf_grid_blocks(vol.nx, vol.ny, vol.nz, &xchunks, &blocks)) return;
  const dim3 grid(blocks), block(TSDF_X, TSDF_ROWS);
  hipLaunchKernelGGL(tsdf_emit_vertices_kernel, grid, block, 0, s, vol, xchunks, edge_mask, vert_offs, V, vertices,
                     vcolors);
  hipLaunchKernelGGL(tsdf_emit_faces_kernel, grid, block, 0, s, vol, xchunks, tri_count, edge_mask, vert_offs, tri_offs,
                     F, faces);
}

}  // namespace

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

static int tsdf_volume_ok(const GsrTsdfVolume* v) {
  if (!v) return fail(GSR_E_BADARG, "volume is NULL");
  if (v->nx <= 0 || v->ny <= 0 || v->nz <= 0) return fail(GSR_E_BADARG, "volume dims must be positive");
  // 32-bit indices with seven edge slots per grid point: never wrap
  if ((unsigned long long)v->nx * (unsigned long long)v->ny >= (1ull << 31) ||
      7ull * (unsigned long long)v->nx * (unsigned long long)v->ny * (unsigned long long)v->nz >= (1ull << 31))
    return fail(GSR_E_BADARG, "volume too large: 7 * nx * ny * nz must stay below 2^31");
  unsigned xchunks, blocks;
  if (!tsdf_grid_blocks(v->nx, v->ny, v->nz, &xchunks, &blocks))
    return fail(GSR_E_BADARG, "volume shape needs a launch of 2^32 work-items or more");
  if (!(v->voxel_size > 0.0f) || !(v->sdf_trunc > 0.0f)) return fail(GSR_E_BADARG, "voxel_size and sdf_trunc must be positive");
  if (!v->tsdf || !v->weight) return fail(GSR_E_BADARG, "tsdf / weight is NULL");
  if (!aligned({v->tsdf, v->weight, v->color}, 3u)) return fail(GSR_E_ALIGN, "volume fields must be 4-byte aligned");
  return 0;
}
static int tsdf_view_ok(const GsrTsdfVolume* vol, const GsrTsdfView* view) {
  if (!view) return fail(GSR_E_BADARG, "view is NULL");
  if (!image_shape_ok(view->height, view->width)) return fail(GSR_E_BADARG, "bad image shape");
  if (!view->viewmatrix || !view->depth) return fail(GSR_E_BADARG, "viewmatrix / depth is NULL");
  if ((vol->color != nullptr) != (view->color != nullptr))
    return fail(GSR_E_BADARG, "a colour image is given exactly when the volume has a colour field");
  if (!(view->fx > 0.0f) || !(view->fy > 0.0f) || !(view->weight > 0.0f) || !(view->max_depth > 0.0f) ||
      !(view->max_weight > 0.0f))
    return fail(GSR_E_BADARG, "fx, fy, weight, max_depth and max_weight must be positive (+inf: no limit)");
  if (!aligned({view->viewmatrix, view->depth, view->color}, 3u)) return fail(GSR_E_ALIGN, "view arrays must be 4-byte aligned");
  return 0;
}
static int tsdf_contraction_ok(const GsrTsdfContraction* c) {
  if (!c) return fail(GSR_E_BADARG, "contraction is NULL");
  const auto finite = [](float v) { return v - v == 0.0f; };             // false for NaN and +-inf
  if (!finite(c->center[0]) || !finite(c->center[1]) || !finite(c->center[2]))
    return fail(GSR_E_BADARG, "the contraction's center must be finite");
  if (!(c->radius > 0.0f) || !finite(c->radius)) return fail(GSR_E_BADARG, "the contraction's radius must be positive and finite");
  if (!(c->q_max > 1.0f && c->q_max < 2.0f)) return fail(GSR_E_BADARG, "q_max must lie in (1, 2)");
  return 0;
}
int gsr_tsdf_integrate(const GsrTsdfVolume* vol, const GsrTsdfView* view, void* stream) {
  if (int rc = tsdf_volume_ok(vol)) return rc;
  if (int rc = tsdf_view_ok(vol, view)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_tsdf_integrate(*vol, nullptr, *view, s);
  return check(false, s, "tsdf_integrate");
}
int gsr_tsdf_integrate_contracted(const GsrTsdfVolume* vol, const GsrTsdfContraction* contraction, const GsrTsdfView* view,
                                  void* stream) {
  if (int rc = tsdf_volume_ok(vol)) return rc;
  if (int rc = tsdf_contraction_ok(contraction)) return rc;
  if (int rc = tsdf_view_ok(vol, view)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_tsdf_integrate(*vol, contraction, *view, s);
  return check(false, s, "tsdf_integrate_contracted");
}
int gsr_tsdf_uncontract_points(float* xyz, int64_t n, const GsrTsdfContraction* contraction, void* stream) {
  if (int rc = tsdf_contraction_ok(contraction)) return rc;
  if (n < 0 || n >= ((int64_t)1 << 31)) return fail(GSR_E_BADARG, "n must lie in 0 .. 2^31 - 1");
  if (n == 0) return 0;
  if (!xyz) return fail(GSR_E_BADARG, "xyz is NULL");
  if (!aligned({xyz}, 3u)) return fail(GSR_E_ALIGN, "xyz must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_contract_points_inverse(xyz, n, *contraction, s);
  return check(false, s, "tsdf_uncontract_points");
}
int gsr_tsdf_mesh_count(const GsrTsdfVolume* vol, float min_weight, uint8_t* tri_count, uint8_t* edge_mask,
                        uint8_t* vert_count, void* stream) {
  if (int rc = tsdf_volume_ok(vol)) return rc;
  if (!tri_count || !edge_mask || !vert_count) return fail(GSR_E_BADARG, "NULL argument");
  if (min_weight != min_weight) return fail(GSR_E_BADARG, "min_weight is NaN");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_tsdf_mesh_count(*vol, min_weight, tri_count, edge_mask, vert_count, s);
  return check(false, s, "tsdf_mesh_count");
}
int gsr_tsdf_mesh_emit(const GsrTsdfVolume* vol, const uint8_t* tri_count, const uint8_t* edge_mask,
                       const int64_t* vert_offs, const int64_t* tri_offs, int64_t V, int64_t F, float* vertices,
                       float* vcolors, int32_t* faces, void* stream) {
  if (int rc = tsdf_volume_ok(vol)) return rc;
  if (!tri_count || !edge_mask || !vert_offs || !tri_offs || !vertices || !faces) return fail(GSR_E_BADARG, "NULL argument");
  if (vcolors && !vol->color) return fail(GSR_E_BADARG, "vertex colours need a volume with a colour field");
  const int64_t N = (int64_t)vol->nx * vol->ny * vol->nz;
  if (V <= 0 || F <= 0 || V > 7 * N || F > 12 * N) return fail(GSR_E_BADARG, "V must lie in 1..7 N and F in 1..12 N");
  if (!aligned({vert_offs, tri_offs}, 7u)) return fail(GSR_E_ALIGN, "offsets must be 8-byte aligned");
  if (!aligned({vertices, vcolors, faces}, 3u)) return fail(GSR_E_ALIGN, "outputs must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_tsdf_mesh_emit(*vol, tri_count, edge_mask, vert_offs, tri_offs, V, F, vertices, vcolors, faces, s);
  return check(false, s, "tsdf_mesh_emit");
}

}  // extern "C"
