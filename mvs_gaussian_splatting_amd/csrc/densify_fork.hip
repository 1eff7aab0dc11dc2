// The fork's densification (scene/gaussian_model.py:751-773): the clone + split branch with the learned tensors
// (:509-610) and the grow branch (densify_and_grow :612-677, densify_and_growsplit :679-749), then the prune, as one plan
// and one read-once / write-once pass per tensor -- densify.hip's shape, with more roles per source row.
//
// A grown row shares scaling, opacity and _split_scale with its source, so every decision of either branch is a decision
// about the P source rows.  Each source row i yields up to four output roles, all subject to the final prune:
//
//   orig   : row i itself                 kept unless it is split or pruned
//   extra  : its clone / its grown copy   exists when sel & !big, kept unless pruned
//   child  : the split children of row i (and, in the grow branch, of its grown copy), when sel & big and not pruned
//
//   out = [ orig | extra | children #1 of orig | (grow) #1 of grown | children #2 of orig | (grow) #2 of grown ]
//
// which is the reference's order: clone + split gives [kept | clones | first | second]; grow gives A = [P | G grown],
// then B = [A without split rows | first children in A order | second children in A order], then the prune.
//
//   plan      : g = accum / denom (NaN -> 0); sel = g >= thr; big = max(exp(scaling)) > pd*extent; the prune test of
//               the children reads exp(log(exp(scaling) / (2k))) with the row's own k (0.8, or 0.6 sigmoid(split_scale)
//               + 0.5 with learn_split_scale)
//   positions : exclusive scans of the five classes {orig, extra, child, split-selected, selected}; sel_src lists the
//               selected rows in row order
//   gather    : dst row <- src row with a per-role value policy (copy, a constant, or left to the computed-row pass);
//               16-byte accesses for rows of 4k floats (_dirs_prob is 512 B per row at 128 directions)
//   rows      : the computed rows of the selected Gaussians -- grown xyz, children xyz and scaling, the normalised
//               conti_dirs re-init -- one wave per row when the direction needs the argmax over _dirs_prob
//
// The per-Gaussian arithmetic keeps the reference's float32 operation order (built with -ffp-contract=off).
#include "gsr_common.h"
#include "gsr_entry.h"
#include "gsr_launch.h"
#include "grow_common.h"
#include "row_plan.h"

namespace gsr {

constexpr int DF_BLOCK = PRE_BLOCK;
constexpr int DF_NC = 5;
enum : uint8_t { DF_ORIG = 1, DF_EXTRA = 2, DF_CHILD = 4, DF_SPLIT_SEL = 8, DF_SEL = 16 };

// 2 (0.6 sigmoid(_split_scale) + 0.5) or 0.8 * 2 (:560-563 / :714-718): `splitscale * N` in float32
__device__ inline float fork_split_div(const float* __restrict__ split_scale, int i) {
  return split_scale ? (0.6f * sigmoidf_(split_scale[i]) + 0.5f) * 2.0f : 1.6f;
}

__global__ __launch_bounds__(DF_BLOCK) void densify_fork_plan_kernel(int P, const float* __restrict__ accum,
                                                                      const float* __restrict__ denom,
                                                                      const float* __restrict__ scaling,
                                                                      const float* __restrict__ opacity,
                                                                      const float* __restrict__ split_scale, float thr,
                                                                      float pde, float min_opacity, float ws_limit,
                                                                      int use_ws, uint8_t* __restrict__ flags,
                                                                      uint32_t* __restrict__ block_counts, int stride) {
  const int i = blockIdx.x * DF_BLOCK + threadIdx.x;
  uint8_t f = 0;
  if (i < P) {
    float g = accum[i] / denom[i];
    if (g != g) g = 0.0f;
    const float s0 = expf(scaling[3 * i]), s1 = expf(scaling[3 * i + 1]), s2 = expf(scaling[3 * i + 2]);
    const float mx = fmaxf(fmaxf(s0, s1), s2);
    const bool sel = g >= thr, big = mx > pde;
    const float op = 1.0f / (1.0f + expf(-opacity[i]));
    const bool low = op < min_opacity;
    const bool prune_o = low || (use_ws && mx > ws_limit);
    const float k = fork_split_div(split_scale, i);
    const float c0 = expf(logf(s0 / k)), c1 = expf(logf(s1 / k)), c2 = expf(logf(s2 / k));
    const bool prune_c = low || (use_ws && fmaxf(fmaxf(c0, c1), c2) > ws_limit);
    if (!(sel && big) && !prune_o) f |= DF_ORIG;
    if (sel && !big && !prune_o) f |= DF_EXTRA;
    if (sel && big && !prune_c) f |= DF_CHILD;
    if (sel && big) f |= DF_SPLIT_SEL;
    if (sel) f |= DF_SEL;
    flags[i] = f;
  }
  block_count_classes<DF_NC>(f, block_counts, stride);
}

// pos[c * P + i] = rank of row i in class c, or -1; sel_src[rank among the selected] = i
__global__ __launch_bounds__(DF_BLOCK) void densify_fork_positions_kernel(int P, const uint8_t* __restrict__ flags,
                                                                           const uint32_t* __restrict__ block_offs,
                                                                           int stride, int32_t* __restrict__ pos,
                                                                           int32_t* __restrict__ sel_src) {
  const int i = blockIdx.x * DF_BLOCK + threadIdx.x;
  int32_t rank[DF_NC];
  block_rank_classes<DF_NC>(i < P ? flags[i] : 0, block_offs, stride, rank);
  if (i >= P) return;
#pragma unroll
  for (int b = 0; b < DF_NC; ++b) pos[(size_t)b * P + i] = rank[b];
  if (rank[DF_NC - 1] >= 0) sel_src[rank[DF_NC - 1]] = i;      // rank < #selected <= P
}

__device__ inline float splat_const(float, float c) { return c; }
__device__ inline float4 splat_const(float4, float c) { return make_float4(c, c, c, c); }

// One chunk (a float or a float4) of one source row per thread; every output role of the row gets its policy's value.
// Non-selected originals always copy: the flag byte's DF_SEL bit is read only when pol_orig is not a copy, so a plan
// whose flags have no such bit (densify.hip's) is served with pol_orig = GSR_ROW_COPY.  ncopies: children per split row
// (2 clone + split, 4 grow).
template <typename V>
__global__ __launch_bounds__(256) void densify_fork_gather_kernel(size_t total, int wv, int P,
                                                                   const V* __restrict__ src,
                                                                   const uint8_t* __restrict__ flags,
                                                                   const int32_t* __restrict__ pos, uint32_t n_orig,
                                                                   uint32_t n_extra, uint32_t n_child, int ncopies,
                                                                   int pol_orig, int pol_extra, int pol_child,
                                                                   float value, V* __restrict__ dst) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const uint32_t i = (uint32_t)(e / (size_t)wv), c = (uint32_t)(e - (size_t)i * wv);
  const int32_t po = pos[i], pe = pos[(size_t)P + i], pc = pos[2 * (size_t)P + i];
  const int o_pol = (pol_orig != GSR_ROW_COPY && (flags[i] & DF_SEL)) ? pol_orig : GSR_ROW_COPY;
  const bool w_o = po >= 0 && o_pol != GSR_ROW_SKIP, w_e = pe >= 0 && pol_extra != GSR_ROW_SKIP,
             w_c = pc >= 0 && pol_child != GSR_ROW_SKIP;
  if (!w_o && !w_e && !w_c) return;
  const bool need = (w_o && o_pol == GSR_ROW_COPY) || (w_e && pol_extra == GSR_ROW_COPY) ||
                    (w_c && pol_child == GSR_ROW_COPY);
  const V k = splat_const(V{}, value);
  const V v = need ? src[e] : k;
  if (w_o) dst[(size_t)po * wv + c] = o_pol == GSR_ROW_COPY ? v : k;
  if (w_e) dst[((size_t)n_orig + pe) * wv + c] = pol_extra == GSR_ROW_COPY ? v : k;
  if (w_c) {
    const V vc = pol_child == GSR_ROW_COPY ? v : k;
    for (int j = 0; j < ncopies; ++j) dst[((size_t)n_orig + n_extra + (size_t)j * n_child + pc) * wv + c] = vc;
  }
}

struct ForkRowsArgs {
  GsrDensifyFork f;
  const int32_t* pos;
  const int32_t* sel_src;
  uint32_t n_orig, n_extra, n_child, n_split, n_sel;
  float* xyz_out;
  float* scaling_out;
  float* conti_out;
};

// The computed rows of selected row i; dir: the grow direction (grow branch only).
__device__ inline void fork_rows(const ForkRowsArgs& a, int i, const float* dir) {
  const GsrDensifyFork& f = a.f;
  const size_t P = (size_t)f.P;
  const int32_t po = a.pos[i], pe = a.pos[P + i], pc = a.pos[2 * P + i];
  const bool grow = (f.mode & GSR_DENSIFY_GROW) != 0;
  const int ncopies = grow ? 4 : 2;
  const size_t child0 = (size_t)a.n_orig + a.n_extra;
  float stds[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) stds[c] = expf(f.scaling[3 * i + c]);
  const float* p = f.xyz + 3 * (size_t)i;
  float gx[3] = {p[0], p[1], p[2]};
  if (grow) {       // :632-635, read before the re-init of :645-655
    const float s = fmaxf(fmaxf(stds[0], stds[1]), stds[2]);
    const float d = (f.mode & GSR_GROW_DISTANCE) ? 2.0f * sigmoidf_(f.grow_dist[i]) : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gx[c] = p[c] + (dir[c] * s) * d;
    if (pe >= 0)
      for (int c = 0; c < 3; ++c) a.xyz_out[3 * ((size_t)a.n_orig + pe) + c] = gx[c];
  }
  if (a.conti_out) {  // :650-651: every row that comes from row i carries normalize(randn)
    const float* z = f.dir_noise + 3 * (size_t)a.pos[4 * P + i];
    const float n = fmaxf(sqrtf(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]), 1e-12f);
    const float u[3] = {z[0] / n, z[1] / n, z[2] / n};
    for (int c = 0; c < 3; ++c) {
      if (po >= 0) a.conti_out[3 * (size_t)po + c] = u[c];
      if (pe >= 0) a.conti_out[3 * ((size_t)a.n_orig + pe) + c] = u[c];
      if (pc >= 0)
        for (int j = 0; j < ncopies; ++j) a.conti_out[3 * (child0 + (size_t)j * a.n_child + pc) + c] = u[c];
    }
  }
  if (pc < 0) return;
  // children (:523-548 / :694-718): samples, rotation, scaling
  Rot r;
  build_rotation(f.rotation + 4 * (size_t)i, r);
  const float k = fork_split_div(f.split_scale, i);
  float ls[3], sd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ls[c] = logf(stds[c] / k);
    sd[c] = (f.mode & GSR_SPLIT_DISTANCE) ? stds[c] * (2.2f * sigmoidf_(f.split_distance[3 * i + c])) : 0.0f;
  }
  // the split rows of A (the reference's order of samples): originals, then (grow) grown copies
  const uint32_t r_split = (uint32_t)a.pos[3 * P + i], nA = grow ? 2 * a.n_split : a.n_split;
  const int nsrc = grow ? 2 : 1;
  for (int h = 0; h < 2; ++h) {             // first / second child
    for (int q = 0; q < nsrc; ++q) {        // of the original / of the grown copy
      const uint32_t ra = (uint32_t)q * a.n_split + r_split;      // row of A among its split rows
      float s[3];
      if (f.mode & GSR_SPLIT_DISTANCE) {
        for (int c = 0; c < 3; ++c) s[c] = h ? -sd[c] : sd[c];
      } else if (f.mode & GSR_DENSIFY_SYMMETRIC) {
        const float* z = f.noise + 3 * (size_t)ra;
        for (int c = 0; c < 3; ++c) { const float v = 0.0f + stds[c] * z[c]; s[c] = h ? -v : v; }
      } else {
        const float* z = f.noise + 3 * ((size_t)h * nA + ra);
        for (int c = 0; c < 3; ++c) s[c] = 0.0f + stds[c] * z[c];
      }
      const float* ctr = q ? gx : p;
      const size_t o = 3 * (child0 + (size_t)(h * nsrc + q) * a.n_child + pc);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* R = r.R + 3 * c;
        a.xyz_out[o + c] = ((R[0] * s[0] + R[1] * s[1]) + R[2] * s[2]) + ctr[c];
        a.scaling_out[o + c] = ls[c];
      }
    }
  }
}

// one thread per selected row (no argmax needed)
__global__ __launch_bounds__(256) void densify_fork_rows_kernel(ForkRowsArgs a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n_sel) return;
  const int i = a.sel_src[j];
  float dir[3] = {0.f, 0.f, 0.f};
  if ((a.f.mode & GSR_DENSIFY_GROW) && (a.f.mode & GSR_GROW_CONTINUOUS)) {
    const float* v = a.f.conti_dirs + 3 * (size_t)i;
    const float n = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-12f);   // F.normalize (:623)
    dir[0] = v[0] / n; dir[1] = v[1] / n; dir[2] = v[2] / n;
  }
  fork_rows(a, i, dir);
}

// one wave per selected row: the straight-through one-hot of softmax(_dirs_prob) times dirs (:617-621, :360-366)
__global__ __launch_bounds__(256) void densify_fork_rows_dir_kernel(ForkRowsArgs a) {
  const uint32_t j = blockIdx.x * (256 / WAVE) + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (j >= a.n_sel) return;
  const int i = a.sel_src[j];
  const int nd = a.f.num_dirs;
  const float* __restrict__ row = a.f.dirs_prob + (size_t)i * nd;
  float best;
  int bi;
  wave_argmax(row, nd, lane, best, bi);
  float sum = 0.0f;
  for (int n = lane; n < nd; n += WAVE) sum += expf(row[n] - best);
  sum = wave_reduce_add_f32(sum);
  if (lane != 0) return;
  const float y = 1.0f / sum;           // softmax at the argmax
  const float h = (1.0f - y) + y;       // y_hard - y_soft.detach() + y_soft
  const float dir[3] = {h * a.f.dirs[3 * bi], h * a.f.dirs[3 * bi + 1], h * a.f.dirs[3 * bi + 2]};
  fork_rows(a, i, dir);
}

// ---- host side ------------------------------------------------------------------------------------------------
// counts = {kept originals, kept clones / grown, kept children per copy, split-selected, selected}; behind the plan's
// head, pos[5][P] and sel_src[P]
struct DensifyForkLayout : RowPlanLayout {
  size_t pos, sel_src;
  explicit DensifyForkLayout(int P) : RowPlanLayout(P, DF_NC) {
    pos = bytes;
    sel_src = align_up(pos + 4 * DF_NC * rows, 256);
    bytes = align_up(sel_src + 4 * rows, 256);
  }
  int32_t* pos_of(const void* ws) const { return at<int32_t>(ws, pos); }
  int32_t* sel_src_of(const void* ws) const { return at<int32_t>(ws, sel_src); }
};

static void launch_densify_fork_plan(int P, const float* accum, const float* denom, const float* scaling,
                                     const float* opacity, const float* split_scale, float thr, float pde,
                                     float min_opacity, float ws_limit, int use_ws, void* ws, hipStream_t s) {
  const DensifyForkLayout L(P);
  hipLaunchKernelGGL(densify_fork_plan_kernel, dim3(L.nblocks), dim3(DF_BLOCK), 0, s, P, accum, denom, scaling, opacity,
                     split_scale, thr, pde, min_opacity, ws_limit, use_ws, L.flags_of(ws), L.block_counts_of(ws),
                     L.stride);
  launch_class_scans(L, ws, s);
  hipLaunchKernelGGL(densify_fork_positions_kernel, dim3(L.nblocks), dim3(DF_BLOCK), 0, s, P, L.flags_of(ws),
                     L.block_offs_of(ws), L.stride, L.pos_of(ws), L.sel_src_of(ws));
}

// gsr_launch.h: the gather of this file's plan and of densify.hip's (whose pos holds the same first three classes)
void launch_gather_rows(int P, int w, const float* src, const uint8_t* flags, const int32_t* pos,
                        const uint32_t counts[3], int ncopies, int po, int pe, int pc, float value, float* dst,
                        hipStream_t s) {
  const bool vec = (w & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0;
  const int wv = vec ? w / 4 : w;
  const size_t total = (size_t)P * wv;
  if (total == 0) return;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (vec)
    hipLaunchKernelGGL(densify_fork_gather_kernel<float4>, grid, dim3(256), 0, s, total, wv, P,
                       reinterpret_cast<const float4*>(src), flags, pos, counts[0], counts[1], counts[2], ncopies, po,
                       pe, pc, value, reinterpret_cast<float4*>(dst));
  else
    hipLaunchKernelGGL(densify_fork_gather_kernel<float>, grid, dim3(256), 0, s, total, wv, P, src, flags, pos,
                       counts[0], counts[1], counts[2], ncopies, po, pe, pc, value, dst);
}

static void launch_densify_fork_rows(const GsrDensifyFork& f, const void* ws, const uint32_t counts[5], float* xyz_out,
                                     float* scaling_out, float* conti_out, hipStream_t s) {
  const DensifyForkLayout L(f.P);
  ForkRowsArgs a;
  a.f = f;
  a.pos = L.pos_of(ws);
  a.sel_src = L.sel_src_of(ws);
  a.n_orig = counts[0]; a.n_extra = counts[1]; a.n_child = counts[2]; a.n_split = counts[3]; a.n_sel = counts[4];
  a.xyz_out = xyz_out; a.scaling_out = scaling_out; a.conti_out = conti_out;
  if (a.n_sel == 0) return;
  if ((f.mode & GSR_DENSIFY_GROW) && (f.mode & GSR_GROW_DIR))
    hipLaunchKernelGGL(densify_fork_rows_dir_kernel, dim3((a.n_sel + 3) / 4), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(densify_fork_rows_kernel, dim3((a.n_sel + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_densify_fork_workspace_bytes(int32_t P) { return P < 0 ? 0 : DensifyForkLayout(P).bytes; }
int gsr_densify_fork_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                          const float* opacity_raw, const float* split_scale_raw, float grad_threshold,
                          float percent_dense_extent, float min_opacity, float max_world_scale, void* workspace,
                          size_t workspace_bytes, uint32_t counts_host[5], void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (!counts_host) return fail(GSR_E_BADARG, "NULL counts_host");
  for (int k = 0; k < 5; ++k) counts_host[k] = 0;
  if (P == 0) return 0;
  if (!xyz_gradient_accum || !denom || !scaling_raw || !opacity_raw || !workspace) return fail(GSR_E_BADARG, "NULL input");
  if (!aligned({workspace}, 255u)) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  const DensifyForkLayout L(P);
  if (workspace_bytes < L.bytes) return fail(GSR_E_CAPACITY, "densify_fork workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_fork_plan(P, xyz_gradient_accum, denom, scaling_raw, opacity_raw, split_scale_raw, grad_threshold,
                           percent_dense_extent, min_opacity, max_world_scale, max_world_scale >= 0.0f ? 1 : 0,
                           workspace, s);
  if (int rc = check(false, s, "densify_fork_plan")) return rc;
  return read_class_totals(L, workspace, counts_host, s);
}
int gsr_densify_fork_gather_rows(int32_t P, int32_t row_floats, const float* src, const void* workspace,
                                 const uint32_t counts[5], int32_t grow_branch, int32_t policy, float value, float* dst,
                                 void* stream) {
  if (P < 0 || row_floats <= 0) return fail(GSR_E_BADARG, "bad P / row_floats");
  if (policy < 0 || policy >= 64 || (policy & 3) == 3 || ((policy >> 2) & 3) == 3 || ((policy >> 4) & 3) == 3)
    return fail(GSR_E_BADARG, "bad row policy");
  if (P == 0) return 0;
  if (!src || !workspace || !counts) return fail(GSR_E_BADARG, "NULL argument");
  if (!dst && counts[0] + counts[1] + counts[2] > 0) return fail(GSR_E_BADARG, "NULL dst");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const DensifyForkLayout L(P);
  launch_gather_rows(P, row_floats, src, L.flags_of(workspace), L.pos_of(workspace), counts, grow_branch ? 4 : 2,
                     policy & 3, (policy >> 2) & 3, (policy >> 4) & 3, value, dst, s);
  return check(false, s, "densify_fork_gather_rows");
}
int gsr_densify_fork_rows(const GsrDensifyFork* f, const void* workspace, const uint32_t counts[5], float* xyz_out,
                          float* scaling_out, float* conti_dirs_out, void* stream) {
  if (!f || !counts) return fail(GSR_E_BADARG, "NULL argument");
  if (f->P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (f->P == 0 || counts[4] == 0 || counts[0] + counts[1] + counts[2] == 0) return 0;     // nothing to write
  if (counts[4] > (uint32_t)f->P || counts[3] > counts[4] || counts[2] > counts[3])
    return fail(GSR_E_BADARG, "counts do not come from gsr_densify_fork_plan of this P");
  GsrDensifyFork g = *f;
  const int grow = (g.mode & GSR_DENSIFY_GROW) != 0;
  if (grow && ((g.mode & GSR_GROW_DIR) != 0) == ((g.mode & GSR_GROW_CONTINUOUS) != 0))
    return fail(GSR_E_BADARG, "the grow branch needs exactly one of GSR_GROW_DIR and GSR_GROW_CONTINUOUS");
  if (!g.xyz || !g.scaling || !g.rotation || !workspace || !xyz_out || !scaling_out)
    return fail(GSR_E_BADARG, "NULL model tensor or output");
  if (grow && (g.mode & GSR_GROW_DIR) && (!g.dirs_prob || !g.dirs || g.num_dirs <= 0))
    return fail(GSR_E_BADARG, "GSR_GROW_DIR needs dirs_prob, dirs and num_dirs > 0");
  if (grow && (g.mode & GSR_GROW_CONTINUOUS) && !g.conti_dirs) return fail(GSR_E_BADARG, "NULL conti_dirs");
  if (grow && (g.mode & GSR_GROW_DISTANCE) && !g.grow_dist) return fail(GSR_E_BADARG, "NULL grow_dist");
  if ((g.mode & GSR_SPLIT_DISTANCE) && !g.split_distance) return fail(GSR_E_BADARG, "NULL split_distance");
  if ((g.mode & GSR_SPLIT_SCALE) && !g.split_scale) return fail(GSR_E_BADARG, "NULL split_scale");
  if (!(g.mode & GSR_SPLIT_DISTANCE) && counts[3] > 0 && !g.noise) return fail(GSR_E_BADARG, "NULL noise");
  if (conti_dirs_out && (!grow || !(g.mode & GSR_GROW_CONTINUOUS) || !g.dir_noise))
    return fail(GSR_E_BADARG, "conti_dirs_out needs the continuous grow branch and dir_noise");
  if (!(g.mode & GSR_SPLIT_SCALE)) g.split_scale = nullptr;     // the kernels read k = 1.6 from a NULL split_scale
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_fork_rows(g, workspace, counts, xyz_out, scaling_out, conti_dirs_out, s);
  return check(false, s, "densify_fork_rows");
}

}  // extern "C"
