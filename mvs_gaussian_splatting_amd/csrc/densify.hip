// Densification bookkeeping: scene/gaussian_model.py:750-772 densify_and_prune with its clone
// (:580-610), split (:506-578), postfix (:466-504) and prune (:401-449) steps as one plan + row-gather passes.
//
// The reference builds the new model through ~60 boolean-mask indexing / cat / repeat launches (each mask index is a
// nonzero + gather with a host sync) and touches every parameter and Adam moment three times.  Here one kernel
// classifies every Gaussian, four block scans place the survivors, and each tensor is read once and written once:
//
//   out = [ kept originals | kept clones | kept first children | kept second children ]      (the reference's order)
//
//   plan      : per Gaussian  grad = accum / denom (NaN -> 0);  sel = grad >= thr;  big = max(exp(scaling)) > pd*extent
//               clone = sel & !big; split = sel & big;  prune = sigmoid(opacity) < min_opacity | max scale > 0.1*extent
//               with the absolute-gradient accumulator of AbsGS / PGSR (gsr_densify_plan_abs): split = (sel | sel_abs) & big,
//               sel_abs = accum_abs / denom (NaN -> 0) >= abs_thr; clone and prune as without it
//               (the screen-size test of :762 always reads the zeros that densification_postfix has just stored, :503)
//   positions : exclusive scans (block totals -> block offsets -> in-block) of the four flag classes
//   gather    : dst row <- src row for kept / clone / child rows (moments: zeros for the new rows, :458-459), by
//               densify_fork.hip's gather kernel (launch_gather_rows)
//   children  : xyz = R(rotation) (exp(scaling) * noise) + xyz ;  scaling = log(exp(scaling) / (0.8 * 2))
#include "gsr_common.h"
#include "gsr_entry.h"
#include "gsr_launch.h"
#include "row_plan.h"

namespace gsr {

constexpr int DN_BLOCK = PRE_BLOCK;
enum : uint8_t { DN_KEEP = 1, DN_CLONE = 2, DN_CHILD = 4, DN_SPLIT_SEL = 8 };

__global__ __launch_bounds__(DN_BLOCK) void densify_plan_kernel(int P, const float* __restrict__ accum,
                                                                 const float* __restrict__ accum_abs, float abs_thr,
                                                                 const float* __restrict__ denom,
                                                                 const float* __restrict__ scaling,
                                                                 const float* __restrict__ opacity, float thr, float pde,
                                                                 float min_opacity, float ws_limit, int use_ws,
                                                                 uint8_t* __restrict__ flags,
                                                                 uint32_t* __restrict__ block_counts, int stride) {
  const int i = blockIdx.x * DN_BLOCK + threadIdx.x;
  uint8_t f = 0;
  if (i < P) {
    float g = accum[i] / denom[i];
    if (g != g) g = 0.0f;
    const float s0 = expf(scaling[3 * i]), s1 = expf(scaling[3 * i + 1]), s2 = expf(scaling[3 * i + 2]);
    const float mx = fmaxf(fmaxf(s0, s1), s2);
    const bool sel = g >= thr;
    bool sel_split = sel;
    if (accum_abs) {      // uniform over the grid
      float ga = accum_abs[i] / denom[i];
      if (ga != ga) ga = 0.0f;
      sel_split = sel || ga >= abs_thr;
    }
    const bool clone = sel && mx <= pde, split = sel_split && mx > pde;
    const float op = 1.0f / (1.0f + expf(-opacity[i]));
    const bool low = op < min_opacity;
    const bool prune_o = low || (use_ws && mx > ws_limit);
    // the children carry log(scale / 1.6); the prune test sees exp() of that (:548, :760-763)
    const float c0 = expf(logf(s0 / 1.6f)), c1 = expf(logf(s1 / 1.6f)), c2 = expf(logf(s2 / 1.6f));
    const bool prune_c = low || (use_ws && fmaxf(fmaxf(c0, c1), c2) > ws_limit);
    if (!split && !prune_o) f |= DN_KEEP;
    if (clone && !prune_o) f |= DN_CLONE;
    if (split && !prune_c) f |= DN_CHILD;
    if (split) f |= DN_SPLIT_SEL;
    flags[i] = f;
  }
  block_count_classes<4>(f, block_counts, stride);
}

// pos[c][i] = output row of Gaussian i in class c (keep / clone / child), or -1; sel_rank[i] = rank among the
// split-selected (the row of its first noise sample), or -1.
__global__ __launch_bounds__(DN_BLOCK) void densify_positions_kernel(int P, const uint8_t* __restrict__ flags,
                                                                      const uint32_t* __restrict__ block_offs, int stride,
                                                                      int32_t* __restrict__ pos) {
  const int i = blockIdx.x * DN_BLOCK + threadIdx.x;
  int32_t rank[4];
  block_rank_classes<4>(i < P ? flags[i] : 0, block_offs, stride, rank);
  if (i >= P) return;
#pragma unroll
  for (int b = 0; b < 4; ++b) pos[(size_t)b * P + i] = rank[b];
}

__global__ void densify_split_children_kernel(int P, const float* __restrict__ xyz, const float* __restrict__ scaling,
                                              const float* __restrict__ rotation, const float* __restrict__ noise,
                                              const int32_t* __restrict__ pos, uint32_t n_keep, uint32_t n_clone,
                                              uint32_t n_child, uint32_t n_sel, float* __restrict__ dst_xyz,
                                              float* __restrict__ dst_scaling) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  const int32_t ph = pos[2 * (size_t)P + i];
  if (ph < 0) return;
  const uint32_t r = (uint32_t)pos[3 * (size_t)P + i];
  const float qr = rotation[4 * i], qx = rotation[4 * i + 1], qy = rotation[4 * i + 2], qz = rotation[4 * i + 3];
  const float norm = sqrtf(qr * qr + qx * qx + qy * qy + qz * qz);          // utils/general_utils.py:78-99
  const float w = qr / norm, x = qx / norm, y = qy / norm, z = qz / norm;
  const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - w * z), R02 = 2.f * (x * z + w * y);
  const float R10 = 2.f * (x * y + w * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - w * x);
  const float R20 = 2.f * (x * z - w * y), R21 = 2.f * (y * z + w * x), R22 = 1.f - 2.f * (x * x + y * y);
  const float s0 = expf(scaling[3 * i]), s1 = expf(scaling[3 * i + 1]), s2 = expf(scaling[3 * i + 2]);
  const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
  const float l0 = logf(s0 / 1.6f), l1 = logf(s1 / 1.6f), l2 = logf(s2 / 1.6f);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float* z3 = noise + 3 * ((size_t)k * n_sel + r);
    const float a = s0 * z3[0], b = s1 * z3[1], c = s2 * z3[2];
    const size_t o = (size_t)n_keep + n_clone + (size_t)k * n_child + ph;
    dst_xyz[3 * o] = (R00 * a + R01 * b + R02 * c) + px;
    dst_xyz[3 * o + 1] = (R10 * a + R11 * b + R12 * c) + py;
    dst_xyz[3 * o + 2] = (R20 * a + R21 * b + R22 * c) + pz;
    dst_scaling[3 * o] = l0; dst_scaling[3 * o + 1] = l1; dst_scaling[3 * o + 2] = l2;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
// counts = {kept originals, kept clones, kept children per copy, split-selected}; behind the plan's head, pos[4][P]
struct DensifyLayout : RowPlanLayout {
  size_t pos;
  explicit DensifyLayout(int P) : RowPlanLayout(P, 4) { pos = bytes; bytes = align_up(pos + 4 * 4 * rows, 256); }
  int32_t* pos_of(const void* ws) const { return at<int32_t>(ws, pos); }
};

static void launch_densify_plan(int P, const float* accum, const float* accum_abs, float abs_thr, const float* denom,
                                const float* scaling, const float* opacity, float thr, float pde, float min_opacity, float ws_limit, int use_ws, void* ws,
                                hipStream_t s) {
  const DensifyLayout L(P);
  hipLaunchKernelGGL(densify_plan_kernel, dim3(L.nblocks), dim3(DN_BLOCK), 0, s, P, accum, accum_abs, abs_thr, denom,
                     scaling, opacity, thr, pde, min_opacity, ws_limit, use_ws, L.flags_of(ws), L.block_counts_of(ws),
                     L.stride);
  launch_class_scans(L, ws, s);
  hipLaunchKernelGGL(densify_positions_kernel, dim3(L.nblocks), dim3(DN_BLOCK), 0, s, P, L.flags_of(ws),
                     L.block_offs_of(ws), L.stride, L.pos_of(ws));
}

static void launch_densify_split_children(int P, const float* xyz, const float* scaling, const float* rotation,
                                          const float* noise, const void* ws, const uint32_t counts[4], float* dst_xyz,
                                          float* dst_scaling, hipStream_t s) {
  const int32_t* pos = DensifyLayout(P).pos_of(ws);
  if (P == 0 || counts[2] == 0) return;
  hipLaunchKernelGGL(densify_split_children_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, xyz, scaling, rotation,
                     noise, pos, counts[0], counts[1], counts[2], counts[3], dst_xyz, dst_scaling);
}

}  // namespace gsr

// ---- entry points (include/gsr.h) -----------------------------------------------------------------------------------
using namespace gsr;

extern "C" {

size_t gsr_densify_workspace_bytes(int32_t P) { return P < 0 ? 0 : DensifyLayout(P).bytes; }
int gsr_densify_plan_abs(int32_t P, const float* xyz_gradient_accum, const float* xyz_gradient_accum_abs,
                         const float* denom, const float* scaling_raw, const float* opacity_raw, float grad_threshold,
                         float abs_grad_threshold, float percent_dense_extent, float min_opacity, float max_world_scale,
                         void* workspace, size_t workspace_bytes, uint32_t counts_host[4], void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (!counts_host) return fail(GSR_E_BADARG, "NULL counts_host");
  counts_host[0] = counts_host[1] = counts_host[2] = counts_host[3] = 0;
  if (P == 0) return 0;
  if (!xyz_gradient_accum || !denom || !scaling_raw || !opacity_raw || !workspace) return fail(GSR_E_BADARG, "NULL input");
  if (!aligned({workspace}, 255u)) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  const DensifyLayout L(P);
  if (workspace_bytes < L.bytes) return fail(GSR_E_CAPACITY, "densify workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_plan(P, xyz_gradient_accum, xyz_gradient_accum_abs, abs_grad_threshold, denom, scaling_raw, opacity_raw,
                      grad_threshold, percent_dense_extent, min_opacity, max_world_scale, max_world_scale >= 0.0f ? 1 : 0, workspace, s);
  if (int rc = check(false, s, "densify_plan")) return rc;
  return read_class_totals(L, workspace, counts_host, s);
}
int gsr_densify_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                     const float* opacity_raw, float grad_threshold, float percent_dense_extent, float min_opacity,
                     float max_world_scale, void* workspace, size_t workspace_bytes, uint32_t counts_host[4],
                     void* stream) {
  return gsr_densify_plan_abs(P, xyz_gradient_accum, nullptr, denom, scaling_raw, opacity_raw, grad_threshold, 0.0f,
                              percent_dense_extent, min_opacity, max_world_scale, workspace, workspace_bytes, counts_host,
                              stream);
}
int gsr_densify_gather_rows(int32_t P, int32_t row_floats, const float* src, const void* workspace,
                            const uint32_t counts[4], int32_t zero_new, float* dst, void* stream) {
  if (P < 0 || row_floats <= 0) return fail(GSR_E_BADARG, "bad P / row_floats");
  if (P == 0) return 0;
  if (!src || !workspace || !counts) return fail(GSR_E_BADARG, "NULL argument");
  if (!dst && counts[0] + counts[1] + counts[2] > 0) return fail(GSR_E_BADARG, "NULL dst");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the fork's gather with two child copies: originals copy, clones and children copy or (zero_new: the Adam moments of
  // new points, :458-459) receive zeros; no policy looks at a selected bit, so the flag bytes are not read
  const DensifyLayout L(P);
  const int pol_new = zero_new ? GSR_ROW_CONST : GSR_ROW_COPY;
  launch_gather_rows(P, row_floats, src, L.flags_of(workspace), L.pos_of(workspace), counts, 2, GSR_ROW_COPY, pol_new,
                     pol_new, 0.0f, dst, s);
  return check(false, s, "densify_gather_rows");
}
int gsr_densify_split_children(int32_t P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                               const float* noise, const void* workspace, const uint32_t counts[4], float* dst_xyz,
                               float* dst_scaling, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (!counts) return fail(GSR_E_BADARG, "NULL counts");
  if (P == 0 || counts[2] == 0) return 0;
  if (!xyz || !scaling_raw || !rotation_raw || !noise || !workspace || !dst_xyz || !dst_scaling)
    return fail(GSR_E_BADARG, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_split_children(P, xyz, scaling_raw, rotation_raw, noise, workspace, counts, dst_xyz, dst_scaling, s);
  return check(false, s, "densify_split_children");
}

}  // extern "C"
