/*
 * gsr.h — C ABI of the MI355X-native differentiable Gaussian rasterizer (libgsr_hip.so).
 *
 * This is the drop-in boundary for the reference's `diff_gaussian_rasterization._C` pybind
 * module (absent from /root/reference: un-vendored submodule, .gitmodules:4-6).  The
 * reference binds it at
 *     gaussian_renderer/__init__.py:15      (import of GaussianRasterizationSettings/GaussianRasterizer)
 *     gaussian_renderer/__init__.py:42-57   (settings tuple + module construction, every frame)
 *     gaussian_renderer/__init__.py:257-265 (the call)
 * and reaches the backward through loss.backward() at train.py:107.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer marked "device" is HIP device memory owned
 *     by the caller (PyTorch on the Python side); the library never allocates or frees device
 *     memory and keeps no global mutable state (forward and backward arrive on different OS
 *     threads: train.py:107 runs backward on an autograd engine thread);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it; the only host
 *     synchronisation is the read-back of (num_rendered, num_visible) in gsr_forward_preprocess();
 *   - return value 0 = success, >0 = hipError_t, <0 = library error (GSR_E_*); the message is
 *     available per thread from gsr_last_error();
 *   - all float tensors are contiguous fp32; matrices are the row-vector-convention 4x4s the
 *     reference builds at scene/cameras.py:54-57 (p_view = [x,y,z,1] @ viewmatrix).
 */
#ifndef GSR_H_
#define GSR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_ABI_VERSION 47

enum {
  GSR_OK = 0,
  GSR_E_BADARG = -1,    /* null / inconsistent arguments (both-or-neither of shs/colors, scales+rotations/cov3D) */
  GSR_E_CAPACITY = -2,  /* binning workspace smaller than gsr_binning_bytes(num_rendered) */
  GSR_E_ALIGN = -3      /* a pointer violates the documented alignment */
};

/* One call's inputs.  Replaces the positional arguments of the reference-side
 * `_C.rasterize_gaussians(bg, means3D, colors, opacity, scales, rotations, scale_modifier,
 * cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh, degree, campos,
 * prefiltered, debug)` implied by gaussian_renderer/__init__.py:42-55,257-265. */
typedef struct GsrParams {
  int32_t P;              /* number of Gaussians */
  int32_t M;              /* SH coefficients stored per Gaussian in `shs` ((max_sh_degree+1)^2); 0 with colors_precomp */
  int32_t D;              /* active SH degree evaluated (0..3), settings.sh_degree */
  int32_t width, height;  /* settings.image_width / image_height */
  float tan_fovx, tan_fovy;
  float scale_modifier;
  int32_t prefiltered;    /* accepted and ignored: the reference always passes False (gaussian_renderer/__init__.py:53);
                             culled Gaussians are simply skipped whatever its value */
  int32_t debug;          /* 1: synchronise and check after every kernel */
  const float* means3D;        /* device [P,3] */
  const float* shs;            /* device [P,M,3] or NULL (16-byte aligned) */
  const float* colors_precomp; /* device [P,3] or NULL */
  const float* opacities;      /* device [P] (the reference passes [P,1]) */
  const float* scales;         /* device [P,3] or NULL */
  const float* rotations;      /* device [P,4] (w,x,y,z) or NULL (16-byte aligned) */
  const float* cov3D_precomp;  /* device [P,6] (xx,xy,xz,yy,yz,zz) or NULL */
  const float* viewmatrix;     /* device [16] */
  const float* projmatrix;     /* device [16] */
  const float* campos;         /* device [3] */
  const float* bg;             /* device [3] */
  void* profile;               /* NULL, or a handle from gsr_profile_create(): HIP-event stage timers */
  /* Fused-input extension (removes the caller's torch.cat / exp / normalize / sigmoid of
   * scene/gaussian_model.py:151-183 and their autograd): */
  const float* shs_rest;       /* NULL, or device [P,M-1,3] (16-byte aligned): then `shs` is [P,1,3] (f_dc) */
  int32_t act_flags;           /* GSR_ACT_*: inputs are RAW parameters, the activation (and its gradient) is applied here */
  int32_t binning_mode;        /* GSR_BINNING_*; same value in every call of a frame */
  uint32_t* counts_pinned;     /* NULL, or HOST-PINNED, device-accessible uint32[4] (hipHostMalloc / torch pin_memory):
                                  the scan kernel stores (num_rendered, num_visible, smallest and largest depth key) there and gsr_forward_preprocess
                                  waits on an event behind that kernel only, so the depth sort it has already
                                  enqueued keeps the GPU busy while the host sizes and launches stage 2 */
  int32_t forward_only;        /* 1: no gsr_backward will follow (inference): the compositing kernel does not track the
                                  last contributor and the per-pixel / per-Gaussian state the backward reads (final
                                  transmittance, contributor counts, gradient-row slots) is not written.  Same image. */
  int32_t debug_flags;         /* GSR_DEBUG_* bits: switches the tests use (never read from the environment) */
  uint8_t* visible_out;        /* NULL, or device [P] (ABI v12): the forward also stores radii[i] > 0 there -- the
                                  `visibility_filter = radii > 0` of the reference's render()
                                  (gaussian_renderer/__init__.py:311) without a pass of its own over the radii */
  int32_t depth_span_lt24;     /* gsr_forward only (ABI v13).  1: the caller expects the frame's depth keys (float32 bits of the
                                  view depths of the visible Gaussians) to span fewer than 2^24 steps -- counts_pinned[3] -
                                  counts_pinned[2] < 2^24, about two binades of depth -- and the depth sort's fourth pass (three
                                  launches that find nothing to do on such a frame) is NOT enqueued.  The caller must check
                                  the two words once the counts event has completed, exactly as it checks the capacity: a
                                  frame that spans more is sorted on its low 24 key bits only (no out-of-bounds access,
                                  but lists in the wrong depth order) and must be discarded / redone with 0.
                                  0: the pass is enqueued and decides on the device (any frame is right). */
} GsrParams;

enum {
  GSR_DEBUG_NO_MINIBLOCK_CULL = 1  /* forward compositing: every staged instance enters all 16 mini-block lists (the
                                      image must not change by a bit: tests/test_gpu_miniblock_cull.py) */
};

enum {
  GSR_BINNING_TWO_LEVEL = 0,   /* depth-sort the visible Gaussians (u32 keys), emit instances in depth order, stable
                                  partition by tile id (u32 keys): same lists as KEYS64 for ~2.5x less sort traffic */
  GSR_BINNING_KEYS64 = 1,      /* upstream layout: duplicateWithKeys + radix sort of u64 tile<<32|depth keys */
  GSR_BINNING_TWO_LEVEL_CULLED = 2 /* TWO_LEVEL minus the (Gaussian, tile) instances whose tile the alpha >= 1/255
                                  ellipse provably cannot reach (rects of > 32 tiles shrink to the ellipse's bounding box;
                                  rects of <= 32 tiles get an exact per-tile ellipse test with a safety margin): such
                                  instances are rejected pixel by pixel by the alpha test anyway,
                                  so colour, radii and every gradient are bit-identical to the other modes; only the
                                  internal lists (and n_contrib positions) are shorter */
};

enum {
  GSR_ACT_SCALE_EXP = 1,       /* scales    = exp(raw)              scene/gaussian_model.py:34,151-153 */
  GSR_ACT_ROT_NORMALIZE = 2,   /* rotations = raw / max(|raw|,1e-12) scene/gaussian_model.py:42,167-169 */
  GSR_ACT_OPACITY_SIGMOID = 4  /* opacity   = sigmoid(raw)          scene/gaussian_model.py:39,181-183 */
};

/* Gradient outputs of the backward.  Replaces the tuple returned by the reference-side
 * `_C.rasterize_gaussians_backward(...)`.  Every buffer is written in full by the call
 * (no caller zero-fill required); NULL is allowed for the members that do not apply
 * (dL_dshs without shs, dL_dcolors without colors_precomp, dL_dscales/dL_drotations with
 * cov3D_precomp, dL_dcov3D without it). */
typedef struct GsrGrads {
  float* dL_dmeans3D;   /* device [P,3] */
  float* dL_dmeans2D;   /* device [P,3] (x,y in NDC units scaled by 0.5*W / 0.5*H; z = 0) */
  float* dL_dshs;       /* device [P,M,3] */
  float* dL_dcolors;    /* device [P,3] */
  float* dL_dopacities; /* device [P] */
  float* dL_dscales;    /* device [P,3] */
  float* dL_drotations; /* device [P,4] */
  float* dL_dcov3D;     /* device [P,6] */
  float* dL_dshs_rest;  /* device [P,M-1,3]; required with shs_rest (dL_dshs is then [P,1,3]) */
  /* Fused densification statistics (scene/gaussian_model.py:775-777 + train.py:130): all three
   * NULL, or all three set -- then the per-Gaussian backward kernel, which holds dL_dmeans2D and the radius in
   * registers, also does  xyz_gradient_accum[i] += ||dL_dmeans2D[i].xy||, denom[i] += 1,
   * max_radii2D[i] = max(max_radii2D[i], radii[i])  for every Gaussian with radii[i] > 0 (same arithmetic as
   * gsr_densify_stats, which stays available as the stand-alone step). */
  float* stats_xyz_gradient_accum; /* device [P] (the reference keeps [P,1]) */
  float* stats_denom;              /* device [P] */
  float* stats_max_radii2D;        /* device [P] */
  /* Camera gradients (ABI v20): all three NULL, or all three set -- then camera_ws is required, the per-Gaussian
   * backward runs its camera instantiation and a one-block kernel behind it stores the three gradients (float32,
   * written in full, reproducible bit for bit: block partials in double, added in a fixed order, no atomics).
   * Layout as the inputs: m[4*row + col] of the row-vector-convention matrices.  dL_dviewmatrix column 3 and
   * dL_dprojmatrix column 2 are exact zeros (the rasterizer does not read those entries); dL_dcampos is exactly zero
   * with colors_precomp or at active SH degree 0.  Every other output is bit-identical with and without them. */
  float* dL_dviewmatrix;           /* device [16] */
  float* dL_dprojmatrix;           /* device [16] */
  float* dL_dcampos;               /* device [3] */
  void* camera_ws;                 /* device scratch of gsr_camera_grad_bytes(P) bytes, 256-byte aligned */
} GsrGrads;

/* ---- introspection ------------------------------------------------------------------ */
int gsr_abi_version(void);
const char* gsr_last_error(void);       /* thread-local, never NULL */
const char* gsr_build_info(void);       /* "gfx950 ..." */

/* ---- workspace sizing (bytes; all workspaces must be 256-byte aligned) ----------------- */
size_t gsr_geom_bytes(int32_t P);                        /* per-Gaussian state (upstream "geomBuffer") */
size_t gsr_image_bytes(int32_t width, int32_t height);   /* per-pixel + per-tile state ("imgBuffer") */
size_t gsr_binning_bytes(uint32_t num_rendered, uint32_t num_visible, int32_t width, int32_t height,
                         int32_t binning_mode);          /* keys/values/sort scratch ("binningBuffer") */
size_t gsr_backward_bytes(int32_t P, uint32_t num_rendered); /* per-instance gradient rows + flags */
size_t gsr_camera_grad_bytes(int32_t P);                 /* GsrGrads.camera_ws: 27 double sums per block of 256 Gaussians */

/* ---- forward -------------------------------------------------------------------------- */
/* Stage 1: preprocess (cull, project, cov3D->cov2D->conic, radius, tile rect, SH->RGB) and the
 * prefix sum of tiles_touched.  Writes radii[P] (int32), *num_rendered (instances) and *num_visible (host).
 * Blocks the calling thread until the two counts have been read back (the one sync of the forward). */
int gsr_forward_preprocess(const GsrParams* p, void* geom_ws, int32_t* radii, void* stream,
                           uint32_t* num_rendered, uint32_t* num_visible);

/* Stage 2: tile binning (see binning_mode), identifyTileRanges, per-tile compositing.
 * Writes out_color[3,H,W].  bin_ws must hold gsr_binning_bytes(num_rendered, num_visible, W, H, mode). */
int gsr_forward_render(const GsrParams* p, void* geom_ws, void* bin_ws, size_t bin_ws_bytes,
                       void* img_ws, uint32_t num_rendered, uint32_t num_visible, float* out_color, void* stream);

/* Both stages in one call with NO host synchronisation (SURVEY §7 "hard parts": caller-provided capacity + overflow
 * flag instead of upstream's per-forward num_rendered read-back, gaussian_renderer/__init__.py:257-265).
 *   capacity     : instances the binning workspace can hold; bin_ws must hold
 *                  gsr_binning_bytes(capacity, P, W, H, mode) bytes.  Every launch is sized for (capacity, P) and the
 *                  kernels take the real counts from device memory.
 *   p->counts_pinned (required): receives (num_rendered, num_visible, min depth key, max depth key) when the scan
 *                  kernel has run; `counts_event` (a handle from gsr_event_create, or NULL) is recorded right behind it.
 *   Overflow     : when num_rendered > capacity the instances past the capacity are dropped (no out-of-bounds
 *                  access, but the image and every gradient of the frame are INCOMPLETE): the caller must compare
 *                  counts_pinned[0] with its capacity once the event has completed and discard / redo the frame.
 *   Depth span   : with p->depth_span_lt24 = 1 the same check covers counts_pinned[3] - counts_pinned[2] < 2^24 (see the field).
 *   Backward     : call gsr_backward with num_rendered = capacity and num_visible = P (the values the workspaces
 *                  were laid out with); gsr_backward_bytes(P, capacity) sizes its workspace.
 * Only GSR_BINNING_TWO_LEVEL / _CULLED (the 64-bit key mode keeps the two-call path). */
int gsr_forward(const GsrParams* p, void* geom_ws, void* bin_ws, size_t bin_ws_bytes, uint32_t capacity, void* img_ws,
                int32_t* radii, float* out_color, void* counts_event, void* stream);
/* events for the deferred count check (plain HIP events without timing; usable from any thread) */
int gsr_event_create(void** event);
int gsr_event_destroy(void* event);
int gsr_event_wait(void* event);                 /* blocks the calling thread until the event has completed */
int gsr_event_query(void* event, int32_t* done); /* *done = 1 when completed; never blocks */

/* ---- backward -------------------------------------------------------------------------
 * geom_ws, bin_ws and img_ws as the forward of the SAME frame left them: besides the sorted point list, bin_ws holds the
 * 16-bit mini-block reach mask of every instance, which the forward's compositing stores in list order (in the tile
 * sort's spare payload buffer) when p->forward_only is 0 and the backward's compositing reads instead of re-deriving. */
int gsr_backward(const GsrParams* p, const int32_t* radii, const void* geom_ws, const void* bin_ws,
                 const void* img_ws, uint32_t num_rendered, uint32_t num_visible,
                 const float* dL_dout_color /* [3,H,W] */,
                 void* bwd_ws, size_t bwd_ws_bytes, const GsrGrads* grads, void* stream);

/* ---- depth, inverse-depth and accumulated-opacity maps of a rendered frame, ABI v22 (csrc/depth.hip) -----------------
 * For a pixel, let i run over the list entries the colour pass composited there (the first n_contrib entries of the
 * tile's list that pass the alpha >= 1/255 test: the colour pass's own decisions, taken with its own arithmetic),
 * w_i = alpha_i T_i and z_i the view-space depth of entry i's Gaussian:
 *     maps[0] = depth = sum_i w_i z_i,   maps[1] = invdepth = sum_i w_i / z_i,   maps[2] = alpha = sum_i w_i
 * alpha equals 1 - (final transmittance of the colour pass) bit for bit.  No background term; a pixel outside every
 * list is 0 in all three.  Kernels of their own: a frame that does not call these entry points runs exactly the launches
 * it ran before they existed, and GsrParams / GsrGrads keep their layouts.
 * GsrAuxFrame names the state a forward with p->forward_only = 0 left behind (the arguments of gsr_backward): both calls
 * only read it, so they may run before or after the frame's gsr_backward, any number of times. */
typedef struct GsrAuxFrame {
  int32_t P, width, height;
  int32_t binning_mode;          /* of the frame's forward */
  uint32_t num_rendered;         /* what the workspaces were laid out for: the real counts after the two-call forward, */
  uint32_t num_visible;          /*   (capacity, P) after gsr_forward */
  const void* geom_ws;           /* device; may be NULL when P == 0 */
  const void* bin_ws;            /* device; may be NULL when num_rendered == 0 */
  const void* img_ws;            /* device */
  const int32_t* radii;          /* device [P] (backward only) */
} GsrAuxFrame;

/* Gradient outputs of gsr_aux_maps_backward, each written in full: the maps' own contribution to the gradients of the
 * frame's inputs, in the conventions of GsrGrads (dL_dmeans2D included); the caller adds them to the colour path's.
 * dL_dscales / dL_drotations (with scales + rotations) or dL_dcov3D (with cov3D_precomp) may be NULL when not wanted.
 * With GsrParams.act_flags the gradients are those of the raw parameters, as in gsr_backward. */
typedef struct GsrAuxGrads {
  float* dL_dmeans3D;   /* device [P,3] */
  float* dL_dmeans2D;   /* device [P,3] */
  float* dL_dopacities; /* device [P] */
  float* dL_dscales;    /* device [P,3] */
  float* dL_drotations; /* device [P,4] */
  float* dL_dcov3D;     /* device [P,6] */
} GsrAuxGrads;

/* maps: device [3,H,W], written in full. */
int gsr_aux_maps_forward(const GsrAuxFrame* frame, float* maps, void* stream);
/* p: the inputs of the frame's forward (SH / colour members are not read).  dL_dmaps: device [3,H,W].
 * acc_ws: device scratch of gsr_aux_maps_backward_bytes(P) bytes, 256-byte aligned: the [P,8] float accumulator the
 * compositing backward adds into with float atomics (d mean2D x / y in pixels, d conic xx / xy / yy, d opacity, d z, one
 * spare word); the call zero-fills it.  Atomics reorder: the gradients are reproducible to rounding, not bit for bit. */
size_t gsr_aux_maps_backward_bytes(int32_t P);
int gsr_aux_maps_backward(const GsrParams* p, const GsrAuxFrame* frame, const float* dL_dmaps, void* acc_ws,
                          size_t acc_ws_bytes, const GsrAuxGrads* grads, void* stream);

/* ---- per-Gaussian feature vectors composited to C-channel maps of a rendered frame, ABI v26 (csrc/features.hip) -------
 * With i, w_i as above (the entries and weights of the depth / alpha maps) and features a device [P,C] float array,
 * contiguous and row-major, C >= 1:
 *     maps[c] = sum_i w_i features[id_i][c],   c = 0 .. C-1          (no background term, no clamp)
 * Kernels of their own; the frame is only read.  maps: device [C,H,W], written in full, the same bits
 * from run to run. */
int gsr_feature_maps_forward(const GsrAuxFrame* frame, const float* features, int32_t C, float* maps, void* stream);
/* p: the inputs of the frame's forward, as for gsr_aux_maps_backward.  dL_dmaps: device [C,H,W].
 * dL_dfeatures: device [P,C], written in full (zero-filled, then added into with float atomics); NULL: not wanted.
 * grads: the geometry gradients of the maps, as gsr_aux_maps_backward writes them; NULL: the feature gradient only -- the
 * per-Gaussian geometry kernel is not launched and acc_ws may be NULL.
 * acc_ws: device scratch of gsr_feature_maps_backward_bytes(P) bytes, 256-byte aligned (the [P,8] accumulator of
 * gsr_aux_maps_backward; its d z word stays 0).  Gradients are reproducible to rounding, not bit for bit. */
size_t gsr_feature_maps_backward_bytes(int32_t P);
int gsr_feature_maps_backward(const GsrParams* p, const GsrAuxFrame* frame, const float* features, int32_t C,
                              const float* dL_dmaps, float* dL_dfeatures, void* acc_ws, size_t acc_ws_bytes,
                              const GsrAuxGrads* grads, void* stream);

/* ---- absolute view-space gradient of a rendered frame (AbsGS), ABI v40 (csrc/abs_grad.hip) ----------
 * For Gaussian k let p run over the pixels where the colour pass composited k (the rule above), d = mean2D_k - p (pixels),
 * (cxx, cxy, cyy) its conic and h_kp = opacity_k G_kp dL/dalpha_kp of the COLOUR image for the incoming dL_dcolor,
 * background term included (the 0.99 clamp passes the gradient on, as in gsr_backward):
 *     abs_means2D[k][0] = 0.5 W sum_p | h_kp (cxx dx + cxy dy) |
 *     abs_means2D[k][1] = 0.5 H sum_p | h_kp (cxy dx + cyy dy) |,      abs_means2D[k][2] = 0
 * GsrGrads.dL_dmeans2D is the same sum taken with the terms' signs (times -1), so abs >= |dL_dmeans2D| per component up
 * to rounding.  A kernel of its own on the maps' walk; gsr_backward is untouched and a frame that does not call this entry
 * point runs exactly the launches it ran before.  The frame is only read, as for gsr_aux_maps_backward.
 * p: the inputs of the frame's forward; only P, width, height, forward_only, debug and bg are read.  dL_dcolor: device
 * [3,H,W].  abs_means2D: device [P,3], written in full (zero-filled, then added into with at most two float atomics per
 * tile and list entry): rows of Gaussians with radii == 0 and of Gaussians nothing composited are exactly 0.
 * Reproducible to rounding, not bit for bit. */
int gsr_abs_grad_backward(const GsrParams* p, const GsrAuxFrame* frame, const float* dL_dcolor, float* abs_means2D,
                          void* stream);

/* ---- depth-distortion map of a rendered frame, ABI v29 (csrc/distortion.hip) -------------------------
 * With i, w_i, z_i as above (the entries and weights of the depth / alpha maps), the regulariser of 2DGS:
 *     dist = sum_i sum_{j<i} w_i w_j (m_i - m_j)^2,   m_i = m(z_i)        (no background term)
 *     mapping 0 ("linear"): m(z) = z;   mapping 1 ("ndc"): m(z) = far / (far - near) * (1 - near / z)
 * evaluated with recurrences over differences of m, not as A M2 - M1^2: a pixel whose contributors lie in a thin slab
 * keeps its relative accuracy.  A pixel with zero or one contributor is exactly 0.  near / far are read with mapping 1 only.
 * dist: device [1,H,W], state: device [2,H,W], both written in full, the same bits from run to run.  state is what the
 * backward needs per pixel (m_last - mean m, dist / alpha); its content is opaque and belongs to the frame and mapping it
 * was written for.  Every argument is checked before any HIP call: GSR_E_BADARG for a mapping outside {0, 1}, mapping 1
 * without finite 0 < near < far, a NULL pointer, a workspace that is too small; GSR_E_ALIGN for acc_ws.  Nothing
 * allocates, synchronises or reads back. */
int gsr_distortion_forward(const GsrAuxFrame* frame, int32_t mapping, float near, float far, float* dist, float* state,
                           void* stream);
/* p: the inputs of the frame's forward, as for gsr_aux_maps_backward.  state: what the forward wrote; dL_ddist: device
 * [1,H,W].  acc_ws: device scratch of gsr_distortion_backward_bytes(P) bytes, 256-byte aligned (the [P,8] accumulator of
 * gsr_aux_maps_backward; the call zero-fills it).  grads: written in full, as by gsr_aux_maps_backward.  Gradients are
 * reproducible to rounding, not bit for bit (float atomics). */
size_t gsr_distortion_backward_bytes(int32_t P);
int gsr_distortion_backward(const GsrParams* p, const GsrAuxFrame* frame, int32_t mapping, float near, float far,
                            const float* state, const float* dL_ddist, void* acc_ws, size_t acc_ws_bytes,
                            const GsrAuxGrads* grads, void* stream);

/* ---- median-depth map and Gaussian id map of a rendered frame, ABI v30 (csrc/median.hip) ------------
 * With i, z_i as above (the entries of the depth / alpha maps, in list order) and T_i the colour pass's transmittance
 * BEFORE entry i (float32, its single-fma update), k* = the last composited entry with T_i > 0.5 -- the rule of 2DGS,
 * `if (T > 0.5) { median_depth = depth; median_contributor = i; }`:
 *     median = z_{k*},   median_id = id_{k*} (the Gaussian's row in the caller's tensors)
 * The first composited entry always qualifies (T = 1); a ray that never gets below one half keeps its last composited
 * entry; a pixel without a composited entry gets 0 / -1.  The walk of a pixel ends where its T reaches one half.
 * median: device [1,H,W] float32, median_id: device [H,W] int32, state: device [H,W] uint32, all three written in full,
 * the same bits from run to run.  state is what the backward needs per pixel (the list position of k*); its content is
 * opaque and belongs to the frame it was written for.  Every argument is checked before any HIP call.  Nothing allocates,
 * synchronises or reads back. */
int gsr_median_depth_forward(const GsrAuxFrame* frame, float* median, int32_t* median_id, uint32_t* state, void* stream);
/* The selection is piecewise constant: dL/dz_{k*} = dL_dmedian[pixel] and nothing else, so only means3D receives a
 * gradient: dL_dmeans3D[id] = (sum over the pixels that chose id of dL_dmedian) * viewmatrix[0:3, 2].
 * p: the inputs of the frame's forward; only P, width, height, forward_only, debug and viewmatrix are read.
 * state: what the forward wrote; dL_dmedian: device [1,H,W].  acc_ws: device scratch of
 * gsr_median_depth_backward_bytes(P) bytes, 256-byte aligned: a [P] float accumulator (the call zero-fills it) that
 * receives at most one float atomic per tile and list entry.  dL_dmeans3D: device [P,3], written in full (rows no pixel
 * chose are zero).  GSR_E_CAPACITY for a short workspace, GSR_E_ALIGN for acc_ws.  Gradients are reproducible to
 * rounding, not bit for bit (float atomics). */
size_t gsr_median_depth_backward_bytes(int32_t P);
int gsr_median_depth_backward(const GsrParams* p, const GsrAuxFrame* frame, const uint32_t* state, const float* dL_dmedian,
                              void* acc_ws, size_t acc_ws_bytes, float* dL_dmeans3D, void* stream);

/* ---- per-Gaussian contribution statistics of a rendered frame, ABI v24 (csrc/contribution.hip) ----------------------
 * For Gaussian g let p run over the pixels where the colour pass composited g (the rule above: the first n_contrib
 * entries of the tile's list that pass alpha >= 1/255) and w = alpha T, the weight the maps above sum.  Three int64 per
 * Gaussian, ADDED INTO the caller's buffer:
 *     stats[g][0] += sum_p round-to-nearest(w * 2^30)     (w <= 0.99, so a term fits 30 bits)
 *     stats[g][1] += number of such pixels
 *     stats[g][2]  = max(stats[g][2], float32 bit pattern of max_p w)   (w > 0: integer order is float order; 0 = never)
 * Integer adds and an integer max only: the result is the same bits from run to run and whatever the order of the
 * views, so many views accumulate in one buffer on the device.  Range of column 0: 2^63 / 2^30 weight units, about 4000
 * fully covered 1920x1080 frames for a single Gaussian.
 * pixel_mask: NULL, or device uint8 [H,W]: pixels whose byte is 0 are left out of all three numbers.
 * frame: the state of a forward with p->forward_only = 0 (the kernel reads the contributor counts); radii is not read.
 * A frame with P == 0 or num_rendered == 0 returns success and launches nothing.  stats: device [P,3], 8-byte aligned. */
int gsr_contribution_accumulate(const GsrAuxFrame* frame, const uint8_t* pixel_mask, int64_t* stats, void* stream);

/* `_C.mark_visible(means3D, viewmatrix, projmatrix)` of the upstream module (unused by the reference): visible[i] = 1
 * when Gaussian i passes the near-plane test of the preprocess stage (view z > 0.2). */
int gsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, uint8_t* visible, void* stream);

/* ---- unit entry points (each stage callable on its own; used by the parity tests) ------- */
/* keys_out/vals_out receive the result; *_tmp are scratch of the same size; bits sorted: [0,end_bit) */
size_t gsr_sort_scratch_bytes(uint32_t n);
int gsr_sort_pairs_u64(uint64_t* keys, uint32_t* vals, uint64_t* keys_tmp, uint32_t* vals_tmp,
                       uint32_t n, int32_t end_bit, void* scratch, void* stream,
                       int32_t* result_in_tmp /* host out: 1 if the sorted data ended in *_tmp */);
/* The 32-bit-key sorts of the two-level binning (the default mode), same conventions as gsr_sort_pairs_u64.
 * val_words = 1: uint32 values (the tile sort); 2: 8-byte values, 8-byte aligned (the depth sort's payload).
 * n_dev = NULL: `capacity` is the element count.  Otherwise the count is read from device memory (*n_dev <= capacity),
 * the grids are sized for `capacity`, and nothing at index *n_dev or beyond is read or written.  Buffers hold `capacity`
 * elements; scratch: gsr_sort_scratch_bytes(capacity).  end_bit in [0, 32]. */
int gsr_sort_pairs_u32(uint32_t* keys, void* vals, uint32_t* keys_tmp, void* vals_tmp, uint32_t capacity,
                       const uint32_t* n_dev, int32_t end_bit, int32_t val_words, void* scratch, void* stream,
                       int32_t* result_in_tmp);
/* One more stable pass on bits [shift, shift + nbits) of 32-bit keys with 8-byte values, nbits in [1, 8]: the depth
 * sort's top-digit pass.  Reads *_in, writes *_out; *n_dev = 0 writes nothing. */
int gsr_sort_extra_pass_u32(const uint32_t* keys_in, const void* vals_in, uint32_t* keys_out, void* vals_out,
                            uint32_t capacity, const uint32_t* n_dev, int32_t shift, int32_t nbits, void* scratch,
                            void* stream);
/* The tile sort of the two-level binning with what it derives from its own histograms: a gsr_sort_pairs_u32 (uint32
 * values) of keys in [0, n_keys), then -- when the sort took at most two passes (*runs_valid = 1) -- ranges[k] =
 * [first, last + 1) of key k in the sorted array, (0, 0) for a key without items, and `order`: per chunk of 8192 keys a
 * permutation of the chunk's keys, longest run first by length bucket.  With *runs_valid = 0 ranges and order are not
 * written.  ranges: device uint32 [n_keys, 2], 16-byte aligned (also the sort's scratch for relative runs); order:
 * device uint32 [n_keys].  end_bit: what the forward passes for an image of n_keys tiles, max(1, ceil(log2 n_keys))
 * (tile_sort_bits at the tile sort of enqueue_stage2, csrc/gsr_api.hip); n_keys <= 2^end_bit is required. */
int gsr_sort_tile_runs_u32(uint32_t* keys, uint32_t* vals, uint32_t* keys_tmp, uint32_t* vals_tmp, uint32_t capacity,
                           const uint32_t* n_dev, int32_t end_bit, uint32_t n_keys, void* ranges, uint32_t* order,
                           void* scratch, void* stream, int32_t* result_in_tmp, int32_t* runs_valid);
/* copies internal state out for inspection (any pointer may be NULL) */
int gsr_debug_read_geom(const void* geom_ws, int32_t P, float* xy /*[P,2]*/, float* conic_opacity /*[P,4]*/,
                        float* rgb /*[P,3]*/, float* depth /*[P]*/, uint32_t* tiles_touched /*[P]*/,
                        uint32_t* point_offsets /*[P]*/, uint32_t* rect /*[P,4] x0,y0,x1,y1*/,
                        uint32_t* clamped /*[P]*/, void* stream);
/* keys_sorted are the (tile<<32|depth) keys of the sorted instances (rebuilt from the result in two-level mode).
 * (num_rendered, num_visible) = what the binning workspace was laid out for: after gsr_forward that is (capacity, P),
 * and only the first real-count entries of the outputs are meaningful. */
int gsr_debug_read_binning(const void* geom_ws, int32_t P, const void* bin_ws, uint32_t num_rendered,
                           uint32_t num_visible, int32_t width, int32_t height, int32_t binning_mode,
                           uint64_t* keys_sorted, uint32_t* point_list, void* stream);
/* the device-side counters of a frame: out[0] num_rendered, [1] num_visible, [2] Gaussians with more than 64 instances
 * (their gradient rows are pre-summed cooperatively), [3] reserved, [4] ~(smallest depth key), [5] largest depth key,
 * [6] element count of the depth sort's top-digit pass (0: the frame's depths fit 24 key bits), [7] instances the binning
 * workspace received (min(num_rendered, capacity)).  Synchronises the stream. */
int gsr_debug_read_counts(const void* geom_ws, int32_t P, uint32_t out_host[8], void* stream);
int gsr_debug_read_image(const void* img_ws, int32_t width, int32_t height, float* final_T,
                         uint32_t* n_contrib, uint32_t* ranges /*[T,2]*/, void* stream);

/* forward compositing re-run with work counters; stats = device u64[8], zeroed by the caller:
 * [0] instances in all tile lists, [1] staged into LDS, [2] visited after the sub-block cull,
 * [3] sub-block evaluations, [4] evaluations with at least one contributing lane, [5] sum of per-tile last contributor */
int gsr_debug_render_stats(const GsrParams* p, const void* geom_ws, const void* bin_ws, void* img_ws,
                           uint32_t num_rendered, uint32_t num_visible, float* out_color, unsigned long long* stats,
                           void* stream);

/* ---- stage timers (opt-in; HIP events recorded on the call's stream around each stage) ------ */
enum {
  GSR_STAGE_PREPROCESS_FWD = 0, GSR_STAGE_SCAN, GSR_STAGE_DUPLICATE, GSR_STAGE_SORT, GSR_STAGE_RANGES,
  GSR_STAGE_RENDER_FWD, GSR_STAGE_RENDER_BWD, GSR_STAGE_PREPROCESS_BWD, GSR_STAGE_COUNT
};
int gsr_profile_create(void** handle);
int gsr_profile_destroy(void* handle);
/* waits for the recorded events, adds their elapsed times into ms_sum[GSR_STAGE_COUNT] and the number of
 * recorded intervals into counts[GSR_STAGE_COUNT], then clears the handle for reuse */
int gsr_profile_collect(void* handle, double* ms_sum, uint32_t* counts);
const char* gsr_stage_name(int32_t stage);
/* roctx ranges ("gsr:<stage>") around the same stages, for rocprofv3 --marker-trace.  Off by default;
 * on = 1 loads librocprofiler-sdk-roctx.so (or libroctx64.so) at run time and returns GSR_E_BADARG if neither is
 * there.  Process-wide switch, safe to call from any thread. */
int gsr_enable_markers(int32_t on);

/* ---- caller-side steps of the train loop ---------------------------- */
/* L1 loss (utils/loss_utils.py:17-18) forward + gradient in one pass:
 * loss_sum[0] = sum|x-gt| (written, not accumulated; the caller divides by n), dL_dx = sign(x-gt) * scale.
 * `workspace`: device scratch of gsr_l1_loss_workspace_bytes() for the per-block partial sums, which are added in a
 * fixed order (no atomics): the loss is bitwise reproducible from run to run. */
size_t gsr_l1_loss_workspace_bytes(void);
int gsr_l1_loss_fwd_bwd(const float* x, const float* gt, size_t n, float scale, float* loss_sum,
                        float* dL_dx, void* workspace, void* stream);
/* The reference's training loss (train.py:99-101) in two kernels: (1-lambda)*L1 + lambda*(1 - SSIM) with SSIM as
 * utils/loss_utils.py:23-63 (11x11 Gaussian window, sigma 1.5, zero padding, mean over C*H*W).
 * dssim_mode GSR_DSSIM_ONE_MINUS_MEAN: sums[0] += sum|x-gt|, sums[1] += sum SSIM
 *   (caller zero-fills; loss = (1-lambda)*sums[0]/n + lambda*(1 - sums[1]/n));
 * dssim_mode GSR_DSSIM_CLAMPED_HALF (the 2D script's combined_loss, 2d_gaussian_splatting.py:196-202):
 *   sums[1] += sum clamp((1-SSIM)/2, 0, 1); loss = (1-lambda)*sums[0]/n + lambda*sums[1]/n.
 * dL_dx receives the full gradient of that loss; workspace: gsr_l1_dssim_workspace_bytes (three derivative maps +
 * one pair of partial sums per 16x16 tile; the sums are formed in a fixed order, so the value is reproducible). */
#define GSR_DSSIM_ONE_MINUS_MEAN 0
#define GSR_DSSIM_CLAMPED_HALF 1
size_t gsr_l1_dssim_workspace_bytes(int32_t C, int32_t H, int32_t W);
int gsr_l1_dssim_loss_fwd_bwd(const float* x, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                              int32_t dssim_mode, float* sums, float* dL_dx, void* workspace, void* stream);

/* ---- per-view evaluation (train.py:210-235 training_report, metrics.py:71-78, render.py / train.py:63) ------------
 * gsr_eval_image: one streaming read of x, gt (device, [3,H,W] float32, contiguous) gives the view's L1, PSNR and, with
 * GSR_EVAL_SSIM, its SSIM (the training loss' 11x11 window, forward only: no derivative maps), and optionally the 8-bit
 * [H,W,3] image of x.  flags:
 *   GSR_EVAL_CLAMP_X / GSR_EVAL_CLAMP_GT  clamp that image to [0, 1] on load (training_report clamps both);
 *   GSR_EVAL_SSIM                         also run the SSIM tile kernel (same clamps);
 *   GSR_EVAL_PSNR_WHOLE                   PSNR of the whole image (psnr() of a [1,3,H,W] batch, metrics.py) instead of
 *                                         the mean of the three per-channel values (psnr() of a [3,H,W] image,
 *                                         training_report): the rows of utils/image_utils.py:18 view(shape[0], -1);
 *   GSR_EVAL_U8_TRUNCATE                  u8_out = (clamp(x,0,1) * 255) truncated (train.py:63); default
 *                                         (clamp(x,0,1) * 255 + 0.5) truncated (torchvision save_image).  The bytes
 *                                         always come from clamp(x, 0, 1), whatever GSR_EVAL_CLAMP_X says.
 * view_out (device float[GSR_EVAL_VIEW_FLOATS], or NULL): l1, psnr, ssim (0 without GSR_EVAL_SSIM), sum|d| of the three
 *   channels, sum d^2 of the three channels, PSNR of the three channels.  psnr = 20 log10(1 / sqrt(mse)): +inf for
 *   mse == 0, as the reference.
 * acc (device double[4], or NULL): {sum l1, sum psnr, sum ssim, views} += this view, in double before the rounding to
 *   float32 -- the reference's .double() running sums; the caller zero-fills it once and reads it back once per report.
 * u8_out (device uint8 [H,W,3], or NULL).  workspace: gsr_eval_workspace_bytes(C, H, W, flags) bytes of device scratch
 * for the per-block partial sums, which are added in a fixed order in double (no atomics: bitwise reproducible).
 * C must be 3.  Asynchronous on `stream`; nothing is allocated; arguments are checked before any HIP call.
 * gsr_image_to_u8: the conversion alone (flags: 0 or GSR_EVAL_U8_TRUNCATE); same bytes as the fused output. */
#define GSR_EVAL_CLAMP_X 1
#define GSR_EVAL_CLAMP_GT 2
#define GSR_EVAL_SSIM 4
#define GSR_EVAL_PSNR_WHOLE 8
#define GSR_EVAL_U8_TRUNCATE 16
#define GSR_EVAL_VIEW_FLOATS 12
size_t gsr_eval_workspace_bytes(int32_t C, int32_t H, int32_t W, int32_t flags);
int gsr_eval_image(const float* x, const float* gt, int32_t C, int32_t H, int32_t W, int32_t flags, float* view_out,
                   double* acc, uint8_t* u8_out, void* workspace, void* stream);
int gsr_image_to_u8(const float* x, int32_t C, int32_t H, int32_t W, int32_t flags, uint8_t* u8_out, void* stream);

/* BASELINE config 1: `generate_2D_gaussian_splatting(kernel_size, sigma_x, sigma_y, rho, coords, colours, image_size)`
 * (2D-Gaussian-Splatting-main/2d_gaussian_splatting.py:44-123) without the N x 3 x H x W intermediate.
 *   sigma_x, sigma_y, rho [N]; coords [N,2] (normalised translation, x then y); colours [N,3];
 *   ax [K]: the kernel-grid abscissae `-5 + 10 * linspace(0, 1, K)` as the host framework evaluates them (:66-71);
 *   out [3,H,W] channel-major (the reference returns `.permute(1, 2, 0)` of exactly that buffer, :120-121).
 * The workspace (gsr_splat2d_workspace_bytes, 256-byte aligned) carries the forward state to gsr_splat2d_backward.
 * not_pd_host, when non-NULL, makes the call synchronise the stream and receive 1 if any covariance has det <= 0
 * (the reference raises ValueError there, :59-61).  Returns GSR_E_BADARG if K > min(H, W) (:93-94) or K > 2048. */
size_t gsr_splat2d_workspace_bytes(int32_t N, int32_t H, int32_t W);
int gsr_splat2d_forward(int32_t N, int32_t K, int32_t H, int32_t W, const float* sigma_x, const float* sigma_y,
                        const float* rho, const float* coords, const float* colours, const float* ax, void* workspace,
                        size_t workspace_bytes, float* out, int32_t* not_pd_host, void* stream);
/* dL_dout [3,H,W] -> gradients of all five inputs (overwritten, not accumulated; deterministic). */
int gsr_splat2d_backward(int32_t N, int32_t K, int32_t H, int32_t W, const float* sigma_x, const float* sigma_y,
                         const float* rho, const float* ax, void* workspace, size_t workspace_bytes,
                         const float* dL_dout, float* dL_dsigma_x, float* dL_dsigma_y, float* dL_drho,
                         float* dL_dcoords, float* dL_dcolours, void* stream);
/* Replacement for `simple_knn._C.distCUDA2(points[N,3]) -> meanDist2[N]` (scene/gaussian_model.py:21,210; the
 * submodule is absent from the reference): mean of the squared distances to the 3 nearest OTHER points, exact. */
size_t gsr_knn3_workspace_bytes(int32_t N);
int gsr_dist2_knn3(const float* points, int32_t N, float* mean_dist2, void* workspace, size_t workspace_bytes,
                   void* stream);
/* scene/gaussian_model.py:775-777 + train.py:130 fused: for radii>0:
 * xyz_gradient_accum += ||dL_dmeans2D.xy||, denom += 1, max_radii2D = max(max_radii2D, radii) */
int gsr_densify_stats(int32_t P, const float* dL_dmeans2D /*[P,3]*/, const int32_t* radii,
                      float* xyz_gradient_accum, float* denom, float* max_radii2D, void* stream);
/* ABI v40, the accumulator of AbsGS / PGSR next to it: for radii>0: xyz_gradient_accum_abs += ||abs_means2D.xy||, with
 * abs_means2D what gsr_abs_grad_backward wrote.  The count (denom) is the one gsr_densify_stats keeps. */
int gsr_densify_stats_abs(int32_t P, const float* abs_means2D /*[P,3]*/, const int32_t* radii,
                          float* xyz_gradient_accum_abs, void* stream);

/* scene/gaussian_model.py:750-772 `densify_and_prune` (plain branch: clone :580-610, split :506-578 with N = 2,
 * postfix :466-504, prune :401-449) as one plan and one read-once / write-once pass per tensor.
 *   gsr_densify_plan: classifies every Gaussian from xyz_gradient_accum / denom (NaN -> 0), the RAW scaling [P,3] and
 *     RAW opacity [P]; percent_dense_extent = percent_dense * scene_extent; max_world_scale = 0.1 * extent, or < 0
 *     when the caller's max_screen_size is None / 0 (then only the opacity test prunes, :759-764).  Synchronises the
 *     stream and returns counts_host = {kept originals, kept clones, kept children PER COPY, split-selected}.
 *     The output has counts[0] + counts[1] + 2*counts[2] rows in the reference's order:
 *     [kept originals | clones | first children | second children].
 *   gsr_densify_gather_rows: dst[rows_out, row_floats] <- src[P, row_floats]; zero_new = 1 stores zeros in the appended
 *     rows (Adam exp_avg / exp_avg_sq of new points, :458-459).
 *   gsr_densify_split_children: overwrites the children's rows of dst_xyz / dst_scaling with
 *     R(rotation) (exp(scaling) * noise) + xyz and log(exp(scaling) / 1.6); noise [2*counts[3], 3] holds the standard-
 *     normal draws of `torch.normal(mean=0, std=stds)` (:537-539) in the reference's order (all first samples of the
 *     selected Gaussians, then all second samples). */
size_t gsr_densify_workspace_bytes(int32_t P);
int gsr_densify_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                     const float* opacity_raw, float grad_threshold, float percent_dense_extent, float min_opacity,
                     float max_world_scale, void* workspace, size_t workspace_bytes, uint32_t counts_host[4],
                     void* stream);
/* ABI v40: gsr_densify_plan with the absolute-gradient accumulator of AbsGS / PGSR (xyz_gradient_accum_abs [P], what
 * gsr_densify_stats-style accumulation of ||abs_means2D.xy|| left; same denom) and its threshold
 * (densify_abs_grad_threshold).  With grad = accum / denom and grad_abs = accum_abs / denom (NaN -> 0 each) and
 * big = max(exp(scaling)) > percent_dense_extent:
 *     clone  unchanged: grad >= grad_threshold and !big
 *     split           : (grad >= grad_threshold || grad_abs >= abs_grad_threshold) and big
 *     prune  unchanged
 * This rule and nothing more: no parity with any one upstream trainer is claimed beyond it.  xyz_gradient_accum_abs ==
 * NULL: the rule of gsr_densify_plan (which is this call with NULL), abs_grad_threshold is not read.  Workspace, counts
 * and the gather / children calls are those of gsr_densify_plan. */
int gsr_densify_plan_abs(int32_t P, const float* xyz_gradient_accum, const float* xyz_gradient_accum_abs,
                         const float* denom, const float* scaling_raw, const float* opacity_raw, float grad_threshold,
                         float abs_grad_threshold, float percent_dense_extent, float min_opacity, float max_world_scale,
                         void* workspace, size_t workspace_bytes, uint32_t counts_host[4], void* stream);
int gsr_densify_gather_rows(int32_t P, int32_t row_floats, const float* src, const void* workspace,
                            const uint32_t counts[4], int32_t zero_new, float* dst, void* stream);
int gsr_densify_split_children(int32_t P, const float* xyz, const float* scaling_raw, const float* rotation_raw,
                               const float* noise, const void* workspace, const uint32_t counts[4], float* dst_xyz,
                               float* dst_scaling, void* stream);

/* The fork's grow / learned-split branch of render() (gaussian_renderer/__init__.py:91-253), ABI v14.  Every frame the
 * branch runs, G "virtual" Gaussians are appended after the P of the model (row P + j has source row src[j], in row
 * order), the extended raw-parameter arrays feed the rasterizer unchanged, and the gradients of the virtual rows are
 * folded back onto their sources.  mode: GSR_GROW_DIR or GSR_GROW_CONTINUOUS (grow mode, :94-119, optionally with
 * GSR_GROW_DISTANCE), else GSR_SPLIT_DISTANCE and / or GSR_SPLIT_SCALE (learned split, :186-253).
 *   gsr_grow_plan: g = xyz_gradient_accum / denom (NaN -> 0); grow mode selects |g| >= grad_threshold, split mode
 *     |g| >= grad_threshold & max(exp(scaling_raw)) > percent_dense_extent.  Writes vidx[P] (virtual row or -1),
 *     src[P] (first G entries used) and selected[P] (0 / 1), synchronises the stream and returns counts_host =
 *     {G, selected rows whose max scale exceeds percent_dense_extent}.
 *   gsr_grow_expand: out arrays have P + G rows: bit copies, then the grown / split positions and split scales
 *     (raw - log(k)).  noise [G,3]: the standard-normal draws of torch.normal(0, stds) when GSR_SPLIT_DISTANCE is off.
 *   gsr_grow_fold: GsrGrowGrads.in[k] are the [P+G]-row gradients of (xyz, means2D, f_dc, f_rest, opacity, scaling,
 *     rotation), out[k] the [P]-row gradients of the same inputs; d_* the dense [P, ...] gradients of the learned
 *     tensors of the mode (NULL otherwise), zeroed by the caller: only the selected rows are written. */
enum {
  GSR_GROW_DIR = 1,
  GSR_GROW_CONTINUOUS = 2,
  GSR_GROW_DISTANCE = 4,
  GSR_SPLIT_DISTANCE = 8,
  GSR_SPLIT_SCALE = 16
};

typedef struct GsrGrow {
  int32_t P, G, mode, num_dirs, n_rest;        /* n_rest: floats per row of f_rest (45 or 0) */
  const float* xyz;                            /* device [P,3] raw model tensors */
  const float* f_dc;                           /* [P,1,3] */
  const float* f_rest;                         /* [P,15,3] or NULL */
  const float* opacity;                        /* [P,1] raw */
  const float* scaling;                        /* [P,3] raw */
  const float* rotation;                       /* [P,4] raw */
  const float* dirs_prob;                      /* [P,num_dirs] logits (GSR_GROW_DIR) */
  const float* dirs;                           /* [num_dirs,3] (GSR_GROW_DIR) */
  const float* conti_dirs;                     /* [P,3] (GSR_GROW_CONTINUOUS) */
  const float* grow_dist;                      /* [P,1] raw (GSR_GROW_DISTANCE) */
  const float* split_distance;                 /* [P,3] raw (GSR_SPLIT_DISTANCE) */
  const float* split_scale;                    /* [P,1] raw (GSR_SPLIT_SCALE) */
  const float* noise;                          /* [G,3] (split without GSR_SPLIT_DISTANCE) */
  const int32_t* vidx;                         /* [P] from gsr_grow_plan */
  const int32_t* src;                          /* [G] from gsr_grow_plan */
} GsrGrow;

typedef struct GsrGrowGrads {
  const float* in[7];
  float* out[7];
  float* d_dirs_prob;
  float* d_conti_dirs;
  float* d_grow_dist;
  float* d_split_distance;
  float* d_split_scale;
} GsrGrowGrads;

size_t gsr_grow_workspace_bytes(int32_t P);
int gsr_grow_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                  float grad_threshold, float percent_dense_extent, int32_t mode, void* workspace, size_t workspace_bytes,
                  int32_t* vidx, int32_t* src, uint8_t* selected, uint32_t counts_host[2], void* stream);
int gsr_grow_expand(const GsrGrow* g, float* xyz_out, float* f_dc_out, float* f_rest_out, float* opacity_out,
                    float* scaling_out, float* rotation_out, void* stream);
int gsr_grow_fold(const GsrGrow* g, const GsrGrowGrads* grads, void* stream);

/* The fork's densify_and_prune (scene/gaussian_model.py:751-773), ABI v15: the clone + split branch with the learned
 * tensors (:509-610) and the grow branch (densify_and_grow :612-677, densify_and_growsplit :679-749), then the prune,
 * as one plan and one read-once / write-once pass per tensor.  mode: the GSR_GROW_* / GSR_SPLIT_* bits of the model's
 * flags, GSR_DENSIFY_GROW when the grow branch runs (:755), GSR_DENSIFY_SYMMETRIC for modelcg.symmetric_split.
 *   gsr_densify_fork_plan: as gsr_densify_plan, with split_scale_raw [P,1] (NULL without learn_split_scale) giving
 *     each row's child divisor 2 (0.6 sigmoid + 0.5) instead of 1.6 (:560-563, also in the children's prune test).
 *     Synchronises the stream and returns counts_host = {kept originals, kept clones / grown copies, kept children
 *     PER COPY, split-selected, selected}.  The output has counts[0] + counts[1] + c * counts[2] rows, c = 4 in the
 *     grow branch (children of the originals and of their grown copies), else 2:
 *       [kept originals | clones or grown | first children (of originals, then of grown) | second children (same)]
 *   gsr_densify_fork_gather_rows: dst[rows_out, row_floats] <- src[P, row_floats] with a value policy per role
 *     (GSR_ROW_POLICY(selected originals, clones / grown, children)): GSR_ROW_COPY, GSR_ROW_CONST (`value`: 0 for the
 *     new rows' Adam moments :458-459 and the re-inits of :560-574 / :653-655, 1 / num_dirs for :646-648) or
 *     GSR_ROW_SKIP (written by gsr_densify_fork_rows).  Originals that are not selected always copy.
 *   gsr_densify_fork_rows: the computed rows -- grown xyz + dir * max(exp(scaling)) * d (:617-635, dir the largest
 *     logit of _dirs_prob, lowest index on ties, or normalize(_conti_dirs)), the children's xyz R s + centre and
 *     scaling log(exp(scaling) / k), and (conti_out != NULL) normalize(dir_noise) into every row of a selected Gaussian
 *     (:650-651).  noise: the standard-normal draws of torch.normal(0, stds) over the split rows of the reference's
 *     order, [2n,3], or [n,3] with GSR_DENSIFY_SYMMETRIC (second child = -first), unused with GSR_SPLIT_DISTANCE;
 *     n = counts[3] (clone + split) or 2 counts[3] (grow).  dir_noise [counts[4],3]: torch.randn of :650. */
enum {
  GSR_DENSIFY_GROW = 32,
  GSR_DENSIFY_SYMMETRIC = 64
};
enum { GSR_ROW_COPY = 0, GSR_ROW_CONST = 1, GSR_ROW_SKIP = 2 };
#define GSR_ROW_POLICY(orig_sel, extra, child) ((orig_sel) | ((extra) << 2) | ((child) << 4))

typedef struct GsrDensifyFork {
  int32_t P, mode, num_dirs;
  const float* xyz;                            /* device [P,3] raw model tensors */
  const float* scaling;                        /* [P,3] raw */
  const float* rotation;                       /* [P,4] raw */
  const float* dirs_prob;                      /* [P,num_dirs] (grow branch with GSR_GROW_DIR) */
  const float* dirs;                           /* [num_dirs,3] (grow branch with GSR_GROW_DIR) */
  const float* conti_dirs;                     /* [P,3] (grow branch with GSR_GROW_CONTINUOUS) */
  const float* grow_dist;                      /* [P,1] raw (grow branch with GSR_GROW_DISTANCE) */
  const float* split_distance;                 /* [P,3] raw (GSR_SPLIT_DISTANCE) */
  const float* split_scale;                    /* [P,1] raw (GSR_SPLIT_SCALE) */
  const float* noise;                          /* split draws, see above */
  const float* dir_noise;                      /* [counts[4],3] (conti_out != NULL) */
} GsrDensifyFork;

size_t gsr_densify_fork_workspace_bytes(int32_t P);
int gsr_densify_fork_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                          const float* opacity_raw, const float* split_scale_raw, float grad_threshold,
                          float percent_dense_extent, float min_opacity, float max_world_scale, void* workspace,
                          size_t workspace_bytes, uint32_t counts_host[5], void* stream);
int gsr_densify_fork_gather_rows(int32_t P, int32_t row_floats, const float* src, const void* workspace,
                                 const uint32_t counts[5], int32_t grow_branch, int32_t policy, float value, float* dst,
                                 void* stream);
int gsr_densify_fork_rows(const GsrDensifyFork* f, const void* workspace, const uint32_t counts[5], float* xyz_out,
                          float* scaling_out, float* conti_dirs_out, void* stream);

/* One Adam step over up to GSR_ADAM_MAX_TENSORS tensors in one launch, ABI v16: the update of torch.optim.Adam's
 * default (`foreach`) path, `_multi_tensor_adam` with weight_decay = 0, amsgrad = maximize = capturable = False, as the
 * reference's `gaussians.optimizer.step()` runs it (train.py:136-139; optimizer built at scene/gaussian_model.py:264).
 * Per element, each line one torch op with its own float32 rounding:
 *     exp_avg    = lerp(exp_avg, grad, lerp_weight)            (ATen/native/Lerp.h, small-weight branch for |w| < 0.5)
 *     exp_avg_sq = exp_avg_sq * beta2
 *     exp_avg_sq = exp_avg_sq + sq_weight * (grad * grad)       (addcmul)
 *     d = sqrt(exp_avg_sq);  d = d / bc2_sqrt;  d = d + eps
 *     param      = param + step_size * (exp_avg / d)            (addcdiv)
 * The scalars are torch's, computed by the caller in double and converted to float: lerp_weight = 1 - beta1,
 * sq_weight = 1 - beta2, bc2_sqrt = (1 - beta2**step) ** 0.5, step_size = -(lr / (1 - beta1**step)), step the
 * tensor's own count after its increment.  All four arrays are contiguous fp32 with `numel` elements and must not
 * overlap; any alignment (16-byte aligned tensors take 16-byte accesses).  Entries with numel = 0 are skipped.
 * Returns GSR_E_BADARG for a NULL batch, count outside 0..GSR_ADAM_MAX_TENSORS, a negative numel or a NULL array of a
 * non-empty entry.  No host synchronisation. */
#define GSR_ADAM_MAX_TENSORS 16

typedef struct GsrAdamTensor {
  float* param;                                /* device [numel], updated in place */
  const float* grad;                           /* device [numel] */
  float* exp_avg;                              /* device [numel], updated in place */
  float* exp_avg_sq;                           /* device [numel], updated in place */
  int64_t numel;
  float lerp_weight, beta2, sq_weight, bc2_sqrt, eps, step_size;
} GsrAdamTensor;

typedef struct GsrAdamBatch {
  int32_t count;                               /* entries of t[] in use */
  int32_t reserved;                            /* 0 */
  GsrAdamTensor t[GSR_ADAM_MAX_TENSORS];
} GsrAdamBatch;

int gsr_adam_step(const GsrAdamBatch* batch, void* stream);

/* The same step for the rows one frame saw, ABI v21 ("sparse Adam").  Every tensor of the batch is [rows, numel / rows]
 * and `visibility` has one entry per row: GSR_ADAM_VIS_U8, one byte, visible iff non-zero (a torch bool / uint8
 * tensor), or GSR_ADAM_VIS_I32, an int32, visible iff > 0 (the rasterizer's `radii`, as it stands).
 *   visible rows:   every element gets exactly the update of gsr_adam_step, bit for bit;
 *   invisible rows: param, exp_avg and exp_avg_sq keep their bits (NaN payloads included) and the gradient is never
 *                   used: a NaN or Inf there reaches nothing.
 * Memory that holds invisible rows only is neither read nor written (in 16-byte pieces on the aligned path, per element
 * otherwise); a 16-byte piece that two rows of different visibility share is read and written back whole.  The scalars
 * of t[] are those of gsr_adam_step: the caller counts a step for every tensor it passes, seen or not, so a visible row
 * gets what the dense step would have given it from the same state.  (This is not the sparse kernel of upstream 3DGS,
 * which drops the bias correction.)
 * Returns GSR_E_BADARG for the cases of gsr_adam_step and for an unknown visibility_kind, negative rows, a NULL
 * visibility with a non-empty tensor and a numel that is not a multiple of rows; GSR_E_ALIGN for an int32 visibility
 * that is not 4-byte aligned.  No host synchronisation, no allocation. */
#define GSR_ADAM_VIS_U8 0
#define GSR_ADAM_VIS_I32 1

typedef struct GsrAdamRowsBatch {
  const void* visibility;                      /* device [rows], see visibility_kind */
  int64_t rows;
  int32_t visibility_kind;                     /* GSR_ADAM_VIS_* */
  int32_t count;                               /* entries of t[] in use */
  GsrAdamTensor t[GSR_ADAM_MAX_TENSORS];       /* row_floats of t[k] = t[k].numel / rows */
} GsrAdamRowsBatch;

int gsr_adam_step_rows(const GsrAdamRowsBatch* batch, void* stream);

/* The model's per-opacity lifecycle steps, ABI v18 (csrc/model.hip).  opacity_raw is the model's `_opacity`, device
 * [P,1] fp32, pre-activation.  Nothing here allocates, synchronises or reads back: every call can sit in a captured
 * graph.
 *   gsr_opacity_sparsity_fwd: the fork's sparsity term of train.py:102-106.  With o = sigmoid(raw) in float,
 *     S = {i : o_i < threshold} (train.py:102 uses 0.005) and n = |S|, writes the 16-byte aligned device record
 *       record[0] = float  weight / n * sum_S |o_i - 1|     (0 when n == 0: the reference skips the term, :104)
 *       record[1] = uint32 n
 *       record[2] = float  weight / n                        (0 when n == 0)
 *       record[3] = 0
 *     One streaming pass leaves a (sum, count) pair per block in `workspace`
 *     (gsr_opacity_sparsity_workspace_bytes(), 4-byte aligned), one block adds them in a fixed order in double: the
 *     result is the same from run to run.
 *   gsr_opacity_sparsity_bwd: grad_raw[i] = grad_out[0] * record[2] * sign(o_i - 1) * o_i * (1 - o_i) on S, 0
 *     elsewhere (dense [P,1]).  grad_out is the DEVICE address of the upstream 0-dim gradient.
 *   gsr_reset_opacity: reset_opacity (scene/gaussian_model.py:312-315) in place: raw <- log(c / (1 - c)) with
 *     c = min(sigmoid(raw), cap), each op rounded to float as torch does (rows below the cap make the round trip too),
 *     and exp_avg / exp_avg_sq (each NULL or [P]) zero-filled as replace_tensor_to_optimizer does (:391-392). */
size_t gsr_opacity_sparsity_workspace_bytes(void);
int gsr_opacity_sparsity_fwd(const float* opacity_raw, int64_t P, float weight, float threshold, float* record,
                             void* workspace, void* stream);
int gsr_opacity_sparsity_bwd(const float* opacity_raw, int64_t P, float threshold, const float* record,
                             const float* grad_out, float* grad_raw, void* stream);
int gsr_reset_opacity(float* opacity_raw, int64_t P, float cap, float* exp_avg, float* exp_avg_sq, void* stream);

/* Load-time image ingest, ABI v19 (csrc/image.hip): the per-image work of the reference's scene loading between the
 * file decode and the training target, on the caller's stream.  Images are device uint8, HWC, densely packed.
 *   gsr_image_composite_u8: the Blender reader's alpha composite (scene/dataset_readers.py:204-210).  rgba [H,W,4]
 *     (4-byte aligned) -> rgb [H,W,3]; per channel, in float64 with every operation rounded on its own,
 *       n = v / 255.0;  arr = n_rgb * n_a + bg * (1 - n_a);  byte = low 8 bits of trunc(arr * 255.0)
 *     (the reference casts to int8 and hands those bytes to an 8-bit RGB image).  bg: three values in [0, 1].
 *   gsr_image_resize_u8: Pillow's Image.resize((out_w, out_h)) with its default bicubic filter for C = 1 or 3, bit
 *     for bit: a horizontal pass, then a vertical one; a pass whose size does not change is skipped (with neither, a
 *     copy).  Per output index o a pass reads bounds[2o] = first input index, bounds[2o+1] = tap count (<= ksize) and
 *     int32 taps[o*ksize .. ], the host's restatement of Pillow's precompute_coeffs / normalize_coeffs_8bpc
 *     (image_ingest.resize_tables); out = clamp((2^21 + sum pixel * tap) >> 22, 0, 255), stored as uint8 between the
 *     passes.  h_* may be NULL when out_w == in_w, v_* when out_h == in_h; tmp ([in_h, out_w, C] bytes) only when both
 *     passes run.  src, tmp and dst must not overlap.
 *   gsr_image_to_float_chw: src [H,W,C], C = 3 or 4 (4: 4-byte aligned) -> dst float [3,H,W]:
 *     clamp(float(v) / 255.0f, 0, 1), times float(a) / 255.0f when C == 4 (utils/general_utils.py:21-27,
 *     utils/camera_utils.py:43-47, scene/cameras.py:39-46); bit-equal to torch's `uint8 / 255.0` and `*=`. */
int gsr_image_composite_u8(const uint8_t* rgba, int32_t H, int32_t W, double bg_r, double bg_g, double bg_b,
                           uint8_t* rgb, void* stream);
int gsr_image_resize_u8(const uint8_t* src, int32_t C, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                        const int32_t* h_bounds, const int32_t* h_taps, int32_t h_ksize, const int32_t* v_bounds,
                        const int32_t* v_taps, int32_t v_ksize, uint8_t* tmp, uint8_t* dst, void* stream);
int gsr_image_to_float_chw(const uint8_t* src, int32_t C, int32_t H, int32_t W, float* dst, void* stream);

/* Per-image exposure compensation, ABI v23 (csrc/exposure.hip): upstream 3DGS's learnable 3x4 colour affine on the
 * rendered image.  x, y, g, dx: device fp32 [3,H,W] in planes; A, dA: device fp32 [3,4] row-major, read from device
 * memory.  With k the input channel, c the output channel and p the pixel,
 *     y[c,p]  = x[0,p]*A[0,c] + x[1,p]*A[1,c] + x[2,p]*A[2,c] + A[c,3]
 *     dx[k,p] = A[k,0]*g[0,p] + A[k,1]*g[1,p] + A[k,2]*g[2,p]                    (g = dL/dy)
 *     dA[k,c] = sum_p x[k,p]*g[c,p]  (k, c in 0..2)        dA[c,3] = sum_p g[c,p]
 * (upstream's matmul(img.permute(1,2,0), A[:3,:3]).permute(2,0,1) + A[:3,3,None,None]); no clamp.  y and dx are summed
 * left to right as written, every operation rounded to float32 on its own: with A = eye(3,4) and finite inputs y == x
 * and dx == g bit for bit (a -0 comes out as +0).  dA: products and sums in double, one 12-double slot per block in
 * `workspace` (gsr_exposure_workspace_bytes(H, W) bytes, 8-byte aligned), the slots added by one block in a fixed order,
 * one rounding to float32; no atomics, the same bits from run to run.
 * dx may be NULL (the image needs no gradient; A may then be NULL) and dA may be NULL (the exposure needs none; x and
 * workspace may then be NULL).  Nothing here allocates, synchronises or reads back. */
size_t gsr_exposure_workspace_bytes(int32_t H, int32_t W);
int gsr_exposure_apply_fwd(const float* x, const float* A, int32_t H, int32_t W, float* y, void* stream);
int gsr_exposure_apply_bwd(const float* x, const float* A, const float* g, int32_t H, int32_t W, float* dx, float* dA,
                           void* workspace, void* stream);

/* MCMC densification ("3DGS as Markov-chain Monte Carlo"), ABI v25 (csrc/mcmc.hip; mcmc.py).
 * Every input is a RAW model tensor, device fp32: opacity_raw [P,1], scaling_raw [P,3], rotation_raw [P,4] (16-byte
 * aligned).  The activations are formed in float32 exactly as GSR_ACT_* forms them in preprocess:
 *     o = 1 / (1 + expf(-raw))      s = expf(raw)      q = raw / fmaxf(sqrtf(((x x + y y) + z z) + w w), 1e-12f)
 * Every call is asynchronous on `stream`, allocates nothing, reads nothing back and can sit in a captured graph; it
 * returns GSR_E_BADARG (NULL pointer, a count outside 0..2^31-1, a workspace that is too small) or GSR_E_ALIGN before
 * any HIP call, and 0 without a launch for an empty problem.  No kernel waits on another workgroup.
 *
 *   gsr_mcmc_noise: xyz [P,3] += Sigma v in place, Sigma = R(q) diag(s^2) R(q)^T never formed, noise [P,3] the caller's
 *     standard-normal draws.  One streaming pass (56 B read, 12 B written per row), float32, no contraction, in this
 *     order:
 *         gate = 1 / (1 + expf(-100 * ((1 - o) - 0.995f)))           v_k = (noise_k * gate) * step_scale
 *         R = the rotation of q as preprocess forms it for cov3D (r, x, y, z = q[0..3])
 *         u_j = (R_0j v_0 + R_1j v_1) + R_2j v_2     w_j = (s_j s_j) u_j     d_i = (R_i0 w_0 + R_i1 w_1) + R_i2 w_2
 *         xyz_i = xyz_i + d_i
 *     A row with o >= 0.9 has gate == 0 exactly (expf overflows to +inf) and keeps its bits, as does a row whose noise
 *     is 0 (a -0 coordinate comes out as +0).
 *   gsr_mcmc_reg_fwd: record (16-byte aligned, 4 floats) =
 *         { opacity_reg * mean_i o_i + scale_reg * mean_ij s_ij,  opacity_reg / P,  scale_reg / (3 P),  0 }
 *     The float32 activations are added in double, one pair of sums per block in `workspace`
 *     (gsr_mcmc_reg_workspace_bytes(), 8-byte aligned), the pairs by one block in a fixed order; each record entry is
 *     rounded once from double.  The same bits from run to run.
 *   gsr_mcmc_reg_bwd: grad_opacity [P,1] = (g * record[1]) * (o * (1 - o)), grad_scaling [P,3] = (g * record[2]) * s,
 *     dense; g = grad_out[0], the DEVICE address of the upstream 0-dim gradient.
 *   gsr_mcmc_sample: n samples with replacement, exact in integers.  w_i = round-to-nearest(o_i 2^30) as int64 where
 *     o_i > alive_threshold, else 0 (alive_threshold < 0: every row); C_i the inclusive prefix sum, T = C_{P-1}.  For
 *     draw r = draws[j] (int64, uniform in [0, 2^63)): t = floor(r T / 2^63) by the 128-bit product, idx_out[j] (int32) =
 *     the smallest i with C_i > t: a row of weight 0 is never returned.  count_out [P] (int32) is zero-filled, then
 *     counts the samples per row (integer atomics).  T == 0: every idx_out is -1, the counts are 0.  T stays on the
 *     device.  workspace: gsr_mcmc_sample_workspace_bytes(P) bytes, 8-byte aligned.  Every output is the same bits
 *     whatever the launch shape.
 *   gsr_mcmc_relocation: per sample j, with i = idx[j] and N = min(count[i] + 1, 51), in double from the float32
 *     activations o, s to one final rounding:
 *         o' = 1 - (1 - o)^(1/N)
 *         D  = sum_{m=1..N} sum_{k=0..m-1} C(m-1,k) (-1)^k / sqrt(k+1) * o'^(k+1)       (m outer, k inner, ascending)
 *         new_scaling_raw[j]  = log((o / D) * s)
 *         new_opacity_raw[j]  = log(o'' / (1 - o'')),  o'' = clamp(o', 0.005, 1 - 2^-23)
 *     A pure function of the sample: the outputs are arrays of their own ([n], [n,3]).  idx[j] < 0 writes zeros. */
int gsr_mcmc_noise(int64_t P, float* xyz, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                   const float* noise, float step_scale, void* stream);
size_t gsr_mcmc_reg_workspace_bytes(void);
int gsr_mcmc_reg_fwd(const float* opacity_raw, const float* scaling_raw, int64_t P, float opacity_reg, float scale_reg,
                     float* record, void* workspace, size_t workspace_bytes, void* stream);
int gsr_mcmc_reg_bwd(const float* opacity_raw, const float* scaling_raw, int64_t P, const float* record,
                     const float* grad_out, float* grad_opacity, float* grad_scaling, void* stream);
size_t gsr_mcmc_sample_workspace_bytes(int64_t P);
int gsr_mcmc_sample(int64_t P, const float* opacity_raw, float alive_threshold, const int64_t* draws, int64_t n,
                    int32_t* idx_out, int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream);
int gsr_mcmc_relocation(int64_t n, const int32_t* idx, const int32_t* count, const float* opacity_raw,
                        const float* scaling_raw, float* new_opacity_raw, float* new_scaling_raw, void* stream);

/* ---- TSDF fusion of depth maps and marching-tetrahedra mesh extraction, ABI v27 (csrc/tsdf.hip; tsdf.py)
 * A dense volume of nx x ny x nz grid points; point (i, j, k) is the sample at origin + voxel_size * (i, j, k), linear
 * index (k * ny + j) * nx + i.  Device fields, float32, contiguous: tsdf [nz,ny,nx] (1 = untouched), weight [nz,ny,nx],
 * color [nz,ny,nx,3] or NULL.  Indices are 32-bit: 7 * nx * ny * nz < 2^31 is required (seven edge slots per point).
 * Every call checks its arguments before any HIP call (GSR_E_BADARG: NULL pointer, non-positive dims / voxel_size /
 * sdf_trunc / image size / weight, an index space or launch that would overflow; GSR_E_ALIGN), is asynchronous on
 * `stream`, allocates nothing and reads nothing back. */
typedef struct GsrTsdfVolume {
  int32_t nx, ny, nz;
  float origin[3];
  float voxel_size, sdf_trunc;
  float* tsdf;
  float* weight;
  float* color;
} GsrTsdfVolume;

typedef struct GsrTsdfView {
  int32_t width, height;
  float fx, fy;                 /* W / (2 tan_fovx), H / (2 tan_fovy): the rasterizer's pixel-centre convention with */
                                /* cx = (W - 1) / 2, cy = (H - 1) / 2 */
  float weight;                 /* > 0 */
  float max_depth, max_weight;  /* +inf: none */
  const float* viewmatrix;      /* device [16], row-vector convention */
  const float* depth;           /* device [H,W]; 0 marks an invalid pixel */
  const float* color;           /* device [3,H,W]; given exactly when the volume has a colour field */
} GsrTsdfView;

/* One launch, one lane per grid point, float32 with every operation rounded on its own; the order is the header comment
 * of csrc/tsdf.hip: project, nearest pixel, sdf = d - z, skip if z <= 0.2 / outside the image / d <= 0 / d > max_depth /
 * sdf < -sdf_trunc, else running averages of min(1, sdf / sdf_trunc) and the pixel's colour with the view's weight.
 * Skipped points are not written. */
int gsr_tsdf_integrate(const GsrTsdfVolume* vol, const GsrTsdfView* view, void* stream);
/* Marching tetrahedra on the Kuhn decomposition, first half.  Per grid point (uint8 [nz,ny,nx] each, written in full):
 * tri_count = triangles of the cube based there (0 unless all eight corner weights >= min_weight), edge_mask = the owned
 * edges (directions (1,0,0) (0,1,0) (0,0,1) (1,1,0) (0,1,1) (1,0,1) (1,1,1) = bits 0..6) that carry a referenced vertex,
 * vert_count = its population count.  The caller scans vert_count and tri_count (exclusive, int64) and reads the totals. */
int gsr_tsdf_mesh_count(const GsrTsdfVolume* vol, float min_weight, uint8_t* tri_count, uint8_t* edge_mask,
                        uint8_t* vert_count, void* stream);
/* Second half: vertices [V,3] float32 ordered by (owning point, direction), vcolors [V,3] or NULL (needs vol->color),
 * faces [F,3] int32 ordered by (cube, tetrahedron, triangle), wound so that normals point from tsdf < 0 to tsdf >= 0.
 * vert_offs / tri_offs: the exclusive scans, device int64 [nz,ny,nx], 8-byte aligned.  V and F must be positive (an
 * empty mesh needs no call); nothing at or beyond row V / F is written whatever the offsets hold.  Plain stores at
 * slots the scans fix: the same bits from run to run. */
int gsr_tsdf_mesh_emit(const GsrTsdfVolume* vol, const uint8_t* tri_count, const uint8_t* edge_mask,
                       const int64_t* vert_offs, const int64_t* tri_offs, int64_t V, int64_t F, float* vertices,
                       float* vcolors, int32_t* faces, void* stream);

/* ---- TSDF fusion in contracted space: unbounded scenes, ABI v33 (csrc/tsdf.hip; tsdf.py)
 * The Mip-NeRF 360 contraction of a normalised point x = (p - center) / radius: contract(x) = x for |x| <= 1 and
 * (2 - 1 / |x|) x / |x| otherwise.  Its inverse on |q| < 2 with m = |q|: s = 1, g = 1 for m <= 1; s = 1 / ((2 - m) m),
 * g = 1 / (2 - m) for m > 1; p = center + radius * (q * s).  A contracted volume is a GsrTsdfVolume (same fields, layout
 * and index limits) whose grid point (i, j, k) is the contracted-space sample q = origin + voxel_size * (i, j, k);
 * sdf_trunc stays in world units, as it applies inside the unit ball. */
typedef struct GsrTsdfContraction {
  float center[3];
  float radius;                 /* > 0, finite */
  float q_max;                  /* in (1, 2): grid points with |q| >= q_max are never touched */
} GsrTsdfContraction;
/* gsr_tsdf_integrate on a contracted volume, one launch of the same kernel body.  Per grid point, float32, every
 * operation rounded on its own: m2 = (q.x q.x + q.y q.y) + q.z q.z, skip unless m2 < q_max q_max (before any load);
 * m = sqrtf(m2); p = center + radius * (q * s); trunc = sdf_trunc * g; then the sequence of gsr_tsdf_integrate from p on
 * with trunc in the place of sdf_trunc.  With center 0, radius 1 and every |q| <= 1 the result is gsr_tsdf_integrate's
 * bit for bit.  Checked before any HIP call: everything gsr_tsdf_integrate checks, and GSR_E_BADARG for a NULL
 * contraction, a center or radius that is not finite, radius <= 0, q_max outside (1, 2). */
int gsr_tsdf_integrate_contracted(const GsrTsdfVolume* vol, const GsrTsdfContraction* contraction, const GsrTsdfView* view,
                                  void* stream);
/* xyz device float32 [n,3], in place, one lane per row: q -> center + radius * (q * s), s as above from
 * m2 = (q.x q.x + q.y q.y) + q.z q.z -- the vertices gsr_tsdf_mesh_emit wrote for a contracted volume, taken to world
 * space (rows must have |q| < 2; every vertex of such a mesh has |q| < q_max).  0 <= n < 2^31; n == 0 is a successful
 * no-op (xyz may be NULL).  Asynchronous on `stream`, allocates nothing, reads nothing back. */
int gsr_tsdf_uncontract_points(float* xyz, int64_t n, const GsrTsdfContraction* contraction, void* stream);

/* ---- Depth-normal consistency loss, ABI v28 (csrc/normal_consistency.hip; normal_consistency.py)
 * The normal-consistency term of 2DGS on the maps of a rendered frame: depth [H,W] = sum w z, alpha [H,W] = sum w,
 * normal [3,H,W] = sum w n (un-normalised), device float32, contiguous.  Pixel convention of GsrTsdfView:
 * fx = W / (2 tanfovx), fy = H / (2 tanfovy), each rounded once on the host, cx = (W - 1) / 2, cy = (H - 1) / 2; view
 * space +z forward, x right, y down.
 *     covered(q) = alpha(q) >= alpha_min       d(q) = depth(q) / alpha(q)       P(q) = (d (x - cx) / fx, d (y - cy) / fy, d)
 *     tx = P(x+1,y) - P(x-1,y)     ty = P(x,y+1) - P(x,y-1)     c = ty x tx     s = |c|^2
 *     valid(q): 1 <= x <= W-2, 1 <= y <= H-2, q and its four axis neighbours covered, s finite and s > 1e-20
 *     n_d(q) = c / sqrt(s)  (faces the camera: a fronto-parallel plane gives (0,0,-1))
 *     e(q) = alpha(q) - normal(q) . n_d(q)     loss = sum_valid e(q) / (H W)
 * record (16-byte aligned, 4 floats) = { loss, n_valid as uint32 bits, 0, 0 }: written, not accumulated.
 * dL_ddepth [H,W], dL_dalpha [H,W], dL_dnormal [3,H,W]: all three or none (NULL); the exact derivatives of `loss` for a
 * unit upstream gradient, validity a decision without gradient; written in full (zeros where nothing arrives).
 * depth_normal [3,H,W] or NULL: n_d on valid pixels, 0 elsewhere.  The loss and depth_normal are the same bits with and
 * without the gradients, and every output is the same bits from run to run (a gather, no atomics; the loss is summed
 * per workgroup and then over workgroups in a fixed order).  workspace: gsr_normal_consistency_workspace_bytes(H, W)
 * bytes, 8-byte aligned (0: a shape the call refuses).
 * Every argument is checked before any HIP call: GSR_E_BADARG for H, W < 1 (or H W > 2^28), a tan that is not positive,
 * alpha_min outside (0, 1], a NULL input / record / workspace, a partial set of gradient pointers; GSR_E_ALIGN.
 * Asynchronous on `stream`, allocates nothing, reads nothing back.  An image without interior (H < 3 or W < 3) or
 * without a valid pixel gives loss = 0, n_valid = 0 and all-zero outputs. */
size_t gsr_normal_consistency_workspace_bytes(int32_t H, int32_t W);
int gsr_normal_consistency_fwd_bwd(const float* depth, const float* alpha, const float* normal, int32_t H, int32_t W,
                                   float tanfovx, float tanfovy, float alpha_min, float* record, float* dL_ddepth,
                                   float* dL_dalpha, float* dL_dnormal, float* depth_normal, void* workspace,
                                   void* stream);

/* ---- Mesh cleaning: connected components of an indexed triangle mesh and compaction, ABI v31 (csrc/mesh.hip; mesh.py;
 * DESIGN.md §7.18).  faces [F,3] int32, vertices / colors [V,3] float32, device, contiguous; 1 <= V, F < 2^31.
 * Every call checks its arguments before any HIP call (GSR_E_BADARG: a NULL pointer that is not marked optional, a size
 * outside its range; GSR_E_ALIGN: int32 / float arrays 4-byte, int64 / uint64 arrays 8-byte), is asynchronous on
 * `stream`, allocates nothing and reads nothing back; an empty mesh needs no call.
 * status: device int32 [1], zeroed by the caller.  A face with an index outside 0..V-1 is never used as an index: the
 * kernel that meets it skips it and stores 1 there; the caller reads the word back with its sizes and refuses the mesh.
 * stats: NULL, or device uint64 [2], zeroed by the caller: the hooks add their find steps to [0] and their retries (an
 * atomicMin that found its node linked already) to [1].  The labelling is the same with and without.
 *
 * Labelling is a lock-free union-find over n nodes, parent int32 [n]; parent[x] <= x at every instant, every loop step
 * strictly lowers an index, and no lane waits for another.  The call sequence on one stream:
 *   vertex connectivity (nodes = vertices, n = V; faces that share a vertex are connected):
 *     gsr_mesh_cc_init(V, parent, first); gsr_mesh_cc_hook_faces; gsr_mesh_cc_flatten(V, parent);
 *     gsr_mesh_cc_mark(faces, F, V, parent, first, face_root, mark)
 *   edge connectivity (nodes = faces, n = F; faces that share an undirected edge are connected):
 *     gsr_mesh_cc_init(F, parent, NULL); gsr_mesh_edge_keys; the caller sorts the keys; gsr_mesh_cc_hook_runs;
 *     gsr_mesh_cc_flatten(F, parent); gsr_mesh_cc_mark(NULL, F, 0, parent, NULL, NULL, mark)  (face_root is parent)
 *   then: ids = exclusive scan of mark (int64), K = its total; gsr_mesh_cc_label.
 * After flatten parent[x] is the smallest node of x's component, whatever order the atomics landed in: the same bits
 * from run to run, as is every output below. */
/* parent[i] = i; first (NULL, or int32 [n]): first[i] = INT32_MAX. */
int gsr_mesh_cc_init(int64_t n, int32_t* parent, int32_t* first, void* stream);
/* Each face (v0, v1, v2) unites (v0, v1) and (v0, v2) in parent [V]: find both roots, atomicMin(parent[larger], smaller),
 * and from the value returned again if it is not `larger`. */
int gsr_mesh_cc_hook_faces(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int32_t* status, uint64_t* stats,
                           void* stream);
/* keys int64 [3 F], owner int32 [3 F]: slot 3 f + e holds (min(a, b) << 32) | max(a, b) for the edge (a, b) =
 * (v_e, v_(e+1) mod 3) of face f, and f.  A self-pair (a, a) is an ordinary key.  The three keys of a refused face are
 * -(3 f + e) - 1: equal to no other. */
int gsr_mesh_edge_keys(const int32_t* faces, int64_t F, int64_t V, int64_t* keys, int32_t* owner, int32_t* status,
                       void* stream);
/* keys_sorted int64 [m]: the keys in ascending order; order int64 [m]: the slot each came from (a sort's indices);
 * owner int32 [m] as written above (unsorted); m = 3 F, n = F.  For every i with keys_sorted[i] == keys_sorted[i-1]:
 * unite(owner[order[i-1]], owner[order[i]]) in parent [n].  An order or owner entry out of range is skipped and sets
 * status. */
int gsr_mesh_cc_hook_runs(const int64_t* keys_sorted, const int64_t* order, const int32_t* owner, int64_t m, int64_t n,
                          int32_t* parent, int32_t* status, uint64_t* stats, void* stream);
/* A launch of its own behind the hooks: parent[i] = root of i. */
int gsr_mesh_cc_flatten(int64_t n, int32_t* parent, void* stream);
/* mark uint8 [F]: 1 where face f is the smallest face of its component, else 0.  faces, first and face_root all NULL
 * (parent is [F], nodes are faces): mark[f] = parent[f] == f.  All three given (parent and first are [V], first as
 * gsr_mesh_cc_init left it): two launches, first[parent[v0]] = min over the faces f (one atomicMin per wave and root),
 * then face_root[f] = first[parent[v0]], int32 [F], and mark[f] = face_root[f] == f.  A refused face stands alone. */
int gsr_mesh_cc_mark(const int32_t* faces, int64_t F, int64_t V, const int32_t* parent, int32_t* first,
                     int32_t* face_root, uint8_t* mark, void* stream);
/* face_root int32 [F]: the smallest face of each face's component (parent itself with face nodes); ids int64 [F]: the
 * exclusive scan of mark; K = the number of marks, 1 <= K <= F.  face_component[f] = ids[face_root[f]], int32 [F]:
 * components are numbered 0..K-1 in the order of their smallest face.  component_faces int64 [K], zeroed by the caller:
 * the number of faces of each component, accumulated with integer atomics (one per wave and component).  A face whose
 * root or id is out of range is not written or counted. */
int gsr_mesh_cc_label(const int32_t* face_root, const int64_t* ids, int64_t F, int64_t K, int32_t* face_component,
                      int64_t* component_faces, void* stream);
/* Compaction, first half.  keep uint8 [F]; vertex_mark uint8 [V], zeroed by the caller: plain stores of 1 at the three
 * vertices of every face with keep[f] != 0. */
int gsr_mesh_mark_vertices(const int32_t* faces, const uint8_t* keep, int64_t F, int64_t V, uint8_t* vertex_mark,
                           int32_t* status, void* stream);
/* Second half, one launch.  vert_offs int64 [V] / face_offs int64 [F]: the exclusive scans of vertex_mark / keep != 0;
 * Vk, Fk: their totals, 1 <= Vk <= V, 1 <= Fk <= F (an empty result needs no call).  Marked vertex i: row i of vertices
 * (and of colors, given together with out_colors or both NULL) is copied to row vert_offs[i] of out_vertices [Vk,3]
 * (out_colors).  Kept face f: out_faces [Fk,3] row face_offs[f] = vert_offs of its three indices.  Vertices and faces
 * keep their order, the rows are bit-copies, and nothing at or beyond row Vk / Fk is written whatever the scans hold. */
int gsr_mesh_compact(const float* vertices, const float* colors, const int32_t* faces, const uint8_t* keep,
                     const uint8_t* vertex_mark, const int64_t* vert_offs, const int64_t* face_offs, int64_t V, int64_t F,
                     int64_t Vk, int64_t Fk, float* out_vertices, float* out_colors, int32_t* out_faces, int32_t* status,
                     void* stream);

/* ---- Cross-set nearest point, ABI v32 (csrc/nearest.hip on the index of csrc/knn.hip; geometry_eval.py).
 * ref [R,3], query [Q,3] float32, device, contiguous, 4-byte aligned; 0 <= R, Q <= GSR_NN_MAX_POINTS = 2^31 - 256 (a box
 * of 128 points and a workgroup of 256 queries past the last one still index in 32 bits; more is GSR_E_BADARG).  For every query point the
 * minimum over the reference of d2 = ((dx dx + dy dy) + dz dz), dx = q.x - r.x, every operation rounded to float32 on its
 * own (no fused multiply-add), and the smallest reference index that attains it: exact, the bits of a float32 brute force.
 * Coordinates must be finite: NaN / Inf give an unspecified value, never an access out of range.
 * Every call checks its arguments before any HIP call (GSR_E_BADARG: a NULL pointer, a negative count; GSR_E_CAPACITY: a
 * buffer shorter than the matching *_bytes; GSR_E_ALIGN: index / workspace 256-byte, the arrays 4-byte), is asynchronous
 * on `stream`, allocates nothing and reads nothing back.
 * index: caller-owned device memory of gsr_nn_index_bytes(R) bytes, written by gsr_nn_build and read by any number of
 * gsr_nn_query calls: the encoded bounding box, the sorted 30-bit Morton keys, the sorted points as (x, y, z, original
 * index), the bounds of every box of 128 sorted points and of every super-box of 64 boxes -- and the scratch of the build,
 * so that a build needs no second buffer.  Nothing in it is read before the build wrote it.  R = 0 needs no build (the
 * call is a success that writes nothing) and no index. */
#define GSR_NN_MAX_POINTS 2147483392
size_t gsr_nn_index_bytes(int32_t R);
int gsr_nn_build(const float* ref, int32_t R, void* index, size_t index_bytes, void* stream);
/* dist2 float32 [Q], nearest int32 [Q]; workspace: gsr_nn_query_workspace_bytes(Q) bytes (the queries' Morton keys, their
 * sort).  R = 0: dist2 = +inf, nearest = -1 (index and workspace may be NULL).  Q = 0: success, nothing is written. */
size_t gsr_nn_query_workspace_bytes(int32_t Q);
int gsr_nn_query(const void* index, size_t index_bytes, int32_t R, const float* query, int32_t Q, float* dist2,
                 int32_t* nearest, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Point-to-point ICP between two nearest-point queries, ABI v43 (csrc/icp.hip, csrc/icp_math.h; geometry_eval.py;
 * DESIGN.md §7.30).  Device arrays are float32 / int32, contiguous, 4-byte aligned; `matrix` and `pivots` are HOST arrays
 * of finite doubles, read before the call returns.  0 <= Q, R <= GSR_NN_MAX_POINTS.  Every call checks its arguments
 * before any HIP call, is asynchronous on `stream`, allocates nothing and reads nothing back.  No atomics: the same
 * arguments give the same bits whatever the workspace held.
 * gsr_icp_transform: matrix = the upper 3x4 of a similarity, row-major (s R | t).  out[i] = (float)(((m0 x + m1 y) + m2 z)
 * + m3) per axis, in float64, every operation rounded on its own (no fused multiply-add), one rounding to float32.
 * out may be points.  Q = 0: success, nothing is written. */
#define GSR_ICP_WORDS 18
#define GSR_ICP_BLOCK 256
#define GSR_ICP_MAX_BLOCKS 1024
int gsr_icp_transform(const float* points, int32_t Q, const double* matrix, float* out, void* stream);
/* gsr_icp_accumulate: q [Q,3] the transformed source; dist2 [Q], nearest [Q] as gsr_nn_query wrote them against target
 * [R,3]; pivots = c_q (3), c_r (3).  A pair i is accepted when dist2[i] <= thr2 (thr2 >= 0, +inf allowed; a NaN dist2 is
 * not accepted) and 0 <= nearest[i] < R (-1, the empty target, never is).  With a = (double)q_i - c_q and b =
 * (double)target[nearest[i]] - c_r, out (device, 8-byte aligned, GSR_ICP_WORDS 8-byte words) receives the int64 count of
 * accepted pairs and 17 doubles: sum a (3), sum b (3), sum a_i b_j row-major (9), sum ((a0 a0 + a1 a1) + a2 a2), sum
 * (double)dist2.  Accumulation is float64 in a fixed order (the header comment of csrc/icp.hip): min(ceil(Q / 256),
 * GSR_ICP_MAX_BLOCKS) workgroups leave one partial each in `workspace` (gsr_icp_workspace_bytes(Q) bytes, 256-byte
 * aligned), and a second launch of one workgroup adds the partials.  No pair accepted: count 0 and sums +0.0.  Q = 0:
 * out is still written (zeros); the arrays and the workspace may be NULL. */
size_t gsr_icp_workspace_bytes(int32_t Q);
int gsr_icp_accumulate(const float* q, const float* dist2, const int32_t* nearest, int32_t Q, const float* target,
                       int32_t R, float thr2, const double* pivots, void* workspace, size_t workspace_bytes, void* out,
                       void* stream);

/* ---- Depth-prior loss of a rendered inverse-depth map, ABI v44 (csrc/depth_prior.hip, csrc/depth_prior_math.h;
 * depth_prior.py).  invdepth (x), prior (y) and the optional weight (w; NULL: 1 everywhere) are device
 * float32 [H,W], contiguous, 4-byte aligned, 1 <= H W <= 2^28.  A pixel is valid when w > 0 and w, x, y are finite; an
 * invalid pixel enters no sum and gets gradient +0.  mode:
 *   GSR_DEPTH_PRIOR_L1          sum w |x - (scale y + offset)| / (H W), upstream 3DGS's term; scale, offset finite
 *   GSR_DEPTH_PRIOR_ALIGNED_L1  sum w |x - (s y + t)| / sum w under the weighted least-squares fit s, t of x on y, a constant
 *   GSR_DEPTH_PRIOR_PEARSON     1 - r, r the weighted Pearson correlation of x and y
 * (scale and offset are ignored by the two fitted modes).  A fitted mode is degenerate below 2 valid pixels or when the
 * weighted variance of x or of y is not above 2^-40 of its mean square: loss 0, gradient 0, s = 1, t = 0, r = 0.
 * record (device, 8-byte aligned, 8 doubles) receives (loss, valid pixels, sum w, s, t, r, degenerate 0 / 1, 0); in the l1
 * mode s, t are scale, offset and r is 0.  grad (device [H,W] float32, or NULL: not written) receives dL/dx, computed in
 * float64 and rounded once.  Sums are float64 in a fixed order (the header comment of csrc/depth_prior.hip): min(ceil(H W /
 * GSR_DEPTH_PRIOR_BLOCK), GSR_DEPTH_PRIOR_MAX_BLOCKS) workgroups leave one partial each in `workspace`
 * (gsr_depth_prior_workspace_bytes(H, W) bytes, 256-byte aligned) and a launch of one workgroup adds them; no atomics: the
 * same arguments give the same bits whatever the workspace held.  After a fitted mode the workspace's 8-byte words
 * GSR_DEPTH_PRIOR_FIT_COUNT_WORD .. + GSR_DEPTH_PRIOR_SUM_WORDS - 1 hold the int64 count of valid pixels and the six sums
 * of w, wx, wy, wxx, wxy, wyy.  2 (l1), 4 (aligned_l1) or 3 (pearson) launches on `stream`; every argument is checked
 * before any HIP call; nothing is allocated or read back. */
#define GSR_DEPTH_PRIOR_L1 0
#define GSR_DEPTH_PRIOR_ALIGNED_L1 1
#define GSR_DEPTH_PRIOR_PEARSON 2
#define GSR_DEPTH_PRIOR_BLOCK 256
#define GSR_DEPTH_PRIOR_MAX_BLOCKS 1024
#define GSR_DEPTH_PRIOR_SUM_WORDS 7
#define GSR_DEPTH_PRIOR_RECORD_WORDS 8
#define GSR_DEPTH_PRIOR_FIT_COUNT_WORD 16
size_t gsr_depth_prior_workspace_bytes(int32_t H, int32_t W);
int gsr_depth_prior_fwd_bwd(const float* invdepth, const float* prior, const float* weight, int32_t H, int32_t W,
                            int32_t mode, double scale, double offset, double* record, float* grad, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- Training under a per-image mask, ABI v45 (csrc/masked_loss.hip; masked_loss.py).
 * gsr_masked_l1_dssim_loss_fwd_bwd: the training loss of gsr_l1_dssim_loss_fwd_bwd (GSR_DSSIM_ONE_MINUS_MEAN) under a mask.
 * x, gt (device float32 [C,H,W]) and mask (device float32 [H,W], values in [0, 1]: documented, not checked) are contiguous
 * and 4-byte aligned; 1 <= C <= 65535, 1 <= H W <= 2^28, H <= 16 * 65535.  With x' = m x and y' = m gt, float32 products
 * rounded once (+0 where m is 0, whatever the images hold there), and S the SSIM map of x', y' (the window, padding and
 * constants of the unmasked loss):
 *   GSR_MASKED_LOSS_NORM_IMAGE  L1 = sum|x' - y'| / (C H W), Ds = 1 - sum S / (C H W): upstream 3DGS's and gsplat's rule,
 *                               the unmasked loss of the pre-multiplied images
 *   GSR_MASKED_LOSS_NORM_MASK   Z = C sum m; L1 = sum|x' - y'| / Z, Ds = sum_{c,p} m_p (1 - S_cp) / Z; with Z = 0 the loss
 *                               and every gradient are 0 and the record's degenerate word is 1
 * loss = (1 - lambda) L1 + lambda Ds, lambda in [0, 1].  record (device, 8-byte aligned, GSR_MASKED_LOSS_RECORD_WORDS
 * doubles) receives (loss, L1, Ds, Z, sum m (0 in image mode), degenerate 0 / 1, 0, 0).  dL_dx (device [C,H,W] float32, or
 * NULL: the backward launch is left out) receives dL/dx = m dL/dx', +0 where m is 0; gt and mask get no gradient.  sum m is
 * reduced on the device (at most GSR_MASKED_LOSS_MAX_BLOCKS partials) and read from device memory by the later launches.
 * Every sum is one partial per workgroup added by a one-workgroup launch in float64 in a fixed order, no atomics: the same
 * arguments give the same bits whatever `workspace` (gsr_masked_l1_dssim_workspace_bytes(C, H, W) bytes, 256-byte
 * aligned) held.  3 (image) or 5 (mask) launches on `stream`, one fewer without dL_dx; every argument is checked before
 * any HIP call (GSR_E_BADARG: NULL pointer, shape, lambda, unknown normalize; GSR_E_CAPACITY; GSR_E_ALIGN); nothing is
 * allocated or read back. */
#define GSR_MASKED_LOSS_NORM_IMAGE 0
#define GSR_MASKED_LOSS_NORM_MASK 1
#define GSR_MASKED_LOSS_RECORD_WORDS 8
#define GSR_MASKED_LOSS_MAX_BLOCKS 1024
size_t gsr_masked_l1_dssim_workspace_bytes(int32_t C, int32_t H, int32_t W);
int gsr_masked_l1_dssim_loss_fwd_bwd(const float* x, const float* gt, const float* mask, int32_t C, int32_t H, int32_t W,
                                     double lambda_dssim, int32_t normalize, double* record, float* dL_dx, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* gsr_alpha_mask_loss_fwd_bwd: the silhouette term of a rendered alpha map against the mask, both device float32 [H,W],
 * contiguous, 4-byte aligned, 1 <= H W <= 2^28.  mode:
 *   GSR_ALPHA_MASK_L1   mean|a - m|; gradient sign(a - m) / (H W), sign(0) = 0
 *   GSR_ALPHA_MASK_BCE  -mean(m log a^ + (1 - m) log(1 - a^)), a^ = clamp(a, 1e-6f, 1 - 1e-6f) (float32 constants); gradient
 *                       (a^ - m) / (a^ (1 - a^)) / (H W), and 0 where a was clamped
 * evaluated per pixel in float64 and rounded once.  record (device, 8-byte aligned, 4 doubles) receives (loss, H W, mode, 0);
 * dL_dalpha (device [H,W] float32, or NULL: not written) the gradient; the mask gets none.  One elementwise launch of at most
 * GSR_MASKED_LOSS_MAX_BLOCKS workgroups and the same fixed-order float64 finish; workspace:
 * gsr_alpha_mask_workspace_bytes(H, W) bytes, 8-byte aligned.  Checked before any HIP call as above. */
#define GSR_ALPHA_MASK_L1 0
#define GSR_ALPHA_MASK_BCE 1
size_t gsr_alpha_mask_workspace_bytes(int32_t H, int32_t W);
int gsr_alpha_mask_loss_fwd_bwd(const float* alpha, const float* mask, int32_t H, int32_t W, int32_t mode, double* record,
                                float* dL_dalpha, void* workspace, size_t workspace_bytes, void* stream);

/* ---- k-means vector quantisation of attribute rows, ABI v46 (csrc/kmeans.hip, csrc/kmeans_math.h; compress.py;
 * DESIGN.md §7.33).  All arrays are device memory, contiguous, row-major; 1 <= D <= GSR_KMEANS_MAX_D,
 * 1 <= K <= GSR_KMEANS_MAX_K, 1 <= N <= 2^31 - 1.  The rule (kmeans_math.h), for a point x[D] and a code c[D]:
 *   dot = fmaf(x[D-1], c[D-1], ... fmaf(x[0], c[0], 0.0f)), cnorm = the same chain of c with itself,
 *   score = fmaf(-2.0f, dot, cnorm); index = the code of the smallest score, the smallest index among equal scores;
 *   dist2 = max(0, xnorm + score) with xnorm the chain of x with itself (a diagnostic).
 * Inputs are expected finite (compress.py refuses others); nothing here checks values.
 * gsr_kmeans_code_norms: cnorm[K] of codebook [K,D]; one launch.
 * gsr_kmeans_assign: index_out int32 [N] and, unless NULL, dist2_out float [N], of x [N,D] against codebook [K,D] with the
 *   cnorm that gsr_kmeans_code_norms wrote; one launch, the dot products on v_mfma_f32_32x32x2_f32, whose accumulator is
 *   that fmaf chain bit for bit.  No atomics; the same bits from run to run and whatever the order of the rows of x.
 * gsr_kmeans_assign_valu: the same rule and the same bits on the vector ALU, D <= 4 only (GSR_E_BADARG above): the
 *   cross-check of the matrix-core path.
 * gsr_kmeans_update: the new centres.  keys_sorted int64 [N] and order int64 [N] are the caller's stable ascending sort of
 *   the indices (values and permutation), head uint8 [N] what gsr_simplify_run_heads gives for keys_sorted.  For every code
 *   c with rows: codebook[c] = (float)(sum_i w_i x_i / sum_i w_i), float64 sums over its rows in ascending row index from
 *   the first row on, the products exact, one rounding to float32; weights float [N] or NULL (w = 1).  A code without a row
 *   or with sum w = 0 keeps its centre and adds 1 to counters[0]; counters[1] becomes 1 if an index lies outside 0..K-1
 *   or a slot of order outside 0..N-1 (such rows are skipped).  counters (int32 [2]) is only ever added to / or-ed: the
 *   caller zeroes it once.  runs: int32 [2 K] workspace.  One memset and two launches.
 * Every call checks its arguments before any HIP call (GSR_E_BADARG: NULL pointer, a size outside its range; GSR_E_ALIGN:
 * float / int32 arrays 4-byte, int64 arrays 8-byte), is asynchronous on `stream`, allocates nothing and reads nothing back. */
#define GSR_KMEANS_MAX_D 64
#define GSR_KMEANS_MAX_K 65536
int gsr_kmeans_code_norms(const float* codebook, int32_t K, int32_t D, float* cnorm, void* stream);
int gsr_kmeans_assign(const float* x, int64_t N, int32_t D, const float* codebook, const float* cnorm, int32_t K,
                      int32_t* index_out, float* dist2_out, void* stream);
int gsr_kmeans_assign_valu(const float* x, int64_t N, int32_t D, const float* codebook, const float* cnorm, int32_t K,
                           int32_t* index_out, float* dist2_out, void* stream);
int gsr_kmeans_update(const float* x, const float* weights, int64_t N, int32_t D, const int64_t* keys_sorted,
                      const int64_t* order, const uint8_t* head, int32_t K, int32_t* runs, float* codebook,
                      int32_t* counters, void* stream);

/* ---- Multi-view geometric consistency of depth maps and back-projection, ABI v34 (csrc/mvs.hip; mvs.py).
 * The check of MVSNet's / COLMAP's fusion: a reference pixel goes into a source view at its depth, the source's depth is
 * read there (bilinear over four pixels that all hold depth), the result comes back, and the pixel is consistent with
 * that source when it lands within pix_thresh pixels of where it started and within depth_thresh (relative) of the depth
 * it started with.  Pixel convention of GsrTsdfView: cx = (W - 1) / 2, cy = (H - 1) / 2; depth 0 = none.  The float32
 * operation order is the header comment of csrc/mvs.hip (-ffp-contract=off).
 * One row of the device-resident source table, 8-byte aligned, 152 bytes: the source's depth [height,width] (device,
 * float32, contiguous, 4-byte aligned), its intrinsics, and ref_to_src = inv(V_ref) V_src, src_to_ref = inv(V_src) V_ref in
 * the row-vector convention (M[4 * row + col]), formed in float64 from the float32 view matrices and rounded once. */
#define GSR_MVS_MAX_SOURCES 64
typedef struct GsrMvsSource {
  const float* depth;
  int32_t width, height;
  float fx, fy;
  float ref_to_src[16];
  float src_to_ref[16];
} GsrMvsSource;
/* depth [H,W] -> count uint8 [H,W]: the number of sources (table order, 0 <= S <= 64) the pixel is consistent with;
 * fused float32 [H,W]: (d + sum of the consistent round-trip depths) / (count + 1) where count >= min_views, else 0.  A
 * pixel without depth gives 0, 0; every pixel of both outputs is written; S = 0 is valid (count 0; fused = depth when
 * min_views = 0, else 0).  One launch with the loop over the sources inside; sums in table order in registers: the same
 * bits from run to run.  Checked before any HIP call: GSR_E_BADARG for a NULL pointer, H or W < 1 or H W > 2^28, S outside
 * 0..64, a NULL table with S > 0, fx / fy / pix_thresh / depth_thresh not positive and finite, min_views < 0;
 * GSR_E_ALIGN for depth / fused (4 bytes) and the table (8).  Asynchronous, allocates nothing, reads nothing back.  The
 * table's rows are device memory and are not checked: width / height must describe the row's depth array. */
int gsr_mvs_consistency(const float* depth, int32_t H, int32_t W, float fx, float fy, const GsrMvsSource* sources, int32_t S,
                        float pix_thresh, float depth_thresh, int32_t min_views, uint8_t* count, float* fused, void* stream);
/* depth [H,W] -> xyz [H W,3] (device): pixel (px, py) with depth d > 0 is (((px - cx) d) / fx, ((py - cy) d) / fy, d)
 * through cam_to_world (HOST, 16 floats, row-vector convention: the float64 inverse of the view matrix rounded once; it
 * is read during the call), x = ((xr M[0] + yr M[4]) + zr M[8]) + M[12] and likewise y, z; a pixel without depth gives a
 * zero row.  H W = 0 is a successful no-op (after the scalar checks).  GSR_E_BADARG: negative H / W, H W > 2^28, fx / fy
 * not positive and finite, a NULL pointer; GSR_E_ALIGN: 4 bytes. */
int gsr_depth_backproject(const float* depth, int32_t H, int32_t W, float fx, float fy, const float* cam_to_world,
                          float* xyz, void* stream);

/* ---- Multi-view geometric consistency loss, value and gradients, ABI v35 (csrc/mvs_loss.hip; mvs.multi_view_geo_loss;
 * DESIGN.md §7.22).  The multi-view geometric term of PGSR on one (reference, source) pair: per reference pixel with
 * depth, the round trip of gsr_mvs_consistency (the same code, the same bits) up to (ub, vb, zb); phi = sqrt(du^2 + dv^2).
 * The pixel is valid when every gate of that check passes (zs > 0.2, the 2 x 2 footprint inside the source, four taps > 0,
 * zb > 0.2), phi < pix_max, and -- only with depth_thresh > 0 -- |zb - d| < depth_thresh d.  With w = exp(-phi) held
 * constant: raw = sum_valid w phi, n = the number of valid pixels, loss = raw / max(n, 1).
 * source: ONE GsrMvsSource row in device memory.  record (device, float[4]): (loss, n as uint32 bits, raw, 0), written.
 * grad_ref [H,W], may be NULL: d raw / d ref_depth, every pixel written (zero where not valid).  grad_src [src_H,src_W],
 * may be NULL: d raw / d source depth, zeroed on the stream by this call, then accumulated with float atomic adds.  Both
 * are UNIT gradients of raw: the caller applies upstream / max(n, 1).  src_H, src_W size the zeroing of grad_src and must
 * equal the row's height and width (the row lives on the device and is not read here; the kernel leaves grad_src zero
 * when they differ); they are ignored when grad_src is NULL.  record and grad_ref are the same bits from run to run;
 * grad_src is NOT (the order of the atomic additions varies).  workspace: gsr_mvs_geo_loss_workspace_bytes(H, W) bytes,
 * 8-byte aligned (per-workgroup partial sums); the size is 0 for a shape the call refuses.
 * Checked before any HIP call: GSR_E_BADARG for NULL ref_depth / source / record / workspace, H or W < 1, H W > 2^28 or a
 * launch of 2^32 work-items or more, fx / fy / pix_max not positive and finite, a NaN depth_thresh (<= 0: the depth test
 * is off), a bad src_H / src_W with grad_src; GSR_E_ALIGN for the float arrays (4 bytes), the row and the workspace (8).
 * Asynchronous, allocates nothing, reads nothing back. */
size_t gsr_mvs_geo_loss_workspace_bytes(int32_t H, int32_t W);
int gsr_mvs_geo_loss_fwd_bwd(const float* ref_depth, int32_t H, int32_t W, float fx, float fy, const GsrMvsSource* source,
                             float pix_max, float depth_thresh, float* record, float* grad_ref, float* grad_src,
                             int32_t src_H, int32_t src_W, void* workspace, void* stream);

/* ---- Multi-view photometric (NCC) loss, value and gradients, ABI v36 (csrc/mvs_ncc.hip; mvs.multi_view_ncc_loss;
 * DESIGN.md §7.23).  The photometric half of PGSR's multi-view term on one (reference, source) pair: per reference pixel
 * p with depth d > 0 and view-space normal N (camera-facing, any magnitude), the plane m = N / (d (N . r(p))) carries the
 * (2 patch_radius + 1)^2 patch of ref_gray about p into src_gray (Y = r(q) A[0:3,0:3] + (m . r(q)) A[3,0:3], A =
 * ref_to_src), where it is read bilinearly; ncc = clamp(1 - cross^2 / (var_r var_s + 1e-8), 0, 2) over the patch's sums.
 * The pixel counts when its whole patch lies in the reference, |N|^2 > 1e-12, |N . r(p)| >= min_cos |N| |r(p)|, the round
 * trip of gsr_mvs_consistency passes every gate with phi < pix_max, every tap has m . r(q) > 0, Y_z > 0 and its 2 x 2
 * footprint inside the source, and ncc < ncc_max.  With w = exp(-phi) held constant: raw = sum_counted w ncc, n = the
 * number of counted pixels, loss = raw / max(n, 1).  The float32 order of operations is the kernel file's header comment.
 * ref_depth [H,W], ref_normal [3,H,W], ref_gray [H,W]; source: ONE GsrMvsSource row in device memory (its depth enters
 * the weight and the gates only); src_gray: [source height, source width].  pixels: NULL (every pixel, n_pixels ignored
 * beyond its range check) or n_pixels flat indices py W + px, one lane each; an index outside [0, H W) is skipped;
 * duplicate indices are the caller's error.  record (device, float[4]): (loss, n as uint32 bits, raw, 0), written.
 * grad_depth [H,W] and grad_normal [3,H,W], each may be NULL: d raw / d ref_depth and d raw / d ref_normal.  Without a
 * list every pixel is written (zero where not counted); with one both maps are zeroed on the stream by this call and the
 * listed pixels written.  No atomics: record and both gradients are the same bits from run to run.  workspace:
 * gsr_mvs_ncc_loss_workspace_bytes(H, W, n_pixels) bytes (n_pixels = 0 for a call without a list), 8-byte aligned; the
 * size is 0 for a shape the call refuses.
 * Checked before any HIP call: GSR_E_BADARG for a NULL required pointer, H or W < 1, H W > 2^28 or a launch of 2^32
 * work-items, n_pixels < 0 or > H W, patch_radius outside 1..4, non-positive or non-finite fx / fy / pix_max, ncc_max
 * outside (0, 2], min_cos outside [0, 1); GSR_E_ALIGN for the float and index arrays (4 bytes), the row and the workspace
 * (8).  Asynchronous, allocates nothing, reads nothing back. */
size_t gsr_mvs_ncc_loss_workspace_bytes(int32_t H, int32_t W, int32_t n_pixels);
int gsr_mvs_ncc_loss_fwd_bwd(const float* ref_depth, const float* ref_normal, const float* ref_gray, int32_t H, int32_t W,
                             float fx, float fy, const GsrMvsSource* source, const float* src_gray, const int32_t* pixels,
                             int32_t n_pixels, int32_t patch_radius, float pix_max, float ncc_max, float min_cos,
                             float* record, float* grad_depth, float* grad_normal, void* workspace, void* stream);

/* ---- Per-Gaussian planes and PGSR's unbiased plane depth, ABI v37 (csrc/planes.hip, csrc/plane_depth.hip;
 * features.gaussian_planes, surface.plane_depth).
 * gsr_gaussian_planes_fwd: planes [P,4] from scales [P,3] (only their order is read), rotations [P,4] (raw quaternions
 * r, x, y, z) and means3D [P,3], all device.  viewmatrix (16 floats, row-vector convention, its upper-left 3 x 3 is read)
 * and campos (3 floats) are HOST memory, read during the call: they travel as kernel arguments.  Per row q = rot /
 * max(|rot|, 1e-12), R the rotation matrix of q, axis the index of the smallest scale (the smallest index among equals),
 * n_w = R[:, axis] times -1 when n_w . (campos - mean) < 0 (exactly 0 keeps +1); planes = (n_w @ viewmatrix[:3,:3],
 * n_w . (campos - mean)): the view-space unit normal and the distance of the camera centre from the Gaussian's plane,
 * >= 0.  gsr_gaussian_planes_bwd: from dL_dplanes [P,4] it writes dL_drotations [P,4] (through the matrix column and the
 * normalisation) and dL_dmeans3D [P,3] = -dL/dd n_w; axis and sign are decisions and carry no gradient.  Every row of
 * every output is written.  One launch each, no atomics: the same bits from run to run.  Intermediates are doubles; each
 * output is rounded to float32 once.
 * P = 0 is a successful no-op (after the checks of P, viewmatrix and campos).  Checked before any HIP call: GSR_E_BADARG
 * for P < 0, a NULL pointer, a viewmatrix[:3,:3] or campos that is not finite; GSR_E_ALIGN: rotations, planes, dL_dplanes
 * and dL_drotations 16 bytes, the others 4.  Asynchronous, allocates nothing, reads nothing back. */
int gsr_gaussian_planes_fwd(const float* scales, const float* rotations, const float* means3D, int32_t P,
                            const float* viewmatrix, const float* campos, float* planes, void* stream);
int gsr_gaussian_planes_bwd(const float* scales, const float* rotations, const float* means3D, int32_t P,
                            const float* viewmatrix, const float* campos, const float* dL_dplanes, float* dL_drotations,
                            float* dL_dmeans3D, void* stream);

/* gsr_plane_depth_fwd: normal [3,H,W] = sum w n (un-normalised), distance [H,W] = sum w d, alpha [H,W] = sum w, device.
 * Pixel convention of GsrTsdfView and gsr_normal_consistency_fwd_bwd: fx = W / (2 tanfovx) and fy = H / (2 tanfovy),
 * each rounded to float32 once on the host, cx = (W - 1) / 2, cy = (H - 1) / 2, r = ((x - cx) / fx, (y - cy) / fy, 1).
 * c = -(N . r); a pixel is valid when alpha >= alpha_min, D > 0, c > 0, c >= min_cos |N| |r|, every input is finite
 * and every result is a finite float32.  z [H,W] = D / c on valid pixels, 0 elsewhere.  dz_ddistance [H,W] = 1 / c and
 * dz_dnormal [3,H,W] = (D / c^2) r, zeros on pixels that are not valid: both NULL (value only; z has the same bits) or
 * both set.  alpha decides validity only.  gsr_plane_depth_bwd: dL_ddistance = dL_dz dz_ddistance and dL_dnormal[a] =
 * dL_dz dz_dnormal[a] per pixel, exactly 0 where the unit gradient is 0.  One launch each, no atomics: the same bits
 * from run to run.
 * Checked before any HIP call: GSR_E_BADARG for H or W < 1, H W > 2^28, tanfovx / tanfovy not positive and finite,
 * alpha_min outside (0, 1], min_cos outside [0, 1), a NULL required pointer, one unit-gradient pointer without the other;
 * GSR_E_ALIGN: 4 bytes.  Asynchronous, allocates nothing, reads nothing back. */
int gsr_plane_depth_fwd(const float* normal, const float* distance, const float* alpha, int32_t H, int32_t W,
                        float tanfovx, float tanfovy, float alpha_min, float min_cos, float* z, float* dz_ddistance,
                        float* dz_dnormal, void* stream);
int gsr_plane_depth_bwd(const float* dL_dz, const float* dz_ddistance, const float* dz_dnormal, int32_t H, int32_t W,
                        float* dL_ddistance, float* dL_dnormal, void* stream);

/* ---- Per-image bilateral grids, ABI v38 (csrc/bilagrid.hip, csrc/bilagrid_math.h; bilagrid.py).
 * The grid of "Bilateral Guided Radiance Field Processing": grid [12,L,Hg,Wg] (device), channel 4 c + k = A[c,k] with c
 * the output colour, k the input colour and k = 3 the offset; 2 <= Wg, Hg <= 64, 2 <= L <= 16.  For pixel (px, py) of
 * the image x [3,H,W]: u = (px + 0.5) / W (Wg - 1), v = (py + 0.5) / H (Hg - 1), gray = 0.299 x0 + 0.587 x1 + 0.114 x2,
 * z = clamp(gray, 0, 1) (L - 1); cell i0 = min(floor(u), Wg - 2), tu = u - i0, likewise v and z; every coefficient by
 * nested lerps a + t (b - a) along x, then y, then z; y[c] = A[c,0] x0 + A[c,1] x1 + A[c,2] x2 + A[c,3], no clamp.
 * Doubles between the float32 loads and the one rounding of each output.  A grid that is constant over a pixel's cell
 * gives that value bit for bit: with the identity grid (A = eye(3,4) everywhere) y = x and dx = g bit for bit on finite
 * input.
 * gsr_bilagrid_slice_fwd: y [3,H,W].  staging: GSR_BILAGRID_STAGE_AUTO (the library's choice: LDS for a grid that
 * fits under an image of at least 262144 pixels), _CACHE (the cells are read through the caches) or _LDS (a workgroup
 * first copies the whole grid into LDS; GSR_E_BADARG for a grid of more than 24576 floats); the bits of y, and of dx
 * below, do not depend on it.
 * gsr_bilagrid_slice_bwd: from g = dL/dy [3,H,W], dx [3,H,W] = dL/dx (may be NULL; grid may then be NULL), with the
 * second path through the luminance: dx[k] = sum_c A[c,k] g[c] + coef_k dz/dgray sum_c g[c] sum_k' dA[c,k']/dz xt[k'],
 * xt = (x0, x1, x2, 1), dz/dgray = L - 1 for 0 < gray < 1 and exactly 0 otherwise (a gray that is not finite included);
 * and dgrid [12,L,Hg,Wg] = dL/dgrid (may be NULL), dgrid[4 c + k, cell] = sum_p w_cell(p) g[c,p] xt[k,p] with the
 * trilinear weight of pixel p on the cell.  Which cells a pixel touches and whether gray is clamped are decisions and
 * carry no gradient.  dgrid is gathered by grid vertex into double partial sums in `workspace`
 * (gsr_bilagrid_workspace_bytes(H, W, Wg, Hg, L) bytes, 8-byte aligned) and added in a fixed order, no atomics: the
 * same bits from run to run; every element is written, zero where no pixel touches it.  Both NULL: a no-op.
 * gsr_bilagrid_tv_fwd_bwd: grids [N,12,L,Hg,Wg], 1 <= N <= 65536; value (device, one float) = (1/N) sum_n sum_{axis in
 * z,y,x} mean((grids[n] shifted by one along the axis - grids[n])^2), the mean over the 12 * (size with that axis
 * reduced by one) differences of one image; dgrids (same shape, may be NULL) = d value / d grids.  Sums in double in a
 * fixed order: the same bits from run to run.  workspace: gsr_bilagrid_workspace_bytes(0, 0, Wg, Hg, L) bytes (H = W = 0
 * names this call's workspace, which does not depend on N), 8-byte aligned.
 * gsr_bilagrid_workspace_bytes is 0 for a shape the calls refuse.
 * Checked before any HIP call: GSR_E_BADARG for a NULL required pointer, H or W < 1, H W > 2^28, a grid size outside its
 * range, N outside its range, an unknown staging; GSR_E_ALIGN for the float arrays (4 bytes) and the workspace (8).
 * Asynchronous, allocates nothing, reads nothing back. */
enum { GSR_BILAGRID_STAGE_AUTO = 0, GSR_BILAGRID_STAGE_CACHE = 1, GSR_BILAGRID_STAGE_LDS = 2 };
size_t gsr_bilagrid_workspace_bytes(int32_t H, int32_t W, int32_t Wg, int32_t Hg, int32_t L);
int gsr_bilagrid_slice_fwd(const float* x, const float* grid, int32_t H, int32_t W, int32_t Wg, int32_t Hg, int32_t L,
                           int32_t staging, float* y, void* stream);
int gsr_bilagrid_slice_bwd(const float* x, const float* grid, const float* g, int32_t H, int32_t W, int32_t Wg,
                           int32_t Hg, int32_t L, int32_t staging, float* dx, float* dgrid, void* workspace,
                           void* stream);
int gsr_bilagrid_tv_fwd_bwd(const float* grids, int32_t N, int32_t Wg, int32_t Hg, int32_t L, float* value,
                            float* dgrids, void* workspace, void* stream);

/* ---- Mesh simplification by vertex clustering on a uniform grid, ABI v39 (csrc/mesh_simplify.hip,
 * csrc/mesh_simplify_math.h; mesh.simplify_mesh).  The kernels around the caller's sorts and scans;
 * gsr_mesh_mark_vertices and gsr_mesh_compact (above) mark the referenced vertices in front and compact behind.
 * vertices / colors [V,3] float32, faces [F,3] int32, device, contiguous; 1 <= V, F < 2^31; 1 <= K <= V clusters.
 * Every call checks its arguments before any HIP call (GSR_E_BADARG: a NULL pointer that is not marked optional, a size
 * outside its range; GSR_E_ALIGN: int32 / float arrays 4-byte, int64 / double arrays 8-byte), is asynchronous on
 * `stream`, allocates nothing and reads nothing back.  No float atomics: every output is the same bits from run to run.
 * status: device int32 [1], zeroed by the caller; the kernels OR the bits below into it and never use what they refuse
 * as an index.  The caller reads the word back with its sizes and refuses the mesh. */
enum {
  GSR_SIMPLIFY_BAD_INDEX = 1,     /* a face, order, start or cluster index outside its range */
  GSR_SIMPLIFY_NOT_FINITE = 2,    /* a marked vertex has a coordinate that is not finite */
  GSR_SIMPLIFY_OUT_OF_RANGE = 4   /* a marked vertex has a cell index outside 0 .. 2^21 - 1 */
};
/* The default origin, three launches: origin (three doubles on the device) = the per-axis minimum over the finite
 * coordinates of the vertices with vertex_mark[v] != 0, converted to double, minus voxel_size / 2.  lowest int32 [3]:
 * scratch (the minimum as integers that order as the floats do, by integer atomicMin: the same bits whatever order they
 * land in).  No finite marked coordinate: origin is NaN, and gsr_simplify_cell_keys refuses every marked vertex. */
int gsr_simplify_default_origin(const float* vertices, const uint8_t* vertex_mark, int64_t V, double voxel_size,
                                int32_t* lowest, double* origin, void* stream);
/* keys int64 [V].  vertex_mark uint8 [V]; origin: three doubles on the device; h = voxel_size, finite and positive.  A
 * marked vertex gets ix << 42 | iy << 21 | iz with i = floor(((double)x - origin) / h) per axis; an unmarked one, and a
 * marked one that sets GSR_SIMPLIFY_NOT_FINITE or _OUT_OF_RANGE, gets INT64_MAX, which sorts last. */
int gsr_simplify_cell_keys(const float* vertices, const uint8_t* vertex_mark, int64_t V, const double* origin,
                           double voxel_size, int64_t* keys, int32_t* status, void* stream);
/* keys_sorted int64 [V] ascending; head uint8 [V]: 1 where slot i holds a cell (not INT64_MAX) that slot i - 1 does not.
 * The inclusive scan of head, minus one, is the cluster of every slot; its total is K. */
int gsr_simplify_run_heads(const int64_t* keys_sorted, int64_t V, uint8_t* head, void* stream);
/* order int64 [V]: the vertex each sorted slot came from (a stable sort's indices, so a cell's members ascend); ends int64
 * [V]: the inclusive scan of head.  Two launches.  start int32 [K + 1] (scratch): the first slot of every cluster, then
 * the first slot without a cell (or V); cluster_of_vertex int32 [V]: the cluster of every vertex, -1 for one without a
 * cell.  Then one lane per cluster: out_vertices [K,3] (out_colors [K,3], given together with colors or both NULL) = the
 * mean of the members' rows, summed in float64 in slot order from the first member on and rounded to float32 once: a
 * cluster of one member is a bit-copy. */
int gsr_simplify_reduce(const float* vertices, const float* colors, const int64_t* keys_sorted, const int64_t* order,
                        const int64_t* ends, int64_t V, int64_t K, int32_t* start, float* out_vertices, float* out_colors,
                        int32_t* cluster_of_vertex, int32_t* status, void* stream);
/* tri int32 [F,3]: the clusters of each face's corners, in corner order; keep uint8 [F]: 1 unless two of them are equal;
 * key_first int64 [F], key_third int32 [F]: the triple rotated so that its smallest index comes first, as first << 32 |
 * second and third; INT64_MAX and INT32_MAX for a face that is not kept.  A face with a corner outside 0..V-1 or without
 * a cluster sets GSR_SIMPLIFY_BAD_INDEX and is not kept. */
int gsr_simplify_face_keys(const int32_t* faces, const int32_t* cluster_of_vertex, int64_t F, int64_t V, int64_t K,
                           int32_t* tri, uint8_t* keep, int64_t* key_first, int32_t* key_third, int32_t* status,
                           void* stream);
/* The caller sorts the faces stably by key_third and then stably by key_first: first_sorted int64 [F] is key_first in
 * that order, perm int64 [F] the face of every slot; key_third stays unsorted.  A slot whose rotated triple equals its
 * predecessor's clears keep of its face: of the faces with one triple the smallest face index survives. */
int gsr_simplify_face_unique(const int64_t* first_sorted, const int64_t* perm, const int32_t* key_third, int64_t F,
                             uint8_t* keep, int32_t* status, void* stream);
/* cluster_mark uint8 [K] and cluster_offs int64 [K]: what gsr_mesh_mark_vertices wrote for tri and keep, and its
 * exclusive scan.  vertex_cluster int32 [V] = cluster_offs[c] for a vertex whose cluster c is marked, else -1. */
int gsr_simplify_vertex_map(const int32_t* cluster_of_vertex, const uint8_t* cluster_mark, const int64_t* cluster_offs,
                            int64_t V, int64_t K, int32_t* vertex_cluster, void* stream);

/* ---- Culling a mesh by the views that saw it, ABI v41 (csrc/mesh_cull.hip, csrc/mesh_cull_math.h; mesh.vertex_view_counts,
 * mesh.cull_mesh_by_views, mesh.dilate_mask).  Every vertex is projected into every view of a table and
 * two things are counted: the views whose image it lands in, and of those the views in which it lands on the object mask
 * and not behind the view's depth map.  The protocols are rules on these counts (DTU: visible in every view that was
 * counted, with dilated masks; Tanks and Temples: visible somewhere).  Pixel convention of GsrTsdfView / GsrMvsSource:
 * cx = (W - 1) / 2, cy = (H - 1) / 2.  The float32 operation order is csrc/mesh_cull_math.h (-ffp-contract=off), written
 * once for device and host.
 * One row of the device-resident view table, 8-byte aligned, 96 bytes.  The rows are device memory and are not checked:
 * width and height (each 1 .. 2^24, width height at most 2^28) must describe the row's mask and depth arrays -- that is
 * the caller's contract; mesh.vertex_view_counts checks every map against its camera before it builds the table. */
#define GSR_CULL_MAX_VIEWS 65535
typedef struct GsrCullView {
  const uint8_t* mask;     /* device [height,width] or NULL (no mask); non-zero = object */
  const float* depth;      /* device [height,width], 4-byte aligned, or NULL (no occlusion test); 0 = no surface */
  int32_t width, height;
  float fx, fy;
  float world_to_view[16]; /* row-vector convention, M[4 * row + col]: the camera's float32 world_view_transform */
} GsrCullView;
/* vertices [V,3] float32 -> in_view int32 [V], visible int32 [V].  Per vertex (x, y, z) and per row in table order:
 *     (xv, yv, zv) = (x, y, z, 1) through world_to_view, x' = ((x M[0] + y M[4]) + z M[8]) + M[12] and likewise y', z'
 *     next view unless zv > near_plane                                     (a NaN fails)
 *     u = (fx xv) / zv + cx, v = (fy yv) / zv + cy;  ix = floorf(u + 0.5f), iy = floorf(v + 0.5f)
 *     next view unless 0 <= ix <= width - 1 and 0 <= iy <= height - 1       (in float; a NaN fails)
 *     in_view += 1
 *     next view if mask and mask[iy, ix] == 0
 *     next view if depth and not (ds = depth[iy, ix]) > 0 and zv - ds <= depth_tol ds
 *     visible += 1
 * Every row of both outputs is written.  accumulate != 0: the counters start from the arrays' contents instead of 0, so
 * the views can be fed in chunks; counts over chunks equal counts over one table.  One launch, one lane per vertex, the
 * loop over the views inside, integer counters in registers: the same bits from run to run.  V = 0 is a success that
 * writes nothing; S = 0 writes zeros (or, accumulating, leaves the arrays as they are).  Checked before any HIP call:
 * GSR_E_BADARG for V outside 0 .. 2^31 - 1, S outside 0 .. 65535, a NULL table with S > 0, a NULL array with V > 0,
 * near_plane not finite and positive, depth_tol not finite or negative; GSR_E_ALIGN for the arrays (4 bytes) and the table
 * (8).  Asynchronous, allocates nothing, reads nothing back. */
int gsr_cull_view_counts(const float* vertices, int64_t V, const GsrCullView* views, int32_t S, float near_plane,
                         float depth_tol, int32_t accumulate, int32_t* in_view, int32_t* visible, void* stream);
/* faces int32 [F,3], vkeep uint8 [V] -> keep uint8 [F]: 1 where all three corners have vkeep != 0, else 0.  A corner
 * outside 0 .. V - 1 ORs 1 into status (device int32 [1], zeroed by the caller) and keeps nothing, as
 * gsr_mesh_mark_vertices refuses it.  0 <= F, V <= 2^31 - 1; F = 0 is a success that writes nothing. */
int gsr_cull_face_keep(const int32_t* faces, const uint8_t* vkeep, int64_t F, int64_t V, uint8_t* keep, int32_t* status,
                       void* stream);
/* Binary dilation of mask uint8 [H,W] (non-zero = set) by a (2 radius + 1) x (2 radius + 1) square -> out uint8 [H,W] of
 * 0 / 1, as two separable passes: rows into tmp uint8 [H,W] (scratch), then columns into out.  Pixels outside the image
 * count as 0; radius = 0 only normalises the mask.  out may be mask itself; tmp may be neither.  GSR_E_BADARG: a NULL
 * pointer, H or W < 1 or H W > 2^28, radius outside 0 .. 1024, tmp equal to mask or out. */
#define GSR_DILATE_MAX_RADIUS 1024
int gsr_mask_dilate(const uint8_t* mask, int32_t H, int32_t W, int32_t radius, uint8_t* tmp, uint8_t* out, void* stream);

/* ---- Rasterizing a mesh from a camera, ABI v42 (csrc/mesh_raster.hip, csrc/mesh_raster_math.h; mesh.rasterize_mesh,
 * mesh.face_view_counts, mesh.cull_invisible_faces).  A z-buffer of one uint64 per pixel,
 * key = float_bits(z) << 32 | face, all ones where nothing landed, kept by integer atomicMin: the nearest surface wins, the
 * smallest face index at equal depth, and the result is the same bits whatever order the faces arrive in.  The rule of a
 * (face, view) pair -- view transform, near-plane clipping, the snap to 8 sub-pixel bits, int64 edge functions with the
 * top-left rule, perspective-correct depth in float64 -- is stated in csrc/mesh_raster_math.h, one body for device and
 * host, built with -ffp-contract=off.  The camera is a HOST GsrCullView row (mask and depth are not read); its width and
 * height are at most 2^14 each and 2^28 together.
 * Workspaces, the caller's: keys uint64 [height width], 8-byte aligned; queue: gsr_raster_queue_bytes(F) bytes, 8-byte
 * aligned -- a 256-byte head (uint32 words: the queue's length, the pieces dropped, the faces with an index outside
 * 0 .. V-1) and one uint32 slot for each of the 2 F pieces a mesh can have.  gsr_raster_queue_bytes is 0 for an F the
 * calls refuse.  Every call checks its arguments before any HIP call (GSR_E_BADARG, GSR_E_ALIGN, GSR_E_CAPACITY for a
 * short queue), is asynchronous on `stream`, allocates nothing and reads nothing back. */
#define GSR_RASTER_MAX_SIDE 16384
#define GSR_RASTER_LANE_PIXELS 16   /* a piece whose clipped bounding box holds more pixels than this goes to the queue */
#define GSR_RASTER_DRAIN_WAVES 256  /* the fixed grid that drains the queue: 64 workgroups of four waves, one piece per wave */
enum {
  GSR_RASTER_CLEAR = 1,           /* first set every key to all ones and zero the head's dropped / bad-face counts */
  GSR_RASTER_CULL_BACKFACES = 2,  /* drop the pieces that face away (csrc/mesh_raster_math.h, step 4) */
  GSR_RASTER_NO_LOAD_SKIP = 4     /* A/B only: every covered centre issues its atomicMin, no load in front (same keys) */
};
size_t gsr_raster_queue_bytes(int64_t F);
/* vertices float32 [V,3], faces int32 [F,3] (device) into keys.  A face with an index outside 0 .. V-1 is counted in the
 * head and skipped; a piece with a snapped coordinate outside +-2^29 is counted and dropped.  view_scratch: NULL, or
 * float32 [V,3] device scratch -- then the vertices are taken to view space once, in a launch of their own, and the faces
 * gather from it (the same keys; which is faster is recorded in profiles/mesh_raster/NOTES.md).  Without GSR_RASTER_CLEAR
 * the keys are only ever lowered, so several meshes can share one buffer if their face indices are kept apart.
 * 0 <= V, F <= 2^31 - 1; F = 0 still clears. */
int gsr_raster_view(const float* vertices, int64_t V, const int32_t* faces, int64_t F, const GsrCullView* view,
                    float near_plane, int32_t flags, uint64_t* keys, void* queue, size_t queue_bytes, float* view_scratch,
                    void* stream);
/* keys -> depth float32 [H,W] (0 where no surface, the project's convention) and face_id int32 [H,W] (-1 there).  Every
 * pixel of both is written. */
int gsr_raster_resolve(const uint64_t* keys, int32_t H, int32_t W, float* depth, int32_t* face_id, void* stream);
/* counts int32 [F] += 1 for every face that owns at least one pixel of keys, once per view: stamp int32 [F] (the
 * caller's, zeroed before the first view) is exchanged with stamp_value = view + 1 (positive, distinct per view) and the
 * count is raised when the old stamp differed.  A face id at or above F is ignored.  Integer atomics only: the counts are
 * the same from run to run.  F = 0 is a success that launches nothing. */
int gsr_raster_count_faces(const uint64_t* keys, int32_t H, int32_t W, int64_t F, int32_t stamp_value, int32_t* stamp,
                           int32_t* counts, void* stream);

/* ---- Mip-Splatting's 3D smoothing filter, ABI v47 (csrc/filter3d.hip, csrc/filter3d_math.h; filter3d.py; DESIGN.md
 * §7.34).  A per-Gaussian scalar `filter`, computed from the training cameras (the sampling pass and its finish), and its
 * fused application to the raw scales and opacities, forward and backward.  The float32 operation order of the sampling
 * pass and the float64 closed forms of the application are csrc/filter3d_math.h (-ffp-contract=off), written once for
 * device and host.
 * One row of the device-resident view table, 8-byte aligned, 80 bytes.  The rows are device memory and are not checked:
 * finite entries, width and height 1 .. 2^24 are the caller's contract (filter3d.compute_3d_filter checks its cameras). */
#define GSR_FILTER3D_MAX_VIEWS 65535
enum { GSR_FILTER3D_MIP_SPLATTING = 0, GSR_FILTER3D_PAPER = 1 };
typedef struct GsrFilterView {
  float world_to_view[16]; /* row-vector convention, M[4 * row + col]: the camera's float32 world_view_transform */
  float fx, fy;
  int32_t width, height;
} GsrFilterView;
/* The workspace both calls share: one (max, min) pair of floats per 64 rows and the pass's 16-byte result.  0 for a P the
 * calls refuse. */
size_t gsr_filter3d_workspace_bytes(int64_t P);
/* xyz float32 [P,3] -> min_depth float32 [P], max_rate float32 [P], seen uint8 [P].  Per row (x, y, z) and per view in
 * table order, float32, every operation rounded on its own:
 *     (xv, yv, zv) = (x, y, z, 1) through world_to_view, x' = ((x M[0] + y M[4]) + z M[8]) + M[12] and likewise y', z'
 *     next view unless zv > near_plane                                      (a NaN fails)
 *     u = (xv / zv) fx + W / 2,  w = (yv / zv) fy + H / 2
 *     next view unless -margin W <= u <= (1 + margin) W and -margin H <= w <= (1 + margin) H     (inclusive; a NaN fails)
 *     min_depth = min(min_depth, zv);  max_rate = max(max_rate, fx / zv);  seen = 1
 * starting from (+inf, 0, 0) -- or, with accumulate != 0, from the arrays' contents, so that more than 65535 views can be
 * fed in chunks; the result over chunks is the result over one table.  The call also leaves, in ws, per 64 rows the
 * maximum of min_depth and the minimum of max_rate over the seen rows, for gsr_filter3d_finish: the last call's stand.
 * One launch, one lane per row, the loop over the views inside; registers and wave shuffles only, no LDS, no atomics:
 * the same bits from run to run.  P = 0 is a success that writes nothing; V = 0 writes the start values.  Checked before
 * any HIP call: GSR_E_BADARG for P outside 0 .. 2^31 - 1, V outside 0 .. 65535, a NULL table with V > 0, a NULL array
 * with P > 0, near_plane not finite and positive, margin not finite or negative; GSR_E_ALIGN for the arrays (4 bytes), the
 * table (8) and ws (16); GSR_E_CAPACITY for a short ws.  Asynchronous, allocates nothing, reads nothing back. */
int gsr_filter3d_sample(const float* xyz, int64_t P, const GsrFilterView* views, int32_t V, float near_plane, float margin,
                        int32_t accumulate, float* min_depth, float* max_rate, uint8_t* seen, void* ws, size_t ws_bytes,
                        void* stream);
/* The three arrays and ws of gsr_filter3d_sample -> filter float32 [P] and none_seen int32 [1] (device; 1 when no row
 * was seen, else 0; always written).  With D the largest min_depth and R the smallest max_rate over the seen rows:
 *     GSR_FILTER3D_MIP_SPLATTING   filter = ((seen ? min_depth : D) / focal_max) sqrtf(variance)
 *     GSR_FILTER3D_PAPER           filter = sqrtf(variance) / (seen ? max_rate : R)
 * and 0 everywhere when no row was seen.  focal_max: the largest fx over ALL views, the caller's.  Two launches: one
 * workgroup reduces the per-64-row pairs, then one lane per row writes.  A maximum does not depend on the order: the same
 * bits from run to run.  GSR_E_BADARG for P outside 0 .. 2^31 - 1, an unknown rule, focal_max or variance not finite and
 * positive, a NULL pointer (none_seen always; the arrays with P > 0); GSR_E_ALIGN; GSR_E_CAPACITY.  P = 0 writes
 * none_seen = 1. */
int gsr_filter3d_finish(int64_t P, const float* min_depth, const float* max_rate, const uint8_t* seen, int32_t rule,
                        float focal_max, float variance, void* ws, size_t ws_bytes, float* filter, int32_t* none_seen,
                        void* stream);
/* Raw scales [P,3], raw opacities [P] and filter [P] (float32) -> the EFFECTIVE raw parameters: with f = filter,
 * a_i = exp(2 s_i), c = sqrt(prod a_i / prod (a_i + f^2)),
 *     s'_i = s_i + log1p(f^2 exp(-2 s_i)) / 2           so that exp(s'_i) = sqrt(a_i + f^2)
 *     o'   = logit(sigmoid(o) c)                        so that sigmoid(o') = sigmoid(o) c
 * o' in the form that is stable for large |o| (csrc/filter3d_math.h).  Evaluated in float64 inside the lane, each output
 * the float64 result rounded once.  f = 0 returns s and o bit for bit.  One launch, one lane per row; the outputs may not
 * alias the inputs.  P = 0 is a success that launches nothing. */
int gsr_filter3d_apply(const float* scaling, const float* opacity, const float* filter, int64_t P, float* scaling_out,
                       float* opacity_out, void* stream);
/* The gradient of gsr_filter3d_apply: dL_dscaling_out [P,3], dL_dopacity_out [P] -> dL_dscaling [P,3], dL_dopacity [P];
 * the filter carries no gradient.  Recomputed from the inputs in float64, one launch, rounded once. */
int gsr_filter3d_apply_bwd(const float* scaling, const float* opacity, const float* filter, int64_t P,
                           const float* dL_dscaling_out, const float* dL_dopacity_out, float* dL_dscaling,
                           float* dL_dopacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H_ */
