// extern "C" entry points of libgsr_hip.so (declared in include/gsr.h).  Host logic only:
// argument validation, workspace carving, kernel sequencing on the caller's stream.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include <cmath>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <string>
#include <vector>

#include "gsr_common.h"
#include "gsr_launch.h"

using namespace gsr;

namespace {
thread_local std::string g_err = "";

int fail(int code, const char* msg) {
  g_err = msg;
  return code;
}
int hip_fail(hipError_t e, const char* where) {
  g_err = std::string(where) + ": " + hipGetErrorString(e);
  return (int)e;
}
#define GSR_HIP(expr)                                        \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) return hip_fail(_e, #expr);        \
  } while (0)

// after a batch of launches: surface launch errors; in debug mode also synchronise
int check(const GsrParams* p, hipStream_t s, const char* where) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, where);
  if (p && p->debug) {
    e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, where);
  }
  return 0;
}

int validate(const GsrParams* p) {
  if (!p) return fail(GSR_E_BADARG, "params is NULL");
  if (p->P < 0 || p->width <= 0 || p->height <= 0) return fail(GSR_E_BADARG, "bad P / image size");
  if (p->width > 8191 * TILE || p->height > 8191 * TILE) return fail(GSR_E_BADARG, "image too large (13-bit tile coordinates)");
  if (p->P == 0) return 0;
  if (!p->means3D || !p->opacities || !p->viewmatrix || !p->projmatrix || !p->bg)
    return fail(GSR_E_BADARG, "means3D / opacities / viewmatrix / projmatrix / bg must be non-NULL");
  if ((p->shs == nullptr) == (p->colors_precomp == nullptr))
    return fail(GSR_E_BADARG, "provide exactly one of shs / colors_precomp");
  const bool sr = p->scales != nullptr || p->rotations != nullptr;
  if (sr && (p->scales == nullptr || p->rotations == nullptr))
    return fail(GSR_E_BADARG, "scales and rotations must be given together");
  if (sr == (p->cov3D_precomp != nullptr))
    return fail(GSR_E_BADARG, "provide exactly one of (scales, rotations) / cov3D_precomp");
  if (p->shs) {
    if (p->D < 0 || p->D > 3) return fail(GSR_E_BADARG, "sh degree must be 0..3");
    if (p->M < (p->D + 1) * (p->D + 1)) return fail(GSR_E_BADARG, "M smaller than (D+1)^2");
    if (!p->campos) return fail(GSR_E_BADARG, "campos required with shs");
    if (((uintptr_t)p->shs & 15u) != 0 && p->M == 16 && !p->shs_rest)
      return fail(GSR_E_ALIGN, "shs must be 16-byte aligned");
    if (p->shs_rest) {
      if (p->M != 16) return fail(GSR_E_BADARG, "split SH inputs (shs_rest) require M == 16");
      if (((uintptr_t)p->shs_rest & 15u) != 0) return fail(GSR_E_ALIGN, "shs_rest must be 16-byte aligned");
    }
  } else if (p->shs_rest) {
    return fail(GSR_E_BADARG, "shs_rest given without shs");
  }
  if (p->binning_mode != GSR_BINNING_TWO_LEVEL && p->binning_mode != GSR_BINNING_KEYS64 &&
      p->binning_mode != GSR_BINNING_TWO_LEVEL_CULLED)
    return fail(GSR_E_BADARG, "unknown binning_mode");
  if ((p->act_flags & (GSR_ACT_SCALE_EXP | GSR_ACT_ROT_NORMALIZE)) && !p->scales)
    return fail(GSR_E_BADARG, "scale / rotation activations need the scales + rotations inputs");
  if (p->rotations && ((uintptr_t)p->rotations & 15u) != 0) return fail(GSR_E_ALIGN, "rotations must be 16-byte aligned");
  return 0;
}

// ---- opt-in stage timers: event pairs recorded on the caller's stream ----------------------------
// Forward and backward of one frame arrive on different OS threads (autograd engine): every access takes `mu`.
struct Profile {
  struct Span { int stage; hipEvent_t a, b; };
  std::mutex mu;
  std::vector<Span> used;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    std::lock_guard<std::mutex> lock(mu);
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
  }
  void push(const Span& sp) {
    std::lock_guard<std::mutex> lock(mu);
    used.push_back(sp);
  }
};
// The count read-back of the two-call forward waits on one event per frame: it is created once per (thread, device)
// and lives as long as the thread (a fresh hipEventCreate / Destroy per frame cost ~10 us of host time).
struct ThreadEvent {
  int dev = -1;
  hipEvent_t e = nullptr;
  ~ThreadEvent() { if (e) (void)hipEventDestroy(e); }
  hipError_t get(hipEvent_t* out) {
    int d = 0;
    hipError_t err = hipGetDevice(&d);
    if (err != hipSuccess) return err;
    if (e && d != dev) { (void)hipEventDestroy(e); e = nullptr; }
    if (!e) {
      err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
      if (err != hipSuccess) { e = nullptr; return err; }
      dev = d;
    }
    *out = e;
    return hipSuccess;
  }
};
thread_local ThreadEvent g_count_event;

// ---- opt-in roctx ranges: resolved at run time, so that the library has no link-time dependency
// on a profiler; one process-wide switch (gsr_enable_markers)
typedef int (*roctx_push_fn)(const char*);
typedef int (*roctx_pop_fn)(void);
std::atomic<roctx_push_fn> g_roctx_push{nullptr};
std::atomic<roctx_pop_fn> g_roctx_pop{nullptr};
std::mutex g_roctx_mu;
const char* const kStageNames[GSR_STAGE_COUNT] = {"preprocess_fwd", "scan_block_sums", "duplicate_with_keys", "radix_sort",
                                                  "identify_tile_ranges", "render_fwd", "render_bwd", "preprocess_bwd"};
const char* const kStageMarkers[GSR_STAGE_COUNT] = {"gsr:preprocess_fwd", "gsr:scan_block_sums", "gsr:duplicate_with_keys",
                                                    "gsr:radix_sort", "gsr:identify_tile_ranges", "gsr:render_fwd",
                                                    "gsr:render_bwd", "gsr:preprocess_bwd"};

// one stage of a call: HIP-event pair on the stream when a profile handle is attached, roctx range when markers are on
struct StageTimer {
  Profile* pr; hipStream_t s; Profile::Span sp; roctx_pop_fn pop;
  StageTimer(const GsrParams* p, int stage, hipStream_t st)
      : pr(p ? static_cast<Profile*>(p->profile) : nullptr), s(st), pop(nullptr) {
    if (roctx_push_fn push = g_roctx_push.load(std::memory_order_acquire)) {
      (void)push(kStageMarkers[stage]);
      pop = g_roctx_pop.load(std::memory_order_acquire);
    }
    if (!pr) return;
    sp.stage = stage; sp.a = pr->get(); sp.b = pr->get();
    if (sp.a) (void)hipEventRecord(sp.a, s);
  }
  ~StageTimer() {
    if (pr) {
      if (sp.b) (void)hipEventRecord(sp.b, s);
      pr->push(sp);
    }
    if (pop) (void)pop();
  }
};

template <typename T>
T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
template <typename T>
const T* at(const void* base, size_t off) { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }

// where the sorted point list (and the sorted tile ids / keys) of a frame ended up
struct SortedViews {
  const uint32_t* point_list;
  const uint32_t* tile_sorted;   // mode 0
  const uint64_t* keys_sorted;   // mode 1
  // the sort's other payload buffer, free once the sort is done: render_fwd leaves the mini-block reach mask of every
  // instance (list order, 2 bytes each) there for render_bwd
  uint16_t* inst_mask;
};
SortedViews sorted_views(const void* bin_ws, uint32_t R, uint32_t V, int W, int H, int mode) {
  const ImageLayout I(W, H);
  const BinLayout B(R, V, mode);
  SortedViews v{nullptr, nullptr, nullptr, nullptr};
  char* ws = const_cast<char*>(static_cast<const char*>(bin_ws));
  if (mode == GSR_BINNING_KEYS64) {
    const bool in_b = (sort_passes(32 + tile_bits(I.tiles)) & 1) != 0;
    v.point_list = at<uint32_t>(bin_ws, in_b ? B.vals_b : B.vals_a);
    v.keys_sorted = at<uint64_t>(bin_ws, in_b ? B.keys_b : B.keys_a);
    v.inst_mask = reinterpret_cast<uint16_t*>(ws + (in_b ? B.vals_a : B.vals_b));
  } else {
    const bool in_b = (sort_passes(tile_sort_bits(I.tiles)) & 1) != 0;
    v.point_list = at<uint32_t>(bin_ws, in_b ? B.ig_b : B.ig_a);
    v.tile_sorted = at<uint32_t>(bin_ws, in_b ? B.itile_b : B.itile_a);
    v.inst_mask = reinterpret_cast<uint16_t*>(ws + (in_b ? B.ig_a : B.ig_b));
  }
  return v;
}
}  // namespace

extern "C" {

int gsr_abi_version(void) { return GSR_ABI_VERSION; }
const char* gsr_last_error(void) { return g_err.c_str(); }
const char* gsr_build_info(void) { return "libgsr_hip gfx950 wave64 tile16 radix6-9 binning:culled|two_level|keys64 (HIP " __DATE__ ")"; }

size_t gsr_geom_bytes(int32_t P) { return GeomLayout(P < 0 ? 0 : P).bytes; }
size_t gsr_image_bytes(int32_t width, int32_t height) { return ImageLayout(width, height).bytes; }
size_t gsr_binning_bytes(uint32_t num_rendered, uint32_t num_visible, int32_t, int32_t, int32_t mode) {
  return BinLayout(num_rendered, num_visible, mode).bytes;
}
size_t gsr_backward_bytes(int32_t P, uint32_t num_rendered) { return BwdLayout(P, num_rendered).bytes; }
size_t gsr_camera_grad_bytes(int32_t P) { return camera_grad_bytes(P); }
size_t gsr_sort_scratch_bytes(uint32_t n) { return SortLayout(n).bytes; }

}  // extern "C"

static void enqueue_depth_top_pass(const GsrParams* p, void* geom_ws, hipStream_t s);

// Stage 1 on the stream: preprocess, scan of the block totals (counts -> total[] and the pinned mirror), `counted`
// recorded behind the scan, then -- two-level modes -- compaction of the visible Gaussians and their depth sort.
// None of it needs a host-side count: the grids are sized for P and the kernels read V from the device.
// top_pass: WITH = enqueued here, decides on the device (gsr_forward); LATER = the host enqueues it behind stage 1 for the
// frames that need it (two-call path, which knows the span); NEVER = the caller vouches for a narrow frame
// (GsrParams::depth_span_lt24): the device-side switch stays off whatever the span.
enum TopPass { TOP_PASS_WITH, TOP_PASS_LATER, TOP_PASS_NEVER };
static int enqueue_stage1(const GsrParams* p, void* geom_ws, int32_t* radii, hipStream_t s, uint32_t capacity,
                          hipEvent_t counted, TopPass top_pass) {
  const GeomLayout L(p->P);
  {
    StageTimer t(p, GSR_STAGE_PREPROCESS_FWD, s);
    launch_preprocess_fwd(*p, at<GeomRec>(geom_ws, L.rec), at<BinInfo>(geom_ws, L.bin),
                          at<uint32_t>(geom_ws, L.block_sums), at<uint32_t>(geom_ws, L.block_vis), radii,
                          at<uint32_t>(geom_ws, L.block_big), at<uint32_t>(geom_ws, L.big_list),
                          at<uint2>(geom_ws, L.block_range), s);
  }
  if (int rc = check(p, s, "preprocess_fwd")) return rc;
  uint32_t* total = at<uint32_t>(geom_ws, L.total);
  {
    StageTimer t(p, GSR_STAGE_SCAN, s);
    launch_scan_block_sums(at<uint32_t>(geom_ws, L.block_sums), at<uint32_t>(geom_ws, L.block_offs), total + TOTAL_R,
                           at<uint32_t>(geom_ws, L.block_vis), at<uint32_t>(geom_ws, L.block_vis_offs), total + TOTAL_V,
                           L.nblocks, s, p->counts_pinned, at<uint2>(geom_ws, L.block_range),
                           at<uint32_t>(geom_ws, L.block_big), at<uint32_t>(geom_ws, L.block_big_offs), total + TOTAL_BIG);
  }
  if (int rc = check(p, s, "scan_block_sums")) return rc;
  if (counted) GSR_HIP(hipEventRecord(counted, s));
  if (p->binning_mode != GSR_BINNING_KEYS64) {
    StageTimer t(p, GSR_STAGE_SORT, s);
    launch_compact_visible(p->P, at<BinInfo>(geom_ws, L.bin), at<uint32_t>(geom_ws, L.block_vis_offs),
                           at<uint32_t>(geom_ws, L.block_offs),
                           p->forward_only ? nullptr : at<uint32_t>(geom_ws, L.slot_base), total, capacity,
                           (p->width + TILE - 1) / TILE, at<uint32_t>(geom_ws, L.dkey_a), at<uint2>(geom_ws, L.didx_a), s,
                           top_pass != TOP_PASS_NEVER);
    launch_sort_pairs_u32_v64(at<uint32_t>(geom_ws, L.dkey_a), at<uint2>(geom_ws, L.didx_a),
                              at<uint32_t>(geom_ws, L.dkey_b), at<uint2>(geom_ws, L.didx_b), (uint32_t)p->P,
                              DEPTH_SORT_BITS, at<char>(geom_ws, L.dsort), s, total + TOTAL_V);
    if (top_pass == TOP_PASS_WITH) enqueue_depth_top_pass(p, geom_ws, s);
  }
  return check(p, s, "depth_sort");
}

// The depth sort's fourth pass (bits 24..31 of the relative depth key).  Its element count is total[TOTAL_TOP_PASS_N]:
// V for a frame that spans more than 2^24 float32 steps of depth, 0 otherwise (the three kernels then exit at once).
// The consumers (count_tiles / emit_instances) read the same word to pick the buffer the sorted payload ended in.
static void enqueue_depth_top_pass(const GsrParams* p, void* geom_ws, hipStream_t s) {
  const GeomLayout L(p->P);
  const bool in_b = (sort_passes(DEPTH_SORT_BITS) & 1) != 0;
  launch_sort_extra_pass_u32(at<uint32_t>(geom_ws, in_b ? L.dkey_b : L.dkey_a), at<uint2>(geom_ws, in_b ? L.didx_b : L.didx_a),
                             at<uint32_t>(geom_ws, in_b ? L.dkey_a : L.dkey_b), at<uint2>(geom_ws, in_b ? L.didx_a : L.didx_b),
                             (uint32_t)p->P, at<uint32_t>(geom_ws, L.total) + TOTAL_TOP_PASS_N, DEPTH_SORT_BITS,
                             32 - DEPTH_SORT_BITS, at<char>(geom_ws, L.dsort), s);
}

// Stage 2 on the stream: instance emission, tile sort, tile ranges, compositing.  (r_cap, v_cap) are what the binning
// workspace is laid out for: the real counts in the two-call forward (device_counts = false), the caller's capacity
// and P in gsr_forward (device_counts = true: every kernel takes the real counts from total[]).
static int enqueue_stage2(const GsrParams* p, void* geom_ws, void* bin_ws, size_t bin_ws_bytes, void* img_ws,
                          uint32_t r_cap, uint32_t v_cap, bool device_counts, float* out_color, hipStream_t s) {
  const ImageLayout I(p->width, p->height);
  uint2* ranges = at<uint2>(img_ws, I.ranges);
  // two-level modes: the ranges come out of the tile sort's own histogram (no memset, no pass over the sorted keys), and
  // they and the tile order are built by a workgroup that rides in the sort's last scatter launch (SortedRuns::order);
  // 64-bit key mode, or nothing to bin: upstream's identifyTileRanges into a zero-filled array
  SortedRuns runs;
  runs.valid = false;
  runs.fused = false;
  runs.runs_rel = ranges;
  runs.n_keys = (uint32_t)I.tiles;
  runs.order = at<uint32_t>(img_ws, I.tile_order);
  const uint32_t* point_list = nullptr;
  uint16_t* inst_mask = nullptr;     // the sort's spare payload buffer (see SortedViews)
  const GeomRec* rec = nullptr;
  if (p->P > 0 && r_cap > 0) {
    if (!geom_ws || !bin_ws) return fail(GSR_E_BADARG, "geom_ws / bin_ws is NULL");
    if (v_cap == 0 || v_cap > (uint32_t)p->P || (!device_counts && v_cap > r_cap))
      return fail(GSR_E_BADARG, "num_visible inconsistent with num_rendered / P");
    const int mode = p->binning_mode;
    const BinLayout B(r_cap, v_cap, mode);
    if (bin_ws_bytes < B.bytes) return fail(GSR_E_CAPACITY, "binning workspace too small for num_rendered / num_visible");
    if (((uintptr_t)bin_ws & 255u) != 0) return fail(GSR_E_ALIGN, "bin_ws must be 256-byte aligned");
    const GeomLayout L(p->P);
    rec = at<GeomRec>(geom_ws, L.rec);
    const BinInfo* bin = at<BinInfo>(geom_ws, L.bin);
    const uint32_t* total = at<uint32_t>(geom_ws, L.total);
    const int tb = mode == GSR_BINNING_KEYS64 ? tile_bits(I.tiles) : tile_sort_bits(I.tiles);
    if (mode == GSR_BINNING_KEYS64) {
      if (device_counts) return fail(GSR_E_BADARG, "gsr_forward supports the two-level binning modes only");
      uint64_t* ka = at<uint64_t>(bin_ws, B.keys_a);
      uint64_t* kb = at<uint64_t>(bin_ws, B.keys_b);
      uint32_t* va = at<uint32_t>(bin_ws, B.vals_a);
      uint32_t* vb = at<uint32_t>(bin_ws, B.vals_b);
      {
        StageTimer t(p, GSR_STAGE_DUPLICATE, s);
        launch_duplicate_with_keys(p->P, I.grid_x, bin, at<uint32_t>(geom_ws, L.block_offs),
                                   at<uint32_t>(geom_ws, L.slot_base), at<uint32_t>(geom_ws, L.offsets), ka, va, s);
      }
      if (int rc = check(p, s, "duplicate_with_keys")) return rc;
      bool in_b;
      {
        StageTimer t(p, GSR_STAGE_SORT, s);
        in_b = launch_sort_pairs(ka, va, kb, vb, r_cap, 32 + tb, at<char>(bin_ws, B.sort), s);
      }
      if (int rc = check(p, s, "sort_pairs")) return rc;
      {
        StageTimer t(p, GSR_STAGE_RANGES, s);
        GSR_HIP(hipMemsetAsync(ranges, 0, 8 * (size_t)I.tiles, s));
        launch_identify_tile_ranges(r_cap, in_b ? kb : ka, ranges, s);
      }
      point_list = in_b ? vb : va;
      inst_mask = reinterpret_cast<uint16_t*>(in_b ? va : vb);
    } else {
      uint32_t* ita = at<uint32_t>(bin_ws, B.itile_a);
      uint32_t* itb = at<uint32_t>(bin_ws, B.itile_b);
      uint32_t* iga = at<uint32_t>(bin_ws, B.ig_a);
      uint32_t* igb = at<uint32_t>(bin_ws, B.ig_b);
      uint32_t* bsum2 = at<uint32_t>(bin_ws, B.bsum2);
      uint32_t* boffs2 = at<uint32_t>(bin_ws, B.boffs2);
      // depth-sorted payload: produced by stage 1 in the geometry workspace, in d3 or (after the top-digit pass) in d4
      const bool in_b3 = (sort_passes(DEPTH_SORT_BITS) & 1) != 0;
      const uint2* d3 = at<uint2>(geom_ws, in_b3 ? L.didx_b : L.didx_a);
      const uint2* d4 = at<uint2>(geom_ws, in_b3 ? L.didx_a : L.didx_b);
      const uint32_t cap = device_counts ? r_cap : 0xffffffffu;
      {
        StageTimer t(p, GSR_STAGE_DUPLICATE, s);   // instances emitted in depth order
        launch_count_tiles(v_cap, total, d3, d4, bin, bsum2, s);
        if (emit_is_wide(v_cap)) {      // small frame: the emission sums the block totals itself, no scan launch
          launch_emit_instances(v_cap, total, I.grid_x, d3, d4, bin, bsum2, ita, iga, cap, s);
        } else {
          launch_scan_block_sums(bsum2, boffs2, boffs2 + B.nblocks2 + 1, nullptr, nullptr, nullptr, (int)B.nblocks2, s);
          launch_emit_instances(v_cap, total, I.grid_x, d3, d4, bin, boffs2, ita, iga, cap, s);
        }
      }
      if (int rc = check(p, s, "emit_instances")) return rc;
      const uint32_t* r_dev = device_counts ? total + TOTAL_R_CLAMPED : nullptr;
      bool in_b;
      {
        StageTimer t(p, GSR_STAGE_SORT, s);     // stable partition by tile id
        in_b = launch_sort_pairs_u32(ita, iga, itb, igb, r_cap, tb, at<char>(bin_ws, B.sort), s, r_dev, &runs);
      }
      if (int rc = check(p, s, "tile_sort")) return rc;
      if (!runs.valid) {       // more than 2^18 tiles: three passes -- read the ranges off the sorted keys
        StageTimer t(p, GSR_STAGE_RANGES, s);
        GSR_HIP(hipMemsetAsync(ranges, 0, 8 * (size_t)I.tiles, s));
        launch_identify_tile_ranges_u32(r_cap, in_b ? itb : ita, ranges, s, r_dev);
      }
      point_list = in_b ? igb : iga;
      inst_mask = reinterpret_cast<uint16_t*>(in_b ? iga : igb);
    }
    if (int rc = check(p, s, "identify_tile_ranges")) return rc;
  } else {
    GSR_HIP(hipMemsetAsync(ranges, 0, 8 * (size_t)I.tiles, s));      // nothing to bin: every tile is empty
  }
  if (!runs.fused) {     // fused: the ranges stage has no interval of its own (its stage count stays 0)
    StageTimer t(p, GSR_STAGE_RANGES, s);
    if (runs.valid) launch_ranges_and_order_from_sort(I.tiles, runs, ranges, at<uint32_t>(img_ws, I.tile_order), s);
    else launch_build_tile_order(I.tiles, ranges, at<uint32_t>(img_ws, I.tile_order), s);
  }
  {
    StageTimer t(p, GSR_STAGE_RENDER_FWD, s);
    const bool track = !p->forward_only;
    launch_render_fwd(p->width, p->height, ranges, point_list, rec, p->bg, out_color,
                      track ? at<float>(img_ws, I.final_T) : nullptr, track ? at<uint32_t>(img_ws, I.n_contrib) : nullptr,
                      track ? at<uint32_t>(img_ws, I.tile_max) : nullptr, at<uint32_t>(img_ws, I.tile_order), s, nullptr,
                      (p->debug_flags & GSR_DEBUG_NO_MINIBLOCK_CULL) ? 0 : 1, track ? inst_mask : nullptr);
  }
  return check(p, s, "render_fwd");
}

// ---- shared by the map entry points below (depth, features, distortion, median, contribution) ----------------------
// what the map kernels read of a validated frame that is not empty
static MapFrame map_frame(const GsrAuxFrame* f) {
  const ImageLayout I(f->width, f->height);
  const GeomLayout L(f->P);
  const SortedViews sv = sorted_views(f->bin_ws, f->num_rendered, f->num_visible, f->width, f->height, f->binning_mode);
  return MapFrame{f->width, f->height, I.grid_x, I.tiles, at<uint2>(f->img_ws, I.ranges), sv.point_list,
                  at<GeomRec>(f->geom_ws, L.rec), at<BinInfo>(f->geom_ws, L.bin), at<uint32_t>(f->img_ws, I.n_contrib),
                  at<float>(f->img_ws, I.final_T), at<uint32_t>(f->img_ws, I.tile_order)};
}

// A map's backward behind its refusals: zero acc [P,8] (nullptr: the geometry side is not wanted, and g is NULL), then
// also_zero (the features' dL_dfeatures; nullptr: nothing), run the map's own kernel (launch, named where) on the frame's
// lists, then take acc to the inputs with aux_geom_bwd
template <typename Launch>
static int run_geom_backward(const GsrParams* p, const GsrAuxFrame* f, float* acc, const GsrAuxGrads* g, hipStream_t s,
                             const char* where, Launch launch, void* also_zero = nullptr, size_t also_zero_bytes = 0) {
  if (acc) GSR_HIP(hipMemsetAsync(acc, 0, 32 * (size_t)p->P, s));
  if (also_zero) GSR_HIP(hipMemsetAsync(also_zero, 0, also_zero_bytes, s));
  if (f->num_rendered > 0) {
    launch(map_frame(f));
    if (int rc = check(p, s, where)) return rc;
  }
  if (!g) return 0;
  launch_aux_geom_bwd(*p, f->radii, acc, *g, s);
  return check(p, s, "aux_geom_bwd");
}

extern "C" {

int gsr_forward_preprocess(const GsrParams* p, void* geom_ws, int32_t* radii, void* stream, uint32_t* num_rendered,
                           uint32_t* num_visible) {
  if (int rc = validate(p)) return rc;
  if (!num_rendered || !num_visible) return fail(GSR_E_BADARG, "num_rendered / num_visible is NULL");
  *num_rendered = 0;
  *num_visible = 0;
  if (p->P == 0) return 0;
  if (!geom_ws || !radii) return fail(GSR_E_BADARG, "geom_ws / radii is NULL");
  if (((uintptr_t)geom_ws & 255u) != 0) return fail(GSR_E_ALIGN, "geom_ws must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GeomLayout L(p->P);
  hipEvent_t counted = nullptr;
  if (p->counts_pinned) GSR_HIP(g_count_event.get(&counted));
  // the first half of the two-level binning is enqueued before the read-back, so that the GPU sorts while the host
  // round-trips; the top-digit pass follows only for the frames that need it (the host knows once the counts are in)
  if (int rc = enqueue_stage1(p, geom_ws, radii, s, 0xffffffffu, counted, TOP_PASS_LATER)) return rc;
  uint32_t depth_min = 0, depth_max = 0;
  if (counted) {
    const hipError_t e = hipEventSynchronize(counted);     // waits for the scan kernel only
    if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize(counted)");
    *num_rendered = p->counts_pinned[0];
    *num_visible = p->counts_pinned[1];
    depth_min = p->counts_pinned[2];
    depth_max = p->counts_pinned[3];
  } else {
    uint32_t host[6] = {0, 0, 0, 0, 0, 0};
    GSR_HIP(hipMemcpyAsync(host, at<uint32_t>(geom_ws, L.total), sizeof(host), hipMemcpyDeviceToHost, s));
    GSR_HIP(hipStreamSynchronize(s));
    *num_rendered = host[TOTAL_R];
    *num_visible = host[TOTAL_V];
    depth_min = ~host[TOTAL_DEPTH_INV_MIN];
    depth_max = host[TOTAL_DEPTH_MAX];
  }
  if (p->binning_mode != GSR_BINNING_KEYS64 && *num_visible > 0 && depth_max >= depth_min &&
      ((uint64_t)depth_max - depth_min) >> DEPTH_SORT_BITS) {
    StageTimer t(p, GSR_STAGE_SORT, s);
    enqueue_depth_top_pass(p, geom_ws, s);
    if (int rc = check(p, s, "depth_sort_top_digit")) return rc;
  }
  return 0;
}

int gsr_forward_render(const GsrParams* p, void* geom_ws, void* bin_ws, size_t bin_ws_bytes, void* img_ws,
                       uint32_t R, uint32_t V, float* out_color, void* stream) {
  if (int rc = validate(p)) return rc;
  if (!img_ws || !out_color) return fail(GSR_E_BADARG, "img_ws / out_color is NULL");
  return enqueue_stage2(p, geom_ws, bin_ws, bin_ws_bytes, img_ws, R, V, false, out_color, static_cast<hipStream_t>(stream));
}

int gsr_forward(const GsrParams* p, void* geom_ws, void* bin_ws, size_t bin_ws_bytes, uint32_t capacity, void* img_ws,
                int32_t* radii, float* out_color, void* counts_event, void* stream) {
  if (int rc = validate(p)) return rc;
  if (!img_ws || !out_color) return fail(GSR_E_BADARG, "img_ws / out_color is NULL");
  if (p->P > 0 && p->binning_mode == GSR_BINNING_KEYS64)
    return fail(GSR_E_BADARG, "gsr_forward supports the two-level binning modes only");
  if (p->P > 0 && !p->counts_pinned)
    return fail(GSR_E_BADARG, "gsr_forward needs counts_pinned (the caller detects an overflow of `capacity` there)");
  if (p->P > 0 && capacity == 0) return fail(GSR_E_BADARG, "capacity is 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p->P > 0) {
    if (!geom_ws || !radii) return fail(GSR_E_BADARG, "geom_ws / radii is NULL");
    if (((uintptr_t)geom_ws & 255u) != 0) return fail(GSR_E_ALIGN, "geom_ws must be 256-byte aligned");
    // the depth sort's fourth pass: enqueued (and decided on the device) unless the caller vouches for a narrow frame
    if (int rc = enqueue_stage1(p, geom_ws, radii, s, capacity, static_cast<hipEvent_t>(counts_event),
                                p->depth_span_lt24 ? TOP_PASS_NEVER : TOP_PASS_WITH))
      return rc;
  } else if (counts_event) {
    GSR_HIP(hipEventRecord(static_cast<hipEvent_t>(counts_event), s));
  }
  return enqueue_stage2(p, geom_ws, bin_ws, bin_ws_bytes, img_ws, p->P > 0 ? capacity : 0u, (uint32_t)p->P, true, out_color, s);
}

int gsr_event_create(void** event) {
  if (!event) return fail(GSR_E_BADARG, "event is NULL");
  hipEvent_t e = nullptr;
  GSR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  *event = e;
  return 0;
}
int gsr_event_destroy(void* event) {
  if (event) GSR_HIP(hipEventDestroy(static_cast<hipEvent_t>(event)));
  return 0;
}
int gsr_event_wait(void* event) {
  if (!event) return fail(GSR_E_BADARG, "event is NULL");
  GSR_HIP(hipEventSynchronize(static_cast<hipEvent_t>(event)));
  return 0;
}
int gsr_event_query(void* event, int32_t* done) {
  if (!event || !done) return fail(GSR_E_BADARG, "NULL argument");
  const hipError_t e = hipEventQuery(static_cast<hipEvent_t>(event));
  if (e != hipSuccess && e != hipErrorNotReady) return hip_fail(e, "hipEventQuery");
  *done = e == hipSuccess ? 1 : 0;
  return 0;
}

int gsr_enable_markers(int32_t on) {
  std::lock_guard<std::mutex> lock(g_roctx_mu);
  if (!on) {
    g_roctx_push.store(nullptr, std::memory_order_release);
    return 0;
  }
  if (g_roctx_push.load(std::memory_order_acquire)) return 0;
  static const char* const libs[] = {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so",
                                     "libroctx64.so.4"};
  for (const char* name : libs) {
    void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    if (!h) continue;
    roctx_push_fn push = reinterpret_cast<roctx_push_fn>(dlsym(h, "roctxRangePushA"));
    roctx_pop_fn pop = reinterpret_cast<roctx_pop_fn>(dlsym(h, "roctxRangePop"));
    if (push && pop) {
      g_roctx_pop.store(pop, std::memory_order_release);
      g_roctx_push.store(push, std::memory_order_release);
      return 0;
    }
  }
  return fail(GSR_E_BADARG, "no roctx library found (librocprofiler-sdk-roctx.so / libroctx64.so)");
}

int gsr_backward(const GsrParams* p, const int32_t* radii, const void* geom_ws, const void* bin_ws, const void* img_ws,
                 uint32_t R, uint32_t V, const float* dL_dout_color, void* bwd_ws, size_t bwd_ws_bytes,
                 const GsrGrads* grads, void* stream) {
  if (p && p->forward_only) return fail(GSR_E_BADARG, "the forward ran with forward_only = 1: no state for a backward");
  if (int rc = validate(p)) return rc;
  if (!grads) return fail(GSR_E_BADARG, "grads is NULL");
  const int n_cam = (grads->dL_dviewmatrix != nullptr) + (grads->dL_dprojmatrix != nullptr) + (grads->dL_dcampos != nullptr);
  if (n_cam != 0 && n_cam != 3)
    return fail(GSR_E_BADARG, "dL_dviewmatrix / dL_dprojmatrix / dL_dcampos must be given together");
  if (n_cam && !grads->camera_ws) return fail(GSR_E_BADARG, "camera gradients need camera_ws (gsr_camera_grad_bytes(P) bytes)");
  if (n_cam && ((uintptr_t)grads->camera_ws & 255u) != 0) return fail(GSR_E_ALIGN, "camera_ws must be 256-byte aligned");
  if (p->P == 0) {
    if (n_cam) {        // no Gaussian: the three camera gradients are zeros
      launch_camera_grad_finish(*grads, 0, static_cast<hipStream_t>(stream));
      return check(p, static_cast<hipStream_t>(stream), "camera_grad_finish");
    }
    return 0;
  }
  if (!radii || !geom_ws || !img_ws || !dL_dout_color || !bwd_ws) return fail(GSR_E_BADARG, "NULL workspace / input");
  if (!grads->dL_dmeans3D || !grads->dL_dmeans2D || !grads->dL_dopacities)
    return fail(GSR_E_BADARG, "dL_dmeans3D / dL_dmeans2D / dL_dopacities must be non-NULL");
  if (p->shs && !grads->dL_dshs) return fail(GSR_E_BADARG, "dL_dshs required with shs");
  if (p->shs_rest && !grads->dL_dshs_rest) return fail(GSR_E_BADARG, "dL_dshs_rest required with shs_rest");
  if (p->shs_rest && ((uintptr_t)grads->dL_dshs_rest & 15u) != 0) return fail(GSR_E_ALIGN, "dL_dshs_rest must be 16-byte aligned");
  if (p->shs && !p->shs_rest && p->M == 16 && ((uintptr_t)grads->dL_dshs & 15u) != 0)
    return fail(GSR_E_ALIGN, "dL_dshs must be 16-byte aligned");
  if (p->colors_precomp && !grads->dL_dcolors) return fail(GSR_E_BADARG, "dL_dcolors required with colors_precomp");
  {
    const int n_stats = (grads->stats_xyz_gradient_accum != nullptr) + (grads->stats_denom != nullptr) +
                        (grads->stats_max_radii2D != nullptr);
    if (n_stats != 0 && n_stats != 3) return fail(GSR_E_BADARG, "the three stats_* pointers must be given together");
  }
  const BwdLayout Wl(p->P, R);
  if (bwd_ws_bytes < Wl.bytes) return fail(GSR_E_CAPACITY, "backward workspace too small");
  if (((uintptr_t)bwd_ws & 255u) != 0) return fail(GSR_E_ALIGN, "bwd_ws must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GeomLayout L(p->P);
  const ImageLayout I(p->width, p->height);
  GradRow* rows = at<GradRow>(bwd_ws, Wl.rows);
  uint8_t* flags = at<uint8_t>(bwd_ws, Wl.flags);
  const GeomRec* rec = at<GeomRec>(geom_ws, L.rec);
  if (R > 0) {
    if (!bin_ws) return fail(GSR_E_BADARG, "bin_ws is NULL");
    const SortedViews sv = sorted_views(bin_ws, R, V, p->width, p->height, p->binning_mode);
    const uint32_t* point_list = sv.point_list;
    GSR_HIP(hipMemsetAsync(flags, 0, R, s));
    {
      StageTimer t(p, GSR_STAGE_RENDER_BWD, s);
      launch_render_bwd(p->width, p->height, at<uint2>(img_ws, I.ranges), point_list, rec,
                        at<uint32_t>(geom_ws, L.slot_base), p->bg,
                        at<float>(img_ws, I.final_T), at<uint32_t>(img_ws, I.n_contrib),
                        at<uint32_t>(img_ws, I.tile_max), dL_dout_color, rows, flags,
                        at<uint32_t>(img_ws, I.tile_order), s, sv.inst_mask);
    }
    if (int rc = check(p, s, "render_bwd")) return rc;
  }
  {
    StageTimer t(p, GSR_STAGE_PREPROCESS_BWD, s);
    launch_sum_big_rows(at<uint32_t>(geom_ws, L.total) + TOTAL_BIG, at<uint32_t>(geom_ws, L.block_big_offs), L.nblocks,
                        at<uint32_t>(geom_ws, L.big_list), rec, at<uint32_t>(geom_ws, L.slot_base), rows, flags, s);
    launch_preprocess_bwd(*p, radii, rec, at<uint32_t>(geom_ws, L.slot_base), rows, flags, *grads, s);
  }
  return check(p, s, "preprocess_bwd");
}

// ---- depth / inverse-depth / alpha maps (csrc/depth.hip) -----------------------------------------------------------
static int validate_aux_frame(const GsrAuxFrame* f) {
  if (!f) return fail(GSR_E_BADARG, "frame is NULL");
  if (f->P < 0 || f->width <= 0 || f->height <= 0) return fail(GSR_E_BADARG, "bad P / image size");
  if (f->width > 8191 * TILE || f->height > 8191 * TILE) return fail(GSR_E_BADARG, "image too large (13-bit tile coordinates)");
  if (!f->img_ws) return fail(GSR_E_BADARG, "img_ws is NULL");
  if (f->binning_mode != GSR_BINNING_TWO_LEVEL && f->binning_mode != GSR_BINNING_KEYS64 &&
      f->binning_mode != GSR_BINNING_TWO_LEVEL_CULLED)
    return fail(GSR_E_BADARG, "unknown binning_mode");
  if (f->P > 0 && f->num_rendered > 0 && (!f->geom_ws || !f->bin_ws)) return fail(GSR_E_BADARG, "geom_ws / bin_ws is NULL");
  return 0;
}

// the members of GsrParams the maps' backward reads (validate() also insists on a colour input, which it does not need)
static int validate_aux_inputs(const GsrParams* p) {
  if (p->P <= 0) return 0;
  if (!p->means3D || !p->opacities || !p->viewmatrix || !p->projmatrix)
    return fail(GSR_E_BADARG, "means3D / opacities / viewmatrix / projmatrix must be non-NULL");
  const bool sr = p->scales != nullptr || p->rotations != nullptr;
  if (sr && (p->scales == nullptr || p->rotations == nullptr))
    return fail(GSR_E_BADARG, "scales and rotations must be given together");
  if (sr == (p->cov3D_precomp != nullptr))
    return fail(GSR_E_BADARG, "provide exactly one of (scales, rotations) / cov3D_precomp");
  if ((p->act_flags & (GSR_ACT_SCALE_EXP | GSR_ACT_ROT_NORMALIZE)) && !p->scales)
    return fail(GSR_E_BADARG, "scale / rotation activations need the scales + rotations inputs");
  if (p->rotations && ((uintptr_t)p->rotations & 15u) != 0) return fail(GSR_E_ALIGN, "rotations must be 16-byte aligned");
  return 0;
}

// nothing was binned: every list is empty
static bool frame_is_empty(const GsrAuxFrame* f) { return f->P == 0 || f->num_rendered == 0; }

// The refusals the maps' backwards share.  A map's own argument checks sit between them, where they have always sat:
// refuse_backward opens every backward, refuse_mismatch follows the map's checks, and behind the "P == 0: nothing to
// do" return come refuse_geom_outputs (the maps with a [P,8] accumulator) or refuse_acc_ws alone (the median).
static int refuse_backward(const GsrParams* p, const GsrAuxFrame* f) {
  if (!p) return fail(GSR_E_BADARG, "params is NULL");
  if (p->forward_only) return fail(GSR_E_BADARG, "the forward ran with forward_only = 1: no state for a backward");
  return validate_aux_frame(f);
}
static int refuse_mismatch(const GsrParams* p, const GsrAuxFrame* f) {
  if (f->P != p->P || f->width != p->width || f->height != p->height) return fail(GSR_E_BADARG, "frame and params disagree");
  return 0;
}
// short_code: what a workspace of fewer than `need` bytes is answered with
static int refuse_acc_ws(const void* acc_ws, size_t acc_ws_bytes, size_t need, int short_code) {
  if (acc_ws_bytes < need) return fail(short_code, "accumulator workspace too small");
  if (((uintptr_t)acc_ws & 255u) != 0) return fail(GSR_E_ALIGN, "acc_ws must be 256-byte aligned");
  return 0;
}
// have_inputs: the map's own input pointers are all there
static int refuse_geom_outputs(const GsrParams* p, const GsrAuxFrame* f, bool have_inputs, const void* acc_ws,
                               size_t acc_ws_bytes, const GsrAuxGrads* g, int short_code) {
  if (!have_inputs || !acc_ws || !f->radii) return fail(GSR_E_BADARG, "NULL workspace / input");
  if (!g->dL_dmeans3D || !g->dL_dmeans2D || !g->dL_dopacities)
    return fail(GSR_E_BADARG, "dL_dmeans3D / dL_dmeans2D / dL_dopacities must be non-NULL");
  return refuse_acc_ws(acc_ws, acc_ws_bytes, gsr_aux_maps_backward_bytes(p->P), short_code);
}

size_t gsr_aux_maps_backward_bytes(int32_t P) { return align_up(32 * (size_t)(P > 0 ? P : 1), 256); }

int gsr_aux_maps_forward(const GsrAuxFrame* f, float* maps, void* stream) {
  if (int rc = validate_aux_frame(f)) return rc;
  if (!maps) return fail(GSR_E_BADARG, "maps is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (frame_is_empty(f)) {
    GSR_HIP(hipMemsetAsync(maps, 0, 12 * (size_t)f->width * f->height, s));
    return 0;
  }
  launch_aux_maps_fwd(map_frame(f), maps, s);
  return check(nullptr, s, "aux_maps_fwd");
}

int gsr_aux_maps_backward(const GsrParams* p, const GsrAuxFrame* f, const float* dL_dmaps, void* acc_ws,
                          size_t acc_ws_bytes, const GsrAuxGrads* g, void* stream) {
  if (int rc = refuse_backward(p, f)) return rc;
  if (int rc = validate_aux_inputs(p)) return rc;
  if (int rc = refuse_mismatch(p, f)) return rc;
  if (!g) return fail(GSR_E_BADARG, "grads is NULL");
  if (p->P == 0) return 0;
  if (int rc = refuse_geom_outputs(p, f, dL_dmaps != nullptr, acc_ws, acc_ws_bytes, g, GSR_E_CAPACITY)) return rc;
  float* acc = static_cast<float*>(acc_ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return run_geom_backward(p, f, acc, g, s, "aux_maps_bwd",
                           [&](const MapFrame& mf) { launch_aux_maps_bwd(mf, dL_dmaps, acc, s); });
}

// ---- per-Gaussian feature vectors composited to C-channel maps (csrc/features.hip) ---------------------------------
static int validate_features(const float* features, int32_t C) {
  if (C < 1) return fail(GSR_E_BADARG, "C must be >= 1");
  if (C > 8 * 65535) return fail(GSR_E_BADARG, "C too large (65535 channel groups)");
  if (!features) return fail(GSR_E_BADARG, "features is NULL");
  return 0;
}

size_t gsr_feature_maps_backward_bytes(int32_t P) { return gsr_aux_maps_backward_bytes(P); }

int gsr_feature_maps_forward(const GsrAuxFrame* f, const float* features, int32_t C, float* maps, void* stream) {
  if (int rc = validate_aux_frame(f)) return rc;
  if (int rc = validate_features(features, C)) return rc;
  if (!maps) return fail(GSR_E_BADARG, "maps is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (frame_is_empty(f)) {
    GSR_HIP(hipMemsetAsync(maps, 0, 4 * (size_t)C * f->width * f->height, s));
    return 0;
  }
  launch_feature_maps_fwd(map_frame(f), features, C, maps, s);
  return check(nullptr, s, "feature_maps_fwd");
}

int gsr_feature_maps_backward(const GsrParams* p, const GsrAuxFrame* f, const float* features, int32_t C,
                              const float* dL_dmaps, float* dL_dfeatures, void* acc_ws, size_t acc_ws_bytes,
                              const GsrAuxGrads* g, void* stream) {
  if (int rc = refuse_backward(p, f)) return rc;
  if (int rc = validate_features(features, C)) return rc;
  if (int rc = refuse_mismatch(p, f)) return rc;
  if (p->P == 0 || (!g && !dL_dfeatures)) return 0;
  if (!dL_dmaps) return fail(GSR_E_BADARG, "dL_dmaps is NULL");
  if (g) {
    if (int rc = validate_aux_inputs(p)) return rc;
    if (int rc = refuse_geom_outputs(p, f, true, acc_ws, acc_ws_bytes, g, GSR_E_CAPACITY)) return rc;
  }
  float* acc = g ? static_cast<float*>(acc_ws) : nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return run_geom_backward(
      p, f, acc, g, s, "feature_maps_bwd",
      [&](const MapFrame& mf) { launch_feature_maps_bwd(mf, features, C, dL_dmaps, acc, dL_dfeatures, s); }, dL_dfeatures,
      dL_dfeatures ? 4 * (size_t)p->P * (size_t)C : 0);
}

// ---- depth-distortion map (csrc/distortion.hip) --------------------------------------------------------------------
static int validate_distortion_mapping(int32_t mapping, float near, float far) {
  if (mapping != 0 && mapping != 1) return fail(GSR_E_BADARG, "mapping must be 0 (linear) or 1 (ndc)");
  if (mapping == 1 && !(std::isfinite(near) && std::isfinite(far) && near > 0.0f && near < far))
    return fail(GSR_E_BADARG, "mapping 1 needs finite 0 < near < far");
  return 0;
}

size_t gsr_distortion_backward_bytes(int32_t P) { return gsr_aux_maps_backward_bytes(P); }

int gsr_distortion_forward(const GsrAuxFrame* f, int32_t mapping, float near, float far, float* dist, float* state,
                           void* stream) {
  if (int rc = validate_aux_frame(f)) return rc;
  if (int rc = validate_distortion_mapping(mapping, near, far)) return rc;
  if (!dist || !state) return fail(GSR_E_BADARG, "dist / state is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (frame_is_empty(f)) {
    GSR_HIP(hipMemsetAsync(dist, 0, 4 * (size_t)f->width * f->height, s));
    GSR_HIP(hipMemsetAsync(state, 0, 8 * (size_t)f->width * f->height, s));
    return 0;
  }
  launch_distortion_fwd(map_frame(f), mapping, near, far, dist, state, s);
  return check(nullptr, s, "distortion_fwd");
}

int gsr_distortion_backward(const GsrParams* p, const GsrAuxFrame* f, int32_t mapping, float near, float far,
                            const float* state, const float* dL_ddist, void* acc_ws, size_t acc_ws_bytes,
                            const GsrAuxGrads* g, void* stream) {
  if (int rc = refuse_backward(p, f)) return rc;
  if (int rc = validate_distortion_mapping(mapping, near, far)) return rc;
  if (int rc = validate_aux_inputs(p)) return rc;
  if (int rc = refuse_mismatch(p, f)) return rc;
  if (!g) return fail(GSR_E_BADARG, "grads is NULL");
  if (p->P == 0) return 0;
  // a short workspace is GSR_E_BADARG here, GSR_E_CAPACITY in the other backwards: callers have seen both
  if (int rc = refuse_geom_outputs(p, f, state && dL_ddist, acc_ws, acc_ws_bytes, g, GSR_E_BADARG)) return rc;
  float* acc = static_cast<float*>(acc_ws);
  hipStream_t s = static_cast<hipStream_t>(stream);
  return run_geom_backward(p, f, acc, g, s, "distortion_bwd", [&](const MapFrame& mf) {
    launch_distortion_bwd(mf, mapping, near, far, state, dL_ddist, acc, s);
  });
}

// ---- median-depth map and Gaussian id map (csrc/median.hip) ----------------------------------------------------------
size_t gsr_median_depth_backward_bytes(int32_t P) { return align_up(4 * (size_t)(P > 0 ? P : 1), 256); }

int gsr_median_depth_forward(const GsrAuxFrame* f, float* median, int32_t* median_id, uint32_t* state, void* stream) {
  if (int rc = validate_aux_frame(f)) return rc;
  if (!median || !median_id || !state) return fail(GSR_E_BADARG, "median / median_id / state is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (frame_is_empty(f)) {
    const size_t hw = (size_t)f->width * f->height;
    GSR_HIP(hipMemsetAsync(median, 0, 4 * hw, s));
    GSR_HIP(hipMemsetAsync(median_id, 0xff, 4 * hw, s));      // -1
    GSR_HIP(hipMemsetAsync(state, 0xff, 4 * hw, s));          // no entry
    return 0;
  }
  launch_median_depth_fwd(map_frame(f), median, median_id, state, s);
  return check(nullptr, s, "median_depth_fwd");
}

int gsr_median_depth_backward(const GsrParams* p, const GsrAuxFrame* f, const uint32_t* state, const float* dL_dmedian,
                              void* acc_ws, size_t acc_ws_bytes, float* dL_dmeans3D, void* stream) {
  if (int rc = refuse_backward(p, f)) return rc;
  if (int rc = refuse_mismatch(p, f)) return rc;
  if (p->P == 0) return 0;
  if (!p->viewmatrix) return fail(GSR_E_BADARG, "viewmatrix must be non-NULL");
  if (!state || !dL_dmedian || !acc_ws || !dL_dmeans3D) return fail(GSR_E_BADARG, "NULL workspace / input / output");
  if (int rc = refuse_acc_ws(acc_ws, acc_ws_bytes, gsr_median_depth_backward_bytes(p->P), GSR_E_CAPACITY)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* acc = static_cast<float*>(acc_ws);
  GSR_HIP(hipMemsetAsync(acc, 0, 4 * (size_t)p->P, s));
  if (f->num_rendered > 0) {
    launch_median_depth_bwd(map_frame(f), state, dL_dmedian, acc, s);
    if (int rc = check(p, s, "median_depth_bwd")) return rc;
  }
  launch_median_depth_finish(p->P, p->viewmatrix, acc, dL_dmeans3D, s);
  return check(p, s, "median_depth_finish");
}

// ---- per-Gaussian contribution statistics (csrc/contribution.hip) --------------------------------------------------
int gsr_contribution_accumulate(const GsrAuxFrame* f, const uint8_t* pixel_mask, int64_t* stats, void* stream) {
  if (int rc = validate_aux_frame(f)) return rc;
  if (frame_is_empty(f)) return 0;
  if (!stats) return fail(GSR_E_BADARG, "stats is NULL");
  if (((uintptr_t)stats & 7u) != 0) return fail(GSR_E_ALIGN, "stats must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_contribution(map_frame(f), pixel_mask, stats, s);
  return check(nullptr, s, "contribution");
}

int gsr_profile_create(void** handle) {
  if (!handle) return fail(GSR_E_BADARG, "handle is NULL");
  *handle = new Profile();
  return 0;
}
int gsr_profile_destroy(void* handle) {
  Profile* pr = static_cast<Profile*>(handle);
  if (!pr) return 0;
  for (auto& sp : pr->used) { if (sp.a) (void)hipEventDestroy(sp.a); if (sp.b) (void)hipEventDestroy(sp.b); }
  for (auto e : pr->pool) (void)hipEventDestroy(e);
  delete pr;
  return 0;
}
int gsr_profile_collect(void* handle, double* ms_sum, uint32_t* counts) {
  Profile* pr = static_cast<Profile*>(handle);
  if (!pr || !ms_sum || !counts) return fail(GSR_E_BADARG, "NULL argument");
  std::vector<Profile::Span> spans;
  {
    std::lock_guard<std::mutex> lock(pr->mu);
    spans.swap(pr->used);
  }
  hipError_t err = hipSuccess;
  for (auto& sp : spans) {
    if (sp.a && sp.b && err == hipSuccess) {
      err = hipEventSynchronize(sp.b);
      float ms = 0.f;
      if (err == hipSuccess) err = hipEventElapsedTime(&ms, sp.a, sp.b);
      if (err == hipSuccess && sp.stage >= 0 && sp.stage < GSR_STAGE_COUNT) { ms_sum[sp.stage] += ms; counts[sp.stage] += 1; }
    }
    std::lock_guard<std::mutex> lock(pr->mu);     // the events go back to the pool on every path
    if (sp.a) pr->pool.push_back(sp.a);
    if (sp.b) pr->pool.push_back(sp.b);
  }
  if (err != hipSuccess) return hip_fail(err, "gsr_profile_collect");
  return 0;
}
const char* gsr_stage_name(int32_t stage) {
  return (stage >= 0 && stage < GSR_STAGE_COUNT) ? kStageNames[stage] : "?";
}

// Re-runs the forward compositing with work counters (debug / tuning only):
// stats[0] instances in all tile lists, [1] instances staged into LDS, [2] instances visited after the
// sub-block cull, [3] sub-block evaluations, [4] evaluations with >= 1 contributing lane, [5] sum of tile_max.
int gsr_debug_render_stats(const GsrParams* p, const void* geom_ws, const void* bin_ws, void* img_ws, uint32_t R,
                           uint32_t V, float* out_color, unsigned long long* stats /* device [8], zeroed by caller */,
                           void* stream) {
  if (int rc = validate(p)) return rc;
  if (!geom_ws || !bin_ws || !img_ws || !out_color || !stats || R == 0) return fail(GSR_E_BADARG, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const ImageLayout I(p->width, p->height);
  const GeomLayout L(p->P);
  const SortedViews sv = sorted_views(bin_ws, R, V, p->width, p->height, p->binning_mode);
  launch_render_fwd(p->width, p->height, at<uint2>(img_ws, I.ranges), sv.point_list,
                    at<GeomRec>(geom_ws, L.rec), p->bg, out_color, at<float>(img_ws, I.final_T),
                    at<uint32_t>(img_ws, I.n_contrib), at<uint32_t>(img_ws, I.tile_max),
                    at<uint32_t>(img_ws, I.tile_order), s, stats,
                    (p->debug_flags & GSR_DEBUG_NO_MINIBLOCK_CULL) ? 0 : 1, sv.inst_mask);
  return check(p, s, "render_stats");
}

int gsr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, uint8_t* visible, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (P == 0) return 0;
  if (!means3D || !viewmatrix || !visible) return fail(GSR_E_BADARG, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mark_visible(P, means3D, viewmatrix, visible, s);
  return check(nullptr, s, "mark_visible");
}

int gsr_sort_pairs_u64(uint64_t* keys, uint32_t* vals, uint64_t* keys_tmp, uint32_t* vals_tmp, uint32_t n,
                       int32_t end_bit, void* scratch, void* stream, int32_t* result_in_tmp) {
  if (!result_in_tmp) return fail(GSR_E_BADARG, "result_in_tmp is NULL");
  *result_in_tmp = 0;
  if (n == 0) return 0;
  if (!keys || !vals || !keys_tmp || !vals_tmp || !scratch) return fail(GSR_E_BADARG, "NULL buffer");
  if (end_bit < 0 || end_bit > 64) return fail(GSR_E_BADARG, "end_bit out of range");
  hipStream_t s = static_cast<hipStream_t>(stream);
  *result_in_tmp = launch_sort_pairs(keys, vals, keys_tmp, vals_tmp, n, end_bit, scratch, s) ? 1 : 0;
  return check(nullptr, s, "sort_pairs");
}

int gsr_sort_pairs_u32(uint32_t* keys, void* vals, uint32_t* keys_tmp, void* vals_tmp, uint32_t capacity,
                       const uint32_t* n_dev, int32_t end_bit, int32_t val_words, void* scratch, void* stream,
                       int32_t* result_in_tmp) {
  if (!result_in_tmp) return fail(GSR_E_BADARG, "result_in_tmp is NULL");
  *result_in_tmp = 0;
  if (val_words != 1 && val_words != 2) return fail(GSR_E_BADARG, "val_words must be 1 or 2");
  if (end_bit < 0 || end_bit > 32) return fail(GSR_E_BADARG, "end_bit out of range");
  if (capacity == 0) return 0;
  if (!keys || !vals || !keys_tmp || !vals_tmp || !scratch) return fail(GSR_E_BADARG, "NULL buffer");
  if (val_words == 2 && ((((uintptr_t)vals) | ((uintptr_t)vals_tmp)) & 7u) != 0)
    return fail(GSR_E_ALIGN, "two-word values must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool in_tmp =
      val_words == 1
          ? launch_sort_pairs_u32(keys, static_cast<uint32_t*>(vals), keys_tmp, static_cast<uint32_t*>(vals_tmp), capacity,
                                  end_bit, scratch, s, n_dev)
          : launch_sort_pairs_u32_v64(keys, static_cast<uint2*>(vals), keys_tmp, static_cast<uint2*>(vals_tmp), capacity,
                                      end_bit, scratch, s, n_dev);
  *result_in_tmp = in_tmp ? 1 : 0;
  return check(nullptr, s, "sort_pairs_u32");
}

int gsr_sort_extra_pass_u32(const uint32_t* keys_in, const void* vals_in, uint32_t* keys_out, void* vals_out,
                            uint32_t capacity, const uint32_t* n_dev, int32_t shift, int32_t nbits, void* scratch,
                            void* stream) {
  if (nbits < 1 || nbits > 8 || shift < 0 || shift + nbits > 32) return fail(GSR_E_BADARG, "shift / nbits out of range");
  if (capacity == 0) return 0;
  if (!keys_in || !vals_in || !keys_out || !vals_out || !scratch) return fail(GSR_E_BADARG, "NULL buffer");
  if (((((uintptr_t)vals_in) | ((uintptr_t)vals_out)) & 7u) != 0)
    return fail(GSR_E_ALIGN, "two-word values must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_sort_extra_pass_u32(keys_in, static_cast<const uint2*>(vals_in), keys_out, static_cast<uint2*>(vals_out), capacity,
                             n_dev, shift, nbits, scratch, s);
  return check(nullptr, s, "sort_extra_pass_u32");
}

int gsr_sort_tile_runs_u32(uint32_t* keys, uint32_t* vals, uint32_t* keys_tmp, uint32_t* vals_tmp, uint32_t capacity,
                           const uint32_t* n_dev, int32_t end_bit, uint32_t n_keys, void* ranges, uint32_t* order,
                           void* scratch, void* stream, int32_t* result_in_tmp, int32_t* runs_valid) {
  if (!result_in_tmp || !runs_valid) return fail(GSR_E_BADARG, "result_in_tmp / runs_valid is NULL");
  *result_in_tmp = 0;
  *runs_valid = 0;
  if (end_bit < 1 || end_bit > 32) return fail(GSR_E_BADARG, "end_bit out of range");
  // every key value needs a digit row in the last pass and a slot in ranges / order
  if (n_keys == 0 || n_keys > 0x7fffffffu || (end_bit < 32 && n_keys > (1u << end_bit)))
    return fail(GSR_E_BADARG, "n_keys does not fit end_bit");
  if (capacity == 0) return 0;
  if (!keys || !vals || !keys_tmp || !vals_tmp || !scratch || !ranges || !order) return fail(GSR_E_BADARG, "NULL buffer");
  if (((uintptr_t)ranges & 15u) != 0) return fail(GSR_E_ALIGN, "ranges must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  SortedRuns runs;
  runs.valid = false;
  runs.fused = false;
  runs.runs_rel = static_cast<uint2*>(ranges);
  runs.n_keys = n_keys;
  runs.order = nullptr;      // the raw entry keeps the stand-alone ranges-and-order kernel behind the sort
  *result_in_tmp = launch_sort_pairs_u32(keys, vals, keys_tmp, vals_tmp, capacity, end_bit, scratch, s, n_dev, &runs) ? 1 : 0;
  if (int rc = check(nullptr, s, "tile_sort")) return rc;
  *runs_valid = runs.valid ? 1 : 0;
  if (runs.valid) launch_ranges_and_order_from_sort((int)n_keys, runs, static_cast<uint2*>(ranges), order, s);
  return check(nullptr, s, "ranges_and_order_from_sort");
}

int gsr_debug_read_geom(const void* geom_ws, int32_t P, float* xy, float* conic_opacity, float* rgb, float* depth,
                        uint32_t* tiles_touched, uint32_t* point_offsets, uint32_t* rect, uint32_t* clamped,
                        void* stream) {
  if (!geom_ws || P < 0) return fail(GSR_E_BADARG, "bad geom_ws / P");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GeomLayout L(P);
  launch_unpack_geom(P, at<GeomRec>(geom_ws, L.rec), at<BinInfo>(geom_ws, L.bin), at<uint32_t>(geom_ws, L.block_offs), xy,
                     conic_opacity, rgb, depth, tiles_touched, point_offsets, rect, clamped, s);
  return check(nullptr, s, "unpack_geom");
}

int gsr_debug_read_binning(const void* geom_ws, int32_t P, const void* bin_ws, uint32_t R, uint32_t V, int32_t width,
                           int32_t height, int32_t mode, uint64_t* keys_sorted, uint32_t* point_list, void* stream) {
  if (R == 0) return 0;
  if (!bin_ws || !geom_ws) return fail(GSR_E_BADARG, "bin_ws / geom_ws is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const SortedViews v = sorted_views(bin_ws, R, V, width, height, mode);
  if (keys_sorted) {
    if (mode == GSR_BINNING_KEYS64) {
      GSR_HIP(hipMemcpyAsync(keys_sorted, v.keys_sorted, 8 * (size_t)R, hipMemcpyDeviceToDevice, s));
    } else {
      const GeomLayout L(P);
      launch_reconstruct_keys(R, (uint32_t)P, v.tile_sorted, v.point_list, at<BinInfo>(geom_ws, L.bin), keys_sorted, s);
    }
  }
  if (point_list) GSR_HIP(hipMemcpyAsync(point_list, v.point_list, 4 * (size_t)R, hipMemcpyDeviceToDevice, s));
  return check(nullptr, s, "read_binning");
}

int gsr_debug_read_counts(const void* geom_ws, int32_t P, uint32_t out_host[8], void* stream) {
  if (!geom_ws || !out_host || P < 0) return fail(GSR_E_BADARG, "bad geom_ws / out / P");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GeomLayout L(P);
  GSR_HIP(hipMemcpyAsync(out_host, at<uint32_t>(geom_ws, L.total), 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  GSR_HIP(hipStreamSynchronize(s));
  return 0;
}

int gsr_debug_read_image(const void* img_ws, int32_t width, int32_t height, float* final_T, uint32_t* n_contrib,
                         uint32_t* ranges, void* stream) {
  if (!img_ws) return fail(GSR_E_BADARG, "img_ws is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const ImageLayout I(width, height);
  const size_t px = (size_t)width * height;
  if (final_T) GSR_HIP(hipMemcpyAsync(final_T, at<float>(img_ws, I.final_T), 4 * px, hipMemcpyDeviceToDevice, s));
  if (n_contrib) GSR_HIP(hipMemcpyAsync(n_contrib, at<uint32_t>(img_ws, I.n_contrib), 4 * px, hipMemcpyDeviceToDevice, s));
  if (ranges) GSR_HIP(hipMemcpyAsync(ranges, at<uint32_t>(img_ws, I.ranges), 8 * (size_t)I.tiles, hipMemcpyDeviceToDevice, s));
  return 0;
}

size_t gsr_l1_loss_workspace_bytes(void) { return l1_loss_workspace_bytes(); }
int gsr_l1_loss_fwd_bwd(const float* x, const float* gt, size_t n, float scale, float* loss_sum, float* dL_dx,
                        void* workspace, void* stream) {
  if (!x || !gt || !loss_sum || !workspace) return fail(GSR_E_BADARG, "NULL input");
  if ((((uintptr_t)x | (uintptr_t)gt | (uintptr_t)dL_dx) & 15u) != 0) return fail(GSR_E_ALIGN, "16-byte alignment required");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_l1_loss(x, gt, n, scale, loss_sum, dL_dx, static_cast<float*>(workspace), s);
  return check(nullptr, s, "l1_loss");
}

size_t gsr_l1_dssim_workspace_bytes(int32_t C, int32_t H, int32_t W) {
  if (C <= 0 || H <= 0 || W <= 0) return 0;
  const size_t blocks = (size_t)((W + 15) / 16) * (size_t)((H + 15) / 16) * (size_t)C;      // 16x16 output tiles
  return sizeof(float) * (3 * (size_t)C * (size_t)H * (size_t)W + 2 * blocks);
}
int gsr_l1_dssim_loss_fwd_bwd(const float* x, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                              int32_t dssim_mode, float* sums, float* dL_dx, void* workspace, void* stream) {
  if (!x || !gt || !sums || !dL_dx || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  if (C <= 0 || H <= 0 || W <= 0 || C > 65535) return fail(GSR_E_BADARG, "bad image shape");
  if (dssim_mode != GSR_DSSIM_ONE_MINUS_MEAN && dssim_mode != GSR_DSSIM_CLAMPED_HALF)
    return fail(GSR_E_BADARG, "unknown dssim_mode");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_l1_dssim(x, gt, C, H, W, lambda_dssim, dssim_mode, sums, dL_dx, static_cast<float*>(workspace), s);
  return check(nullptr, s, "l1_dssim");
}

static const int32_t kEvalFlags = GSR_EVAL_CLAMP_X | GSR_EVAL_CLAMP_GT | GSR_EVAL_SSIM | GSR_EVAL_PSNR_WHOLE |
                                  GSR_EVAL_U8_TRUNCATE;
size_t gsr_eval_workspace_bytes(int32_t C, int32_t H, int32_t W, int32_t flags) {
  if (C != 3 || H <= 0 || W <= 0 || (flags & ~kEvalFlags)) return 0;
  return sizeof(float) * (6 * (size_t)EVAL_MAX_BLOCKS + ((flags & GSR_EVAL_SSIM) ? eval_ssim_blocks(H, W) : 0));
}
int gsr_eval_image(const float* x, const float* gt, int32_t C, int32_t H, int32_t W, int32_t flags, float* view_out,
                   double* acc, uint8_t* u8_out, void* workspace, void* stream) {
  if (!x || !gt) return fail(GSR_E_BADARG, "NULL image");
  if (!workspace) return fail(GSR_E_BADARG, "NULL workspace");
  if (!view_out && !acc && !u8_out) return fail(GSR_E_BADARG, "no output: view_out, acc and u8_out are all NULL");
  if (H <= 0 || W <= 0) return fail(GSR_E_BADARG, "bad image shape");
  if (C != 3) return fail(GSR_E_BADARG, "evaluation needs a 3-channel image");
  if (flags & ~kEvalFlags) return fail(GSR_E_BADARG, "unknown evaluation flag bits");
  if ((((uintptr_t)x | (uintptr_t)gt | (uintptr_t)view_out | (uintptr_t)workspace) & 3u) != 0 || ((uintptr_t)acc & 7u) != 0)
    return fail(GSR_E_ALIGN, "images, view_out and workspace must be 4-byte aligned, acc 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_eval_image(x, gt, H, W, flags, view_out, acc, u8_out, static_cast<float*>(workspace), s);
  return check(nullptr, s, "eval_image");
}
int gsr_image_to_u8(const float* x, int32_t C, int32_t H, int32_t W, int32_t flags, uint8_t* u8_out, void* stream) {
  if (!x || !u8_out) return fail(GSR_E_BADARG, "NULL image");
  if (H <= 0 || W <= 0) return fail(GSR_E_BADARG, "bad image shape");
  if (C != 3) return fail(GSR_E_BADARG, "the 8-bit output needs a 3-channel image");
  if (flags & ~GSR_EVAL_U8_TRUNCATE) return fail(GSR_E_BADARG, "unknown conversion flag bits");
  if (((uintptr_t)x & 3u) != 0) return fail(GSR_E_ALIGN, "image must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_eval_image(x, nullptr, H, W, flags, nullptr, nullptr, u8_out, nullptr, s);
  return check(nullptr, s, "image_to_u8");
}

size_t gsr_splat2d_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  return (N < 0 || H <= 0 || W <= 0) ? 0 : Splat2dLayout(N, H, W).bytes;
}
static int splat2d_validate(int32_t N, int32_t K, int32_t H, int32_t W, const void* ws, size_t ws_bytes) {
  if (N < 0 || H <= 0 || W <= 0 || K <= 0) return fail(GSR_E_BADARG, "bad N / K / image size");
  if (K > H || K > W) return fail(GSR_E_BADARG, "Kernel size should be smaller or equal to the image size.");
  if (K > splat2d_max_kernel_size()) return fail(GSR_E_BADARG, "kernel size above 2048");
  if (!ws) return fail(GSR_E_BADARG, "NULL workspace");
  if (((uintptr_t)ws & 255u) != 0) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  if (ws_bytes < Splat2dLayout(N, H, W).bytes) return fail(GSR_E_CAPACITY, "splat2d workspace too small");
  return 0;
}
int gsr_splat2d_forward(int32_t N, int32_t K, int32_t H, int32_t W, const float* sigma_x, const float* sigma_y,
                        const float* rho, const float* coords, const float* colours, const float* ax, void* workspace,
                        size_t workspace_bytes, float* out, int32_t* not_pd_host, void* stream) {
  if (int rc = splat2d_validate(N, K, H, W, workspace, workspace_bytes)) return rc;
  if (!out || !ax) return fail(GSR_E_BADARG, "NULL argument");
  if (N > 0 && (!sigma_x || !sigma_y || !rho || !coords || !colours)) return fail(GSR_E_BADARG, "NULL input");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_splat2d_fwd(N, K, H, W, sigma_x, sigma_y, rho, coords, colours, ax, workspace, out, s);
  if (int rc = check(nullptr, s, "splat2d_forward")) return rc;
  if (not_pd_host) {
    int flag = 0;
    GSR_HIP(hipMemcpyAsync(&flag, static_cast<char*>(workspace) + Splat2dLayout(N, H, W).flag, 4, hipMemcpyDeviceToHost, s));
    GSR_HIP(hipStreamSynchronize(s));
    *not_pd_host = flag;
  }
  return 0;
}
int gsr_splat2d_backward(int32_t N, int32_t K, int32_t H, int32_t W, const float* sigma_x, const float* sigma_y,
                         const float* rho, const float* ax, void* workspace, size_t workspace_bytes,
                         const float* dL_dout, float* dL_dsigma_x, float* dL_dsigma_y, float* dL_drho,
                         float* dL_dcoords, float* dL_dcolours, void* stream) {
  if (int rc = splat2d_validate(N, K, H, W, workspace, workspace_bytes)) return rc;
  if (!dL_dout || !ax) return fail(GSR_E_BADARG, "NULL argument");
  if (N > 0 && (!sigma_x || !sigma_y || !rho || !dL_dsigma_x || !dL_dsigma_y || !dL_drho || !dL_dcoords || !dL_dcolours))
    return fail(GSR_E_BADARG, "NULL input / gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_splat2d_bwd(N, K, H, W, sigma_x, sigma_y, rho, ax, workspace, dL_dout, dL_dsigma_x, dL_dsigma_y, dL_drho,
                     dL_dcoords, dL_dcolours, s);
  return check(nullptr, s, "splat2d_backward");
}

size_t gsr_knn3_workspace_bytes(int32_t N) { return knn_workspace_bytes(N); }
int gsr_dist2_knn3(const float* points, int32_t N, float* mean_dist2, void* workspace, size_t workspace_bytes,
                   void* stream) {
  if (N < 0) return fail(GSR_E_BADARG, "N < 0");
  if (N == 0) return 0;
  if (!points || !mean_dist2 || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  if (workspace_bytes < knn_workspace_bytes(N)) return fail(GSR_E_CAPACITY, "knn workspace too small");
  if (((uintptr_t)workspace & 255u) != 0) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_knn3(points, N, mean_dist2, workspace, s);
  return check(nullptr, s, "knn3");
}

// ---- cross-set nearest point (csrc/nearest.hip) ------------------------------------------------------------------------
size_t gsr_nn_index_bytes(int32_t R) { return nn_index_bytes(R); }
size_t gsr_nn_query_workspace_bytes(int32_t Q) { return nn_query_workspace_bytes(Q); }
int gsr_nn_build(const float* ref, int32_t R, void* index, size_t index_bytes, void* stream) {
  if (R < 0 || R > GSR_NN_MAX_POINTS) return fail(GSR_E_BADARG, "R must lie in 0..2^31-256");
  if (R == 0) return 0;
  if (!ref || !index) return fail(GSR_E_BADARG, "NULL argument");
  if (index_bytes < nn_index_bytes(R)) return fail(GSR_E_CAPACITY, "nn index too small");
  if (((uintptr_t)index & 255u) != 0) return fail(GSR_E_ALIGN, "index must be 256-byte aligned");
  if (((uintptr_t)ref & 3u) != 0) return fail(GSR_E_ALIGN, "ref must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_nn_build(ref, R, index, s);
  return check(nullptr, s, "nn_build");
}
int gsr_nn_query(const void* index, size_t index_bytes, int32_t R, const float* query, int32_t Q, float* dist2,
                 int32_t* nearest, void* workspace, size_t workspace_bytes, void* stream) {
  if (R < 0 || Q < 0 || R > GSR_NN_MAX_POINTS || Q > GSR_NN_MAX_POINTS)
    return fail(GSR_E_BADARG, "R and Q must lie in 0..2^31-256");
  if (Q == 0) return 0;
  if (!query || !dist2 || !nearest) return fail(GSR_E_BADARG, "NULL argument");
  if ((((uintptr_t)query | (uintptr_t)dist2 | (uintptr_t)nearest) & 3u) != 0)
    return fail(GSR_E_ALIGN, "query / dist2 / nearest must be 4-byte aligned");
  if (R > 0) {
    if (!index || !workspace) return fail(GSR_E_BADARG, "NULL index / workspace");
    if (index_bytes < nn_index_bytes(R)) return fail(GSR_E_CAPACITY, "nn index too small");
    if (workspace_bytes < nn_query_workspace_bytes(Q)) return fail(GSR_E_CAPACITY, "nn query workspace too small");
    if ((((uintptr_t)index | (uintptr_t)workspace) & 255u) != 0)
      return fail(GSR_E_ALIGN, "index / workspace must be 256-byte aligned");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_nn_query(index, R, query, Q, dist2, nearest, workspace, s);
  return check(nullptr, s, "nn_query");
}

int gsr_densify_stats(int32_t P, const float* dL_dmeans2D, const int32_t* radii, float* xyz_gradient_accum, float* denom,
                      float* max_radii2D, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (P == 0) return 0;
  if (!dL_dmeans2D || !radii || !xyz_gradient_accum || !denom || !max_radii2D) return fail(GSR_E_BADARG, "NULL input");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_stats(P, dL_dmeans2D, radii, xyz_gradient_accum, denom, max_radii2D, s);
  return check(nullptr, s, "densify_stats");
}

size_t gsr_densify_workspace_bytes(int32_t P) { return P < 0 ? 0 : DensifyLayout(P).bytes; }
int gsr_densify_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                     const float* opacity_raw, float grad_threshold, float percent_dense_extent, float min_opacity,
                     float max_world_scale, void* workspace, size_t workspace_bytes, uint32_t counts_host[4],
                     void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (!counts_host) return fail(GSR_E_BADARG, "NULL counts_host");
  counts_host[0] = counts_host[1] = counts_host[2] = counts_host[3] = 0;
  if (P == 0) return 0;
  if (!xyz_gradient_accum || !denom || !scaling_raw || !opacity_raw || !workspace) return fail(GSR_E_BADARG, "NULL input");
  if (((uintptr_t)workspace & 255u) != 0) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  const DensifyLayout L(P);
  if (workspace_bytes < L.bytes) return fail(GSR_E_CAPACITY, "densify workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_plan(P, xyz_gradient_accum, denom, scaling_raw, opacity_raw, grad_threshold, percent_dense_extent,
                      min_opacity, max_world_scale, max_world_scale >= 0.0f ? 1 : 0, workspace, s);
  if (int rc = check(nullptr, s, "densify_plan")) return rc;
  GSR_HIP(hipMemcpyAsync(counts_host, static_cast<char*>(workspace) + L.totals, 16, hipMemcpyDeviceToHost, s));
  GSR_HIP(hipStreamSynchronize(s));
  return 0;
}
int gsr_densify_gather_rows(int32_t P, int32_t row_floats, const float* src, const void* workspace,
                            const uint32_t counts[4], int32_t zero_new, float* dst, void* stream) {
  if (P < 0 || row_floats <= 0) return fail(GSR_E_BADARG, "bad P / row_floats");
  if (P == 0) return 0;
  if (!src || !workspace || !counts) return fail(GSR_E_BADARG, "NULL argument");
  if (!dst && counts[0] + counts[1] + counts[2] > 0) return fail(GSR_E_BADARG, "NULL dst");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_gather_rows(P, row_floats, src, workspace, counts, zero_new, dst, s);
  return check(nullptr, s, "densify_gather_rows");
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
  return check(nullptr, s, "densify_split_children");
}

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
  if (((uintptr_t)workspace & 255u) != 0) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  const DensifyForkLayout L(P);
  if (workspace_bytes < L.bytes) return fail(GSR_E_CAPACITY, "densify_fork workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_densify_fork_plan(P, xyz_gradient_accum, denom, scaling_raw, opacity_raw, split_scale_raw, grad_threshold,
                           percent_dense_extent, min_opacity, max_world_scale, max_world_scale >= 0.0f ? 1 : 0,
                           workspace, s);
  if (int rc = check(nullptr, s, "densify_fork_plan")) return rc;
  GSR_HIP(hipMemcpyAsync(counts_host, static_cast<char*>(workspace) + L.totals, 20, hipMemcpyDeviceToHost, s));
  GSR_HIP(hipStreamSynchronize(s));
  return 0;
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
  launch_densify_fork_gather_rows(P, row_floats, src, workspace, counts, grow_branch ? 4 : 2, policy, value, dst, s);
  return check(nullptr, s, "densify_fork_gather_rows");
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
  return check(nullptr, s, "densify_fork_rows");
}

size_t gsr_grow_workspace_bytes(int32_t P) { return P < 0 ? 0 : GrowLayout(P).bytes; }
int gsr_grow_plan(int32_t P, const float* xyz_gradient_accum, const float* denom, const float* scaling_raw,
                  float grad_threshold, float percent_dense_extent, int32_t mode, void* workspace, size_t workspace_bytes,
                  int32_t* vidx, int32_t* src, uint8_t* selected, uint32_t counts_host[2], void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "P < 0");
  if (!counts_host) return fail(GSR_E_BADARG, "NULL counts_host");
  counts_host[0] = counts_host[1] = 0;
  if (P == 0) return 0;
  if (!xyz_gradient_accum || !denom || !scaling_raw || !workspace || !vidx || !src || !selected)
    return fail(GSR_E_BADARG, "NULL argument");
  if (((uintptr_t)workspace & 255u) != 0) return fail(GSR_E_ALIGN, "workspace must be 256-byte aligned");
  const GrowLayout L(P);
  if (workspace_bytes < L.bytes) return fail(GSR_E_CAPACITY, "grow workspace too small");
  const int grow = (mode & (GSR_GROW_DIR | GSR_GROW_CONTINUOUS)) != 0;
  if (!grow && !(mode & (GSR_SPLIT_DISTANCE | GSR_SPLIT_SCALE))) return fail(GSR_E_BADARG, "mode selects no branch");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_grow_plan(P, xyz_gradient_accum, denom, scaling_raw, grad_threshold, percent_dense_extent, grow ? 0 : 1,
                   workspace, vidx, src, selected, s);
  if (int rc = check(nullptr, s, "grow_plan")) return rc;
  GSR_HIP(hipMemcpyAsync(counts_host, static_cast<char*>(workspace) + L.totals, 8, hipMemcpyDeviceToHost, s));
  GSR_HIP(hipStreamSynchronize(s));
  return 0;
}

static int grow_validate(const GsrGrow* g) {
  if (!g) return fail(GSR_E_BADARG, "NULL GsrGrow");
  if (g->P < 0 || g->G < 0 || g->G > g->P) return fail(GSR_E_BADARG, "bad P / G");
  if (g->n_rest != 0 && g->n_rest != 45) return fail(GSR_E_BADARG, "n_rest must be 0 or 45");
  if (g->P > 0 && (!g->xyz || !g->f_dc || !g->opacity || !g->scaling || !g->rotation || (g->n_rest && !g->f_rest)))
    return fail(GSR_E_BADARG, "NULL model tensor");
  const int grow = (g->mode & (GSR_GROW_DIR | GSR_GROW_CONTINUOUS)) != 0;
  if ((g->mode & GSR_GROW_DIR) && (g->mode & GSR_GROW_CONTINUOUS))
    return fail(GSR_E_BADARG, "GSR_GROW_DIR and GSR_GROW_CONTINUOUS are exclusive");
  if (!grow && !(g->mode & (GSR_SPLIT_DISTANCE | GSR_SPLIT_SCALE))) return fail(GSR_E_BADARG, "mode selects no branch");
  if (g->P == 0) return 0;
  if (!g->vidx || (g->G > 0 && !g->src)) return fail(GSR_E_BADARG, "NULL vidx / src");
  if ((g->mode & GSR_GROW_DIR) && (!g->dirs_prob || !g->dirs || g->num_dirs <= 0))
    return fail(GSR_E_BADARG, "GSR_GROW_DIR needs dirs_prob, dirs and num_dirs > 0");
  if ((g->mode & GSR_GROW_CONTINUOUS) && !g->conti_dirs) return fail(GSR_E_BADARG, "NULL conti_dirs");
  if (grow && (g->mode & GSR_GROW_DISTANCE) && !g->grow_dist) return fail(GSR_E_BADARG, "NULL grow_dist");
  if (!grow && (g->mode & GSR_SPLIT_DISTANCE) && !g->split_distance) return fail(GSR_E_BADARG, "NULL split_distance");
  if (!grow && (g->mode & GSR_SPLIT_SCALE) && !g->split_scale) return fail(GSR_E_BADARG, "NULL split_scale");
  if (!grow && !(g->mode & GSR_SPLIT_DISTANCE) && g->G > 0 && !g->noise) return fail(GSR_E_BADARG, "NULL noise");
  return 0;
}

int gsr_grow_expand(const GsrGrow* g, float* xyz_out, float* f_dc_out, float* f_rest_out, float* opacity_out,
                    float* scaling_out, float* rotation_out, void* stream) {
  if (int rc = grow_validate(g)) return rc;
  if (g->P == 0) return 0;
  if (!xyz_out || !f_dc_out || !opacity_out || !scaling_out || !rotation_out || (g->n_rest && !f_rest_out))
    return fail(GSR_E_BADARG, "NULL output");
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* const out[6] = {xyz_out, f_dc_out, f_rest_out, opacity_out, scaling_out, rotation_out};
  launch_grow_expand(*g, out, s);
  return check(nullptr, s, "grow_expand");
}

int gsr_grow_fold(const GsrGrow* g, const GsrGrowGrads* grads, void* stream) {
  if (int rc = grow_validate(g)) return rc;
  if (!grads) return fail(GSR_E_BADARG, "NULL grads");
  if (g->P == 0) return 0;
  for (int k = 0; k < 7; ++k) {
    if (k == 3 && !g->n_rest) continue;
    if (!grads->in[k] || !grads->out[k]) return fail(GSR_E_BADARG, "NULL gradient array");
  }
  const int grow = (g->mode & (GSR_GROW_DIR | GSR_GROW_CONTINUOUS)) != 0;
  if (((g->mode & GSR_GROW_DIR) && !grads->d_dirs_prob) || ((g->mode & GSR_GROW_CONTINUOUS) && !grads->d_conti_dirs) ||
      (grow && (g->mode & GSR_GROW_DISTANCE) && !grads->d_grow_dist) ||
      (!grow && (g->mode & GSR_SPLIT_DISTANCE) && !grads->d_split_distance) ||
      (!grow && (g->mode & GSR_SPLIT_SCALE) && !grads->d_split_scale))
    return fail(GSR_E_BADARG, "NULL gradient of a learned tensor of the mode");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_grow_fold(*g, *grads, s);
  return check(nullptr, s, "grow_fold");
}

int gsr_adam_step(const GsrAdamBatch* batch, void* stream) {
  if (!batch) return fail(GSR_E_BADARG, "NULL batch");
  if (batch->count < 0 || batch->count > GSR_ADAM_MAX_TENSORS)
    return fail(GSR_E_BADARG, "count must be 0..GSR_ADAM_MAX_TENSORS");
  for (int k = 0; k < batch->count; ++k) {
    const GsrAdamTensor& t = batch->t[k];
    if (t.numel < 0) return fail(GSR_E_BADARG, "negative numel");
    if (t.numel > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))
      return fail(GSR_E_BADARG, "NULL param / grad / exp_avg / exp_avg_sq");
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (launch_adam_step(*batch, s)) return fail(GSR_E_BADARG, "batch too large for one launch (more than 2^32 work-items)");
  return check(nullptr, s, "adam_step");
}

int gsr_adam_step_rows(const GsrAdamRowsBatch* batch, void* stream) {
  if (!batch) return fail(GSR_E_BADARG, "NULL batch");
  if (batch->count < 0 || batch->count > GSR_ADAM_MAX_TENSORS)
    return fail(GSR_E_BADARG, "count must be 0..GSR_ADAM_MAX_TENSORS");
  if (batch->visibility_kind != GSR_ADAM_VIS_U8 && batch->visibility_kind != GSR_ADAM_VIS_I32)
    return fail(GSR_E_BADARG, "unknown visibility_kind");
  if (batch->rows < 0) return fail(GSR_E_BADARG, "negative rows");
  for (int k = 0; k < batch->count; ++k) {
    const GsrAdamTensor& t = batch->t[k];
    if (t.numel < 0) return fail(GSR_E_BADARG, "negative numel");
    if (t.numel == 0) continue;
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)
      return fail(GSR_E_BADARG, "NULL param / grad / exp_avg / exp_avg_sq");
    if (!batch->visibility) return fail(GSR_E_BADARG, "NULL visibility with a non-empty tensor");
    if (batch->rows == 0 || t.numel % batch->rows != 0) return fail(GSR_E_BADARG, "numel is not a multiple of rows");
  }
  if (batch->visibility_kind == GSR_ADAM_VIS_I32 && ((uintptr_t)batch->visibility & 3u) != 0)
    return fail(GSR_E_ALIGN, "an int32 visibility must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (launch_adam_step_rows(*batch, s))
    return fail(GSR_E_BADARG, "batch too large for one launch (more than 2^32 work-items)");
  return check(nullptr, s, "adam_step_rows");
}

size_t gsr_opacity_sparsity_workspace_bytes(void) { return (size_t)OPACITY_MAX_BLOCKS * (sizeof(float) + sizeof(uint32_t)); }
int gsr_opacity_sparsity_fwd(const float* opacity_raw, int64_t P, float weight, float threshold, float* record,
                             void* workspace, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "negative P");
  if (!record || !workspace || (P > 0 && !opacity_raw)) return fail(GSR_E_BADARG, "NULL argument");
  if ((((uintptr_t)opacity_raw | (uintptr_t)workspace) & 3u) != 0 || ((uintptr_t)record & 15u) != 0)
    return fail(GSR_E_ALIGN, "opacity and workspace must be 4-byte aligned, the record 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_opacity_sparsity_fwd(opacity_raw, (size_t)P, weight, threshold, record, workspace, s);
  return check(nullptr, s, "opacity_sparsity_fwd");
}
int gsr_opacity_sparsity_bwd(const float* opacity_raw, int64_t P, float threshold, const float* record,
                             const float* grad_out, float* grad_raw, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "negative P");
  if (!record || !grad_out || (P > 0 && (!opacity_raw || !grad_raw))) return fail(GSR_E_BADARG, "NULL argument");
  if ((((uintptr_t)opacity_raw | (uintptr_t)grad_raw | (uintptr_t)record | (uintptr_t)grad_out) & 3u) != 0)
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_opacity_sparsity_bwd(opacity_raw, (size_t)P, threshold, record, grad_out, grad_raw, s);
  return check(nullptr, s, "opacity_sparsity_bwd");
}
int gsr_reset_opacity(float* opacity_raw, int64_t P, float cap, float* exp_avg, float* exp_avg_sq, void* stream) {
  if (P < 0) return fail(GSR_E_BADARG, "negative P");
  if (P > 0 && !opacity_raw) return fail(GSR_E_BADARG, "NULL opacity");
  if (!(cap > 0.0f && cap < 1.0f)) return fail(GSR_E_BADARG, "cap must lie in (0, 1)");
  if ((((uintptr_t)opacity_raw | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3u) != 0)
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_reset_opacity(opacity_raw, (size_t)P, cap, exp_avg, exp_avg_sq, s);
  return check(nullptr, s, "reset_opacity");
}

static int image_shape_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * (int64_t)W <= (int64_t)1 << 28; }
int gsr_image_composite_u8(const uint8_t* rgba, int32_t H, int32_t W, double bg_r, double bg_g, double bg_b,
                           uint8_t* rgb, void* stream) {
  if (!rgba || !rgb) return fail(GSR_E_BADARG, "NULL image");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  const double bg[3] = {bg_r, bg_g, bg_b};
  for (double b : bg)
    if (!(b >= 0.0 && b <= 1.0)) return fail(GSR_E_BADARG, "background must lie in [0, 1]");
  if (((uintptr_t)rgba & 3u) != 0) return fail(GSR_E_ALIGN, "the RGBA image must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_image_composite_u8(rgba, (size_t)H * (size_t)W, bg, rgb, s);
  return check(nullptr, s, "image_composite_u8");
}
int gsr_image_resize_u8(const uint8_t* src, int32_t C, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w,
                        const int32_t* h_bounds, const int32_t* h_taps, int32_t h_ksize, const int32_t* v_bounds,
                        const int32_t* v_taps, int32_t v_ksize, uint8_t* tmp, uint8_t* dst, void* stream) {
  if (!src || !dst) return fail(GSR_E_BADARG, "NULL image");
  if (C != 1 && C != 3) return fail(GSR_E_BADARG, "resize takes 1 or 3 channels");
  if (!image_shape_ok(in_h, in_w) || !image_shape_ok(out_h, out_w) || !image_shape_ok(in_h, out_w))
    return fail(GSR_E_BADARG, "bad image shape");
  const bool horiz = out_w != in_w, vert = out_h != in_h;
  if (horiz && (!h_bounds || !h_taps || h_ksize <= 0)) return fail(GSR_E_BADARG, "horizontal pass needs its tap table");
  if (vert && (!v_bounds || !v_taps || v_ksize <= 0)) return fail(GSR_E_BADARG, "vertical pass needs its tap table");
  if (horiz && vert && !tmp) return fail(GSR_E_BADARG, "two passes need the intermediate image");
  if ((((uintptr_t)h_bounds | (uintptr_t)h_taps | (uintptr_t)v_bounds | (uintptr_t)v_taps) & 3u) != 0)
    return fail(GSR_E_ALIGN, "tap tables must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!horiz && !vert) {
    GSR_HIP(hipMemcpyAsync(dst, src, (size_t)in_h * (size_t)in_w * (size_t)C, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  const uint8_t* mid = src;
  if (horiz) {
    uint8_t* out = vert ? tmp : dst;
    launch_image_resize_pass(false, C, src, in_w, out_w, in_h, h_bounds, h_taps, h_ksize, out, s);
    mid = out;
  }
  if (vert) launch_image_resize_pass(true, C, mid, in_h, out_h, out_w, v_bounds, v_taps, v_ksize, dst, s);
  return check(nullptr, s, "image_resize_u8");
}
int gsr_image_to_float_chw(const uint8_t* src, int32_t C, int32_t H, int32_t W, float* dst, void* stream) {
  if (!src || !dst) return fail(GSR_E_BADARG, "NULL image");
  if (C != 3 && C != 4) return fail(GSR_E_BADARG, "the float target needs a 3- or 4-channel image");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if (((uintptr_t)dst & 3u) != 0 || (C == 4 && ((uintptr_t)src & 3u) != 0))
    return fail(GSR_E_ALIGN, "the float image and a 4-channel source must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_image_to_float_chw(src, C, (size_t)H * (size_t)W, dst, s);
  return check(nullptr, s, "image_to_float_chw");
}

size_t gsr_exposure_workspace_bytes(int32_t H, int32_t W) {
  return image_shape_ok(H, W) ? exposure_workspace_bytes((size_t)H * (size_t)W) : 0;
}
int gsr_exposure_apply_fwd(const float* x, const float* A, int32_t H, int32_t W, float* y, void* stream) {
  if (!x || !A || !y) return fail(GSR_E_BADARG, "NULL argument");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if ((((uintptr_t)x | (uintptr_t)A | (uintptr_t)y) & 3u) != 0) return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_exposure_apply_fwd(x, A, (size_t)H * (size_t)W, y, s);
  return check(nullptr, s, "exposure_apply_fwd");
}
int gsr_exposure_apply_bwd(const float* x, const float* A, const float* g, int32_t H, int32_t W, float* dx, float* dA,
                           void* workspace, void* stream) {
  if (!g || (dx && !A) || (dA && (!x || !workspace))) return fail(GSR_E_BADARG, "NULL argument");
  if (!image_shape_ok(H, W)) return fail(GSR_E_BADARG, "bad image shape");
  if ((((uintptr_t)x | (uintptr_t)A | (uintptr_t)g | (uintptr_t)dx | (uintptr_t)dA) & 3u) != 0)
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (dA && ((uintptr_t)workspace & 7u) != 0) return fail(GSR_E_ALIGN, "the workspace must be 8-byte aligned");
  if (!dx && !dA) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_exposure_apply_bwd(x, A, g, (size_t)H * (size_t)W, dx, dA, workspace, s);
  return check(nullptr, s, "exposure_apply_bwd");
}

// ---- TSDF fusion and mesh extraction (csrc/tsdf.hip) ----------------------------------------------------------------
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
  if ((((uintptr_t)v->tsdf | (uintptr_t)v->weight | (uintptr_t)v->color) & 3u) != 0)
    return fail(GSR_E_ALIGN, "volume fields must be 4-byte aligned");
  return 0;
}
int gsr_tsdf_integrate(const GsrTsdfVolume* vol, const GsrTsdfView* view, void* stream) {
  if (int rc = tsdf_volume_ok(vol)) return rc;
  if (!view) return fail(GSR_E_BADARG, "view is NULL");
  if (!image_shape_ok(view->height, view->width)) return fail(GSR_E_BADARG, "bad image shape");
  if (!view->viewmatrix || !view->depth) return fail(GSR_E_BADARG, "viewmatrix / depth is NULL");
  if ((vol->color != nullptr) != (view->color != nullptr))
    return fail(GSR_E_BADARG, "a colour image is given exactly when the volume has a colour field");
  if (!(view->fx > 0.0f) || !(view->fy > 0.0f) || !(view->weight > 0.0f) || !(view->max_depth > 0.0f) ||
      !(view->max_weight > 0.0f))
    return fail(GSR_E_BADARG, "fx, fy, weight, max_depth and max_weight must be positive (+inf: no limit)");
  if ((((uintptr_t)view->viewmatrix | (uintptr_t)view->depth | (uintptr_t)view->color) & 3u) != 0)
    return fail(GSR_E_ALIGN, "view arrays must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_tsdf_integrate(*vol, *view, s);
  return check(nullptr, s, "tsdf_integrate");
}
int gsr_tsdf_mesh_count(const GsrTsdfVolume* vol, float min_weight, uint8_t* tri_count, uint8_t* edge_mask,
                        uint8_t* vert_count, void* stream) {
  if (int rc = tsdf_volume_ok(vol)) return rc;
  if (!tri_count || !edge_mask || !vert_count) return fail(GSR_E_BADARG, "NULL argument");
  if (min_weight != min_weight) return fail(GSR_E_BADARG, "min_weight is NaN");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_tsdf_mesh_count(*vol, min_weight, tri_count, edge_mask, vert_count, s);
  return check(nullptr, s, "tsdf_mesh_count");
}
int gsr_tsdf_mesh_emit(const GsrTsdfVolume* vol, const uint8_t* tri_count, const uint8_t* edge_mask,
                       const int64_t* vert_offs, const int64_t* tri_offs, int64_t V, int64_t F, float* vertices,
                       float* vcolors, int32_t* faces, void* stream) {
  if (int rc = tsdf_volume_ok(vol)) return rc;
  if (!tri_count || !edge_mask || !vert_offs || !tri_offs || !vertices || !faces) return fail(GSR_E_BADARG, "NULL argument");
  if (vcolors && !vol->color) return fail(GSR_E_BADARG, "vertex colours need a volume with a colour field");
  const int64_t N = (int64_t)vol->nx * vol->ny * vol->nz;
  if (V <= 0 || F <= 0 || V > 7 * N || F > 12 * N) return fail(GSR_E_BADARG, "V must lie in 1..7 N and F in 1..12 N");
  if ((((uintptr_t)vert_offs | (uintptr_t)tri_offs) & 7u) != 0) return fail(GSR_E_ALIGN, "offsets must be 8-byte aligned");
  if ((((uintptr_t)vertices | (uintptr_t)vcolors | (uintptr_t)faces) & 3u) != 0)
    return fail(GSR_E_ALIGN, "outputs must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_tsdf_mesh_emit(*vol, tri_count, edge_mask, vert_offs, tri_offs, V, F, vertices, vcolors, faces, s);
  return check(nullptr, s, "tsdf_mesh_emit");
}

// ---- mesh cleaning: connected components and compaction (csrc/mesh.hip) -----------------------------------------------
static bool mesh_size_ok(int64_t n) { return n >= 1 && n <= (int64_t)INT32_MAX; }
static bool mesh_aligned(std::initializer_list<const void*> ptrs, uintptr_t mask) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & mask) == 0;
}
int gsr_mesh_cc_init(int64_t n, int32_t* parent, int32_t* first, void* stream) {
  if (!mesh_size_ok(n)) return fail(GSR_E_BADARG, "n must lie in 1..2^31-1");
  if (!parent) return fail(GSR_E_BADARG, "parent is NULL");
  if (!mesh_aligned({parent, first}, 3u)) return fail(GSR_E_ALIGN, "parent / first must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_cc_init(n, parent, first, s);
  return check(nullptr, s, "mesh_cc_init");
}
int gsr_mesh_cc_hook_faces(const int32_t* faces, int64_t F, int64_t V, int32_t* parent, int32_t* status, uint64_t* stats,
                           void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (!faces || !parent || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!mesh_aligned({faces, parent, status}, 3u)) return fail(GSR_E_ALIGN, "faces / parent / status must be 4-byte aligned");
  if (!mesh_aligned({stats}, 7u)) return fail(GSR_E_ALIGN, "stats must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_cc_hook_faces(faces, F, V, parent, status, stats, s);
  return check(nullptr, s, "mesh_cc_hook_faces");
}
int gsr_mesh_edge_keys(const int32_t* faces, int64_t F, int64_t V, int64_t* keys, int32_t* owner, int32_t* status,
                       void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (!faces || !keys || !owner || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!mesh_aligned({faces, owner, status}, 3u)) return fail(GSR_E_ALIGN, "faces / owner / status must be 4-byte aligned");
  if (!mesh_aligned({keys}, 7u)) return fail(GSR_E_ALIGN, "keys must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_edge_keys(faces, F, V, keys, owner, status, s);
  return check(nullptr, s, "mesh_edge_keys");
}
int gsr_mesh_cc_hook_runs(const int64_t* keys_sorted, const int64_t* order, const int32_t* owner, int64_t m, int64_t n,
                          int32_t* parent, int32_t* status, uint64_t* stats, void* stream) {
  if (m < 1 || m > 3 * (int64_t)INT32_MAX || !mesh_size_ok(n))
    return fail(GSR_E_BADARG, "n must lie in 1..2^31-1 and m in 1..3 (2^31-1)");
  if (!keys_sorted || !order || !owner || !parent || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!mesh_aligned({owner, parent, status}, 3u)) return fail(GSR_E_ALIGN, "owner / parent / status must be 4-byte aligned");
  if (!mesh_aligned({keys_sorted, order, stats}, 7u)) return fail(GSR_E_ALIGN, "keys / order / stats must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_cc_hook_runs(keys_sorted, order, owner, m, n, parent, status, stats, s);
  return check(nullptr, s, "mesh_cc_hook_runs");
}
int gsr_mesh_cc_flatten(int64_t n, int32_t* parent, void* stream) {
  if (!mesh_size_ok(n)) return fail(GSR_E_BADARG, "n must lie in 1..2^31-1");
  if (!parent) return fail(GSR_E_BADARG, "parent is NULL");
  if (!mesh_aligned({parent}, 3u)) return fail(GSR_E_ALIGN, "parent must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_cc_flatten(n, parent, s);
  return check(nullptr, s, "mesh_cc_flatten");
}
int gsr_mesh_cc_mark(const int32_t* faces, int64_t F, int64_t V, const int32_t* parent, int32_t* first,
                     int32_t* face_root, uint8_t* mark, void* stream) {
  if (!mesh_size_ok(F)) return fail(GSR_E_BADARG, "F must lie in 1..2^31-1");
  if (!parent || !mark) return fail(GSR_E_BADARG, "NULL argument");
  const int given = (faces != nullptr) + (first != nullptr) + (face_root != nullptr);
  if (given != 0 && given != 3) return fail(GSR_E_BADARG, "give faces, first and face_root together (vertex nodes) or none");
  if (given == 3 && !mesh_size_ok(V)) return fail(GSR_E_BADARG, "V must lie in 1..2^31-1");
  if (!mesh_aligned({faces, parent, first, face_root}, 3u)) return fail(GSR_E_ALIGN, "int32 arrays must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_cc_mark(faces, F, V, parent, first, face_root, mark, s);
  return check(nullptr, s, "mesh_cc_mark");
}
int gsr_mesh_cc_label(const int32_t* face_root, const int64_t* ids, int64_t F, int64_t K, int32_t* face_component,
                      int64_t* component_faces, void* stream) {
  if (!mesh_size_ok(F) || K < 1 || K > F) return fail(GSR_E_BADARG, "F must lie in 1..2^31-1 and K in 1..F");
  if (!face_root || !ids || !face_component || !component_faces) return fail(GSR_E_BADARG, "NULL argument");
  if (!mesh_aligned({face_root, face_component}, 3u)) return fail(GSR_E_ALIGN, "int32 arrays must be 4-byte aligned");
  if (!mesh_aligned({ids, component_faces}, 7u)) return fail(GSR_E_ALIGN, "int64 arrays must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_cc_label(face_root, ids, F, K, face_component, component_faces, s);
  return check(nullptr, s, "mesh_cc_label");
}
int gsr_mesh_mark_vertices(const int32_t* faces, const uint8_t* keep, int64_t F, int64_t V, uint8_t* vertex_mark,
                           int32_t* status, void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (!faces || !keep || !vertex_mark || !status) return fail(GSR_E_BADARG, "NULL argument");
  if (!mesh_aligned({faces, status}, 3u)) return fail(GSR_E_ALIGN, "faces / status must be 4-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_mark_vertices(faces, keep, F, V, vertex_mark, status, s);
  return check(nullptr, s, "mesh_mark_vertices");
}
int gsr_mesh_compact(const float* vertices, const float* colors, const int32_t* faces, const uint8_t* keep,
                     const uint8_t* vertex_mark, const int64_t* vert_offs, const int64_t* face_offs, int64_t V, int64_t F,
                     int64_t Vk, int64_t Fk, float* out_vertices, float* out_colors, int32_t* out_faces, int32_t* status,
                     void* stream) {
  if (!mesh_size_ok(F) || !mesh_size_ok(V)) return fail(GSR_E_BADARG, "F and V must lie in 1..2^31-1");
  if (Vk < 1 || Vk > V || Fk < 1 || Fk > F) return fail(GSR_E_BADARG, "Vk must lie in 1..V and Fk in 1..F");
  if (!vertices || !faces || !keep || !vertex_mark || !vert_offs || !face_offs || !out_vertices || !out_faces || !status)
    return fail(GSR_E_BADARG, "NULL argument");
  if ((colors != nullptr) != (out_colors != nullptr)) return fail(GSR_E_BADARG, "give colors and out_colors together or neither");
  if (!mesh_aligned({vertices, colors, faces, out_vertices, out_colors, out_faces, status}, 3u))
    return fail(GSR_E_ALIGN, "float and int32 arrays must be 4-byte aligned");
  if (!mesh_aligned({vert_offs, face_offs}, 7u)) return fail(GSR_E_ALIGN, "offsets must be 8-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mesh_compact(vertices, colors, faces, keep, vertex_mark, vert_offs, face_offs, V, F, Vk, Fk, out_vertices,
                      out_colors, out_faces, status, s);
  return check(nullptr, s, "mesh_compact");
}

// ---- depth-normal consistency loss (csrc/normal_consistency.hip) ------------------------------------------------------
size_t gsr_normal_consistency_workspace_bytes(int32_t H, int32_t W) {
  return image_shape_ok(H, W) ? normal_consistency_workspace_bytes(H, W) : 0;
}
int gsr_normal_consistency_fwd_bwd(const float* depth, const float* alpha, const float* normal, int32_t H, int32_t W,
                                   float tanfovx, float tanfovy, float alpha_min, float* record, float* dL_ddepth,
                                   float* dL_dalpha, float* dL_dnormal, float* depth_normal, void* workspace,
                                   void* stream) {
  unsigned xtiles, blocks;
  if (!image_shape_ok(H, W) || !normal_consistency_blocks(H, W, &xtiles, &blocks))
    return fail(GSR_E_BADARG, "bad image shape");
  if (!(tanfovx > 0.0f) || !(tanfovy > 0.0f) || tanfovx > 3.0e38f || tanfovy > 3.0e38f)
    return fail(GSR_E_BADARG, "tanfovx and tanfovy must be positive and finite");
  if (!(alpha_min > 0.0f) || !(alpha_min <= 1.0f)) return fail(GSR_E_BADARG, "alpha_min must lie in (0, 1]");
  if (!depth || !alpha || !normal || !record || !workspace) return fail(GSR_E_BADARG, "NULL argument");
  const int ngrad = (dL_ddepth != nullptr) + (dL_dalpha != nullptr) + (dL_dnormal != nullptr);
  if (ngrad != 0 && ngrad != 3) return fail(GSR_E_BADARG, "give all three gradient pointers or none");
  if ((((uintptr_t)depth | (uintptr_t)alpha | (uintptr_t)normal | (uintptr_t)dL_ddepth | (uintptr_t)dL_dalpha |
        (uintptr_t)dL_dnormal | (uintptr_t)depth_normal) & 3u) != 0)
    return fail(GSR_E_ALIGN, "maps must be 4-byte aligned");
  if (((uintptr_t)record & 15u) != 0) return fail(GSR_E_ALIGN, "the record must be 16-byte aligned");
  if (((uintptr_t)workspace & 7u) != 0) return fail(GSR_E_ALIGN, "the workspace must be 8-byte aligned");
  const float fx = (float)((double)W / (2.0 * (double)tanfovx)), fy = (float)((double)H / (2.0 * (double)tanfovy));
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_normal_consistency(depth, alpha, normal, H, W, fx, fy, alpha_min, record, dL_ddepth, dL_dalpha, dL_dnormal,
                            depth_normal, workspace, s);
  return check(nullptr, s, "normal_consistency_fwd_bwd");
}

// ---- MCMC densification (csrc/mcmc.hip) -----------------------------------------------------------------------------
static int mcmc_rows_ok(int64_t P) { return P >= 0 && P <= (int64_t)INT32_MAX; }
int gsr_mcmc_noise(int64_t P, float* xyz, const float* scaling_raw, const float* rotation_raw, const float* opacity_raw,
                   const float* noise, float step_scale, void* stream) {
  if (!mcmc_rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (P > 0 && (!xyz || !scaling_raw || !rotation_raw || !opacity_raw || !noise)) return fail(GSR_E_BADARG, "NULL argument");
  if ((((uintptr_t)xyz | (uintptr_t)scaling_raw | (uintptr_t)opacity_raw | (uintptr_t)noise) & 3u) != 0 ||
      ((uintptr_t)rotation_raw & 15u) != 0)
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned, rotations 16-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mcmc_noise((size_t)P, xyz, scaling_raw, rotation_raw, opacity_raw, noise, step_scale, s);
  return check(nullptr, s, "mcmc_noise");
}
size_t gsr_mcmc_reg_workspace_bytes(void) { return mcmc_reg_workspace_bytes(); }
int gsr_mcmc_reg_fwd(const float* opacity_raw, const float* scaling_raw, int64_t P, float opacity_reg, float scale_reg,
                     float* record, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mcmc_rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (!record || !workspace || (P > 0 && (!opacity_raw || !scaling_raw))) return fail(GSR_E_BADARG, "NULL argument");
  if (workspace_bytes < mcmc_reg_workspace_bytes()) return fail(GSR_E_BADARG, "workspace smaller than gsr_mcmc_reg_workspace_bytes()");
  if ((((uintptr_t)opacity_raw | (uintptr_t)scaling_raw) & 3u) != 0 || ((uintptr_t)workspace & 7u) != 0 ||
      ((uintptr_t)record & 15u) != 0)
    return fail(GSR_E_ALIGN, "arrays must be 4-byte, the workspace 8-byte and the record 16-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mcmc_reg_fwd((size_t)P, opacity_raw, scaling_raw, opacity_reg, scale_reg, record, workspace, s);
  return check(nullptr, s, "mcmc_reg_fwd");
}
int gsr_mcmc_reg_bwd(const float* opacity_raw, const float* scaling_raw, int64_t P, const float* record,
                     const float* grad_out, float* grad_opacity, float* grad_scaling, void* stream) {
  if (!mcmc_rows_ok(P)) return fail(GSR_E_BADARG, "P must lie in 0..2^31-1");
  if (!record || !grad_out || (P > 0 && (!opacity_raw || !scaling_raw || !grad_opacity || !grad_scaling)))
    return fail(GSR_E_BADARG, "NULL argument");
  if ((((uintptr_t)opacity_raw | (uintptr_t)scaling_raw | (uintptr_t)record | (uintptr_t)grad_out |
        (uintptr_t)grad_opacity | (uintptr_t)grad_scaling) & 3u) != 0)
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mcmc_reg_bwd((size_t)P, opacity_raw, scaling_raw, record, grad_out, grad_opacity, grad_scaling, s);
  return check(nullptr, s, "mcmc_reg_bwd");
}
size_t gsr_mcmc_sample_workspace_bytes(int64_t P) { return mcmc_rows_ok(P) ? mcmc_sample_workspace_bytes((size_t)P) : 0; }
int gsr_mcmc_sample(int64_t P, const float* opacity_raw, float alive_threshold, const int64_t* draws, int64_t n,
                    int32_t* idx_out, int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!mcmc_rows_ok(P) || !mcmc_rows_ok(n)) return fail(GSR_E_BADARG, "P and n must lie in 0..2^31-1");
  if ((P > 0 && (!opacity_raw || !count_out || !workspace)) || (n > 0 && (!draws || !idx_out)))
    return fail(GSR_E_BADARG, "NULL argument");
  if (n > 0 && P == 0) return fail(GSR_E_BADARG, "samples asked of an empty model");
  if (P > 0 && workspace_bytes < mcmc_sample_workspace_bytes((size_t)P))
    return fail(GSR_E_BADARG, "workspace smaller than gsr_mcmc_sample_workspace_bytes(P)");
  if ((((uintptr_t)opacity_raw | (uintptr_t)idx_out | (uintptr_t)count_out) & 3u) != 0 ||
      (((uintptr_t)draws | (uintptr_t)workspace) & 7u) != 0)
    return fail(GSR_E_ALIGN, "float / int32 arrays must be 4-byte, draws and workspace 8-byte aligned");
  if (P == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mcmc_sample((size_t)P, opacity_raw, alive_threshold, draws, (size_t)n, idx_out, count_out, workspace, s);
  return check(nullptr, s, "mcmc_sample");
}
int gsr_mcmc_relocation(int64_t n, const int32_t* idx, const int32_t* count, const float* opacity_raw,
                        const float* scaling_raw, float* new_opacity_raw, float* new_scaling_raw, void* stream) {
  if (!mcmc_rows_ok(n)) return fail(GSR_E_BADARG, "n must lie in 0..2^31-1");
  if (n > 0 && (!idx || !count || !opacity_raw || !scaling_raw || !new_opacity_raw || !new_scaling_raw))
    return fail(GSR_E_BADARG, "NULL argument");
  if ((((uintptr_t)idx | (uintptr_t)count | (uintptr_t)opacity_raw | (uintptr_t)scaling_raw | (uintptr_t)new_opacity_raw |
        (uintptr_t)new_scaling_raw) & 3u) != 0)
    return fail(GSR_E_ALIGN, "arrays must be 4-byte aligned");
  if (n == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  launch_mcmc_relocation((size_t)n, idx, count, opacity_raw, scaling_raw, new_opacity_raw, new_scaling_raw, s);
  return check(nullptr, s, "mcmc_relocation");
}

}  // extern "C"
