// The host-side launchers that cross a file boundary: those gsr_api.hip sequences into a frame (preprocess, binning,
// render, the maps, launch_unpack_geom) and the few that one kernel file borrows from another (the scan and the pair
// sort; launch_ssim_metric; launch_gather_rows).  Each is defined next to its kernel, so that the translation units can be compiled with
// different floating-point contraction settings.  A launcher with one caller in its own file is not declared here.
#pragma once
#include "gsr_common.h"

namespace gsr {

// preprocess.hip
// block_big / big_list: every block lists its Gaussians with more than ROWS_COOP instances at big_list[block * PRE_BLOCK ..]
// and writes how many (no counter to zero in front of the frame, no atomics); the scan launch below turns the counts
// into offsets
void launch_preprocess_fwd(const GsrParams& p, GeomRec* rec, BinInfo* bin, uint32_t* block_sums, uint32_t* block_vis,
                           int32_t* radii, uint32_t* block_big, uint32_t* big_list, uint2* block_range, hipStream_t s);
// folds the gradient rows of every listed Gaussian into its first row (wave-cooperative, fixed order); nb = blocks of
// preprocess_fwd, big_offs = the scanned block_big (nb + 1 entries)
void launch_sum_big_rows(const uint32_t* big_count, const uint32_t* big_offs, int nb, const uint32_t* big_list,
                         const GeomRec* rec, const uint32_t* slot_base, GradRow* rows, uint8_t* row_flags, hipStream_t s);
// exclusive scans of up to three per-block arrays in one launch (block 0: a, block 1: b, block 3: c; block 2 folds
// block_range, and c comes only with it); total_x = grand total.  Every sums_x and offs_x must be 16-byte aligned (the
// kernel moves whole 32-entry lines as uint4) and offs_x holds nb + 1 entries; arrays carved out of one buffer sit
// scan_array_stride(nb) words apart, which keeps each of them 256-byte aligned when the first one is
inline int scan_array_stride(int nb) { return (int)align_up((size_t)nb + 1, 64); }
void launch_scan_block_sums(const uint32_t* sums_a, uint32_t* offs_a, uint32_t* total_a, const uint32_t* sums_b,
                            uint32_t* offs_b, uint32_t* total_b, int nb, hipStream_t s,
                            uint32_t* host_mirror = nullptr, const uint2* block_range = nullptr,
                            const uint32_t* sums_c = nullptr, uint32_t* offs_c = nullptr, uint32_t* total_c = nullptr);
void launch_preprocess_bwd(const GsrParams& p, const int32_t* radii, const GeomRec* rec, const uint32_t* slot_base,
                           const GradRow* rows,
                           const uint8_t* row_flags, const GsrGrads& g, hipStream_t s);
// camera gradients (GsrGrads.dL_dviewmatrix ...): launch_preprocess_bwd then runs the camera instantiation, whose blocks
// leave 27 double sums each in g.camera_ws (camera_grad_bytes(P) bytes), and the one-block finish that adds the first
// nslots of them in a fixed order (nslots = 0: writes zeros)
size_t camera_grad_bytes(int P);
void launch_camera_grad_finish(const GsrGrads& g, int nslots, hipStream_t s);

// binning.hip
void launch_duplicate_with_keys(int P, int grid_x, const BinInfo* bin, const uint32_t* block_offs, uint32_t* slot_base,
                                uint32_t* point_offsets, uint64_t* keys, uint32_t* vals, hipStream_t s);
// returns true when the sorted result ended in (keys_b, vals_b)
bool launch_sort_pairs(uint64_t* keys_a, uint32_t* vals_a, uint64_t* keys_b, uint32_t* vals_b, uint32_t n,
                       int end_bit, void* scratch, hipStream_t s);
// n_dev != NULL: the element count is read from device memory and n is the capacity the grid is sized for
// In / out of a sort that also delivers where every key value's run lies in the sorted array, without a pass over it
// (binning.hip: seg_block, radix_rowscan_kernel, ranges_and_order_from_sort_body).
struct SortedRuns {
  uint2* runs_rel;               // in: [n_keys] array the last pass's row scan writes RELATIVE runs into (two-pass sorts)
  uint32_t n_keys;               // in: number of key values (tiles)
  uint32_t* order;               // in: nullptr, or the [n_keys] tile order: the last scatter then carries a workgroup that
                                 //     completes runs_rel into the tile ranges and fills order (ranges_and_order_from_sort_body)
  bool valid;                    // out: false = more than two passes (use identify_tile_ranges)
  bool fused;                    // out: the ranges and the order are already enqueued (valid, and order was given): the
                                 //      caller skips launch_ranges_and_order_from_sort
  bool relative;                 // out: runs_rel was written (two passes); false: one pass, the runs are the digit totals' scan
  const uint32_t* totals_last;   // out: digit totals of the last pass
  int lo_bits, hi_bits;          // out: digit widths of the first / last pass (lo_bits = 0: one pass)
};
// runs != NULL: sorts of at most two passes run their last pass segmented and fill *runs
bool launch_sort_pairs_u32(uint32_t* keys_a, uint32_t* vals_a, uint32_t* keys_b, uint32_t* vals_b, uint32_t n,
                           int end_bit, void* scratch, hipStream_t s, const uint32_t* n_dev = nullptr,
                           SortedRuns* runs = nullptr);
// r_dev != NULL: the instance count is read from device memory and R is the capacity the grid is sized for
void launch_identify_tile_ranges_u32(uint32_t R, const uint32_t* tiles, uint2* ranges, hipStream_t s,
                                     const uint32_t* r_dev = nullptr);
inline int sort_passes(int end_bit) { return (end_bit + RADIX_BITS - 1) / RADIX_BITS; }
void launch_identify_tile_ranges(uint32_t R, const uint64_t* keys, uint2* ranges, hipStream_t s);
void launch_build_tile_order(int tiles, const uint2* ranges, uint32_t* order, hipStream_t s);
// two-level binning: tile ranges ((0,0) for empty tiles) from the tile sort's histogram + the tile order, one kernel
void launch_ranges_and_order_from_sort(int tiles, const SortedRuns& sr, uint2* ranges, uint32_t* order, hipStream_t s);
// also derives the device-side counts of the later stages (GeomLayout::total[TOTAL_TOP_PASS_N / TOTAL_R_CLAMPED]);
// capacity: instances the binning workspace holds (0xffffffff when the host sizes it from the real count)
// top_pass_enqueued = false: total[TOTAL_TOP_PASS_N] stays 0 whatever the frame's depth span (nobody will run the pass)
void launch_compact_visible(int P, const BinInfo* bin, const uint32_t* block_vis_offs, const uint32_t* block_offs,
                            uint32_t* slot_base, uint32_t* total, uint32_t capacity, int grid_x, uint32_t* dkey,
                            uint2* dval, hipStream_t s, bool top_pass_enqueued = true);
// (32-bit key, 64-bit value) pairs: the depth sort, whose payload is (index, packed rect)
bool launch_sort_pairs_u32_v64(uint32_t* keys_a, uint2* vals_a, uint32_t* keys_b, uint2* vals_b, uint32_t n,
                               int end_bit, void* scratch, hipStream_t s, const uint32_t* n_dev = nullptr);
void launch_sort_extra_pass_u32(const uint32_t* kin, const uint2* vin, uint32_t* kout, uint2* vout, uint32_t n,
                                const uint32_t* n_dev, int shift, int nbits, void* scratch, hipStream_t s);
// The two-level binning sorts the visible Gaussians on (depth bits - smallest depth bits of the frame).  Three 8-bit
// passes (24 bits: up to two binades of depth, e.g. 3 .. 12) are enqueued before the host knows the counts; a frame
// that spans more gets the fourth 8-bit pass on bits 24..31: its kernels take their element count from
// total[TOTAL_TOP_PASS_N] (V or 0, set on the device), and the consumers pick the buffer the result ended in.
// (Three 9-bit passes were measured too: as slow as four 8-bit ones -- wider digits rank and scatter more slowly.)
// d3 / d4: the depth-sorted payload after the three regular passes / after the top-digit pass (chosen on the device)
void launch_count_tiles(uint32_t v_cap, const uint32_t* total, const uint2* d3, const uint2* d4, const BinInfo* bin,
                        uint32_t* block_sums2, hipStream_t s);
// Small frames (at most EMIT_WIDE_MAX_BLOCKS blocks of 256 depth-sorted Gaussians): emit_instances runs with 1024 threads
// per block and takes the block TOTALS of count_tiles as block_offs2 (it sums the totals in front of each block itself):
// the caller then skips the scan between the two kernels.
constexpr uint32_t EMIT_WIDE_MAX_BLOCKS = 512;
inline bool emit_is_wide(uint32_t v_cap) { return (v_cap + PRE_BLOCK - 1) / PRE_BLOCK <= EMIT_WIDE_MAX_BLOCKS; }
void launch_emit_instances(uint32_t v_cap, const uint32_t* total, int grid_x, const uint2* d3, const uint2* d4,
                           const BinInfo* bin, const uint32_t* block_offs2, uint32_t* inst_tile, uint32_t* inst_g,
                           uint32_t capacity, hipStream_t s);
void launch_reconstruct_keys(uint32_t R, uint32_t P, const uint32_t* tile_sorted, const uint32_t* point_list,
                             const BinInfo* bin, uint64_t* keys, hipStream_t s);

// render.hip
void launch_render_fwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const GeomRec* rec,
                       const float* bg, float* out_color, float* final_T, uint32_t* n_contrib, uint32_t* tile_max,
                       const uint32_t* tile_order, hipStream_t s, unsigned long long* stats, int cull, uint16_t* inst_mask);
void launch_render_bwd(int W, int H, const uint2* ranges, const uint32_t* point_list, const GeomRec* rec,
                       const uint32_t* slot_base,
                       const float* bg, const float* final_T, const uint32_t* n_contrib, const uint32_t* tile_max,
                       const float* dL_dpix, GradRow* rows, uint8_t* row_flags, const uint32_t* tile_order,
                       hipStream_t s, const uint16_t* inst_mask);

// What the map kernels read of a rendered frame (gsr_api.hip: map_frame builds it from a validated GsrAuxFrame).
struct MapFrame {
  int W, H, grid_x, tiles;
  const uint2* ranges;
  const uint32_t* point_list;
  const GeomRec* rec;
  const BinInfo* bin;
  const uint32_t* n_contrib;
  const float* final_T;
  const uint32_t* tile_order;
};

// depth.hip: depth / inverse-depth / alpha maps of a rendered frame and their gradients (acc: zeroed [P,8] floats)
void launch_aux_maps_fwd(const MapFrame& f, float* out, hipStream_t s);
void launch_aux_maps_bwd(const MapFrame& f, const float* dL_dmaps, float* acc, hipStream_t s);
void launch_aux_geom_bwd(const GsrParams& p, const int32_t* radii, const float* acc, const GsrAuxGrads& g, hipStream_t s);

// features.hip: per-Gaussian feature rows features[P,C] composited to C-channel maps of a rendered frame (the entries and
// weights of depth.hip), and the backward: geometry sums into acc [P,8] (the layout launch_aux_geom_bwd reads; nullptr:
// not wanted), dL/dfeatures added into dL_dfeatures [P,C] (zeroed by the caller; nullptr: not wanted)
void launch_feature_maps_fwd(const MapFrame& f, const float* features, int C, float* out, hipStream_t s);
void launch_feature_maps_bwd(const MapFrame& f, const float* features, int C, const float* dL_dmaps, float* acc,
                             float* dL_dfeatures, hipStream_t s);

// abs_grad.hip: the absolute view-space gradient of the COLOUR image (AbsGS): per Gaussian the sum over its composited
// pixels of |d colour-loss / d mean2D| per component, added into abs_means2D [P,3] (zeroed by the caller; columns 0 and 1,
// GsrGrads.dL_dmeans2D's scale); bg: device [3], the frame's background; dL_dcolor: device [3,H,W]
void launch_abs_grad_bwd(const MapFrame& f, const float* bg, const float* dL_dcolor, float* abs_means2D, hipStream_t s);

// distortion.hip: the depth-distortion map dist [1,H,W] of a rendered frame (the entries and weights of depth.hip; mapping
// 0: m = z, 1: m = far / (far - near) (1 - near / z)), the per-pixel state [2,H,W] its backward reads, and the backward:
// sums into acc [P,8] (zeroed by the caller; the layout launch_aux_geom_bwd reads, d z word included)
void launch_distortion_fwd(const MapFrame& f, int mapping, float near, float far, float* dist, float* state, hipStream_t s);
void launch_distortion_bwd(const MapFrame& f, int mapping, float near, float far, const float* state, const float* dL_ddist,
                           float* acc, hipStream_t s);

// median.hip: the median-depth map median [1,H,W] of a rendered frame (z of the last composited entry whose transmittance
// in front of it exceeds one half; the entries of depth.hip), the id of that entry's Gaussian median_id [H,W] (-1: none) and
// its list position state [H,W] (0xffffffff: none); the backward adds dL_dmedian into acc [P] (zeroed by the caller, one
// global atomic per tile and entry) and the finish kernel writes d_means3D [P,3] = acc * viewmatrix[0:3, 2] in full
void launch_median_depth_fwd(const MapFrame& f, float* median, int32_t* median_id, uint32_t* state, hipStream_t s);
void launch_median_depth_bwd(const MapFrame& f, const uint32_t* state, const float* dL_dmedian, float* acc, hipStream_t s);
void launch_median_depth_finish(int P, const float* viewmatrix, const float* acc, float* d_means3D, hipStream_t s);

// contribution.hip: per-Gaussian blending-weight statistics of a rendered frame, added into stats [P,3] (int64: sum of
// round(w 2^30), pixel count, float bits of the largest w) with integer atomics; pixel_mask: nullptr or [H,W] bytes
void launch_contribution(const MapFrame& f, const uint8_t* pixel_mask, int64_t* stats, hipStream_t s);

// loss.hip, called by metrics.hip: forward-only SSIM of the evaluation path, one partial per 16x16 tile and channel, no
// derivative maps
void launch_ssim_metric(const float* x, const float* gt, int C, int H, int W, int clamp_flags, float* partials,
                        hipStream_t s);

// densify_fork.hip, called by densify.hip too: one gather of a densification plan.  Source row i (w floats) goes to
// dst rows pos[i] (original), counts[0] + pos[P + i] (clone / grown) and counts[0] + counts[1] + j counts[2] + pos[2P + i]
// (child copy j < ncopies), wherever that pos is not -1.  po / pe / pc: GSR_ROW_COPY, GSR_ROW_CONST (`value`) or
// GSR_ROW_SKIP per role; po binds only the originals whose flag byte has the fork's selected bit, the others copy, and
// with po = GSR_ROW_COPY flags is not read.  Bit copies only: no contraction setting can change its results.
void launch_gather_rows(int P, int w, const float* src, const uint8_t* flags, const int32_t* pos,
                        const uint32_t counts[3], int ncopies, int po, int pe, int pc, float value, float* dst,
                        hipStream_t s);

// aux.hip: the unpack kernel behind gsr_debug_read_geom
void launch_unpack_geom(int P, const GeomRec* rec, const BinInfo* bin, const uint32_t* block_offs, float* xy,
                        float* conic_opacity, float* rgb, float* depth, uint32_t* tiles, uint32_t* point_offsets,
                        uint32_t* rect, uint32_t* clamped, hipStream_t s);

}  // namespace gsr
