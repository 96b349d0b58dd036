// pcv_sort_plan.h — what a radix sort will launch, worked out before anything is launched: the geometry, the passes with their
// histogram source and downsweep form, the two-pass rows form of the single-chain build's record sort, the scratch layout, the
// map-in-LDS budget and the condition for the settling pass. Standard C++: no HIP header and no global is read, so that the plan
// can be built and checked on a machine without a GPU (tests/test_sort_plan_cpu.py). pcv_sort.hip and pcv_sort_rec12.hip launch
// what the plan says; pcv_sort_dev.h holds the kernels' side of the same constants.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "pcv_color_stage.h"

constexpr int kPcvSortRadix = 256;       // digit values of a pass (8-bit digits)
constexpr int kPcvSortMaxGroups = 1024;  // sort workgroups (and pieces of a second pass) at most: one scan workgroup covers them
constexpr int kPcvSortTileUnit = 4096;   // chunk granularity of the 256-lane kernels: 256 lanes x 16 keys
constexpr int kPcvSortRec12Tile = 8192;  // tile of the 12-byte record downsweep: 1 024 lanes x 8 records
constexpr int kPcvSortMaxPasses = 8;     // 64 bits in 8-bit digits

struct PcvSortGeom {
  uint64_t n;
  uint64_t chunk;  // keys per workgroup, a multiple of the tile
  int groups;
};
PcvSortGeom pcv_sort_geom(uint64_t n, uint64_t unit = kPcvSortTileUnit);

// true-rank counters per sort workgroup the scratch holds (hist12_from_rows_kernel): 2^14, and 2^15 for clouds big enough to have
// that many leaves (128 MB of scratch instead of 64), 2^16 from 500 M points on (256 MB). `forced`: PcvSwitches::rows_true_bins.
uint32_t pcv_sort_rows_true_bins(uint64_t n, uint32_t forced);

// The sort's scratch block, byte offsets in this order: two histograms ([256][1 024] words) with their digit totals (256 words),
// the second pass's piece ranges (uint2 per piece) and launch order, and the rank counts re-indexed by true rank (rows_true:
// bins x 1 024 words) — the last only for inputs whose record sort can take the two-pass rows form at all (12-byte records in
// tiles of 8 192, i.e. >= 8 sort workgroups: n >= 65 536); small builds get by with 2 MB. pcv_sort_scratch_bytes(n) = end + slack.
struct PcvSortScratch {
  size_t hist, totals, hist2, totals2, ranges, order, rows_true, end;
};
constexpr size_t kPcvSortScratchSlack = 256;
PcvSortScratch pcv_sort_scratch(uint64_t n, uint32_t rows_true_bins_forced);

// The rank map in the dynamic LDS of the first rows pass (downsweep_rec12_kernel<.., MAP = 1>, half words): how many entries a
// kernel form admits (bigger maps are gathered from global memory, MAP = 2) and the dynamic LDS the form is allowed to ask for.
// Static LDS of the kernel the figures rest on, of the 163 840 bytes a workgroup can have: tiles of 8 192 records (12 bytes, 16
// with the intensity plane) + the digit state of 16 waves for 128 / 256 digit values = 107 584 / 116 800 bytes without a plane,
// 140 352 / 149 568 with it (.group_segment_fixed_size of the instantiations); static + attr_bytes stays inside.
struct PcvSortMapLds {
  uint32_t max_entries;  // map_entries <= this: MAP = 1
  uint32_t attr_bytes;   // hipFuncAttributeMaxDynamicSharedMemorySize of the instantiation
};
constexpr PcvSortMapLds pcv_sort_map_lds(bool plane, int R) {
  return !plane ? PcvSortMapLds{16384u, 32768u} : R == 128 ? PcvSortMapLds{10000u, 20480u} : PcvSortMapLds{5000u, 10240u};
}

// The staged colours of that pass (pcv_color_stage.h): where the records arrive without their colour, the workgroup fetches a
// tile's colour bytes as aligned 16-byte pieces into a buffer in the same dynamic LDS, behind the map. ONE rule says what fits:
//   static LDS of the form + the map's half words (rounded up to 16 bytes) + the buffer <= 163 840 bytes.
// (pcv_sort_rec12.hip asserts that the static part is what pcv_sort_rec12_static_lds says.)
// The packed hand-over (PcvSortFacts::packed) needs the buffer, so the map gives way: it stays in LDS up to
// pcv_sort_map_lds_staged(R, stride) entries — 15 824 / 11 216 entries at stride 3 for 128 / 256 digit values, 11 728 / 7 120 at
// stride 4 — and is gathered from global memory above that. 12-byte records with color_in (the stage entry, PCV_COLOR_LATE) keep
// their plan — a map of up to 16 384 entries in LDS, which leaves no room for the buffer — and their colour loads per lane.
constexpr uint32_t kPcvSortLdsBytes = 163840;
constexpr uint32_t pcv_sort_rec12_static_lds(bool plane, int R) {
  return (uint32_t)kPcvSortRec12Tile * (plane ? 16u : 12u) + (uint32_t)R * 4u * (16u + 2u) + 64u;
}
constexpr uint32_t pcv_sort_color_buffer(int stride) { return pcv_color_stage_bytes(kPcvSortRec12Tile, (uint32_t)stride); }
constexpr uint32_t pcv_sort_map_lds_staged(int R, int stride) {
  return ((kPcvSortLdsBytes - pcv_sort_rec12_static_lds(false, R) - pcv_sort_color_buffer(stride)) / 16u) * 8u < pcv_sort_map_lds(false, R).max_entries
             ? ((kPcvSortLdsBytes - pcv_sort_rec12_static_lds(false, R) - pcv_sort_color_buffer(stride)) / 16u) * 8u
             : pcv_sort_map_lds(false, R).max_entries;
}
static_assert(pcv_sort_rec12_static_lds(false, 256) + 2 * (size_t)pcv_sort_map_lds_staged(256, 4) + pcv_sort_color_buffer(4) <= kPcvSortLdsBytes &&
                  pcv_sort_rec12_static_lds(false, 128) + 2 * (size_t)pcv_sort_map_lds_staged(128, 3) + pcv_sort_color_buffer(3) <= kPcvSortLdsBytes,
              "the lowered limits fit");
// what the packed instantiations may ask for: everything the static part leaves (pcv_sort_rec12.hip asserts the static part)
constexpr uint32_t pcv_sort_rec12_dyn_attr(int R) { return kPcvSortLdsBytes - pcv_sort_rec12_static_lds(false, R); }
// The packed hand-over of the single-chain build (chain_pass_kernel DIAG 2 -> the first pass above), stated once.
// Tried — the chain pass runs in the form that can pack — for 12-byte records of raw (not routed) input without an intensity plane.
constexpr bool pcv_packed_handover_tried(bool switched_on, bool compact, bool routed, bool intensity) {
  return switched_on && compact && !routed && !intensity;
}
// ... and the records are the 8-byte ones where the predicted tree T'' has at most 65 536 nodes: a predicted leaf is named by its
// node index, which then fits the record's 16 bits. The chain pass asks the device's count of the nodes, the host its mirror of
// the same tree; the sort's map has one entry per node. (constexpr: callable from kernels.)
constexpr uint32_t kPcvPackedRanks = 65536;
constexpr bool pcv_packed_handover(uint32_t tree_nodes) { return tree_nodes <= kPcvPackedRanks; }

// upsweep_map_kernel<kMapLds = true> holds the map as words: 60 000 bytes next to its 4 KB of counters, inside the 64 KB a kernel
// gets without opting in
constexpr uint32_t kPcvSortUpsweepMapLdsEntries = 15000;

// Does the held-back second pass settle the leaves' points itself (downsweep_settle_kernel)? With an intensity plane the pass
// has no LDS for 256 digit values, and it needs the octree's intensity blob to write to. pcv_build_finish decides with this
// whether to plan for it and to hand a PcvSortFuse over; pcv_radix_sort_records_second whether to launch it.
constexpr bool pcv_sort_second_settles(int nbits, bool plane, bool intensity_blob) {
  return (nbits <= 7 || !plane) && (!plane || intensity_blob);
}
// ...and in which form: colour-only records in tiles of 4 096 (512 lanes, two workgroups per CU), with the plane in tiles of
// 8 192; ranks of 16 bits (colour-only): 256 digit values, tiles of 8 192
enum PcvSortSettleForm { PCV_SETTLE_512 = 0, PCV_SETTLE_1024_PLANE = 1, PCV_SETTLE_1024_R256 = 2 };
constexpr PcvSortSettleForm pcv_sort_settle_form(int nbits, bool plane) {
  return nbits > 7 ? PCV_SETTLE_1024_R256 : plane ? PCV_SETTLE_1024_PLANE : PCV_SETTLE_512;
}

enum PcvSortHist {
  PCV_HIST_UPSWEEP = 0,      // upsweep_kernel counts the keys
  PCV_HIST_UPSWEEP_MAP = 1,  // upsweep_map_kernel translates the ranks through the map and counts them
  PCV_HIST_ROWS = 2,         // hist_from_rows_kernel: from the rank counts, the keys are not read
  PCV_HIST_ROWS_TRUE = 3,    // two-pass rows form: hist12_from_rows_kernel (first pass), pass2_layout_kernel (second)
};
enum PcvSortDown {
  PCV_DOWN_KEYS = 0,
  PCV_DOWN_REC_UINT4 = 1,   // downsweep_rec_kernel: 20-byte records (+ planes)
  PCV_DOWN_REC_UINT2 = 2,   // 12-byte records with more than one plane
  PCV_DOWN_REC_PLANES = 3,  // key + planes, no payload word
  PCV_DOWN_REC12_CHUNKS = 4,  // downsweep_rec12_kernel, workgroup g takes chunk g
  PCV_DOWN_REC12_PIECES = 5,  // ... takes piece order[g] = the records ranges[.] of whole first-pass runs
};
struct PcvSortPass {
  int shift, nbits;
  PcvSortHist hist;
  bool plain_add;  // upsweep: one LDS add per key (the upper digits of a record sort, after a pass has mixed them)
  bool map_lds;    // upsweep with map: the map (words) in dynamic LDS
  PcvSortDown down;
  // rec12 forms: digit values of the instantiation (128 for digits of <= 7 bits), the plane, the map (0: none, 1: in LDS,
  // 2: in global memory) and the dynamic LDS the launch asks for
  int R;
  bool PL;
  int MAP;
  size_t dyn_lds;
  // first pass of the rows form: the records are the chain pass's packed 8-byte ones, and the bytes of the staged colours' buffer
  // behind the map's dyn_lds (0 for every other form)
  bool packed;
  size_t color_lds;
};

struct PcvSortFacts {
  uint64_t n = 0;
  int key_bytes = 4;
  int begin_bit = 0, end_bit = 0;
  // the payload's shape (PcvSortPayload)
  bool vec_in = false;
  int vec_bytes = 16;
  int nwords = 0;
  bool color_in = false;  // (changes no pass: the first pass of the rows form reads the colour where it is set)
  int color_stride = 3;
  // the chain pass's packed hand-over: 8-byte records {codes / pool entry, code z | predicted rank << 16}, no key array, the
  // colour in the caller's array (color_in). Rows form without a plane and map_entries <= kPcvPackedRanks only.
  bool packed = false;
  // single-chain build: the rank map, the rank-count rows, a PcvSortSecond to hold the second pass back in
  bool map = false;
  uint32_t map_entries = 0;
  bool rows = false;
  bool second = false;
  // PcvSwitches
  bool sort_rows2 = true, sort_msd = false;
  uint32_t rows_true_bins = 0;
};

struct PcvSortPlan {
  bool records, compact, with_plane, rec12;
  PcvSortGeom geom;
  int npasses;
  PcvSortPass pass[kPcvSortMaxPasses];
  // two-pass rows form: pass[0] and pass[1] are its first and second pass (the rank's lower digit first, unless msd) and there
  // is no other; piece k of the second pass = first digit k / blocks, workgroups [blk * gpb, (blk + 1) * gpb) of the first pass
  bool two_pass, msd;
  int blocks, gpb, pieces;
  bool held_back;  // the second pass is left to pcv_radix_sort_records_second
  bool result_in_a;
};

// Returns null and fills *plan, or the reason why there is no such sort. An empty sort (n == 0, no bits) has no passes.
const char* pcv_sort_plan(const PcvSortFacts& f, PcvSortPlan* plan);
