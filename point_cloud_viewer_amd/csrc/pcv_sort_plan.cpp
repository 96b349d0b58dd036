// pcv_sort_plan.cpp — the passes of a radix sort from its facts (pcv_sort_plan.h). Standard C++, no HIP.
#include "pcv_sort_plan.h"

PcvSortGeom pcv_sort_geom(uint64_t n, uint64_t unit) {
  PcvSortGeom g;
  g.n = n;
  const uint64_t tiles = (n + unit - 1) / unit;
  uint64_t tiles_per_group = (tiles + kPcvSortMaxGroups - 1) / kPcvSortMaxGroups;
  if (tiles_per_group == 0) tiles_per_group = 1;
  g.chunk = tiles_per_group * unit;
  g.groups = (int)((n + g.chunk - 1) / g.chunk);
  if (g.groups < 1) g.groups = 1;
  return g;
}

uint32_t pcv_sort_rows_true_bins(uint64_t n, uint32_t forced) {
  if (forced) return forced;
  return n >= 500000000ull ? 65536u : n >= 200000000ull ? 32768u : 16384u;
}

PcvSortScratch pcv_sort_scratch(uint64_t n, uint32_t rows_true_bins_forced) {
  constexpr size_t kHist = (size_t)kPcvSortRadix * kPcvSortMaxGroups * sizeof(uint32_t), kTotals = kPcvSortRadix * sizeof(uint32_t);
  const bool two_pass_possible = pcv_sort_geom(n, kPcvSortRec12Tile).groups >= 8;
  PcvSortScratch s;
  s.hist = 0;
  s.totals = s.hist + kHist;
  s.hist2 = s.totals + kTotals;
  s.totals2 = s.hist2 + kHist;
  s.ranges = s.totals2 + kTotals;
  s.order = s.ranges + (size_t)kPcvSortMaxGroups * 2 * sizeof(uint32_t);
  s.rows_true = s.order + (size_t)kPcvSortMaxGroups * sizeof(uint32_t);
  s.end = s.rows_true +
          (two_pass_possible ? (size_t)pcv_sort_rows_true_bins(n, rows_true_bins_forced) * kPcvSortMaxGroups * sizeof(uint32_t) : 0);
  return s;
}

namespace {

int digit_values(int nbits) { return nbits <= 7 ? 128 : 256; }

PcvSortPass rec12_pass(int shift, int nbits, PcvSortHist hist, PcvSortDown down, bool plane) {
  PcvSortPass p{};
  p.shift = shift, p.nbits = nbits;
  p.hist = hist, p.down = down;
  p.R = digit_values(nbits), p.PL = plane;
  return p;
}

// The first pass(es) of a mapped 12-byte record sort whose histograms come from the rank counts: one pass on the first digit, or
// — where the rank has two digits, the scratch holds its counters and there are enough workgroups — the whole sort in two.
void plan_rows_form(const PcvSortFacts& f, int width, PcvSortPlan* plan) {
  const int shift = f.begin_bit, total_bits = f.end_bit - f.begin_bit;
  const int nbits = total_bits < width ? total_bits : width;
  const int nbits2 = f.end_bit - (shift + width) < width ? f.end_bit - (shift + width) : width;
  const uint32_t bins = pcv_sort_rows_true_bins(f.n, f.rows_true_bins);
  // (ranks of 15 bits — trees of up to 32 768 leaves — where the scratch holds their counters)
  plan->two_pass = f.sort_rows2 && f.map_entries <= bins && shift + width < f.end_bit && shift + width + nbits2 >= f.end_bit &&
                   (1ull << total_bits) <= bins && nbits2 >= 1 && plan->geom.groups >= 8;
  plan->msd = f.sort_msd && plan->two_pass;  // upper digit first, the second pass sorts inside every bucket
  const int p1_shift = plan->msd ? shift + width : shift, p1_bits = plan->msd ? nbits2 : nbits;
  // the map's place is judged by the LOWER digit's width, msd or not: never the more generous of the two kernel forms
  const uint32_t lds_entries = f.packed ? pcv_sort_map_lds_staged(digit_values(nbits), f.color_stride)
                                        : pcv_sort_map_lds(plan->with_plane, digit_values(nbits)).max_entries;
  const bool map_in_lds = f.map_entries <= lds_entries;
  PcvSortPass& first = plan->pass[plan->npasses++];
  first = rec12_pass(p1_shift, p1_bits, plan->two_pass ? PCV_HIST_ROWS_TRUE : PCV_HIST_ROWS, PCV_DOWN_REC12_CHUNKS, plan->with_plane);
  first.MAP = map_in_lds ? 1 : 2;
  first.dyn_lds = map_in_lds ? (((size_t)f.map_entries * 2 + 15) & ~(size_t)15) : 0;
  first.packed = f.packed;
  first.color_lds = f.packed ? pcv_sort_color_buffer(f.color_stride) : 0;
  if (!plan->two_pass) return;
  // second pass: pieces of whole first-pass runs
  const int D1 = 1 << p1_bits;
  plan->blocks = kPcvSortMaxGroups / D1;
  if (plan->blocks > plan->geom.groups) plan->blocks = plan->geom.groups;
  if (plan->blocks < 1) plan->blocks = 1;
  plan->gpb = (plan->geom.groups + plan->blocks - 1) / plan->blocks;
  plan->pieces = D1 * plan->blocks;
  plan->pass[plan->npasses++] = rec12_pass(plan->msd ? shift : shift + width, plan->msd ? nbits : nbits2, PCV_HIST_ROWS_TRUE,
                                           PCV_DOWN_REC12_PIECES, plan->with_plane);
  plan->held_back = f.second && !plan->msd;
}

}  // namespace

const char* pcv_sort_plan(const PcvSortFacts& f, PcvSortPlan* plan) {
  *plan = PcvSortPlan{};
  plan->result_in_a = true;
  plan->blocks = plan->gpb = 1;
  if (f.n == 0 || f.end_bit <= f.begin_bit) return nullptr;
  if (f.n >= 0xffffffffull) return "radix sort: n must be < 2^32 - 1";
  plan->records = f.vec_in || f.nwords > 0;
  if (plan->records && f.key_bytes != 4) return "record sort needs 32-bit keys";
  plan->compact = plan->records && f.vec_in && f.vec_bytes == 8;  // 12-byte records
  // 12-byte records, alone or with ONE 4-byte plane (intensity); more planes (the exact pipeline's wide codes) take the 256-lane kernel
  plan->with_plane = plan->compact && f.nwords == 1;
  plan->rec12 = plan->compact && (f.nwords == 0 || plan->with_plane);
  plan->geom = pcv_sort_geom(f.n, plan->rec12 ? kPcvSortRec12Tile : kPcvSortTileUnit);
  // Records: as few passes as 8-bit digits allow, but of EQUAL width (13 bits -> 7 + 6, not 8 + 5): the run a digit gets
  // inside a tile is tile / 2^width records, and the 4-byte key runs of an 8-bit pass (8 keys = 32 bytes) are partial
  // sectors. Keys-only sorts keep full 8-bit digits (fewest passes is what counts there).
  const int total_bits = f.end_bit - f.begin_bit;
  const int passes = (total_bits + 7) / 8;
  const int width = plan->records ? (total_bits + passes - 1) / passes : 8;
  int shift = f.begin_bit;
  if (f.packed && !(f.map && f.rows && plan->rec12 && !plan->with_plane && f.color_in && f.map_entries <= kPcvPackedRanks))
    return "record sort: packed records need the rows form without a plane, color_in and a map of <= 65 536 entries";
  if (f.map && f.rows && plan->rec12) {
    plan_rows_form(f, width, plan);
    shift = plan->two_pass ? f.end_bit : f.begin_bit + width;
  }
  for (; shift < f.end_bit; shift += width) {
    const int nbits = f.end_bit - shift < width ? f.end_bit - shift : width;
    PcvSortPass& p = plan->pass[plan->npasses++];
    p = rec12_pass(shift, nbits, PCV_HIST_UPSWEEP, PCV_DOWN_KEYS, plan->with_plane);
    if (f.map && shift == f.begin_bit && f.key_bytes == 4 && f.vec_in) {  // finalize fused into the first upsweep
      p.hist = PCV_HIST_UPSWEEP_MAP;
      p.map_lds = f.map_entries && f.map_entries <= kPcvSortUpsweepMapLdsEntries;
    } else {
      p.plain_add = plan->records && shift != f.begin_bit;
    }
    if (plan->rec12) p.down = PCV_DOWN_REC12_CHUNKS;
    else if (plan->compact) p.down = PCV_DOWN_REC_UINT2;
    else if (f.vec_in) p.down = PCV_DOWN_REC_UINT4;
    else if (plan->records) p.down = PCV_DOWN_REC_PLANES;
    if (!plan->rec12) p.R = kPcvSortRadix, p.PL = false;
  }
  plan->result_in_a = plan->npasses % 2 == 0;
  return nullptr;
}
