// pcv_sort_records_check.cpp — the argument checks of pcv_sort_records (pcv_sort_records_check.h). Standard C++, no HIP.
#include "pcv_sort_records_check.h"

const char* pcv_sort_records_check(const pcv_sort_records_args* a, const PcvSortRecordsSwitches& sw, PcvSortFacts* facts,
                                   PcvSortPlan* plan) {
  if (!a) return "pcv_sort_records: args is null";
  if (a->mem != PCV_MEM_HOST && a->mem != PCV_MEM_DEVICE) return "pcv_sort_records: bad mem";
  if (a->vec_bytes != 0 && a->vec_bytes != 8 && a->vec_bytes != 16) return "pcv_sort_records: vec_bytes must be 0, 8 or 16";
  if (a->nwords < 0 || a->nwords > 8) return "pcv_sort_records: nwords must be 0..8";
  if (a->vec_bytes == 0 && a->nwords == 0) return "pcv_sort_records: a record needs a payload or a plane";
  const bool compact = a->vec_bytes == 8;
  if (a->key_bits < 1 || a->key_bits > (compact ? 24 : 32)) return "pcv_sort_records: key_bits outside the key's rank field";
  if (a->n >= 0xffffffffull) return "radix sort: n must be < 2^32 - 1";
  if (a->rows_mode != PCV_SORT_ROWS_NONE && a->rows_mode != PCV_SORT_ROWS_GIVEN && a->rows_mode != PCV_SORT_ROWS_DEVICE)
    return "pcv_sort_records: bad rows_mode";
  if (a->color_stride != 3 && a->color_stride != 4 && a->color_in) return "pcv_sort_records: color_stride must be 3 or 4";
  const bool rec12 = compact && a->nwords <= 1;
  const bool rows = a->rows_mode != PCV_SORT_ROWS_NONE;
  if (a->map && a->map_entries == 0) return "pcv_sort_records: a map without entries";
  if (a->map && a->vec_bytes == 0) return "pcv_sort_records: the map is applied to records with a payload word only";
  if (rows && !(a->map && rec12)) return "pcv_sort_records: rows need a map and 12-byte records with at most one plane";
  if (rows && a->map_entries > (1u << 18)) return "pcv_sort_records: rows of more than 2^18 ranks";
  if (a->color_in && !rows) return "pcv_sort_records: color_in is read by the first pass of the rows form only";
  if (a->plane0_in && a->nwords == 0) return "pcv_sort_records: plane0_in without a plane";
  const bool packed = (a->flags & PCV_SORT_RECORDS_PACKED) != 0;
  if (packed && !(rows && compact && a->nwords == 0 && a->color_in && a->map_entries <= kPcvPackedRanks))
    return "pcv_sort_records: packed records need vec_bytes 8, no plane, rows, color_in and a map of <= 65 536 entries";
  if (a->n != 0) {
    if (!a->keys) return "pcv_sort_records: keys is null";
    if (a->vec_bytes != 0 && !a->vec) return "pcv_sort_records: vec is null";
    for (int w = 0; w < a->nwords; ++w)
      if (!a->planes[w]) return "pcv_sort_records: a plane is null";
    if (a->rows_mode == PCV_SORT_ROWS_GIVEN && !a->rows) return "pcv_sort_records: rows is null";
  }
  PcvSortFacts f;
  const int base = compact ? 8 : 0;
  f.n = a->n, f.key_bytes = 4, f.begin_bit = base, f.end_bit = base + a->key_bits;
  f.vec_in = a->vec_bytes != 0, f.vec_bytes = a->vec_bytes ? a->vec_bytes : 16, f.nwords = a->nwords, f.color_in = a->color_in != nullptr;
  f.color_stride = (int)a->color_stride, f.packed = packed;
  f.map = a->map != nullptr, f.map_entries = a->map ? a->map_entries : 0, f.rows = rows, f.second = a->map && a->hold_second;
  f.sort_rows2 = sw.sort_rows2, f.sort_msd = sw.sort_msd, f.rows_true_bins = sw.rows_true_bins;
  if (const char* why = pcv_sort_plan(f, plan)) return why;
  // the map in LDS is a table of half words: 15 bits of true rank and the replay mark
  if (plan->npasses && plan->pass[0].MAP == 1 && a->key_bits > 15)
    return "pcv_sort_records: a map of so few entries travels as half words: key_bits must be <= 15";
  *facts = f;
  return nullptr;
}

const char* pcv_sort_records_check_packed(const uint32_t* vec, uint64_t n, uint32_t map_entries) {
  for (uint64_t i = 0; i < n; ++i)
    if ((vec[2 * i + 1] >> 16) >= map_entries) return "pcv_sort_records: a record's predicted rank lies outside the map";
  return nullptr;
}

const char* pcv_sort_records_check_keys(const uint32_t* keys, uint64_t n, int vec_bytes, uint32_t map_entries) {
  const int shift = vec_bytes == 8 ? 8 : 0;
  for (uint64_t i = 0; i < n; ++i)
    if ((keys[i] >> shift) >= map_entries) return "pcv_sort_records: a key's predicted rank lies outside the map";
  return nullptr;
}

void pcv_sort_records_plan_info(const PcvSortPlan& plan, pcv_sort_plan_info* out) {
  *out = pcv_sort_plan_info{};
  out->npasses = plan.npasses;
  out->two_pass = plan.two_pass, out->held_back = plan.held_back;
  out->pieces = plan.pieces, out->blocks = plan.blocks, out->gpb = plan.gpb;
  out->groups = plan.geom.groups, out->chunk = plan.geom.chunk;
  for (int k = 0; k < plan.npasses; ++k) {
    const PcvSortPass& p = plan.pass[k];
    pcv_sort_pass_info& o = out->pass[k];
    o.shift = p.shift, o.nbits = p.nbits, o.hist = (int32_t)p.hist, o.down = (int32_t)p.down;
    o.R = p.R, o.MAP = p.MAP, o.PL = p.PL, o.map_lds = p.map_lds, o.dyn_lds = p.dyn_lds;
  }
}
