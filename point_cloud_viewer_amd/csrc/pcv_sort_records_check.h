// pcv_sort_records_check.h — the host-only part of pcv_sort_records (pcv_stage_api.hip): what the entry refuses before it
// touches anything, the facts and the plan of the sort it will run, and the plan as the entry hands it back. Standard C++, no
// HIP header, so that it can be built and run under sanitizers on a machine without a GPU (tests/test_sort_records_cpu.py).
#pragma once
#include "../../include/pcv_hip.h"
#include "pcv_sort_plan.h"

// the library's switches that shape a plan (PcvSwitches; the defaults are what libpcv_hip.so runs with)
struct PcvSortRecordsSwitches {
  bool sort_rows2 = true, sort_msd = false;
  uint32_t rows_true_bins = 0;
};

// Returns null and fills *facts and *plan, or the reason why the call is refused. Reads no array.
const char* pcv_sort_records_check(const pcv_sort_records_args* a, const PcvSortRecordsSwitches& sw, PcvSortFacts* facts,
                                   PcvSortPlan* plan);
// PCV_SORT_RECORDS_CHECK_KEYS: every predicted rank of `keys` (host memory) lies inside the map. Null, or the reason.
const char* pcv_sort_records_check_keys(const uint32_t* keys, uint64_t n, int vec_bytes, uint32_t map_entries);
// ... of packed records (PCV_SORT_RECORDS_PACKED: the rank sits in the upper half of a record's second word)
const char* pcv_sort_records_check_packed(const uint32_t* vec, uint64_t n, uint32_t map_entries);
void pcv_sort_records_plan_info(const PcvSortPlan& plan, pcv_sort_plan_info* out);
