// pcv_switches.h — the A/B switches of the experiment library, in one table.
//
// libpcv_hip_exp.so (the same sources with -DPCV_EXPERIMENTS) reads each switch from the environment variable named in
// pcv_switches(), once per process: the tests of the alternative kernels and two tools under tools/ set them. In the
// shipped library pcv_switches() is a constant: every branch on a switch folds away and no environment variable is read.
// A field holds the value the shipped library uses; its comment says what the other value selects and who sets it.
#pragma once
#include <stdint.h>

struct PcvSwitches {
  bool code_steps = true;          // 0: every Float32 level step of the chain in full (test_gpu_single_chain)
  bool color_late = false;         // 1: the record sort's first pass fetches the colour, not the chain pass (test_gpu_single_chain)
  bool compact_records = true;     // 0: 20-byte records in the single-chain build (test_gpu_single_chain)
  bool packed_handover = true;     // 0: the chain pass hands the sort 12-byte records with their colour (test_gpu_packed_handover)
  int rec_wc = 0;                  // bit 0 / 1: write-combining downsweep in the record sort's first / second pass (test_gpu_single_chain)
  uint32_t rows_true_bins = 0;     // 32768 / 65536: the 15- / 16-bit rank geometry on a cloud of any size (test_gpu_single_chain)
  bool sample_counts = false;      // 1: the sample tree by counting the keys instead of sorting them (test_gpu_single_chain)
  bool sample_tree_split = false;  // 1: the sample tree by node split + scan / emit, fifteen launches (test_gpu_spec_tree)
  bool settle_by_leaf = true;      // 0: slot-wise settle and climb kernels, nothing settled by the sort (test_gpu_single_chain)
  bool settle_in_sort = true;      // 0: the record sort runs to its end, `settle` reads the records (test_gpu_single_chain)
  bool sort_msd = false;           // 1: the record sort takes the upper digit first (test_gpu_single_chain, tools/ab_msd.sh)
  bool sort_rows = true;           // 0: the sort's first pass counts and maps the keys in a pass of its own (test_gpu_single_chain)
  bool sort_rows2 = true;          // 0: the sort's second pass counts its keys itself (test_gpu_single_chain)
  bool split2 = true;              // 0: node split one level per launch pair; implies sample_tree_split (test_gpu_single_chain)
  uint64_t xray_accum_grid = 0;         // workgroups of the xray accumulation, 0: as many as are resident (test_gpu_xray)
  uint64_t xray_max_group_buckets = 0;  // buckets a group of xray tiles holds at most, 0: 2^30 (test_gpu_xray)
  uint64_t xray_sort_lds_records = 0;   // LDS bucket limit of the sorted xray accumulation, 0: the kernel's own (test_gpu_xray_intensity)
  bool spec_time = false;          // set: pcv_spec_simulate times pcv_spec_resolve (tools/spec_resolve_time.py)
  unsigned writer_threads = 0;     // threads that write the node files, 0: by the host's size (tools/e2e_probe.py)
};

#ifdef PCV_EXPERIMENTS
#include <stdlib.h>
inline const PcvSwitches& pcv_switches() {
  static const PcvSwitches table = [] {
    PcvSwitches s;
    const auto flag = [](const char* name, bool* v) {
      if (const char* e = getenv(name)) *v = atoi(e) != 0;
    };
    const auto at_least_one = [](const char* name, uint64_t* v) {
      if (const char* e = getenv(name)) *v = strtoull(e, nullptr, 10) > 1 ? strtoull(e, nullptr, 10) : 1;
    };
    flag("PCV_CODE_STEPS", &s.code_steps);
    flag("PCV_COLOR_LATE", &s.color_late);
    flag("PCV_COMPACT_RECORDS", &s.compact_records);
    flag("PCV_PACKED_HANDOVER", &s.packed_handover);
    if (const char* e = getenv("PCV_REC_WC")) s.rec_wc = atoi(e);
    if (const char* e = getenv("PCV_ROWS_TRUE_BINS")) s.rows_true_bins = (uint32_t)atoi(e);
    flag("PCV_SAMPLE_COUNTS", &s.sample_counts);
    flag("PCV_SAMPLE_TREE_SPLIT", &s.sample_tree_split);
    flag("PCV_SETTLE_BY_LEAF", &s.settle_by_leaf);
    flag("PCV_SETTLE_IN_SORT", &s.settle_in_sort);
    flag("PCV_SORT_MSD", &s.sort_msd);
    flag("PCV_SORT_ROWS", &s.sort_rows);
    flag("PCV_SORT_ROWS2", &s.sort_rows2);
    flag("PCV_SPLIT2", &s.split2);
    at_least_one("PCV_XRAY_ACCUM_GRID", &s.xray_accum_grid);
    at_least_one("PCV_XRAY_MAX_GROUP_BUCKETS", &s.xray_max_group_buckets);
    at_least_one("PCV_XRAY_SORT_LDS_RECORDS", &s.xray_sort_lds_records);
    s.spec_time = getenv("PCV_SPEC_TIME") != nullptr;
    if (const char* e = getenv("PCV_WRITER_THREADS")) s.writer_threads = (unsigned)(atoi(e) > 1 ? atoi(e) : 1);
    return s;
  }();
  return table;
}
#else
constexpr PcvSwitches pcv_switches() { return PcvSwitches{}; }
#endif
