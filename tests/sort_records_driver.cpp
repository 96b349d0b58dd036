// Stand-alone driver of csrc/pcv_sort_records_check.cpp — the host-only part of pcv_sort_records: what it refuses and the plan
// it hands back — for tests/test_sort_records_cpu.py (built with ASan + UBSan, no HIP, no library). One call per input line:
//   n key_bits vec_bytes nwords map_entries rows_mode hold_second color_stride first_in0 null_mask mem
// map_entries 0: no map; color_stride 0: no color_in; null_mask: bit 0 keys, 1 vec, 2 the last plane, 3 rows are null.
// The arrays are never read by the check: every non-null pointer is the same small block. Prints the plan (pcv_sort_plan_info) or
// the refusal as JSON lines. `keys`: the key check over a few hand-made arrays.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../point_cloud_viewer_amd/csrc/pcv_sort_records_check.h"

static int key_checks() {
  std::vector<uint32_t> k = {0u, 5u << 8, 299u << 8 | 0xffu, 17u << 8};
  int bad = 0;
  bad += pcv_sort_records_check_keys(k.data(), k.size(), 8, 300) != nullptr;         // all inside
  bad += pcv_sort_records_check_keys(k.data(), k.size(), 8, 299) == nullptr;         // 299 is outside a map of 299 entries
  bad += pcv_sort_records_check_keys(k.data(), k.size(), 16, 76800) != nullptr;      // without a colour byte the whole key counts
  bad += pcv_sort_records_check_keys(k.data(), k.size(), 16, 76799) == nullptr;
  bad += pcv_sort_records_check_keys(k.data(), 0, 16, 1) != nullptr;                 // no keys
  bad += pcv_sort_records_check_keys(nullptr, 0, 8, 1) != nullptr;
  printf("{\"key_checks_failed\":%d}\n", bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (std::string(argv[1]) == "keys") return key_checks();
  std::ifstream in(argv[1]);
  if (!in) return 2;
  uint32_t block[8] = {};
  unsigned long long n;
  while (in >> n) {
    pcv_sort_records_args a{};
    int rows_mode, hold, first_in0, nulls, mem;
    unsigned stride, entries;
    if (!(in >> a.key_bits >> a.vec_bytes >> a.nwords >> entries >> rows_mode >> hold >> stride >> first_in0 >> nulls >> mem)) return 3;
    a.n = n, a.map_entries = entries, a.rows_mode = rows_mode, a.hold_second = hold, a.mem = mem;
    a.keys = nulls & 1 ? nullptr : block;
    a.vec = a.vec_bytes && !(nulls & 2) ? block : nullptr;
    for (int w = 0; w < a.nwords && w < 8; ++w) a.planes[w] = (nulls & 4) && w == a.nwords - 1 ? nullptr : block;
    a.map = entries ? block : nullptr;
    a.rows = rows_mode == PCV_SORT_ROWS_GIVEN && !(nulls & 8) ? block : nullptr;
    a.color_in = stride ? (const uint8_t*)block : nullptr;
    a.color_stride = stride ? stride : 3;
    a.plane0_in = first_in0 ? block : nullptr;
    PcvSortFacts f;
    PcvSortPlan plan;
    const char* why = pcv_sort_records_check(&a, PcvSortRecordsSwitches(), &f, &plan);
    if (why) {
      printf("{\"error\":\"%s\"}\n", why);
      continue;
    }
    pcv_sort_plan_info o;
    pcv_sort_records_plan_info(plan, &o);
    printf("{\"npasses\":%d,\"two_pass\":%d,\"held_back\":%d,\"pieces\":%d,\"blocks\":%d,\"gpb\":%d,\"groups\":%d,\"chunk\":%llu,"
           "\"begin\":%d,\"end\":%d,\"passes\":[",
           o.npasses, o.two_pass, o.held_back, o.pieces, o.blocks, o.gpb, o.groups, (unsigned long long)o.chunk, f.begin_bit, f.end_bit);
    for (int k = 0; k < o.npasses; ++k) {
      const pcv_sort_pass_info& p = o.pass[k];
      printf("%s{\"shift\":%d,\"nbits\":%d,\"hist\":%d,\"down\":%d,\"R\":%d,\"MAP\":%d,\"PL\":%d,\"map_lds\":%d,\"dyn_lds\":%llu}", k ? "," : "",
             p.shift, p.nbits, p.hist, p.down, p.R, p.MAP, p.PL, p.map_lds, (unsigned long long)p.dyn_lds);
    }
    printf("]}\n");
  }
  pcv_sort_records_args none{};
  none.mem = 7;
  PcvSortFacts f;
  PcvSortPlan plan;
  printf("{\"null_args\":%d,\"bad_mem\":%d}\n", pcv_sort_records_check(nullptr, PcvSortRecordsSwitches(), &f, &plan) != nullptr,
         pcv_sort_records_check(&none, PcvSortRecordsSwitches(), &f, &plan) != nullptr);
  return 0;
}
