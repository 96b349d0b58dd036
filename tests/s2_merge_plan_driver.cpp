// Stand-alone driver of csrc/pcv_s2_merge_plan.cpp (no HIP, no library; tests/test_s2_merge_plan_cpu.py builds it with
// -fsanitize=address,undefined). argv[1] is a file of cases, whitespace-separated integers:
//   chunk_points num_parts, then per part: num_cells, then num_cells pairs "id count"
// For every case one block of lines: "plan <rc> <n>", then "ids ...", "counts ...", "offsets ...", "segments" with four numbers
// per segment (dst_offset src_offset part count), "chunks ...". A refused case prints "plan <rc> 0" and the reason.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <vector>

#include "../point_cloud_viewer_amd/csrc/pcv_s2_merge_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  uint64_t chunk_points, num_parts;
  int cases = 0;
  while (in >> chunk_points >> num_parts) {
    std::vector<std::vector<uint64_t>> ids(num_parts), counts(num_parts);
    for (uint64_t p = 0; p < num_parts; ++p) {
      uint64_t cells;
      if (!(in >> cells)) return 3;
      ids[p].resize(cells), counts[p].resize(cells);
      for (uint64_t k = 0; k < cells; ++k)
        if (!(in >> ids[p][k] >> counts[p][k])) return 3;
    }
    std::vector<PcvS2MergePart> parts(num_parts);
    for (uint64_t p = 0; p < num_parts; ++p) parts[p] = PcvS2MergePart{ids[p].data(), counts[p].data(), ids[p].size()};
    PcvS2MergePlan plan;
    std::string why;
    const int rc = pcv_s2_merge_plan(parts.data(), (uint32_t)num_parts, (uint32_t)chunk_points, &plan, &why);
    std::cout << "plan " << rc << " " << plan.n << "\n";
    if (rc != PCV_OK) {
      std::cout << why << "\n";
    } else {
      auto row = [](const char* name, const std::vector<uint64_t>& v) {
        std::cout << name;
        for (uint64_t x : v) std::cout << " " << x;
        std::cout << "\n";
      };
      row("ids", plan.ids), row("counts", plan.counts), row("offsets", plan.offsets);
      std::cout << "segments";
      for (const pcv_s2_merge_segment& s : plan.segments) std::cout << " " << s.dst_offset << " " << s.src_offset << " " << s.part << " " << s.count;
      std::cout << "\n";
      row("chunks", plan.chunk_first_segment);
    }
    ++cases;
  }
  std::cout << "cases " << cases << "\n";
  return 0;
}
