// Stand-alone driver of csrc/pcv_sort_plan.cpp for tests/test_sort_plan_packed_cpu.py (ASan + UBSan, no HIP, no library): the
// plan of the record sort's first pass where the records come without their colour — packed 8-byte records, or 12-byte records
// with color_in — with the LDS the pass would be launched with, and the hand-over rule of the single-chain build.
//   sort_plan_packed_driver <file>   one sort per line: n bits map_entries plane packed color_stride rows
//   sort_plan_packed_driver rule     pcv_packed_handover_tried / pcv_packed_handover over their arguments
#include <cstdio>
#include <fstream>
#include <string>

#include "../point_cloud_viewer_amd/csrc/pcv_sort_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (std::string(argv[1]) == "rule") {
    for (int sw = 0; sw < 2; ++sw)
      for (int compact = 0; compact < 2; ++compact)
        for (int routed = 0; routed < 2; ++routed)
          for (int inten = 0; inten < 2; ++inten)
            printf("{\"switch\":%d,\"compact\":%d,\"routed\":%d,\"intensity\":%d,\"tried\":%d}\n", sw, compact, routed, inten,
                   pcv_packed_handover_tried(sw, compact, routed, inten));
    for (uint32_t nodes : {1u, 65535u, 65536u, 65537u, 1u << 20})
      printf("{\"nodes\":%u,\"packed\":%d}\n", nodes, pcv_packed_handover(nodes));
    for (int R : {128, 256})
      for (int stride : {3, 4})
        printf("{\"R\":%d,\"stride\":%d,\"static\":%u,\"buffer\":%u,\"staged_entries\":%u,\"attr\":%u}\n", R, stride,
               pcv_sort_rec12_static_lds(false, R), pcv_sort_color_buffer(stride), pcv_sort_map_lds_staged(R, stride), pcv_sort_rec12_dyn_attr(R));
    return 0;
  }
  std::ifstream in(argv[1]);
  if (!in) return 2;
  unsigned long long n;
  while (in >> n) {
    int bits, plane, packed, stride, rows;
    PcvSortFacts f;
    if (!(in >> bits >> f.map_entries >> plane >> packed >> stride >> rows)) return 3;
    f.n = n, f.begin_bit = 8, f.end_bit = 8 + bits, f.vec_in = true, f.vec_bytes = 8, f.nwords = plane;
    f.color_in = true, f.color_stride = stride, f.packed = packed != 0;
    f.map = true, f.rows = rows != 0, f.second = true;
    PcvSortPlan p;
    const char* why = pcv_sort_plan(f, &p);
    printf("{\"n\":%llu,\"bits\":%d,\"map_entries\":%u,\"plane\":%d,\"packed\":%d,\"stride\":%d,\"rows\":%d,", n, bits, f.map_entries, plane, packed,
           stride, rows);
    if (why) {
      printf("\"error\":\"%s\"}\n", why);
      continue;
    }
    const PcvSortPass& q = p.pass[0];
    // what the launch asks for: the form's static part + the map + the colours' buffer
    const unsigned long long lds = (unsigned long long)pcv_sort_rec12_static_lds(q.PL, q.R) + q.dyn_lds + q.color_lds;
    printf("\"R\":%d,\"PL\":%d,\"MAP\":%d,\"dyn_lds\":%zu,\"color_lds\":%zu,\"pass_packed\":%d,\"lds\":%llu,\"two_pass\":%d,\"later_color_lds\":%zu}\n",
           q.R, q.PL, q.MAP, q.dyn_lds, q.color_lds, q.packed, lds, p.two_pass, p.npasses > 1 ? p.pass[1].color_lds : (size_t)0);
  }
  return 0;
}
