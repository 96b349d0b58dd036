// Stand-alone driver of csrc/pcv_levels.cpp for tests/test_levels_cpu.py (built with ASan + UBSan, no HIP, no library):
// reads cases from the file named on the command line, calls pcv_make_levels (with and without `lv`), pcv_level_table,
// pcv_level_shortcuts and pcv_promote_assign, and prints what they return. Doubles travel as C99 hex floats both ways.
//   levels  <name> <min x y z> <max x y z> <resolution> <cap>
//   promote <name> <n> <with_slots> <m> then per node: id_high id_low first count level parent first_child child_mask is_leaf
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../point_cloud_viewer_amd/csrc/pcv_levels.h"

static double next_double(std::istream& in) {
  std::string tok;
  in >> tok;
  return strtod(tok.c_str(), nullptr);
}
static uint64_t next_u64(std::istream& in) {
  std::string tok;
  in >> tok;
  return strtoull(tok.c_str(), nullptr, 0);
}

static int run_levels(std::istream& in, const std::string& name) {
  double bmin[3], bmax[3];
  for (double& v : bmin) v = next_double(in);
  for (double& v : bmax) v = next_double(in);
  const double resolution = next_double(in);
  const int cap = (int)next_u64(in);
  printf("case %s\n", name.c_str());
  // the C entry point: levels 0..ml into arrays of cap + 2
  std::vector<double> edge(cap + 2, -1.0);
  std::vector<int32_t> enc(cap + 2, -1);
  const int ml = pcv_level_table(bmin, bmax, resolution, cap, edge.data(), enc.data());
  printf("table %d\n", ml);
  for (int k = 0; k <= ml; ++k) printf("L %d %a %d\n", k, edge[k], enc[k]);
  // without lv: the vectors alone must say the same
  std::vector<double> e;
  std::vector<int32_t> c;
  int ml2 = -1;
  if (pcv_make_levels(bmin, bmax, resolution, cap, nullptr, &ml2, &e, &c) != PCV_OK) return 1;
  if (ml2 != ml || (int)e.size() != ml + 1 || (int)c.size() != ml + 1) return 1;
  for (int k = 0; k <= ml; ++k)
    if (c[k] != enc[k] || std::memcmp(&e[k], &edge[k], 8) != 0) return 1;
  // with lv, and no other output
  PcvLevels lv;
  int ml3 = -1;
  if (pcv_make_levels(bmin, bmax, resolution, cap, &lv, &ml3, nullptr, nullptr) != PCV_OK || ml3 != ml) return 1;
  printf("lv %d %d %d %d %d %d %d\n", lv.nlevels, lv.fast_ok, lv.first_f32, lv.first_u16, lv.first_u8, lv.code_begin, lv.code_end);
  for (int k = 0; k < PCV_MAX_LEVELS + 2; ++k)
    printf("M %d %a %a %a %u %a %u\n", k, lv.edge[k], lv.inv_edge[k], lv.inv_edge_lo[k], lv.enc[k], lv.digit_half[k], lv.digit_mode[k]);
  for (int k = 0; k < PCV_MAX_KEY_LEVELS + 2; ++k) printf("T %d %u\n", k, lv.code_thr_hi[k]);
  // with everything at once: the same table again
  PcvLevels lv2;
  if (pcv_make_levels(bmin, bmax, resolution, cap, &lv2, nullptr, &e, &c) != PCV_OK || std::memcmp(&lv, &lv2, sizeof(lv)) != 0) return 1;
  uint32_t mode[PCV_MAX_KEY_LEVELS + 2];
  double thr[PCV_MAX_KEY_LEVELS + 2];
  const int ml4 = pcv_level_shortcuts(bmin, bmax, resolution, mode, thr);
  printf("shortcuts %d\n", ml4);
  for (int k = 0; k < PCV_MAX_KEY_LEVELS + 2; ++k) printf("S %d %u %a\n", k, mode[k], thr[k]);
  return 0;
}

static int run_promote(std::istream& in, const std::string& name) {
  const uint64_t n = next_u64(in);
  const bool with_slots = next_u64(in) != 0;
  const uint64_t m = next_u64(in);
  std::vector<pcv_split_node> nodes(m);
  for (pcv_split_node& nd : nodes) {
    nd.id_high = next_u64(in);
    nd.id_low = next_u64(in);
    nd.first = next_u64(in);
    nd.count = next_u64(in);
    nd.level = (uint32_t)next_u64(in);
    nd.parent = (uint32_t)next_u64(in);
    nd.first_child = (uint32_t)next_u64(in);
    nd.child_mask = (uint32_t)next_u64(in);
    nd.is_leaf = (uint32_t)next_u64(in);
    nd.reserved = 0;
  }
  std::vector<pcv_promote_node> per(m);
  std::vector<uint32_t> node_of(with_slots ? n : 0, 0xffffffffu), slot_in(with_slots ? n : 0, 0xffffffffu);
  const int rc = pcv_promote_assign(nodes.data(), m, per.data(), n, with_slots ? node_of.data() : nullptr, with_slots ? slot_in.data() : nullptr);
  printf("case %s\npromote %d\n", name.c_str(), rc);
  if (rc != PCV_OK) return 0;
  for (uint64_t i = 0; i < m; ++i)
    printf("P %llu %llu %llu %llu\n", (unsigned long long)i, (unsigned long long)per[i].stream_len, (unsigned long long)per[i].num_points,
           (unsigned long long)per[i].child_offset);
  for (uint64_t j = 0; j < node_of.size(); ++j) printf("Q %llu %u %u\n", (unsigned long long)j, node_of[j], slot_in[j]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string kind, name;
  while (in >> kind >> name) {
    int rc = 2;
    if (kind == "levels") rc = run_levels(in, name);
    if (kind == "promote") rc = run_promote(in, name);
    if (rc) {
      fprintf(stderr, "case %s failed (%d)\n", name.c_str(), rc);
      return rc;
    }
  }
  return 0;
}
