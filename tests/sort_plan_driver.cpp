// Stand-alone driver of csrc/pcv_sort_plan.cpp for tests/test_sort_plan_cpu.py (built with ASan + UBSan, no HIP, no library):
// prints the plan of a radix sort, the scratch layout and the map-in-LDS / settle tables as JSON lines, the facts they were made
// from included.
//   sort_plan_driver sweep         every n, bit count, payload shape, map size and switch set of the test's sweep
//   sort_plan_driver <file>        one sort per line: n key_bytes begin_bit end_bit vec_in vec_bytes nwords color_in map
//                                  map_entries rows second sort_rows2 sort_msd rows_true_bins
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include "../point_cloud_viewer_amd/csrc/pcv_sort_plan.h"

static void print_plan(const PcvSortFacts& f) {
  PcvSortPlan p;
  const char* why = pcv_sort_plan(f, &p);
  printf("{\"n\":%llu,\"key_bytes\":%d,\"begin\":%d,\"end\":%d,\"vec_in\":%d,\"vec_bytes\":%d,\"nwords\":%d,\"color_in\":%d,\"map\":%d,"
         "\"map_entries\":%u,\"rows\":%d,\"second\":%d,\"sort_rows2\":%d,\"sort_msd\":%d,\"bins\":%u,",
         (unsigned long long)f.n, f.key_bytes, f.begin_bit, f.end_bit, f.vec_in, f.vec_bytes, f.nwords, f.color_in, f.map, f.map_entries,
         f.rows, f.second, f.sort_rows2, f.sort_msd, f.rows_true_bins);
  if (why) {
    printf("\"error\":\"%s\"}\n", why);
    return;
  }
  printf("\"records\":%d,\"compact\":%d,\"with_plane\":%d,\"rec12\":%d,\"groups\":%d,\"chunk\":%llu,\"two_pass\":%d,\"msd\":%d,\"blocks\":%d,"
         "\"gpb\":%d,\"pieces\":%d,\"held_back\":%d,\"result_in_a\":%d,\"passes\":[",
         p.records, p.compact, p.with_plane, p.rec12, p.geom.groups, (unsigned long long)p.geom.chunk, p.two_pass, p.msd, p.blocks, p.gpb,
         p.pieces, p.held_back, p.result_in_a);
  for (int k = 0; k < p.npasses; ++k) {
    const PcvSortPass& q = p.pass[k];
    const PcvSortMapLds lds = pcv_sort_map_lds(q.PL, q.R);
    printf("%s{\"shift\":%d,\"nbits\":%d,\"hist\":%d,\"plain_add\":%d,\"map_lds\":%d,\"down\":%d,\"R\":%d,\"PL\":%d,\"MAP\":%d,\"dyn_lds\":%zu,"
           "\"lds_entries\":%u,\"lds_attr\":%u}",
           k ? "," : "", q.shift, q.nbits, (int)q.hist, q.plain_add, q.map_lds, (int)q.down, q.R, q.PL, q.MAP, q.dyn_lds, lds.max_entries,
           lds.attr_bytes);
  }
  printf("]");
  if (p.two_pass)  // the held-back pass's settle eligibility, with and without the octree's intensity blob, and its form
    printf(",\"settles\":%d,\"settles_without_blob\":%d,\"settle_form\":%d", pcv_sort_second_settles(p.pass[1].nbits, p.with_plane, true),
           pcv_sort_second_settles(p.pass[1].nbits, p.with_plane, false), (int)pcv_sort_settle_form(p.pass[1].nbits, p.with_plane));
  printf("}\n");
}

static void print_scratch(uint64_t n, uint32_t forced) {
  const PcvSortScratch s = pcv_sort_scratch(n, forced);
  printf("{\"scratch\":[%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu],\"n\":%llu,\"bins\":%u,\"bytes\":%zu,\"groups8192\":%d,\"rows_true_bins\":%u}\n", s.hist,
         s.totals, s.hist2, s.totals2, s.ranges, s.order, s.rows_true, s.end, (unsigned long long)n, forced, s.end + kPcvSortScratchSlack,
         pcv_sort_geom(n, kPcvSortRec12Tile).groups, pcv_sort_rows_true_bins(n, forced));
}

static void sweep() {
  const uint64_t ns[] = {1, 4095, 4096, 4097, 8209, 65535, 65536, 200000, 100000000ull, 200000000ull, 500000000ull, 0xfffffffeull};
  const uint32_t maps[] = {0, 1, 4999, 5000, 5001, 10000, 10001, 16384, 16385, 32768, 65536};
  struct Shape { bool vec; int vec_bytes, nwords; };
  const Shape other[] = {{false, 16, 1}, {false, 16, 8}, {true, 16, 0}, {true, 16, 1}, {true, 16, 4}, {true, 8, 2}, {true, 8, 4}};
  struct Switches { bool rows2, msd; uint32_t bins; };
  const Switches sw[] = {{true, false, 0}, {false, false, 0}, {true, true, 0}, {true, false, 32768}, {true, false, 65536}};
  for (uint64_t n : ns) {
    for (uint32_t forced : {0u, 32768u, 65536u}) print_scratch(n, forced);
    for (int kb : {8, 4})  // keys only
      for (int bits = 1; bits <= kb * 8; ++bits) {
        PcvSortFacts f;
        f.n = n, f.key_bytes = kb, f.end_bit = bits;
        print_plan(f);
      }
    for (const Shape& s : other)  // records of the 256-lane kernels, plain and with the map in the first upsweep
      for (int bits = 1; bits <= 32; ++bits)
        for (uint32_t me : {0u, 5000u, 15001u}) {
          PcvSortFacts f;
          f.n = n, f.end_bit = bits, f.vec_in = s.vec, f.vec_bytes = s.vec_bytes, f.nwords = s.nwords;
          f.map = me != 0, f.map_entries = me;
          print_plan(f);
        }
    for (int plane = 0; plane < 2; ++plane)  // 12-byte records: the rank in bits 8.. of the key
      for (int color = 0; color < 2; ++color)
        for (int bits = 1; bits <= 24; ++bits)
          for (int form = 0; form < 4; ++form)  // no map; map; map + rows; map + rows + second
            for (uint32_t me : maps)
              for (const Switches& w : sw) {
                if (form == 0 && (me != 0 || w.bins != 0 || w.msd || !w.rows2)) continue;
                if (color && (w.bins != 0 || w.msd || !w.rows2)) continue;  // (the colour's source changes no pass: default switches only)
                PcvSortFacts f;
                f.n = n, f.begin_bit = 8, f.end_bit = 8 + bits, f.vec_in = true, f.vec_bytes = 8, f.nwords = plane, f.color_in = color != 0;
                f.map = form >= 1, f.map_entries = me, f.rows = form >= 2, f.second = form >= 3;
                f.sort_rows2 = w.rows2, f.sort_msd = w.msd, f.rows_true_bins = w.bins;
                print_plan(f);
              }
  }
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (std::string(argv[1]) == "sweep") {
    sweep();
    return 0;
  }
  std::ifstream in(argv[1]);
  if (!in) return 2;
  unsigned long long n;
  while (in >> n) {
    PcvSortFacts f;
    int vec, color, map, rows, second, rows2, msd;
    f.n = n;
    if (!(in >> f.key_bytes >> f.begin_bit >> f.end_bit >> vec >> f.vec_bytes >> f.nwords >> color >> map >> f.map_entries >> rows >> second >>
          rows2 >> msd >> f.rows_true_bins))
      return 3;
    f.vec_in = vec, f.color_in = color, f.map = map, f.rows = rows, f.second = second, f.sort_rows2 = rows2, f.sort_msd = msd;
    print_plan(f);
    print_scratch(f.n, f.rows_true_bins);
  }
  return 0;
}
