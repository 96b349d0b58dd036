// Stand-alone driver of the LAS host code for a sanitizer build (tests/test_las_cpu.py compiles it with csrc/pcv_las.cpp and
// -fsanitize=address,undefined; no library involved): argv[1] is a valid LAS file, argv[2] a scratch path. The header parser and
// the host reader run over the valid file, every truncation of its first 400 bytes, every single-byte flip of the header and
// 1 000 seeded random flips anywhere in the file. The driver checks that nothing but PCV_OK, PCV_E_INVALID and PCV_E_IO comes
// back and that a result holds as many points as its info says; the sanitizers check the rest.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pcv_las.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static const char* scratch = nullptr;
static int runs = 0, oks = 0;

static bool status_ok(int rc) {
  if (rc == PCV_OK || rc == PCV_E_INVALID || rc == PCV_E_IO) return true;
  std::fprintf(stderr, "unexpected status %d\n", rc);
  return false;
}

static bool run_case(const std::vector<uint8_t>& f) {
  std::FILE* fp = std::fopen(scratch, "wb");
  if (!fp) return false;
  if (!f.empty() && std::fwrite(f.data(), 1, f.size(), fp) != f.size()) return false;
  std::fclose(fp);
  ++runs;
  // the parser over a copy of exactly the bytes there are: a read past them is a sanitizer report
  std::vector<uint8_t> head(f.begin(), f.begin() + (long)(f.size() < kLasMaxHeader ? f.size() : kLasMaxHeader));
  pcv_las_header h;
  std::string why;
  const int rc = pcv_las_parse_header(head.data() ? head.data() : (const uint8_t*)"", head.size(), f.size(), &h, &why);
  if (!status_ok(rc) || (rc != PCV_OK && why.empty())) return false;
  pcv_las_header h2;
  if (pcv_las_read_header(scratch, &h2, &why) != rc) return false;
  // the reader: every extra the (possibly changed) format has, intensity kept, colour by AUTO; then a filter and a transform
  for (int pass = 0; pass < 2; ++pass) {
    pcv_las_params p{};
    p.keep_intensity = 1;
    if (rc == PCV_OK) {
      const PcvLasFormat fm = pcv_las_format(h.point_format);
      for (uint32_t id = 0; id < kLasNumExtras; ++id)
        if (pcv_las_format_has(fm, id)) p.extras[p.num_extras++] = pcv_las_extra_name(id);
    }
    if (pass == 1) {
      p.class_mask[0] = 0x5555555555555555ull, p.drop_withheld = 1, p.use_transform = 1, p.color_mode = PCV_LAS_COLOR_INTENSITY;
      const double iso[7] = {1e6, -2e6, 3e6, 0.5, 0.5, 0.5, 0.5};
      std::memcpy(p.global_from_local, iso, sizeof(iso));
    }
    pcv_las* las = nullptr;
    const int rr = pcv_las_read_file(scratch, &p, &las, &why);
    if (!status_ok(rr) || (rr == PCV_OK) != (las != nullptr)) return false;
    if (rr == PCV_OK) {
      if (rc != PCV_OK || las->n != las->info.num_kept || las->x.size() != las->n || las->color.size() != 3 * las->n) return false;
      oks += pass == 0;
      delete las;
    } else if (rc == PCV_OK && rr != PCV_E_INVALID) {
      return false;  // the header was fine and the file long enough: only the params can be refused
    }
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  scratch = argv[2];
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  std::vector<uint8_t> good;
  uint8_t buf[4096];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof(buf), fp)) > 0) good.insert(good.end(), buf, buf + k);
  std::fclose(fp);
  if (good.size() < 400) return 2;
  if (!run_case(good) || oks != 1) return 3;
  pcv_las_header h;
  std::string why;
  if (pcv_las_parse_header(good.data(), good.size(), good.size(), &h, &why) != PCV_OK) return 3;
  for (size_t n = 0; n < 400; ++n)  // truncations
    if (!run_case(std::vector<uint8_t>(good.begin(), good.begin() + (long)n))) return 4;
  for (size_t i = 0; i < h.header_size; ++i) {  // one byte of the header flipped
    std::vector<uint8_t> f(good);
    f[i] ^= (uint8_t)(1u << (i % 8));
    if (!run_case(f)) return 5;
  }
  for (int m = 0; m < 1000; ++m) {  // random flips, half of them inside the header, some with the file cut as well
    std::vector<uint8_t> f(good);
    const int edits = 1 + (int)(rnd() % 4);
    for (int e = 0; e < edits; ++e) f[rnd() % (m & 1 ? h.header_size : f.size())] ^= (uint8_t)(1u << (rnd() % 8));
    if (rnd() % 8 == 0) f.resize(1 + rnd() % f.size());
    if (!run_case(f)) return 6;
  }
  std::printf("%d cases, %d accepted\n", runs, oks);
  return 0;
}
