// Stand-alone driver of pcv_png_decode for a sanitizer build (tests/test_xray_merge_cpu.py compiles it with the decoder
// and -fsanitize=address,undefined): argv[1] is a valid RGBA8 PNG. Every truncation, every single-byte flip and 1 000
// seeded random mutations (half of them with the chunk CRCs made right again, so that the damage reaches the inflate and
// the row filters) go through the decoder with an output buffer of exactly the size the valid file needs. The driver
// checks that nothing but PCV_OK, PCV_E_INVALID and PCV_E_IO comes back; the sanitizers check the rest.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcv_hip.h"

static uint32_t crc32_of(const uint8_t* p, size_t n) {
  uint32_t crc = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = crc & 1 ? 0xedb88320u ^ (crc >> 1) : crc >> 1;
  }
  return crc ^ 0xffffffffu;
}

// rewrites the CRC of every chunk whose length field still fits the file
static void fix_crcs(std::vector<uint8_t>& f) {
  size_t pos = 8;
  while (f.size() >= 12 && pos <= f.size() - 12) {
    const uint32_t n = (uint32_t)f[pos] << 24 | (uint32_t)f[pos + 1] << 16 | (uint32_t)f[pos + 2] << 8 | f[pos + 3];
    if (n > f.size() - pos - 12) return;
    const uint32_t c = crc32_of(f.data() + pos + 4, 4 + (size_t)n);
    uint8_t* o = f.data() + pos + 8 + n;
    o[0] = (uint8_t)(c >> 24), o[1] = (uint8_t)(c >> 16), o[2] = (uint8_t)(c >> 8), o[3] = (uint8_t)c;
    pos += 12 + (size_t)n;
  }
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static size_t capacity = 0;
static int runs = 0, oks = 0;
static bool decode(const std::vector<uint8_t>& f) {
  // copies of exactly the sizes in play: a read past the input or a write past the capacity is a sanitizer report
  std::vector<uint8_t> in(f), out(capacity);
  uint32_t w = 0, h = 0;
  const int rc = pcv_png_decode(in.data(), in.size(), &w, &h, out.data(), out.size());
  ++runs;
  oks += rc == PCV_OK;
  if (rc != PCV_OK && rc != PCV_E_INVALID && rc != PCV_E_IO) {
    std::fprintf(stderr, "unexpected status %d\n", rc);
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  std::vector<uint8_t> good;
  uint8_t buf[4096];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof(buf), fp)) > 0) good.insert(good.end(), buf, buf + k);
  std::fclose(fp);
  uint32_t w = 0, h = 0;
  if (pcv_png_decode(good.data(), good.size(), &w, &h, nullptr, 0) != PCV_OK) return 3;
  capacity = 4 * (size_t)w * h;
  if (!decode(good) || oks != 1) return 3;
  for (size_t n = 0; n < good.size(); ++n)  // truncations
    if (!decode(std::vector<uint8_t>(good.begin(), good.begin() + (long)n))) return 4;
  for (size_t i = 0; i < good.size(); ++i)  // one byte flipped, with and without the CRCs made right
    for (int fix = 0; fix < 2; ++fix) {
      std::vector<uint8_t> f(good);
      f[i] ^= (uint8_t)(1u << (i % 8));
      if (fix) fix_crcs(f);
      if (!decode(f)) return 5;
    }
  for (int m = 0; m < 1000; ++m) {  // random mutations
    std::vector<uint8_t> f(good);
    const int edits = 1 + (int)(rnd() % 4);
    for (int e = 0; e < edits; ++e) f[rnd() % f.size()] = (uint8_t)rnd();
    if (rnd() & 1) f.resize(1 + rnd() % f.size());
    if (m & 1) fix_crcs(f);
    if (!decode(f)) return 6;
  }
  std::printf("%d decodes, %d accepted\n", runs, oks);
  return 0;
}
