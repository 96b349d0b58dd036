// Stand-alone driver of pcv_xray_png_encode_ex for a sanitizer build (tests/test_xray_png_cpu.py compiles it with
// pcv_png.cpp and -fsanitize=address,undefined). argv[1] is a file of tiles: u32 count, then per tile u32 w and w * w * 4
// bytes of RGBA8. Every tile, and 1 000 seeded tiles after them (sparse, banded and noisy, edges 1 .. 40), goes through both
// modes with `needed` asked first, an output buffer of exactly that size, a buffer one byte short (nothing may be
// written) and back through pcv_png_decode. The sanitizers check the reads and writes; the driver checks the answers.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcv_hip.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static int runs = 0;
static uint64_t raw_bytes = 0, deflate_bytes = 0;

static bool check(const std::vector<uint8_t>& px, uint32_t w, uint32_t h) {
  for (int mode = PCV_XRAY_PNG_STORED; mode <= PCV_XRAY_PNG_DEFLATE; ++mode) {
    std::vector<uint8_t> in(px);  // exactly the bytes of the image: a read past them is a sanitizer report
    uint64_t needed = 0, again = 0;
    if (pcv_xray_png_encode_ex(in.data(), w, h, mode, nullptr, 0, &needed) != PCV_OK || needed == 0) return false;
    if (needed > pcv_xray_png_bound(w, h, mode)) return false;
    std::vector<uint8_t> shy(needed - 1, 0xa5);
    if (pcv_xray_png_encode_ex(in.data(), w, h, mode, shy.data(), shy.size(), &again) != PCV_OK || again != needed) return false;
    for (uint8_t b : shy)
      if (b != 0xa5) return false;
    std::vector<uint8_t> file(needed);
    if (pcv_xray_png_encode_ex(in.data(), w, h, mode, file.data(), file.size(), &again) != PCV_OK || again != needed) return false;
    uint32_t dw = 0, dh = 0;
    std::vector<uint8_t> back(px.size());
    if (pcv_png_decode(file.data(), file.size(), &dw, &dh, back.data(), back.size()) != PCV_OK || dw != w || dh != h) return false;
    if (std::memcmp(back.data(), px.data(), px.size()) != 0) return false;
    if (mode == PCV_XRAY_PNG_STORED) {
      std::vector<uint8_t> old(needed);
      if (pcv_xray_png_encode(in.data(), w, h, old.data(), old.size(), &again) != PCV_OK || again != needed || old != file) return false;
    } else {
      raw_bytes += (uint64_t)h * (1 + 4ull * w);
      deflate_bytes += needed;
    }
    ++runs;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* fp = std::fopen(argv[1], "rb");
  if (!fp) return 2;
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, fp) != 1) return 2;
  for (uint32_t t = 0; t < count; ++t) {
    uint32_t w = 0;
    if (std::fread(&w, 4, 1, fp) != 1 || w == 0 || w > 4096) return 2;
    std::vector<uint8_t> px(4ull * w * w);
    if (std::fread(px.data(), 1, px.size(), fp) != px.size()) return 2;
    if (!check(px, w, w)) {
      std::fprintf(stderr, "tile %u of the file (w = %u) failed\n", t, w);
      return 3;
    }
  }
  std::fclose(fp);
  for (int m = 0; m < 1000; ++m) {
    const uint32_t w = 1 + rnd() % 40, h = m % 3 ? w : 1 + rnd() % 40;
    const uint32_t bg = rnd() & 1 ? 0xffffffffu : 0u, kind = rnd() % 4;
    std::vector<uint8_t> px(4ull * w * h);
    for (uint32_t i = 0; i < w * h; ++i) {
      uint32_t v = bg;
      if (kind == 0 && rnd() % 50 == 0) v = rnd();               // sparse points
      if (kind == 1) v = (i / w / 3) * 0x01010101u;              // bands of equal rows
      if (kind == 2) v = rnd();                                  // noise
      if (kind == 3 && rnd() % 4 == 0) v = (rnd() % 3) * 0x90u;  // few values around the 8 / 9 bit literal border
      std::memcpy(&px[4ull * i], &v, 4);
    }
    if (!check(px, w, h)) {
      std::fprintf(stderr, "seeded tile %d (%u x %u, kind %u) failed\n", m, w, h, kind);
      return 4;
    }
  }
  if (pcv_xray_png_encode_ex(nullptr, 0, 4, PCV_XRAY_PNG_DEFLATE, nullptr, 0, nullptr) != PCV_E_INVALID) return 5;
  if (pcv_xray_png_encode_ex(nullptr, 4, 4, 7, nullptr, 0, nullptr) != PCV_E_INVALID) return 5;
  std::printf("%d encodes, %llu scanline bytes as %llu bytes of deflate files\n", runs, (unsigned long long)raw_bytes,
              (unsigned long long)deflate_bytes);
  return 0;
}
