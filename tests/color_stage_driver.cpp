// Stand-alone driver of csrc/pcv_color_stage.h for tests/test_color_stage_cpu.py (built with ASan + UBSan, no HIP, no library):
// plays the record sort's cooperative colour load on the CPU, exactly as the kernel uses the plan — every piece of a tile fetched
// with one aligned 16-byte copy or, where the plan says so, byte by byte; every record's colour then read back out of the staged
// buffer as the two aligned words around it — over an array that is allocated with NOTHING behind its last byte, at every
// pointer offset 0..15. Prints one JSON line per (stride, offset, n): tiles, pieces by kind, records checked, and the first
// violation if there is one (a byte outside the array, a misaligned or oversized piece, a colour that came back wrong).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../point_cloud_viewer_amd/csrc/pcv_color_stage.h"

constexpr uint32_t kTile = 8192;

struct Tally {
  long tiles = 0, full = 0, partial = 0, partial_bytes = 0, records = 0, max_pieces = 0;
  std::string bad;
};

static uint8_t colour_byte(uint64_t i) { return (uint8_t)((i * 131u + (i >> 7) * 17u + 5u) & 0xffu); }

// one tile [base, base + tile_n) of an array of n records at `color` (exactly n * stride bytes are readable there)
static void play_tile(const uint8_t* color, uint32_t stride, uint64_t n, uint64_t base, uint32_t tile_n, Tally& t) {
  const PcvColorTile ct = pcv_color_tile((uint32_t)((uintptr_t)color & 15u), stride, base, tile_n);
  const uint32_t buffer_bytes = pcv_color_stage_bytes(kTile, stride);
  std::vector<uint8_t> buf(buffer_bytes, 0xEE);
  std::vector<uint8_t> written(buffer_bytes, 0);
  auto fail = [&](const char* what) {
    if (t.bad.empty()) t.bad = std::string(what) + " (base " + std::to_string(base) + ", tile_n " + std::to_string(tile_n) + ")";
  };
  ++t.tiles;
  if (ct.npieces > pcv_color_stage_pieces(kTile, stride)) return fail("more pieces than the buffer holds");
  if ((long)ct.npieces > t.max_pieces) t.max_pieces = ct.npieces;
  if (ct.skew > 15u || ct.first + (int64_t)ct.skew != (int64_t)(base * stride)) return fail("skew");
  const int64_t bytes = (int64_t)(n * stride);
  for (uint32_t k = 0; k < ct.npieces; ++k) {
    const PcvColorSpan sp = pcv_color_piece(ct, k, n, stride);
    if (sp.at != ct.first + 16 * (int64_t)k) return fail("piece offset");
    if (sp.lo > sp.hi || sp.hi > 16u) return fail("span");
    if (sp.lo < sp.hi && (sp.at + (int64_t)sp.lo < 0 || sp.at + (int64_t)sp.hi > bytes)) return fail("a byte outside the array");
    uint8_t piece[16] = {0};
    if (sp.lo == 0u && sp.hi == 16u) {
      if (((uintptr_t)(color + sp.at) & 15u) != 0u) return fail("a 16-byte load that is not aligned");
      std::memcpy(piece, color + sp.at, 16);  // (ASan: nothing is readable behind the array's last byte)
      ++t.full;
    } else {
      for (uint32_t b = sp.lo; b < sp.hi; ++b) piece[b] = color[sp.at + (int64_t)b];
      ++t.partial;
      t.partial_bytes += sp.hi - sp.lo;
      // a partial piece exists only at the array's two ends
      if (!(sp.at < 0 || sp.at + 16 > bytes)) return fail("a piece inside the array fetched byte by byte");
    }
    std::memcpy(&buf[16 * (size_t)k], piece, 16);
    for (uint32_t b = sp.lo; b < sp.hi; ++b) written[16 * (size_t)k + b] = 1;
  }
  for (uint32_t r = 0; r < tile_n; ++r) {
    const uint32_t at = pcv_color_record_at(ct, r, stride);
    if ((size_t)(at >> 2) * 4 + 8 > buffer_bytes) return fail("a record's words lie outside the buffer");
    if (!(written[at] && written[at + 1] && written[at + 2])) return fail("a record's bytes were not staged");
    uint32_t w0, w1;
    std::memcpy(&w0, &buf[(size_t)(at >> 2) * 4], 4);
    std::memcpy(&w1, &buf[(size_t)(at >> 2) * 4 + 4], 4);
    const uint32_t rgb = (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8u * (at & 3u))) & 0xffffffu;  // v_alignbyte_b32
    const uint64_t i = (base + r) * stride;
    const uint32_t want = (uint32_t)colour_byte(i) | ((uint32_t)colour_byte(i + 1) << 8) | ((uint32_t)colour_byte(i + 2) << 16);
    if (rgb != want) return fail("a record's colour came back wrong");
    ++t.records;
  }
}

int main() {
  const uint64_t ns[] = {1, 2, 5, 6, 8191, 8192, 8193, 16385};
  for (uint32_t stride : {3u, 4u})
    for (uint32_t off = 0; off < 16; ++off)
      for (uint64_t n : ns) {
        const size_t bytes = (size_t)(n * stride);
        // the array ends where its allocation ends; `off` bytes in front of it belong to the allocation but not to the array
        void* mem = nullptr;  // (16-byte aligned; the sanitizer's red zone starts right behind the last byte)
        if (posix_memalign(&mem, 16, off + bytes) != 0 || ((uintptr_t)mem & 15u)) return 3;
        uint8_t* exact = (uint8_t*)mem;
        std::memset(exact, 0x77, off);
        uint8_t* color = exact + off;
        for (size_t i = 0; i < bytes; ++i) color[i] = colour_byte(i);
        Tally t;
        unsigned residues = 0;
        auto tile = [&](uint64_t base) {
          if (base >= n) return;
          residues |= 1u << ((base * stride) & 15u);
          play_tile(color, stride, n, base, (uint32_t)(n - base < kTile ? n - base : kTile), t);
        };
        for (uint64_t base = 0; base < n; base += kTile) tile(base);             // the tiles of chunks that start at tile multiples
        for (uint64_t start : {4ull, 8ull, 12ull, 8196ull, 8200ull, 8204ull}) {  // chunk starts that are only 4-record-aligned
          tile(start);
          tile(start + kTile);
        }
        printf("{\"stride\":%u,\"offset\":%u,\"n\":%llu,\"tiles\":%ld,\"full\":%ld,\"partial\":%ld,\"partial_bytes\":%ld,\"records\":%ld,"
               "\"max_pieces\":%ld,\"residues\":%u,\"bad\":\"%s\"}\n",
               stride, off, (unsigned long long)n, t.tiles, t.full, t.partial, t.partial_bytes, t.records, t.max_pieces, residues, t.bad.c_str());
        std::free(exact);
      }
  return 0;
}
