// pcv_xray_png_dev.h — the run-length deflate stream of compressed xray tiles (PCV_XRAY_PNG_DEFLATE), stated once for
// the host encoder (pcv_png.cpp, plain C++) and the device encoder (pcv_xray_png.hip): the row filters, the tokens of a
// run of equal bytes with their fixed Huffman codes (RFC 1951 3.2.6), their bit counts, and the capacity bound.
//
//   scanlines   row 0: filter byte 1 (Sub, 4 bytes per pixel), every other row: filter byte 2 (Up); 1 + 4 w bytes a row
//   bands       PCV_XRAY_PNG_BAND_ROWS(w) consecutive rows, the last band may be shorter; one band = one fixed-Huffman
//               block (BFINAL 0) followed by an empty stored block (3 header bits, pad, 00 00 FF FF), so every band
//               starts and ends on a byte boundary; the stored block after the last band carries BFINAL 1
//   tokens      per maximal run of L equal bytes inside a band: one literal, then with r = L - 1 matches of
//               min(r, 258) at distance 1 while r >= 3, then r (0, 1 or 2) literals; end-of-block closes the band
//   zlib        78 01, the bands, Adler-32 of the filtered scanlines, big-endian
#pragma once
#include <stdint.h>

#include "../../include/pcv_hip.h"

#if defined(__HIPCC__)
#define PCV_PNG_HD __host__ __device__
#else
#define PCV_PNG_HD
#endif

struct PcvPngToken {
  uint32_t bits;   // as they go into the LSB-first bit stream: the Huffman code reversed, extra bits above it
  uint32_t nbits;
};

PCV_PNG_HD inline uint32_t pcv_png_reverse(uint32_t code, uint32_t n) {  // the low n (<= 9) bits, mirrored
  uint32_t r = 0;
  for (uint32_t k = 0; k < n; ++k) r |= ((code >> k) & 1u) << (n - 1 - k);
  return r;
}

PCV_PNG_HD inline PcvPngToken pcv_png_literal(uint32_t v) {
  return v < 144 ? PcvPngToken{pcv_png_reverse(0x30u + v, 8), 8} : PcvPngToken{pcv_png_reverse(0x190u + (v - 144), 9), 9};
}

// a match of `len` (3 .. 258) bytes at distance 1: length symbol, its extra bits, distance code 0 (5 zero bits)
PCV_PNG_HD inline PcvPngToken pcv_png_match(uint32_t len) {
  uint32_t sym, extra = 0, nextra = 0;
  if (len == 258) {
    sym = 285;
  } else if (len < 11) {
    sym = 257 + (len - 3);
  } else {
    const uint32_t x = len - 3;  // 8 .. 254: groups of four symbols per power of two
    nextra = 1;
    while (x >> (nextra + 3)) ++nextra;
    sym = 261 + 4 * nextra + ((x >> nextra) & 3u);
    extra = x & ((1u << nextra) - 1u);
  }
  const uint32_t nsym = sym < 280 ? 7 : 8;
  const uint32_t code = sym < 280 ? sym - 256 : 0xc0u + (sym - 280);
  return PcvPngToken{pcv_png_reverse(code, nsym) | extra << nsym, nsym + nextra + 5};
}

// bits of the tokens of one run of `len` (>= 1) bytes of value v
PCV_PNG_HD inline uint32_t pcv_png_run_bits(uint32_t len, uint32_t v) {
  const uint32_t lit = v < 144 ? 8 : 9;
  uint32_t r = len - 1;
  if (r < 3) return lit * (1 + r);
  uint32_t bits = lit + 13 * (r / 258);  // symbol 285: 8 + 5 bits
  r %= 258;
  return bits + (r >= 3 ? pcv_png_match(r).nbits : lit * r);
}

// the tokens of that run in stream order, each handed to put(bits, nbits)
template <typename Put>
PCV_PNG_HD inline void pcv_png_run_emit(uint32_t len, uint32_t v, Put&& put) {
  const PcvPngToken lit = pcv_png_literal(v);
  put(lit.bits, lit.nbits);
  uint32_t r = len - 1;
  if (r >= 3) {
    const PcvPngToken full = pcv_png_match(258);
    for (; r >= 258; r -= 258) put(full.bits, full.nbits);
    if (r >= 3) {
      const PcvPngToken m = pcv_png_match(r);
      put(m.bits, m.nbits);
      r = 0;
    }
  }
  for (; r; --r) put(lit.bits, lit.nbits);
}

// byte `col` (0: the filter byte) of filtered scanline `row` of a w pixel wide RGBA8 image
PCV_PNG_HD inline uint32_t pcv_png_filtered(const uint8_t* rgba, uint32_t w, uint32_t row, uint32_t col) {
  if (col == 0) return row == 0 ? 1u : 2u;
  const uint32_t i = col - 1;
  const uint8_t* cur = rgba + (uint64_t)row * 4 * w;
  if (row == 0) return (uint8_t)(cur[i] - (i >= 4 ? cur[i - 4] : 0));
  return (uint8_t)(cur[i] - (cur - 4ull * w)[i]);
}

// capacity of one band of n filtered bytes with its stored block: ceil((3 + 9 n + 7) / 8) + 5
PCV_PNG_HD inline uint64_t pcv_png_band_bound(uint64_t n) { return (3 + 9 * n + 7 + 7) / 8 + 5; }

// capacity of the zlib stream of a w x h image: 2 + its bands + 4
PCV_PNG_HD inline uint64_t pcv_png_stream_bound(uint32_t w, uint32_t h) {
  const uint64_t rows = PCV_XRAY_PNG_BAND_ROWS(w), row = 1 + 4ull * w;
  const uint64_t full = h / rows, rest = h % rows;
  return 2 + full * pcv_png_band_bound(rows * row) + (rest ? pcv_png_band_bound(rest * row) : 0) + 4;
}

constexpr uint64_t kPcvPngWrap = 8 + (12 + 13) + 12 + 12;  // signature, IHDR, the IDAT's and IEND's chunk frames

// host only (pcv_png.cpp)
uint32_t pcv_crc32_update(uint32_t crc, const uint8_t* p, uint64_t n);  // running value: start and finish with ~0
uint64_t pcv_png_stored_size(uint32_t w, uint32_t h);
void pcv_png_stored_encode(const uint8_t* rgba, uint32_t w, uint32_t h, uint8_t* out);  // pcv_png_stored_size bytes
// the whole file around a finished zlib stream of a w x h RGBA8 image: kPcvPngWrap + zlen bytes
void pcv_png_wrap(uint32_t w, uint32_t h, const uint8_t* z, uint64_t zlen, uint8_t* out);
