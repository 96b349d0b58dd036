// pcv_color_stage.h — the address plan of the record sort's cooperative colour load (pcv_sort_rec12.hip, first pass). A tile is
// kPcvSortRec12Tile consecutive records in input order, so its colours are tile x stride contiguous bytes of the caller's array:
// the workgroup fetches them as aligned 16-byte pieces into an LDS buffer, and every record picks its three bytes out of that
// buffer. The array is only byte-aligned and belongs to the caller: NO load may touch a byte outside [color, color + n x stride),
// so the pieces that stick out at either end of the array are fetched byte by byte, inside bytes only. Everything the kernel
// needs to know — which pieces a tile loads, which bytes of a piece are inside the array, where a record's bytes lie in the
// buffer — is answered here, in functions the host can call too (tests/color_stage_driver.cpp walks every case on the CPU).
// Standard C++: no HIP header is needed.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCV_COLOR_HD __host__ __device__
#else
#define PCV_COLOR_HD
#endif

constexpr uint32_t kPcvColorPiece = 16;
// pieces a tile can touch at most (the first one may begin up to 15 bytes in front of the tile's first colour), and the bytes of
// the LDS buffer: the pieces + one piece of slack (a record's bytes are read as the two aligned words around them, see below)
constexpr uint32_t pcv_color_stage_pieces(uint32_t tile, uint32_t stride) { return (kPcvColorPiece - 1 + tile * stride + kPcvColorPiece - 1) / kPcvColorPiece; }
constexpr uint32_t pcv_color_stage_bytes(uint32_t tile, uint32_t stride) { return (pcv_color_stage_pieces(tile, stride) + 1) * kPcvColorPiece; }

struct PcvColorTile {
  int64_t first;     // byte offset of piece 0 from the array's first byte (negative: the piece begins in front of the array)
  uint32_t skew;     // the tile's first colour byte lies this far into piece 0 (0..15)
  uint32_t npieces;  // pieces 0 .. npieces - 1 cover the tile's bytes
};
// ptr_low4: the low four bits of the array's address; base: the tile's first record; tile_n: its records (>= 1)
PCV_COLOR_HD inline PcvColorTile pcv_color_tile(uint32_t ptr_low4, uint32_t stride, uint64_t base, uint32_t tile_n) {
  const uint64_t at = base * stride;
  PcvColorTile t;
  t.skew = (uint32_t)((at + (ptr_low4 & 15u)) & 15u);
  t.first = (int64_t)at - (int64_t)t.skew;
  t.npieces = (t.skew + tile_n * stride + kPcvColorPiece - 1) / kPcvColorPiece;
  return t;
}
// piece k of the tile: its byte offset from the array's first byte, and which of its 16 bytes [lo, hi) lie inside the array of n
// records. lo == 0 and hi == 16: one aligned 16-byte load; anything else: bytes lo .. hi - 1 one by one, the others read as zero.
// (The kernel's 1 024 lanes take two pieces each; the one piece more that a full tile of 4-byte colours behind a skewed start
// has — the 2 049th — it fetches as single bytes lo .. hi - 1 as well: narrower than the plan allows, never wider.)
struct PcvColorSpan {
  int64_t at;
  uint32_t lo, hi;
};
PCV_COLOR_HD inline PcvColorSpan pcv_color_piece(const PcvColorTile& t, uint32_t k, uint64_t n, uint32_t stride) {
  PcvColorSpan s;
  s.at = t.first + (int64_t)k * kPcvColorPiece;
  const int64_t left = (int64_t)(n * stride) - s.at;  // bytes of the array from the piece's first byte on
  s.lo = s.at < 0 ? (uint32_t)(-s.at) : 0u;
  s.hi = left >= (int64_t)kPcvColorPiece ? kPcvColorPiece : left > 0 ? (uint32_t)left : 0u;
  if (s.lo > s.hi) s.lo = s.hi;
  return s;
}
// record r of the tile (0 .. tile_n - 1): its red, green, blue are bytes at, at + 1, at + 2 of the buffer (piece k at 16 k).
// The kernel reads the aligned words at >> 2 and (at >> 2) + 1 and shifts by at & 3: the second word may lie in the slack.
PCV_COLOR_HD inline uint32_t pcv_color_record_at(const PcvColorTile& t, uint32_t r, uint32_t stride) { return t.skew + r * stride; }
