// pcv_xray_png.h — the device encoder of compressed xray tiles (pcv_xray_png.hip) as pcv_xray_files.hip drives it.
#pragma once
#include "pcv_internal.h"
#include "pcv_xray_png_dev.h"

// Device scratch of one chunk of at most `tiles` W x W tiles, every size from the capacity bound alone: a slot per
// (tile, band), the band tables, and the compacted streams with their count + 1 offsets.
struct PcvPngWork {
  uint32_t W = 0, rows = 0, bands = 0;  // rows per band, bands per tile
  uint64_t tiles = 0;
  uint64_t slot_bytes = 0;   // pcv_png_band_bound of a full band, rounded up to 4
  uint64_t tile_bound = 0;   // pcv_png_stream_bound(W, W)
  uint8_t* slots = nullptr;
  uint32_t* band_bytes = nullptr;  // per (tile, band): bytes of the band with its stored block
  uint32_t* band_off = nullptr;    // per (tile, band): where the band starts inside its tile's stream, after the 78 01
  uint32_t* band_adler = nullptr;  // per (tile, band): sum of the bytes, sum of (n - j) * byte j, both mod 65521
  uint32_t* tile_adler = nullptr;
  uint64_t* offsets = nullptr;     // tiles + 1
  uint8_t* out = nullptr;          // tiles * tile_bound
};
int pcv_xray_png_work_alloc(pcv_ctx* ctx, uint32_t W, uint64_t tiles, PcvPngWork* wk);
void pcv_xray_png_work_free(pcv_ctx* ctx, PcvPngWork* wk);
// `count` (<= wk.tiles) tiles: tile i is a + i * 4 W W for i < na, b + (i - na) * 4 W W after that. Three launches on the
// context's stream (bands, layout, gather); afterwards wk.offsets[0 .. count] and wk.out[0, offsets[count]) are the zlib
// streams of the tiles, back to back.
int pcv_xray_png_launch(pcv_ctx* ctx, const PcvPngWork& wk, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t count);
