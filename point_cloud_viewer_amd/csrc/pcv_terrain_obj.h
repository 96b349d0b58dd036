// pcv_terrain_obj.h — what the renderer reads of a finished terrain (pcv_terrain.hip owns the object; pcv_render.hip draws it).
#pragma once
#include <stdint.h>

#include "pcv_internal.h"
#include "pcv_terrain_dev.h"

// Tiles are kept ascending by (x, y); this key ascends the same way as a signed 64-bit integer, so the tile of a vertex is
// found by a binary search.
PCV_TERRAIN_HD int64_t pcv_terrain_tile_key(int32_t x, int32_t y) {
  return (int64_t)(((uint64_t)(uint32_t)x << 32) | (uint64_t)((uint32_t)y ^ 0x80000000u));
}

struct PcvTerrainLayerView {
  PcvTerrainGrid grid;
  uint32_t T;
  uint64_t ntiles;
  const int64_t* d_tile_keys;  // ntiles, ascending (null when there is no tile)
  const float* d_heights;      // ntiles x T x T x 2
  const uint8_t* d_colors;     // ntiles x T x T x 4
};

// The device side of a finished terrain of `ctx`; the key table is made on first use and lives as long as the terrain.
// PCV_E_INVALID (with a message) for a terrain that is not finished, failed earlier or belongs to another context.
int pcv_terrain_layer_view(pcv_terrain* t, pcv_ctx* ctx, PcvTerrainLayerView* out);
