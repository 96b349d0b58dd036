// pcv_maptiles_dev.h — the rules of the map-tile product that the host entries and the kernels of
// pcv_maptiles.hip share: the pixel of a point, the value of a pixel, and the slippy <-> xray quadtree index mapping.
//
//   pixel   floor(WebMercatorCoord::to_zoomed_coordinate(z)) of the point's web-mercator coordinate (reference
//           src/math/web_mercator.rs:70-77; TILE_SIZE and MAX_ZOOM :18-23) on top of wmr::project: S = 256 * 2^z is a power
//           of two, so u * S is exact and the floor is the floor of the chain's own u
//   value   xray's `colored` (PointColorColoringStrategy without binning) over exact integer sums, then the background rule
//   index   the xray quadtree puts child 1 top-left, 0 bottom-left, 3 top-right, 2 bottom-right (build_parent): the digit of
//           a slippy tile bit pair is 2 * xbit + (1 - ybit), most significant bit first
#pragma once
#include "pcv_wmr_dev.h"

constexpr uint32_t kMapTilePx = 256;      // TILE_SIZE (web_mercator.rs:18)
constexpr uint32_t kMapTileMaxZoom = 23;  // MAX_ZOOM (web_mercator.rs:23)
constexpr uint64_t kMapTileNoKey = ~0ull; // a dropped point's key
constexpr uint32_t kMapTilePixelLimit = 1u << 24;  // points per pixel: 255 * 2^24 < 2^32, and `colored`'s alpha is 1 up to here

// the global pixel of a point at `zoom`; false: the point is dropped (a coordinate that is not finite, lng = pi, a v that
// rounds outside)
__host__ __device__ inline bool pcv_maptiles_pixel(uint32_t zoom, double x, double y, double z, uint32_t* gx, uint32_t* gy) {
  double u, v;
  wmr::project(x, y, z, &u, &v);
  const double S = (double)((uint64_t)kMapTilePx << zoom);
  const double us = u * S, vs = v * S;
  // the chain's atan2 gives some infinite coordinates a finite (u, v) (atan2(1, inf) = 0): a point with a coordinate that is
  // not finite is dropped whatever the chain makes of it
  const double big = 1.7976931348623157e308;
  const bool finite = wmr::abs_f64(x) <= big && wmr::abs_f64(y) <= big && wmr::abs_f64(z) <= big;
  if (!(finite && us >= 0.0 && us < S && vs >= 0.0 && vs < S)) {  // a NaN or infinite u S or v S fails here
    *gx = *gy = 0;
    return false;
  }
  *gx = (uint32_t)us;  // < 2^31; truncation is the floor of a value >= 0
  *gy = (uint32_t)vs;
  return true;
}
__host__ __device__ inline uint64_t pcv_maptiles_key(uint32_t gx, uint32_t gy) { return (uint64_t)gx | ((uint64_t)gy << 32); }

// Color<f32>::to_u8's `f32 as u8` (src/color.rs:29-36): truncation, saturating
__host__ __device__ inline uint32_t pcv_maptiles_sat_u8(float v) {
  if (!(v > 0.0f)) return 0;
  if (v >= 255.0f) return 255;
  return (uint32_t)v;
}
// packed RGBA8 of a pixel with the exact sums sr, sg, sb over n points, 1 <= n: xray's `colored` (the channel mean rounded
// once to f32; alpha = min(n, 2^24) as f32 / n as f32), then pixels with alpha < 128 take the background. n = 0: background.
__host__ __device__ inline uint32_t pcv_maptiles_rgba(uint64_t sr, uint64_t sg, uint64_t sb, uint64_t n, uint32_t background) {
  if (n == 0) return background;  // TRANSPARENT has alpha 0
  const double dn = 255.0 * (double)n;
  const float asum = (float)(n < (1ull << 24) ? n : (1ull << 24));
  const uint32_t a = pcv_maptiles_sat_u8((asum / (float)n) * 255.0f);
  if (a < 128) return background;
  const uint32_t r = pcv_maptiles_sat_u8((float)((double)sr / dn) * 255.0f), g = pcv_maptiles_sat_u8((float)((double)sg / dn) * 255.0f),
                 b = pcv_maptiles_sat_u8((float)((double)sb / dn) * 255.0f);
  return r | (g << 8) | (b << 16) | (a << 24);
}

// the xray quadtree index of slippy tile (x, y) at `zoom`, and back
__host__ __device__ inline uint64_t pcv_maptiles_quad_index(uint32_t zoom, uint32_t x, uint32_t y) {
  uint64_t index = 0;
  for (int b = (int)zoom - 1; b >= 0; --b) index = (index << 2) | (uint64_t)(2u * ((x >> b) & 1u) + (1u - ((y >> b) & 1u)));
  return index;
}
__host__ __device__ inline void pcv_maptiles_quad_tile(uint32_t zoom, uint64_t index, uint32_t* x, uint32_t* y) {
  uint32_t tx = 0, ty = 0;
  for (int b = (int)zoom - 1; b >= 0; --b) {
    const uint32_t c = (uint32_t)(index >> (2 * b)) & 3u;
    tx = (tx << 1) | (c >> 1);
    ty = (ty << 1) | (1u - (c & 1u));
  }
  *x = tx, *y = ty;
}
