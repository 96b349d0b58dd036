// pcv_tiles3d_dev.h — the position chain of the 3D Tiles export, one text for host and device (include/pcv_hip.h
// "3D Tiles"). A stored coordinate of a node (a u8 / u16 code, or an f32 / f64 unit value) becomes a u16 of POSITION_QUANTIZED
// or an f32 of POSITION about the tile's RTC_CENTER. Every step is one correctly rounded f64 operation (or an exact integer
// one) in a fixed order, no libm call, and `fma` only where it is written; the build's -ffp-contract=off keeps the rest
// unfused, so pcv_tiles3d_tile_host and tiles3d_pack_kernel agree bit for bit.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/pcv_hip.h"

#if defined(__HIPCC__)
#define PCV_TILES3D_HD __host__ __device__ inline
#else
#define PCV_TILES3D_HD inline
#endif

// rc[a] = (double)(float)(cube_min[a] + cube_edge / 2): a centre that a reader's float32 keeps as it is
PCV_TILES3D_HD double pcv_tiles3d_rtc(double cube_min, double cube_edge) { return (double)(float)(cube_min + cube_edge / 2.0); }

// bytes of one coordinate as the node stores it
PCV_TILES3D_HD uint32_t pcv_tiles3d_src_bytes(uint32_t enc) {
  return enc == PCV_ENC_UINT8 ? 1u : enc == PCV_ENC_UINT16 ? 2u : enc == PCV_ENC_FLOAT32 ? 4u : 8u;
}
// the form AUTO takes for a node: the codes verbatim where there are codes, an f32 about the centre where there are none
PCV_TILES3D_HD uint32_t pcv_tiles3d_mode_of(uint32_t position_mode, uint32_t enc) {
  if (position_mode != PCV_TILES3D_POS_AUTO) return position_mode;
  return enc == PCV_ENC_UINT8 || enc == PCV_ENC_UINT16 ? PCV_TILES3D_POS_QUANTIZED : PCV_TILES3D_POS_FLOAT;
}

// The stored coordinate as the chain takes it: `code` for u8 / u16 nodes, `t` (the unit value, an f32 widened exactly) else.
struct PcvTiles3dCoord {
  uint32_t code;
  double t;
};
PCV_TILES3D_HD PcvTiles3dCoord pcv_tiles3d_load(uint32_t enc, const uint8_t* p) {  // p: the coordinate's bytes, any alignment
  PcvTiles3dCoord c{0u, 0.0};
  if (enc == PCV_ENC_UINT8) {
    c.code = p[0];
  } else if (enc == PCV_ENC_UINT16) {
    c.code = (uint32_t)p[0] | (uint32_t)p[1] << 8;
  } else if (enc == PCV_ENC_FLOAT32) {
    float f;
    memcpy(&f, p, 4);
    c.t = (double)f;
  } else {
    memcpy(&c.t, p, 8);
  }
  return c;
}

// POSITION_QUANTIZED: c * 257 for a u8 code (exact: c / 255 = 257 c / 65535), a u16 code verbatim, trunc(65535 t) else
PCV_TILES3D_HD uint16_t pcv_tiles3d_quantized(uint32_t enc, PcvTiles3dCoord c) {
  if (enc == PCV_ENC_UINT8) return (uint16_t)(c.code * 257u);
  if (enc == PCV_ENC_UINT16) return (uint16_t)c.code;
  return (uint16_t)(uint32_t)(int32_t)(65535.0 * c.t);  // the conversion truncates
}

// POSITION: the node's decode (code / max, or t, times the edge plus the minimum in one fma) minus the centre, as f32
PCV_TILES3D_HD float pcv_tiles3d_float(uint32_t enc, PcvTiles3dCoord c, double cube_min, double cube_edge, double rc) {
  double u;
  if (enc == PCV_ENC_UINT8) u = (double)c.code / 255.0;
  else if (enc == PCV_ENC_UINT16) u = (double)c.code / 65535.0;
  else u = c.t;
  return (float)(__builtin_fma(u, cube_edge, cube_min) - rc);
}
