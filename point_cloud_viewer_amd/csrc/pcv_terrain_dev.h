// pcv_terrain_dev.h — the terrain grid's chain, one text for host and device (include/pcv_hip.h "terrain layers").
// Everything here is f64 (or integer) arithmetic in a fixed order; the build's -ffp-contract=off keeps it unfused, so
// pcv_terrain_vertex_host and the kernels of pcv_terrain.hip agree bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PCV_TERRAIN_HD __host__ __device__ inline
#else
#define PCV_TERRAIN_HD inline
#endif

// terrain_from_world and the grid, as the kernels take it by value
struct PcvTerrainGrid {
  double m[9];  // rotation rows of terrain_from_world
  double t[3];  // translation of world_from_terrain: l = M (p - t)
  double o[3];  // grid origin
  double res;
};

struct PcvTerrainVertex {
  int64_t i, j;
  float h;
  double dz;  // l_z - o_z
};

PCV_TERRAIN_HD uint32_t pcv_terrain_f32_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
// the usual monotone map of f32 bits onto u32: total order, -0 < +0
PCV_TERRAIN_HD uint32_t pcv_terrain_ord(float f) {
  const uint32_t b = pcv_terrain_f32_bits(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
PCV_TERRAIN_HD float pcv_terrain_unord(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
PCV_TERRAIN_HD bool pcv_terrain_finite(double a) { return fabs(a) <= 1.7976931348623157e308; }  // false for NaN

// The chain of one point. false: u, v or h is not finite, or an index is beyond +-2^62 (no vertex; `out` is zeroed).
PCV_TERRAIN_HD bool pcv_terrain_vertex(const PcvTerrainGrid& g, double px, double py, double pz, PcvTerrainVertex* out) {
  const double dx = px - g.t[0], dy = py - g.t[1], dz = pz - g.t[2];
  const double lx = (g.m[0] * dx + g.m[1] * dy) + g.m[2] * dz;
  const double ly = (g.m[3] * dx + g.m[4] * dy) + g.m[5] * dz;
  const double lz = (g.m[6] * dx + g.m[7] * dy) + g.m[8] * dz;
  const double u = (lx - g.o[0]) / g.res;
  const double v = (ly - g.o[1]) / g.res;
  const double fi = floor(u + 0.5);
  const double fj = floor(v + 0.5);
  const double hz = lz - g.o[2];
  // round to nearest even, with the cast kept inside f32's range: up to the midpoint above FLT_MAX the nearest f32 is FLT_MAX,
  // from there on (and for NaN) the height has no finite f32 and the point is dropped
  const double f32_max = 3.4028234663852886e38, f32_over = 3.4028235677973366e38;  // 2^128 - 2^104, 2^128 - 2^103
  const double ahz = fabs(hz);
  const bool h_ok = ahz < f32_over;
  const float h = !h_ok ? 0.0f : ahz <= f32_max ? (float)hz : (hz < 0.0 ? -3.4028234663852886e38f : 3.4028234663852886e38f);
  const double lim = 4611686018427387904.0;  // 2^62
  out->i = 0, out->j = 0, out->h = 0.0f, out->dz = 0.0;
  if (!pcv_terrain_finite(u) || !pcv_terrain_finite(v) || !h_ok) return false;
  if (!(fabs(fi) < lim) || !(fabs(fj) < lim)) return false;
  out->i = (int64_t)fi, out->j = (int64_t)fj, out->h = h, out->dz = hz;
  return true;
}

PCV_TERRAIN_HD int64_t pcv_terrain_floor_div(int64_t a, int64_t b) {  // b > 0
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
PCV_TERRAIN_HD int64_t pcv_terrain_floor_mod(int64_t a, int64_t b) {  // b > 0
  const int64_t r = a % b;
  return r < 0 ? r + b : r;
}
// the id bit of quad (qx, qy): three residues per axis, so that no unrendered quad has three corners sharing an id
PCV_TERRAIN_HD uint32_t pcv_terrain_quad_bit(int64_t qx, int64_t qy) {
  return 1u << (uint32_t)(pcv_terrain_floor_mod(qx, 3) + 3 * pcv_terrain_floor_mod(qy, 3));
}

// MAX / MIN: one u64 per vertex, larger wins; 0 is "no point" (the count says so too)
PCV_TERRAIN_HD uint64_t pcv_terrain_key(float h, uint32_t r, uint32_t g, uint32_t b, bool is_min) {
  const uint32_t o = is_min ? ~pcv_terrain_ord(h) : pcv_terrain_ord(h);
  return ((uint64_t)o << 32) | (r << 16) | (g << 8) | b;
}
PCV_TERRAIN_HD float pcv_terrain_key_height(uint64_t key, bool is_min) {
  const uint32_t o = (uint32_t)(key >> 32);
  return pcv_terrain_unord(is_min ? ~o : o);
}
// MEAN: |dz| < 2^21, so |hq| <= 2^31 and 2^32 - 1 of them sum inside an i64
PCV_TERRAIN_HD int64_t pcv_terrain_hq(double dz) { return (int64_t)rint(dz * 1024.0); }
PCV_TERRAIN_HD float pcv_terrain_mean_height(int64_t sum, uint32_t count) { return (float)(((double)sum / (double)count) / 1024.0); }
PCV_TERRAIN_HD uint32_t pcv_terrain_mean_channel(uint64_t sum, uint32_t count) { return (uint32_t)((sum + count / 2) / count); }
