// pcv_s2_dev.h — the per-point chain of S2Splitter::write (reference src/read_write/s2.rs:60-79): the validity test of an
// ECEF point and `CellID::from_point(p).parent(level)` of the s2 crate, restated from the public S2 definition,
// shared by the host twins and the kernels of pcv_s2.hip.
//
// Every step is a single correctly rounded f64 operation: * + / sqrt and comparisons, no libm, no contraction
// (-ffp-contract=off) — the device's cell id IS pcv_s2_cell_ids_host's, bit for bit. A NaN never decides anything by its
// payload: every comparison with one is false on both sides, and st_to_ij maps it to 0.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace s2 {

constexpr int kMaxLevel = 30;
constexpr double kMaxSize = 1073741824.0;      // 2^30 leaf cells along an edge of a face
constexpr double kRadiusMax = 6384400.0;       // EARTH_RADIUS_MAX_M (src/math/mod.rs)
constexpr double kRadiusMin = 6352800.0;       // EARTH_RADIUS_MIN_M

// The Hilbert curve of the S2 definition: posToIJ[orientation][pos] = (i << 1 | j) of the pos-th subcell,
// posToOrientation[pos] = what the subcell xors into the orientation. The chain needs the inverse of the first (ij -> pos),
// 16 entries of 2 bits packed into one word, and the second packed into a byte — registers, not a table in memory.
constexpr uint32_t kPosToIJ[4][4] = {{0, 1, 3, 2}, {0, 2, 3, 1}, {3, 2, 0, 1}, {3, 1, 0, 2}};
constexpr uint32_t kPosToOrientation[4] = {1, 0, 0, 3};
constexpr uint32_t pack_ij_to_pos() {
  uint32_t w = 0;
  for (uint32_t o = 0; o < 4; ++o)
    for (uint32_t pos = 0; pos < 4; ++pos) w |= pos << (2 * (o * 4 + kPosToIJ[o][pos]));
  return w;
}
constexpr uint32_t pack_pos_to_orientation() {
  uint32_t w = 0;
  for (uint32_t pos = 0; pos < 4; ++pos) w |= kPosToOrientation[pos] << (2 * pos);
  return w;
}
constexpr uint32_t kIjToPos = pack_ij_to_pos();
constexpr uint32_t kOrientationOfPos = pack_pos_to_orientation();

// S2Splitter::write's radius test plus the stated departure: a NaN coordinate is invalid too
__host__ __device__ inline bool valid_ecef(double x, double y, double z) {
  if (x != x || y != y || z != z) return false;
  const double radius = sqrt(x * x + y * y + z * z);
  return !(radius > kRadiusMax || radius < kRadiusMin);
}

// uv -> st, the quadratic projection
__host__ __device__ inline double uv_to_st(double u) {
  return u >= 0.0 ? 0.5 * sqrt(1.0 + 3.0 * u) : 1.0 - 0.5 * sqrt(1.0 - 3.0 * u);
}

// clamp((int)floor(2^30 s), 0, 2^30 - 1); zero, negatives and NaN give 0 (truncation is floor from there on)
__host__ __device__ inline uint32_t st_to_ij(double s) {
  const double f = kMaxSize * s;
  if (!(f > 0.0)) return 0u;
  if (f >= kMaxSize) return (1u << kMaxLevel) - 1u;
  return (uint32_t)f;
}

// face, i, j -> leaf id: thirty 2-bit steps from the most significant bit down. (The definition's 1 024-entry table takes eight
// 4-bit steps over 32 bits of i and j; the two leading zero bits give pos 0 twice and hand the orientation back unchanged.)
__host__ __device__ inline uint64_t leaf_from_face_ij(uint32_t face, uint32_t i, uint32_t j) {
  uint32_t o = face & 1u;
  uint32_t hi = 0, lo = 0;  // 60 bits of position: the upper 15 levels, the lower 15 levels
#pragma unroll
  for (int k = 29; k >= 15; --k) {
    const uint32_t ij = (((i >> k) & 1u) << 1) | ((j >> k) & 1u);
    const uint32_t pos = (kIjToPos >> (2u * (o * 4u + ij))) & 3u;
    hi = (hi << 2) | pos;
    o ^= (kOrientationOfPos >> (2u * pos)) & 3u;
  }
#pragma unroll
  for (int k = 14; k >= 0; --k) {
    const uint32_t ij = (((i >> k) & 1u) << 1) | ((j >> k) & 1u);
    const uint32_t pos = (kIjToPos >> (2u * (o * 4u + ij))) & 3u;
    lo = (lo << 2) | pos;
    o ^= (kOrientationOfPos >> (2u * pos)) & 3u;
  }
  const uint64_t position = ((uint64_t)hi << 30) | (uint64_t)lo;
  return ((((uint64_t)face << 60) | position) << 1) | 1ull;
}

// CellID::from_point: normalise (Point::from_coords), face with ties to the later axis, (u, v) of the face, st, ij, the curve
__host__ __device__ inline uint64_t leaf_from_point(double x, double y, double z) {
  const double n2 = x * x + y * y + z * z;
  const double r = 1.0 / sqrt(n2);
  x = x * r;
  y = y * r;
  z = z * r;
  const double ax = fabs(x), ay = fabs(y), az = fabs(z);
  const uint32_t axis = ax > ay ? (ax > az ? 0u : 2u) : (ay > az ? 1u : 2u);
  const double major = axis == 0u ? x : (axis == 1u ? y : z);
  const uint32_t face = axis + (major < 0.0 ? 3u : 0u);
  double nu, nv;  // numerators of u and v; both are divided by the major component
  switch (face) {
    case 0: nu = y, nv = z; break;
    case 1: nu = -x, nv = z; break;
    case 2: nu = -x, nv = -y; break;
    case 3: nu = z, nv = y; break;
    case 4: nu = z, nv = -x; break;
    default: nu = -y, nv = -x; break;
  }
  const double u = nu / major, v = nv / major;
  return leaf_from_face_ij(face, st_to_ij(uv_to_st(u)), st_to_ij(uv_to_st(v)));
}

__host__ __device__ inline uint64_t lsb_for_level(uint32_t level) { return 1ull << (2u * ((uint32_t)kMaxLevel - level)); }
// CellID::parent(level)
__host__ __device__ inline uint64_t parent(uint64_t id, uint32_t level) {
  const uint64_t lsb = lsb_for_level(level);
  return (id & (0ull - lsb)) | lsb;
}
__host__ __device__ inline uint64_t range_min(uint64_t id) { return id - ((id & (0ull - id)) - 1ull); }
__host__ __device__ inline uint64_t range_max(uint64_t id) { return id + ((id & (0ull - id)) - 1ull); }

// index of the first entry >= key in an ascending list
__host__ __device__ inline uint32_t lower_bound(const uint64_t* list, uint32_t count, uint64_t key) {
  uint32_t lo = 0, hi = count;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (list[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// CellUnion::contains_cellid(leaf) over ascending cell ids
__host__ __device__ inline bool union_contains(const uint64_t* cells, uint32_t count, uint64_t leaf) {
  const uint32_t at = lower_bound(cells, count, leaf);
  if (at < count && range_min(cells[at]) <= leaf) return true;
  return at > 0 && range_max(cells[at - 1]) >= leaf;
}

}  // namespace s2
