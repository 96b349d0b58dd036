// pcv_s2_region_dev.h — the region side of the s2 crate that S2Cells::nodes_in_location asks for (reference
// src/s2_cells/mod.rs:160-241): a Cell from its id, Cell::rect_bound, CellUnion::normalize / rect_bound / intersects_cellid and
// Rect::intersects_cell, restated from the public S2 definition, shared by the host twins and the kernels of
// pcv_s2_query.hip.
//
// As in pcv_s2_dev.h every step is one correctly rounded f64 operation: + - * / sqrt, comparisons, and the transcendentals of
// pcv_wmr_dev.h (atan2_f64, sincos_f64), which are such chains themselves; no libm, no contraction (-ffp-contract=off). The
// device's decision IS the host twin's, bit for bit.
//
// A rect is four doubles: lat.lo, lat.hi (an R1 interval, empty when lo > hi), lng.lo, lng.hi (an S1 interval: inverted when
// lo > hi, empty = (pi, -pi), full = (-pi, pi)).
#pragma once
#include "pcv_s2_dev.h"
#include "pcv_wmr_dev.h"

namespace s2 {

constexpr double kPi = 3.141592653589793;
constexpr double kPiO2 = 1.5707963267948966;
constexpr double kTwoPi = 6.283185307179586;
constexpr double kDblEpsilon = 2.220446049250313e-16;

constexpr uint32_t pack_pos_to_ij() {
  uint32_t w = 0;
  for (uint32_t o = 0; o < 4; ++o)
    for (uint32_t pos = 0; pos < 4; ++pos) w |= kPosToIJ[o][pos] << (2 * (o * 4 + pos));
  return w;
}
constexpr uint32_t kPosToIjPacked = pack_pos_to_ij();

// ---- cell ids -----------------------------------------------------------------------------------------------------------
// a cell id: face 0..5 in the top three bits, the lowest set bit at an even position 0..60
__host__ __device__ inline bool valid_cell(uint64_t id) {
  if (id == 0 || (id >> 61) > 5u) return false;
  return (id & (0ull - id) & 0x1555555555555555ull) != 0;
}
__host__ __device__ inline uint32_t level_of(uint64_t id) { return (uint32_t)kMaxLevel - ((uint32_t)__builtin_ctzll(id) >> 1); }
__host__ __device__ inline bool cell_contains(uint64_t a, uint64_t b) { return range_min(a) <= b && b <= range_max(a); }
__host__ __device__ inline uint64_t immediate_parent(uint64_t id) {
  const uint64_t nlsb = (id & (0ull - id)) << 2;
  return (id & (0ull - nlsb)) | nlsb;
}
__host__ __device__ inline bool are_siblings(uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
  if ((a ^ b ^ c) != d) return false;
  uint64_t mask = (d & (0ull - d)) << 1;
  mask = ~(mask + (mask << 1));
  const uint64_t m = d & mask;
  return (a & mask) == m && (b & mask) == m && (c & mask) == m && level_of(d) != 0u;
}

// CellUnion::normalize on an ASCENDING list, in place: cells contained in another are dropped, four siblings become their
// parent (again and again). Returns the new length.
__host__ __device__ inline uint32_t normalize_sorted(uint64_t* ids, uint32_t n) {
  uint32_t out = 0;
  for (uint32_t k = 0; k < n; ++k) {
    uint64_t ci = ids[k];
    if (out > 0 && cell_contains(ids[out - 1], ci)) continue;
    while (out > 0 && cell_contains(ci, ids[out - 1])) --out;
    while (out >= 3 && are_siblings(ids[out - 3], ids[out - 2], ids[out - 1], ci)) {
      out -= 3;
      ci = immediate_parent(ci);
    }
    ids[out++] = ci;
  }
  return out;
}

// CellUnion::intersects_cellid over an ascending list
__host__ __device__ inline bool union_intersects(const uint64_t* cells, uint32_t count, uint64_t id) {
  const uint32_t at = lower_bound(cells, count, id);
  if (at < count && range_min(cells[at]) <= range_max(id)) return true;
  return at > 0 && range_max(cells[at - 1]) >= range_min(id);
}

// face and the (i, j) of the cell's lowest corner in leaf units: `level` steps of the curve, inverted
__host__ __device__ inline void face_ij_lo(uint64_t id, uint32_t level, uint32_t* face, uint32_t* i_lo, uint32_t* j_lo) {
  const uint32_t f = (uint32_t)(id >> 61);
  uint32_t o = f & 1u, i = 0, j = 0;
  for (uint32_t k = 0; k < level; ++k) {
    const uint32_t pos = (uint32_t)(id >> (59u - 2u * k)) & 3u;
    const uint32_t ij = (kPosToIjPacked >> (2u * (o * 4u + pos))) & 3u;
    i = (i << 1) | (ij >> 1);
    j = (j << 1) | (ij & 1u);
    o ^= (kOrientationOfPos >> (2u * pos)) & 3u;
  }
  *face = f;
  *i_lo = i << ((uint32_t)kMaxLevel - level);
  *j_lo = j << ((uint32_t)kMaxLevel - level);
}

// ---- projections --------------------------------------------------------------------------------------------------------
__host__ __device__ inline double st_to_uv(double s) {
  return s >= 0.5 ? (1.0 / 3.0) * (4.0 * s * s - 1.0) : (1.0 / 3.0) * (1.0 - 4.0 * (1.0 - s) * (1.0 - s));
}
__host__ __device__ inline void face_uv_to_xyz(uint32_t face, double u, double v, double* p) {
  switch (face) {
    case 0: p[0] = 1.0, p[1] = u, p[2] = v; break;
    case 1: p[0] = -u, p[1] = 1.0, p[2] = v; break;
    case 2: p[0] = -u, p[1] = -v, p[2] = 1.0; break;
    case 3: p[0] = -1.0, p[1] = -v, p[2] = -u; break;
    case 4: p[0] = v, p[1] = -1.0, p[2] = -u; break;
    default: p[0] = v, p[1] = u, p[2] = -1.0; break;
  }
}
// (u, v) of a point on a face's plane; false when the point is not on that face's side of the origin
__host__ __device__ inline bool face_xyz_to_uv(uint32_t face, double x, double y, double z, double* u, double* v) {
  switch (face) {
    case 0: if (!(x > 0.0)) return false; *u = y / x, *v = z / x; break;
    case 1: if (!(y > 0.0)) return false; *u = -x / y, *v = z / y; break;
    case 2: if (!(z > 0.0)) return false; *u = -x / z, *v = -y / z; break;
    case 3: if (!(x < 0.0)) return false; *u = z / x, *v = y / x; break;
    case 4: if (!(y < 0.0)) return false; *u = z / y, *v = -x / y; break;
    default: if (!(z < 0.0)) return false; *u = -y / z, *v = -x / z; break;
  }
  return true;
}
__host__ __device__ inline double latitude(const double* p) { return wmr::atan2_f64(p[2], sqrt(p[0] * p[0] + p[1] * p[1])); }
__host__ __device__ inline double longitude(const double* p) { return wmr::atan2_f64(p[1], p[0]); }
// Vector::normalize: the zero vector stays
__host__ __device__ inline void normalize3(double* p) {
  const double n2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
  if (n2 == 0.0) return;
  const double r = 1.0 / sqrt(n2);
  p[0] = p[0] * r, p[1] = p[1] * r, p[2] = p[2] * r;
}
// Point::from(LatLng)
__host__ __device__ inline void point_from_lat_lng(double lat, double lng, double* p) {
  double sphi, cphi, sth, cth;
  wmr::sincos_f64(lat, &sphi, &cphi);
  wmr::sincos_f64(lng, &sth, &cth);
  p[0] = cth * cphi, p[1] = sth * cphi, p[2] = sphi;
}

// ---- S1 intervals -------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool s1_empty(double lo, double hi) { return lo == kPi && hi == -kPi; }
__host__ __device__ inline bool s1_full(double lo, double hi) { return lo == -kPi && hi == kPi; }
__host__ __device__ inline bool s1_fast_contains(double lo, double hi, double p) {
  if (lo > hi) return (p >= lo || p <= hi) && !s1_empty(lo, hi);
  return p >= lo && p <= hi;
}
__host__ __device__ inline bool s1_contains(double lo, double hi, double p) { return s1_fast_contains(lo, hi, p == -kPi ? kPi : p); }
__host__ __device__ inline double positive_distance(double a, double b) {
  const double d = b - a;
  return d >= 0.0 ? d : (b + kPi) - (a - kPi);
}
__host__ __device__ inline void s1_add_point(double* lo, double* hi, double p) {
  if (p == -kPi) p = kPi;
  if (s1_fast_contains(*lo, *hi, p)) return;
  if (s1_empty(*lo, *hi)) {
    *lo = *hi = p;
    return;
  }
  if (positive_distance(p, *lo) < positive_distance(*hi, p)) *lo = p;
  else *hi = p;
}
__host__ __device__ inline void s1_from_point_pair(double p1, double p2, double* lo, double* hi) {
  if (p1 == -kPi) p1 = kPi;
  if (p2 == -kPi) p2 = kPi;
  if (positive_distance(p1, p2) <= kPi) *lo = p1, *hi = p2;
  else *lo = p2, *hi = p1;
}
__host__ __device__ inline bool s1_contains_interval(double lo, double hi, double olo, double ohi) {
  if (lo > hi) {
    if (olo > ohi) return olo >= lo && ohi <= hi;
    return (olo >= lo || ohi <= hi) && !s1_empty(lo, hi);
  }
  if (olo > ohi) return s1_full(lo, hi) || s1_empty(olo, ohi);
  return olo >= lo && ohi <= hi;
}
__host__ __device__ inline bool s1_intersects(double lo, double hi, double olo, double ohi) {
  if (s1_empty(lo, hi) || s1_empty(olo, ohi)) return false;
  if (lo > hi) return olo > ohi || olo <= hi || ohi >= lo;
  if (olo > ohi) return olo <= hi || ohi >= lo;
  return olo <= hi && ohi >= lo;
}
// the union rule of DESIGN §9d
__host__ __device__ inline void s1_union(double* lo, double* hi, double olo, double ohi) {
  if (s1_empty(olo, ohi)) return;
  if (s1_fast_contains(*lo, *hi, olo)) {
    if (s1_fast_contains(*lo, *hi, ohi)) {
      if (s1_contains_interval(*lo, *hi, olo, ohi)) return;
      *lo = -kPi, *hi = kPi;
      return;
    }
    *hi = ohi;
    return;
  }
  if (s1_fast_contains(*lo, *hi, ohi)) {
    *lo = olo;
    return;
  }
  if (s1_empty(*lo, *hi) || s1_fast_contains(olo, ohi, *lo)) {
    *lo = olo, *hi = ohi;
    return;
  }
  if (positive_distance(ohi, *lo) < positive_distance(*hi, olo)) *lo = olo;
  else *hi = ohi;
}
__host__ __device__ inline double s1_length(double lo, double hi) {
  double l = hi - lo;
  if (l >= 0.0) return l;
  l = l + kTwoPi;
  return l > 0.0 ? l : -1.0;
}
__host__ __device__ inline double s1_center(double lo, double hi) {
  const double c = 0.5 * (lo + hi);
  if (!(lo > hi)) return c;
  return c <= 0.0 ? c + kPi : c - kPi;
}
// IEEE remainder(x, 2 pi) for |x| < 3 pi
__host__ __device__ inline double wrap_two_pi(double x) { return x > kPi ? x - kTwoPi : (x < -kPi ? x + kTwoPi : x); }
__host__ __device__ inline void s1_expand(double* lo, double* hi, double margin) {
  if (s1_empty(*lo, *hi)) return;
  if (s1_length(*lo, *hi) + 2.0 * margin + 2.0 * kDblEpsilon >= kTwoPi) {
    *lo = -kPi, *hi = kPi;
    return;
  }
  double l = wrap_two_pi(*lo - margin), h = wrap_two_pi(*hi + margin);
  if (l == -kPi && h != kPi) l = kPi;  // Interval::from_endpoints
  if (h == -kPi && l != kPi) h = kPi;
  if (l <= -kPi) l = kPi;
  *lo = l, *hi = h;
}

// ---- rects --------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void rect_set_empty(double* r) { r[0] = 1.0, r[1] = 0.0, r[2] = kPi, r[3] = -kPi; }
__host__ __device__ inline bool rect_empty(const double* r) { return r[0] > r[1]; }
__host__ __device__ inline bool rect_contains_lat_lng(const double* r, double lat, double lng) {
  return r[0] <= lat && lat <= r[1] && s1_contains(r[2], r[3], lng);
}
__host__ __device__ inline bool r1_intersects(double lo, double hi, double olo, double ohi) {
  if (lo <= olo) return olo <= hi && olo <= ohi;
  return lo <= ohi && lo <= hi;
}
__host__ __device__ inline bool rect_intersects(const double* r, const double* o) {
  return r1_intersects(r[0], r[1], o[0], o[1]) && s1_intersects(r[2], r[3], o[2], o[3]);
}
__host__ __device__ inline void rect_union(double* r, const double* o) {
  if (o[0] <= o[1]) {  // R1 union: an empty side gives the other
    if (r[0] > r[1]) r[0] = o[0], r[1] = o[1];
    else {
      if (o[0] < r[0]) r[0] = o[0];
      if (o[1] > r[1]) r[1] = o[1];
    }
  }
  s1_union(&r[2], &r[3], o[2], o[3]);
}

// ---- a cell -------------------------------------------------------------------------------------------------------------
struct CellGeom {
  uint32_t face;
  double uv[4];    // u.lo u.hi v.lo v.hi
  double rect[4];  // Cell::rect_bound
  double cll[2];   // lat, lng of the centre (CellID::raw_point)
  double vtx[12];  // four unit vertices: (lo, lo) (hi, lo) (hi, hi) (lo, hi)
  double vll[8];   // lat, lng of each
};
constexpr int kCellPlanes = 30;  // the doubles of a CellGeom, as the cell table keeps them (one plane each)

// Cell::rect_bound for level >= 1, from the face and the (u, v) bounds
__host__ __device__ inline void cell_rect_bound(uint32_t face, const double* uv, double* rect) {
  const double u = uv[0] + uv[1], v = uv[2] + uv[3];
  const bool u_has_z = face == 3u || face == 4u, v_has_z = face == 0u || face == 1u;
  const int i = u_has_z ? (u > 0.0) : (u < 0.0), j = v_has_z ? (v > 0.0) : (v < 0.0);
  const double ui = i ? uv[1] : uv[0], uo = i ? uv[0] : uv[1], vj = j ? uv[3] : uv[2], vo = j ? uv[2] : uv[3];
  double p[3];
  face_uv_to_xyz(face, ui, vj, p);
  const double lat_a = latitude(p);
  face_uv_to_xyz(face, uo, vo, p);
  const double lat_b = latitude(p);
  double lat_lo = lat_a < lat_b ? lat_a : lat_b, lat_hi = lat_a < lat_b ? lat_b : lat_a;
  double lng_lo = kPi, lng_hi = -kPi;
  face_uv_to_xyz(face, ui, vo, p);
  s1_add_point(&lng_lo, &lng_hi, longitude(p));
  face_uv_to_xyz(face, uo, vj, p);
  s1_add_point(&lng_lo, &lng_hi, longitude(p));
  // Rect::expanded by 2 eps in both, clamped to the valid latitudes, then the polar closure
  const double margin = 2.0 * kDblEpsilon;
  lat_lo = lat_lo - margin, lat_hi = lat_hi + margin;
  s1_expand(&lng_lo, &lng_hi, margin);
  if (lat_lo < -kPiO2) lat_lo = -kPiO2;
  if (lat_hi > kPiO2) lat_hi = kPiO2;
  if (lat_lo == -kPiO2 || lat_hi == kPiO2) lng_lo = -kPi, lng_hi = kPi;
  rect[0] = lat_lo, rect[1] = lat_hi, rect[2] = lng_lo, rect[3] = lng_hi;
}

__host__ __device__ inline void cell_uv_bounds(uint64_t id, uint32_t* face, double* uv, double* su, double* sv) {
  const uint32_t level = level_of(id);
  uint32_t i, j;
  face_ij_lo(id, level, face, &i, &j);
  const uint32_t size = 1u << ((uint32_t)kMaxLevel - level);
  const double inv = 1.0 / kMaxSize;
  uv[0] = st_to_uv((double)i * inv);
  uv[1] = st_to_uv((double)(i + size) * inv);
  uv[2] = st_to_uv((double)j * inv);
  uv[3] = st_to_uv((double)(j + size) * inv);
  // the centre in (si, ti) units of 2^-31: twice the low corner plus one cell size
  *su = (0.5 * inv) * (double)(2ull * i + size);
  *sv = (0.5 * inv) * (double)(2ull * j + size);
}

// everything Rect::intersects_cell reads of a cell of level >= 1
__host__ __device__ inline void cell_geom(uint64_t id, CellGeom* g) {
  double su, sv, p[3];
  cell_uv_bounds(id, &g->face, g->uv, &su, &sv);
  cell_rect_bound(g->face, g->uv, g->rect);
  face_uv_to_xyz(g->face, st_to_uv(su), st_to_uv(sv), p);
  g->cll[0] = latitude(p), g->cll[1] = longitude(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double* q = g->vtx + 3 * k;
    face_uv_to_xyz(g->face, g->uv[(k == 1 || k == 2) ? 1 : 0], g->uv[2 + (k >= 2 ? 1 : 0)], q);
    normalize3(q);
    g->vll[2 * k] = latitude(q), g->vll[2 * k + 1] = longitude(q);
  }
}

// a CellGeom as kCellPlanes planes of n doubles, cell c at column c (the cell table of a cloud, the cells of a shape table's
// unions, and n = 1: pcv_s2_cell_geometry_host)
__host__ __device__ inline void store_geom(const CellGeom& g, double* table, size_t n, size_t c) {
  double* t = table + c;
#pragma unroll
  for (int k = 0; k < 4; ++k) t[(size_t)k * n] = g.rect[k];
  t[4 * n] = g.cll[0], t[5 * n] = g.cll[1];
#pragma unroll
  for (int k = 0; k < 4; ++k) t[(size_t)(6 + k) * n] = g.uv[k];
#pragma unroll
  for (int k = 0; k < 12; ++k) t[(size_t)(10 + k) * n] = g.vtx[k];
#pragma unroll
  for (int k = 0; k < 8; ++k) t[(size_t)(22 + k) * n] = g.vll[k];
}
static_assert(kCellPlanes == 30, "store_geom / load_geom write and read 30 planes");

__host__ __device__ inline void load_geom(const double* table, size_t n, size_t c, uint64_t id, CellGeom* g) {
  const double* t = table + c;
  g->face = (uint32_t)(id >> 61);
#pragma unroll
  for (int k = 0; k < 4; ++k) g->rect[k] = t[(size_t)k * n];
  g->cll[0] = t[4 * n], g->cll[1] = t[5 * n];
#pragma unroll
  for (int k = 0; k < 4; ++k) g->uv[k] = t[(size_t)(6 + k) * n];
#pragma unroll
  for (int k = 0; k < 12; ++k) g->vtx[k] = t[(size_t)(10 + k) * n];
#pragma unroll
  for (int k = 0; k < 8; ++k) g->vll[k] = t[(size_t)(22 + k) * n];
}

// rect_bound of a union: the union of its cells' rects. False when a cell is of level 0.
__host__ __device__ inline bool union_rect_bound(const uint64_t* ids, uint32_t n, double* rect) {
  rect_set_empty(rect);
  for (uint32_t k = 0; k < n; ++k) {
    if (level_of(ids[k]) == 0u) return false;
    uint32_t face;
    double uv[4], su, sv, r[4];
    cell_uv_bounds(ids[k], &face, uv, &su, &sv);
    cell_rect_bound(face, uv, r);
    rect_union(rect, r);
  }
  return true;
}

// cells_in_convex_polyhedron's region (mod.rs:224-231): the corners' leaf cells, normalized, their rect bound. `ids`: eight
// slots of working memory (a kernel that may not spill hands in LDS: the sort and the normalization index them by variables).
__host__ __device__ inline bool corners_rect_in(const double* corners, uint64_t* ids, double* rect) {
#pragma unroll
  for (int k = 0; k < 8; ++k) ids[k] = leaf_from_point(corners[3 * k], corners[3 * k + 1], corners[3 * k + 2]);
  for (int a = 1; a < 8; ++a) {  // insertion sort
    const uint64_t key = ids[a];
    int b = a - 1;
    while (b >= 0 && ids[b] > key) {
      ids[b + 1] = ids[b];
      --b;
    }
    ids[b + 1] = key;
  }
  return union_rect_bound(ids, normalize_sorted(ids, 8), rect);
}
__host__ __device__ inline bool corners_rect(const double* corners, double* rect) {
  uint64_t ids[8];
  return corners_rect_in(corners, ids, rect);
}

// ---- Rect::intersects_cell ----------------------------------------------------------------------------------------------
__host__ __device__ inline bool cell_contains_point(const CellGeom& g, const double* p) {
  double u, v;
  if (!face_xyz_to_uv(g.face, p[0], p[1], p[2], &u, &v)) return false;
  return u >= g.uv[0] - kDblEpsilon && u <= g.uv[1] + kDblEpsilon && v >= g.uv[2] - kDblEpsilon && v <= g.uv[3] + kDblEpsilon;
}
__host__ __device__ inline void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
// do the interiors of the edges ab and cd cross: plain f64 signs (a stated departure from exact predicates)
__host__ __device__ inline bool simple_crossing(const double* a, const double* b, const double* c, const double* d) {
  double ab[3], cd[3];
  cross3(a, b, ab);
  const double acb = -dot3(ab, c), bda = dot3(ab, d);
  if (!(acb * bda > 0.0)) return false;
  cross3(c, d, cd);
  const double cbd = -dot3(cd, b), dac = dot3(cd, a);
  return acb * cbd > 0.0 && acb * dac > 0.0;
}
__host__ __device__ inline bool intersects_lng_edge(const double* a, const double* b, double lat_lo, double lat_hi, double lng) {
  double c[3], d[3];
  point_from_lat_lng(lat_lo, lng, c);
  point_from_lat_lng(lat_hi, lng, d);
  return simple_crossing(a, b, c, d);
}
__host__ __device__ inline bool intersects_lat_edge(const double* a, const double* b, double lat, double lng_lo, double lng_hi) {
  double s[3] = {a[0] + b[0], a[1] + b[1], a[2] + b[2]}, t[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, z[3];
  cross3(s, t, z);  // the normal of the plane ab, made to point north
  normalize3(z);
  if (z[2] < 0.0) z[0] = -z[0], z[1] = -z[1], z[2] = -z[2];
  double y[3] = {z[1], -z[0], 0.0}, x[3];  // z x (0, 0, 1)
  normalize3(y);
  cross3(y, z, x);  // where the great circle reaches its highest latitude
  double sin_lat, cos_lat;
  wmr::sincos_f64(lat, &sin_lat, &cos_lat);
  if (!(wmr::abs_f64(sin_lat) < x[2])) return false;  // the great circle does not reach the latitude
  const double cos_theta = sin_lat / x[2];
  const double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
  const double theta = wmr::atan2_f64(sin_theta, cos_theta);
  double ab_lo, ab_hi;
  s1_from_point_pair(wmr::atan2_f64(dot3(a, y), dot3(a, x)), wmr::atan2_f64(dot3(b, y), dot3(b, x)), &ab_lo, &ab_hi);
  if (s1_contains(ab_lo, ab_hi, theta)) {
    const double ix = x[0] * cos_theta + y[0] * sin_theta, iy = x[1] * cos_theta + y[1] * sin_theta;
    if (s1_contains(lng_lo, lng_hi, wmr::atan2_f64(iy, ix))) return true;
  }
  if (s1_contains(ab_lo, ab_hi, -theta)) {
    const double ix = x[0] * cos_theta - y[0] * sin_theta, iy = x[1] * cos_theta - y[1] * sin_theta;
    if (s1_contains(lng_lo, lng_hi, wmr::atan2_f64(iy, ix))) return true;
  }
  return false;
}

// The order of DESIGN §9d. (The rejection of step 4 may run first: steps 2 and 3 cannot pass where it rejects, the bound being
// 2 eps wider than the cell; pcv_s2_query.hip's pair kernel does so, and so does the host twin, through the same function.)
__host__ __device__ inline bool rect_intersects_cell_after_bound(const double* r, const CellGeom& g) {
  if (rect_contains_lat_lng(r, g.cll[0], g.cll[1])) return true;
  double c[3];
  point_from_lat_lng(0.5 * (r[0] + r[1]), s1_center(r[2], r[3]), c);
  if (cell_contains_point(g, c)) return true;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (rect_contains_lat_lng(r, g.vll[2 * k], g.vll[2 * k + 1])) return true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = (k + 1) & 3;
    double e_lo, e_hi;
    s1_from_point_pair(g.vll[2 * k + 1], g.vll[2 * n + 1], &e_lo, &e_hi);
    if (!s1_intersects(r[2], r[3], e_lo, e_hi)) continue;
    const double *a = g.vtx + 3 * k, *b = g.vtx + 3 * n;
    if (s1_contains(e_lo, e_hi, r[2]) && intersects_lng_edge(a, b, r[0], r[1], r[2])) return true;
    if (s1_contains(e_lo, e_hi, r[3]) && intersects_lng_edge(a, b, r[0], r[1], r[3])) return true;
    if (intersects_lat_edge(a, b, r[0], r[2], r[3])) return true;
    if (intersects_lat_edge(a, b, r[1], r[2], r[3])) return true;
  }
  return false;
}
__host__ __device__ inline bool rect_intersects_cell(const double* r, const CellGeom& g) {
  if (rect_empty(r) || !rect_intersects(r, g.rect)) return false;
  return rect_intersects_cell_after_bound(r, g);
}

}  // namespace s2
