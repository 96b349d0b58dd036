// pcv_polygon_dev.h — the two rules of a polygon location (PCV_SHAPE_POLYGON), shared by the host twins, the walk
// (pcv_polygon.hip) and the point kernels (pcv_query.hip, pcv_s2_points.hip).
//
// Plain f64 arithmetic, every operation rounded on its own (-ffp-contract=off on both sides), comparisons otherwise: the
// device's verdict IS the host twin's, bit for bit.
//
//   point rule   the polygon's edge table holds every non-horizontal edge from its LOWER endpoint (lx, ly) to its upper one
//                (ux, uy), ly < uy, with slope = (ux - lx) / (uy - ly): {lx, ly, uy, slope}. inside(px, py) is the parity of
//                the edges with ly <= py && py < uy && px < lx + (py - ly) * slope. An edge shared by two polygons is the same
//                table entry in both, whatever their orientation, so polygons that tile a region keep every point in exactly
//                one of them.
//   node rule    a square [x0, x1] x [y0, y1] is hit by an edge a -> b (horizontal ones included) iff their bounding intervals
//                overlap in x and in y and the four corners' side = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) are neither
//                all > 0 nor all < 0.
#pragma once
#include <cstdint>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace poly {

constexpr uint32_t kMaxVertices = 65535;  // per polygon, all rings together

// one edge of the point rule's table: 4 doubles {lx, ly, uy, slope}
__host__ __device__ inline bool crosses(double lx, double ly, double uy, double slope, double px, double py) {
  return ly <= py && py < uy && px < lx + (py - ly) * slope;
}

// On the device a pointer read out of a shape is a generic one, which the compiler loads through the vector path even where the
// address is wave-uniform. The tables live in global memory and are never written by a kernel: as constant-address-space
// pointers, uniform addresses become scalar (scalar-cached) loads.
#if defined(__HIP_DEVICE_COMPILE__)
#define PCV_POLY_TABLE __attribute__((address_space(4)))
#else
#define PCV_POLY_TABLE
#endif

// the point rule: `edges` holds n entries of 4 doubles
__host__ __device__ inline bool inside(const double* __restrict__ table, uint32_t n, double px, double py) {
  const PCV_POLY_TABLE double* edges = (const PCV_POLY_TABLE double*)table;
  uint32_t parity = 0;
#pragma unroll 4  // (four edges' loads in flight; the arithmetic and its order are the same)
  for (uint32_t e = 0; e < n; ++e) parity ^= crosses(edges[4 * e], edges[4 * e + 1], edges[4 * e + 2], edges[4 * e + 3], px, py) ? 1u : 0u;
  return parity != 0;
}

__host__ __device__ inline double side(double ax, double ay, double bx, double by, double cx, double cy) {
  return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// the node rule's edge test: a -> b against the square [x0, x1] x [y0, y1]
__host__ __device__ inline bool edge_hits_square(double ax, double ay, double bx, double by, double x0, double y0, double x1, double y1) {
  const double exl = ax < bx ? ax : bx, exh = ax < bx ? bx : ax;
  const double eyl = ay < by ? ay : by, eyh = ay < by ? by : ay;
  if (!(exl <= x1 && exh >= x0 && eyl <= y1 && eyh >= y0)) return false;
  const double s0 = side(ax, ay, bx, by, x0, y0), s1 = side(ax, ay, bx, by, x1, y0);
  const double s2 = side(ax, ay, bx, by, x0, y1), s3 = side(ax, ay, bx, by, x1, y1);
  const bool all_pos = s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s3 > 0.0;
  const bool all_neg = s0 < 0.0 && s1 < 0.0 && s2 < 0.0 && s3 < 0.0;
  return !(all_pos || all_neg);
}

// the node rule of the xy frame for the cube (min, edge): hi = min + edge per axis. `segs`: every edge a -> b as given, 4 doubles
// {ax, ay, bx, by}; `edges`: the point rule's table.
__host__ __device__ inline bool cube_hits(const double* __restrict__ edges, uint32_t nedges, const double* __restrict__ segs, uint32_t nsegs,
                                          double z_min, double z_max, double mnx, double mny, double mnz, double edge) {
  const double hx = mnx + edge, hy = mny + edge, hz = mnz + edge;
  if (!(z_min <= hz && z_max >= mnz)) return false;
  if (inside(edges, nedges, mnx, mny)) return true;
  for (uint32_t k = 0; k < nsegs; ++k)
    if (edge_hits_square(segs[4 * k], segs[4 * k + 1], segs[4 * k + 2], segs[4 * k + 3], mnx, mny, hx, hy)) return true;
  return false;
}

}  // namespace poly
