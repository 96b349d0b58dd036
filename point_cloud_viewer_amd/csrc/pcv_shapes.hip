// pcv_shapes.hip — prepared query shapes for gfx950: pcv_shapes_create / _create_ex / _free / _count / _get /
// _get_ex / _union / _create_ex2 / _polygon.
//
//   K7a shape_setup      Frustum::from_matrix4 / intersector / cache_separating_axes_for_aabb
//                        (reference src/geometry/frustum.rs:111-166, src/math/sat.rs:111-143), Obb (obb.rs:48-80),
//                        WebMercatorRect::intersector (web_mercator_rect.rs:85-116)
//
// Arithmetic follows the nalgebra 0.22 formulas restated in DESIGN.md ("query arithmetic"): left-to-right dot
// products, gemv column accumulation, division by the norm, no fused multiply-add (-ffp-contract=off).
// The node kernels that read the prepared shapes are in pcv_cull.hip, the point kernels in pcv_query.hip.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "pcv_query_dev.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_region_dev.h"

// ---------------------------------------------------------------------------------------------
// device math
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ V3d v_normalize(V3d v) {
  double n = sqrt(v_dot(v, v));
  return {v.x / n, v.y / n, v.z / n};
}

__device__ bool m4_try_inverse(const double* m, double* out) {
  double inv[16];
  inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
  if (det == 0.0) return false;
  double inv_det = 1.0 / det;
  for (int i = 0; i < 16; ++i) out[i] = inv[i] * inv_det;
  return true;
}

// ---------------------------------------------------------------------------------------------
// prepared shapes
// ---------------------------------------------------------------------------------------------
// PcvShapeDev, PcvShapeWide and pcv_shapes: pcv_query_dev.h (the frame renderer reads the frusta's clip matrices)

namespace {

__device__ void project8(const double* corners, V3d axis, double* mn, double* mx) {  // sat.rs:196-205
  double lo = 1.7976931348623157e308, hi = -1.7976931348623157e308;
  for (int i = 0; i < 8; ++i) {
    double p = v_dot(V3d{corners[3 * i], corners[3 * i + 1], corners[3 * i + 2]}, axis);
    lo = fmin(lo, p);
    hi = fmax(hi, p);
  }
  *mn = lo;
  *mx = hi;
}

// cache_separating_axes against the unit edges / normals of an AABB (sat.rs:111-143)
__device__ int cache_axes_for_aabb(double* axes, int cap, const V3d* edges, int ne, const V3d* normals, int nn) {
  const V3d unit[3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  V3d all[6 + 3 + 36];
  int na = 0;
  for (int i = 0; i < nn; ++i) all[na++] = normals[i];
  for (int i = 0; i < 3; ++i) all[na++] = unit[i];
  for (int i = 0; i < ne; ++i)
    for (int j = 0; j < 3; ++j) {
      V3d c = v_normalize(v_cross(edges[i], unit[j]));
      if (isfinite(c.x) && isfinite(c.y) && isfinite(c.z)) all[na++] = c;
    }
  int nd = 0;
  for (int i = 0; i < na; ++i) {
    bool dupe = false;
    for (int j = 0; j < nd; ++j) {
      V3d a2 = {axes[3 * j], axes[3 * j + 1], axes[3 * j + 2]};
      V3d dm = v_sub(all[i], a2), dp = v_add(all[i], a2);
      double d1 = v_dot(dm, dm), d2 = v_dot(dp, dp);
      if (fmin(d1, d2) < 2.220446049250313e-16) {
        dupe = true;
        break;
      }
    }
    if (!dupe && nd < cap) {
      axes[3 * nd] = all[i].x;
      axes[3 * nd + 1] = all[i].y;
      axes[3 * nd + 2] = all[i].z;
      ++nd;
    }
  }
  return nd;
}

__global__ __launch_bounds__(64) void shape_setup_kernel(PcvShapeDev* shapes, uint32_t count) {
  uint32_t f = blockIdx.x * 64 + threadIdx.x;
  if (f >= count) return;
  PcvShapeDev* s = shapes + f;
  s->valid = 1;
  if (s->kind == PCV_SHAPE_FRUSTUM || s->kind == PCV_SHAPE_FRUSTUM_WITH_INVERSE) {
    if (s->kind == PCV_SHAPE_FRUSTUM) {
      double inv[16];
      if (!m4_try_inverse(s->clip_from_query, inv)) {
        s->valid = 0;
        s->naxes = 0;
        return;
      }
      for (int i = 0; i < 16; ++i) s->query_from_clip[i] = inv[i];
    }
    const double sg[2] = {-1.0, 1.0};
    V3d k[8];
    int c = 0;
    for (int ix = 0; ix < 2; ++ix)
      for (int iy = 0; iy < 2; ++iy)
        for (int iz = 0; iz < 2; ++iz) k[c++] = m4_transform_point(s->query_from_clip, V3d{sg[ix], sg[iy], sg[iz]});
    for (int i = 0; i < 8; ++i) {
      s->corners[3 * i] = k[i].x;
      s->corners[3 * i + 1] = k[i].y;
      s->corners[3 * i + 2] = k[i].z;
    }
    V3d e[6], n[5];
    e[0] = v_normalize(v_sub(k[4], k[0]));
    e[1] = v_normalize(v_sub(k[2], k[0]));
    e[2] = v_normalize(v_sub(k[1], k[0]));
    e[3] = v_normalize(v_sub(k[3], k[2]));
    e[4] = v_normalize(v_sub(k[5], k[4]));
    e[5] = v_normalize(v_sub(k[7], k[6]));
    n[0] = v_normalize(v_cross(e[0], e[1]));
    n[1] = v_normalize(v_cross(e[0], e[2]));
    n[2] = v_normalize(v_cross(e[0], e[3]));
    n[3] = v_normalize(v_cross(e[1], e[2]));
    n[4] = v_normalize(v_cross(e[1], e[4]));
    s->naxes = cache_axes_for_aabb(s->axes, PCV_MAX_AXES, e, 6, n, 5);
  } else if (s->kind == PCV_SHAPE_OBB) {
    // s->iso holds query_from_obb on entry; corners/edges use it, contains() needs the inverse (obb.rs:35-41)
    const double* q = s->iso + 3;
    V3d t = {s->iso[0], s->iso[1], s->iso[2]};
    const double sx[8] = {-1, 1, -1, 1, -1, 1, -1, 1}, sy[8] = {-1, -1, 1, 1, -1, -1, 1, 1}, sz[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
    for (int c = 0; c < 8; ++c) {
      V3d p = v_add(quat_rotate(q, V3d{sx[c] * s->half[0], sy[c] * s->half[1], sz[c] * s->half[2]}), t);
      s->corners[3 * c] = p.x;
      s->corners[3 * c + 1] = p.y;
      s->corners[3 * c + 2] = p.z;
    }
    V3d e[3];
    e[0] = v_normalize(quat_rotate(q, V3d{1, 0, 0}));
    e[1] = v_normalize(quat_rotate(q, V3d{0, 1, 0}));
    e[2] = v_normalize(quat_rotate(q, V3d{0, 0, 1}));
    s->naxes = cache_axes_for_aabb(s->axes, PCV_MAX_AXES, e, 3, e, 3);
    double qi[4] = {-q[0], -q[1], -q[2], q[3]};  // Isometry3::inverse
    V3d ti = quat_rotate(qi, V3d{-t.x, -t.y, -t.z});
    s->iso[0] = ti.x;
    s->iso[1] = ti.y;
    s->iso[2] = ti.z;
    s->iso[3] = qi[0];
    s->iso[4] = qi[1];
    s->iso[5] = qi[2];
    s->iso[6] = qi[3];
  } else if (s->kind == PCV_SHAPE_AABB) {  // aabb.rs:98-125
    const double* mn = s->bmin;
    const double* mx = s->bmax;
    const double cs[24] = {mn[0], mn[1], mn[2], mx[0], mn[1], mn[2], mn[0], mx[1], mn[2], mx[0], mx[1], mn[2],
                           mn[0], mn[1], mx[2], mx[0], mn[1], mx[2], mn[0], mx[1], mx[2], mx[0], mx[1], mx[2]};
    for (int i = 0; i < 24; ++i) s->corners[i] = cs[i];
    const double ax[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) s->axes[i] = ax[i];
    s->naxes = 3;
  } else if (s->kind == PCV_SHAPE_WEB_MERCATOR_RECT) {
    // s->corners came up from the host (pcv_wmr_corners); edges and face normals in intersector()'s order
    // (web_mercator_rect.rs:85-116)
    V3d k[8];
    for (int i = 0; i < 8; ++i) k[i] = V3d{s->corners[3 * i], s->corners[3 * i + 1], s->corners[3 * i + 2]};
    V3d e[12], n[6];
    for (int i = 0; i < 4; ++i) {
      e[i] = v_normalize(v_sub(k[(i + 1) & 3], k[i]));              // N E S W edge, down
      e[4 + i] = v_normalize(v_sub(k[4 + ((i + 1) & 3)], k[4 + i]));  // N E S W edge, up
      e[8 + i] = v_normalize(v_sub(k[4 + i], k[i]));                // NW NE SE SW edge
    }
    for (int i = 0; i < 4; ++i) n[i] = v_normalize(v_cross(e[i], e[8 + i]));  // N E S W face
    n[4] = v_normalize(v_cross(e[1], e[0]));                                  // down face
    n[5] = v_normalize(v_cross(e[5], e[4]));                                  // up face
    PcvShapeWide* w = s->wide;
    w->naxes = cache_axes_for_aabb(w->axes, PCV_WIDE_AXES, e, 12, n, 6);
    for (int a = 0; a < w->naxes; ++a)
      project8(s->corners, V3d{w->axes[3 * a], w->axes[3 * a + 1], w->axes[3 * a + 2]}, &w->amin[a], &w->amax[a]);
    s->naxes = 0;
  } else if (s->kind == PCV_SHAPE_S2_CELL_UNION || s->kind == PCV_SHAPE_POLYGON) {
    // no corners, no axes. Not valid to the traversals of the other kinds, which then report nothing for it; its own walk and
    // point instances (pcv_union.hip / pcv_polygon.hip, pcv_query.hip) read s->cell_union / s->polygon and do not look at this
    // flag. (A web-mercator polygon arrives here as the web-mercator rectangle over its vertices.)
    s->valid = 0;
    s->naxes = 0;
  } else {
    s->naxes = 0;  // AllPoints
  }
  for (int a = 0; a < s->naxes; ++a)
    project8(s->corners, V3d{s->axes[3 * a], s->axes[3 * a + 1], s->axes[3 * a + 2]}, &s->amin[a], &s->amax[a]);
}

}  // namespace

static void release_shapes(pcv_shapes* s) {
  if (s->d_union) s->ctx->dev_free(s->d_union);
  if (s->d_polygon) s->ctx->dev_free(s->d_polygon);
  if (s->wide) s->ctx->dev_free(s->wide);
  if (s->dev) s->ctx->dev_free(s->dev);
  delete s;
}

static int shapes_create(pcv_ctx* ctx, const pcv_shape* shapes, uint32_t count, bool with_unions, uint32_t num_unions,
                         const uint32_t* union_first, const uint64_t* union_cells, bool with_polygons, uint32_t num_polygons,
                         const uint32_t* polygon_first, const uint32_t* ring_first, const double* vertices, pcv_shapes** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out || (count && !shapes)) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  std::vector<uint32_t> union_shapes, union_of, polygon_shapes, polygon_of;
  std::vector<int32_t> polygon_frame;
  if (with_polygons) {
    std::string why;
    if (pcv_polygon_check_table(num_polygons, polygon_first, ring_first, vertices, &why)) return ctx->fail(PCV_E_INVALID, why);
  }
  if (with_unions) {
    std::string why;
    if (pcv_s2_check_unions(num_unions, union_first, union_cells, &why)) return ctx->fail(PCV_E_INVALID, why);
    for (uint32_t k = 0; num_unions && k < union_first[num_unions]; ++k)
      if (s2::level_of(union_cells[k]) == 0u) return ctx->fail(PCV_E_INVALID, "a union with a level-0 cell has no geometry");
  }
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<PcvShapeDev> h(count);
  std::vector<uint32_t> wide_of;  // the shapes with a PcvShapeWide
  for (uint32_t i = 0; i < count; ++i) {
    const pcv_shape& s = shapes[i];
    PcvShapeDev& d = h[i];
    std::memset(&d, 0, sizeof(d));
    d.kind = d.point_kind = s.kind;
    switch (s.kind) {
      case PCV_SHAPE_ALL: break;
      case PCV_SHAPE_AABB:
        for (int a = 0; a < 3; ++a) {  // Aabb::new: inf / sup of the two corners (aabb.rs:21-26)
          d.bmin[a] = std::fmin(s.params[a], s.params[3 + a]);
          d.bmax[a] = std::fmax(s.params[a], s.params[3 + a]);
        }
        break;
      case PCV_SHAPE_FRUSTUM:
        for (int a = 0; a < 16; ++a) d.clip_from_query[a] = s.params[a];
        break;
      case PCV_SHAPE_FRUSTUM_WITH_INVERSE:
        for (int a = 0; a < 16; ++a) {
          d.clip_from_query[a] = s.params[a];
          d.query_from_clip[a] = s.params[16 + a];
        }
        break;
      case PCV_SHAPE_OBB:
        for (int a = 0; a < 7; ++a) d.iso[a] = s.params[a];
        for (int a = 0; a < 3; ++a) d.half[a] = s.params[7 + a];
        break;
      case PCV_SHAPE_WEB_MERCATOR_RECT:  // the corners on the host (libm), everything after them on the device
        d.bmin[0] = s.params[0];
        d.bmin[1] = s.params[1];
        d.bmax[0] = s.params[2];
        d.bmax[1] = s.params[3];
        if (pcv_wmr_corners(s.params, d.corners) != PCV_OK) return ctx->fail(PCV_E_INVALID, "web-mercator rectangle: corners");
        wide_of.push_back(i);
        break;
      case PCV_SHAPE_S2_CELL_UNION:
        if (!with_unions) return ctx->fail(PCV_E_INVALID, "a cell union needs its cells: pcv_shapes_create_ex");
        if (s.reserved < 0 || (uint32_t)s.reserved >= num_unions) return ctx->fail(PCV_E_INVALID, "union index out of range");
        union_shapes.push_back(i);
        union_of.push_back((uint32_t)s.reserved);
        break;
      case PCV_SHAPE_POLYGON: {
        if (!with_polygons) return ctx->fail(PCV_E_INVALID, "a polygon needs its rings: pcv_shapes_create_ex2");
        if (s.reserved < 0 || (uint32_t)s.reserved >= num_polygons) return ctx->fail(PCV_E_INVALID, "polygon index out of range");
        std::string why;
        const uint32_t p = (uint32_t)s.reserved;
        if (pcv_polygon_check_shape(s.params[2], s.params[0], s.params[1], polygon_first[p + 1] - polygon_first[p], ring_first + polygon_first[p],
                                    vertices, &why))
          return ctx->fail(PCV_E_INVALID, "shape " + std::to_string(i) + ": " + why);
        d.polygon.z_min = s.params[0];
        d.polygon.z_max = s.params[1];
        polygon_shapes.push_back(i);
        polygon_of.push_back(p);
        polygon_frame.push_back(s.params[2] == 1.0 ? 1 : 0);
        if (s.params[2] == 1.0) wide_of.push_back(i);  // the rectangle over its vertices (pcv_polygon_prepare_shapes)
        break;
      }
      default: return ctx->fail(PCV_E_INVALID, "unknown shape kind");
    }
  }
  pcv_shapes* r = new pcv_shapes();
  r->ctx = ctx;
  r->count = count;
  r->dev = nullptr;
  r->kinds.resize(count);
  for (uint32_t i = 0; i < count; ++i) r->kinds[i] = shapes[i].kind;
  void* p = nullptr;
  int rc = ctx->dev_alloc(&p, sizeof(PcvShapeDev) * (count ? count : 1));
  if (rc) {
    release_shapes(r);
    return rc;
  }
  r->dev = (PcvShapeDev*)p;
  if (!union_shapes.empty()) {
    r->union_first.assign(union_first, union_first + num_unions + 1);
    r->union_cells.assign(union_cells, union_cells + union_first[num_unions]);
    r->union_shapes = union_shapes;
    r->union_of = union_of;
    if ((rc = pcv_union_prepare_shapes(ctx, r, h.data()))) {
      release_shapes(r);
      return rc;
    }
  }
  if (!polygon_shapes.empty()) {
    const uint32_t nrings = polygon_first[num_polygons];
    r->polygon_first.assign(polygon_first, polygon_first + num_polygons + 1);
    r->ring_first.assign(ring_first, ring_first + nrings + 1);
    r->vertices.assign(vertices, vertices + 2 * (size_t)ring_first[nrings]);
    r->polygon_shapes = polygon_shapes;
    r->polygon_of = polygon_of;
    r->polygon_frame = polygon_frame;
    if ((rc = pcv_polygon_prepare_shapes(ctx, r, h.data()))) {
      release_shapes(r);
      return rc;
    }
  }
  if (!wide_of.empty()) {
    if ((rc = ctx->dev_alloc(&p, sizeof(PcvShapeWide) * wide_of.size()))) {
      release_shapes(r);
      return rc;
    }
    r->wide = (PcvShapeWide*)p;
    for (size_t w = 0; w < wide_of.size(); ++w) {
      h[wide_of[w]].wide = r->wide + w;
    }
  }
  if (count) {
    hipError_t e = hipMemcpyAsync(r->dev, h.data(), sizeof(PcvShapeDev) * count, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(shape_setup_kernel, dim3((count + 63) / 64), dim3(64), 0, ctx->stream, r->dev, count);
      e = hipStreamSynchronize(ctx->stream);  // `h` must outlive the copy
    }
    if (e != hipSuccess) {
      release_shapes(r);
      return ctx->fail(PCV_E_HIP, hipGetErrorString(e));
    }
  }
  *out = r;
  return PCV_OK;
}

extern "C" int pcv_shapes_create(pcv_ctx* ctx, const pcv_shape* shapes, uint32_t count, pcv_shapes** out) {
  return shapes_create(ctx, shapes, count, false, 0, nullptr, nullptr, false, 0, nullptr, nullptr, nullptr, out);
}

extern "C" int pcv_shapes_create_ex(pcv_ctx* ctx, const pcv_shape* shapes, uint32_t count, uint32_t num_unions, const uint32_t* union_first,
                                    const uint64_t* union_cells, pcv_shapes** out) {
  return shapes_create(ctx, shapes, count, true, num_unions, union_first, union_cells, false, 0, nullptr, nullptr, nullptr, out);
}

extern "C" int pcv_shapes_create_ex2(pcv_ctx* ctx, const pcv_shape* shapes, uint32_t count, uint32_t num_unions, const uint32_t* union_first,
                                     const uint64_t* union_cells, uint32_t num_polygons, const uint32_t* polygon_first,
                                     const uint32_t* ring_first, const double* vertices, pcv_shapes** out) {
  return shapes_create(ctx, shapes, count, true, num_unions, union_first, union_cells, true, num_polygons, polygon_first, ring_first, vertices,
                       out);
}

extern "C" void pcv_shapes_free(pcv_shapes* s) {
  if (!s) return;
  release_shapes(s);
}

extern "C" int pcv_shapes_union(pcv_shapes* s, uint32_t i, uint64_t capacity, uint64_t* cells, uint32_t* num_cells) {
  if (!s || i >= s->count) return PCV_E_INVALID;
  const auto it = std::lower_bound(s->union_shapes.begin(), s->union_shapes.end(), i);
  if (it == s->union_shapes.end() || *it != i) return s->ctx->fail(PCV_E_INVALID, "shape " + std::to_string(i) + " is not a cell union");
  if (!num_cells || (capacity && !cells)) return s->ctx->fail(PCV_E_INVALID, "null argument");
  const uint32_t u = s->union_of[it - s->union_shapes.begin()];
  const uint32_t n = s->union_first[u + 1] - s->union_first[u];
  *num_cells = n;
  if (capacity && n) std::memcpy(cells, s->union_cells.data() + s->union_first[u], 8 * (size_t)std::min<uint64_t>(n, capacity));
  return PCV_OK;
}

extern "C" int pcv_shapes_polygon(pcv_shapes* s, uint32_t i, uint32_t ring_capacity, uint32_t* ring_first, uint32_t* num_rings,
                                  uint32_t vertex_capacity, double* vertices, uint32_t* num_vertices) {
  if (!s || i >= s->count) return PCV_E_INVALID;
  const auto it = std::lower_bound(s->polygon_shapes.begin(), s->polygon_shapes.end(), i);
  if (it == s->polygon_shapes.end() || *it != i) return s->ctx->fail(PCV_E_INVALID, "shape " + std::to_string(i) + " is not a polygon");
  if (!num_rings || !num_vertices || (ring_capacity && !ring_first) || (vertex_capacity && !vertices)) return s->ctx->fail(PCV_E_INVALID, "null argument");
  const uint32_t p = s->polygon_of[it - s->polygon_shapes.begin()];
  const uint32_t r0 = s->polygon_first[p], nr = s->polygon_first[p + 1] - r0, v0 = s->ring_first[r0], nv = s->ring_first[r0 + nr] - v0;
  *num_rings = nr;
  *num_vertices = nv;
  if (ring_capacity >= nr && vertex_capacity >= nv && ring_capacity) {
    for (uint32_t k = 0; k <= nr; ++k) ring_first[k] = s->ring_first[r0 + k] - v0;
    std::memcpy(vertices, s->vertices.data() + 2 * (size_t)v0, 16 * (size_t)nv);
  }
  return PCV_OK;
}

extern "C" uint32_t pcv_shapes_count(const pcv_shapes* s) { return s ? s->count : 0; }

extern "C" int pcv_shapes_get(pcv_shapes* s, uint32_t i, double corners[24], double axes[78], uint32_t* num_axes,
                              int* valid) {
  if (!s || i >= s->count) return PCV_E_INVALID;
  if (s->kinds[i] == PCV_SHAPE_S2_CELL_UNION) return s->ctx->fail(PCV_E_INVALID, "a cell union has no corners or axes: pcv_shapes_union gives its cells");
  if (s->kinds[i] == PCV_SHAPE_POLYGON) return s->ctx->fail(PCV_E_INVALID, "a polygon has no corners or axes: pcv_shapes_polygon gives its rings");
  if (s->kinds[i] != PCV_SHAPE_WEB_MERCATOR_RECT) {  // (all 78 doubles, as ever)
    pcv_ctx* ctx = s->ctx;
    PcvShapeDev h;
    PCV_HIP_CHECK(ctx, hipMemcpy(&h, s->dev + i, sizeof(h), hipMemcpyDeviceToHost));
    if (corners) std::memcpy(corners, h.corners, sizeof(h.corners));
    if (axes) std::memcpy(axes, h.axes, sizeof(h.axes));
    if (num_axes) *num_axes = (uint32_t)h.naxes;
    if (valid) *valid = h.valid;
    return PCV_OK;
  }
  uint32_t na = 0;
  double wide_axes[3 * PCV_WIDE_AXES];
  const int rc = pcv_shapes_get_ex(s, i, corners, wide_axes, PCV_WIDE_AXES, &na, valid);
  if (rc) return rc;
  if (na > PCV_MAX_AXES) return s->ctx->fail(PCV_E_INVALID, "shape has more than 26 axes: use pcv_shapes_get_ex");
  if (axes) std::memcpy(axes, wide_axes, sizeof(double) * 3 * na);
  if (num_axes) *num_axes = na;
  return PCV_OK;
}

extern "C" int pcv_shapes_get_ex(pcv_shapes* s, uint32_t i, double corners[24], double* axes, uint32_t axes_capacity,
                                 uint32_t* num_axes, int* valid) {
  if (!s || i >= s->count) return PCV_E_INVALID;
  pcv_ctx* ctx = s->ctx;
  if (s->kinds[i] == PCV_SHAPE_S2_CELL_UNION) return ctx->fail(PCV_E_INVALID, "a cell union has no corners or axes: pcv_shapes_union gives its cells");
  if (s->kinds[i] == PCV_SHAPE_POLYGON) return ctx->fail(PCV_E_INVALID, "a polygon has no corners or axes: pcv_shapes_polygon gives its rings");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvShapeDev h;
  PCV_HIP_CHECK(ctx, hipMemcpy(&h, s->dev + i, sizeof(h), hipMemcpyDeviceToHost));
  if (corners) std::memcpy(corners, h.corners, sizeof(h.corners));
  uint32_t na = (uint32_t)h.naxes;
  const double* src = h.axes;
  PcvShapeWide w;
  if (h.kind == PCV_SHAPE_WEB_MERCATOR_RECT) {
    PCV_HIP_CHECK(ctx, hipMemcpy(&w, h.wide, sizeof(w), hipMemcpyDeviceToHost));
    na = (uint32_t)w.naxes;
    src = w.axes;
  }
  if (axes) std::memcpy(axes, src, sizeof(double) * 3 * std::min(na, axes_capacity));
  if (num_axes) *num_axes = na;
  if (valid) *valid = h.valid;
  return PCV_OK;
}
