// pcv_contain_dev.h — PointCulling::contains of a prepared shape, per kind: what the point kernels of pcv_query.hip (octree
// nodes) and pcv_s2_points.hip (S2 cells) test every point with. Device only; each source gets its own copy (internal linkage).
#pragma once
#include "pcv_query_dev.h"
#include "pcv_wmr_dev.h"

namespace {

// What contains() needs of a shape, fetched once per wave (wave-uniform: it lives in scalar registers) instead of
// once per point: the clip matrix (frustum), mins / maxs (AABB) or isometry + half extents (OBB). The point kernels
// are compiled per KIND (PCV_SHAPE_FRUSTUM stands for both frustum kinds), so the inner loops carry no shape switch.
template <int KIND>
struct ContainParams {
  double p[KIND == PCV_SHAPE_FRUSTUM ? 16 : KIND == PCV_SHAPE_OBB ? 10 : KIND == PCV_SHAPE_AABB ? 6 : KIND == PCV_SHAPE_WEB_MERCATOR_RECT ? 4 : 1];
};
template <int KIND>
__device__ __forceinline__ ContainParams<KIND> load_contain(const PcvShapeDev* __restrict__ shape) {
  ContainParams<KIND> c;
  if (KIND == PCV_SHAPE_AABB) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      c.p[i] = shape->bmin[i];
      c.p[3 + i] = shape->bmax[i];
    }
  } else if (KIND == PCV_SHAPE_FRUSTUM) {
#pragma unroll
    for (int i = 0; i < 16; ++i) c.p[i] = shape->clip_from_query[i];
  } else if (KIND == PCV_SHAPE_OBB) {
#pragma unroll
    for (int i = 0; i < 7; ++i) c.p[i] = shape->iso[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) c.p[7 + i] = shape->half[i];
  } else if (KIND == PCV_SHAPE_WEB_MERCATOR_RECT) {  // north_west in bmin[0..1], south_east in bmax[0..1]
    c.p[0] = shape->bmin[0];
    c.p[1] = shape->bmin[1];
    c.p[2] = shape->bmax[0];
    c.p[3] = shape->bmax[1];
  } else {
    c.p[0] = 0.0;
  }
  return c;
}
template <int KIND>
__device__ __forceinline__ bool shape_contains(const ContainParams<KIND>& s, V3d p) {
  if (KIND == PCV_SHAPE_AABB) {  // aabb.rs:46-48: mins <= p < maxs
    return s.p[0] <= p.x && s.p[1] <= p.y && s.p[2] <= p.z && p.x < s.p[3] && p.y < s.p[4] && p.z < s.p[5];
  } else if (KIND == PCV_SHAPE_FRUSTUM) {  // frustum.rs:120-125
    const V3d c = m4_transform_point(s.p, p);
    const double mn = fmin(fmin(c.x, c.y), c.z), mx = fmax(fmax(c.x, c.y), c.z);
    return mn > -1.0 && mx < 1.0;
  } else if (KIND == PCV_SHAPE_OBB) {  // obb.rs:83-90
    const V3d q = v_add(quat_rotate(s.p + 3, p), V3d{s.p[0], s.p[1], s.p[2]});
    return fabs(q.x) <= s.p[7] && fabs(q.y) <= s.p[8] && fabs(q.z) <= s.p[9];
  } else if (KIND == PCV_SHAPE_WEB_MERCATOR_RECT) {  // web_mercator_rect.rs:121-127: the chain of pcv_wmr_dev.h
    return wmr::contains(s.p, p.x, p.y, p.z);
  }
  return true;  // AllPoints
}

}  // namespace
