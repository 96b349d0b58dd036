// pcv_query.hip — per-point culling, the point queries and the batch for gfx950.
//
//   K8  cull_points      FilteredIterator keep mask (src/iterator.rs:96-119; frustum.rs:120-125, obb.rs:83-90,
//                        aabb.rs:46-48), on raw f64 positions or on a node's encoded bytes decoded on the fly
//                        (src/read_write/codec.rs:124-139)
//   K9  transform_points Isometry3 * Point3 (xray/src/generation.rs:493-497)
//   N3  pcv_query_points / _node_points, N3b pcv_query_batch_*, N4 pcv_octree_nodes_blob
//
// The shapes come prepared from pcv_shapes.hip. Node culling is pcv_cull.hip's: the point query reaches it through
// pcv_launch_relation_row and pcv_launch_node_lists (pcv_query_dev.h), never through a kernel.
// Arithmetic follows the nalgebra 0.22 formulas restated in DESIGN.md ("query arithmetic"): left-to-right dot
// products, gemv column accumulation, no fused multiply-add (-ffp-contract=off). Bound: K8 / K9 are HBM streams.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "pcv_query_dev.h"
#include "pcv_wmr_dev.h"
#include "pcv_contain_dev.h"
#include "pcv_polygon_dev.h"
#include "pcv_s2_dev.h"

namespace {

// the kernel instance of a shape kind
#define PCV_DISPATCH_KIND(kind, CALL)                                  \
  switch (kind) {                                                      \
    case PCV_SHAPE_AABB: CALL(PCV_SHAPE_AABB); break;                  \
    case PCV_SHAPE_FRUSTUM:                                            \
    case PCV_SHAPE_FRUSTUM_WITH_INVERSE: CALL(PCV_SHAPE_FRUSTUM); break; \
    case PCV_SHAPE_OBB: CALL(PCV_SHAPE_OBB); break;                    \
    case PCV_SHAPE_WEB_MERCATOR_RECT: CALL(PCV_SHAPE_WEB_MERCATOR_RECT); break; \
    default: CALL(PCV_SHAPE_ALL); break;                               \
  }

// ---- wave chunks -------------------------------------------------------------------------------------------------
// A wave owns one chunk of consecutive points: kGroup x m of them, m chosen on the host so that the chunk's encoded
// bytes (3, 6, 12 or 24 per point; 16-byte aligned per node in the blob) fill at most kStageSlots 16-byte LDS slots.
// When the chunk lies in one node, those bytes are fetched with aligned 16-byte loads, all issued before the first is
// used (6 KiB in flight per wave — the kernel is latency bound, so bytes in flight are what buy bandwidth), and
// decoded from LDS; the keep flags leave as one dword store per lane and group of 256 points.
constexpr uint32_t kGroup = 256;                       // points per keep-store group (4 ballots)
constexpr uint32_t kStageSlots = kGroup * 24 / 16 + 1;  // uint4 slots per wave: 6 KiB of codes + the alignment skew
constexpr uint32_t kStageLoads = (kStageSlots + 63) / 64;

static inline uint32_t enc_stride_host(uint32_t enc) { return 3u * (uint32_t)pcv_bytes_per_coordinate(enc); }
// points per wave for nodes of at most `max_stride` encoded bytes per point
static inline uint32_t chunk_points(uint32_t max_stride) { return kGroup * (24u / max_stride); }

// The chunk's aligned 16-byte pieces, in registers between stage_issue (all loads in flight) and stage_commit (LDS).
// src = blob + off: the pointer keeps the blob's (global) address space, so the loads are global_load_dwordx4.
struct StageRegs {
  uint4 t0, t1, t2, t3, t4, t5, t6;
  uint32_t skew, n16;
};
static_assert(kStageLoads == 7, "the staging loads are written out by hand");
__device__ __forceinline__ StageRegs stage_issue(const uint8_t* __restrict__ blob, uint64_t off, uint32_t nbytes, uint32_t lane) {
  StageRegs r;
  r.skew = (uint32_t)((reinterpret_cast<uintptr_t>(blob) + off) & 15u);
  const uint4* g = reinterpret_cast<const uint4*>(blob + (off - r.skew));
  r.n16 = (r.skew + nbytes + 15u) >> 4;
  const uint32_t last = r.n16 - 1;  // slots past the end re-read the last one: no branches between the loads
  r.t0 = g[min(lane, last)];
  r.t1 = g[min(lane + 64u, last)];
  r.t2 = g[min(lane + 128u, last)];
  r.t3 = g[min(lane + 192u, last)];
  r.t4 = g[min(lane + 256u, last)];
  r.t5 = g[min(lane + 320u, last)];
  r.t6 = g[min(lane + 384u, last)];
  return r;
}
__device__ __forceinline__ void stage_commit(const StageRegs& r, uint4* stage, uint32_t lane) {
  if (lane < r.n16) stage[lane] = r.t0;
  if (lane + 64u < r.n16) stage[lane + 64u] = r.t1;
  if (lane + 128u < r.n16) stage[lane + 128u] = r.t2;
  if (lane + 192u < r.n16) stage[lane + 192u] = r.t3;
  if (lane + 256u < r.n16) stage[lane + 256u] = r.t4;
  if (lane + 320u < r.n16) stage[lane + 320u] = r.t5;
  if (lane + 384u < r.n16) stage[lane + 384u] = r.t6;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int ENC>
__device__ __forceinline__ V3d staged_point(const uint8_t* at, const double* cube_min, double cube_edge) {
  uint64_t c[3];
  if (ENC == PCV_ENC_UINT8) {
    c[0] = at[0];
    c[1] = at[1];
    c[2] = at[2];
  } else if (ENC == PCV_ENC_UINT16) {
    const uint16_t* q = reinterpret_cast<const uint16_t*>(at);
    c[0] = q[0];
    c[1] = q[1];
    c[2] = q[2];
  } else if (ENC == PCV_ENC_FLOAT32) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(at);
    c[0] = q[0];
    c[1] = q[1];
    c[2] = q[2];
  } else {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(at);
    c[0] = q[0];
    c[1] = q[1];
    c[2] = q[2];
  }
  return {pcv_decode_coord(ENC, c[0], cube_min[0], cube_edge), pcv_decode_coord(ENC, c[1], cube_min[1], cube_edge),
          pcv_decode_coord(ENC, c[2], cube_min[2], cube_edge)};
}

__device__ __forceinline__ uint32_t enc_stride(uint32_t enc) {
  return enc == PCV_ENC_UINT8 ? 3u : enc == PCV_ENC_UINT16 ? 6u : enc == PCV_ENC_FLOAT32 ? 12u : 24u;
}

// a group's keep flags from its 4 ballots (lane l of ballot r = point 64 r + l): lane l writes points 4 l .. 4 l + 3
__device__ __forceinline__ void store_keep(uint8_t* __restrict__ keep, uint32_t cnt, const unsigned long long b[4],
                                           uint32_t lane) {
  const uint32_t r = lane >> 4;
  const unsigned long long sel = r == 0 ? b[0] : r == 1 ? b[1] : r == 2 ? b[2] : b[3];
  const uint32_t bits = (uint32_t)(sel >> ((lane & 15u) * 4u)) & 0xfu;
  const uint32_t word = (bits * 0x00204081u) & 0x01010101u;  // bit j -> byte j
  const uint32_t q = lane * 4;
  if ((reinterpret_cast<uintptr_t>(keep) & 3u) == 0 && q + 3 < cnt) {
    *reinterpret_cast<uint32_t*>(keep + q) = word;
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
      if (q + j < cnt) keep[q + j] = (uint8_t)((word >> (8 * j)) & 1u);
  }
}

// keep flags of one chunk of `cnt` points of ONE node whose encoded bytes sit in the wave's LDS slice at `skew`
// (attr = the chunk's first attribute or null); returns how many were kept
template <int KIND, int ENC>
__device__ __forceinline__ uint32_t staged_keep_enc(const ContainParams<KIND>& shape, const uint4* stage, uint32_t skew,
                                                    const double* cube_min, double cube_edge, uint32_t cnt,
                                                    const float* __restrict__ attr, double lo, double hi, uint32_t lane,
                                                    uint8_t* __restrict__ keep) {
  constexpr uint32_t stride = ENC == PCV_ENC_UINT8 ? 3u : ENC == PCV_ENC_UINT16 ? 6u : ENC == PCV_ENC_FLOAT32 ? 12u : 24u;
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage) + skew;
  uint32_t tot = 0;
  for (uint32_t g0 = 0; g0 < cnt; g0 += kGroup) {
    unsigned long long b[4];
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t q = g0 + r * 64 + lane;
      bool k = false;
      if (q < cnt) {
        k = shape_contains<KIND>(shape, staged_point<ENC>(bytes + q * stride, cube_min, cube_edge));
        if (attr) {  // iterator.rs:82-91 + math/mod.rs:86-88
          const double a = (double)attr[q];
          k = k && (lo <= a && a <= hi);
        }
      }
      b[r] = __ballot(k);
    }
    store_keep(keep + g0, cnt - g0, b, lane);
    tot += (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]));
  }
  return tot;
}
// The same for a web-mercator rectangle. The test is some hundreds of f64 operations per point (three atan2, two sin / cos,
// a ln, a sqrt and nine divisions), so the kernel is bound by the f64 pipe, not by HBM: the decode is the (wave-uniform) switch
// and the chain exists ONCE in the instance — not once per encoding and unrolled ballot, which would be 16 copies of it.
__device__ __forceinline__ uint32_t staged_keep_wmr(const ContainParams<PCV_SHAPE_WEB_MERCATOR_RECT>& shape, const uint4* stage,
                                                    uint32_t skew, uint32_t enc, const double* cube_min, double cube_edge,
                                                    uint32_t cnt, const float* __restrict__ attr, double lo, double hi,
                                                    uint32_t lane, uint8_t* __restrict__ keep) {
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage) + skew;
  uint32_t tot = 0;
  for (uint32_t g0 = 0; g0 < cnt; g0 += kGroup) {
    unsigned long long b[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t q = g0 + r * 64 + lane;
      bool k = false;
      if (q < cnt) {
        V3d p;
        switch (enc) {  // wave-uniform
          case PCV_ENC_UINT8: p = staged_point<PCV_ENC_UINT8>(bytes + q * 3u, cube_min, cube_edge); break;
          case PCV_ENC_UINT16: p = staged_point<PCV_ENC_UINT16>(bytes + q * 6u, cube_min, cube_edge); break;
          case PCV_ENC_FLOAT32: p = staged_point<PCV_ENC_FLOAT32>(bytes + q * 12u, cube_min, cube_edge); break;
          default: p = staged_point<PCV_ENC_FLOAT64>(bytes + q * 24u, cube_min, cube_edge); break;
        }
        k = true;
        if (attr) {  // iterator.rs:82-91 + math/mod.rs:86-88 — first: a point outside the interval skips the chain
          const double a = (double)attr[q];
          k = lo <= a && a <= hi;
        }
        if (k) k = wmr::contains(shape.p, p.x, p.y, p.z);
      }
      const unsigned long long bal = __ballot(k);
      b[0] = r == 0 ? bal : b[0];
      b[1] = r == 1 ? bal : b[1];
      b[2] = r == 2 ? bal : b[2];
      b[3] = r == 3 ? bal : b[3];
    }
    store_keep(keep + g0, cnt - g0, b, lane);
    tot += (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]));
  }
  return tot;
}
// The same for a cell union (PointLocation::S2Cells): CellUnion::contains_cellid(CellID::from_point(p)) on the decoded position —
// the leaf id by pcv_s2_dev.h's chain (a sqrt, three divisions, thirty curve steps), then a binary search in the union's ascending
// cells. Like the web-mercator chain it exists once, in kernels of its own (query_flags_union_kernel, cull_points_union_kernel).
__device__ __forceinline__ uint32_t staged_keep_union(const uint64_t* __restrict__ cells, uint32_t ncells, const uint4* stage, uint32_t skew,
                                                      uint32_t enc, const double* cube_min, double cube_edge, uint32_t cnt,
                                                      const float* __restrict__ attr, double lo, double hi, uint32_t lane,
                                                      uint8_t* __restrict__ keep) {
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage) + skew;
  uint32_t tot = 0;
  for (uint32_t g0 = 0; g0 < cnt; g0 += kGroup) {
    unsigned long long b[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t q = g0 + r * 64 + lane;
      bool k = false;
      if (q < cnt) {
        V3d p;
        switch (enc) {  // wave-uniform
          case PCV_ENC_UINT8: p = staged_point<PCV_ENC_UINT8>(bytes + q * 3u, cube_min, cube_edge); break;
          case PCV_ENC_UINT16: p = staged_point<PCV_ENC_UINT16>(bytes + q * 6u, cube_min, cube_edge); break;
          case PCV_ENC_FLOAT32: p = staged_point<PCV_ENC_FLOAT32>(bytes + q * 12u, cube_min, cube_edge); break;
          default: p = staged_point<PCV_ENC_FLOAT64>(bytes + q * 24u, cube_min, cube_edge); break;
        }
        k = s2::union_contains(cells, ncells, s2::leaf_from_point(p.x, p.y, p.z));
        if (attr) {  // iterator.rs:82-91 + math/mod.rs:86-88
          const double a = (double)attr[q];
          k = k && (lo <= a && a <= hi);
        }
      }
      const unsigned long long bal = __ballot(k);
      b[0] = r == 0 ? bal : b[0];
      b[1] = r == 1 ? bal : b[1];
      b[2] = r == 2 ? bal : b[2];
      b[3] = r == 3 ? bal : b[3];
    }
    store_keep(keep + g0, cnt - g0, b, lane);
    tot += (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]));
  }
  return tot;
}
// The same for a polygon (PCV_SHAPE_POLYGON): the point rule of pcv_polygon_dev.h on the decoded position (xy frame,
// with the closed z range) or on its web-mercator projection (the chain of pcv_wmr_dev.h, once per point). What the test needs of
// the shape is wave-uniform; the edge loop runs outside every divergent branch, so its trip count and its addresses are uniform
// too and the table is read with scalar loads. Like the chains above it exists once, in kernels of its own.
struct PolygonParams {
  const double* edges;
  uint32_t nedges;
  int32_t frame;
  double z_min, z_max;
};
__device__ __forceinline__ PolygonParams load_polygon(const PcvShapeDev* __restrict__ sh) {
  return PolygonParams{sh->polygon.edges, sh->polygon.nedges, sh->polygon.frame, sh->polygon.z_min, sh->polygon.z_max};
}
// `live`: the lane holds a point (p is anything otherwise)
__device__ __forceinline__ bool polygon_keep(const PolygonParams& pg, bool live, V3d p) {
  double px = p.x, py = p.y;
  bool k = live;
  if (pg.frame) {  // wave-uniform
    if (live) wmr::project(p.x, p.y, p.z, &px, &py);
  } else {
    k = k && (pg.z_min <= p.z && p.z <= pg.z_max);
  }
  return poly::inside(pg.edges, pg.nedges, px, py) && k;
}
__device__ __forceinline__ uint32_t staged_keep_polygon(const PolygonParams& pg, const uint4* stage, uint32_t skew, uint32_t enc,
                                                        const double* cube_min, double cube_edge, uint32_t cnt,
                                                        const float* __restrict__ attr, double lo, double hi, uint32_t lane,
                                                        uint8_t* __restrict__ keep) {
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage) + skew;
  uint32_t tot = 0;
  for (uint32_t g0 = 0; g0 < cnt; g0 += kGroup) {
    unsigned long long b[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (uint32_t r = 0; r < 4; ++r) {
      const uint32_t q = g0 + r * 64 + lane;
      const bool live = q < cnt;
      V3d p = {0.0, 0.0, 0.0};
      bool in_interval = true;
      if (live) {
        switch (enc) {  // wave-uniform
          case PCV_ENC_UINT8: p = staged_point<PCV_ENC_UINT8>(bytes + q * 3u, cube_min, cube_edge); break;
          case PCV_ENC_UINT16: p = staged_point<PCV_ENC_UINT16>(bytes + q * 6u, cube_min, cube_edge); break;
          case PCV_ENC_FLOAT32: p = staged_point<PCV_ENC_FLOAT32>(bytes + q * 12u, cube_min, cube_edge); break;
          default: p = staged_point<PCV_ENC_FLOAT64>(bytes + q * 24u, cube_min, cube_edge); break;
        }
        if (attr) {  // iterator.rs:82-91 + math/mod.rs:86-88
          const double a = (double)attr[q];
          in_interval = lo <= a && a <= hi;
        }
      }
      const bool k = polygon_keep(pg, live, p) && in_interval;
      const unsigned long long bal = __ballot(k);
      b[0] = r == 0 ? bal : b[0];
      b[1] = r == 1 ? bal : b[1];
      b[2] = r == 2 ? bal : b[2];
      b[3] = r == 3 ? bal : b[3];
    }
    store_keep(keep + g0, cnt - g0, b, lane);
    tot += (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]));
  }
  return tot;
}
template <int KIND>
__device__ __forceinline__ uint32_t staged_keep(const ContainParams<KIND>& shape, const uint4* stage, uint32_t skew,
                                                uint32_t enc, const double* cube_min, double cube_edge, uint32_t cnt,
                                                const float* __restrict__ attr, double lo, double hi, uint32_t lane,
                                                uint8_t* __restrict__ keep) {
  if constexpr (KIND == PCV_SHAPE_WEB_MERCATOR_RECT) {
    return staged_keep_wmr(shape, stage, skew, enc, cube_min, cube_edge, cnt, attr, lo, hi, lane, keep);
  } else {
    switch (enc) {  // wave-uniform
      case PCV_ENC_UINT8:
        return staged_keep_enc<KIND, PCV_ENC_UINT8>(shape, stage, skew, cube_min, cube_edge, cnt, attr, lo, hi, lane, keep);
      case PCV_ENC_UINT16:
        return staged_keep_enc<KIND, PCV_ENC_UINT16>(shape, stage, skew, cube_min, cube_edge, cnt, attr, lo, hi, lane, keep);
      case PCV_ENC_FLOAT32:
        return staged_keep_enc<KIND, PCV_ENC_FLOAT32>(shape, stage, skew, cube_min, cube_edge, cnt, attr, lo, hi, lane, keep);
      default:
        return staged_keep_enc<KIND, PCV_ENC_FLOAT64>(shape, stage, skew, cube_min, cube_edge, cnt, attr, lo, hi, lane, keep);
    }
  }
}

// K8 on one view (raw f64 SoA, or one node's encoded bytes): a wave per `chunk` points, one counter update per workgroup
template <int KIND>
__global__ __launch_bounds__(256) void cull_points_kernel(const PcvShapeDev* __restrict__ shape_dev, PointsView v, uint32_t chunk,
                                                           uint8_t* __restrict__ keep, unsigned long long* __restrict__ kept) {
  __shared__ uint4 stage[4][kStageSlots];
  __shared__ uint32_t wave_cnt[4];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t base = ((uint64_t)blockIdx.x * 4 + wave) * chunk;
  uint32_t tot = 0;
  if (base < v.n) {
    const ContainParams<KIND> shape = load_contain<KIND>(shape_dev);
    const uint32_t cnt = (uint32_t)(v.n - base < chunk ? v.n - base : chunk);
    if (v.encoded) {
      const StageRegs sr = stage_issue(v.encoded, base * enc_stride(v.enc), cnt * enc_stride(v.enc), lane);
      stage_commit(sr, stage[wave], lane);
      tot = staged_keep<KIND>(shape, stage[wave], sr.skew, v.enc, v.cube_min, v.cube_edge, cnt,
                        v.has_interval ? v.attr + base : nullptr, v.lo, v.hi, lane, keep + base);
    } else {
      for (uint32_t g0 = 0; g0 < cnt; g0 += kGroup) {
        unsigned long long b[4];
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
          const uint32_t q = g0 + r * 64 + lane;
          bool k = false;
          if (q < cnt) {
            const uint64_t i = base + q;
            k = shape_contains<KIND>(shape, V3d{v.x[i], v.y[i], v.z[i]});
            if (v.has_interval) {
              const double a = (double)v.attr[i];
              k = k && (v.lo <= a && a <= v.hi);
            }
          }
          b[r] = __ballot(k);
        }
        store_keep(keep + base + g0, cnt - g0, b, lane);
        tot += (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]));
      }
    }
  }
  if (lane == 0) wave_cnt[wave] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (t) atomicAdd(kept, (unsigned long long)t);
  }
}

// K8 for a cell union: cull_points_kernel's frame around the union's own test
__global__ __launch_bounds__(256) void cull_points_union_kernel(const PcvShapeDev* __restrict__ shape_dev, PointsView v, uint32_t chunk,
                                                                 uint8_t* __restrict__ keep, unsigned long long* __restrict__ kept) {
  __shared__ uint4 stage[4][kStageSlots];
  __shared__ uint32_t wave_cnt[4];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t base = ((uint64_t)blockIdx.x * 4 + wave) * chunk;
  uint32_t tot = 0;
  if (base < v.n) {
    const uint64_t* cells = shape_dev->cell_union.cells;
    const uint32_t ncells = shape_dev->cell_union.count;
    const uint32_t cnt = (uint32_t)(v.n - base < chunk ? v.n - base : chunk);
    if (v.encoded) {
      const StageRegs sr = stage_issue(v.encoded, base * enc_stride(v.enc), cnt * enc_stride(v.enc), lane);
      stage_commit(sr, stage[wave], lane);
      tot = staged_keep_union(cells, ncells, stage[wave], sr.skew, v.enc, v.cube_min, v.cube_edge, cnt,
                              v.has_interval ? v.attr + base : nullptr, v.lo, v.hi, lane, keep + base);
    } else {
      for (uint32_t g0 = 0; g0 < cnt; g0 += kGroup) {
        unsigned long long b[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (uint32_t r = 0; r < 4; ++r) {
          const uint32_t q = g0 + r * 64 + lane;
          bool k = false;
          if (q < cnt) {
            const uint64_t i = base + q;
            k = s2::union_contains(cells, ncells, s2::leaf_from_point(v.x[i], v.y[i], v.z[i]));
            if (v.has_interval) {
              const double a = (double)v.attr[i];
              k = k && (v.lo <= a && a <= v.hi);
            }
          }
          const unsigned long long bal = __ballot(k);
          b[0] = r == 0 ? bal : b[0];
          b[1] = r == 1 ? bal : b[1];
          b[2] = r == 2 ? bal : b[2];
          b[3] = r == 3 ? bal : b[3];
        }
        store_keep(keep + base + g0, cnt - g0, b, lane);
        tot += (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]));
      }
    }
  }
  if (lane == 0) wave_cnt[wave] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (t) atomicAdd(kept, (unsigned long long)t);
  }
}

// K8 for a polygon: cull_points_kernel's frame around the polygon's own test
__global__ __launch_bounds__(256) void cull_points_polygon_kernel(const PcvShapeDev* __restrict__ shape_dev, PointsView v, uint32_t chunk,
                                                                   uint8_t* __restrict__ keep, unsigned long long* __restrict__ kept) {
  __shared__ uint4 stage[4][kStageSlots];
  __shared__ uint32_t wave_cnt[4];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t base = ((uint64_t)blockIdx.x * 4 + wave) * chunk;
  uint32_t tot = 0;
  if (base < v.n) {
    const PolygonParams pg = load_polygon(shape_dev);
    const uint32_t cnt = (uint32_t)(v.n - base < chunk ? v.n - base : chunk);
    if (v.encoded) {
      const StageRegs sr = stage_issue(v.encoded, base * enc_stride(v.enc), cnt * enc_stride(v.enc), lane);
      stage_commit(sr, stage[wave], lane);
      tot = staged_keep_polygon(pg, stage[wave], sr.skew, v.enc, v.cube_min, v.cube_edge, cnt, v.has_interval ? v.attr + base : nullptr, v.lo,
                                v.hi, lane, keep + base);
    } else {
      for (uint32_t g0 = 0; g0 < cnt; g0 += kGroup) {
        unsigned long long b[4] = {0, 0, 0, 0};
#pragma unroll 1
        for (uint32_t r = 0; r < 4; ++r) {
          const uint32_t q = g0 + r * 64 + lane;
          const bool live = q < cnt;
          V3d p = {0.0, 0.0, 0.0};
          bool in_interval = true;
          if (live) {
            const uint64_t i = base + q;
            p = V3d{v.x[i], v.y[i], v.z[i]};
            if (v.has_interval) {
              const double a = (double)v.attr[i];
              in_interval = v.lo <= a && a <= v.hi;
            }
          }
          const bool k = polygon_keep(pg, live, p) && in_interval;
          const unsigned long long bal = __ballot(k);
          b[0] = r == 0 ? bal : b[0];
          b[1] = r == 1 ? bal : b[1];
          b[2] = r == 2 ? bal : b[2];
          b[3] = r == 3 ? bal : b[3];
        }
        store_keep(keep + base + g0, cnt - g0, b, lane);
        tot += (uint32_t)(__popcll(b[0]) + __popcll(b[1]) + __popcll(b[2]) + __popcll(b[3]));
      }
    }
  }
  if (lane == 0) wave_cnt[wave] = tot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    if (t) atomicAdd(kept, (unsigned long long)t);
  }
}

// K9
__global__ __launch_bounds__(256) void transform_points_kernel(uint64_t n, const double* __restrict__ x,
                                                                const double* __restrict__ y, const double* __restrict__ z,
                                                                double t0, double t1, double t2, double q0, double q1,
                                                                double q2, double q3, double* __restrict__ ox,
                                                                double* __restrict__ oy, double* __restrict__ oz) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double q[4] = {q0, q1, q2, q3};
  const V3d r = v_add(quat_rotate(q, V3d{x[i], y[i], z[i]}), V3d{t0, t1, t2});
  ox[i] = r.x;
  oy[i] = r.y;
  oz[i] = r.z;
}

// ---- point query (the work of ParallelIterator + FilteredIterator for one or many locations) ----------
// A segment is one (shape, node) pair, in traversal order. Every segment is cut into chunks of its node's own size — as many
// points as fill a wave's LDS slice at the node's encoding (256 f64, 512 f32, 1024 u16, 2048 u8 points), >> shift — so a chunk
// never spans two nodes, and segments are padded to 4 flags so that the keep flags of a chunk start on a 4-byte boundary.
//   chunks   one 64-byte descriptor per chunk; `enc` carries the kind and the shape index
//   flags    keep flag per point + kept count per chunk (query_flags_kernel)
//   scan     kept points per chunk -> u64 offsets (pcv_batch_scan)
//   compact  the kept points of a range of chunks into the caller's buffers (query_compact_kernel)
struct BatchIval {  // ClosedInterval of one shape on intensity
  double lo, hi;
  uint32_t used, pad;
};

// the chunk size of a query over `total` points (or flags): small queries get smaller chunks (more waves, each with less
// serial work)
inline uint32_t chunk_shift(uint64_t total) { return total < (1u << 19) ? 2u : total < (1u << 22) ? 1u : 0u; }

// the descriptor of chunk c of the segment of node `nd` whose first chunk is `first_chunk` and first flag `first_flag`, for
// shape `shape` of kind `kind`; chunks hold (LDS slice / stride) >> shift points
__host__ __device__ inline ChunkDesc make_chunk_desc(const BatchNode& nd, uint64_t first_chunk, uint64_t first_flag, uint32_t shape,
                                                     int32_t kind, uint64_t c, uint32_t shift) {
  const uint32_t stride = nd.enc == PCV_ENC_UINT8 ? 3u : nd.enc == PCV_ENC_UINT16 ? 6u : nd.enc == PCV_ENC_FLOAT32 ? 12u : 24u;
  const uint32_t per = (kGroup * (24u / stride)) >> shift;
  const uint64_t kk = (c - first_chunk) * per;
  if (kind == PCV_SHAPE_FRUSTUM_WITH_INVERSE) kind = PCV_SHAPE_FRUSTUM;  // the point test needs the clip matrix only
  ChunkDesc d;
  d.src = nd.xyz_off + kk * stride;
  d.attr_index = nd.point_off + kk;
  d.cube_min[0] = nd.cube_min[0];
  d.cube_min[1] = nd.cube_min[1];
  d.cube_min[2] = nd.cube_min[2];
  d.cube_edge = nd.cube_edge;
  d.keep_off = first_flag + kk;
  d.enc = nd.enc | ((uint32_t)kind << 4) | (shape << 8);
  d.cnt = (uint32_t)(nd.n - kk < per ? nd.n - kk : per);
  return d;
}

// one descriptor per chunk: its segment is the last one whose first chunk is <= c (empty segments share their
// successor's first chunk), its shape the last one whose first segment is <= that segment
__global__ __launch_bounds__(256) void query_chunks_kernel(const uint64_t* __restrict__ shape_first, uint32_t nshapes,
                                                            const PcvShapeDev* __restrict__ shapes, const uint32_t* __restrict__ seg_node,
                                                            const uint64_t* __restrict__ seg_chunk, const uint64_t* __restrict__ seg_flags,
                                                            uint64_t nseg, const BatchNode* __restrict__ nodes, uint64_t nchunks,
                                                            uint32_t shift, ChunkDesc* __restrict__ desc) {
  for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += (uint64_t)gridDim.x * 256) {
    uint64_t lo = 0, hi = nseg;
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (seg_chunk[mid] <= c) lo = mid;
      else hi = mid;
    }
    uint32_t a = 0, b = nshapes;
    while (b - a > 1) {
      const uint32_t mid = (a + b) >> 1;
      if (shape_first[mid] <= lo) a = mid;
      else b = mid;
    }
    const BatchNode nd = nodes[seg_node[lo]];
    desc[c] = make_chunk_desc(nd, seg_chunk[lo], seg_flags[lo], a, shapes[a].point_kind, c, shift);
  }
}

// keep flags of one chunk: the shape and its interval are the chunk's (scalar loads), the kind a wave-uniform switch; KIND >= 0:
// one location, every chunk of shape 0 and kind KIND (the shape's loads do not depend on the chunk)
template <int KIND>
__device__ __forceinline__ uint32_t query_keep_chunk(const PcvShapeDev* __restrict__ shapes, const BatchIval* __restrict__ ivals,
                                                     const ChunkDesc& d, const uint4* stage, uint32_t skew,
                                                     const float* __restrict__ inten_blob, uint8_t* __restrict__ keep, uint32_t lane) {
  const uint32_t s = KIND >= 0 ? 0u : d.enc >> 8, kind = KIND >= 0 ? (uint32_t)KIND : (d.enc >> 4) & 15u, enc = d.enc & 15u;
  const PcvShapeDev* sh = shapes + s;
  const BatchIval iv = ivals[s];
  const float* attr = iv.used ? inten_blob + d.attr_index : nullptr;
  uint8_t* kp = keep + d.keep_off;
  // A web-mercator rectangle has its own instance only. In a mixed batch (KIND < 0) the chain stays out of the instance the other
  // kinds run in, whose code is what it was: to it such a chunk is the default case (every flag 1), and query_flags_wmr_kernel,
  // launched behind it on the same stream, stages the chunk again and overwrites its flags and its count.
  if constexpr (KIND == PCV_SHAPE_WEB_MERCATOR_RECT)
    return staged_keep<PCV_SHAPE_WEB_MERCATOR_RECT>(load_contain<PCV_SHAPE_WEB_MERCATOR_RECT>(sh), stage, skew, enc, d.cube_min,
                                                    d.cube_edge, d.cnt, attr, iv.lo, iv.hi, lane, kp);
  switch (kind) {
    case PCV_SHAPE_AABB:
      return staged_keep<PCV_SHAPE_AABB>(load_contain<PCV_SHAPE_AABB>(sh), stage, skew, enc, d.cube_min, d.cube_edge, d.cnt, attr,
                                         iv.lo, iv.hi, lane, kp);
    case PCV_SHAPE_FRUSTUM:
      return staged_keep<PCV_SHAPE_FRUSTUM>(load_contain<PCV_SHAPE_FRUSTUM>(sh), stage, skew, enc, d.cube_min, d.cube_edge, d.cnt,
                                            attr, iv.lo, iv.hi, lane, kp);
    case PCV_SHAPE_OBB:
      return staged_keep<PCV_SHAPE_OBB>(load_contain<PCV_SHAPE_OBB>(sh), stage, skew, enc, d.cube_min, d.cube_edge, d.cnt, attr,
                                        iv.lo, iv.hi, lane, kp);
    default:
      return staged_keep<PCV_SHAPE_ALL>(load_contain<PCV_SHAPE_ALL>(sh), stage, skew, enc, d.cube_min, d.cube_edge, d.cnt, attr,
                                        iv.lo, iv.hi, lane, kp);
  }
}

// keep flag per point of every chunk + kept count per chunk. Persistent waves: wave w takes chunks w, w + W, ... and has the
// next chunk's encoded bytes in flight (registers) and the descriptor after that on its way while it decodes the current chunk
// from LDS, so a chunk's memory latency hides behind the f64 work of the one before. KIND: as query_keep_chunk.
template <int KIND>
__global__ __launch_bounds__(256) void query_flags_kernel(const PcvShapeDev* __restrict__ shapes, const BatchIval* __restrict__ ivals,
                                                           const ChunkDesc* __restrict__ desc, uint32_t nchunks,
                                                           const uint8_t* __restrict__ xyz_blob, const float* __restrict__ inten_blob,
                                                           uint8_t* __restrict__ keep, uint32_t* __restrict__ chunk_counts) {
  __shared__ uint4 stage_all[4][kStageSlots];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint4* stage = stage_all[wave];
  const uint32_t nwaves = gridDim.x * 4;
  uint32_t c = blockIdx.x * 4 + wave;
  if (c >= nchunks) return;
  ChunkDesc d = desc[c];  // wave-uniform: scalar loads
  ChunkDesc dn = desc[min(c + nwaves, nchunks - 1)];
  StageRegs sr = stage_issue(xyz_blob, d.src, d.cnt * enc_stride(d.enc & 15u), lane);
  for (;;) {
    const uint32_t skew = sr.skew;
    stage_commit(sr, stage, lane);
    const uint32_t cn = c + nwaves;
    if (cn < nchunks) sr = stage_issue(xyz_blob, dn.src, dn.cnt * enc_stride(dn.enc & 15u), lane);
    const ChunkDesc dnn = desc[min(cn + nwaves, nchunks - 1)];
    const uint32_t tot = query_keep_chunk<KIND>(shapes, ivals, d, stage, skew, inten_blob, keep, lane);
    if (lane == 0) chunk_counts[c] = tot;
    if (cn >= nchunks) break;
    // the LDS slice is rewritten by the next commit: every lane must be done reading it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    c = cn;
    d = dn;
    dn = dnn;
  }
}

// The web-mercator chunks of a mixed batch: query_flags_kernel<-1> treated them as AllPoints chunks (their bytes are read twice,
// 3..24 B per point against the chain's 358 f64 instructions); this kernel, behind it on the stream, overwrites flags and counts. A wave per chunk, grid-stride, the other kinds' chunks skipped at the cost of their descriptor's scalar load. No prefetch of the next chunk: the f64 work of a chunk
// (some 10^5 operations per wave) dwarfs its 6 KiB of loads, and the waves of a SIMD overlap the rest.
__global__ __launch_bounds__(256) void query_flags_wmr_kernel(const PcvShapeDev* __restrict__ shapes, const BatchIval* __restrict__ ivals,
                                                               const ChunkDesc* __restrict__ desc, uint32_t nchunks,
                                                               const uint8_t* __restrict__ xyz_blob, const float* __restrict__ inten_blob,
                                                               uint8_t* __restrict__ keep, uint32_t* __restrict__ chunk_counts) {
  __shared__ uint4 stage_all[4][kStageSlots];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint4* stage = stage_all[wave];
  const uint32_t nwaves = gridDim.x * 4;
  for (uint32_t c = blockIdx.x * 4 + wave; c < nchunks; c += nwaves) {
    const ChunkDesc d = desc[c];  // wave-uniform: scalar loads
    if (((d.enc >> 4) & 15u) != (uint32_t)PCV_SHAPE_WEB_MERCATOR_RECT) continue;
    const StageRegs sr = stage_issue(xyz_blob, d.src, d.cnt * enc_stride(d.enc & 15u), lane);
    stage_commit(sr, stage, lane);
    const uint32_t tot =
        query_keep_chunk<PCV_SHAPE_WEB_MERCATOR_RECT>(shapes + (d.enc >> 8), ivals + (d.enc >> 8), d, stage, sr.skew, inten_blob, keep, lane);
    if (lane == 0) chunk_counts[c] = tot;
    // the LDS slice is rewritten by the next commit: every lane must be done reading it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// The cell-union chunks, of a mixed batch (behind query_flags_kernel<-1>, to which they were AllPoints chunks, as the web-mercator
// ones are) or of one location (every chunk: shape 0 of `shapes`): a wave per chunk, grid-stride, the other kinds' chunks skipped.
// The shape and its interval are the chunk's (scalar loads).
__global__ __launch_bounds__(256) void query_flags_union_kernel(const PcvShapeDev* __restrict__ shapes, const BatchIval* __restrict__ ivals,
                                                                 const ChunkDesc* __restrict__ desc, uint32_t nchunks,
                                                                 const uint8_t* __restrict__ xyz_blob, const float* __restrict__ inten_blob,
                                                                 uint8_t* __restrict__ keep, uint32_t* __restrict__ chunk_counts) {
  __shared__ uint4 stage_all[4][kStageSlots];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint4* stage = stage_all[wave];
  const uint32_t nwaves = gridDim.x * 4;
  for (uint32_t c = blockIdx.x * 4 + wave; c < nchunks; c += nwaves) {
    const ChunkDesc d = desc[c];  // wave-uniform: scalar loads
    if (((d.enc >> 4) & 15u) != (uint32_t)PCV_SHAPE_S2_CELL_UNION) continue;
    const PcvShapeDev* sh = shapes + (d.enc >> 8);
    const BatchIval iv = ivals[d.enc >> 8];
    const StageRegs sr = stage_issue(xyz_blob, d.src, d.cnt * enc_stride(d.enc & 15u), lane);
    stage_commit(sr, stage, lane);
    const uint32_t tot = staged_keep_union(sh->cell_union.cells, sh->cell_union.count, stage, sr.skew, d.enc & 15u, d.cube_min, d.cube_edge,
                                           d.cnt, iv.used ? inten_blob + d.attr_index : nullptr, iv.lo, iv.hi, lane, keep + d.keep_off);
    if (lane == 0) chunk_counts[c] = tot;
    // the LDS slice is rewritten by the next commit: every lane must be done reading it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// The polygon chunks, of a mixed batch (behind query_flags_kernel<-1>, to which they were AllPoints chunks) or of one location
// (every chunk: shape 0 of `shapes`): a wave per chunk, grid-stride, the other kinds' chunks skipped; 64 points per step in the
// lanes, the edge loop wave-uniform.
__global__ __launch_bounds__(256) void query_flags_polygon_kernel(const PcvShapeDev* __restrict__ shapes, const BatchIval* __restrict__ ivals,
                                                                   const ChunkDesc* __restrict__ desc, uint32_t nchunks,
                                                                   const uint8_t* __restrict__ xyz_blob, const float* __restrict__ inten_blob,
                                                                   uint8_t* __restrict__ keep, uint32_t* __restrict__ chunk_counts) {
  __shared__ uint4 stage_all[4][kStageSlots];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint4* stage = stage_all[wave];
  const uint32_t nwaves = gridDim.x * 4;
  for (uint32_t c = blockIdx.x * 4 + wave; c < nchunks; c += nwaves) {
    const ChunkDesc d = desc[c];  // wave-uniform: scalar loads
    if (((d.enc >> 4) & 15u) != (uint32_t)PCV_SHAPE_POLYGON) continue;
    const PolygonParams pg = load_polygon(shapes + (d.enc >> 8));
    const BatchIval iv = ivals[d.enc >> 8];
    const StageRegs sr = stage_issue(xyz_blob, d.src, d.cnt * enc_stride(d.enc & 15u), lane);
    stage_commit(sr, stage, lane);
    const uint32_t tot = staged_keep_polygon(pg, stage, sr.skew, d.enc & 15u, d.cube_min, d.cube_edge, d.cnt,
                                             iv.used ? inten_blob + d.attr_index : nullptr, iv.lo, iv.hi, lane, keep + d.keep_off);
    if (lane == 0) chunk_counts[c] = tot;
    // the LDS slice is rewritten by the next commit: every lane must be done reading it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- u64 exclusive scan of u32 counters: tile sums, one workgroup over the tile sums, tiles -------------------------
constexpr uint32_t kScanPer = 16, kScanTile = 256 * kScanPer;
__device__ __forceinline__ uint64_t wave_inclusive_scan(uint64_t x, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += t;
  }
  return x;
}
__global__ __launch_bounds__(256) void batch_scan_reduce_kernel(const uint32_t* __restrict__ in, uint64_t n,
                                                                 uint64_t* __restrict__ tile_sums) {
  __shared__ uint64_t part[4];
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
  uint64_t s = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    const uint64_t i = base + j * 256 + threadIdx.x;  // coalesced
    if (i < n) s += in[i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
__global__ __launch_bounds__(1024) void batch_scan_tiles_kernel(uint64_t* __restrict__ sums, uint64_t ntiles,
                                                                 uint64_t* __restrict__ total) {
  __shared__ uint64_t wsum[16];
  __shared__ uint64_t step;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (uint64_t b = 0; b < ntiles; b += 1024) {
    const uint64_t i = b + threadIdx.x;
    const uint64_t v = i < ntiles ? sums[i] : 0;
    const uint64_t inc = wave_inclusive_scan(v, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (wave == 0) {
      const uint64_t w = lane < 16 ? wsum[lane] : 0;
      const uint64_t wi = wave_inclusive_scan(w, lane);
      if (lane < 16) wsum[lane] = wi - w;
      if (lane == 15) step = wi;
    }
    __syncthreads();
    if (i < ntiles) sums[i] = carry + wsum[wave] + inc - v;
    carry += step;
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = carry;
}
// tile_sums null: n fits one tile, its total goes to out[n]
__global__ __launch_bounds__(256) void batch_scan_down_kernel(const uint32_t* __restrict__ in, uint64_t n,
                                                               const uint64_t* __restrict__ tile_sums, uint64_t* __restrict__ out) {
  __shared__ uint64_t wsum[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t first = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanPer;
  uint32_t v[kScanPer];
  uint64_t s = 0;
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    v[j] = first + j < n ? in[first + j] : 0u;
    s += v[j];
  }
  const uint64_t inc = wave_inclusive_scan(s, lane);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint64_t e = (tile_sums ? tile_sums[blockIdx.x] : 0) + inc - s;
  for (uint32_t w = 0; w < wave; ++w) e += wsum[w];
#pragma unroll
  for (uint32_t j = 0; j < kScanPer; ++j) {
    if (first + j < n) out[first + j] = e;
    e += v[j];
  }
  if (!tile_sums && threadIdx.x == 255) out[n] = e;
}

// stable compaction of the chunks [c0, c1): decoded f64 positions, colours and intensity of the kept points, at the chunk's
// scanned offset - `base` + the rank among the chunk's kept points, the first `limit` of them; a wave per chunk, grid-stride
__global__ __launch_bounds__(256) void query_compact_kernel(const ChunkDesc* __restrict__ desc, uint64_t c0, uint64_t c1,
                                                             const uint8_t* __restrict__ xyz_blob, const uint8_t* __restrict__ rgb_blob,
                                                             const float* __restrict__ inten_blob, const uint8_t* __restrict__ keep,
                                                             const uint64_t* __restrict__ chunk_off, uint64_t base, uint64_t limit,
                                                             double* __restrict__ ox, double* __restrict__ oy, double* __restrict__ oz,
                                                             uint8_t* __restrict__ orgb, float* __restrict__ ointen) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  for (uint64_t ci = c0 + (uint64_t)blockIdx.x * 4 + wave; ci < c1; ci += (uint64_t)gridDim.x * 4) {
    uint64_t pos0 = chunk_off[ci] - base;
    if (pos0 >= limit) break;  // (uniform) this chunk and the wave's later ones are past the caller's buffers: offsets only grow
    const ChunkDesc& d = desc[ci];
    const PointsView v = points_view_of(d, xyz_blob);
    const uint8_t* kp = keep + d.keep_off;
    for (uint32_t q0 = 0; q0 < d.cnt; q0 += 64) {
      const uint32_t q = q0 + lane;
      const unsigned long long b = __ballot(q < d.cnt && kp[q]);
      const uint64_t pos = pos0 + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
      if (((b >> lane) & 1ull) && pos < limit) {
        const V3d p = load_point(v, q);
        ox[pos] = p.x;
        oy[pos] = p.y;
        oz[pos] = p.z;
        const uint8_t* c = rgb_blob + 3 * (d.attr_index + q);
        orgb[3 * pos] = c[0];
        orgb[3 * pos + 1] = c[1];
        orgb[3 * pos + 2] = c[2];
        if (ointen) ointen[pos] = inten_blob[d.attr_index + q];
      }
      pos0 += (uint64_t)__popcll(b);
    }
  }
}

// grid of a grid-stride launch over `n` items of `per_block` each
inline uint32_t stride_grid(uint64_t n, uint32_t per_block) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, 1u << 16));
}

// keep flags of `nchunks` chunks, their kept counts in chunk_counts, by `kernel` (an instance of query_flags_kernel, or
// query_flags_wmr_kernel): persistent, as many workgroups as are resident at once
int launch_flags(pcv_ctx* ctx, decltype(&query_flags_wmr_kernel) kernel, const PcvShapeDev* shapes, const BatchIval* ivals,
                 const ChunkDesc* desc, uint32_t nchunks, const pcv_octree* tree, uint8_t* keep, uint32_t* chunk_counts) {
  int cus = 0, per_cu = 0;
  PCV_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0));
  const uint32_t nb = (uint32_t)std::min<uint64_t>((nchunks + 3ull) / 4, (uint64_t)std::max(cus, 1) * (uint64_t)std::max(per_cu, 1));
  hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, ctx->stream, shapes, ivals, desc, nchunks, tree->d_xyz, (const float*)tree->d_int, keep,
                     chunk_counts);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}
// kind < 0: the chunks' own shapes and kinds; otherwise one location (shape 0 of every descriptor) of that kind
int launch_query_flags(pcv_ctx* ctx, int32_t kind, const PcvShapeDev* shapes, const BatchIval* ivals, const ChunkDesc* desc,
                       uint32_t nchunks, const pcv_octree* tree, uint8_t* keep, uint32_t* chunk_counts) {
  if (kind == PCV_SHAPE_S2_CELL_UNION) return launch_flags(ctx, query_flags_union_kernel, shapes, ivals, desc, nchunks, tree, keep, chunk_counts);
  if (kind == PCV_SHAPE_POLYGON) return launch_flags(ctx, query_flags_polygon_kernel, shapes, ivals, desc, nchunks, tree, keep, chunk_counts);
  auto kernel = query_flags_kernel<-1>;
#define PCV_CALL(K) kernel = query_flags_kernel<K>
  if (kind >= 0) {
    PCV_DISPATCH_KIND(kind, PCV_CALL)
  }
#undef PCV_CALL
  return launch_flags(ctx, kernel, shapes, ivals, desc, nchunks, tree, keep, chunk_counts);
}

// The planes of a set of points, in host or device memory: x / y / z and, where set, rgb (3 bytes per point) and intensity.
struct PointPlanes {
  double *x = nullptr, *y = nullptr, *z = nullptr;
  uint8_t* rgb = nullptr;
  float* intensity = nullptr;
};
// device scratch for the planes `like` has
int planes_alloc(PcvScratch& sc, uint64_t n, const PointPlanes& like, PointPlanes* d) {
  int rc;
  if ((rc = sc.get(&d->x, n)) || (rc = sc.get(&d->y, n)) || (rc = sc.get(&d->z, n))) return rc;
  if (like.rgb && (rc = sc.get(&d->rgb, 3 * n))) return rc;
  if (like.intensity && (rc = sc.get(&d->intensity, n))) return rc;
  return PCV_OK;
}
// the planes `dst` has, from `src`, on ctx->stream
int planes_copy(pcv_ctx* ctx, const PointPlanes& dst, const PointPlanes& src, uint64_t n, hipMemcpyKind kind) {
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst.x, src.x, 8 * n, kind, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst.y, src.y, 8 * n, kind, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst.z, src.z, 8 * n, kind, ctx->stream));
  if (dst.rgb) PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst.rgb, src.rgb, 3 * n, kind, ctx->stream));
  if (dst.intensity) PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst.intensity, src.intensity, 4 * n, kind, ctx->stream));
  return PCV_OK;
}

// the kept points of the chunks [c0, c1), which start at scanned offset `base`, the first `np` of them, into the caller's host
// or device buffers; `label` names the compaction in the profile
int compact_chunks(pcv_ctx* ctx, int label, const pcv_octree* tree, const ChunkDesc* desc, const uint8_t* keep, const uint64_t* chunk_off,
                   uint64_t c0, uint64_t c1, uint64_t base, uint64_t np, int mem, double* x, double* y, double* z, uint8_t* rgb,
                   float* intensity) {
  PcvScratch sc(ctx);
  int rc;
  const PointPlanes out{x, y, z, rgb, tree->has_intensity ? intensity : nullptr};
  PointPlanes d = out;
  if (mem == PCV_MEM_HOST && (rc = planes_alloc(sc, np, out, &d))) return rc;
  {
    PcvProf prof(ctx, label);
    hipLaunchKernelGGL(query_compact_kernel, dim3(stride_grid(c1 - c0, 4)), dim3(256), 0, ctx->stream, desc, c0, c1, tree->d_xyz,
                       tree->d_rgb, (const float*)tree->d_int, keep, chunk_off, base, np, d.x, d.y, d.z, d.rgb, d.intensity);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (mem == PCV_MEM_HOST && (rc = planes_copy(ctx, out, d, np, hipMemcpyDeviceToHost))) return rc;
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

}  // namespace

// out[0 .. n] = exclusive u64 scan of in[0 .. n), out[n] the total (asynchronous on ctx->stream)
int pcv_batch_scan(pcv_ctx* ctx, PcvScratch& sc, const uint32_t* in, uint64_t n, uint64_t* out) {
  if (n <= kScanTile) {  // one tile: one launch
    hipLaunchKernelGGL(batch_scan_down_kernel, dim3(1), dim3(256), 0, ctx->stream, in, n, (const uint64_t*)nullptr, out);
    PCV_HIP_CHECK(ctx, hipGetLastError());
    return PCV_OK;
  }
  const uint64_t ntiles = (n + kScanTile - 1) / kScanTile;
  uint64_t* sums;
  int rc;
  if ((rc = sc.get(&sums, ntiles))) return rc;
  hipLaunchKernelGGL(batch_scan_reduce_kernel, dim3((uint32_t)ntiles), dim3(256), 0, ctx->stream, in, n, sums);
  hipLaunchKernelGGL(batch_scan_tiles_kernel, dim3(1), dim3(1024), 0, ctx->stream, sums, ntiles, out + n);
  hipLaunchKernelGGL(batch_scan_down_kernel, dim3((uint32_t)ntiles), dim3(256), 0, ctx->stream, in, n, sums, out);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// K8 on a view whose positions and attribute are on the device: keep flags into `keep` (a host buffer if keep_host), the
// kept count into *kept
static int launch_cull_points(pcv_ctx* ctx, PcvScratch& sc, const pcv_shapes* shapes, uint32_t shape_index, const PointsView& v,
                              bool keep_host, uint8_t* keep, uint64_t* kept) {
  uint8_t* d_keep = keep;
  unsigned long long* d_cnt;
  int rc;
  if ((keep_host && (rc = sc.get(&d_keep, v.n))) || (rc = sc.get(&d_cnt, 1))) return rc;
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_cnt, 0, 8, ctx->stream));
  {
    PcvProf prof(ctx, PCV_K_CULL_POINTS);
    const uint32_t chunk = v.encoded ? chunk_points(enc_stride_host(v.enc)) : kGroup;
    const dim3 grid((unsigned)((v.n + 4ull * chunk - 1) / (4ull * chunk)));
#define PCV_CALL(K) hipLaunchKernelGGL(cull_points_kernel<K>, grid, dim3(256), 0, ctx->stream, shapes->dev + shape_index, v, chunk, d_keep, d_cnt)
    if (shapes->kinds[shape_index] == PCV_SHAPE_S2_CELL_UNION) {
      hipLaunchKernelGGL(cull_points_union_kernel, grid, dim3(256), 0, ctx->stream, shapes->dev + shape_index, v, chunk, d_keep, d_cnt);
    } else if (shapes->kinds[shape_index] == PCV_SHAPE_POLYGON) {
      hipLaunchKernelGGL(cull_points_polygon_kernel, grid, dim3(256), 0, ctx->stream, shapes->dev + shape_index, v, chunk, d_keep, d_cnt);
    } else {
      PCV_DISPATCH_KIND(shapes->kinds[shape_index], PCV_CALL)
    }
#undef PCV_CALL
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (keep_host) PCV_HIP_CHECK(ctx, hipMemcpyAsync(keep, d_keep, v.n, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  if (kept) *kept = ctx->mailbox[0];
  return PCV_OK;
}

// K8 on a view whose positions are on the device: the closed interval on `attr` (n floats in `attr_mem`), the flags into
// `keep` (a host buffer if keep_host)
static int run_cull_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, PointsView v, const float* attr,
                           const double* interval, int attr_mem, bool keep_host, uint8_t* keep, uint64_t* kept) {
  if (!shapes || shape_index >= shapes->count || !keep) return ctx->fail(PCV_E_INVALID, "bad shape / null output");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  int rc;
  if (kept) *kept = 0;
  if (v.n == 0) return PCV_OK;
  if (interval) {
    if (!attr) return ctx->fail(PCV_E_INVALID, "interval without attribute");
    v.has_interval = 1;
    v.lo = interval[0];
    v.hi = interval[1];
    if (attr_mem == PCV_MEM_HOST) {
      float* da;
      if ((rc = sc.get(&da, v.n))) return rc;
      PCV_HIP_CHECK(ctx, hipMemcpyAsync(da, attr, v.n * 4, hipMemcpyHostToDevice, ctx->stream));
      v.attr = da;
    } else {
      v.attr = attr;
    }
  }
  return launch_cull_points(ctx, sc, shapes, shape_index, v, keep_host, keep, kept);
}

extern "C" int pcv_cull_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_points* points,
                               const double* interval, uint8_t* keep, uint64_t* kept) {
  if (!ctx) return PCV_E_INVALID;
  if (!points) return ctx->fail(PCV_E_INVALID, "points is null");
  if (points->n > 0 && (!points->x || !points->y || !points->z)) return ctx->fail(PCV_E_INVALID, "x/y/z must be non-null");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  const PointPlanes in{const_cast<double*>(points->x), const_cast<double*>(points->y), const_cast<double*>(points->z)};
  PointPlanes d = in;
  int rc;
  if (points->mem == PCV_MEM_HOST && points->n &&
      ((rc = planes_alloc(sc, points->n, in, &d)) || (rc = planes_copy(ctx, d, in, points->n, hipMemcpyHostToDevice))))
    return rc;
  PointsView v{};
  v.n = points->n;
  v.x = d.x;
  v.y = d.y;
  v.z = d.z;
  return run_cull_points(ctx, shapes, shape_index, v, points->intensity, interval, points->mem, points->mem == PCV_MEM_HOST, keep, kept);
}

extern "C" int pcv_cull_node_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, pcv_octree* tree,
                                    uint64_t node, const double* interval, uint8_t* keep, uint64_t* kept) {
  if (!ctx) return PCV_E_INVALID;
  if (!tree || node >= tree->nodes.size()) return ctx->fail(PCV_E_INVALID, "bad node");
  int rc = pcv_octree_ensure_query(tree);
  if (rc) return rc;
  const pcv_node_info& n = tree->nodes[node];
  PointsView v{};
  v.n = (uint64_t)n.num_points;
  v.encoded = tree->d_xyz + n.xyz_offset;
  v.enc = n.encoding;
  for (int a = 0; a < 3; ++a) v.cube_min[a] = n.cube_min[a];
  v.cube_edge = n.cube_edge;
  const float* attr = tree->has_intensity ? reinterpret_cast<const float*>(tree->d_int) + n.point_offset : nullptr;
  if (interval && !attr) return ctx->fail(PCV_E_INVALID, "octree has no intensity attribute to filter on");
  if (kept) *kept = 0;
  if (v.n == 0) return PCV_OK;
  // keep is a HOST buffer here; the attribute already lives on the device
  return run_cull_points(ctx, shapes, shape_index, v, attr, interval, PCV_MEM_DEVICE, true, keep, kept);
}

extern "C" int pcv_transform_points(pcv_ctx* ctx, const double iso[7], const pcv_points* points, double* ox, double* oy,
                                    double* oz) {
  if (!ctx) return PCV_E_INVALID;
  if (!iso || !points || !ox || !oy || !oz) return ctx->fail(PCV_E_INVALID, "null argument");
  const uint64_t n = points->n;
  if (n == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  const PointPlanes in{const_cast<double*>(points->x), const_cast<double*>(points->y), const_cast<double*>(points->z)}, out{ox, oy, oz};
  PointPlanes di = in, d = out;
  int rc;
  if (points->mem == PCV_MEM_HOST && ((rc = planes_alloc(sc, n, in, &di)) || (rc = planes_alloc(sc, n, out, &d)) ||
                                      (rc = planes_copy(ctx, di, in, n, hipMemcpyHostToDevice))))
    return rc;
  {
    PcvProf prof(ctx, PCV_K_TRANSFORM_POINTS);
    hipLaunchKernelGGL(transform_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, di.x, di.y, di.z,
                       iso[0], iso[1], iso[2], iso[3], iso[4], iso[5], iso[6], d.x, d.y, d.z);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (points->mem == PCV_MEM_HOST && (rc = planes_copy(ctx, out, d, n, hipMemcpyDeviceToHost))) return rc;
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

// N3: nodes_in_location + per-point culling + stable compaction for one location in a handful of launches.
// only_node == nullptr: every node PointCloud::nodes_in_location reports for the shape; otherwise that one node
// (stream_points_for_query_in_node, src/iterator.rs:185-205: the node's points through the FilteredIterator)
static int query_points_impl(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, pcv_octree* tree,
                             const uint64_t* only_node, const double* interval, uint64_t capacity, int mem, double* x, double* y,
                             double* z, uint8_t* rgb, float* intensity, uint64_t* count) {
  if (!ctx) return PCV_E_INVALID;
  if (!shapes || shape_index >= shapes->count || !tree || !count) return ctx->fail(PCV_E_INVALID, "bad argument");
  if (capacity && (!x || !y || !z || !rgb)) return ctx->fail(PCV_E_INVALID, "null output");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  *count = 0;
  if (tree->nodes.empty()) return PCV_OK;
  if (interval && !tree->has_intensity) return ctx->fail(PCV_E_INVALID, "octree has no intensity attribute to filter on");
  int rc = pcv_octree_ensure_query(tree);
  if (rc) return rc;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  const uint32_t m = tree->query->m;
  std::vector<uint32_t> nodes;
  if (only_node) {
    if (*only_node >= tree->nodes.size()) return ctx->fail(PCV_E_INVALID, "bad node");
    nodes.push_back((uint32_t)*only_node);
  } else if (shapes->kinds[shape_index] == PCV_SHAPE_S2_CELL_UNION) {
    // 1. a cell union has no Relation: its own walk gives the list (pcv_union.hip)
    if ((rc = pcv_union_node_list(ctx, shapes, shape_index, tree, &nodes))) return rc;
  } else if (shapes->polygon_frame_of(shape_index) == 0) {
    // 1. nor has a polygon in the xy frame (pcv_polygon.hip); a web-mercator one is its bounding rectangle below
    if ((rc = pcv_polygon_node_list(ctx, shapes, shape_index, tree, &nodes))) return rc;
  } else {
    // 1. PointCloud::nodes_in_location for this one shape: the Relation of every node cube in one dense launch
    //    (same sat() as the traversal kernel), then the breadth-first walk of NodeIdsIterator on the host.
    uint8_t* d_rel;
    if ((rc = sc.get(&d_rel, m)) || (rc = pcv_launch_relation_row(ctx, shapes, shape_index, tree, d_rel))) return rc;
    std::vector<uint8_t> rel(m);
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(rel.data(), d_rel, m, hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    pcv_query_walk(rel.data(), tree->query->h_first_child.data(), tree->query->h_child_mask.data(), m, &nodes);
  }
  const uint32_t nn = (uint32_t)nodes.size();
  // 2. one segment per non-empty node, in traversal order, chunked as the batch chunks its segments (shape 0 of
  //    shapes->dev + shape_index). Small queries get their descriptors straight from the host.
  uint64_t total = 0;
  for (uint32_t k = 0; k < nn; ++k) total += (uint64_t)std::max<int64_t>(tree->nodes[nodes[k]].num_points, 0);
  if (total == 0) return PCV_OK;
  const uint32_t shift = chunk_shift(total);
  const int32_t kind = shapes->kinds[shape_index];
  std::vector<uint32_t> seg_node;
  std::vector<uint64_t> seg_chunk, seg_flags;
  uint64_t nchunks = 0, keep_total = 0;
  for (uint32_t k = 0; k < nn; ++k) {
    const BatchNode nd = batch_node(tree->nodes[nodes[k]]);
    if (nd.n == 0) continue;
    seg_node.push_back(nodes[k]);
    seg_chunk.push_back(nchunks);
    seg_flags.push_back(keep_total);
    const uint32_t per = chunk_points(enc_stride_host(nd.enc)) >> shift;
    nchunks += (nd.n + per - 1) / per;
    keep_total += (nd.n + 3ull) & ~3ull;
  }
  const uint64_t nseg = seg_node.size();
  const bool host_desc = nchunks <= 2048;
  // the one upload: the descriptors (at offset 0) or what query_chunks_kernel makes them from, and the interval
  std::vector<uint64_t> up;
  auto put = [&up](const void* p, size_t bytes) {
    const size_t at = up.size();
    up.resize(at + (bytes + 7) / 8);
    std::memcpy(up.data() + at, p, bytes);
    return at;
  };
  size_t at_first = 0, at_node = 0, at_chunk = 0, at_flags = 0;
  if (host_desc) {
    for (uint64_t s = 0; s < nseg; ++s) {
      const BatchNode nd = batch_node(tree->nodes[seg_node[s]]);
      const uint64_t end = s + 1 < nseg ? seg_chunk[s + 1] : nchunks;
      for (uint64_t c = seg_chunk[s]; c < end; ++c) {
        const ChunkDesc d = make_chunk_desc(nd, seg_chunk[s], seg_flags[s], 0, kind, c, shift);
        put(&d, sizeof(d));
      }
    }
  } else {
    const uint64_t shape_first[2] = {0, nseg};
    at_first = put(shape_first, sizeof(shape_first));
    at_chunk = put(seg_chunk.data(), 8 * nseg);
    at_flags = put(seg_flags.data(), 8 * nseg);
    at_node = put(seg_node.data(), 4 * nseg);
  }
  const BatchIval iv{interval ? interval[0] : 0.0, interval ? interval[1] : 0.0, interval ? 1u : 0u, 0u};
  const size_t at_iv = put(&iv, sizeof(iv));
  uint64_t* d_up;
  ChunkDesc* d_desc;
  uint8_t* d_keep;
  uint32_t* d_cc;
  uint64_t* d_off;
  if ((rc = sc.get(&d_up, up.size())) || (!host_desc && (rc = sc.get(&d_desc, nchunks))) || (rc = sc.get(&d_keep, keep_total)) ||
      (rc = sc.get(&d_cc, nchunks)) || (rc = sc.get(&d_off, nchunks + 1)))
    return rc;
  if (host_desc) d_desc = (ChunkDesc*)d_up;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_up, up.data(), 8 * up.size(), hipMemcpyHostToDevice, ctx->stream));
  {
    PcvProf prof(ctx, PCV_K_CULL_POINTS);
    if (!host_desc)
      hipLaunchKernelGGL(query_chunks_kernel, dim3(stride_grid(nchunks, 256)), dim3(256), 0, ctx->stream, d_up + at_first, 1u,
                         shapes->dev + shape_index, (const uint32_t*)(d_up + at_node), d_up + at_chunk, d_up + at_flags, nseg,
                         tree->query->nodes, nchunks, shift, d_desc);
    if ((rc = launch_query_flags(ctx, kind, shapes->dev + shape_index, (const BatchIval*)(d_up + at_iv), d_desc, (uint32_t)nchunks, tree,
                                 d_keep, d_cc)))
      return rc;
  }
  if ((rc = pcv_batch_scan(ctx, sc, d_cc, nchunks, d_off))) return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_off + nchunks, 8, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // also keeps `up` alive until the copy is done
  const uint64_t kept = ctx->mailbox[0];
  *count = kept;
  const uint64_t nout = kept < capacity ? kept : capacity;
  if (nout && (rc = compact_chunks(ctx, PCV_K_QUERY_COMPACT, tree, d_desc, d_keep, d_off, 0, nchunks, 0, nout, mem, x, y, z, rgb,
                                   intensity)))
    return rc;
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_query_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, pcv_octree* tree,
                                const double* interval, uint64_t capacity, int mem, double* x, double* y, double* z,
                                uint8_t* rgb, float* intensity, uint64_t* count) {
  return query_points_impl(ctx, shapes, shape_index, tree, nullptr, interval, capacity, mem, x, y, z, rgb, intensity, count);
}
extern "C" int pcv_query_node_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, pcv_octree* tree,
                                     uint64_t node, const double* interval, uint64_t capacity, int mem, double* x, double* y,
                                     double* z, uint8_t* rgb, float* intensity, uint64_t* count) {
  return query_points_impl(ctx, shapes, shape_index, tree, &node, interval, capacity, mem, x, y, z, rgb, intensity, count);
}

// N4: the /nodes_data reply blob of octree_web_viewer (octree_web_viewer/src/backend.rs:90-177): per node
// min xyz (3 x f64 LE), edge (f64), num_points (u32), bytes per coordinate (u8), pad to 8, raw .xyz, pad to 8,
// raw .rgb, pad to 8. Returns the blob size in *needed; writes it when it fits in `capacity`.
extern "C" int pcv_octree_nodes_blob(pcv_octree* t, const uint64_t* node_indices, uint64_t count, uint8_t* out,
                                     uint64_t capacity, uint64_t* needed) {
  if (!t || !needed || (count && !node_indices)) return PCV_E_INVALID;
  auto pad8 = [](uint64_t v) { return (v + 7) & ~7ull; };
  uint64_t size = 0;
  for (uint64_t k = 0; k < count; ++k) {
    if (node_indices[k] >= t->nodes.size()) return t->ctx->fail(PCV_E_NOT_FOUND, "Could not get node.");
    const pcv_node_info& nd = t->nodes[node_indices[k]];
    const uint64_t np = (uint64_t)nd.num_points;
    size += pad8(32 + 4 + 1) + pad8(np * 3 * (uint64_t)pcv_bytes_per_coordinate(nd.encoding)) + pad8(np * 3);
  }
  *needed = size;
  if (!out || capacity < size) return PCV_OK;
  uint8_t* w = out;
  for (uint64_t k = 0; k < count; ++k) {
    const pcv_node_info& nd = t->nodes[node_indices[k]];
    const uint8_t *xyz, *rgbp;
    uint64_t lx, lr;
    int rc = pcv_octree_node_data(t, node_indices[k], 0, &xyz, &lx);
    if (rc) return rc;
    if ((rc = pcv_octree_node_data(t, node_indices[k], 1, &rgbp, &lr))) return rc;
    uint8_t* start = w;
    std::memcpy(w, nd.cube_min, 24);
    std::memcpy(w + 24, &nd.cube_edge, 8);
    const uint32_t np32 = (uint32_t)nd.num_points;
    std::memcpy(w + 32, &np32, 4);
    w[36] = (uint8_t)pcv_bytes_per_coordinate(nd.encoding);
    w += 37;
    while ((uint64_t)(w - start) % 8) *w++ = 0;
    std::memcpy(w, xyz, lx);
    w += lx;
    while ((uint64_t)(w - out) % 8) *w++ = 0;
    std::memcpy(w, rgbp, lr);
    w += lr;
    while ((uint64_t)(w - out) % 8) *w++ = 0;
  }
  return PCV_OK;
}

// ---------------------------------------------------------------------------------------------
// N3b: one point query over many locations (pcv_query_batch_*)
// ---------------------------------------------------------------------------------------------
// One run culls the points of S locations over one octree and keeps the result on the device as a segment table: one
// segment per (shape, node PointCloud::nodes_in_location reports for it), shape-major, in traversal order, with u64 point
// offsets. The host reads back three sets of totals; it walks no tree and synchronises once per run stage, not per shape.
//   nodes    cull_nodes_tree_kernel<false, true> (+ nodes_in_location_kernel for the shapes it hands back) twice: counts, a
//            u64 scan into the rows of the segment table, then the lists straight into their rows — nothing grows as S x m
//   sizes    per segment its padded flag count and its chunk count at each of the three chunk sizes; u64 scans
//   chunks   one 64-byte descriptor per chunk (a chunk never spans two nodes); `enc` carries the kind and the shape index
//   flags    the persistent staged decode of query_flags_kernel over the chunks of every shape; the shape's ContainParams
//            and interval are scalar loads per chunk, the kind a wave-uniform switch
//   scan     kept points per chunk -> u64 offsets; a segment starts at its first chunk's offset (an empty one at its
//            successor's)
//   compact  lazily, for a range of segments, into the caller's buffers (pcv_query_batch_points)
namespace {

// per segment: flags (padded to 4, so that every segment's flags start on a dword) and chunks at shift 0, 1, 2
__global__ __launch_bounds__(256) void batch_seg_sizes_kernel(const uint32_t* __restrict__ seg_node, uint64_t nseg,
                                                               const BatchNode* __restrict__ nodes, uint32_t* __restrict__ flags,
                                                               uint32_t* __restrict__ chunks /* 3 x nseg */) {
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < nseg; k += (uint64_t)gridDim.x * 256) {
    const BatchNode* nd = nodes + seg_node[k];
    const uint32_t n = nd->n, per = kGroup * (24u / enc_stride(nd->enc));
    flags[k] = (n + 3u) & ~3u;
#pragma unroll
    for (uint32_t s = 0; s < 3; ++s) chunks[s * nseg + k] = (n + (per >> s) - 1u) / (per >> s);
  }
}

__global__ __launch_bounds__(256) void batch_seg_offsets_kernel(const uint64_t* __restrict__ seg_chunk, uint64_t nseg,
                                                                 const uint64_t* __restrict__ chunk_off, uint64_t* __restrict__ seg_off) {
  for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k <= nseg; k += (uint64_t)gridDim.x * 256) seg_off[k] = chunk_off[seg_chunk[k]];
}

}  // namespace

extern "C" void pcv_query_batch_free(pcv_query_batch* b) {
  if (!b) return;
  b->ctx->dev_free(b->d_seg_node);
  b->ctx->dev_free(b->d_desc);
  b->ctx->dev_free(b->d_keep);
  b->ctx->dev_free(b->d_chunk_off);
  delete b;
}

static int query_batch_run(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, const double* intervals,
                           const uint8_t* interval_used, pcv_query_batch* b) {
  const uint32_t S = shapes->count;
  b->shape_first.assign((size_t)S + 1, 0);
  b->seg_chunk.assign(1, 0);
  b->seg_off.assign(1, 0);
  if (S == 0 || tree->nodes.empty()) return PCV_OK;
  int rc = pcv_octree_ensure_query(tree);
  if (rc) return rc;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  const uint32_t m = tree->query->m;
  const PcvOctreeQuery* q = tree->query;
  // intervals go up first: the first read-back below also keeps this host vector alive
  std::vector<BatchIval> h_iv(S);
  for (uint32_t s = 0; s < S; ++s) {
    const bool used = intervals && (!interval_used || interval_used[s]);
    h_iv[s] = BatchIval{used ? intervals[2 * (size_t)s] : 0.0, used ? intervals[2 * (size_t)s + 1] : 0.0, used ? 1u : 0u, 0u};
  }
  BatchIval* d_iv;
  uint32_t *d_cnt, *d_lists;
  uint64_t* d_shape_first;
  if ((rc = sc.get(&d_iv, S)) || (rc = sc.get(&d_cnt, S)) || (rc = sc.get(&d_lists, pcv_node_lists_scratch(S, m))) ||
      (rc = sc.get(&d_shape_first, (size_t)S + 1)))
    return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_iv, h_iv.data(), sizeof(BatchIval) * S, hipMemcpyHostToDevice, ctx->stream));
  // 1. node lists: counts, rows, lists
  auto node_lists = [&](uint32_t* out, const uint64_t* rows) {
    return pcv_launch_node_lists(ctx, PCV_K_QUERY_BATCH_NODES, false, shapes, tree, 0, d_cnt, out, d_lists, rows);
  };
  auto scan = [&](const uint32_t* in, uint64_t n, uint64_t* out) {
    PcvProf prof(ctx, PCV_K_QUERY_BATCH_SCAN);
    return pcv_batch_scan(ctx, sc, in, n, out);
  };
  if ((rc = node_lists(nullptr, nullptr)) || (rc = scan(d_cnt, S, d_shape_first))) return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(b->shape_first.data(), d_shape_first, 8 * ((size_t)S + 1), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // read-back 1: the segment count
  const uint64_t nseg = b->shape_first[S];
  b->nseg = nseg;
  if (nseg == 0) return PCV_OK;
  if ((rc = ctx->dev_alloc((void**)&b->d_seg_node, 4 * nseg))) return rc;
  if ((rc = node_lists(b->d_seg_node, d_shape_first))) return rc;
  // 2. segment sizes: flags (padded) and chunks at shift 0, 1, 2; the shift is chosen from the total below, as
  //    query_points_impl chooses it
  uint32_t *d_seg_flags32, *d_seg_chunks32;
  uint64_t *d_seg_flags, *d_seg_chunk;
  if ((rc = sc.get(&d_seg_flags32, nseg)) || (rc = sc.get(&d_seg_chunks32, 3 * nseg)) || (rc = sc.get(&d_seg_flags, nseg + 1)) ||
      (rc = sc.get(&d_seg_chunk, 3 * (nseg + 1))))
    return rc;
  {
    PcvProf prof(ctx, PCV_K_QUERY_BATCH_CHUNKS);
    hipLaunchKernelGGL(batch_seg_sizes_kernel, dim3(stride_grid(nseg, 256)), dim3(256), 0, ctx->stream, b->d_seg_node, nseg, q->nodes,
                       d_seg_flags32, d_seg_chunks32);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = scan(d_seg_flags32, nseg, d_seg_flags))) return rc;
  for (int s = 0; s < 3; ++s)
    if ((rc = scan(d_seg_chunks32 + s * nseg, nseg, d_seg_chunk + s * (nseg + 1)))) return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_seg_flags + nseg, 8, hipMemcpyDeviceToHost, ctx->stream));
  for (int s = 0; s < 3; ++s)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox + 1 + s, d_seg_chunk + s * (nseg + 1) + nseg, 8, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // read-back 2: flags and chunks
  const uint64_t nflags = ctx->mailbox[0];
  const uint32_t shift = chunk_shift(nflags);
  const uint64_t nchunks = ctx->mailbox[1 + shift];
  if (nchunks >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "query batch: more than 2^32 - 2 chunks");
  const uint64_t* d_chunk_first = d_seg_chunk + shift * (nseg + 1);
  b->seg_chunk.resize(nseg + 1);
  b->seg_off.assign(nseg + 1, 0);
  b->nchunks = nchunks;
  if ((rc = ctx->dev_alloc(&b->d_desc, sizeof(ChunkDesc) * nchunks)) || (rc = ctx->dev_alloc((void**)&b->d_keep, nflags)) ||
      (rc = ctx->dev_alloc((void**)&b->d_chunk_off, 8 * (nchunks + 1))))
    return rc;
  uint32_t* d_cc;
  uint64_t* d_seg_off;
  if ((rc = sc.get(&d_cc, nchunks)) || (rc = sc.get(&d_seg_off, nseg + 1))) return rc;
  ChunkDesc* desc = (ChunkDesc*)b->d_desc;
  if (nchunks) {
    {
      PcvProf prof(ctx, PCV_K_QUERY_BATCH_CHUNKS);
      hipLaunchKernelGGL(query_chunks_kernel, dim3(stride_grid(nchunks, 256)), dim3(256), 0, ctx->stream, d_shape_first, S, shapes->dev,
                         b->d_seg_node, d_chunk_first, d_seg_flags, nseg, q->nodes, nchunks, shift, desc);
    }
    // 3. keep flags
    PcvProf prof(ctx, PCV_K_QUERY_BATCH_FLAGS);
    if ((rc = launch_query_flags(ctx, -1, shapes->dev, d_iv, desc, (uint32_t)nchunks, tree, b->d_keep, d_cc))) return rc;
    if (std::find(shapes->kinds.begin(), shapes->kinds.end(), (int32_t)PCV_SHAPE_WEB_MERCATOR_RECT) != shapes->kinds.end() &&
        (rc = launch_flags(ctx, query_flags_wmr_kernel, shapes->dev, d_iv, desc, (uint32_t)nchunks, tree, b->d_keep, d_cc)))
      return rc;
    if (!shapes->union_shapes.empty() &&
        (rc = launch_flags(ctx, query_flags_union_kernel, shapes->dev, d_iv, desc, (uint32_t)nchunks, tree, b->d_keep, d_cc)))
      return rc;
    if (!shapes->polygon_shapes.empty() &&
        (rc = launch_flags(ctx, query_flags_polygon_kernel, shapes->dev, d_iv, desc, (uint32_t)nchunks, tree, b->d_keep, d_cc)))
      return rc;
  }
  // 4. kept points per chunk -> u64 offsets; segment offsets from the first chunk of each segment
  if ((rc = scan(d_cc, nchunks, b->d_chunk_off))) return rc;
  {
    PcvProf prof(ctx, PCV_K_QUERY_BATCH_SCAN);
    hipLaunchKernelGGL(batch_seg_offsets_kernel, dim3(stride_grid(nseg + 1, 256)), dim3(256), 0, ctx->stream, d_chunk_first, nseg,
                       (const uint64_t*)b->d_chunk_off, d_seg_off);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(b->seg_chunk.data(), d_chunk_first, 8 * (nseg + 1), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(b->seg_off.data(), d_seg_off, 8 * (nseg + 1), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // read-back 3: the offsets
  b->npoints = b->seg_off[nseg];
  return PCV_OK;
}

extern "C" int pcv_query_batch_run(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, const double* intervals,
                                   const uint8_t* interval_used, pcv_query_batch** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!shapes || !tree || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (shapes->count >= (1u << kBatchShapeBits)) return ctx->fail(PCV_E_INVALID, "query batch: at most 2^24 - 1 shapes");
  bool any_interval = false;
  for (uint32_t s = 0; intervals && s < shapes->count; ++s) any_interval = any_interval || !interval_used || interval_used[s];
  if (any_interval && !tree->has_intensity) return ctx->fail(PCV_E_INVALID, "octree has no intensity attribute to filter on");
  pcv_query_batch* b = new pcv_query_batch();
  b->ctx = ctx;
  b->tree = tree;
  b->has_intensity = tree->has_intensity;
  b->nshapes = shapes->count;
  const int rc = query_batch_run(ctx, shapes, tree, intervals, interval_used, b);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing queued may still write into what is freed here
    (void)hipGetLastError();
    pcv_query_batch_free(b);
    return rc;
  }
  ctx->prof_resolve();
  *out = b;
  return PCV_OK;
}

extern "C" int pcv_query_batch_sizes(const pcv_query_batch* b, uint64_t* num_segments, uint64_t* num_points) {
  if (!b) return PCV_E_INVALID;
  if (num_segments) *num_segments = b->nseg;
  if (num_points) *num_points = b->npoints;
  return PCV_OK;
}

extern "C" int pcv_query_batch_segments(const pcv_query_batch* b, uint64_t* shape_first_segment, uint32_t* segment_node,
                                        uint64_t* segment_offset) {
  if (!b) return PCV_E_INVALID;
  pcv_ctx* ctx = b->ctx;
  if (shape_first_segment) std::memcpy(shape_first_segment, b->shape_first.data(), 8 * b->shape_first.size());
  if (segment_offset) std::memcpy(segment_offset, b->seg_off.data(), 8 * b->seg_off.size());
  if (segment_node && b->nseg) {
    PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(segment_node, b->d_seg_node, 4 * b->nseg, hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return PCV_OK;
}

extern "C" int pcv_query_batch_points(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, uint64_t capacity, int mem,
                                      double* x, double* y, double* z, uint8_t* rgb, float* intensity) {
  if (!b) return PCV_E_INVALID;
  pcv_ctx* ctx = b->ctx;
  if (first_segment > b->nseg || num_segments > b->nseg - first_segment) return ctx->fail(PCV_E_INVALID, "segment range past the end");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  const uint64_t p0 = b->seg_off[first_segment], np = b->seg_off[first_segment + num_segments] - p0;
  if (np > capacity) return ctx->fail(PCV_E_INVALID, "segment range holds more points than capacity");
  if (np == 0) return PCV_OK;
  if (!x || !y || !z || !rgb) return ctx->fail(PCV_E_INVALID, "null output");
  const uint64_t c0 = b->seg_chunk[first_segment], c1 = b->seg_chunk[first_segment + num_segments];
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const int rc = compact_chunks(ctx, PCV_K_QUERY_BATCH_COMPACT, b->tree, (const ChunkDesc*)b->d_desc, b->d_keep,
                                (const uint64_t*)b->d_chunk_off, c0, c1, p0, np, mem, x, y, z, rgb, intensity);
  if (rc) return rc;
  ctx->prof_resolve();
  return PCV_OK;
}
