// pcv_xray.hip — xray's build_xray_quadtree (xray/src/generation.rs:557-616) on the device, the leaf level: rasterised
// straight from batched point queries, one per cloud of the run — octrees (pcv_query.hip) or S2 cell clouds
// (pcv_s2_points.hip, as pcv_s2_query_dev.h states its result) — without materialising their points. The parent levels
// and the merge are pcv_xray_pyramid.hip, node images and the quadtree directory pcv_xray_files.hip; the handle they
// share (pcv_xray_obj.h) is made, listed and freed here.
//
//   host   leaf geometry   get_bounding_box :550 (Aabb::transform, src/geometry/aabb.rs:58-66),
//                          find_quadtree_bounding_rect_and_levels :515, Node::from_node_id_and_root_bounding_rect and
//                          Node::get_child (quadtree/src/lib.rs:59-97), get_nodes_at_level :534 (DFS pop order)
//   host   one query per leaf tile   xray_from_points :464 — Aabb(tile) or Obb::from(tile).transformed(global_from_query)
//                          (src/geometry/obb.rs:20-47), intensity interval on every shape, through pcv_query_batch_run
//   K_xb   xray_bin        per kept point: decode (the batch's own decode; an S2 candidate: its stored f64),
//                          query_from_global (:493-497), discretise (:119-123); count per (tile, 32 x 32 pixel block), aggregated per wave before the atomic
//   scan   bucket counts -> u64 offsets (pcv_batch_scan)
//   K_xs   xray_scatter    the same walk again, writing one 8-byte record per drawable point into its bucket (+ z as f64
//                          for height_stddev, + the bin as i64 with binning: from the intensity, or over S2 clouds from any
//                          scalar column of the cloud, pcv_xray_run_s2_ex, in an instance of its own)
//   K_xa   xray_accum      one workgroup per bucket: per-pixel state in LDS (run-aggregated atomics), then the strategy's
//                          colour (:159-199, :294-345, :365-408, colormap.rs, src/color.rs:29-36), the background of
//                          assign_background_color (:684) and the block's RGBA rows
//   K_xo   xray_sorted     instead of K_xa for colored_with_intensity and binned colored: the bucket sorted by (pixel, bin,
//                          record) in LDS or, above the LDS limit, in place in the workspace; then per pixel the bin means
//                          in ascending bin order (:138-157, :210-292, :294-362)
//
// Tiles are processed in groups so that the records of a group fit `max_workspace_bytes`. xray and colored are
// order-independent (a set union, integer sums), and xray_sorted reduces in key order, so their bytes do not depend on
// grouping, scheduling or which octree of a several-octree run (PointCloudClient, point_cloud_client/src/lib.rs:102-125)
// a point came from.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "pcv_query_dev.h"
#include "pcv_s2_attr_dev.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_query_dev.h"
#include "pcv_switches.h"
#include "pcv_xray_obj.h"

namespace {

constexpr uint32_t kBlkPx = kBlk * kBlk;
constexpr uint32_t kZWords = 33;  // 1 056 bits per pixel: z buckets 0 ..= 1024 (NUM_Z_BUCKETS = 1024, :31)
constexpr uint32_t kZMax = kZWords * 32 - 1;
constexpr uint64_t kDefaultWorkspace = 2ull << 30;
constexpr uint64_t kMaxGroupBuckets = 1ull << 30;  // (tiles of a group) x blocks per tile: u32 bucket indices

// ---- finalisation: the same code on the host (pcv_xray_finalize, tests) and in xray_accum -----------------------------
struct Rgba8 {
  uint8_t r, g, b, a;
};
// Rust `f32 as u8`: truncation, saturating; NaN -> 0
__host__ __device__ inline uint8_t sat_u8(float v) {
  if (!(v > 0.0f)) return 0;
  if (v >= 255.0f) return 255;
  return (uint8_t)v;
}
// Color<f32>::to_u8 (src/color.rs:29-36)
__host__ __device__ inline Rgba8 to_u8(float r, float g, float b, float a) {
  return {sat_u8(r * 255.0f), sat_u8(g * 255.0f), sat_u8(b * 255.0f), sat_u8(a * 255.0f)};
}
// Jet (xray/src/colormap.rs:17-60), f32 throughout
__host__ __device__ inline float jet_base(float val) {
  auto interp = [](float v, float y0, float x0, float y1, float x1) { return (v - x0) * (y1 - y0) / (x1 - x0) + y0; };
  if (val <= -0.75f) return 0.0f;
  if (val <= -0.25f) return interp(val, 0.0f, -0.75f, 1.0f, -0.25f);
  if (val <= 0.25f) return 1.0f;
  if (val <= 0.75f) return interp(val, 1.0f, 0.25f, 0.0f, 0.75f);
  return 0.0f;
}
__host__ __device__ inline Rgba8 jet(float val) { return to_u8(jet_base(val - 0.5f), jet_base(val), jet_base(val + 0.5f), 1.0f); }
// Monochrome(PURPLISH) (colormap.rs:62-84): from (0.8, 0.8, 1.0) to black
__host__ __device__ inline Rgba8 purplish(float val) {
  return to_u8((1.0f - val) * 0.8f, (1.0f - val) * 0.8f, (1.0f - val) * 1.0f, 1.0f);
}
// PointColorColoringStrategy::get_pixel_color without binning (:294-345): the reference adds c / 255 in f32 in arrival
// order and divides by the count; here the channel sums are exact integers and the mean is rounded once to f32. Alpha is
// a sum of n ones in f32, which stops growing at 2^24, divided by `n as f32`.
__host__ __device__ inline Rgba8 colored(uint64_t sr, uint64_t sg, uint64_t sb, uint64_t n) {
  const double dn = 255.0 * (double)n;
  const float asum = (float)(n < (1ull << 24) ? n : (1ull << 24));
  return to_u8((float)((double)sr / dn), (float)((double)sg / dn), (float)((double)sb / dn), asum / (float)n);
}
// HeightStddevColoringStrategy::get_pixel_color (:399-405): clamp(stddev as f32, 0, max) / max, then the colormap
__host__ __device__ inline Rgba8 height_stddev(double stddev, float max_stddev, uint32_t colormap) {
  float s = (float)stddev;
  s = s < 0.0f ? 0.0f : (s > max_stddev ? max_stddev : s);
  const float v = s / max_stddev;
  return colormap == PCV_XRAY_PURPLISH ? purplish(v) : jet(v);
}
// XRayColoringStrategy (:182-197): value = ((1 - ln(n) / ln(1024)) * 255) as u8 for n distinct z buckets, with the host
// libm's log (what f64::ln calls); entry 0 is never read (a pixel without points is TRANSPARENT)
void xray_value_table(uint8_t table[kZWords * 32 + 1]) {
  const double max_saturation = std::log(1024.0);
  table[0] = 255;
  for (uint32_t n = 1; n <= kZWords * 32; ++n) {
    const double v = (1.0 - std::log((double)n) / max_saturation) * 255.0;
    table[n] = !(v > 0.0) ? 0 : v >= 255.0 ? 255 : (uint8_t)v;
  }
}
__host__ __device__ inline uint32_t pack(Rgba8 c) { return (uint32_t)c.r | (uint32_t)c.g << 8 | (uint32_t)c.b << 16 | (uint32_t)c.a << 24; }
// assign_background_color (:684-708): alpha < 128 -> the background colour
__host__ __device__ inline uint32_t with_background(Rgba8 c, uint32_t bg) { return c.a < 128 ? bg : pack(c); }

// f32 ln shared by the kernel and pcv_xray_finalize: x = m 2^e with m in [sqrt(1/2), sqrt(2)), ln m = 2 atanh(s) with
// s = (m - 1) / (m + 1) as an odd series to s^17 in f64, e ln 2 + ln m rounded to f32 once. Plain f64 arithmetic (no libm,
// no contraction), so host and device agree bit for bit; within an ulp of libm's logf. ln 1 = 0 exactly.
__host__ __device__ inline float ln_f32(float x) {
  if (x != x) return x;
  if (x < 0.0f) return __builtin_nanf("");
  if (x == 0.0f) return -__builtin_inff();
  if (x == __builtin_inff()) return x;
  double m = (double)x;
  uint64_t bits;
  memcpy(&bits, &m, 8);
  int e = (int)((bits >> 52) & 0x7ffu) - 1023;
  bits = (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  memcpy(&m, &bits, 8);
  if (m > 1.4142135623730951) {
    m = m * 0.5;
    e = e + 1;
  }
  const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
  const double poly =
      s2 * (1.0 / 3.0 + s2 * (1.0 / 5.0 + s2 * (1.0 / 7.0 + s2 * (1.0 / 9.0 + s2 * (1.0 / 11.0 + s2 * (1.0 / 13.0 + s2 * (1.0 / 15.0 + s2 * (1.0 / 17.0))))))));
  const double lnm = 2.0 * s + 2.0 * s * poly;
  return (float)((double)e * 0.6931471805599453 + lnm);
}
// Rust's f32::max / f32::min: a NaN operand yields the other one
__host__ __device__ inline float rust_max(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
__host__ __device__ inline float rust_min(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }
// IntensityColoringStrategy::get_pixel_color after the mean (:270-284)
__host__ __device__ inline Rgba8 intensity_color(float mean, float lo, float hi) {
  const float m = rust_min(rust_max(mean, lo), hi);
  const float b = ln_f32(m - lo) / ln_f32(hi - lo);
  return to_u8(b, b, b, 1.0f);
}
using s2attr::rust_i64;  // Rust `f64 as i64`, the bin of generation.rs:150: stated once, in pcv_s2_attr_dev.h

// Rust `f64 as u32`: truncation, saturating; NaN -> 0
__device__ __forceinline__ uint32_t sat_u32(double v) {
  if (!(v > 0.0)) return 0;
  if (v >= 4294967295.0) return 0xffffffffu;
  return (uint32_t)v;
}

// ---- device passes --------------------------------------------------------------------------------------------------
struct XrayTileDev {  // discretisation frame of one created tile: its bbox min and diag (:119-123)
  double min[3];
  double diag[3];
};
// The device reads the pointers of XrayTreeChunks as global ones: a pointer read from memory is otherwise generic, every
// access through it a flat one and the chunk descriptor a vector load
#if defined(__HIP_DEVICE_COMPILE__)
#define PCV_GLOBAL __attribute__((address_space(1)))
#else
#define PCV_GLOBAL
#endif
// one octree's share of a tile group: its query batch's chunks [c0, c0 + n) for the group's shapes sit at [first,
// first + n) of the group's chunk list, and n is the next entry's first minus this one's (the last: nchunks)
struct XrayTreeChunks {
  const PCV_GLOBAL ChunkDesc* desc;
  const PCV_GLOBAL uint8_t* keep;
  const PCV_GLOBAL uint8_t* xyz;
  const PCV_GLOBAL uint8_t* rgb;
  const PCV_GLOBAL uint8_t* inten;  // f32 per point; set only when the strategy or the binning reads intensity
  uint64_t c0;
  uint64_t first;
};
// the bin column of an S2 cloud, parallel to XrayBinArgs::trees (pcv_xray_run_s2_ex, binning on any scalar attribute): the
// cloud's cell-contiguous column and its data type (s2attr, pcv_s2_attr_dev.h). Each cloud converts with its own type.
struct XrayBinColumn {
  const PCV_GLOBAL uint8_t* col;
  int32_t data_type;
  uint32_t pad;
};
struct XrayBinArgs {
  const XrayTreeChunks* trees;      // the group's octrees with at least one chunk, in list order
  uint32_t ntrees;
  uint64_t nchunks;                 // chunks of the group over all its octrees
  const int32_t* created_of_shape;  // created-tile index of each shape, -1 where no octree's query kept anything
  const XrayTileDev* tiles;         // by created index
  uint32_t created0;                // the group's first created tile
  uint32_t W, nbx, nblocks;         // tile edge in pixels, blocks per row, blocks per tile
  uint32_t strategy;
  int32_t has_iso;
  double iso[7];                    // query_from_global: translation xyz, quaternion ijkw
  int32_t binned;                   // colored / colored_with_intensity with binning (on intensity unless `columns` is set)
  double bin_size;
  unsigned long long* negative;     // colored_with_intensity: kept points with intensity < 0 per created tile (count pass)
  const XrayBinColumn* columns;     // S2, binning on a column: one entry per entry of `trees`; read by the COLUMN instance only
};

// per 64 points of a chunk: is the point drawn, its bucket (tile in group x block), its record, (stddev) its z, (binning)
// its bin and (colored_with_intensity) whether its intensity is < 0
struct XrayPoint {
  bool draw, neg;
  uint32_t bucket;
  uint64_t rec;  // low 32 bits: pixel in block | z << 10; high 32: r | g << 8 | b << 16, or the intensity's f32 bits
  double z;
  int64_t bin;
};
// Where a chunk's points come from. An octree batch's chunk: a node's encoded bytes, decoded by the batch's own decode, u8
// keep flags, attributes at attr_index. An S2 query's chunk: up to 1 024 candidates of one cell, the stored f64 positions
// untouched (24-byte AoS: a wave's 64 points are one contiguous 1 536-byte run), u32 keep flags, colour and intensity at
// the same point index.
struct XrayNodeSource {
  static constexpr bool kBinColumn = false;
  const uint8_t* rgb;
  const float* inten;
  const ChunkDesc& d;
  const PointsView& v;
  const PCV_GLOBAL uint8_t* kp;
  __device__ __forceinline__ bool kept(uint32_t q) const { return kp[q]; }
  __device__ __forceinline__ bool has_intensity() const { return inten != nullptr; }
  __device__ __forceinline__ float intensity(uint32_t q) const { return inten[d.attr_index + q]; }
  __device__ __forceinline__ V3d position(uint32_t q) const { return load_point(v, q); }
  __device__ __forceinline__ const uint8_t* color(uint32_t q) const { return rgb + 3 * (d.attr_index + q); }
};
struct XrayS2Source {
  static constexpr bool kBinColumn = false;
  const PCV_GLOBAL double* xyz;   // the chunk's first point
  const PCV_GLOBAL uint8_t* rgb;
  const PCV_GLOBAL float* inten;  // null unless the strategy or the binning reads intensity
  const PCV_GLOBAL uint32_t* kp;
  __device__ __forceinline__ bool kept(uint32_t q) const { return kp[q] != 0u; }
  __device__ __forceinline__ bool has_intensity() const { return inten != nullptr; }
  __device__ __forceinline__ float intensity(uint32_t q) const { return inten[q]; }
  __device__ __forceinline__ V3d position(uint32_t q) const { return {xyz[3 * q], xyz[3 * q + 1], xyz[3 * q + 2]}; }
  __device__ __forceinline__ const PCV_GLOBAL uint8_t* color(uint32_t q) const { return rgb + 3 * q; }
};
// An S2 chunk whose bins come from a column of the cloud: a wave's 64 candidates are consecutive elements of one cell's
// column, one contiguous run of 64, 128, 256 or 512 bytes a step. The data type is the cloud's, so the switch is
// wave-uniform (a scalar branch): one instance for all ten types, not one per type.
struct XrayS2ColumnSource : XrayS2Source {
  static constexpr bool kBinColumn = true;
  const PCV_GLOBAL uint8_t* col;  // the chunk's first element
  int32_t data_type;
  template <typename T>
  __device__ __forceinline__ int64_t bin_as(uint32_t q, double size) const {
    return s2attr::bin<T>(((const PCV_GLOBAL T*)col)[q], size);
  }
  __device__ __forceinline__ int64_t bin(uint32_t q, double size) const {
    switch (data_type) {
      case s2attr::U8: return bin_as<uint8_t>(q, size);
      case s2attr::U16: return bin_as<uint16_t>(q, size);
      case s2attr::U32: return bin_as<uint32_t>(q, size);
      case s2attr::U64: return bin_as<uint64_t>(q, size);
      case s2attr::I8: return bin_as<int8_t>(q, size);
      case s2attr::I16: return bin_as<int16_t>(q, size);
      case s2attr::I32: return bin_as<int32_t>(q, size);
      case s2attr::I64: return bin_as<int64_t>(q, size);
      case s2attr::F32: return bin_as<float>(q, size);
      default: return bin_as<double>(q, size);  // F64: the host admits scalar types only
    }
  }
};
template <class Source>
__device__ __forceinline__ XrayPoint xray_point(const XrayBinArgs& a, const Source& src, const XrayTileDev& t, uint32_t bbase, uint32_t q,
                                                bool kept) {
  XrayPoint o{false, false, 0u, 0ull, 0.0, 0};
  if (!kept) return o;
  float in = 0.0f;
  if (src.has_intensity()) {
    in = src.intensity(q);
    // the `< 0` check runs on every kept point, inside the image or not (:108-127, :248); such points are not drawn
    if (a.strategy == PCV_XRAY_COLORED_WITH_INTENSITY && in < 0.0f) {
      o.neg = true;
      return o;
    }
    if constexpr (!Source::kBinColumn)
      if (a.binned) o.bin = rust_i64((double)in / a.bin_size);  // BinnedColoringStrategy::bins (:138-157)
  }
  if constexpr (Source::kBinColumn) o.bin = src.bin(q, a.bin_size);  // the same, from the cloud's column
  V3d p = src.position(q);
  if (a.has_iso) p = v_add(quat_rotate(a.iso + 3, p), V3d{a.iso[0], a.iso[1], a.iso[2]});
  const double W = (double)a.W;
  const uint32_t x = sat_u32(((p.x - t.min[0]) / t.diag[0]) * W);
  const uint32_t y = sat_u32((1.0 - ((p.y - t.min[1]) / t.diag[1])) * W);
  const uint32_t z = sat_u32(((p.z - t.min[2]) / t.diag[2]) * 1024.0);
  if (x >= a.W || y >= a.W) return o;  // only the image's own pixels are ever read (:507-510): never drawn
  o.draw = true;
  o.bucket = bbase + (y / kBlk) * a.nbx + x / kBlk;
  uint64_t rec = (uint64_t)((y % kBlk) * kBlk + x % kBlk) | (uint64_t)(z < kZMax ? z : kZMax) << 10;
  if (a.strategy == PCV_XRAY_COLORED) {
    const auto* c = src.color(q);
    rec |= ((uint64_t)c[0] | (uint64_t)c[1] << 8 | (uint64_t)c[2] << 16) << 32;
  } else if (a.strategy == PCV_XRAY_COLORED_WITH_INTENSITY) {
    rec |= (uint64_t)__float_as_uint(in) << 32;
  }
  o.rec = rec;
  o.z = p.z;
  return o;
}

// one chunk by one wave, 64 points a step. COUNT: one counter add per distinct bucket of the 64 points (wave match on the
// bucket); SCATTER: the same adds reserve each point's slot in its bucket.
template <bool SCATTER, class Source>
__device__ __forceinline__ void xray_bin_chunk(const XrayBinArgs& a, const Source& src, uint32_t cnt, int32_t created, const XrayTileDev& t,
                                               uint32_t bbase, uint32_t lane, uint32_t* __restrict__ counts,
                                               const uint64_t* __restrict__ offsets, uint64_t* __restrict__ rec, double* __restrict__ recz,
                                               int64_t* __restrict__ recb) {
  for (uint32_t q0 = 0; q0 < cnt; q0 += 64) {
    const uint32_t q = q0 + lane;
    const XrayPoint pt = xray_point(a, src, t, bbase, q, q < cnt && src.kept(q));
    if (!SCATTER && a.negative) {
      const unsigned long long negs = __ballot(pt.neg);
      if (negs && lane == 0) atomicAdd(a.negative + created, (unsigned long long)__popcll(negs));
    }
    unsigned long long live = __ballot(pt.draw);
    while (live) {
      const int leader = __ffsll(live) - 1;
      const uint32_t k = __shfl(pt.bucket, leader);
      const bool peer = pt.draw && pt.bucket == k;
      const unsigned long long peers = __ballot(peer);
      uint32_t base = 0;
      if ((uint32_t)leader == lane) base = atomicAdd(counts + k, (uint32_t)__popcll(peers));
      if (SCATTER) {
        base = __shfl(base, leader);
        if (peer) {
          const uint64_t pos = offsets[k] + base + (uint64_t)__popcll(peers & ((1ull << lane) - 1ull));
          if (pos < offsets[k + 1]) {  // always true: both passes compute the same buckets
            rec[pos] = pt.rec;
            if (recz) recz[pos] = pt.z;
            if (recb) recb[pos] = pt.bin;
          }
        }
      }
      live &= ~peers;
    }
  }
}

// a wave per chunk of the group, whose chunks are those of all its clouds one after another. A wave's chunk index only
// grows, so its cloud is found by a wave-uniform search forward from the last one. S2: the chunks are those of S2 queries
// (XrayTreeChunks::desc is a PcvS2Chunk list, keep the u32 flags, xyz the cloud's f64 positions); past the chunk's
// descriptor the instances of both kinds run xray_bin_chunk. COLUMN (S2 scatter only: the count pass needs no bin): the bin
// of a record is read from the cloud's column, a.columns[k], instead of the intensity.
template <bool SCATTER, bool S2, bool COLUMN = false>
__global__ __launch_bounds__(256) void xray_bin_kernel(XrayBinArgs a, uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets,
                                                       uint64_t* __restrict__ rec, double* __restrict__ recz,
                                                       int64_t* __restrict__ recb) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint32_t k = 0;
  uint64_t kend = a.ntrees > 1 ? a.trees[1].first : a.nchunks;  // first chunk past cloud k
  for (uint64_t gi = (uint64_t)blockIdx.x * 4 + wave; gi < a.nchunks; gi += (uint64_t)gridDim.x * 4) {
    if (gi >= kend) {  // the last entry in (k, ntrees) whose first <= gi
      uint32_t lo = k + 1, hi = a.ntrees - 1;
      while (lo < hi) {
        const uint32_t m = (lo + hi + 1) >> 1;
        if (a.trees[m].first <= gi) lo = m;
        else hi = m - 1;
      }
      k = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
      kend = k + 1 < a.ntrees ? a.trees[k + 1].first : a.nchunks;
    }
    const XrayTreeChunks tr = a.trees[k];
    if constexpr (S2) {
      const PcvS2Chunk c = ((const PCV_GLOBAL PcvS2Chunk*)tr.desc)[tr.c0 + (gi - tr.first)];
      const int32_t created = a.created_of_shape[c.location];
      if (created < 0) continue;  // wave-uniform: no cloud's query kept anything for this tile
      const XrayTileDev t = a.tiles[created];
      const uint32_t bbase = ((uint32_t)created - a.created0) * a.nblocks;
      const XrayS2Source s2src{(const PCV_GLOBAL double*)tr.xyz + 3 * c.src, tr.rgb + 3 * c.src,
                               tr.inten ? (const PCV_GLOBAL float*)tr.inten + c.src : nullptr, (const PCV_GLOBAL uint32_t*)tr.keep + c.first};
      if constexpr (COLUMN) {
        static_assert(SCATTER && S2, "a bin column is read by the S2 scatter pass only");
        const XrayBinColumn bc = a.columns[k];
        XrayS2ColumnSource src{s2src, bc.col + c.src * (uint64_t)s2attr::element_size(bc.data_type), bc.data_type};
        xray_bin_chunk<SCATTER>(a, src, c.count, created, t, bbase, lane, counts, offsets, rec, recz, recb);
      } else {
        xray_bin_chunk<SCATTER>(a, s2src, c.count, created, t, bbase, lane, counts, offsets, rec, recz, recb);
      }
    } else {
      const ChunkDesc d = tr.desc[tr.c0 + (gi - tr.first)];
      const int32_t created = a.created_of_shape[d.enc >> 8];
      if (created < 0) continue;  // wave-uniform: no octree's query kept anything for this tile
      const XrayTileDev t = a.tiles[created];
      const uint32_t bbase = ((uint32_t)created - a.created0) * a.nblocks;
      const PointsView v = points_view_of(d, (const uint8_t*)tr.xyz);
      const XrayNodeSource src{(const uint8_t*)tr.rgb, (const float*)tr.inten, d, v, tr.keep + d.keep_off};
      xray_bin_chunk<SCATTER>(a, src, d.cnt, created, t, bbase, lane, counts, offsets, rec, recz, recb);
    }
  }
}

// Points of one run of equal keys in consecutive lanes are summed by a segmented scan; the run's last lane returns true
// with the run total in `v` and the run length in `len`. Records of a bucket arrive in node order, so runs are long where
// the cloud is dense (VERDICT r06 "What's weak" 5: aggregate before the LDS atomic).
template <typename T>
__device__ __forceinline__ bool run_total(uint32_t key, bool valid, T& v, uint32_t& len, uint32_t lane) {
  const uint32_t kk = valid ? key : 0xffffffffu;
  const uint32_t prev = __shfl_up(kk, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != kk);
  const unsigned long long upto = heads & ((2ull << lane) - 1ull);  // lane 63: all bits
  const uint32_t start = 63u - (uint32_t)__clzll(upto);
#pragma unroll
  for (uint32_t o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o);
    if (lane >= start + o) v += t;
  }
  len = lane - start + 1;
  return valid && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
}

struct XrayAccArgs {
  const uint64_t* rec;
  const double* recz;
  const uint64_t* offsets;
  uint32_t* image;  // created tiles x W x W RGBA8, rows top to bottom
  unsigned long long* drawn;
  uint32_t created0, W, nbx, nblocks;
  uint32_t nbuckets;  // (tiles of the group) x nblocks; the grid strides over them
  uint32_t bg;
  uint32_t colormap;
  float max_stddev;
  uint32_t strategy;  // xray_sorted: PCV_XRAY_COLORED (binned) or PCV_XRAY_COLORED_WITH_INTENSITY
  float min_intensity, max_intensity;
};

template <int STRAT>
struct AccLds {
  static constexpr uint32_t u64s = STRAT == PCV_XRAY_XRAY ? kBlkPx * kZWords / 2 : STRAT == PCV_XRAY_COLORED ? kBlkPx * 7 / 2 : kBlkPx * 5 / 2;
};

// NT threads: 1024 for xray, whose 132 KiB of bit sets allow one workgroup per CU, 256 otherwise. The grid is what is
// resident at once and strides over the buckets, so the dispatch size does not grow with the number of tiles
template <int STRAT, int NT>
__global__ __launch_bounds__(NT) void xray_accum_kernel(XrayAccArgs a, const uint8_t* __restrict__ value_table) {
  __shared__ uint64_t lds[AccLds<STRAT>::u64s];
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t b = blockIdx.x; b < a.nbuckets; b += gridDim.x) {
  const uint32_t slot = b / a.nblocks, blk = b % a.nblocks;
  const uint64_t beg = a.offsets[b], end = a.offsets[b + 1];
  for (uint32_t i = threadIdx.x; i < AccLds<STRAT>::u64s; i += NT) lds[i] = 0;
  __syncthreads();
  uint32_t* bits = reinterpret_cast<uint32_t*>(lds);                        // xray: [pixel][33 words]
  unsigned long long* csum = reinterpret_cast<unsigned long long*>(lds);    // colored: [3][1024] u64 sums
  double* zsum = reinterpret_cast<double*>(lds);                            // stddev: [1024] sums, then means
  double* zss = reinterpret_cast<double*>(lds) + kBlkPx;                    //         [1024] squared deviations
  uint32_t* cnt = reinterpret_cast<uint32_t*>(lds + (STRAT == PCV_XRAY_COLORED ? 3 * kBlkPx : 2 * kBlkPx));
  for (uint64_t i0 = beg; i0 < end; i0 += NT) {
    const uint64_t i = i0 + threadIdx.x;
    const bool valid = i < end;
    const uint64_t r = valid ? a.rec[i] : 0;
    const uint32_t pix = (uint32_t)r & (kBlkPx - 1), z = ((uint32_t)r >> 10) & 2047u;
    if (STRAT == PCV_XRAY_XRAY) {
      // a set: only the last lane of a run of equal (pixel, z) sets the bit
      const uint32_t key = pix << 11 | z;
      const uint32_t kk = valid ? key : 0xffffffffu;
      const uint32_t next = __shfl_down(kk, 1);
      if (valid && (lane == 63 || next != kk)) atomicOr(bits + pix * kZWords + (z >> 5), 1u << (z & 31u));
    } else if (STRAT == PCV_XRAY_COLORED) {
      // 21 bits per channel hold a run's sum (64 x 255)
      const uint32_t c = (uint32_t)(r >> 32);
      uint64_t v = valid ? ((uint64_t)(c & 255u) | (uint64_t)((c >> 8) & 255u) << 21 | (uint64_t)((c >> 16) & 255u) << 42) : 0;
      uint32_t len;
      if (run_total(pix, valid, v, len, lane)) {
        atomicAdd(csum + pix, (unsigned long long)(v & 0x1fffffull));
        atomicAdd(csum + kBlkPx + pix, (unsigned long long)((v >> 21) & 0x1fffffull));
        atomicAdd(csum + 2 * kBlkPx + pix, (unsigned long long)(v >> 42));
        atomicAdd(cnt + pix, len);
      }
    } else {
      double v = valid ? a.recz[i] : 0.0;
      uint32_t len;
      if (run_total(pix, valid, v, len, lane)) {
        atomicAdd(zsum + pix, v);
        atomicAdd(cnt + pix, len);
      }
    }
  }
  __syncthreads();
  if (STRAT == PCV_XRAY_HEIGHT_STDDEV && end > beg) {
    // second sweep over the block's records: squared deviations from the pixel mean (population variance q / n)
    for (uint32_t p = threadIdx.x; p < kBlkPx; p += NT)
      if (cnt[p]) zsum[p] = zsum[p] / (double)cnt[p];
    __syncthreads();
    for (uint64_t i0 = beg; i0 < end; i0 += NT) {
      const uint64_t i = i0 + threadIdx.x;
      const bool valid = i < end;
      const uint32_t pix = valid ? (uint32_t)a.rec[i] & (kBlkPx - 1) : 0u;
      double v = 0.0;
      if (valid) {
        const double dz = a.recz[i] - zsum[pix];
        v = dz * dz;
      }
      uint32_t len;
      if (run_total(pix, valid, v, len, lane)) atomicAdd(zss + pix, v);
    }
    __syncthreads();
  }
  // finalise: the block's pixels of image `created`
  const uint32_t by = blk / a.nbx, bx = blk % a.nbx;
  uint32_t* img = a.image + (uint64_t)(a.created0 + slot) * a.W * a.W;
  for (uint32_t p = threadIdx.x; p < kBlkPx; p += NT) {
    const uint32_t gx = bx * kBlk + (p % kBlk), gy = by * kBlk + (p / kBlk);
    if (gx >= a.W || gy >= a.W) continue;
    Rgba8 c{255, 255, 255, 0};  // TRANSPARENT.to_u8(): no point in this pixel (:507)
    if (STRAT == PCV_XRAY_XRAY) {
      uint32_t n = 0;
      for (uint32_t w = 0; w < kZWords; ++w) n += (uint32_t)__popc(bits[p * kZWords + w]);
      if (n) {
        const uint8_t v = value_table[n];
        c = Rgba8{v, v, v, 255};
      }
    } else if (STRAT == PCV_XRAY_COLORED) {
      if (cnt[p]) c = colored(csum[p], csum[kBlkPx + p], csum[2 * kBlkPx + p], cnt[p]);
    } else {
      if (cnt[p]) c = height_stddev(sqrt(zss[p] / (double)cnt[p]), a.max_stddev, a.colormap);
    }
    img[(uint64_t)gy * a.W + gx] = with_background(c, a.bg);
  }
  if (threadIdx.x == 0 && end > beg) atomicAdd(a.drawn + a.created0 + slot, (unsigned long long)(end - beg));
  __syncthreads();  // the next bucket clears the LDS the finalisation above reads
  }
}

// ---- colored_with_intensity and binning: every (pixel, bin) reduced in a fixed key order ---------------------------------
// A pixel may hold any number of bins, so per-pixel LDS state does not do. Instead a bucket's records are sorted by the key
// (pixel, bin, record) — a total order on their contents, so the sorted bucket, and every f32 sum taken along it, does not
// depend on the order the scatter wrote them in (scheduling, tile grouping, octree order). A bucket of at most `lds_cap`
// records is sorted in LDS; a larger one in place in the group's workspace by the same network, its steps of distance
// below lds_cap on LDS-sized chunks. Then one thread per pixel walks its run: per bin the count and the sum, per pixel the
// bin means in ascending bin order.
constexpr uint32_t kSortCapBinned = 4096;  // 16-byte records: 64 KiB of LDS
constexpr uint32_t kSortCapPlain = 8192;   // 8-byte records
constexpr uint32_t kSortThreads = 512;
// at most this many kept points in one tile of the sorted strategies (checked by the group planning, pcv_xray_plan_groups):
// a bucket then has at most 2^30 records, so the u32 indices and powers of two of the network below cannot overflow
constexpr uint64_t kMaxSortedTilePoints = PCV_XRAY_MAX_SORTED_TILE_POINTS;
static_assert(kMaxSortedTilePoints == 1ull << 30, "xray_sorted's u32 indices need a bucket of at most 2^30 records");

template <bool BINNED>
__device__ __forceinline__ bool key_less(uint64_t ra, int64_t ba, uint64_t rb, int64_t bb) {
  const uint32_t pa = (uint32_t)ra & (kBlkPx - 1), pb = (uint32_t)rb & (kBlkPx - 1);
  if (pa != pb) return pa < pb;
  if (BINNED && ba != bb) return ba < bb;
  return ra < rb;
}
// one step of the bitonic network over [0, n) with the elements past n taken as +inf: every comparator puts the smaller key
// at the lower index (the first step of each merge compares mirrored pairs, i ^ (k - 1)), so the missing tail never
// moves and comparators that reach it are skipped. `comparators` = (n rounded up to a power of two) / 2.
template <bool BINNED>
__device__ __forceinline__ void bitonic_step(uint64_t* R, int64_t* B, uint32_t n, uint32_t comparators, uint32_t k, uint32_t j) {
  for (uint32_t c = threadIdx.x; c < comparators; c += kSortThreads) {
    const uint32_t i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
    const uint32_t p = j == (k >> 1) ? (i ^ (k - 1)) : i + j;
    if (p >= n) continue;
    const uint64_t ri = R[i], rp = R[p];
    const int64_t bi = BINNED ? B[i] : 0, bp = BINNED ? B[p] : 0;
    if (key_less<BINNED>(rp, bp, ri, bi)) {
      R[i] = rp;
      R[p] = ri;
      if (BINNED) {
        B[i] = bp;
        B[p] = bi;
      }
    }
  }
}
__device__ __forceinline__ uint32_t pow2_ceil(uint32_t n) { return n <= 1 ? 1u : 1u << (32 - __clz(n - 1)); }
// stages k = 2 .. kmax of the network on [0, n) (kmax = the power of two >= n: a whole sort)
template <bool BINNED>
__device__ void bitonic_stages(uint64_t* R, int64_t* B, uint32_t n, uint32_t kmax) {
  const uint32_t comparators = pow2_ceil(n) >> 1;
  for (uint32_t k = 2; k <= kmax; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      bitonic_step<BINNED>(R, B, n, comparators, k, j);
      __syncthreads();
    }
}
template <bool BINNED>
__device__ void chunk_load(uint64_t* sr, int64_t* sb, const uint64_t* R, const int64_t* B, uint32_t m) {
  for (uint32_t i = threadIdx.x; i < m; i += kSortThreads) {
    sr[i] = R[i];
    if (BINNED) sb[i] = B[i];
  }
  __syncthreads();
}
template <bool BINNED>
__device__ void chunk_store(const uint64_t* sr, const int64_t* sb, uint64_t* R, int64_t* B, uint32_t m) {
  for (uint32_t i = threadIdx.x; i < m; i += kSortThreads) {
    R[i] = sr[i];
    if (BINNED) B[i] = sb[i];
  }
  __syncthreads();
}
// the bucket [0, n) in global memory, n > L (a power of two): each L-chunk sorted in LDS, then the merges above L, their
// steps of distance >= L in global memory and the rest per chunk in LDS. Global writes of this workgroup are visible to
// its own later loads after the barrier (one CU, workgroup scope).
template <bool BINNED>
__device__ void sort_global(uint64_t* R, int64_t* B, uint32_t n, uint32_t L, uint64_t* sr, int64_t* sb) {
  for (uint32_t c0 = 0; c0 < n; c0 += L) {
    const uint32_t m = min(L, n - c0);
    chunk_load<BINNED>(sr, sb, R + c0, BINNED ? B + c0 : nullptr, m);
    bitonic_stages<BINNED>(sr, sb, m, pow2_ceil(m));
    chunk_store<BINNED>(sr, sb, R + c0, BINNED ? B + c0 : nullptr, m);
  }
  const uint32_t np = pow2_ceil(n);  // <= 2^30 (kMaxSortedTilePoints): k below stops at 2^31 at most
  for (uint64_t k = 2 * (uint64_t)L; k <= np; k <<= 1) {
    for (uint32_t j = k >> 1; j >= L; j >>= 1) {
      bitonic_step<BINNED>(R, B, n, np >> 1, (uint32_t)k, j);
      __syncthreads();
    }
    for (uint32_t c0 = 0; c0 < n; c0 += L) {
      const uint32_t m = min(L, n - c0);
      chunk_load<BINNED>(sr, sb, R + c0, BINNED ? B + c0 : nullptr, m);
      for (uint32_t j = L >> 1; j > 0; j >>= 1) {  // half-cleaners only: j < k / 2
        bitonic_step<BINNED>(sr, sb, m, L >> 1, 0u, j);
        __syncthreads();
      }
      chunk_store<BINNED>(sr, sb, R + c0, BINNED ? B + c0 : nullptr, m);
    }
  }
}
// first index in [0, n) whose pixel is >= p (the records are sorted by pixel first)
__device__ __forceinline__ uint32_t pixel_lower_bound(const uint64_t* R, uint32_t n, uint32_t p) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (((uint32_t)R[mid] & (kBlkPx - 1)) < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
// one pixel's sorted run [lo, hi), bins ascending: IntensityColoringStrategy (:269-291) or PointColorColoringStrategy
// (:347-355). Per bin, `sum / count as f32`; the bin means are added in ascending bin order and divided by `len() as f32`.
// colored's bin sums are exact integers, each bin mean rounded once to f32 as in the unbinned `colored`.
template <bool BINNED>
__device__ Rgba8 sorted_pixel(const XrayAccArgs& a, const uint64_t* R, const int64_t* B, uint32_t lo, uint32_t hi) {
  uint64_t nb = 0;
  if (a.strategy == PCV_XRAY_COLORED_WITH_INTENSITY) {
    float acc = 0.0f;
    for (uint32_t i = lo; i < hi;) {
      const int64_t bin = BINNED ? B[i] : 0;
      float sum = 0.0f;
      uint64_t c = 0;
      do {
        sum += __uint_as_float((uint32_t)(R[i] >> 32));
        ++c;
        ++i;
      } while (i < hi && (!BINNED || B[i] == bin));
      acc += sum / (float)c;
      ++nb;
    }
    return intensity_color(acc / (float)nb, a.min_intensity, a.max_intensity);
  }
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, aa = 0.0f;
  for (uint32_t i = lo; i < hi;) {
    const int64_t bin = BINNED ? B[i] : 0;
    uint64_t sr = 0, sg = 0, sb = 0, c = 0;
    do {
      const uint32_t col = (uint32_t)(R[i] >> 32);
      sr += col & 255u;
      sg += (col >> 8) & 255u;
      sb += (col >> 16) & 255u;
      ++c;
      ++i;
    } while (i < hi && (!BINNED || B[i] == bin));
    const double dn = 255.0 * (double)c;
    ar += (float)((double)sr / dn);
    ag += (float)((double)sg / dn);
    ab += (float)((double)sb / dn);
    aa += (float)(c < (1ull << 24) ? c : (1ull << 24)) / (float)c;
    ++nb;
  }
  const float fn = (float)nb;
  return to_u8(ar / fn, ag / fn, ab / fn, aa / fn);
}

// a grid of resident workgroups striding over the group's buckets, like xray_accum; `rec` / `recb` are written (the
// global path sorts in place)
template <bool BINNED>
__global__ __launch_bounds__(kSortThreads) void xray_sorted_kernel(XrayAccArgs a, uint64_t* __restrict__ rec, int64_t* __restrict__ recb,
                                                                   uint32_t lds_cap) {
  constexpr uint32_t kCap = BINNED ? kSortCapBinned : kSortCapPlain;
  __shared__ uint64_t sr[kCap];
  __shared__ int64_t sb[BINNED ? kCap : 1];
  const uint32_t L = lds_cap < kCap ? lds_cap : kCap;  // a power of two >= 2
  for (uint32_t b = blockIdx.x; b < a.nbuckets; b += gridDim.x) {
    const uint32_t slot = b / a.nblocks, blk = b % a.nblocks;
    const uint64_t beg = a.offsets[b], end = a.offsets[b + 1];
    const uint32_t n = (uint32_t)(end - beg);  // <= kMaxSortedTilePoints: the host refuses larger tiles
    int64_t* gb = BINNED ? recb + beg : nullptr;
    const uint64_t* R;
    const int64_t* B;
    if (n <= L) {
      chunk_load<BINNED>(sr, sb, rec + beg, gb, n);
      bitonic_stages<BINNED>(sr, sb, n, pow2_ceil(n));
      R = sr;
      B = sb;
    } else {
      sort_global<BINNED>(rec + beg, gb, n, L, sr, sb);
      R = rec + beg;
      B = gb;
    }
    const uint32_t by = blk / a.nbx, bx = blk % a.nbx;
    uint32_t* img = a.image + (uint64_t)(a.created0 + slot) * a.W * a.W;
    for (uint32_t p = threadIdx.x; p < kBlkPx; p += kSortThreads) {
      const uint32_t gx = bx * kBlk + (p % kBlk), gy = by * kBlk + (p / kBlk);
      if (gx >= a.W || gy >= a.W) continue;
      Rgba8 c{255, 255, 255, 0};  // TRANSPARENT.to_u8()
      const uint32_t lo = pixel_lower_bound(R, n, p), hi = pixel_lower_bound(R, n, p + 1);
      if (hi > lo) c = sorted_pixel<BINNED>(a, R, B, lo, hi);
      img[(uint64_t)gy * a.W + gx] = with_background(c, a.bg);
    }
    if (threadIdx.x == 0 && end > beg) atomicAdd(a.drawn + a.created0 + slot, (unsigned long long)(end - beg));
    __syncthreads();  // the next bucket overwrites the LDS the finalisation above reads
  }
}

// ---- host: quadtree geometry ----------------------------------------------------------------------------------------
int fail_msg(char* err, uint64_t errcap, const std::string& m) {
  if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
  return PCV_E_INVALID;
}

V3d iso_point(const double* iso, V3d p) { return v_add(quat_rotate(iso + 3, p), V3d{iso[0], iso[1], iso[2]}); }

int leaf_geometry(uint32_t tile_size_px, double pixel_size_m, const double bmin[3], const double bmax[3], const double* iso,
                  uint32_t root_level, uint64_t root_index, bool list, LeafGeometry* g, char* err, uint64_t errcap) {
  if (tile_size_px == 0 || tile_size_px > kMaxTilePx) return fail_msg(err, errcap, "xray: tile_size_px must be in 1 ..= 32768");
  if (!(pixel_size_m > 0.0) || !std::isfinite(pixel_size_m)) return fail_msg(err, errcap, "xray: pixel_size_m must be finite and > 0");
  // get_bounding_box (:550): the meta Aabb, or Aabb::transform — the 8 corners (compute_corners order) folded by grow
  if (iso) {
    V3d c[8];
    int k = 0;
    for (int ix = 0; ix < 2; ++ix)
      for (int iy = 0; iy < 2; ++iy)
        for (int iz = 0; iz < 2; ++iz) c[k++] = V3d{ix ? bmax[0] : bmin[0], iy ? bmax[1] : bmin[1], iz ? bmax[2] : bmin[2]};
    const V3d f = iso_point(iso, c[0]);
    double lo[3] = {f.x, f.y, f.z}, hi[3] = {f.x, f.y, f.z};
    for (int i = 1; i < 8; ++i) {
      const V3d p = iso_point(iso, c[i]);
      const double pv[3] = {p.x, p.y, p.z};
      for (int a = 0; a < 3; ++a) {  // Point3::inf / sup: per-component min / max
        lo[a] = pv[a] < lo[a] ? pv[a] : lo[a];
        hi[a] = pv[a] > hi[a] ? pv[a] : hi[a];
      }
    }
    for (int a = 0; a < 3; ++a) {
      g->bbox_min[a] = lo[a];
      g->bbox_max[a] = hi[a];
    }
  } else {
    for (int a = 0; a < 3; ++a) {
      g->bbox_min[a] = bmin[a];
      g->bbox_max[a] = bmax[a];
    }
  }
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(g->bbox_min[a]) || !std::isfinite(g->bbox_max[a])) return fail_msg(err, errcap, "xray: bounding box is not finite");
  // find_quadtree_bounding_rect_and_levels (:515-532)
  const double dx = g->bbox_max[0] - g->bbox_min[0], dy = g->bbox_max[1] - g->bbox_min[1];
  double cur = (double)tile_size_px * pixel_size_m;
  uint32_t levels = 0;
  while (cur < dx || cur < dy) {
    cur *= 2.0;
    ++levels;
    if (levels > 63) return fail_msg(err, errcap, "xray: more than 63 quadtree levels");
  }
  g->rect[0] = g->bbox_min[0];
  g->rect[1] = g->bbox_min[1];
  g->rect[2] = cur;
  g->deepest_level = levels;
  if (root_level > levels)
    return fail_msg(err, errcap, "xray: root_node_id (level " + std::to_string(root_level) + ") is outside the quadtree of " +
                                     std::to_string(levels) + " levels");
  if (root_level < 32 && root_index >= (1ull << (2 * root_level))) return fail_msg(err, errcap, "xray: root_node_id index out of range");
  const uint32_t depth = levels - root_level;
  if (depth > 12)  // 4^depth > 2^24
    return fail_msg(err, errcap, "xray: " + std::string("more than 2^24 leaf tiles below root_node_id (") + std::to_string(depth) +
                                     " levels): split the job by choosing deeper root_node_ids");
  // Node::from_node_id_and_root_bounding_rect: get_child from the root down (quadtree/src/lib.rs:59-97)
  double mn[2] = {g->rect[0], g->rect[1]}, edge = g->rect[2];
  for (int l = (int)root_level - 1; l >= 0; --l) {
    const uint32_t ci = (uint32_t)(root_index >> (2 * l)) & 3u;
    const double half = edge / 2.0;
    if (ci & 1u) mn[1] += half;
    if (ci & 2u) mn[0] += half;
    edge = half;
  }
  g->index.clear();
  g->rect_min.clear();
  g->leaf_edge = edge;
  for (uint32_t l = 0; l < depth; ++l) g->leaf_edge /= 2.0;
  if (!list) return PCV_OK;
  // get_nodes_at_level (:534-548): a stack, children pushed 0..3, so child 3 is popped first
  struct Item {
    uint64_t index;
    uint32_t level;
    double mn[2], edge;
  };
  std::vector<Item> stack;
  stack.push_back(Item{root_index, root_level, {mn[0], mn[1]}, edge});
  const size_t n = (size_t)1 << (2 * depth);
  g->index.reserve(n);
  g->rect_min.reserve(2 * n);
  while (!stack.empty()) {
    const Item it = stack.back();
    stack.pop_back();
    if (it.level == levels) {
      g->index.push_back(it.index);
      g->rect_min.push_back(it.mn[0]);
      g->rect_min.push_back(it.mn[1]);
      continue;
    }
    const double half = it.edge / 2.0;
    for (uint32_t ci = 0; ci < 4; ++ci) {
      Item c{(it.index << 2) + ci, it.level + 1, {it.mn[0], it.mn[1]}, half};
      if (ci & 1u) c.mn[1] += half;
      if (ci & 2u) c.mn[0] += half;
      stack.push_back(c);
    }
  }
  return PCV_OK;
}

// the tile bbox of create_leaf_nodes (:625-629) and its query shape (xray_from_points :470-476)
void tile_box(const LeafGeometry& g, size_t i, double mn[3], double mx[3]) {
  mn[0] = g.rect_min[2 * i];
  mn[1] = g.rect_min[2 * i + 1];
  mn[2] = g.bbox_min[2];
  mx[0] = mn[0] + g.leaf_edge;  // Rect::max
  mx[1] = mn[1] + g.leaf_edge;
  mx[2] = g.bbox_max[2];
}
// Obb::from(&Aabb) (obb.rs:20-27) transformed by global_from_query = query_from_global.inverse() (obb.rs:44-46):
// query_from_obb = global_from_query * (center, identity); params = translation xyz, quaternion ijkw, half extent xyz
void tile_obb(const double* iso, const double mn[3], const double mx[3], double out[10]) {
  const double qi[4] = {-iso[3], -iso[4], -iso[5], iso[6]};  // UnitQuaternion::inverse: the conjugate
  const V3d ti = quat_rotate(qi, V3d{-iso[0], -iso[1], -iso[2]});  // Isometry3::inverse: rotation^-1 * (-translation)
  const V3d c{(mn[0] + mx[0]) * 0.5, (mn[1] + mx[1]) * 0.5, (mn[2] + mx[2]) * 0.5};  // nalgebra::center
  const V3d t = v_add(ti, quat_rotate(qi, c));                                   // Isometry3 * Isometry3
  // rotation: qi * identity (Quaternion product with (0, 0, 0, 1))
  const double w = qi[3] * 1.0 - ((qi[0] * 0.0 + qi[1] * 0.0) + qi[2] * 0.0);
  out[0] = t.x;
  out[1] = t.y;
  out[2] = t.z;
  out[3] = qi[3] * 0.0 + qi[0] * 1.0 + (qi[1] * 0.0 - qi[2] * 0.0);
  out[4] = qi[3] * 0.0 + qi[1] * 1.0 + (qi[2] * 0.0 - qi[0] * 0.0);
  out[5] = qi[3] * 0.0 + qi[2] * 1.0 + (qi[0] * 0.0 - qi[1] * 0.0);
  out[6] = w;
  for (int a = 0; a < 3; ++a) out[7 + a] = (mx[a] - mn[a]) * 0.5;  // Aabb::diag * 0.5
}

}  // namespace

// ---- the registry of live objects (pcv_xray_obj.h) -------------------------------------------------------------------
namespace {
std::mutex g_xray_mu;
std::unordered_map<const pcv_xray*, uint64_t> g_xray_live;
uint64_t g_xray_serial = 0;
}  // namespace

pcv_xray::pcv_xray() {
  std::lock_guard<std::mutex> g(g_xray_mu);
  g_xray_live[this] = serial = ++g_xray_serial;
}
pcv_xray::~pcv_xray() {
  std::lock_guard<std::mutex> g(g_xray_mu);
  g_xray_live.erase(this);
}
bool xray_is_live(const pcv_xray* x) {
  std::lock_guard<std::mutex> g(g_xray_mu);
  return g_xray_live.count(x) != 0;
}
bool xray_part_alive(const XrayPartRef& r) {
  std::lock_guard<std::mutex> g(g_xray_mu);
  auto it = g_xray_live.find(r.part);
  return it != g_xray_live.end() && it->second == r.serial;
}

extern "C" int pcv_xray_leaf_tiles(uint32_t tile_size_px, double pixel_size_m, const double bbox_min[3], const double bbox_max[3],
                                   const double* query_from_global, uint32_t root_level, uint64_t root_index, uint64_t capacity,
                                   double rect[3], uint32_t* deepest_level, uint64_t* num_leaves, uint64_t* leaf_index,
                                   double* tile_bbox, double* query_obb, char* err, uint64_t errcap) {
  if (!bbox_min || !bbox_max) return fail_msg(err, errcap, "null argument");
  LeafGeometry g;
  const int rc = leaf_geometry(tile_size_px, pixel_size_m, bbox_min, bbox_max, query_from_global, root_level, root_index, capacity > 0, &g,
                               err, errcap);
  if (rc) return rc;
  if (rect) std::memcpy(rect, g.rect, sizeof(g.rect));
  if (deepest_level) *deepest_level = g.deepest_level;
  if (num_leaves) *num_leaves = (uint64_t)1 << (2 * (g.deepest_level - root_level));
  const size_t n = std::min<size_t>(g.index.size(), capacity);
  for (size_t i = 0; i < n; ++i) {
    double mn[3], mx[3];
    tile_box(g, i, mn, mx);
    if (leaf_index) leaf_index[i] = g.index[i];
    if (tile_bbox) {
      std::memcpy(tile_bbox + 6 * i, mn, sizeof(mn));
      std::memcpy(tile_bbox + 6 * i + 3, mx, sizeof(mx));
    }
    if (query_obb && query_from_global) tile_obb(query_from_global, mn, mx, query_obb + 10 * i);
  }
  return PCV_OK;
}

extern "C" int pcv_xray_finalize(int fn, uint64_t count, const double* in, uint8_t* rgba) {
  if ((count && (!in || !rgba)) || fn < PCV_XRAY_FN_XRAY || fn > PCV_XRAY_FN_INTENSITY) return PCV_E_INVALID;
  uint8_t table[kZWords * 32 + 1];
  xray_value_table(table);
  for (uint64_t i = 0; i < count; ++i) {
    Rgba8 c{255, 255, 255, 0};
    if (fn == PCV_XRAY_FN_XRAY) {
      const double n = in[i];
      if (!(n >= 0.0 && n <= 1025.0)) return PCV_E_INVALID;
      if (n >= 1.0) c = Rgba8{table[(uint32_t)n], table[(uint32_t)n], table[(uint32_t)n], 255};
    } else if (fn == PCV_XRAY_FN_COLORED) {
      const double* s = in + 4 * i;
      if (s[3] >= 1.0) c = colored((uint64_t)s[0], (uint64_t)s[1], (uint64_t)s[2], (uint64_t)s[3]);
    } else if (fn == PCV_XRAY_FN_JET) {
      c = jet((float)in[i]);
    } else if (fn == PCV_XRAY_FN_PURPLISH) {
      c = purplish((float)in[i]);
    } else if (fn == PCV_XRAY_FN_INTENSITY) {
      const double* s = in + 3 * i;
      c = intensity_color((float)s[0], (float)s[1], (float)s[2]);
    } else {
      const double* s = in + 4 * i;
      c = to_u8((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
    }
    std::memcpy(rgba + 4 * i, &c, 4);
  }
  return PCV_OK;
}

extern "C" void pcv_xray_free(pcv_xray* x) {
  if (!x) return;
  if (x->ctx) {
    x->ctx->dev_free(x->d_images);
    x->ctx->dev_free(x->d_parents);
  }
  delete x;
}

// PointCloudClientBuilder::build's bounding box (point_cloud_client/src/lib.rs:101-125): the first octree's meta box, grown
// by every octree's min and then its max in list order (Aabb::grow, aabb.rs:41-44: Point3::inf / sup per component); the
// same over S2 cell clouds (:121-131)
template <class Cloud>
static void union_box(Cloud* const* trees, uint32_t K, double lo[3], double hi[3]) {
  for (int a = 0; a < 3; ++a) {
    lo[a] = trees[0]->bbox_min[a];
    hi[a] = trees[0]->bbox_max[a];
  }
  for (uint32_t t = 0; t < K; ++t)
    for (const double* q : {trees[t]->bbox_min, trees[t]->bbox_max})
      for (int a = 0; a < 3; ++a) {
        lo[a] = q[a] < lo[a] ? q[a] : lo[a];
        hi[a] = q[a] > hi[a] ? q[a] : hi[a];
      }
}

// whether colored / colored_with_intensity bin on intensity (xray and height_stddev ignore binning, attributes() :133)
static bool coloring_binned(const pcv_xray_params* p, const pcv_xray_coloring* col) {
  return col && col->binning_attribute && (p->strategy == PCV_XRAY_COLORED || p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY);
}

// tile groups: consecutive created tiles whose records (8 B per kept point, 16 B for height_stddev and with binning: the
// z or the bin plane) and bucket tables fit the workspace, at most max_group_buckets buckets each. group_first gets the
// first tile of every group and nc at the end. A tile over the workspace is PCV_E_OOM; a tile of colored_with_intensity or
// binned colored with more than kMaxSortedTilePoints kept points is PCV_E_INVALID (xray_sorted's u32 bucket indices).
// leaf_pos (nullable) names the tiles in messages.
static int plan_groups(const uint64_t* kept, uint64_t nc, const uint64_t* leaf_pos, uint32_t W, const pcv_xray_params* p,
                       const pcv_xray_coloring* col, std::vector<uint64_t>& group_first, uint64_t* max_pts_out, uint64_t* max_tiles_out,
                       char* err, uint64_t errcap) {
  const bool binned = coloring_binned(p, col);
  const bool sorted = binned || p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY;
  const uint32_t nbx = (W + kBlk - 1) / kBlk, nblocks = nbx * nbx;
  const uint64_t budget = p->max_workspace_bytes ? p->max_workspace_bytes : kDefaultWorkspace;
  const uint64_t rec_bytes = p->strategy == PCV_XRAY_HEIGHT_STDDEV || binned ? 16 : 8, bucket_bytes = 16ull * nblocks;
  // a group also holds at most kMaxGroupBuckets buckets; the experiment build can lower that (tests of the grouping)
  uint64_t max_group_buckets = kMaxGroupBuckets;
  if (pcv_switches().xray_max_group_buckets) max_group_buckets = pcv_switches().xray_max_group_buckets;
  const uint64_t max_group_tiles = std::max<uint64_t>(1, max_group_buckets / nblocks);
  group_first.assign(1, 0);
  uint64_t cur = 0, max_pts = 0, max_tiles = 0, pts = 0;
  for (uint64_t c = 0; c < nc; ++c) {
    const unsigned long long name = (unsigned long long)(leaf_pos ? leaf_pos[c] : c);
    if (sorted && kept[c] > kMaxSortedTilePoints) {
      char m[256];
      std::snprintf(m, sizeof(m), "xray: leaf tile %llu keeps %llu points, more than %llu for colored_with_intensity or binning: "
                    "use a smaller pixel_size_m or tile_size_px", name, (unsigned long long)kept[c], (unsigned long long)kMaxSortedTilePoints);
      fail_msg(err, errcap, m);
      return PCV_E_INVALID;
    }
    const uint64_t need = kept[c] * rec_bytes + bucket_bytes + 16;
    if (need > budget) {
      char m[256];
      std::snprintf(m, sizeof(m), "xray: leaf tile %llu keeps %llu points, %llu bytes of workspace > max_workspace_bytes %llu",
                    name, (unsigned long long)kept[c], (unsigned long long)need, (unsigned long long)budget);
      fail_msg(err, errcap, m);
      return PCV_E_OOM;
    }
    if (cur + need > budget || c - group_first.back() == max_group_tiles) {
      group_first.push_back(c);
      cur = 0;
      pts = 0;
    }
    cur += need;
    pts += kept[c];
    max_pts = std::max(max_pts, pts);
    max_tiles = std::max<uint64_t>(max_tiles, c + 1 - group_first.back());
  }
  group_first.push_back(nc);
  if (max_pts_out) *max_pts_out = max_pts;
  if (max_tiles_out) *max_tiles_out = max_tiles;
  return PCV_OK;
}

extern "C" int pcv_xray_plan_groups(const uint64_t* kept, uint64_t num_tiles, const pcv_xray_params* params,
                                    const pcv_xray_coloring* coloring, uint64_t capacity, uint64_t* num_groups, uint64_t* group_first,
                                    char* err, uint64_t errcap) {
  if (!params || (num_tiles && !kept)) return fail_msg(err, errcap, "null argument");
  if (params->tile_size_px == 0 || params->tile_size_px > kMaxTilePx) return fail_msg(err, errcap, "xray: tile_size_px must be in 1 ..= 32768");
  std::vector<uint64_t> first;
  const int rc = plan_groups(kept, num_tiles, nullptr, params->tile_size_px, params, coloring, first, nullptr, nullptr, err, errcap);
  if (rc) return rc;
  const uint64_t n = num_tiles ? first.size() - 1 : 0;
  if (num_groups) *num_groups = n;
  if (group_first) std::memcpy(group_first, first.data(), 8 * std::min<uint64_t>(n, capacity));
  return PCV_OK;
}

// ---- the leaf level over K octrees (K = 1: pcv_xray_run) ----------------------------------------------------------------
// One shape list, one query batch per octree, every raster pass one launch per tile group over the chunks of all K
// batches: xray_query_tiles, xray_plan_tiles, xray_upload_tables, xray_raster_groups, in that order.

namespace {

// The accumulation a run takes. colored_with_intensity, and colored with binning, take the sorted accumulation
// (xray_sorted); binning is ignored by xray and height_stddev (attributes() :133).
struct XrayAccum {
  const void* kernel;  // for the occupancy query
  uint32_t threads;
  int prof_id;
  void (*launch)(uint32_t grid, hipStream_t stream, const XrayAccArgs& a, uint64_t* rec, int64_t* recb, uint32_t sort_cap, const uint8_t* table);
};
template <bool BINNED>
void launch_sorted(uint32_t grid, hipStream_t stream, const XrayAccArgs& a, uint64_t* rec, int64_t* recb, uint32_t sort_cap, const uint8_t*) {
  hipLaunchKernelGGL(xray_sorted_kernel<BINNED>, dim3(grid), dim3(kSortThreads), 0, stream, a, rec, recb, sort_cap);
}
template <int STRAT, int NT>
void launch_accum(uint32_t grid, hipStream_t stream, const XrayAccArgs& a, uint64_t*, int64_t*, uint32_t, const uint8_t* table) {
  hipLaunchKernelGGL((xray_accum_kernel<STRAT, NT>), dim3(grid), dim3(NT), 0, stream, a, table);
}
XrayAccum xray_accum_of(uint32_t strategy, bool binned) {
  if (binned) return {(const void*)xray_sorted_kernel<true>, kSortThreads, PCV_K_XRAY_SORTED, launch_sorted<true>};
  if (strategy == PCV_XRAY_COLORED_WITH_INTENSITY) return {(const void*)xray_sorted_kernel<false>, kSortThreads, PCV_K_XRAY_SORTED, launch_sorted<false>};
  if (strategy == PCV_XRAY_XRAY) return {(const void*)xray_accum_kernel<PCV_XRAY_XRAY, 1024>, 1024, PCV_K_XRAY_ACCUM, launch_accum<PCV_XRAY_XRAY, 1024>};
  if (strategy == PCV_XRAY_COLORED) return {(const void*)xray_accum_kernel<PCV_XRAY_COLORED, 256>, 256, PCV_K_XRAY_ACCUM, launch_accum<PCV_XRAY_COLORED, 256>};
  return {(const void*)xray_accum_kernel<PCV_XRAY_HEIGHT_STDDEV, 256>, 256, PCV_K_XRAY_ACCUM, launch_accum<PCV_XRAY_HEIGHT_STDDEV, 256>};
}

// the clouds of a run, all of one kind (PointClouds::Octrees or ::S2Cells, point_cloud_client/src/lib.rs:107-132)
// what pcv_xray_run_s2_ex reads of its clouds beyond colour and intensity, after its checks
struct XrayS2Attrs {
  bool has_interval = false;  // an interval on intensity: params->interval, or the list's entry on "intensity"
  double interval[2] = {0.0, 0.0};
  std::vector<std::vector<PcvS2ExtraFilter>> filters;  // per cloud: the list's entries on its extras, every location each
  std::vector<int> bin_extra;                          // per cloud: the extra binned on; empty: intensity, or no binning read
};
struct XrayClouds {
  pcv_octree* const* trees = nullptr;
  pcv_s2_cloud* const* s2 = nullptr;
  uint32_t K = 0;
  const XrayS2Attrs* attrs = nullptr;  // pcv_xray_run_s2_ex only
};
// what the planning reads of one cloud's query over the tile shapes, an octree batch or an S2 query alike: shape -> segments
// -> kept points and chunks, and the pointers the raster passes read the chunks through
struct XraySource {
  const uint64_t* shape_first;  // [S + 1] first segment of each shape
  const uint64_t* seg_kept;     // [segments + 1] kept points before each segment
  const uint64_t* seg_chunk;    // [segments + 1] first chunk of each segment
  XrayTreeChunks chunks;        // desc, keep, xyz, rgb, inten (c0 and first are per tile group)
  XrayBinColumn column;         // S2, binning on a column: the cloud's
  uint64_t kept(uint64_t s) const { return seg_kept[shape_first[s + 1]] - seg_kept[shape_first[s]]; }
  uint64_t chunk_of(uint64_t s) const { return seg_chunk[shape_first[s]]; }
};
// the same shapes through every cloud (try_for_each_batch's jobs, src/iterator.rs:262-270); all K queries stay alive
// until the raster passes are done
struct XrayBatches {
  std::vector<pcv_query_batch*> b;
  std::vector<pcv_s2_query*> s2;
  std::vector<XraySource> src;  // one per cloud, in list order
  ~XrayBatches() {
    for (pcv_query_batch* q : b) pcv_query_batch_free(q);
    for (pcv_s2_query* q : s2) pcv_s2_query_free(q);
  }
};

// step 1: one shape per leaf tile (xray_from_points :470-476) and the K queries, pcv_query_batch_run or pcv_s2_query_run
int xray_query_tiles(pcv_ctx* ctx, const XrayClouds& clouds, const pcv_xray_params* p, const LeafGeometry& g, bool reads_intensity,
                     XrayBatches* batches) {
  const XrayS2Attrs* at = clouds.attrs;
  const bool filter = at ? at->has_interval : p->interval_attribute != nullptr;
  const double* interval = at ? at->interval : p->interval;
  const uint32_t S = (uint32_t)g.index.size();
  std::vector<pcv_shape> shapes(S);
  for (uint32_t i = 0; i < S; ++i) {
    double mn[3], mx[3];
    tile_box(g, i, mn, mx);
    pcv_shape& s = shapes[i];
    std::memset(&s, 0, sizeof(s));
    if (p->has_query_from_global) {
      s.kind = PCV_SHAPE_OBB;
      tile_obb(p->query_from_global, mn, mx, s.params);
    } else {
      s.kind = PCV_SHAPE_AABB;
      std::memcpy(s.params, mn, sizeof(mn));
      std::memcpy(s.params + 3, mx, sizeof(mx));
    }
  }
  std::vector<double> ivals;
  if (filter) {
    ivals.resize(2 * (size_t)S);
    for (uint32_t i = 0; i < S; ++i) {
      ivals[2 * (size_t)i] = interval[0];
      ivals[2 * (size_t)i + 1] = interval[1];
    }
  }
  pcv_shapes* sh = nullptr;
  int rc = pcv_shapes_create(ctx, shapes.data(), S, &sh);
  if (rc) return rc;
  batches->src.reserve(clouds.K);
  for (uint32_t t = 0; t < clouds.K && rc == PCV_OK; ++t) {
    XraySource e{};
    if (clouds.s2) {
      pcv_s2_cloud* c = clouds.s2[t];
      pcv_s2_query* q = nullptr;
      // the list's filters on extras: the same machinery, one launch per filtered column, on every location
      if (at && !at->filters[t].empty()) rc = pcv_s2_query_run_every(c, sh, filter ? ivals.data() : nullptr, at->filters[t], &q);
      else rc = pcv_s2_query_run(c, sh, 0, nullptr, nullptr, filter ? ivals.data() : nullptr, nullptr, &q);
      if (rc) break;
      batches->s2.push_back(q);
      e.shape_first = q->location_first.data();
      e.seg_kept = q->seg_offset.data();
      e.seg_chunk = q->seg_first_chunk.data();
      e.chunks.desc = (decltype(e.chunks.desc))q->d_chunks;
      e.chunks.keep = (decltype(e.chunks.keep))q->d_flags;
      e.chunks.xyz = (decltype(e.chunks.xyz))c->d_xyz;
      e.chunks.rgb = (decltype(e.chunks.rgb))c->d_rgb;
      e.chunks.inten = reads_intensity ? (decltype(e.chunks.inten))c->d_int : nullptr;
      if (at && !at->bin_extra.empty()) {
        const PcvS2Extra& x = c->extras[(size_t)at->bin_extra[t]];
        e.column = XrayBinColumn{(decltype(e.column.col))x.d, x.data_type, 0u};
      }
    } else {
      pcv_octree* tree = clouds.trees[t];
      pcv_query_batch* b = nullptr;
      if ((rc = pcv_query_batch_run(ctx, sh, tree, filter ? ivals.data() : nullptr, nullptr, &b))) break;
      batches->b.push_back(b);
      e.shape_first = b->shape_first.data();
      e.seg_kept = b->seg_off.data();
      e.seg_chunk = b->seg_chunk.data();
      e.chunks.desc = (decltype(e.chunks.desc))b->d_desc;
      e.chunks.keep = (decltype(e.chunks.keep))b->d_keep;
      e.chunks.xyz = (decltype(e.chunks.xyz))tree->d_xyz;
      e.chunks.rgb = (decltype(e.chunks.rgb))tree->d_rgb;
      e.chunks.inten = reads_intensity ? (decltype(e.chunks.inten))tree->d_int : nullptr;
    }
    batches->src.push_back(e);
  }
  pcv_shapes_free(sh);
  return rc;
}

// step 2: the created tiles (into x), their groups and, per group, the clouds that have chunks for its shapes, in list
// order, their chunk ranges end to end (u64 prefix)
struct XrayPlan {
  std::vector<int32_t> created_of_shape;
  std::vector<uint64_t> group_first;  // created tiles [group_first[g], group_first[g + 1]) are group g
  uint64_t max_pts = 0, max_tiles = 0;
  std::vector<XrayTreeChunks> trees;
  std::vector<XrayBinColumn> columns;  // parallel to `trees`
  std::vector<size_t> tree_first;  // group g's entries of `trees`: [tree_first[g], tree_first[g + 1])
  std::vector<uint64_t> group_chunks;
};
void xray_created_tiles(const std::vector<XraySource>& sources, uint32_t S, pcv_xray* x, XrayPlan* pl) {
  // a tile is created iff the queries kept a point (PointStream::callback never delivers an empty batch,
  // iterator.rs:148-151); kept is the sum over the clouds
  pl->created_of_shape.assign(S, -1);
  for (uint32_t s = 0; s < S; ++s) {
    uint64_t k = 0;
    for (const XraySource& b : sources) k += b.kept(s);
    if (k == 0) continue;
    pl->created_of_shape[s] = (int32_t)x->created.size();
    x->created.push_back(s);
    x->kept.push_back(k);
  }
  x->drawn.assign(x->created.size(), 0);
  x->negative.assign(x->created.size(), 0);
}
int xray_plan_tiles(pcv_ctx* ctx, const pcv_xray_params* p, const pcv_xray_coloring* col, const std::vector<XraySource>& sources,
                    const pcv_xray* x, XrayPlan* pl) {
  char m[256] = {0};
  if (int rc = plan_groups(x->kept.data(), x->created.size(), x->created.data(), x->W, p, col, pl->group_first, &pl->max_pts, &pl->max_tiles, m,
                           sizeof(m)))
    return ctx->fail(rc, m);
  pl->tree_first.assign(1, 0);
  for (size_t gi = 0; gi + 1 < pl->group_first.size(); ++gi) {
    const uint64_t s0 = x->created[pl->group_first[gi]], s1 = x->created[pl->group_first[gi + 1] - 1] + 1;
    uint64_t n = 0;
    for (const XraySource& b : sources) {
      const uint64_t c0 = b.chunk_of(s0), c1 = b.chunk_of(s1);
      if (c1 == c0) continue;
      XrayTreeChunks e = b.chunks;
      e.c0 = c0;
      e.first = n;
      pl->trees.push_back(e);
      pl->columns.push_back(b.column);
      n += c1 - c0;
    }
    pl->tree_first.push_back(pl->trees.size());
    pl->group_chunks.push_back(n);
  }
  return PCV_OK;
}

// step 3: the device tables of the raster passes, released with the scratch
struct XrayTables {
  explicit XrayTables(pcv_ctx* ctx) : sc(ctx) {}
  PcvScratch sc;
  int32_t* cos = nullptr;
  XrayTileDev* tiles = nullptr;
  XrayTreeChunks* trees = nullptr;
  XrayBinColumn* columns = nullptr;  // only where the bins come from a column
  uint8_t* table = nullptr;
  unsigned long long *drawn = nullptr, *neg = nullptr;
  uint32_t* counts = nullptr;
  uint64_t *off = nullptr, *rec = nullptr;
  double* recz = nullptr;
  int64_t* recb = nullptr;
  std::vector<XrayTileDev> h_tiles;  // what the uploads read: alive until the raster passes have synchronised
  uint8_t h_table[kZWords * 32 + 1];
};
int xray_upload_tables(pcv_ctx* ctx, const pcv_xray_params* p, bool binned, bool bin_column, const pcv_xray* x, const XrayPlan& pl,
                       uint32_t nblocks, XrayTables* t) {
  const uint64_t nc = x->created.size(), S = pl.created_of_shape.size();
  const uint64_t max_buckets = pl.max_tiles * nblocks, max_pts = std::max<uint64_t>(pl.max_pts, 1);
  PcvScratch& sc = t->sc;
  int rc;
  if ((rc = sc.get(&t->cos, S)) || (rc = sc.get(&t->tiles, nc)) || (rc = sc.get(&t->trees, std::max<size_t>(pl.trees.size(), 1))) ||
      (rc = sc.get(&t->table, kZWords * 32 + 1)) || (rc = sc.get(&t->drawn, nc)) || (rc = sc.get(&t->counts, max_buckets)) ||
      (rc = sc.get(&t->off, max_buckets + 1)) || (rc = sc.get(&t->rec, max_pts)))
    return rc;
  if (p->strategy == PCV_XRAY_HEIGHT_STDDEV && (rc = sc.get(&t->recz, max_pts))) return rc;
  if (binned && (rc = sc.get(&t->recb, max_pts))) return rc;
  if (bin_column && (rc = sc.get(&t->columns, std::max<size_t>(pl.columns.size(), 1)))) return rc;
  if (p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY && (rc = sc.get(&t->neg, nc))) return rc;
  t->h_tiles.resize(nc);
  for (uint64_t c = 0; c < nc; ++c) {
    double mn[3], mx[3];
    tile_box(x->geo, x->created[c], mn, mx);
    for (int a = 0; a < 3; ++a) {
      t->h_tiles[c].min[a] = mn[a];
      t->h_tiles[c].diag[a] = mx[a] - mn[a];  // Aabb::diag
    }
  }
  xray_value_table(t->h_table);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->cos, pl.created_of_shape.data(), 4 * (size_t)S, hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->tiles, t->h_tiles.data(), sizeof(XrayTileDev) * nc, hipMemcpyHostToDevice, ctx->stream));
  if (!pl.trees.empty())
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->trees, pl.trees.data(), sizeof(XrayTreeChunks) * pl.trees.size(), hipMemcpyHostToDevice, ctx->stream));
  if (t->columns && !pl.columns.empty())
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->columns, pl.columns.data(), sizeof(XrayBinColumn) * pl.columns.size(), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->table, t->h_table, sizeof(t->h_table), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemsetAsync(t->drawn, 0, 8 * nc, ctx->stream));
  if (t->neg) PCV_HIP_CHECK(ctx, hipMemsetAsync(t->neg, 0, 8 * nc, ctx->stream));
  return PCV_OK;
}

// step 4: per tile group count, scan, scatter and accumulate, then the per-tile counters
int xray_raster_groups(pcv_ctx* ctx, const pcv_xray_params* p, const pcv_xray_coloring* col, bool binned, bool s2, pcv_xray* x,
                       const XrayPlan& pl, uint32_t nbx, XrayTables& t) {
  const bool cwi = p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY;
  const uint32_t W = x->W, nblocks = nbx * nbx;
  const uint64_t nc = x->created.size();
  XrayBinArgs ba{};
  ba.created_of_shape = t.cos;
  ba.tiles = t.tiles;
  ba.W = W;
  ba.nbx = nbx;
  ba.nblocks = nblocks;
  ba.strategy = p->strategy;
  ba.has_iso = p->has_query_from_global ? 1 : 0;
  for (int i = 0; i < 7; ++i) ba.iso[i] = p->has_query_from_global ? p->query_from_global[i] : 0.0;
  ba.binned = binned ? 1 : 0;
  ba.bin_size = binned ? col->bin_size : 1.0;
  ba.negative = t.neg;
  XrayAccArgs aa{};
  aa.rec = t.rec;
  aa.recz = t.recz;
  aa.offsets = t.off;
  aa.image = x->d_images;
  aa.drawn = t.drawn;
  aa.W = W;
  aa.nbx = nbx;
  aa.nblocks = nblocks;
  aa.bg = x->bg;
  aa.colormap = p->colormap;
  aa.max_stddev = p->max_stddev;
  aa.strategy = p->strategy;
  aa.min_intensity = cwi ? col->min_intensity : 0.0f;
  aa.max_intensity = cwi ? col->max_intensity : 0.0f;
  // the sorted accumulation's LDS bucket limit (records, a power of two); the experiment build can lower it so that
  // small buckets take the global path
  uint32_t sort_cap = binned ? kSortCapBinned : kSortCapPlain;
  if (pcv_switches().xray_sort_lds_records) {
    const uint64_t v = std::min<uint64_t>(std::max<uint64_t>(2, pcv_switches().xray_sort_lds_records), sort_cap);
    sort_cap = 2;
    while ((uint64_t)sort_cap * 2 <= v) sort_cap *= 2;
  }
  // accumulation: as many workgroups as are resident at once, striding over the group's buckets (the experiment build
  // can lower the grid, to test the stride with few tiles)
  const XrayAccum acc = xray_accum_of(p->strategy, binned);
  int cus = 0, per_cu = 0;
  PCV_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, acc.kernel, (int)acc.threads, 0));
  uint64_t accum_grid = (uint64_t)std::max(cus, 1) * (uint64_t)std::max(per_cu, 1);
  if (pcv_switches().xray_accum_grid) accum_grid = pcv_switches().xray_accum_grid;
  for (size_t gi = 0; gi + 1 < pl.group_first.size(); ++gi) {
    const uint64_t f = pl.group_first[gi], l = pl.group_first[gi + 1];  // created tiles [f, l)
    ba.trees = t.trees + pl.tree_first[gi];
    ba.columns = t.columns ? t.columns + pl.tree_first[gi] : nullptr;
    ba.ntrees = (uint32_t)(pl.tree_first[gi + 1] - pl.tree_first[gi]);
    ba.nchunks = pl.group_chunks[gi];
    ba.created0 = (uint32_t)f;
    aa.created0 = (uint32_t)f;
    const uint64_t nb = (l - f) * nblocks;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((ba.nchunks + 3) / 4, 1u << 16));
    PCV_HIP_CHECK(ctx, hipMemsetAsync(t.counts, 0, 4 * nb, ctx->stream));
    {
      PcvProf prof(ctx, PCV_K_XRAY_BIN);
      hipLaunchKernelGGL((s2 ? xray_bin_kernel<false, true> : xray_bin_kernel<false, false>), dim3(grid), dim3(256), 0, ctx->stream, ba,
                         t.counts, (const uint64_t*)nullptr, (uint64_t*)nullptr, (double*)nullptr, (int64_t*)nullptr);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    {
      PcvProf prof(ctx, PCV_K_QUERY_BATCH_SCAN);
      if (int rc = pcv_batch_scan(ctx, t.sc, t.counts, nb, t.off)) return rc;
    }
    PCV_HIP_CHECK(ctx, hipMemsetAsync(t.counts, 0, 4 * nb, ctx->stream));
    {
      PcvProf prof(ctx, PCV_K_XRAY_SCATTER);
      XrayBinArgs bs = ba;
      bs.negative = nullptr;  // counted once, in the count pass
      hipLaunchKernelGGL((t.columns ? xray_bin_kernel<true, true, true> : s2 ? xray_bin_kernel<true, true> : xray_bin_kernel<true, false>),
                         dim3(grid), dim3(256), 0, ctx->stream, bs, t.counts, (const uint64_t*)t.off, t.rec, t.recz, t.recb);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    aa.nbuckets = (uint32_t)nb;
    {
      PcvProf prof(ctx, acc.prof_id);
      acc.launch((uint32_t)std::min<uint64_t>(nb, accum_grid), ctx->stream, aa, t.rec, t.recb, sort_cap, t.table);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(x->drawn.data(), t.drawn, 8 * nc, hipMemcpyDeviceToHost, ctx->stream));
  if (t.neg) PCV_HIP_CHECK(ctx, hipMemcpyAsync(x->negative.data(), t.neg, 8 * nc, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the scratch and the batches are released on return
  return PCV_OK;
}

int xray_run(pcv_ctx* ctx, const XrayClouds& clouds, const pcv_xray_params* p, const pcv_xray_coloring* col, pcv_xray* x) {
  const bool binned = coloring_binned(p, col);
  // the bins of an S2 run may come from a column of the clouds instead of the intensity (pcv_xray_run_s2_ex)
  const bool bin_column = binned && clouds.attrs && !clouds.attrs->bin_extra.empty();
  const bool reads_intensity = p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY || (binned && !bin_column);
  char err[256] = {0};
  double bmin[3], bmax[3];
  if (clouds.s2) union_box(clouds.s2, clouds.K, bmin, bmax);
  else union_box(clouds.trees, clouds.K, bmin, bmax);
  int rc = leaf_geometry(p->tile_size_px, p->pixel_size_m, bmin, bmax, p->has_query_from_global ? p->query_from_global : nullptr,
                         p->root_level, p->root_index, true, &x->geo, err, sizeof(err));
  if (rc) return ctx->fail(rc, err);
  const uint32_t W = p->tile_size_px, nbx = (W + kBlk - 1) / kBlk;
  x->W = W;
  x->root_level = p->root_level;
  x->root_index = p->root_index;
  x->bg = p->background == PCV_XRAY_BG_TRANSPARENT ? 0x00ffffffu : 0xffffffffu;  // TRANSPARENT / WHITE .to_u8()
  XrayBatches batches;
  if ((rc = xray_query_tiles(ctx, clouds, p, x->geo, reads_intensity, &batches))) return rc;
  XrayPlan pl;
  xray_created_tiles(batches.src, (uint32_t)x->geo.index.size(), x, &pl);
  const uint64_t nc = x->created.size();
  if (nc == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if ((rc = xray_plan_tiles(ctx, p, col, batches.src, x, &pl))) return rc;
  if ((rc = ctx->dev_alloc((void**)&x->d_images, 4ull * W * W * nc))) return rc;
  XrayTables t(ctx);
  if ((rc = xray_upload_tables(ctx, p, binned, bin_column, x, pl, nbx * nbx, &t))) return rc;
  return xray_raster_groups(ctx, p, col, binned, clouds.s2 != nullptr, x, pl, nbx, t);
}

}  // namespace

// the object of a checked run, or nothing (a failed run frees what it allocated)
static int xray_new(pcv_ctx* ctx, const XrayClouds& clouds, const pcv_xray_params* p, const pcv_xray_coloring* col, pcv_xray** out) {
  pcv_xray* x = new pcv_xray();
  x->ctx = ctx;
  const int rc = xray_run(ctx, clouds, p, col, x);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    pcv_xray_free(x);
    return rc;
  }
  ctx->prof_resolve();
  *out = x;
  return PCV_OK;
}

// whether the run reads intensity beyond a filter: colored_with_intensity, or binning where the strategy uses it
static bool coloring_needs_intensity(const pcv_xray_params* p, const pcv_xray_coloring* col) {
  return p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY ||
         (col && col->binning_attribute && p->strategy == PCV_XRAY_COLORED);
}

extern "C" int pcv_xray_check_params_ex(const pcv_xray_params* p, const pcv_xray_coloring* col, int tree_has_intensity, char* err,
                                        uint64_t errcap) {
  if (!p) return fail_msg(err, errcap, "null argument");
  if (p->strategy > PCV_XRAY_COLORED_WITH_INTENSITY) return fail_msg(err, errcap, "xray: unknown strategy");
  if (p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY && !col)
    return fail_msg(err, errcap, "xray: colored_with_intensity needs a pcv_xray_coloring (min_intensity, max_intensity)");
  if (col && col->binning_attribute) {
    // BinnedColoringStrategy::bins reads a 1-d attribute (match_1d_attr_data panics on U8Vec3, src/attributes.rs:128);
    // an octree carries only color and intensity
    if (std::strcmp(col->binning_attribute, "intensity") != 0)
      return fail_msg(err, errcap, std::string("xray: binning on attribute '") + col->binning_attribute + "': only intensity can be binned on");
  }
  if (coloring_needs_intensity(p, col) && !tree_has_intensity)
    return fail_msg(err, errcap, p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY ? "xray: octree has no intensity attribute to color by"
                                                                                : "xray: octree has no intensity attribute to bin on");
  if (p->strategy == PCV_XRAY_HEIGHT_STDDEV) {
    if (!(p->max_stddev > 0.0f) || !std::isfinite(p->max_stddev)) return fail_msg(err, errcap, "xray: height_stddev needs 0 < max_stddev < inf");
    if (p->colormap > PCV_XRAY_PURPLISH) return fail_msg(err, errcap, "xray: unknown colormap");
  }
  if (p->background > PCV_XRAY_BG_TRANSPARENT) return fail_msg(err, errcap, "xray: unknown background");
  if (p->interval_attribute) {
    if (std::strcmp(p->interval_attribute, "intensity") != 0)
      return fail_msg(err, errcap, std::string("xray: filter on attribute '") + p->interval_attribute + "': only intensity is supported");
    if (!tree_has_intensity) return fail_msg(err, errcap, "xray: octree has no intensity attribute to filter on");
  }
  return PCV_OK;
}

extern "C" int pcv_xray_check_params(const pcv_xray_params* p, int tree_has_intensity, char* err, uint64_t errcap) {
  if (p && p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY)
    return fail_msg(err, errcap, "xray: colored_with_intensity needs min / max intensity: use pcv_xray_run_ex (pcv_xray_check_params_ex)");
  return pcv_xray_check_params_ex(p, nullptr, tree_has_intensity, err, errcap);
}

extern "C" int pcv_xray_run(pcv_ctx* ctx, pcv_octree* tree, const pcv_xray_params* p, pcv_xray** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!tree || !p || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  char err[256] = {0};
  const int vrc = pcv_xray_check_params(p, tree->has_intensity ? 1 : 0, err, sizeof(err));
  if (vrc) return ctx->fail(vrc, err);
  XrayClouds clouds;
  clouds.trees = &tree;
  clouds.K = 1;
  return xray_new(ctx, clouds, p, nullptr, out);
}

// pcv_xray_run_many (ex = false: colored_with_intensity refused, coloring ignored), pcv_xray_run_ex and pcv_xray_run_s2:
// `what` names the kind of cloud in messages; a cloud without a context of its own is a host-only S2 cloud
template <class Cloud>
static int xray_run_checked(pcv_ctx* ctx, Cloud* const* trees, uint32_t num_trees, const char* what, const pcv_xray_params* p,
                            const pcv_xray_coloring* col, bool ex, pcv_xray** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!p || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  // PointCloudClientBuilder::build (point_cloud_client/src/lib.rs:92-95)
  if (num_trees == 0) return ctx->fail(PCV_E_INVALID, "xray: No locations specified for point cloud client.");
  if (!trees) return ctx->fail(PCV_E_INVALID, "null argument");
  if (num_trees > PCV_XRAY_MAX_TREES)
    return ctx->fail(PCV_E_INVALID, "xray: " + std::to_string(num_trees) + " " + what + "s, more than PCV_XRAY_MAX_TREES (" +
                                        std::to_string(PCV_XRAY_MAX_TREES) + ")");
  char err[256] = {0};
  int vrc = ex ? pcv_xray_check_params_ex(p, col, 1, err, sizeof(err)) : pcv_xray_check_params(p, 1, err, sizeof(err));
  if (vrc) return ctx->fail(vrc, err);
  for (uint32_t t = 0; t < num_trees; ++t) {
    const std::string which = std::string("xray: ") + what + " " + std::to_string(t);
    if (!trees[t]) return ctx->fail(PCV_E_INVALID, which + " is null");
    if (!trees[t]->ctx) return ctx->fail(PCV_E_INVALID, which + " was opened without a context and has no device");
    if (trees[t]->ctx != ctx) return ctx->fail(PCV_E_INVALID, which + " belongs to another context");
    if (p->interval_attribute && !trees[t]->has_intensity)
      return ctx->fail(PCV_E_INVALID, which + " has no intensity attribute to filter on");
    if (ex && coloring_needs_intensity(p, col) && !trees[t]->has_intensity)
      return ctx->fail(PCV_E_INVALID, which + " has no intensity attribute to color or bin by");
  }
  XrayClouds clouds;
  if constexpr (std::is_same<Cloud, pcv_s2_cloud>::value) clouds.s2 = trees;
  else clouds.trees = trees;
  clouds.K = num_trees;
  return xray_new(ctx, clouds, p, ex ? col : nullptr, out);
}

extern "C" int pcv_xray_run_many(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t num_trees, const pcv_xray_params* p, pcv_xray** out) {
  return xray_run_checked(ctx, trees, num_trees, "octree", p, nullptr, false, out);
}

extern "C" int pcv_xray_run_ex(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t num_trees, const pcv_xray_params* p,
                               const pcv_xray_coloring* coloring, pcv_xray** out) {
  if (!coloring) return xray_run_checked(ctx, trees, num_trees, "octree", p, nullptr, false, out);
  return xray_run_checked(ctx, trees, num_trees, "octree", p, coloring, true, out);
}

// build_xray_quadtree's leaf level over S2 cell clouds (PointClouds::S2Cells, point_cloud_client/src/lib.rs:120-131): the
// same run with every tile's points from pcv_s2_query_run's machinery
extern "C" int pcv_xray_run_s2(pcv_ctx* ctx, pcv_s2_cloud* const* clouds, uint32_t num_clouds, const pcv_xray_params* p,
                               const pcv_xray_coloring* coloring, pcv_xray** out) {
  return xray_run_checked(ctx, clouds, num_clouds, "S2 cloud", p, coloring, coloring != nullptr, out);
}

// ---- pcv_xray_run_s2_ex: filters (xray/src/build_quadtree.rs:94-101, FilteredIterator over filter_intervals) and binning
// (:102-107, BinnedColoringStrategy::bins) on any scalar attribute of the clouds ---------------------------------------------
namespace {

// the attributes of one cloud as the checks read them: its extras (name, data type) and whether it has intensity
struct XrayCloudAttrs {
  const char* const* names;
  const int32_t* data_types;
  uint32_t count;
  bool has_intensity;
  int find(const char* name) const {
    for (uint32_t k = 0; k < count; ++k)
      if (names[k] && std::strcmp(names[k], name) == 0) return (int)k;
    return -1;
  }
};

bool binning_on_column(const pcv_xray_coloring* col) {
  return col && col->binning_attribute && std::strcmp(col->binning_attribute, "intensity") != 0;
}

// every check of pcv_xray_run_s2_ex that needs no device; *out (nullable): per cloud the extras the run reads
int check_attrs(const pcv_xray_params* p, const pcv_xray_coloring* col, const pcv_xray_filter* filters, uint32_t num_filters,
                const std::vector<XrayCloudAttrs>& clouds, XrayS2Attrs* out, char* err, uint64_t errcap) {
  if (!p) return fail_msg(err, errcap, "null argument");
  if (clouds.empty()) return fail_msg(err, errcap, "xray: No locations specified for point cloud client.");
  // the checks of pcv_xray_run_s2, which knows no binning name but intensity: the name is checked against the clouds below
  pcv_xray_coloring known{};
  if (col) {
    known = *col;
    if (binning_on_column(col)) known.binning_attribute = nullptr;
  }
  if (int rc = pcv_xray_check_params_ex(p, col ? &known : nullptr, 1, err, errcap)) return rc;
  if (col && col->binning_attribute && col->binning_attribute[0] == '\0') return fail_msg(err, errcap, "xray: the binning attribute has an empty name");
  if (num_filters && !filters) return fail_msg(err, errcap, "null argument");
  for (uint32_t k = 0; k < num_filters; ++k) {
    if (!filters[k].attribute) return fail_msg(err, errcap, "xray: filter " + std::to_string(k) + " has no attribute name");
    const std::string name(filters[k].attribute);
    bool twice = p->interval_attribute && name == "intensity";  // interval_attribute is a filter on intensity
    for (uint32_t j = 0; j < k; ++j) twice = twice || name == filters[j].attribute;
    if (twice) return fail_msg(err, errcap, "xray: two filters on attribute '" + name + "'");
  }
  const bool binned = coloring_binned(p, col), column = binning_on_column(col);
  if (out) {
    *out = XrayS2Attrs{};
    out->filters.resize(clouds.size());
    if (p->interval_attribute) out->has_interval = true, out->interval[0] = p->interval[0], out->interval[1] = p->interval[1];
  }
  for (size_t t = 0; t < clouds.size(); ++t) {
    const XrayCloudAttrs& c = clouds[t];
    const std::string which = "S2 cloud " + std::to_string(t);
    if (p->interval_attribute && !c.has_intensity) return fail_msg(err, errcap, "xray: " + which + " has no intensity attribute to filter on");
    if (coloring_needs_intensity(p, col) && !(column && p->strategy == PCV_XRAY_COLORED) && !c.has_intensity)
      return fail_msg(err, errcap, "xray: " + which + " has no intensity attribute to color or bin by");
    for (uint32_t k = 0; k < num_filters; ++k) {
      const pcv_xray_filter& f = filters[k];
      const std::string name(f.attribute);
      if (name == "intensity") {
        if (!c.has_intensity) return fail_msg(err, errcap, "xray: " + which + " has no intensity attribute to filter on");
        if (out) out->has_interval = true, out->interval[0] = f.lo, out->interval[1] = f.hi;
        continue;
      }
      const int e = name == "color" ? -1 : c.find(f.attribute);
      if (name == "color" || (e >= 0 && !s2attr::is_scalar(c.data_types[e])))
        return fail_msg(err, errcap, "xray: a filter takes a scalar attribute; '" + name + "' of " + which + " is a vector attribute");
      if (e < 0) return fail_msg(err, errcap, "xray: Data type for attribute '" + name + "' not found. (" + which + ")");  // lib.rs:94
      if (out) out->filters[t].push_back(PcvS2ExtraFilter{kPcvS2EveryLocation, e, f.lo, f.hi});
    }
    if (column) {  // the name is checked whatever the strategy; the column is read by colored and colored_with_intensity
      const std::string name(col->binning_attribute);
      const int e = name == "color" ? -1 : c.find(col->binning_attribute);
      if (name == "color" || (e >= 0 && !s2attr::is_scalar(c.data_types[e])))
        return fail_msg(err, errcap, "xray: binning takes a scalar attribute; '" + name + "' of " + which + " is a vector attribute");
      if (e < 0)  // generation.rs:146
        return fail_msg(err, errcap, "xray: Binning attribute needs to be available in points batch. (attribute '" + name + "', " + which + ")");
      if (out && binned) out->bin_extra.push_back(e);
    }
  }
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_xray_check_attrs_host(const pcv_xray_params* p, const pcv_xray_coloring* col, const pcv_xray_filter* filters,
                                         uint32_t num_filters, uint32_t num_clouds, const uint32_t* extras_first, const char* const* names,
                                         const int32_t* data_types, const uint8_t* has_intensity, char* err, uint64_t errcap) {
  if (num_clouds && (!extras_first || !has_intensity)) return fail_msg(err, errcap, "null argument");
  if (num_clouds && extras_first[num_clouds] && (!names || !data_types)) return fail_msg(err, errcap, "null argument");
  std::vector<XrayCloudAttrs> clouds(num_clouds);
  for (uint32_t t = 0; t < num_clouds; ++t) {
    if (extras_first[t + 1] < extras_first[t]) return fail_msg(err, errcap, "xray: extras_first must not descend");
    clouds[t] = XrayCloudAttrs{names ? names + extras_first[t] : nullptr, data_types ? data_types + extras_first[t] : nullptr,
                               extras_first[t + 1] - extras_first[t], has_intensity[t] != 0};
  }
  return check_attrs(p, col, filters, num_filters, clouds, nullptr, err, errcap);
}

extern "C" int pcv_xray_run_s2_ex(pcv_ctx* ctx, pcv_s2_cloud* const* clouds, uint32_t num_clouds, const pcv_xray_params* p,
                                  const pcv_xray_coloring* coloring, const pcv_xray_filter* filters, uint32_t num_filters, pcv_xray** out) {
  if (num_filters == 0 && !binning_on_column(coloring)) return pcv_xray_run_s2(ctx, clouds, num_clouds, p, coloring, out);
  if (!ctx) return PCV_E_INVALID;
  if (!p || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (num_clouds == 0) return ctx->fail(PCV_E_INVALID, "xray: No locations specified for point cloud client.");
  if (!clouds) return ctx->fail(PCV_E_INVALID, "null argument");
  if (num_clouds > PCV_XRAY_MAX_TREES)
    return ctx->fail(PCV_E_INVALID, "xray: " + std::to_string(num_clouds) + " S2 clouds, more than PCV_XRAY_MAX_TREES (" +
                                        std::to_string(PCV_XRAY_MAX_TREES) + ")");
  std::vector<XrayCloudAttrs> attrs(num_clouds);
  std::vector<std::vector<const char*>> names(num_clouds);
  std::vector<std::vector<int32_t>> types(num_clouds);
  for (uint32_t t = 0; t < num_clouds; ++t) {
    const std::string which = "xray: S2 cloud " + std::to_string(t);
    if (!clouds[t]) return ctx->fail(PCV_E_INVALID, which + " is null");
    if (!clouds[t]->ctx) return ctx->fail(PCV_E_INVALID, which + " was opened without a context and has no device");
    if (clouds[t]->ctx != ctx) return ctx->fail(PCV_E_INVALID, which + " belongs to another context");
    for (const PcvS2Extra& e : clouds[t]->extras) names[t].push_back(e.name.c_str()), types[t].push_back(e.data_type);
    attrs[t] = XrayCloudAttrs{names[t].data(), types[t].data(), (uint32_t)names[t].size(), clouds[t]->has_intensity};
  }
  char err[320] = {0};
  XrayS2Attrs reads;
  if (int rc = check_attrs(p, coloring, filters, num_filters, attrs, &reads, err, sizeof(err))) return ctx->fail(rc, err);
  // exactly the columns the run reads, resident before any raster work: a cloud opened from a directory reads an extra's
  // files on first use, and a damaged one is PCV_E_IO naming the file
  for (uint32_t t = 0; t < num_clouds; ++t) {
    for (const PcvS2ExtraFilter& f : reads.filters[t])
      if (int rc = pcv_s2_extra_resident(clouds[t], (size_t)f.extra)) return rc;
    if (!reads.bin_extra.empty())
      if (int rc = pcv_s2_extra_resident(clouds[t], (size_t)reads.bin_extra[t])) return rc;
  }
  XrayClouds cl;
  cl.s2 = clouds;
  cl.K = num_clouds;
  cl.attrs = &reads;
  return xray_new(ctx, cl, p, coloring, out);
}

extern "C" int pcv_xray_bins_host(int32_t data_type, uint64_t n, const void* data, double bin_size, int64_t* out) {
  if (s2attr::element_size(data_type) == 0) return pcv_host_fail(PCV_E_INVALID, "Attribute data type invalid");
  if (!s2attr::is_scalar(data_type)) return pcv_host_fail(PCV_E_INVALID, "binning takes a scalar attribute; a vector attribute has no bins");
  if (n && (!data || !out)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  s2attr::dispatch_scalar(data_type, [&](auto t) {
    using T = decltype(t);
    const uint8_t* src = (const uint8_t*)data;
    for (uint64_t i = 0; i < n; ++i) {
      T v;
      std::memcpy(&v, src + i * sizeof(T), sizeof(T));  // (the caller's buffer may stand at any byte)
      out[i] = s2attr::bin<T>(v, bin_size);
    }
  });
  return PCV_OK;
}

extern "C" int pcv_xray_negative(const pcv_xray* x, uint64_t* negative) {
  if (!x) return PCV_E_INVALID;
  if (x->kind != kXrayBuilt) return xray_not_built(x, "pcv_xray_negative");
  if (negative) std::memcpy(negative, x->negative.data(), 8 * x->negative.size());
  return PCV_OK;
}

extern "C" int pcv_xray_info(const pcv_xray* x, uint32_t* deepest_level, double rect[3], uint64_t* num_leaves, uint64_t* num_created) {
  if (!x) return PCV_E_INVALID;
  if (deepest_level) *deepest_level = x->geo.deepest_level;
  if (rect) std::memcpy(rect, x->geo.rect, sizeof(x->geo.rect));
  if (num_leaves) *num_leaves = x->geo.index.size();
  if (num_created) *num_created = x->created.size();
  return PCV_OK;
}

extern "C" int pcv_xray_tiles(const pcv_xray* x, uint64_t* leaf_index, uint64_t* created, uint64_t* kept, uint64_t* drawn) {
  if (!x) return PCV_E_INVALID;
  if (x->kind != kXrayBuilt) return xray_not_built(x, "pcv_xray_tiles");
  if (leaf_index) std::memcpy(leaf_index, x->geo.index.data(), 8 * x->geo.index.size());
  if (created) std::memcpy(created, x->created.data(), 8 * x->created.size());
  if (kept) std::memcpy(kept, x->kept.data(), 8 * x->kept.size());
  if (drawn) std::memcpy(drawn, x->drawn.data(), 8 * x->drawn.size());
  return PCV_OK;
}

extern "C" int pcv_xray_images(pcv_xray* x, uint64_t first, uint64_t count, uint64_t capacity, int mem, uint8_t* rgba) {
  if (!x) return PCV_E_INVALID;
  if (x->kind != kXrayBuilt) return xray_not_built(x, "pcv_xray_images");
  pcv_ctx* ctx = x->ctx;
  const uint64_t nc = x->created.size();
  if (first > nc || count > nc - first) return ctx->fail(PCV_E_INVALID, "xray: tile range past the end");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  const uint64_t tile_bytes = 4ull * x->W * x->W;
  if (count * tile_bytes > capacity) return ctx->fail(PCV_E_INVALID, "xray: capacity below count x W x W x 4 bytes");
  if (count == 0) return PCV_OK;
  if (!rgba) return ctx->fail(PCV_E_INVALID, "null output");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(rgba, reinterpret_cast<const uint8_t*>(x->d_images) + first * tile_bytes, count * tile_bytes,
                                    mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_xray_nodes(const pcv_xray* x, uint64_t* num_nodes, uint64_t capacity, uint32_t* level, uint64_t* index) {
  if (!x) return PCV_E_INVALID;
  const uint64_t n = xray_num_nodes(x);
  if (num_nodes) *num_nodes = n;
  for (uint64_t i = 0; i < std::min(n, capacity); ++i) {
    const XrayNodeId id = xray_node_id(x, i);
    if (level) level[i] = id.level;
    if (index) index[i] = id.index;
  }
  return PCV_OK;
}

extern "C" uint32_t pcv_xray_tile_size(const pcv_xray* x) { return x ? x->W : 0; }
