// pcv_xray.hip — xray's build_xray_quadtree (xray/src/generation.rs:557-616) on the device: the leaf level rasterised
// straight from batched point queries (pcv_query.hip), one per octree of the run, without materialising their points, then
// every parent level (second half of the file) and the quadtree directory.
//
//   host   leaf geometry   get_bounding_box :550 (Aabb::transform, src/geometry/aabb.rs:58-66),
//                          find_quadtree_bounding_rect_and_levels :515, Node::from_node_id_and_root_bounding_rect and
//                          Node::get_child (quadtree/src/lib.rs:59-97), get_nodes_at_level :534 (DFS pop order)
//   host   one query per leaf tile   xray_from_points :464 — Aabb(tile) or Obb::from(tile).transformed(global_from_query)
//                          (src/geometry/obb.rs:20-47), intensity interval on every shape, through pcv_query_batch_run
//   K_xb   xray_bin        per kept point: decode (the batch's own decode), query_from_global (:493-497), discretise
//                          (:119-123); count per (tile, 32 x 32 pixel block), aggregated per wave before the atomic
//   scan   bucket counts -> u64 offsets (pcv_batch_scan)
//   K_xs   xray_scatter    the same walk again, writing one 8-byte record per drawable point into its bucket (+ z as f64
//                          for height_stddev)
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
#include <unordered_map>
#include <vector>

#include "pcv_query_dev.h"
#include "pcv_switches.h"
#include "pcv_xray_png.h"

namespace {

constexpr uint32_t kBlk = 32;  // pixel block edge: one accumulation workgroup per (tile, 32 x 32 pixels)
constexpr uint32_t kBlkPx = kBlk * kBlk;
constexpr uint32_t kZWords = 33;  // 1 056 bits per pixel: z buckets 0 ..= 1024 (NUM_Z_BUCKETS = 1024, :31)
constexpr uint32_t kZMax = kZWords * 32 - 1;
constexpr uint32_t kMaxTilePx = 1u << 15;
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
// Rust `f64 as i64`: truncation, saturating; NaN -> 0 (the bin of generation.rs:150)
__host__ __device__ inline int64_t rust_i64(double v) {
  if (v != v) return 0;
  if (v >= 9223372036854775808.0) return INT64_MAX;
  if (v < -9223372036854775808.0) return INT64_MIN;
  return (int64_t)v;
}

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
  int32_t binned;                   // colored / colored_with_intensity with binning on intensity
  double bin_size;
  unsigned long long* negative;     // colored_with_intensity: kept points with intensity < 0 per created tile (count pass)
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
__device__ __forceinline__ XrayPoint xray_point(const XrayBinArgs& a, const uint8_t* rgb, const float* inten, const ChunkDesc& d,
                                                const PointsView& v, const XrayTileDev& t, uint32_t bbase, uint32_t q, bool kept) {
  XrayPoint o{false, false, 0u, 0ull, 0.0, 0};
  if (!kept) return o;
  float in = 0.0f;
  if (inten) {
    in = inten[d.attr_index + q];
    // the `< 0` check runs on every kept point, inside the image or not (:108-127, :248); such points are not drawn
    if (a.strategy == PCV_XRAY_COLORED_WITH_INTENSITY && in < 0.0f) {
      o.neg = true;
      return o;
    }
    if (a.binned) o.bin = rust_i64((double)in / a.bin_size);  // BinnedColoringStrategy::bins (:138-157)
  }
  V3d p = load_point(v, q);
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
    const uint8_t* c = rgb + 3 * (d.attr_index + q);
    rec |= ((uint64_t)c[0] | (uint64_t)c[1] << 8 | (uint64_t)c[2] << 16) << 32;
  } else if (a.strategy == PCV_XRAY_COLORED_WITH_INTENSITY) {
    rec |= (uint64_t)__float_as_uint(in) << 32;
  }
  o.rec = rec;
  o.z = p.z;
  return o;
}

// a wave per chunk of the group, whose chunks are those of all its octrees one after another. COUNT: one counter add per
// distinct bucket of the 64 points (wave match on the bucket); SCATTER: the same adds reserve each point's slot in its
// bucket. A wave's chunk index only grows, so its octree is found by a wave-uniform search forward from the last one.
template <bool SCATTER>
__global__ __launch_bounds__(256) void xray_bin_kernel(XrayBinArgs a, uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets,
                                                       uint64_t* __restrict__ rec, double* __restrict__ recz,
                                                       int64_t* __restrict__ recb) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  uint32_t k = 0;
  uint64_t kend = a.ntrees > 1 ? a.trees[1].first : a.nchunks;  // first chunk past octree k
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
    const ChunkDesc d = tr.desc[tr.c0 + (gi - tr.first)];
    const int32_t created = a.created_of_shape[d.enc >> 8];
    if (created < 0) continue;  // wave-uniform: no octree's query kept anything for this tile
    const XrayTileDev t = a.tiles[created];
    const uint32_t bbase = ((uint32_t)created - a.created0) * a.nblocks;
    PointsView v{};
    v.encoded = (const uint8_t*)(tr.xyz + d.src);
    v.enc = d.enc & 15u;
    v.cube_min[0] = d.cube_min[0];
    v.cube_min[1] = d.cube_min[1];
    v.cube_min[2] = d.cube_min[2];
    v.cube_edge = d.cube_edge;
    const PCV_GLOBAL uint8_t* kp = tr.keep + d.keep_off;
    const uint8_t* rgb = (const uint8_t*)tr.rgb;
    const float* inten = (const float*)tr.inten;
    for (uint32_t q0 = 0; q0 < d.cnt; q0 += 64) {
      const uint32_t q = q0 + lane;
      const XrayPoint pt = xray_point(a, rgb, inten, d, v, t, bbase, q, q < d.cnt && kp[q]);
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
struct LeafGeometry {
  double rect[3];  // bounding rect: min x, min y, edge
  uint32_t deepest_level;
  double bbox_min[3], bbox_max[3];  // get_bounding_box
  std::vector<uint64_t> index;      // leaf node indices at deepest_level, get_nodes_at_level order
  std::vector<double> rect_min;     // 2 per leaf
  double leaf_edge;
};

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

// Every live pcv_xray by address with a serial number of its own: a merged quadtree refers to its parts, and asks here
// whether a part is still the object it was given before it touches it (pcv_xray_merge)
namespace {
std::mutex g_xray_mu;
std::unordered_map<const pcv_xray*, uint64_t> g_xray_live;
uint64_t g_xray_serial = 0;
}  // namespace

enum XrayKind : uint32_t { kXrayBuilt = 0, kXrayOpened = 1, kXrayMerged = 2 };

struct XrayPartRef {  // one part of a merged quadtree: its nodes are [first, first + count) of the merged node list
  pcv_xray* part;
  uint64_t serial, first, count;
};

struct pcv_xray {
  pcv_xray() {
    std::lock_guard<std::mutex> g(g_xray_mu);
    g_xray_live[this] = serial = ++g_xray_serial;
  }
  ~pcv_xray() {
    std::lock_guard<std::mutex> g(g_xray_mu);
    g_xray_live.erase(this);
  }
  uint64_t serial = 0;
  XrayKind kind = kXrayBuilt;
  // opened (pcv_xray_open_dir) and merged (pcv_xray_merge) quadtrees: the node list itself; of `geo` only deepest_level
  // and rect are set (the meta's bounding rect), geo.index / created list the nodes at deepest_level
  std::vector<uint32_t> node_level;
  std::vector<uint64_t> node_index;
  uint64_t root_count = 0;   // nodes at the minimum level (a merge needs exactly one, or no node at all)
  std::string dir;           // opened: the directory the PNGs are read from
  std::vector<XrayPartRef> parts;  // merged; the new levels follow the parts' nodes and live in d_parents
  pcv_ctx* ctx = nullptr;    // null: opened without a context (host only)
  uint32_t W = 0;
  LeafGeometry geo;
  uint32_t root_level = 0;
  uint64_t root_index = 0;
  uint32_t bg = 0;                // tile_background_color.to_u8(), packed RGBA8
  std::vector<uint64_t> created;  // positions in the leaf list
  std::vector<uint64_t> kept, drawn;
  std::vector<uint64_t> negative;  // colored_with_intensity: kept points with intensity < 0 per created tile
  uint32_t* d_images = nullptr;
  // parent levels (pcv_xray_build_parents): the node list after the created leaves, deepest - 1 up to root_level, each
  // level in ascending index; level_first[k] is the first parent of level deepest - 1 - k in that list
  bool parents_built = false;
  std::vector<uint32_t> parent_level;
  std::vector<uint64_t> parent_index;
  std::vector<uint64_t> level_first;
  uint32_t* d_parents = nullptr;
};

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

// a failure on a handle that may have no context (opened host only): the message goes where the caller can read it
static int xray_fail(const pcv_xray* x, int code, const std::string& msg) {
  return x->ctx ? x->ctx->fail(code, msg) : pcv_host_fail(code, msg);
}
static int xray_not_built(const pcv_xray* x, const char* what) {
  return xray_fail(x, PCV_E_INVALID, std::string("xray: ") + what + " needs a quadtree built by pcv_xray_run, not an opened or merged one");
}

// PointCloudClientBuilder::build's bounding box (point_cloud_client/src/lib.rs:101-125): the first octree's meta box, grown
// by every octree's min and then its max in list order (Aabb::grow, aabb.rs:41-44: Point3::inf / sup per component)
static void union_box(pcv_octree* const* trees, uint32_t K, double lo[3], double hi[3]) {
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

// the leaf level over K octrees (K = 1: pcv_xray_run): one shape list, one query batch per octree, every raster pass one
// launch per tile group over the chunks of all K batches
static int xray_run(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t K, const pcv_xray_params* p, const pcv_xray_coloring* col,
                    pcv_xray* x) {
  const bool filter = p->interval_attribute != nullptr;
  // colored_with_intensity, and colored with binning, take the sorted accumulation (xray_sorted); binning is ignored by
  // xray and height_stddev (attributes() :133)
  const bool cwi = p->strategy == PCV_XRAY_COLORED_WITH_INTENSITY;
  const bool binned = coloring_binned(p, col);
  const bool sorted = cwi || binned;
  char err[256] = {0};
  double bmin[3], bmax[3];
  union_box(trees, K, bmin, bmax);
  int rc = leaf_geometry(p->tile_size_px, p->pixel_size_m, bmin, bmax, p->has_query_from_global ? p->query_from_global : nullptr,
                         p->root_level, p->root_index, true, &x->geo, err, sizeof(err));
  if (rc) return ctx->fail(rc, err);
  const LeafGeometry& g = x->geo;
  const uint32_t S = (uint32_t)g.index.size(), W = p->tile_size_px;
  x->W = W;
  x->root_level = p->root_level;
  x->root_index = p->root_index;
  x->bg = p->background == PCV_XRAY_BG_TRANSPARENT ? 0x00ffffffu : 0xffffffffu;  // TRANSPARENT / WHITE .to_u8()
  // one shape per leaf tile (xray_from_points :470-476)
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
      ivals[2 * (size_t)i] = p->interval[0];
      ivals[2 * (size_t)i + 1] = p->interval[1];
    }
  }
  pcv_shapes* sh = nullptr;
  if ((rc = pcv_shapes_create(ctx, shapes.data(), S, &sh))) return rc;
  // the same shapes through every octree (try_for_each_batch's jobs, src/iterator.rs:262-270); all K batches stay alive
  // until the raster passes are done
  struct BatchGuard {
    std::vector<pcv_query_batch*> b;
    ~BatchGuard() {
      for (pcv_query_batch* q : b) pcv_query_batch_free(q);
    }
  } guard;
  guard.b.reserve(K);
  for (uint32_t t = 0; t < K && rc == PCV_OK; ++t) {
    pcv_query_batch* b = nullptr;
    rc = pcv_query_batch_run(ctx, sh, trees[t], filter ? ivals.data() : nullptr, nullptr, &b);
    if (rc == PCV_OK) guard.b.push_back(b);
  }
  pcv_shapes_free(sh);
  if (rc) return rc;
  const std::vector<pcv_query_batch*>& batches = guard.b;
  // a tile is created iff the queries kept a point (PointStream::callback never delivers an empty batch,
  // iterator.rs:148-151); kept is the sum over the octrees
  std::vector<int32_t> created_of_shape(S, -1);
  for (uint32_t s = 0; s < S; ++s) {
    uint64_t k = 0;
    for (const pcv_query_batch* b : batches) k += b->seg_off[b->shape_first[s + 1]] - b->seg_off[b->shape_first[s]];
    if (k == 0) continue;
    created_of_shape[s] = (int32_t)x->created.size();
    x->created.push_back(s);
    x->kept.push_back(k);
  }
  const uint64_t nc = x->created.size();
  x->drawn.assign(nc, 0);
  x->negative.assign(nc, 0);
  if (nc == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint32_t nbx = (W + kBlk - 1) / kBlk, nblocks = nbx * nbx;
  const uint64_t img_px = (uint64_t)W * W;
  std::vector<uint64_t> group_first;
  uint64_t max_pts = 0, max_tiles = 0;
  {
    char m[256] = {0};
    if ((rc = plan_groups(x->kept.data(), nc, x->created.data(), W, p, col, group_first, &max_pts, &max_tiles, m, sizeof(m))))
      return ctx->fail(rc, m);
  }
  if ((rc = ctx->dev_alloc((void**)&x->d_images, 4 * img_px * nc))) return rc;
  // per group, the octrees that have chunks for its shapes, in list order, their chunk ranges end to end (u64 prefix)
  std::vector<XrayTreeChunks> h_trees;
  std::vector<size_t> tree_first(1, 0);
  std::vector<uint64_t> group_chunks;
  for (size_t gi = 0; gi + 1 < group_first.size(); ++gi) {
    const uint64_t s0 = x->created[group_first[gi]], s1 = x->created[group_first[gi + 1] - 1] + 1;
    uint64_t n = 0;
    for (uint32_t t = 0; t < K; ++t) {
      const pcv_query_batch* b = batches[t];
      const uint64_t c0 = b->seg_chunk[b->shape_first[s0]], c1 = b->seg_chunk[b->shape_first[s1]];
      if (c1 == c0) continue;
      XrayTreeChunks e{};
      e.desc = (decltype(e.desc))b->d_desc;
      e.keep = (decltype(e.keep))b->d_keep;
      e.xyz = (decltype(e.xyz))trees[t]->d_xyz;
      e.rgb = (decltype(e.rgb))trees[t]->d_rgb;
      e.inten = sorted ? (decltype(e.inten))trees[t]->d_int : nullptr;
      e.c0 = c0;
      e.first = n;
      h_trees.push_back(e);
      n += c1 - c0;
    }
    tree_first.push_back(h_trees.size());
    group_chunks.push_back(n);
  }
  PcvScratch sc(ctx);
  int32_t* d_cos;
  XrayTileDev* d_tiles;
  XrayTreeChunks* d_trees;
  uint8_t* d_table;
  unsigned long long* d_drawn;
  uint32_t* d_counts;
  uint64_t *d_off, *d_rec;
  double* d_recz = nullptr;
  int64_t* d_recb = nullptr;
  unsigned long long* d_neg = nullptr;
  const uint64_t max_buckets = max_tiles * nblocks;
  if ((rc = sc.get(&d_cos, S)) || (rc = sc.get(&d_tiles, nc)) || (rc = sc.get(&d_trees, std::max<size_t>(h_trees.size(), 1))) ||
      (rc = sc.get(&d_table, kZWords * 32 + 1)) || (rc = sc.get(&d_drawn, nc)) || (rc = sc.get(&d_counts, max_buckets)) ||
      (rc = sc.get(&d_off, max_buckets + 1)) || (rc = sc.get(&d_rec, std::max<uint64_t>(max_pts, 1))))
    return rc;
  if (p->strategy == PCV_XRAY_HEIGHT_STDDEV && (rc = sc.get(&d_recz, std::max<uint64_t>(max_pts, 1)))) return rc;
  if (binned && (rc = sc.get(&d_recb, std::max<uint64_t>(max_pts, 1)))) return rc;
  if (cwi && (rc = sc.get(&d_neg, nc))) return rc;
  std::vector<XrayTileDev> h_tiles(nc);
  for (uint64_t c = 0; c < nc; ++c) {
    double mn[3], mx[3];
    tile_box(g, x->created[c], mn, mx);
    for (int a = 0; a < 3; ++a) {
      h_tiles[c].min[a] = mn[a];
      h_tiles[c].diag[a] = mx[a] - mn[a];  // Aabb::diag
    }
  }
  uint8_t table[kZWords * 32 + 1];
  xray_value_table(table);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_cos, created_of_shape.data(), 4 * (size_t)S, hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_tiles, h_tiles.data(), sizeof(XrayTileDev) * nc, hipMemcpyHostToDevice, ctx->stream));
  if (!h_trees.empty())
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_trees, h_trees.data(), sizeof(XrayTreeChunks) * h_trees.size(), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_table, table, sizeof(table), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_drawn, 0, 8 * nc, ctx->stream));
  if (d_neg) PCV_HIP_CHECK(ctx, hipMemsetAsync(d_neg, 0, 8 * nc, ctx->stream));
  XrayBinArgs ba{};
  ba.created_of_shape = d_cos;
  ba.tiles = d_tiles;
  ba.W = W;
  ba.nbx = nbx;
  ba.nblocks = nblocks;
  ba.strategy = p->strategy;
  ba.has_iso = p->has_query_from_global ? 1 : 0;
  for (int i = 0; i < 7; ++i) ba.iso[i] = p->has_query_from_global ? p->query_from_global[i] : 0.0;
  ba.binned = binned ? 1 : 0;
  ba.bin_size = binned ? col->bin_size : 1.0;
  ba.negative = d_neg;
  XrayAccArgs aa{};
  aa.rec = d_rec;
  aa.recz = d_recz;
  aa.offsets = d_off;
  aa.image = x->d_images;
  aa.drawn = d_drawn;
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
  int cus = 0, per_cu = 0;
  PCV_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  if (binned)
    PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xray_sorted_kernel<true>, kSortThreads, 0));
  else if (sorted)
    PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xray_sorted_kernel<false>, kSortThreads, 0));
  else if (p->strategy == PCV_XRAY_XRAY)
    PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xray_accum_kernel<PCV_XRAY_XRAY, 1024>, 1024, 0));
  else if (p->strategy == PCV_XRAY_COLORED)
    PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xray_accum_kernel<PCV_XRAY_COLORED, 256>, 256, 0));
  else
    PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xray_accum_kernel<PCV_XRAY_HEIGHT_STDDEV, 256>, 256, 0));
  uint64_t accum_grid = (uint64_t)std::max(cus, 1) * (uint64_t)std::max(per_cu, 1);
  if (pcv_switches().xray_accum_grid) accum_grid = pcv_switches().xray_accum_grid;
  for (size_t gi = 0; gi + 1 < group_first.size(); ++gi) {
    const uint64_t f = group_first[gi], l = group_first[gi + 1];  // created tiles [f, l)
    ba.trees = d_trees + tree_first[gi];
    ba.ntrees = (uint32_t)(tree_first[gi + 1] - tree_first[gi]);
    ba.nchunks = group_chunks[gi];
    ba.created0 = (uint32_t)f;
    aa.created0 = (uint32_t)f;
    const uint64_t nb = (l - f) * nblocks;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((ba.nchunks + 3) / 4, 1u << 16));
    PCV_HIP_CHECK(ctx, hipMemsetAsync(d_counts, 0, 4 * nb, ctx->stream));
    {
      PcvProf prof(ctx, PCV_K_XRAY_BIN);
      hipLaunchKernelGGL(xray_bin_kernel<false>, dim3(grid), dim3(256), 0, ctx->stream, ba, d_counts, (const uint64_t*)nullptr,
                         (uint64_t*)nullptr, (double*)nullptr, (int64_t*)nullptr);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    {
      PcvProf prof(ctx, PCV_K_QUERY_BATCH_SCAN);
      if ((rc = pcv_batch_scan(ctx, sc, d_counts, nb, d_off))) return rc;
    }
    PCV_HIP_CHECK(ctx, hipMemsetAsync(d_counts, 0, 4 * nb, ctx->stream));
    {
      PcvProf prof(ctx, PCV_K_XRAY_SCATTER);
      XrayBinArgs bs = ba;
      bs.negative = nullptr;  // counted once, in the count pass
      hipLaunchKernelGGL(xray_bin_kernel<true>, dim3(grid), dim3(256), 0, ctx->stream, bs, d_counts, (const uint64_t*)d_off, d_rec, d_recz,
                         d_recb);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    aa.nbuckets = (uint32_t)nb;
    {
      PcvProf prof(ctx, sorted ? PCV_K_XRAY_SORTED : PCV_K_XRAY_ACCUM);
      const uint32_t ag = (uint32_t)std::min<uint64_t>(nb, accum_grid);
      if (binned)
        hipLaunchKernelGGL(xray_sorted_kernel<true>, dim3(ag), dim3(kSortThreads), 0, ctx->stream, aa, d_rec, d_recb, sort_cap);
      else if (sorted)
        hipLaunchKernelGGL(xray_sorted_kernel<false>, dim3(ag), dim3(kSortThreads), 0, ctx->stream, aa, d_rec, d_recb, sort_cap);
      else if (p->strategy == PCV_XRAY_XRAY)
        hipLaunchKernelGGL((xray_accum_kernel<PCV_XRAY_XRAY, 1024>), dim3(ag), dim3(1024), 0, ctx->stream, aa, (const uint8_t*)d_table);
      else if (p->strategy == PCV_XRAY_COLORED)
        hipLaunchKernelGGL((xray_accum_kernel<PCV_XRAY_COLORED, 256>), dim3(ag), dim3(256), 0, ctx->stream, aa, (const uint8_t*)d_table);
      else
        hipLaunchKernelGGL((xray_accum_kernel<PCV_XRAY_HEIGHT_STDDEV, 256>), dim3(ag), dim3(256), 0, ctx->stream, aa,
                           (const uint8_t*)d_table);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(x->drawn.data(), d_drawn, 8 * nc, hipMemcpyDeviceToHost, ctx->stream));
  if (d_neg) PCV_HIP_CHECK(ctx, hipMemcpyAsync(x->negative.data(), d_neg, 8 * nc, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the scratch and the batches are released on return
  return PCV_OK;
}

// the object of a checked run, or nothing (a failed run frees what it allocated)
static int xray_new(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t K, const pcv_xray_params* p, const pcv_xray_coloring* col,
                    pcv_xray** out) {
  pcv_xray* x = new pcv_xray();
  x->ctx = ctx;
  const int rc = xray_run(ctx, trees, K, p, col, x);
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
  return xray_new(ctx, &tree, 1, p, nullptr, out);
}

// pcv_xray_run_many (ex = false: colored_with_intensity refused, coloring ignored) and pcv_xray_run_ex
static int xray_run_checked(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t num_trees, const pcv_xray_params* p,
                            const pcv_xray_coloring* col, bool ex, pcv_xray** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!p || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  // PointCloudClientBuilder::build (point_cloud_client/src/lib.rs:92-95)
  if (num_trees == 0) return ctx->fail(PCV_E_INVALID, "xray: No locations specified for point cloud client.");
  if (!trees) return ctx->fail(PCV_E_INVALID, "null argument");
  if (num_trees > PCV_XRAY_MAX_TREES)
    return ctx->fail(PCV_E_INVALID, "xray: " + std::to_string(num_trees) + " octrees, more than PCV_XRAY_MAX_TREES (" +
                                        std::to_string(PCV_XRAY_MAX_TREES) + ")");
  char err[256] = {0};
  int vrc = ex ? pcv_xray_check_params_ex(p, col, 1, err, sizeof(err)) : pcv_xray_check_params(p, 1, err, sizeof(err));
  if (vrc) return ctx->fail(vrc, err);
  for (uint32_t t = 0; t < num_trees; ++t) {
    const std::string which = "xray: octree " + std::to_string(t);
    if (!trees[t]) return ctx->fail(PCV_E_INVALID, which + " is null");
    if (trees[t]->ctx != ctx) return ctx->fail(PCV_E_INVALID, which + " belongs to another context");
    if (p->interval_attribute && !trees[t]->has_intensity)
      return ctx->fail(PCV_E_INVALID, which + " has no intensity attribute to filter on");
    if (ex && coloring_needs_intensity(p, col) && !trees[t]->has_intensity)
      return ctx->fail(PCV_E_INVALID, which + " has no intensity attribute to color or bin by");
  }
  return xray_new(ctx, trees, num_trees, p, ex ? col : nullptr, out);
}

extern "C" int pcv_xray_run_many(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t num_trees, const pcv_xray_params* p, pcv_xray** out) {
  return xray_run_checked(ctx, trees, num_trees, p, nullptr, false, out);
}

extern "C" int pcv_xray_run_ex(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t num_trees, const pcv_xray_params* p,
                               const pcv_xray_coloring* coloring, pcv_xray** out) {
  if (!coloring) return xray_run_checked(ctx, trees, num_trees, p, nullptr, false, out);
  return xray_run_checked(ctx, trees, num_trees, p, coloring, true, out);
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

// ---- parent levels: create_non_leaf_nodes (:656-682), build_node (:726-759), build_parent (:410-450) -------------------
//
//   host   parent sets     parent_id of the level below, from deepest - 1 up to root_level (create_non_leaf_nodes)
//   host   2:1 Lanczos3    the taps of image 0.23.10 imageops::resize(FilterType::Lanczos3) for a square 2W -> W resize,
//                          as DynamicImage::resize reaches it (sample.rs vertical_sample, then horizontal_sample): a
//                          restatement of the pinned crate version, computed once per W with libm's sinf
//   K_xp   xray_parent     per (parent, 32 x 32 output block): the virtual 2W x 2W image of build_parent (children 1, 0,
//                          3, 2 at (0, 0), (0, W), (W, 0), (W, W); a missing child is the background) over the block's
//                          window into LDS, the vertical pass into LDS as f32, the horizontal pass, clamp, round, u8
//
// Every output pixel is a fixed sequence of f32 multiplies and adds (no FMA: -ffp-contract=off), so the images do not
// depend on scheduling and equal a host evaluation of the same sequence bit for bit.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <mutex>
#include <thread>

namespace {

constexpr uint32_t kTaps = 12;        // 2 x support 6: taps of an interior output index
constexpr uint32_t kWin = 2 * (kBlk - 1) + kTaps;  // 74: input rows / columns a 32-pixel output block reads

struct LanczosTap {  // one output index o: input [left, left + count), normalised weights
  uint32_t left, count;
  float w[kTaps];
};

// image::imageops::sample sinc / lanczos3: f32 throughout, sin = libm sinf (what f32::sin calls on linux-gnu)
float sinc_f32(float t) {
  if (t == 0.0f) return 1.0f;
  const float a = t * 3.14159265358979323846264338327950288f;  // f32::consts::PI
  return ::sinf(a) / a;
}
float lanczos3_f32(float x) { return std::fabs(x) < 3.0f ? sinc_f32(x) * sinc_f32(x / 3.0f) : 0.0f; }

// vertical_sample / horizontal_sample's filter table for 2W -> W: ratio 2, support 3 x 2 = 6
void lanczos_taps(uint32_t W, std::vector<LanczosTap>& taps) {
  taps.assign(W, LanczosTap{});
  const float ratio = 2.0f, sratio = 2.0f, support = 3.0f * sratio;
  const int64_t n = 2 * (int64_t)W;
  for (uint32_t o = 0; o < W; ++o) {
    const float c = ((float)o + 0.5f) * ratio;
    const int64_t left = std::min<int64_t>(std::max<int64_t>((int64_t)std::floor(c - support), 0), n - 1);
    const int64_t right = std::min<int64_t>(std::max<int64_t>((int64_t)std::ceil(c + support), left + 1), n);
    const float ci = c - 0.5f;
    LanczosTap& t = taps[o];
    t.left = (uint32_t)left;
    t.count = (uint32_t)(right - left);
    float sum = 0.0f;
    for (int64_t i = left; i < right; ++i) {
      const float w = lanczos3_f32(((float)i - ci) / sratio);
      t.w[i - left] = w;
      sum += w;
    }
    for (uint32_t k = 0; k < t.count; ++k) t.w[k] /= sum;
  }
}

struct XrayParentArgs {
  const uint32_t* leaves;   // created leaf images, node positions [0, nleaves)
  const uint32_t* parents;  // parent images, node positions [nleaves, ...)
  uint64_t nleaves;
  const int64_t* slots;     // 4 per parent of the level: node position of child c, -1 where it is missing
  uint32_t* out;            // the level's first parent image
  uint64_t nparents;
  const LanczosTap* taps;   // W entries, rows and columns alike
  uint32_t W, nbx, bg;
};

__device__ __forceinline__ float4 unpack_f4(uint32_t p) {
  return make_float4((float)(p & 255u), (float)((p >> 8) & 255u), (float)((p >> 16) & 255u), (float)(p >> 24));
}
// horizontal_sample's store: clamp(t, 0, 255) then FloatNearest (round half away from zero) as u8
__device__ __forceinline__ uint32_t to_u8_round(float t) {
  t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
  return (uint32_t)roundf(t);
}

// 256 threads per (parent, output block); the grid strides over parents x blocks
__global__ __launch_bounds__(256) void xray_parent_kernel(XrayParentArgs a) {
  __shared__ uint32_t win[kWin * kWin];   // input window of the virtual image, RGBA8
  __shared__ float4 mid[kBlk * kWin];     // vertical pass: block rows x window columns, f32 RGBA
  const uint32_t nblocks = a.nbx * a.nbx;
  const uint64_t total = a.nparents * nblocks;
  const uint32_t W = a.W;
  for (uint64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const uint64_t parent = b / nblocks;
    const uint32_t blk = (uint32_t)(b % nblocks), by = blk / a.nbx, bx = blk % a.nbx;
    const uint32_t oy0 = by * kBlk, ox0 = bx * kBlk;
    const uint32_t oy1 = min(oy0 + kBlk, W), ox1 = min(ox0 + kBlk, W);  // exclusive
    const LanczosTap& ty0 = a.taps[oy0];
    const LanczosTap& ty1 = a.taps[oy1 - 1];
    const LanczosTap& tx0 = a.taps[ox0];
    const LanczosTap& tx1 = a.taps[ox1 - 1];
    const uint32_t row0 = ty0.left, nrow = ty1.left + ty1.count - row0;  // <= kWin: left and right never decrease
    const uint32_t col0 = tx0.left, ncol = tx1.left + tx1.count - col0;
    const int64_t* slot = a.slots + 4 * parent;
    // the window: child pixel or background (build_parent's from_pixel + copy_from)
    for (uint32_t i = threadIdx.x; i < nrow * ncol; i += blockDim.x) {
      const uint32_t vy = row0 + i / ncol, vx = col0 + i % ncol;
      const uint32_t top = vy < W, lft = vx < W;
      const uint32_t child = lft ? (top ? 1u : 0u) : (top ? 3u : 2u);
      const int64_t s = slot[child];
      uint32_t px = a.bg;
      if (s >= 0) {
        const uint32_t* img = (uint64_t)s < a.nleaves ? a.leaves + (uint64_t)s * W * W : a.parents + ((uint64_t)s - a.nleaves) * W * W;
        px = img[(uint64_t)(vy - (top ? 0u : W)) * W + (vx - (lft ? 0u : W))];
      }
      win[(i / ncol) * kWin + i % ncol] = px;
    }
    __syncthreads();
    // vertical pass: t = t + p * w in tap order, f32, neither clamped nor rounded
    for (uint32_t i = threadIdx.x; i < (oy1 - oy0) * ncol; i += blockDim.x) {
      const uint32_t r = i / ncol, c = i % ncol;
      const LanczosTap& t = a.taps[oy0 + r];
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const uint32_t* src = win + (t.left - row0) * kWin + c;
      for (uint32_t k = 0; k < t.count; ++k) {
        const float4 p = unpack_f4(src[k * kWin]);
        const float w = t.w[k];
        acc.x = acc.x + p.x * w;
        acc.y = acc.y + p.y * w;
        acc.z = acc.z + p.z * w;
        acc.w = acc.w + p.w * w;
      }
      mid[r * kWin + c] = acc;
    }
    __syncthreads();
    // horizontal pass over the intermediate, then clamp, round, u8
    uint32_t* out = a.out + parent * W * W;
    for (uint32_t i = threadIdx.x; i < kBlkPx; i += blockDim.x) {
      const uint32_t r = i / kBlk, c = i % kBlk;
      const uint32_t oy = oy0 + r, ox = ox0 + c;
      if (oy >= oy1 || ox >= ox1) continue;
      const LanczosTap& t = a.taps[ox];
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float4* src = mid + r * kWin + (t.left - col0);
      for (uint32_t k = 0; k < t.count; ++k) {
        const float4 p = src[k];
        const float w = t.w[k];
        acc.x = acc.x + p.x * w;
        acc.y = acc.y + p.y * w;
        acc.z = acc.z + p.z * w;
        acc.w = acc.w + p.w * w;
      }
      out[(uint64_t)oy * W + ox] = to_u8_round(acc.x) | to_u8_round(acc.y) << 8 | to_u8_round(acc.z) << 16 | to_u8_round(acc.w) << 24;
    }
    __syncthreads();  // the next block overwrites the window and the intermediate
  }
}

// ---- meta.pb (the PNG encoders live in pcv_png.cpp and pcv_xray_png.hip) -----------------------------------------------
// rust-protobuf 2.x, proto3: fields in number order, zero scalars omitted, set message fields always written
void pb_varint(std::vector<uint8_t>& o, uint64_t v) {
  while (v >= 0x80) {
    o.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  o.push_back((uint8_t)v);
}
void pb_double(std::vector<uint8_t>& o, uint32_t field, double v) {
  if (v == 0.0) return;
  pb_varint(o, field << 3 | 1);
  uint8_t b[8];
  std::memcpy(b, &v, 8);
  o.insert(o.end(), b, b + 8);
}
void pb_uint(std::vector<uint8_t>& o, uint32_t field, uint64_t v) {
  if (v == 0) return;
  pb_varint(o, field << 3);
  pb_varint(o, v);
}
void pb_bytes(std::vector<uint8_t>& o, uint32_t field, const std::vector<uint8_t>& m) {
  pb_varint(o, field << 3 | 2);
  pb_varint(o, m.size());
  o.insert(o.end(), m.begin(), m.end());
}

std::string quad_name(uint32_t level, uint64_t index) {  // NodeId Display (quadtree/src/lib.rs:218-234)
  std::string s = "r";
  for (int l = (int)level - 1; l >= 0; --l) s.push_back((char)('0' + ((index >> (2 * l)) & 3u)));
  return s;
}

bool write_at(int dirfd, const std::string& name, const uint8_t* data, uint64_t len) {
  const int fd = openat(dirfd, name.c_str(), O_CREAT | O_WRONLY | O_TRUNC | O_CLOEXEC, 0666);
  if (fd < 0) return false;
  bool ok = true;
  while (len) {
    const ssize_t w = ::write(fd, data, (size_t)len);
    if (w <= 0) {
      ok = false;
      break;
    }
    data += w;
    len -= (uint64_t)w;
  }
  return ::close(fd) == 0 && ok;
}

}  // namespace

extern "C" int pcv_xray_lanczos_taps(uint32_t tile_size_px, uint32_t* left, uint32_t* count, float* weights) {
  if (tile_size_px == 0 || tile_size_px > kMaxTilePx) return PCV_E_INVALID;
  std::vector<LanczosTap> taps;
  lanczos_taps(tile_size_px, taps);
  for (uint32_t o = 0; o < tile_size_px; ++o) {
    if (left) left[o] = taps[o].left;
    if (count) count[o] = taps[o].count;
    if (weights)
      for (uint32_t k = 0; k < kTaps; ++k) weights[(uint64_t)o * kTaps + k] = k < taps[o].count ? taps[o].w[k] : 0.0f;
  }
  return PCV_OK;
}

// The levels above a set of nodes: the node list after them (plevel, pindex; first[k] = the first parent of level
// from - 1 - k in it) and their images on the device
struct XrayLevels {
  std::vector<uint32_t> plevel;
  std::vector<uint64_t> pindex, first;
  uint32_t* d_parents = nullptr;
};

// create_non_leaf_nodes(base, from, to) for the nodes `base` of level `from` (node positions 0 .. base.size() - 1, their
// images at d_base), one xray_parent_kernel launch per level under the kernel-stat id `prof_id`: the parent levels of a
// built quadtree (base = the created leaves) and the upper levels of a merged one (base = the parts' roots)
static int xray_build_levels(pcv_ctx* ctx, uint32_t W, uint32_t bg, const std::vector<uint64_t>& base, uint32_t from, uint32_t to,
                             const uint32_t* d_base, int prof_id, XrayLevels* out) {
  const uint64_t nc = base.size();
  std::vector<uint32_t> plevel;
  std::vector<uint64_t> pindex, first;
  // create_non_leaf_nodes: the parent ids of the level below, to ..= from - 1 (ascending index per level)
  std::vector<uint64_t> below(base);
  for (uint32_t level = from; nc && level > to; --level) {
    std::vector<uint64_t> up(below.size());
    for (size_t i = 0; i < below.size(); ++i) up[i] = below[i] >> 2;
    std::sort(up.begin(), up.end());
    up.erase(std::unique(up.begin(), up.end()), up.end());
    first.push_back(pindex.size());
    for (uint64_t i : up) {
      plevel.push_back(level - 1);
      pindex.push_back(i);
    }
    below.swap(up);
  }
  first.push_back(pindex.size());
  const uint64_t np = pindex.size();
  if (np == 0) return PCV_OK;
  // child slots: node positions of (index << 2) + c one level down, -1 where that child was not created
  std::vector<std::pair<uint64_t, uint64_t>> leaf_pos(nc);  // (leaf index, node position)
  for (uint64_t c = 0; c < nc; ++c) leaf_pos[c] = {base[c], c};
  std::sort(leaf_pos.begin(), leaf_pos.end());
  std::vector<int64_t> slots(4 * np, -1);
  for (size_t k = 0; k + 1 < first.size(); ++k) {
    for (uint64_t p = first[k]; p < first[k + 1]; ++p)
      for (uint64_t c = 0; c < 4; ++c) {
        const uint64_t child = (pindex[p] << 2) + c;
        if (k == 0) {
          auto it = std::lower_bound(leaf_pos.begin(), leaf_pos.end(), std::make_pair(child, (uint64_t)0));
          if (it != leaf_pos.end() && it->first == child) slots[4 * p + c] = (int64_t)it->second;
        } else {
          auto b = pindex.begin() + (ptrdiff_t)first[k - 1], e = pindex.begin() + (ptrdiff_t)first[k];
          auto it = std::lower_bound(b, e, child);
          if (it != e && *it == child) slots[4 * p + c] = (int64_t)(nc + (uint64_t)(it - pindex.begin()));
        }
      }
  }
  std::vector<LanczosTap> taps;
  lanczos_taps(W, taps);
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc;
  uint32_t* d_parents = nullptr;
  if ((rc = ctx->dev_alloc((void**)&d_parents, 4ull * W * W * np)))  // every parent image before any launch
    return ctx->fail(PCV_E_OOM, "xray: no device memory for " + std::to_string(np) + " parent images (" + ctx->last_error + ")");
  PcvScratch sc(ctx);
  int64_t* d_slots;
  LanczosTap* d_taps;
  if ((rc = sc.get(&d_slots, 4 * np)) || (rc = sc.get(&d_taps, W))) {
    ctx->dev_free(d_parents);
    return rc;
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_slots, slots.data(), 8 * slots.size(), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_taps, taps.data(), sizeof(LanczosTap) * W, hipMemcpyHostToDevice, ctx->stream));
  int cus = 0, per_cu = 0;
  PCV_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xray_parent_kernel, 256, 0));
  const uint64_t resident = (uint64_t)std::max(cus, 1) * (uint64_t)std::max(per_cu, 1);
  XrayParentArgs a{};
  a.leaves = d_base;
  a.parents = d_parents;
  a.nleaves = nc;
  a.taps = d_taps;
  a.W = W;
  a.nbx = (W + kBlk - 1) / kBlk;
  a.bg = bg;
  for (size_t k = 0; k + 1 < first.size(); ++k) {  // a level reads the one below: one launch each, in order
    a.slots = d_slots + 4 * first[k];
    a.out = d_parents + first[k] * W * W;
    a.nparents = first[k + 1] - first[k];
    const uint64_t work = a.nparents * a.nbx * a.nbx;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(work, 4 * resident);
    {
      PcvProf prof(ctx, prof_id);
      hipLaunchKernelGGL(xray_parent_kernel, dim3(grid), dim3(256), 0, ctx->stream, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(ctx->stream);
      ctx->dev_free(d_parents);
      return ctx->fail(PCV_E_HIP, std::string("xray_parent_kernel: ") + hipGetErrorString(e));
    }
  }
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    ctx->dev_free(d_parents);
    return ctx->fail(PCV_E_HIP, "xray: parent levels failed");
  }
  out->d_parents = d_parents;
  out->plevel.swap(plevel);
  out->pindex.swap(pindex);
  out->first.swap(first);
  return PCV_OK;
}

static int xray_build_parents(pcv_xray* x) {
  const uint64_t nc = x->created.size();
  std::vector<uint64_t> leaves(nc);
  for (uint64_t c = 0; c < nc; ++c) leaves[c] = x->geo.index[x->created[c]];
  XrayLevels lv;
  const int rc = xray_build_levels(x->ctx, x->W, x->bg, leaves, x->geo.deepest_level, x->root_level, x->d_images, PCV_K_XRAY_PARENT, &lv);
  if (rc) return rc;
  x->d_parents = lv.d_parents;
  x->parent_level.swap(lv.plevel);
  x->parent_index.swap(lv.pindex);
  x->level_first.swap(lv.first);
  return PCV_OK;
}

extern "C" int pcv_xray_build_parents(pcv_xray* x) {
  if (!x) return PCV_E_INVALID;
  if (x->kind != kXrayBuilt) return xray_not_built(x, "pcv_xray_build_parents");
  if (x->parents_built) return PCV_OK;
  const int rc = xray_build_parents(x);
  if (rc) return rc;
  x->parents_built = true;
  x->ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_xray_nodes(const pcv_xray* x, uint64_t* num_nodes, uint64_t capacity, uint32_t* level, uint64_t* index) {
  if (!x) return PCV_E_INVALID;
  const bool listed = x->kind != kXrayBuilt;
  const uint64_t nc = x->created.size(), n = listed ? x->node_index.size() : nc + x->parent_index.size();
  if (num_nodes) *num_nodes = n;
  for (uint64_t i = 0; i < std::min(n, capacity); ++i) {
    if (level) level[i] = listed ? x->node_level[i] : (i < nc ? x->geo.deepest_level : x->parent_level[i - nc]);
    if (index) index[i] = listed ? x->node_index[i] : (i < nc ? x->geo.index[x->created[i]] : x->parent_index[i - nc]);
  }
  return PCV_OK;
}

extern "C" uint32_t pcv_xray_tile_size(const pcv_xray* x) { return x ? x->W : 0; }

// takes the finished file of a node; false: it could not be kept (PCV_E_IO). May be called from several threads at once
// where xray_node_files is asked to work in parallel
using XrayFileSink = std::function<bool(uint64_t node, const uint8_t* file, uint64_t len)>;

// node images [first, first + count) of a built quadtree's node list into dst (host or device), no synchronisation
static int queue_node_images(pcv_xray* x, uint64_t first, uint64_t count, uint8_t* dst, hipMemcpyKind kind) {
  pcv_ctx* ctx = x->ctx;
  const uint64_t nc = x->created.size(), tile_bytes = 4ull * x->W * x->W;
  const uint64_t nl = first < nc ? std::min(count, nc - first) : 0;
  if (nl)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst, reinterpret_cast<const uint8_t*>(x->d_images) + first * tile_bytes, nl * tile_bytes, kind, ctx->stream));
  if (count > nl)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst + nl * tile_bytes, reinterpret_cast<const uint8_t*>(x->d_parents) + (first + nl - nc) * tile_bytes,
                                      (count - nl) * tile_bytes, kind, ctx->stream));
  return PCV_OK;
}

static bool read_file(const std::string& path, std::vector<uint8_t>& data) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  data.clear();
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + k);
  const bool ok = !std::ferror(f);
  std::fclose(f);
  return ok;
}

// node `node` of an opened quadtree, decoded from its file into W x W x 4 host bytes
static int opened_node_to_host(const pcv_xray* x, uint64_t node, uint8_t* dst) {
  const std::string path = x->dir + "/" + quad_name(x->node_level[node], x->node_index[node]) + ".png";
  std::vector<uint8_t> file;
  if (!read_file(path, file)) return xray_fail(x, PCV_E_IO, "xray: cannot read " + path);
  uint32_t w = 0, h = 0;
  int rc = pcv_png_decode(file.data(), file.size(), &w, &h, nullptr, 0);
  if (rc) return xray_fail(x, rc == PCV_E_INVALID ? PCV_E_IO : rc, path + ": " + pcv_host_last_error());
  if (w != x->W || h != x->W)
    return xray_fail(x, PCV_E_INVALID, path + " is " + std::to_string(w) + " x " + std::to_string(h) + ", the meta's tile_size is " + std::to_string(x->W));
  rc = pcv_png_decode(file.data(), file.size(), &w, &h, dst, 4ull * x->W * x->W);
  if (rc) return xray_fail(x, PCV_E_IO, path + ": " + pcv_host_last_error());
  return PCV_OK;
}

static bool xray_part_alive(const XrayPartRef& r) {
  std::lock_guard<std::mutex> g(g_xray_mu);
  auto it = g_xray_live.find(r.part);
  return it != g_xray_live.end() && it->second == r.serial;
}

// node images of any kind of quadtree into checked arguments; returns after the copies have completed
static int xray_node_images(pcv_xray* x, uint64_t first, uint64_t count, int mem, uint8_t* rgba) {
  pcv_ctx* ctx = x->ctx;
  const uint64_t tile_bytes = 4ull * x->W * x->W;
  if (mem == PCV_MEM_DEVICE && !ctx) return xray_fail(x, PCV_E_INVALID, "xray: a quadtree opened without a context has host images only");
  if (ctx) PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (x->kind == kXrayBuilt) {
    const int rc = queue_node_images(x, first, count, rgba, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    if (rc) return rc;
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PCV_OK;
  }
  if (x->kind == kXrayOpened) {
    if (mem == PCV_MEM_HOST) {
      for (uint64_t i = 0; i < count; ++i)
        if (int rc = opened_node_to_host(x, first + i, rgba + i * tile_bytes)) return rc;
      return PCV_OK;
    }
    uint8_t* host = nullptr;  // decoded into pinned memory, one upload
    int rc = ctx->host_alloc((void**)&host, count * tile_bytes);
    if (rc) return rc;
    for (uint64_t i = 0; !rc && i < count; ++i) rc = opened_node_to_host(x, first + i, host + i * tile_bytes);
    if (!rc) {
      hipError_t e = hipMemcpyAsync(rgba, host, count * tile_bytes, hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) rc = ctx->fail(PCV_E_HIP, std::string("xray: image upload: ") + hipGetErrorString(e));
    }
    ctx->host_release(host);
    return rc;
  }
  // merged: runs of nodes that belong to one part go to that part; the new levels are this object's own
  for (const XrayPartRef& r : x->parts)
    if (!xray_part_alive(r)) return ctx->fail(PCV_E_INVALID, "xray: a part of this merged quadtree was freed before it");
  const uint64_t own_first = x->node_index.size() - x->parent_index.size();
  uint64_t at = first;
  const uint64_t end = first + count;
  for (const XrayPartRef& r : x->parts) {
    if (at >= end) break;
    if (at >= r.first + r.count || r.count == 0) continue;
    const uint64_t k = std::min(end, r.first + r.count) - at;
    const int rc = xray_node_images(r.part, at - r.first, k, mem, rgba + (at - first) * tile_bytes);
    if (rc) return r.part->ctx ? rc : ctx->fail(rc, pcv_host_last_error());
    at += k;
  }
  if (at < end) {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(rgba + (at - first) * tile_bytes, reinterpret_cast<const uint8_t*>(x->d_parents) + (at - own_first) * tile_bytes,
                                      (end - at) * tile_bytes, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                      ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return PCV_OK;
}

extern "C" int pcv_xray_node_images(pcv_xray* x, uint64_t first, uint64_t count, uint64_t capacity, int mem, uint8_t* rgba) {
  if (!x) return PCV_E_INVALID;
  uint64_t n = 0;
  pcv_xray_nodes(x, &n, 0, nullptr, nullptr);
  if (first > n || count > n - first) return xray_fail(x, PCV_E_INVALID, "xray: node range past the end");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return xray_fail(x, PCV_E_INVALID, "bad mem");
  const uint64_t tile_bytes = 4ull * x->W * x->W;
  if (count * tile_bytes > capacity) return xray_fail(x, PCV_E_INVALID, "xray: capacity below count x W x W x 4 bytes");
  if (count == 0) return PCV_OK;
  if (!rgba) return xray_fail(x, PCV_E_INVALID, "null output");
  return xray_node_images(x, first, count, mem, rgba);
}

// root_node.bounding_rect of a built quadtree: Node::from_node_id_and_root_bounding_rect(root_node_id, rect), what its
// meta file holds
static void built_root_rect(const pcv_xray* x, double rect[3]) {
  std::memcpy(rect, x->geo.rect, sizeof(x->geo.rect));
  for (int l = (int)x->root_level - 1; l >= 0; --l) {
    const uint32_t ci = (uint32_t)(x->root_index >> (2 * l)) & 3u;
    const double half = rect[2] / 2.0;
    if (ci & 1u) rect[1] += half;
    if (ci & 2u) rect[0] += half;
    rect[2] = half;
  }
}

// Meta (xray_proto Meta, CURRENT_VERSION 3) to get_meta_pb_path: the root id with "r" -> "meta", + ".pb"
static bool write_meta_file(int dirfd, const std::string& dir, uint32_t root_level, uint64_t root_index, const double rect[3],
                            uint32_t deepest_level, uint32_t W, const std::vector<uint32_t>& level, const std::vector<uint64_t>& index,
                            std::string* err) {
  std::vector<uint8_t> meta, r, mn;
  pb_uint(meta, 1, 3);
  pb_double(mn, 1, rect[0]);
  pb_double(mn, 2, rect[1]);
  pb_bytes(r, 3, mn);
  pb_double(r, 4, rect[2]);
  pb_bytes(meta, 2, r);
  pb_uint(meta, 3, deepest_level);
  pb_uint(meta, 4, W);
  for (size_t i = 0; i < index.size(); ++i) {
    std::vector<uint8_t> id;
    pb_uint(id, 1, level[i]);
    pb_uint(id, 2, index[i]);
    pb_bytes(meta, 5, id);
  }
  const std::string name = "meta" + quad_name(root_level, root_index).substr(1) + ".pb";
  if (write_at(dirfd, name, meta.data(), meta.size())) return true;
  *err = "cannot write " + dir + "/" + name;
  return false;
}

// ---- xray_proto Meta, read (Meta::from_proto, xray/src/lib.rs:81-116) --------------------------------------------------
// proto3 wire format of xray_proto_rust/src/proto.proto: Meta { int32 version = 1; Rect bounding_rect = 2; uint32
// deepest_level = 3; uint32 tile_size = 4; repeated NodeId nodes = 5 }, Rect { Vector2f deprecated_min = 1; float
// deprecated_edge_length = 2; Vector2d min = 3; double edge_length = 4 }, NodeId { uint32 level = 1; uint64 index = 2 }.
// Fields may come in any order, a repeated scalar field keeps its last value, unknown fields are skipped.
namespace {

struct PbReader {
  const uint8_t* p;
  size_t n, pos = 0;
  bool bad = false;
  bool more() const { return !bad && pos < n; }
  uint64_t varint() {
    uint64_t v = 0;
    for (int shift = 0; shift < 64; shift += 7) {
      if (pos >= n) break;
      const uint8_t c = p[pos++];
      v |= (uint64_t)(c & 0x7f) << shift;
      if (c < 0x80) return v;
    }
    bad = true;
    return 0;
  }
  // one field: its number, wire type and value (varint / fixed bits in `v`, a length-delimited body in `sub`)
  bool field(uint32_t* num, uint32_t* wt, uint64_t* v, PbReader* sub) {
    const uint64_t key = varint();
    if (bad || (key >> 3) == 0 || (key >> 3) > 0x1fffffffu) return !(bad = true);
    *num = (uint32_t)(key >> 3);
    *wt = (uint32_t)(key & 7);
    *v = 0;
    if (*wt == 0) {
      *v = varint();
    } else if (*wt == 1 || *wt == 5) {
      const size_t k = *wt == 1 ? 8 : 4;
      if (n - pos < k) return !(bad = true);
      std::memcpy(v, p + pos, k);  // little endian, as the wire
      pos += k;
    } else if (*wt == 2) {
      const uint64_t k = varint();
      if (bad || k > n - pos) return !(bad = true);
      *sub = PbReader{p + pos, (size_t)k};
      pos += (size_t)k;
    } else {
      return !(bad = true);  // groups: not in this schema
    }
    return !bad;
  }
};

struct XrayMeta {
  int32_t version = 0;
  bool has_min = false;
  double min[2] = {0, 0}, edge = 0;
  float dmin[2] = {0, 0}, dedge = 0;
  uint32_t deepest_level = 0, tile_size = 0;
  std::vector<std::pair<uint32_t, uint64_t>> nodes;
};

double pb_f64(uint64_t v) {
  double d;
  std::memcpy(&d, &v, 8);
  return d;
}
float pb_f32(uint64_t v) {
  const uint32_t u = (uint32_t)v;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

bool parse_meta(const std::vector<uint8_t>& data, XrayMeta* m) {
  PbReader top{data.data(), data.size()};
  uint32_t f, wt;
  uint64_t v;
  PbReader sub{nullptr, 0};
  while (top.more()) {
    if (!top.field(&f, &wt, &v, &sub)) return false;
    if (f == 1 && wt == 0) m->version = (int32_t)v;
    if (f == 3 && wt == 0) m->deepest_level = (uint32_t)v;
    if (f == 4 && wt == 0) m->tile_size = (uint32_t)v;
    if ((f == 1 || f == 3 || f == 4) && wt != 0) return false;
    if ((f == 2 || f == 5) && wt != 2) return false;
    if (f == 2) {
      PbReader rect = sub, vec{nullptr, 0};
      while (rect.more()) {
        uint32_t g, gw;
        if (!rect.field(&g, &gw, &v, &vec)) return false;
        if ((g == 1 || g == 3) && gw != 2) return false;
        if ((g == 2 && gw != 5) || (g == 4 && gw != 1)) return false;
        if (g == 2) m->dedge = pb_f32(v);
        if (g == 4) m->edge = pb_f64(v);
        if (g == 1 || g == 3) {
          if (g == 3) m->has_min = true;
          PbReader none{nullptr, 0};
          while (vec.more()) {
            uint32_t c, cw;
            if (!vec.field(&c, &cw, &v, &none)) return false;
            if ((c == 1 || c == 2) && cw != (g == 3 ? 1u : 5u)) return false;
            if (c == 1 || c == 2) {
              if (g == 3) m->min[c - 1] = pb_f64(v);
              else m->dmin[c - 1] = pb_f32(v);
            }
          }
          if (vec.bad) return false;
        }
      }
      if (rect.bad) return false;
    }
    if (f == 5) {
      PbReader id = sub, none{nullptr, 0};
      uint32_t level = 0;
      uint64_t index = 0;
      while (id.more()) {
        uint32_t g, gw;
        if (!id.field(&g, &gw, &v, &none)) return false;
        if ((g == 1 || g == 2) && gw != 0) return false;
        if (g == 1) level = (uint32_t)v;
        if (g == 2) index = v;
      }
      if (id.bad) return false;
      m->nodes.emplace_back(level, index);
    }
  }
  return !top.bad;
}

}  // namespace

#include <dirent.h>

extern "C" int pcv_xray_open_dir(pcv_ctx* ctx, const char* directory, uint32_t capacity, pcv_xray** parts, uint32_t* num_parts) {
  auto fail = [&](int code, const std::string& m) { return ctx ? ctx->fail(code, m) : pcv_host_fail(code, m); };
  if (!directory || !num_parts) return fail(PCV_E_INVALID, "null argument");
  const std::string dir(directory);
  DIR* d = opendir(dir.c_str());
  if (!d) return fail(PCV_E_IO, "cannot open directory " + dir);
  std::vector<std::string> names;  // "meta*.pb" (META_PREFIX, META_EXTENSION)
  while (struct dirent* e = readdir(d)) {
    const std::string name(e->d_name);
    if (name.size() >= 7 && name.compare(0, 4, "meta") == 0 && name.compare(name.size() - 3, 3, ".pb") == 0) names.push_back(name);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  *num_parts = (uint32_t)names.size();
  if (capacity < names.size() || names.empty()) return PCV_OK;
  if (!parts) return fail(PCV_E_INVALID, "null argument");
  std::vector<pcv_xray*> made;
  auto undo = [&](int code, const std::string& m) {
    for (pcv_xray* x : made) pcv_xray_free(x);
    return fail(code, m);
  };
  for (const std::string& name : names) {
    const std::string path = dir + "/" + name;
    std::vector<uint8_t> data;
    if (!read_file(path, data)) return undo(PCV_E_IO, "cannot read " + path);
    XrayMeta m;
    if (!parse_meta(data, &m)) return undo(PCV_E_INVALID, "Could not parse " + path);
    if (m.version != 2 && m.version != 3)
      return undo(PCV_E_INVALID, path + ": Invalid version. We only support 3, but found " + std::to_string(m.version) + ".");
    if (m.tile_size == 0 || m.tile_size > kMaxTilePx) return undo(PCV_E_INVALID, path + ": tile_size outside 1 ..= 32768");
    if (m.deepest_level > 31) return undo(PCV_E_INVALID, path + ": deepest_level above 31 (a u64 index holds 32 levels)");
    for (const auto& nd : m.nodes)
      if (nd.first > m.deepest_level || (nd.first < 32 && (nd.second >> (2 * nd.first)) != 0))
        return undo(PCV_E_INVALID, path + ": a node outside the quadtree");
    pcv_xray* x = new pcv_xray();
    made.push_back(x);
    x->ctx = ctx;
    x->kind = kXrayOpened;
    x->W = m.tile_size;
    x->dir = dir;
    x->geo.deepest_level = m.deepest_level;
    // Meta::from_proto: Rect.min where present, else the deprecated f32 fields widened (version 2 files)
    x->geo.rect[0] = m.has_min ? m.min[0] : (double)m.dmin[0];
    x->geo.rect[1] = m.has_min ? m.min[1] : (double)m.dmin[1];
    x->geo.rect[2] = m.has_min ? m.edge : (double)m.dedge;
    // the node set in a stated order: descending level, then ascending index (duplicates of a file fold, as in a set)
    std::sort(m.nodes.begin(), m.nodes.end(), [](const std::pair<uint32_t, uint64_t>& a, const std::pair<uint32_t, uint64_t>& b) {
      return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    m.nodes.erase(std::unique(m.nodes.begin(), m.nodes.end()), m.nodes.end());
    for (const auto& nd : m.nodes) {
      x->node_level.push_back(nd.first);
      x->node_index.push_back(nd.second);
      if (nd.first == m.deepest_level) {
        x->created.push_back(x->geo.index.size());
        x->geo.index.push_back(nd.second);
      }
    }
  }
  for (size_t i = 0; i < made.size(); ++i) parts[i] = made[i];
  return PCV_OK;
}

// ---- merge_xray_quadtrees (xray/src/bin/merge_xray_quadtrees.rs:129-205) ---------------------------------------------
namespace {

struct MergePlan {
  uint32_t L = 0, deepest = 0, W = 0;
  double rect[3] = {0, 0, 0};
  std::vector<int64_t> root_pos;    // per part: position of its root in its own node list, -1 for an empty part
  std::vector<uint64_t> root_index;  // per part: index of its root at level L
};

int merge_plan(pcv_xray* const* parts, uint32_t num_parts, MergePlan* plan, std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = m;
    return PCV_E_INVALID;
  };
  if (num_parts == 0) return bad("No subquadtrees meta files found.");
  if (!parts) return bad("xray merge: null argument");
  struct Root {
    uint32_t level;
    uint64_t index;
  };
  std::vector<Root> roots;
  int first_part = -1;
  plan->root_pos.assign(num_parts, -1);
  plan->root_index.assign(num_parts, 0);
  for (uint32_t k = 0; k < num_parts; ++k) {
    const pcv_xray* x = parts[k];
    if (!x) return bad("xray merge: part " + std::to_string(k) + " is null");
    {
      std::lock_guard<std::mutex> g(g_xray_mu);
      if (!g_xray_live.count(x)) return bad("xray merge: part " + std::to_string(k) + " is not a live pcv_xray");
    }
    if (x->kind == kXrayBuilt && !x->parents_built && !x->created.empty() && x->root_level < x->geo.deepest_level)
      return bad("xray merge: the parent levels of part " + std::to_string(k) + " are not built (pcv_xray_build_parents)");
    uint64_t n = 0;
    pcv_xray_nodes(x, &n, 0, nullptr, nullptr);
    std::vector<uint32_t> level(n);
    std::vector<uint64_t> index(n);
    pcv_xray_nodes(x, &n, n, level.data(), index.data());
    if (n == 0) continue;  // get_root_nodes skips it; it still takes part in the deepest_level and tile_size checks
    uint64_t at = 0, count = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (level[i] < level[at]) at = i, count = 0;
      if (level[i] == level[at]) ++count;
    }
    if (count != 1)
      return bad("xray merge: part " + std::to_string(k) + " has " + std::to_string(count) + " nodes at its minimum level " +
                 std::to_string(level[at]) + ": its root is not defined");
    plan->root_pos[k] = (int64_t)at;
    plan->root_index[k] = index[at];
    roots.push_back(Root{level[at], index[at]});
    if (first_part < 0) first_part = (int)k;
  }
  if (roots.empty()) return bad("All subquadtress are empty.");
  for (size_t a = 0; a < roots.size(); ++a)
    for (size_t b = a + 1; b < roots.size(); ++b)
      if (roots[a].level == roots[b].level && roots[a].index == roots[b].index) return bad("Not all roots are unique.");
  for (const Root& r : roots)
    if (r.level != roots[0].level) return bad("Not all roots have the same level.");
  for (uint32_t k = 1; k < num_parts; ++k)
    if (parts[k]->geo.deepest_level != parts[0]->geo.deepest_level) return bad("Not all meta files have the same deepest level.");
  for (uint32_t k = 1; k < num_parts; ++k)
    if (parts[k]->W != parts[0]->W) return bad("Not all meta files have the same tile size.");
  plan->L = roots[0].level;
  plan->deepest = parts[0]->geo.deepest_level;
  plan->W = parts[0]->W;
  if (plan->L > plan->deepest) return bad("xray merge: the roots' level is above deepest_level");
  // the first root's rect under Node::parent until level 0
  const pcv_xray* x = parts[first_part];
  if (x->kind == kXrayBuilt) built_root_rect(x, plan->rect);
  else std::memcpy(plan->rect, x->geo.rect, sizeof(plan->rect));
  uint64_t idx = roots[0].index;
  for (uint32_t l = plan->L; l > 0; --l, idx >>= 2) {
    const uint32_t ci = (uint32_t)idx & 3u;
    if (ci & 1u) plan->rect[1] -= plan->rect[2];
    if (ci & 2u) plan->rect[0] -= plan->rect[2];
    plan->rect[2] *= 2.0;
  }
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_xray_merge_check(pcv_xray* const* parts, uint32_t num_parts, uint32_t* root_level, double rect[3], char* err,
                                    uint64_t errcap) {
  MergePlan plan;
  std::string m;
  const int rc = merge_plan(parts, num_parts, &plan, &m);
  if (rc) return fail_msg(err, errcap, m);
  if (root_level) *root_level = plan.L;
  if (rect) std::memcpy(rect, plan.rect, sizeof(plan.rect));
  return PCV_OK;
}

extern "C" int pcv_xray_merge(pcv_ctx* ctx, pcv_xray* const* parts, uint32_t num_parts, uint32_t background, pcv_xray** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (background > PCV_XRAY_BG_TRANSPARENT) return ctx->fail(PCV_E_INVALID, "xray: unknown background");
  MergePlan plan;
  std::string m;
  int rc = merge_plan(parts, num_parts, &plan, &m);
  if (rc) return ctx->fail(rc, m);
  for (uint32_t k = 0; k < num_parts; ++k)
    if (parts[k]->ctx && parts[k]->ctx != ctx) return ctx->fail(PCV_E_INVALID, "xray merge: part " + std::to_string(k) + " belongs to another context");
  const uint32_t W = plan.W;
  const uint64_t tile_bytes = 4ull * W * W;
  pcv_xray* x = new pcv_xray();
  x->ctx = ctx;
  x->kind = kXrayMerged;
  x->W = W;
  x->bg = background == PCV_XRAY_BG_TRANSPARENT ? 0x00ffffffu : 0xffffffffu;
  x->geo.deepest_level = plan.deepest;
  std::memcpy(x->geo.rect, plan.rect, sizeof(plan.rect));
  for (uint32_t k = 0; k < num_parts; ++k) {
    uint64_t n = 0;
    pcv_xray_nodes(parts[k], &n, 0, nullptr, nullptr);
    const uint64_t at = x->node_index.size();
    x->parts.push_back(XrayPartRef{parts[k], parts[k]->serial, at, n});
    x->node_level.resize(at + n);
    x->node_index.resize(at + n);
    pcv_xray_nodes(parts[k], &n, n, x->node_level.data() + at, x->node_index.data() + at);
  }
  // the level array of the roots: those of built parts first (device to device), then those of opened parts (decoded
  // into one pinned block, one upload)
  std::vector<uint32_t> order;
  for (int opened = 0; opened < 2; ++opened)
    for (uint32_t k = 0; k < num_parts; ++k)
      if (plan.root_pos[k] >= 0 && (parts[k]->kind == kXrayOpened) == (opened == 1)) order.push_back(k);
  uint64_t num_opened = 0;
  std::vector<uint64_t> base;
  for (uint32_t k : order) {
    base.push_back(plan.root_index[k]);
    num_opened += parts[k]->kind == kXrayOpened;
  }
  auto undo = [&](int code) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    pcv_xray_free(x);
    return code;
  };
  if (plan.L > 0) {
    if (hipSetDevice(ctx->device) != hipSuccess) return undo(ctx->fail(PCV_E_HIP, "hipSetDevice"));
    PcvScratch sc(ctx);
    uint8_t* d_stage = nullptr;
    uint8_t* host = nullptr;
    if ((rc = sc.get(&d_stage, base.size() * tile_bytes)))
      return undo(ctx->fail(PCV_E_OOM, "xray merge: no device memory for " + std::to_string(base.size()) + " root tiles"));
    if (num_opened && (rc = ctx->host_alloc((void**)&host, num_opened * tile_bytes))) return undo(rc);
    const uint64_t num_built = base.size() - num_opened;
    for (uint64_t i = 0; !rc && i < num_opened; ++i) {
      pcv_xray* part = parts[order[num_built + i]];
      rc = opened_node_to_host(part, (uint64_t)plan.root_pos[order[num_built + i]], host + i * tile_bytes);
      if (rc && !part->ctx) ctx->fail(rc, pcv_host_last_error());
    }
    if (!rc) {
      PcvProf prof(ctx, PCV_K_XRAY_MERGE_STAGE);
      for (uint64_t i = 0; !rc && i < num_built; ++i) {
        pcv_xray* part = parts[order[i]];
        if (part->kind == kXrayBuilt) {
          rc = queue_node_images(part, (uint64_t)plan.root_pos[order[i]], 1, d_stage + i * tile_bytes, hipMemcpyDeviceToDevice);
        } else {  // a merged part: through its own parts
          rc = xray_node_images(part, (uint64_t)plan.root_pos[order[i]], 1, PCV_MEM_DEVICE, d_stage + i * tile_bytes);
        }
      }
      if (!rc && num_opened &&
          hipMemcpyAsync(d_stage + num_built * tile_bytes, host, num_opened * tile_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = ctx->fail(PCV_E_HIP, "xray merge: root tile upload");
    }
    XrayLevels lv;
    if (!rc)
      rc = xray_build_levels(ctx, W, x->bg, base, plan.L, 0, reinterpret_cast<const uint32_t*>(d_stage), PCV_K_XRAY_MERGE_PARENT, &lv);
    else
      (void)hipStreamSynchronize(ctx->stream);
    if (host) ctx->host_release(host);  // the upload has completed: xray_build_levels returns after a stream sync
    if (rc) return undo(rc);
    x->d_parents = lv.d_parents;
    x->parent_level.swap(lv.plevel);
    x->parent_index.swap(lv.pindex);
    x->level_first.swap(lv.first);
    x->node_level.insert(x->node_level.end(), x->parent_level.begin(), x->parent_level.end());
    x->node_index.insert(x->node_index.end(), x->parent_index.begin(), x->parent_index.end());
  }
  x->parents_built = true;
  for (size_t i = 0; i < x->node_index.size(); ++i)
    if (x->node_level[i] == plan.deepest) {
      x->created.push_back(x->geo.index.size());
      x->geo.index.push_back(x->node_index[i]);
    }
  ctx->prof_resolve();
  *out = x;
  return PCV_OK;
}

static bool same_directory(const std::string& a, const std::string& b) {  // copy_images :29: canonicalize() of both
  char* ra = realpath(a.c_str(), nullptr);
  char* rb = realpath(b.c_str(), nullptr);
  const bool same = ra && rb && std::strcmp(ra, rb) == 0;
  std::free(ra);
  std::free(rb);
  return same;
}

static int xray_node_files(pcv_xray* x, uint64_t first, uint64_t count, int mode, bool parallel, const XrayFileSink& sink);

// pcv_xray_write_dir_ex of a merged quadtree
static int xray_write_merged(pcv_xray* x, const char* directory, int mode) {
  pcv_ctx* ctx = x->ctx;
  for (const XrayPartRef& r : x->parts)
    if (!xray_part_alive(r)) return ctx->fail(PCV_E_INVALID, "xray: a part of this merged quadtree was freed before it");
  const std::string dir(directory);
  ::mkdir(dir.c_str(), 0777);
  struct stat st;
  if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return ctx->fail(PCV_E_IO, "cannot create directory " + dir);
  const int dirfd = open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
  if (dirfd < 0) return ctx->fail(PCV_E_IO, "cannot open directory " + dir);
  const uint32_t W = x->W;
  const uint64_t tile_bytes = 4ull * W * W, n = x->node_index.size();
  int rc = PCV_OK;
  // copy_images: the files of opened parts, byte for byte; every other node is fetched and encoded
  std::vector<uint64_t> encode;
  std::vector<uint8_t> file;
  for (const XrayPartRef& r : x->parts) {
    const bool copy = r.part->kind == kXrayOpened;
    const bool same = copy && same_directory(r.part->dir, dir);
    for (uint64_t i = 0; !rc && i < r.count; ++i) {
      if (!copy) {
        encode.push_back(r.first + i);
        continue;
      }
      if (same) continue;
      const std::string name = quad_name(x->node_level[r.first + i], x->node_index[r.first + i]) + ".png";
      if (!read_file(r.part->dir + "/" + name, file)) rc = ctx->fail(PCV_E_IO, "cannot read " + r.part->dir + "/" + name);
      else if (!write_at(dirfd, name, file.data(), file.size())) rc = ctx->fail(PCV_E_IO, "cannot write " + dir + "/" + name);
    }
  }
  for (uint64_t i = n - x->parent_index.size(); i < n; ++i) encode.push_back(i);
  if (mode == PCV_XRAY_PNG_DEFLATE) {  // compressed where the images live; the threads below only write
    std::mutex err_mu;
    std::string first_error;
    const XrayFileSink write = [&](uint64_t node, const uint8_t* file, uint64_t len) {
      const std::string name = quad_name(x->node_level[node], x->node_index[node]) + ".png";
      if (write_at(dirfd, name, file, len)) return true;
      std::lock_guard<std::mutex> g(err_mu);
      if (first_error.empty()) first_error = "cannot write " + dir + "/" + name;
      return false;
    };
    for (uint64_t i = 0; !rc && i < encode.size();) {  // runs of consecutive nodes in one call
      uint64_t k = 1;
      while (i + k < encode.size() && encode[i + k] == encode[i] + k) ++k;
      rc = xray_node_files(x, encode[i], k, mode, true, write);
      if (rc == PCV_E_IO && !first_error.empty()) ctx->fail(rc, first_error);
      i += k;
    }
    encode.clear();
  }
  const uint64_t per_chunk = std::max<uint64_t>(1, ctx->xray_chunk_bytes / tile_bytes);
  std::vector<uint8_t> images(std::min<uint64_t>(per_chunk, std::max<uint64_t>(encode.size(), 1)) * tile_bytes);
  unsigned nthreads = std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
  for (uint64_t f = 0; !rc && f < encode.size(); f += per_chunk) {
    const uint64_t c = std::min<uint64_t>(per_chunk, encode.size() - f);
    for (uint64_t i = 0; !rc && i < c;) {  // runs of consecutive nodes in one call
      uint64_t k = 1;
      while (i + k < c && encode[f + i + k] == encode[f + i] + k) ++k;
      rc = xray_node_images(x, encode[f + i], k, PCV_MEM_HOST, images.data() + i * tile_bytes);
      i += k;
    }
    if (rc) break;
    std::atomic<uint64_t> next{0};
    std::atomic<int> failed{0};
    std::string first_error;
    std::mutex err_mu;
    auto worker = [&]() {
      std::vector<uint8_t> png(pcv_png_stored_size(W, W));
      for (;;) {
        const uint64_t i = next.fetch_add(1);
        if (i >= c || failed.load()) return;
        const uint64_t node = encode[f + i];
        const std::string name = quad_name(x->node_level[node], x->node_index[node]) + ".png";
        pcv_png_stored_encode(images.data() + i * tile_bytes, W, W, png.data());
        if (!write_at(dirfd, name, png.data(), png.size())) {
          std::lock_guard<std::mutex> g(err_mu);
          if (!failed.exchange(1)) first_error = "cannot write " + dir + "/" + name;
        }
      }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < (unsigned)std::min<uint64_t>(nthreads, c); ++t) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
    if (failed.load()) rc = ctx->fail(PCV_E_IO, first_error);
  }
  std::string err;
  if (!rc && !write_meta_file(dirfd, dir, 0, 0, x->geo.rect, x->geo.deepest_level, W, x->node_level, x->node_index, &err))
    rc = ctx->fail(PCV_E_IO, err);
  ::close(dirfd);
  return rc;
}

static int xray_write_built_deflate(pcv_xray* x, int dirfd, const std::string& dir);

extern "C" int pcv_xray_write_dir(pcv_xray* x, const char* directory) { return pcv_xray_write_dir_ex(x, directory, PCV_XRAY_PNG_STORED); }

extern "C" int pcv_xray_write_dir_ex(pcv_xray* x, const char* directory, int mode) {
  if (!x) return PCV_E_INVALID;
  if (!directory) return xray_fail(x, PCV_E_INVALID, "null directory");
  if (mode != PCV_XRAY_PNG_STORED && mode != PCV_XRAY_PNG_DEFLATE) return xray_fail(x, PCV_E_INVALID, "xray: unknown PNG mode");
  if (x->kind == kXrayOpened)
    return xray_fail(x, PCV_E_INVALID, "xray: an opened quadtree is written through pcv_xray_merge (its files are already a directory)");
  if (mode == PCV_XRAY_PNG_DEFLATE && x->W > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return xray_fail(x, PCV_E_INVALID, "xray: compressed tiles are at most " + std::to_string(PCV_XRAY_PNG_DEFLATE_MAX_EDGE) + " pixels wide");
  if (x->kind == kXrayMerged) return xray_write_merged(x, directory, mode);
  pcv_ctx* ctx = x->ctx;
  const uint64_t nc = x->created.size(), n = nc + x->parent_index.size();
  if (!x->parents_built && nc && x->root_level < x->geo.deepest_level)
    return ctx->fail(PCV_E_INVALID, "xray: parent levels are not built (pcv_xray_build_parents)");
  const std::string dir(directory);
  ::mkdir(dir.c_str(), 0777);  // build_xray_quadtree :565 ignores errors: the directory may be there
  struct stat st;
  if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return ctx->fail(PCV_E_IO, "cannot create directory " + dir);
  const int dirfd = open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
  if (dirfd < 0) return ctx->fail(PCV_E_IO, "cannot open directory " + dir);
  // the node images come down in chunks through two pinned buffers: chunk k + 1 is copied while a pool of host threads
  // encodes and writes chunk k (no HIP call in a writer thread)
  const uint32_t W = x->W;
  const uint64_t tile_bytes = 4ull * W * W;
  const uint64_t per_chunk = std::max<uint64_t>(1, std::min<uint64_t>(n, ctx->xray_chunk_bytes / tile_bytes));
  const uint64_t chunks = mode == PCV_XRAY_PNG_DEFLATE ? 0 : (n + per_chunk - 1) / per_chunk;
  uint8_t* host[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  int rc = PCV_OK;
  if (mode == PCV_XRAY_PNG_DEFLATE && n) rc = xray_write_built_deflate(x, dirfd, dir);
  if (n && chunks) {
    if (hipSetDevice(ctx->device) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "hipSetDevice");
    for (int k = 0; !rc && k < 2 && (uint64_t)k < chunks; ++k) {
      rc = ctx->host_alloc((void**)&host[k], per_chunk * tile_bytes);
      if (!rc && hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "hipEventCreate");
    }
  }
  unsigned nthreads = std::thread::hardware_concurrency();
  if (nthreads == 0) nthreads = 4;
  if (nthreads > 8) nthreads = 8;  // one directory: more writers queue on its lock (pcv_io.cpp)
  std::atomic<int> failed{0};
  std::string first_error;
  std::mutex err_mu;
  auto queue = [&](uint64_t k) -> int {
    const uint64_t f = k * per_chunk, c = std::min(per_chunk, n - f);
    int r = queue_node_images(x, f, c, host[k & 1], hipMemcpyDeviceToHost);
    if (!r && hipEventRecord(ev[k & 1], ctx->stream) != hipSuccess) r = ctx->fail(PCV_E_HIP, "hipEventRecord");
    return r;
  };
  if (!rc && chunks) rc = queue(0);
  for (uint64_t k = 0; !rc && k < chunks; ++k) {  // stored mode only: in deflate mode there are no chunks here
    if (k + 1 < chunks && (rc = queue(k + 1))) break;  // its buffer's writers (chunk k - 1) have finished
    if (hipEventSynchronize(ev[k & 1]) != hipSuccess) {
      rc = ctx->fail(PCV_E_HIP, "xray: image download failed");
      break;
    }
    const uint64_t f = k * per_chunk, c = std::min(per_chunk, n - f);
    const uint8_t* buf = host[k & 1];
    std::atomic<uint64_t> next{0};
    auto worker = [&]() {
      std::vector<uint8_t> png(pcv_png_stored_size(W, W));
      for (;;) {
        const uint64_t i = next.fetch_add(1);
        if (i >= c || failed.load()) return;
        const uint64_t node = f + i;
        const std::string name = node < nc ? quad_name(x->geo.deepest_level, x->geo.index[x->created[node]]) + ".png"
                                           : quad_name(x->parent_level[node - nc], x->parent_index[node - nc]) + ".png";
        pcv_png_stored_encode(buf + i * tile_bytes, W, W, png.data());
        if (!write_at(dirfd, name, png.data(), png.size())) {
          std::lock_guard<std::mutex> g(err_mu);
          if (!failed.exchange(1)) first_error = "cannot write " + dir + "/" + name;
        }
      }
    };
    const unsigned nt = (unsigned)std::min<uint64_t>(nthreads, c);
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; ++t) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
    if (failed.load()) break;
  }
  if (n) (void)hipStreamSynchronize(ctx->stream);
  for (int k = 0; k < 2; ++k) {
    if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (host[k]) ctx->host_release(host[k]);
  }
  if (!rc && failed.load()) rc = ctx->fail(PCV_E_IO, first_error);
  if (!rc) {
    double rect[3];
    built_root_rect(x, rect);
    std::vector<uint32_t> level(n);
    std::vector<uint64_t> index(n);
    pcv_xray_nodes(x, nullptr, n, level.data(), index.data());
    std::string err;
    if (!write_meta_file(dirfd, dir, x->root_level, x->root_index, rect, x->geo.deepest_level, W, level, index, &err)) rc = ctx->fail(PCV_E_IO, err);
  }
  ::close(dirfd);
  return rc;
}

// ---- compressed tiles: the host side of pcv_xray_png.hip ----------------------------------------------------------------
namespace {

template <typename Fn>
void xray_parallel_for(uint64_t n, bool parallel, Fn&& fn) {
  unsigned nt = parallel ? std::min(8u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
  nt = (unsigned)std::min<uint64_t>(nt, n);
  std::atomic<uint64_t> next{0};
  auto worker = [&]() {
    for (uint64_t i; (i = next.fetch_add(1)) < n;) fn(i);
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nt; ++t) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
}

// One chunk in flight on the device and one on the host: the scratch of pcv_xray_png_launch and two pinned buffers, each
// for the compacted streams of a chunk and their offsets. Only offsets and compressed bytes are copied down.
struct XrayPngPipe {
  pcv_ctx* ctx = nullptr;
  PcvPngWork wk;
  uint8_t* host[2] = {nullptr, nullptr};
  uint64_t* tab[2] = {nullptr, nullptr};
  hipEvent_t ev_tab[2] = {nullptr, nullptr}, ev_bytes[2] = {nullptr, nullptr};
  int open(pcv_ctx* c, uint32_t W, uint64_t tiles, int buffers) {
    ctx = c;
    int rc = pcv_xray_png_work_alloc(ctx, W, tiles, &wk);
    for (int k = 0; !rc && k < buffers; ++k) {
      if ((rc = ctx->host_alloc((void**)&host[k], tiles * wk.tile_bound)) || (rc = ctx->host_alloc((void**)&tab[k], 8 * (tiles + 1)))) break;
      if (hipEventCreateWithFlags(&ev_tab[k], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&ev_bytes[k], hipEventDisableTiming) != hipSuccess)
        rc = ctx->fail(PCV_E_HIP, "hipEventCreate");
    }
    return rc;
  }
  // kernels of a chunk, then its offsets on their way down
  int launch(int s, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t count) {
    if (int rc = pcv_xray_png_launch(ctx, wk, a, na, b, count)) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(tab[s], wk.offsets, 8 * (count + 1), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipEventRecord(ev_tab[s], ctx->stream));
    return PCV_OK;
  }
  // once the offsets are here: exactly the compressed bytes on their way down
  int fetch(int s, uint64_t count) {
    PCV_HIP_CHECK(ctx, hipEventSynchronize(ev_tab[s]));
    const uint64_t total = tab[s][count];
    if (total > count * wk.tile_bound) return ctx->fail(PCV_E_HIP, "xray: compressed chunk larger than its bound");
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(host[s], wk.out, total, hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipEventRecord(ev_bytes[s], ctx->stream));
    return PCV_OK;
  }
  int wait(int s) {
    PCV_HIP_CHECK(ctx, hipEventSynchronize(ev_bytes[s]));
    return PCV_OK;
  }
  void close() {
    if (!ctx) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (int k = 0; k < 2; ++k) {
      if (ev_tab[k]) (void)hipEventDestroy(ev_tab[k]);
      if (ev_bytes[k]) (void)hipEventDestroy(ev_bytes[k]);
      if (host[k]) ctx->host_release(host[k]);
      if (tab[k]) ctx->host_release(tab[k]);
    }
    pcv_xray_png_work_free(ctx, &wk);
  }
};

// The zlib streams of `count` device tiles, per_chunk at a time: src(f, c, &a, &na, &b) names tiles [f, f + c) for
// pcv_xray_png_launch; use(f, c, streams, offsets) runs on the host while the next chunk is compressed and copied.
template <typename Src, typename Use>
int xray_deflate_chunks(pcv_ctx* ctx, uint32_t W, uint64_t count, uint64_t per_chunk, Src&& src, Use&& use) {
  if (count == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  per_chunk = std::max<uint64_t>(1, std::min(per_chunk, count));
  const uint64_t chunks = (count + per_chunk - 1) / per_chunk;
  XrayPngPipe pipe;
  int rc = pipe.open(ctx, W, per_chunk, chunks > 1 ? 2 : 1);
  auto start = [&](uint64_t k) -> int {
    const uint64_t f = k * per_chunk, c = std::min(per_chunk, count - f);
    const uint8_t *a = nullptr, *b = nullptr;
    uint64_t na = 0;
    src(f, c, &a, &na, &b);
    if (int r = pipe.launch((int)(k & 1), a, na, b, c)) return r;
    return pipe.fetch((int)(k & 1), c);
  };
  if (!rc) rc = start(0);
  for (uint64_t k = 0; !rc && k < chunks; ++k) {
    if (k + 1 < chunks && (rc = start(k + 1))) break;  // its buffer's users (chunk k - 1) have finished
    if ((rc = pipe.wait((int)(k & 1)))) break;
    const uint64_t f = k * per_chunk, c = std::min(per_chunk, count - f);
    rc = use(f, c, pipe.host[k & 1], pipe.tab[k & 1]);
  }
  pipe.close();
  return rc;
}

// the device tiles of nodes [f, f + c): a built quadtree's leaves then parents, a merged quadtree's own levels
void xray_device_tiles(const pcv_xray* x, uint64_t f, uint64_t c, const uint8_t** a, uint64_t* na, const uint8_t** b) {
  const uint64_t tile_bytes = 4ull * x->W * x->W;
  if (x->kind == kXrayMerged) {
    *na = 0;
    *b = reinterpret_cast<const uint8_t*>(x->d_parents) + (f - (x->node_index.size() - x->parent_index.size())) * tile_bytes;
    return;
  }
  const uint64_t nc = x->created.size();
  *na = f < nc ? std::min(c, nc - f) : 0;
  *a = reinterpret_cast<const uint8_t*>(x->d_images) + f * tile_bytes;
  *b = reinterpret_cast<const uint8_t*>(x->d_parents) + (f + *na - nc) * tile_bytes;
}

// nodes [first, first + count) whose images are on x's device, encoded in `mode`, each file to the sink
int xray_device_node_files(pcv_xray* x, uint64_t first, uint64_t count, int mode, bool parallel, const XrayFileSink& sink) {
  pcv_ctx* ctx = x->ctx;
  const uint32_t W = x->W;
  const uint64_t tile_bytes = 4ull * W * W;
  const uint64_t per_chunk = std::max<uint64_t>(1, std::min(count, ctx->xray_chunk_bytes / tile_bytes));
  std::atomic<int> failed{0};
  if (mode == PCV_XRAY_PNG_DEFLATE) {
    const int rc = xray_deflate_chunks(
        ctx, W, count, per_chunk,
        [&](uint64_t f, uint64_t c, const uint8_t** a, uint64_t* na, const uint8_t** b) { xray_device_tiles(x, first + f, c, a, na, b); },
        [&](uint64_t f, uint64_t c, const uint8_t* streams, const uint64_t* offs) {
          xray_parallel_for(c, parallel, [&](uint64_t i) {
            if (failed.load()) return;
            std::vector<uint8_t> png(kPcvPngWrap + offs[i + 1] - offs[i]);
            pcv_png_wrap(W, W, streams + offs[i], offs[i + 1] - offs[i], png.data());
            if (!sink(first + f + i, png.data(), png.size())) failed.store(1);
          });
          return failed.load() ? PCV_E_IO : PCV_OK;
        });
    return rc;
  }
  std::vector<uint8_t> images(per_chunk * tile_bytes);
  for (uint64_t f = 0; f < count; f += per_chunk) {
    const uint64_t c = std::min(per_chunk, count - f);
    if (int rc = xray_node_images(x, first + f, c, PCV_MEM_HOST, images.data())) return rc;
    xray_parallel_for(c, parallel, [&](uint64_t i) {
      if (failed.load()) return;
      std::vector<uint8_t> png(pcv_png_stored_size(W, W));
      pcv_png_stored_encode(images.data() + i * tile_bytes, W, W, png.data());
      if (!sink(first + f + i, png.data(), png.size())) failed.store(1);
    });
    if (failed.load()) return PCV_E_IO;
  }
  return PCV_OK;
}

}  // namespace

// the files of nodes [first, first + count) of any kind of quadtree: opened nodes as their files are, the others encoded
static int xray_node_files(pcv_xray* x, uint64_t first, uint64_t count, int mode, bool parallel, const XrayFileSink& sink) {
  if (count == 0) return PCV_OK;
  if (x->kind == kXrayBuilt) return xray_device_node_files(x, first, count, mode, parallel, sink);
  if (x->kind == kXrayOpened) {
    std::vector<uint8_t> file;
    for (uint64_t i = first; i < first + count; ++i) {
      const std::string path = x->dir + "/" + quad_name(x->node_level[i], x->node_index[i]) + ".png";
      if (!read_file(path, file)) return xray_fail(x, PCV_E_IO, "xray: cannot read " + path);
      if (!sink(i, file.data(), file.size())) return PCV_E_IO;
    }
    return PCV_OK;
  }
  pcv_ctx* ctx = x->ctx;
  for (const XrayPartRef& r : x->parts)
    if (!xray_part_alive(r)) return ctx->fail(PCV_E_INVALID, "xray: a part of this merged quadtree was freed before it");
  uint64_t at = first;
  const uint64_t end = first + count;
  for (const XrayPartRef& r : x->parts) {
    if (at >= end) break;
    if (at >= r.first + r.count || r.count == 0) continue;
    const uint64_t k = std::min(end, r.first + r.count) - at;
    const uint64_t shift = r.first;
    const int rc = xray_node_files(r.part, at - r.first, k, mode, parallel,
                                   [&](uint64_t node, const uint8_t* file, uint64_t len) { return sink(node + shift, file, len); });
    if (rc) return r.part->ctx == ctx || rc == PCV_E_IO ? rc : ctx->fail(rc, r.part->ctx ? r.part->ctx->last_error : pcv_host_last_error());
    at += k;
  }
  return at < end ? xray_device_node_files(x, at, end - at, mode, parallel, sink) : PCV_OK;
}

// pcv_xray_write_dir_ex of a built quadtree in deflate mode: compressed chunks come down, the writer threads wrap and write
static int xray_write_built_deflate(pcv_xray* x, int dirfd, const std::string& dir) {
  const uint64_t nc = x->created.size(), n = nc + x->parent_index.size();
  std::mutex err_mu;
  std::string first_error;
  const int rc = xray_node_files(x, 0, n, PCV_XRAY_PNG_DEFLATE, true, [&](uint64_t node, const uint8_t* file, uint64_t len) {
    const std::string name = node < nc ? quad_name(x->geo.deepest_level, x->geo.index[x->created[node]]) + ".png"
                                       : quad_name(x->parent_level[node - nc], x->parent_index[node - nc]) + ".png";
    if (write_at(dirfd, name, file, len)) return true;
    std::lock_guard<std::mutex> g(err_mu);
    if (first_error.empty()) first_error = "cannot write " + dir + "/" + name;
    return false;
  });
  return rc == PCV_E_IO && !first_error.empty() ? x->ctx->fail(rc, first_error) : rc;
}

namespace {
// files appended to a caller's buffer with their offsets; out == nullptr: the offsets alone
struct XrayPngAppend {
  uint8_t* out;
  uint64_t capacity, at = 0, index = 0;
  uint64_t* offsets;
  bool fits = true;
  bool take(const uint8_t* file, uint64_t len) {
    offsets[index++] = at;
    if (out && len <= capacity - std::min(capacity, at)) std::memcpy(out + at, file, len);
    else if (out) fits = false;
    at += len;
    offsets[index] = at;
    return true;
  }
};
}  // namespace

extern "C" int pcv_xray_node_pngs(pcv_xray* x, uint64_t first, uint64_t count, int mode, uint64_t capacity, uint8_t* out, uint64_t* offsets) {
  if (!x) return PCV_E_INVALID;
  uint64_t n = 0;
  pcv_xray_nodes(x, &n, 0, nullptr, nullptr);
  if (first > n || count > n - first) return xray_fail(x, PCV_E_INVALID, "xray: node range past the end");
  if (mode != PCV_XRAY_PNG_STORED && mode != PCV_XRAY_PNG_DEFLATE) return xray_fail(x, PCV_E_INVALID, "xray: unknown PNG mode");
  if (!offsets) return xray_fail(x, PCV_E_INVALID, "null offsets");
  if (mode == PCV_XRAY_PNG_DEFLATE && x->kind != kXrayOpened && x->W > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return xray_fail(x, PCV_E_INVALID, "xray: compressed tiles are at most " + std::to_string(PCV_XRAY_PNG_DEFLATE_MAX_EDGE) + " pixels wide");
  offsets[0] = 0;
  XrayPngAppend app{out, capacity};
  app.offsets = offsets;
  const int rc = xray_node_files(x, first, count, mode, false, [&](uint64_t, const uint8_t* file, uint64_t len) { return app.take(file, len); });
  if (rc) return rc;
  if (!app.fits) return xray_fail(x, PCV_E_INVALID, "xray: capacity below the " + std::to_string(app.at) + " bytes of these files");
  return PCV_OK;
}

extern "C" int pcv_xray_png_encode_tiles(pcv_ctx* ctx, const uint8_t* rgba, int mem, uint32_t w, uint64_t count, uint64_t chunk_tiles,
                                         uint64_t capacity, uint8_t* out, uint64_t* offsets) {
  if (!ctx) return PCV_E_INVALID;
  if (!offsets || (count && !rgba) || w == 0) return ctx->fail(PCV_E_INVALID, "xray: bad arguments to pcv_xray_png_encode_tiles");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (w > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return ctx->fail(PCV_E_INVALID, "xray: compressed tiles are at most " + std::to_string(PCV_XRAY_PNG_DEFLATE_MAX_EDGE) + " pixels wide");
  offsets[0] = 0;
  if (count == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint64_t tile_bytes = 4ull * w * w;
  PcvScratch sc(ctx);
  const uint8_t* tiles = rgba;
  if (mem == PCV_MEM_HOST) {
    uint8_t* d = nullptr;
    if (int rc = sc.get(&d, count * tile_bytes)) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d, rgba, count * tile_bytes, hipMemcpyHostToDevice, ctx->stream));
    tiles = d;
  }
  XrayPngAppend app{out, capacity};
  app.offsets = offsets;
  const uint64_t per_chunk = chunk_tiles ? chunk_tiles : std::max<uint64_t>(1, ctx->xray_chunk_bytes / tile_bytes);
  const int rc = xray_deflate_chunks(
      ctx, w, count, per_chunk,
      [&](uint64_t f, uint64_t, const uint8_t** a, uint64_t* na, const uint8_t** b) {
        *na = 0;
        *a = nullptr;
        *b = tiles + f * tile_bytes;
      },
      [&](uint64_t, uint64_t c, const uint8_t* streams, const uint64_t* offs) {
        std::vector<uint8_t> png;
        for (uint64_t i = 0; i < c; ++i) {
          png.resize(kPcvPngWrap + offs[i + 1] - offs[i]);
          pcv_png_wrap(w, w, streams + offs[i], offs[i + 1] - offs[i], png.data());
          app.take(png.data(), png.size());
        }
        return PCV_OK;
      });
  if (rc) return rc;
  if (!app.fits) return ctx->fail(PCV_E_INVALID, "xray: capacity below the " + std::to_string(app.at) + " bytes of these files");
  return PCV_OK;
}

extern "C" int pcv_ctx_set_xray_chunk_bytes(pcv_ctx* ctx, uint64_t bytes) {
  if (!ctx) return PCV_E_INVALID;
  ctx->xray_chunk_bytes = bytes ? bytes : 64ull << 20;
  return PCV_OK;
}
