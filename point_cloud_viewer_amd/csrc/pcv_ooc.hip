// pcv_ooc.hip — out-of-core build: a stream of PointsBatches larger than the device goes through ONE GPU to the reference's
// octree directory (build_octree, src/octree/generation.rs:289-403, streams any number of points through node files).
//
// It rests on the three facts the sharded build (point_cloud_viewer_amd/distributed.py) relies on: the level-2 bucket of a point
// depends only on the point and the global root cube; every node from level 2 down is built from one bucket's points in input
// order and is final whatever else happens; the root and the level-1 nodes can be assembled from partial builds once the 72
// global stream lengths are known (pcv_build_top_streams / pcv_top_layout). Here the "ranks" are partitions built one after
// the other on the same device, and the points between the two phases wait in host memory:
//
//   phase 1 (pcv_ooc_append)  every batch goes up through the context's pinned ring; ooc_count / ooc_scan / ooc_scatter write it
//                             as 64 stable bucket runs (the level-1 chain state, 16 B per point, where level 1 is Float32-coded;
//                             the raw planes, 27 B, otherwise) plus, per root octant, the level-2 digits of its points in input
//                             order; the runs come back into per-bucket host spills, each in global input order;
//   plan (pcv_ooc_plan)       the 64 global counts give the level-1 split mask (plan_buckets' rule) and a grouping of units —
//                             single buckets under split level-1 nodes, whole octants otherwise — into partitions of at most
//                             max_points_per_pass points;
//   phase 2 (pcv_ooc_finish)  topology pass: every partition is built up to pcv_build_top_streams; the summed lengths give the
//                             global top layout; build pass: every partition again, pcv_build_finish(layout), its nodes of
//                             level >= 2 written, its slots of the global-size root / level-1 nodes OR-ed into one device
//                             accumulator; then the root / level-1 files and meta.pb, last.
//
// An unsplit level-1 node is a leaf whose points must keep their input order across its 8 buckets: the octant's level-2 digit
// sequence (1 B per point, kept only while the octant could still stay unsplit, i.e. holds <= max_points_per_node points)
// interleaves the 8 bucket spills again. When no level-1 node can be split at all, the buckets are the root octants themselves.
#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pcv_chain_dev.h"

namespace {

constexpr int kOocTile = 4096;             // points per workgroup: 4 waves x 16 rows x 64 lanes, wave-striped
constexpr uint64_t kOocSub = 1u << 20;     // points per ring chunk: 31 B each + alignment gaps fit 32 MiB
static_assert(kOocSub * 31 + 64 <= pcv_ctx::kRingChunk, "a piece must fit one ring chunk");

// lanes of the wave whose value agrees with this lane's on the low `bits` bits (match-any by ballots)
template <int BITS>
__device__ __forceinline__ uint64_t ooc_match(uint32_t v, bool valid) {
  uint64_t peers = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < BITS; ++bit) {
    const uint64_t m = __ballot((v >> bit) & 1u);
    peers &= ((v >> bit) & 1u) ? m : ~m;
  }
  return peers;
}

// bucket = 8 * d1 + d2 along the chain route_plan_kernel follows (pcv_chain.hip): the fast Float32 level step with the tie rule
// where the table and the point are tame, the guarded level steps otherwise; octants_only: d1 << 3 (three comparisons)
__device__ __forceinline__ uint32_t ooc_bucket(const PcvLevels& lv, bool fast, bool octants_only, double px, double py, double pz) {
  double mx = lv.root_min[0], my = lv.root_min[1], mz = lv.root_min[2];
  double cx, cy, cz;
  if (octants_only) return pcv_chain_bits(lv.edge[0], px, py, pz, mx, my, mz).digit() << 3;
  uint32_t b = 0;
  if (fast && pcv_point_is_tame(px, py, pz)) {
    const PcvOctBits b1 = pcv_chain_bits(lv.edge[0], px, py, pz, mx, my, mz);
    pcv_chain_apply_bits_t<PCV_ENC_FLOAT32, false>(b1, lv.edge[1], PcvRecip{lv.inv_edge[1], lv.inv_edge_lo[1]}, px, py, pz, mx, my, mz, cx, cy, cz);
    PcvOctBits b2 = pcv_bits_from_codes(0.5, cx, cy, cz);
    if (__builtin_expect(pcv_f32_code_tie(cx, cy, cz), 0)) b2 = pcv_chain_bits(lv.edge[1], px, py, pz, mx, my, mz);
    return (b1.digit() << 3) | b2.digit();
  }
  for (int l = 1; l <= lv.nlevels && l <= 2; ++l)
    b = (b << 3) | pcv_chain_level<true>(lv.enc[l], lv.edge[l - 1], lv.edge[l], PcvRecip{lv.inv_edge[l], lv.inv_edge_lo[l]}, px, py, pz, mx, my, mz, cx, cy, cz);
  if (lv.nlevels < 2) b <<= 3;
  return b;
}

// pass 1: bucket byte of every point + the bucket histogram of every tile. One LDS add per distinct bucket per wave and row
// (the leader of each match-any group), into the wave's own row of counters: no atomics, no cliff on coherent input.
__global__ __launch_bounds__(256) void ooc_count_kernel(PcvLevels lv, bool fast, bool octants_only, uint32_t n, const double* __restrict__ xyz,
                                                         uint8_t* __restrict__ bucket, uint32_t* __restrict__ tile_hist /* [tiles][64] */) {
  __shared__ uint32_t wcnt[4][64];
  reinterpret_cast<uint32_t*>(wcnt)[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  const uint32_t base = blockIdx.x * kOocTile + wave * 1024 + lane;
#pragma unroll 4
  for (int i = 0; i < 16; ++i) {
    const uint32_t idx = base + i * 64;
    const bool valid = idx < n;
    uint32_t b = 0;
    if (valid) {
      b = ooc_bucket(lv, fast, octants_only, xyz[3 * (uint64_t)idx], xyz[3 * (uint64_t)idx + 1], xyz[3 * (uint64_t)idx + 2]);
      bucket[idx] = (uint8_t)b;
    }
    const uint64_t peers = ooc_match<6>(b, valid);
    if (valid && (peers & lane_lt) == 0) wcnt[wave][b] += (uint32_t)__popcll(peers);
  }
  __syncthreads();
  if (threadIdx.x < 64)
    tile_hist[(uint64_t)blockIdx.x * 64 + threadIdx.x] = wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
}

// pass 2 (one workgroup of 64 lanes): where every tile's share of every bucket run starts, and of every octant's digit run (the
// octant's runs and its digit run cover the same range: buckets 8c .. 8c + 7 are consecutive); the 64 counts
__global__ __launch_bounds__(64) void ooc_scan_kernel(const uint32_t* __restrict__ tile_hist, uint32_t ntiles, uint32_t* __restrict__ tile_base,
                                                       uint32_t* __restrict__ tile_obase /* [tiles][8] */, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t total[64];
  const uint32_t b = threadIdx.x;
  uint32_t acc = 0;
  for (uint32_t t = 0; t < ntiles; ++t) {
    const uint32_t v = tile_hist[(uint64_t)t * 64 + b];
    tile_base[(uint64_t)t * 64 + b] = acc;
    acc += v;
  }
  total[b] = acc;
  counts[b] = acc;
  __syncthreads();
  uint32_t start = 0;
  for (uint32_t k = 0; k < b; ++k) start += total[k];
  for (uint32_t t = 0; t < ntiles; ++t) tile_base[(uint64_t)t * 64 + b] += start;
  if (b < 8) {
    uint32_t o = 0;  // octant b's runs (buckets 8b .. 8b + 7) start where bucket 8b's does
    for (uint32_t k = 0; k < 8 * b; ++k) o += total[k];
    for (uint32_t t = 0; t < ntiles; ++t) {
      tile_obase[(uint64_t)t * 8 + b] = o;
      uint32_t s = 0;
      for (uint32_t d = 0; d < 8; ++d) s += tile_hist[(uint64_t)t * 64 + 8 * b + d];
      o += s;
    }
  }
}

struct OocPlanes {
  void* p[5];  // routed: cx, cy, cz, oct_rgb (u32), intensity (f32); raw: x, y, z (f64), rgb (3 B), intensity (f32)
};

// pass 3: every point at its stable place in its bucket run (the level-1 state computed from the coordinates and the known
// digit, as route_scatter_kernel does, or the raw planes), and its level-2 digit at its stable place in its octant's digit run
__global__ __launch_bounds__(256) void ooc_scatter_kernel(PcvLevels lv, bool routed, uint32_t n, const double* __restrict__ xyz,
                                                           const uint8_t* __restrict__ rgb, const float* __restrict__ inten,
                                                           const uint8_t* __restrict__ bucket, const uint32_t* __restrict__ tile_base,
                                                           const uint32_t* __restrict__ tile_obase, OocPlanes out, uint8_t* __restrict__ oseq) {
  __shared__ uint32_t wcnt[4][64];
  __shared__ uint32_t run[4][64];
  __shared__ uint32_t orun[4][8];
  reinterpret_cast<uint32_t*>(wcnt)[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  const uint32_t base = blockIdx.x * kOocTile + wave * 1024 + lane;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t idx = base + i * 64;
    const bool valid = idx < n;
    const uint32_t b = valid ? bucket[idx] : 0u;
    const uint64_t peers = ooc_match<6>(b, valid);
    if (valid && (peers & lane_lt) == 0) wcnt[wave][b] += (uint32_t)__popcll(peers);
  }
  __syncthreads();
  {
    const uint32_t w = threadIdx.x >> 6, b = threadIdx.x & 63;
    uint32_t r = tile_base[(uint64_t)blockIdx.x * 64 + b];
    for (uint32_t k = 0; k < w; ++k) r += wcnt[k][b];
    run[w][b] = r;
    if (threadIdx.x < 32) {
      const uint32_t ow = threadIdx.x >> 3, o = threadIdx.x & 7;
      uint32_t s = tile_obase[(uint64_t)blockIdx.x * 8 + o];
      for (uint32_t k = 0; k < ow; ++k)
        for (uint32_t d = 0; d < 8; ++d) s += wcnt[k][8 * o + d];
      orun[ow][o] = s;
    }
  }
  __syncthreads();
  const double e1 = lv.edge[1];
  const PcvRecip r1{lv.inv_edge[1], lv.inv_edge_lo[1]};
  for (int i = 0; i < 16; ++i) {
    const uint32_t idx = base + i * 64;
    const bool valid = idx < n;
    const uint32_t b = valid ? bucket[idx] : 0u, o = b >> 3;  // (a second read of the byte: it is in L2)
    const uint64_t peers = ooc_match<6>(b, valid), opeers = ooc_match<3>(o, valid);
    // every lane reads its group's running offset before the group's leader moves it on (one wave, program order)
    const uint32_t r = valid ? __hip_atomic_load(&run[wave][b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u;
    const uint32_t orr = valid ? __hip_atomic_load(&orun[wave][o], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0u;
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers & lane_lt) == 0) __hip_atomic_store(&run[wave][b], r + (uint32_t)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (valid && (opeers & lane_lt) == 0) __hip_atomic_store(&orun[wave][o], orr + (uint32_t)__popcll(opeers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_wave_barrier();
    if (!valid) continue;
    const uint32_t pos = r + (uint32_t)__popcll(peers & lane_lt);
    oseq[orr + (uint32_t)__popcll(opeers & lane_lt)] = (uint8_t)(b & 7u);
    const double px = xyz[3 * (uint64_t)idx], py = xyz[3 * (uint64_t)idx + 1], pz = xyz[3 * (uint64_t)idx + 2];
    const uint8_t* c = rgb + 3 * (uint64_t)idx;
    if (routed) {
      const double mx = pcv_step_min(lv.root_min[0], (o & 4u) != 0u, e1), my = pcv_step_min(lv.root_min[1], (o & 2u) != 0u, e1),
                   mz = pcv_step_min(lv.root_min[2], (o & 1u) != 0u, e1);
      double cx, cy, cz;
      if (lv.fast_ok && pcv_point_is_tame(px, py, pz)) {
        cx = pcv_encode_val<PCV_ENC_FLOAT32, false>(px, mx, e1, r1), cy = pcv_encode_val<PCV_ENC_FLOAT32, false>(py, my, e1, r1),
        cz = pcv_encode_val<PCV_ENC_FLOAT32, false>(pz, mz, e1, r1);
      } else {
        cx = pcv_encode_val<PCV_ENC_FLOAT32, true>(px, mx, e1, r1), cy = pcv_encode_val<PCV_ENC_FLOAT32, true>(py, my, e1, r1),
        cz = pcv_encode_val<PCV_ENC_FLOAT32, true>(pz, mz, e1, r1);
      }
      static_cast<uint32_t*>(out.p[0])[pos] = __float_as_uint((float)cx);  // exact: cx is a float value
      static_cast<uint32_t*>(out.p[1])[pos] = __float_as_uint((float)cy);
      static_cast<uint32_t*>(out.p[2])[pos] = __float_as_uint((float)cz);
      static_cast<uint32_t*>(out.p[3])[pos] = o | ((uint32_t)c[0] << 8) | ((uint32_t)c[1] << 16) | ((uint32_t)c[2] << 24);
    } else {
      static_cast<double*>(out.p[0])[pos] = px;
      static_cast<double*>(out.p[1])[pos] = py;
      static_cast<double*>(out.p[2])[pos] = pz;
      uint8_t* d = static_cast<uint8_t*>(out.p[3]) + 3 * (uint64_t)pos;
      d[0] = c[0], d[1] = c[1], d[2] = c[2];
    }
    if (inten) static_cast<float*>(out.p[4])[pos] = inten[idx];
  }
}

// acc |= part, byte-wise over 16-byte words (the slots of the partitions are disjoint, everything else is zero)
__global__ __launch_bounds__(256) void ooc_or_kernel(uint4* __restrict__ acc, const uint4* __restrict__ part, uint64_t words) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (uint64_t)gridDim.x * 256) {
    const uint4 a = acc[i], p = part[i];
    acc[i] = make_uint4(a.x | p.x, a.y | p.y, a.z | p.z, a.w | p.w);
  }
}

inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline uint64_t ceil8(uint64_t v) { return (v + 7) / 8; }

// the bucket-runs pass on device-resident AoS input of n <= 2^32 - 2 points: scratch from the pool, everything on ctx->stream
int ooc_runs(pcv_ctx* ctx, const PcvLevels& lv, bool fast, bool octants_only, bool routed, uint32_t n, const double* xyz, const uint8_t* rgb,
             const float* inten, const OocPlanes& out, uint8_t* oseq, unsigned long long* d_counts) {
  if (n == 0) return PCV_OK;
  PcvScratch sc(ctx);
  const uint32_t ntiles = (n + kOocTile - 1) / kOocTile;
  uint8_t* bucket;
  uint32_t *hist, *tbase, *obase;
  int rc;
  if ((rc = sc.get(&bucket, n)) || (rc = sc.get(&hist, (size_t)ntiles * 64)) || (rc = sc.get(&tbase, (size_t)ntiles * 64)) ||
      (rc = sc.get(&obase, (size_t)ntiles * 8)))
    return rc;
  {
    PcvProf prof(ctx, PCV_K_ROUTE_BUCKET);
    hipLaunchKernelGGL(ooc_count_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, lv, fast, octants_only, n, xyz, bucket, hist);
  }
  hipLaunchKernelGGL(ooc_scan_kernel, dim3(1), dim3(64), 0, ctx->stream, (const uint32_t*)hist, ntiles, tbase, obase, d_counts);
  {
    PcvProf prof(ctx, PCV_K_PARTITION_SCATTER);
    hipLaunchKernelGGL(ooc_scatter_kernel, dim3(ntiles), dim3(256), 0, ctx->stream, lv, routed, n, xyz, rgb, inten, (const uint8_t*)bucket,
                       (const uint32_t*)tbase, (const uint32_t*)obase, out, oseq);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;  // (the scratch goes back to the stream-ordered pool: later users queue behind these kernels)
}

}  // namespace

// ---- the plan (host only, pure) ---------------------------------------------------------------------------------------------
extern "C" int pcv_ooc_plan(const uint64_t counts[64], uint32_t max_points_per_node, int level1_can_split, uint64_t max_points_per_pass,
                            uint32_t partition_of_bucket[64], uint32_t* num_partitions, uint32_t* split_mask, char* err, uint64_t errcap) {
  auto fail = [&](const std::string& m) {
    if (err && errcap) snprintf(err, errcap, "%s", m.c_str());
    return PCV_E_OOM;
  };
  if (!counts || !partition_of_bucket || !num_partitions || !split_mask) return PCV_E_INVALID;
  const uint64_t cap = max_points_per_node ? max_points_per_node : PCV_DEFAULT_MAX_POINTS_PER_NODE;
  uint64_t budget = max_points_per_pass ? max_points_per_pass : PCV_MAX_POINTS_PER_BUILD;
  if (budget > PCV_MAX_POINTS_PER_BUILD) budget = PCV_MAX_POINTS_PER_BUILD;
  *split_mask = 0;
  *num_partitions = 0;
  for (int b = 0; b < 64; ++b) partition_of_bucket[b] = 0xffffffffu;
  uint64_t load = 0;
  uint32_t part = 0;
  bool open = false;
  auto place = [&](uint64_t weight, int first, int nb, const char* what, int which) {
    if (weight > budget) {
      char m[256];
      snprintf(m, sizeof(m), "%s %d holds %llu points, more than max_points_per_pass (%llu); re-bucketing below level 2 is not supported",
               what, which, (unsigned long long)weight, (unsigned long long)budget);
      return fail(m);
    }
    if (open && load + weight > budget) ++part, load = 0;
    open = true;
    load += weight;
    for (int b = first; b < first + nb; ++b)
      if (counts[b]) partition_of_bucket[b] = part;
    return PCV_OK;
  };
  for (int c = 0; c < 8; ++c) {
    uint64_t octant = 0;
    for (int d = 0; d < 8; ++d) octant += counts[c * 8 + d];
    int rc = PCV_OK;
    if (level1_can_split && octant > cap) {
      *split_mask |= 1u << c;
      for (int d = 0; d < 8 && rc == PCV_OK; ++d)
        if (counts[c * 8 + d]) rc = place(counts[c * 8 + d], c * 8 + d, 1, "bucket", c * 8 + d);
    } else if (octant) {
      rc = place(octant, c * 8, 8, "unsplit level-1 octant", c);
    }
    if (rc) return rc;
  }
  *num_partitions = open ? part + 1 : 0;
  return PCV_OK;
}

// distributed.top_layout: the global streams of the top of the tree from the summed stream lengths
extern "C" int pcv_ooc_top_layout(const uint64_t l1[8], const uint64_t l2[64], uint32_t split_mask, pcv_top_layout* out) {
  if (!l1 || !l2 || !out) return PCV_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  for (int c = 0; c < 8; ++c) {
    if ((split_mask >> c) & 1u) {
      uint64_t acc = 0;
      for (int d = 0; d < 8; ++d) {
        if (acc > 0xffffffffull) return PCV_E_INVALID;
        out->l2_offset[c * 8 + d] = (uint32_t)acc;
        acc += ceil8(l2[c * 8 + d]);
      }
      out->l1_stream[c] = acc;
    } else {
      out->l1_stream[c] = l1[c];
    }
  }
  uint64_t acc = 0;
  for (int c = 0; c < 8; ++c) {
    if (acc > 0xffffffffull) return PCV_E_INVALID;
    out->l1_offset[c] = (uint32_t)acc;
    acc += ceil8(out->l1_stream[c]);
  }
  out->root_points = acc;
  return PCV_OK;
}

// ---- stage-level entry: one batch on the device -> 64 bucket runs ---------------------------------------------------------------
extern "C" int pcv_ooc_bucket_runs(pcv_ctx* ctx, const pcv_build_params* params, const double* xyz, const uint8_t* rgb, const float* intensity,
                                   uint64_t n, int routed, void* const planes[5], uint8_t* octant_digits, uint64_t counts[64]) {
  if (!ctx) return PCV_E_INVALID;
  if (!params || !planes || !counts || !octant_digits) return ctx->fail(PCV_E_INVALID, "null argument");
  for (int b = 0; b < 64; ++b) counts[b] = 0;
  if (n == 0) return PCV_OK;
  if (n > PCV_MAX_POINTS_PER_BUILD) return ctx->fail(PCV_E_INVALID, "at most 2^32 - 2 points per call");
  if (!xyz || !rgb || !planes[0] || !planes[1] || !planes[2] || !planes[3] || (intensity && !planes[4]))
    return ctx->fail(PCV_E_INVALID, "null input or output plane");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvLevels lv;
  int max_level;
  pcv_make_levels(params->bbox_min, params->bbox_max, params->resolution, 2, &lv, &max_level, nullptr, nullptr);
  if (routed && (lv.nlevels < 1 || lv.enc[1] != PCV_ENC_FLOAT32))
    return ctx->fail(PCV_E_INVALID, "the level-1 state is only defined for a Float32-encoded level 1: keep raw planes");
  const bool fast = lv.fast_ok && lv.nlevels >= 2 && lv.enc[1] == PCV_ENC_FLOAT32 && lv.digit_mode[1] == 2u;
  const bool octants_only = (params->flags & PCV_ROUTE_OCTANTS_ONLY) != 0u;
  PcvScratch sc(ctx);
  unsigned long long* d_counts;
  int rc;
  if ((rc = sc.get(&d_counts, 64))) return rc;
  OocPlanes out{{planes[0], planes[1], planes[2], planes[3], planes[4]}};
  if ((rc = ooc_runs(ctx, lv, fast, octants_only, routed != 0, (uint32_t)n, xyz, rgb, intensity, out, octant_digits, d_counts))) return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_counts, 64 * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (int b = 0; b < 64; ++b) counts[b] = ctx->mailbox[b];
  return PCV_OK;
}

// ---- the streamed build ------------------------------------------------------------------------------------------------------
struct pcv_ooc {
  pcv_ctx* ctx = nullptr;
  pcv_build_params params{};
  bool has_intensity = false, routed = false, octants_only = false, fast = false, failed = false;
  uint64_t budget = 0, cap = 0;
  int max_level = 0;
  int32_t enc[64] = {};
  PcvLevels lv{};
  int nplanes = 0;
  uint32_t elem[5] = {};
  // device, kept for the stream: one staging chunk, the run planes of one piece, its octant digits, its counts
  uint8_t* stage = nullptr;
  void* dplane[5] = {};
  uint8_t* doseq = nullptr;
  unsigned long long* dcounts = nullptr;
  hipEvent_t ev[4] = {};
  void* back = nullptr;  // pinned: the runs of one piece on their way into the spills
  size_t back_bytes = 0;
  // host spill: per bucket and plane, in global input order; per octant its level-2 digits while it may stay unsplit
  std::vector<uint8_t> spill[64][5];
  uint64_t count[64] = {};
  std::vector<uint8_t> oseq[8];
  bool oseq_dropped[8] = {};
  pcv_ooc_stats st{};
};

static void ooc_release(pcv_ooc* g) {
  pcv_ctx* ctx = g->ctx;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (void* p : {(void*)g->stage, (void*)g->doseq, (void*)g->dcounts, g->dplane[0], g->dplane[1], g->dplane[2], g->dplane[3], g->dplane[4]})
    if (p) ctx->dev_free(p);
  if (g->back) ctx->host_release(g->back);
  for (auto& e : g->ev)
    if (e) (void)hipEventDestroy(e);
  delete g;
}

extern "C" int pcv_ooc_begin(pcv_ctx* ctx, const pcv_build_params* params, int has_intensity, uint64_t max_points_per_pass, pcv_ooc** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!params || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (params->flags & PCV_BUILD_COMPUTE_BBOX)
    return ctx->fail(PCV_E_INVALID, "pcv_ooc_begin: the stream is read once, the bounding box must be given (PCV_BUILD_COMPUTE_BBOX)");
  if (!(params->resolution > 0.0)) return ctx->fail(PCV_E_INVALID, "resolution must be > 0");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc = ctx->ring_ensure();
  if (rc) return rc;
  pcv_ooc* g = new pcv_ooc();
  g->ctx = ctx;
  g->params = *params;
  g->has_intensity = has_intensity != 0;
  g->cap = params->max_points_per_node ? params->max_points_per_node : PCV_DEFAULT_MAX_POINTS_PER_NODE;
  double edge[64];
  g->max_level = pcv_level_table(params->bbox_min, params->bbox_max, params->resolution, 48, edge, g->enc);
  const bool can_split = g->max_level >= 2 && edge[1] > params->resolution;  // distributed.py: ShardedOctreeBuilder.build
  g->octants_only = !can_split;  // no level-1 node can be split: the buckets are the root octants, each in input order
  g->routed = g->max_level >= 1 && g->enc[1] == PCV_ENC_FLOAT32;
  int ml;
  pcv_make_levels(params->bbox_min, params->bbox_max, params->resolution, 2, &g->lv, &ml, nullptr, nullptr);
  g->fast = g->lv.fast_ok && g->lv.nlevels >= 2 && g->lv.enc[1] == PCV_ENC_FLOAT32 && g->lv.digit_mode[1] == 2u;
  const uint32_t e_routed[5] = {4, 4, 4, 4, 4}, e_raw[5] = {8, 8, 8, 3, 4};
  g->nplanes = g->has_intensity ? 5 : 4;
  std::memcpy(g->elem, g->routed ? e_routed : e_raw, sizeof(g->elem));
  if (max_points_per_pass == 0) {  // derived from free device memory: ~80 B per point at a build's peak + the uploaded planes
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
    max_points_per_pass = (uint64_t)(free_b * 0.85) / 112;
    if (max_points_per_pass < kOocSub) max_points_per_pass = kOocSub;
  }
  g->budget = std::min<uint64_t>(max_points_per_pass, PCV_MAX_POINTS_PER_BUILD);
  g->st.routed = g->routed ? 1u : 0u;
  for (int p = 0; p < 5 && rc == PCV_OK; ++p) rc = ctx->dev_alloc(&g->dplane[p], kOocSub * g->elem[p] + 16);
  if (rc == PCV_OK) rc = ctx->dev_alloc((void**)&g->stage, pcv_ctx::kRingChunk);
  if (rc == PCV_OK) rc = ctx->dev_alloc((void**)&g->doseq, kOocSub);
  if (rc == PCV_OK) rc = ctx->dev_alloc((void**)&g->dcounts, 64 * 8);
  g->back_bytes = kOocSub * 32 + 64 * 8 + 256;
  if (rc == PCV_OK) rc = ctx->host_alloc(&g->back, g->back_bytes);
  for (auto& e : g->ev)
    if (rc == PCV_OK && hipEventCreate(&e) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "pcv_ooc_begin: hipEventCreate");
  if (rc) {
    ooc_release(g);
    return rc;
  }
  *out = g;
  return PCV_OK;
}

static float ev_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

// one piece of <= kOocSub points: ring chunk -> DMA -> runs -> back into the spills (synchronous: the chunk is free on return)
static int ooc_piece(pcv_ooc* g, const double* xyz, const uint8_t* rgb, const float* inten, uint32_t m) {
  pcv_ctx* ctx = g->ctx;
  const size_t xyz_bytes = (size_t)m * 24, rgb_off = (xyz_bytes + 255) & ~(size_t)255, int_off = (rgb_off + (size_t)m * 3 + 255) & ~(size_t)255;
  const size_t total = int_off + (g->has_intensity ? (size_t)m * 4 : 0);
  const int slot = ctx->ring_take();
  if (ctx->ring_busy[slot]) PCV_HIP_CHECK(ctx, hipEventSynchronize(ctx->ring_ev[slot]));  // its previous DMA has left the chunk
  ctx->ring_busy[slot] = false;
  uint8_t* chunk = (uint8_t*)ctx->ring[slot];
  std::memcpy(chunk, xyz, xyz_bytes);
  std::memcpy(chunk + rgb_off, rgb, (size_t)m * 3);
  if (g->has_intensity) std::memcpy(chunk + int_off, inten, (size_t)m * 4);
  hipError_t e = hipEventRecord(g->ev[0], ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(g->stage, chunk, total, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipEventRecord(g->ev[1], ctx->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->stream);  // no DMA may still read the chunk when it is handed on
    return ctx->fail(PCV_E_HIP, std::string("pcv_ooc_append: queuing the DMA of a piece failed: ") + hipGetErrorString(e));
  }
  OocPlanes out{{g->dplane[0], g->dplane[1], g->dplane[2], g->dplane[3], g->dplane[4]}};
  int rc = ooc_runs(ctx, g->lv, g->fast, g->octants_only, g->routed, m, (const double*)g->stage, g->stage + rgb_off,
                    g->has_intensity ? (const float*)(g->stage + int_off) : nullptr, out, g->doseq, g->dcounts);
  // the runs come back: counts, then every plane, then the octant digits, packed into the pinned return block
  uint8_t* back = (uint8_t*)g->back;
  size_t off[6], at = 512;
  for (int p = 0; p < g->nplanes; ++p) off[p] = at, at += ((size_t)m * g->elem[p] + 255) & ~(size_t)255;
  off[5] = at;
  if (rc == PCV_OK) {
    e = hipEventRecord(g->ev[2], ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back, g->dcounts, 64 * 8, hipMemcpyDeviceToHost, ctx->stream);
    for (int p = 0; p < g->nplanes && e == hipSuccess; ++p)
      e = hipMemcpyAsync(back + off[p], g->dplane[p], (size_t)m * g->elem[p], hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(back + off[5], g->doseq, m, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(g->ev[3], ctx->stream);
  }
  const hipError_t se = hipStreamSynchronize(ctx->stream);
  if (rc) return rc;
  if (e != hipSuccess || se != hipSuccess)
    return ctx->fail(PCV_E_HIP, std::string("pcv_ooc_append: ") + hipGetErrorString(e != hipSuccess ? e : se));
  g->st.h2d_ms += ev_ms(g->ev[0], g->ev[1]);
  g->st.d2h_ms += ev_ms(g->ev[2], g->ev[3]);
  g->st.h2d_bytes += total;
  g->st.d2h_bytes += 64 * 8 + (uint64_t)m;  // counts + octant digits
  for (int p = 0; p < g->nplanes; ++p) g->st.d2h_bytes += (uint64_t)m * g->elem[p];
  const uint64_t* cnt = (const uint64_t*)back;
  uint64_t start = 0, ostart[8];
  for (int b = 0; b < 64; ++b) {
    if ((b & 7) == 0) ostart[b >> 3] = start;
    const uint64_t c = cnt[b];
    if (c) {
      for (int p = 0; p < g->nplanes; ++p) {
        const uint8_t* src = back + off[p] + start * g->elem[p];
        g->spill[b][p].insert(g->spill[b][p].end(), src, src + c * g->elem[p]);
      }
      g->count[b] += c;
    }
    start += c;
  }
  if (start != m) return ctx->fail(PCV_E_HIP, "pcv_ooc_append: the bucket runs do not cover the piece");
  for (int o = 0; o < 8; ++o) {
    if (g->oseq_dropped[o]) continue;
    uint64_t oc = 0;
    for (int d = 0; d < 8; ++d) oc += g->count[o * 8 + d];
    if (oc > g->cap || g->octants_only) {  // this level-1 node will be split (or its octant is one bucket): the order across its buckets is moot
      g->oseq_dropped[o] = true;
      std::vector<uint8_t>().swap(g->oseq[o]);
      continue;
    }
    uint64_t here = 0;
    for (int d = 0; d < 8; ++d) here += cnt[o * 8 + d];
    const uint8_t* src = back + off[5] + ostart[o];
    g->oseq[o].insert(g->oseq[o].end(), src, src + here);
  }
  g->st.points += m;
  return PCV_OK;
}

extern "C" int pcv_ooc_append(pcv_ooc* g, const double* xyz, const uint8_t* rgb, const float* intensity, uint64_t n) {
  if (!g) return PCV_E_INVALID;
  pcv_ctx* ctx = g->ctx;
  if (g->failed) return ctx->fail(PCV_E_INVALID, "pcv_ooc_append after a failed append: the build can only be finished or aborted");
  if (n == 0) return PCV_OK;
  if (!xyz || !rgb) return ctx->fail(PCV_E_INVALID, "positions and colour are required (on_disk.rs:20-22: colour is always present)");
  if (g->has_intensity && !intensity) return ctx->fail(PCV_E_INVALID, "the build was begun with intensity: every batch must carry it");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const double t0 = now_ms();
  for (uint64_t done = 0; done < n; done += kOocSub) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(n - done, kOocSub);
    const int rc = ooc_piece(g, xyz + done * 3, rgb + done * 3, g->has_intensity ? intensity + done : nullptr, m);
    if (rc) {
      g->failed = true;
      return rc;
    }
  }
  g->st.stream_ms += now_ms() - t0;
  return PCV_OK;
}

extern "C" void pcv_ooc_abort(pcv_ooc* g) {
  if (g) ooc_release(g);  // (a piece is synchronous: no DMA reads the ring chunk once an append has returned)
}

namespace {

// one partition on the device: its units' spills uploaded into fresh planes (an unsplit octant's 8 buckets interleaved again in
// input order), then pcv_build_begin(_routed) with the global split decision
struct OocPart {
  std::vector<int> buckets;  // in bucket order
  uint64_t n = 0;
};

int ooc_upload_begin(pcv_ooc* g, const OocPart& part, uint32_t split_mask, void* planes[5], pcv_octree** tree) {
  pcv_ctx* ctx = g->ctx;
  int rc = PCV_OK;
  for (int p = 0; p < 5; ++p) planes[p] = nullptr;
  for (int p = 0; p < g->nplanes && rc == PCV_OK; ++p) rc = ctx->dev_alloc(&planes[p], part.n * g->elem[p] + 16);
  if (rc) return rc;
  const double t0 = now_ms();
  uint64_t at = 0;
  std::vector<uint8_t> merged;
  for (size_t k = 0; k < part.buckets.size(); ++k) {
    const int b = part.buckets[k], o = b >> 3;
    const bool whole = !g->octants_only && !((split_mask >> o) & 1u);
    if (whole) {  // an unsplit level-1 node: its 8 buckets are one leaf in input order (they are consecutive in part.buckets)
      if (k > 0 && (part.buckets[k - 1] >> 3) == o) continue;
      uint64_t oc = 0;
      for (int d = 0; d < 8; ++d) oc += g->count[o * 8 + d];
      if (g->oseq_dropped[o] || g->oseq[o].size() != oc) return ctx->fail(PCV_E_HIP, "pcv_ooc_finish: the digit sequence of an unsplit octant is incomplete");
      for (int p = 0; p < g->nplanes; ++p) {
        const uint32_t el = g->elem[p];
        merged.resize(oc * el);
        uint64_t cur[8] = {};
        const uint8_t* seq = g->oseq[o].data();
        for (uint64_t i = 0; i < oc; ++i) {
          const int d = seq[i];
          std::memcpy(&merged[i * el], &g->spill[o * 8 + d][p][cur[d]++ * el], el);
        }
        if (oc && hipMemcpy((uint8_t*)planes[p] + at * el, merged.data(), oc * el, hipMemcpyHostToDevice) != hipSuccess)
          return ctx->fail(PCV_E_HIP, "pcv_ooc_finish: upload of a partition failed");
      }
      at += oc;
      g->st.h2d_bytes += oc * (g->routed ? 16 : 27) + (g->has_intensity ? oc * 4 : 0);
      continue;
    }
    const uint64_t c = g->count[b];
    for (int p = 0; p < g->nplanes && c; ++p)
      if (hipMemcpy((uint8_t*)planes[p] + at * g->elem[p], g->spill[b][p].data(), c * g->elem[p], hipMemcpyHostToDevice) != hipSuccess)
        return ctx->fail(PCV_E_HIP, "pcv_ooc_finish: upload of a partition failed");
    at += c;
    g->st.h2d_bytes += c * (g->routed ? 16 : 27) + (g->has_intensity ? c * 4 : 0);
  }
  g->st.h2d_ms += now_ms() - t0;
  if (at != part.n) return ctx->fail(PCV_E_HIP, "pcv_ooc_finish: a partition's upload does not match its count");
  pcv_build_params pr = g->params;
  pr.flags = (pr.flags & ~(uint32_t)PCV_BUILD_FORCE_SPLIT_L1(0xff)) | PCV_BUILD_FORCE_SPLIT_L1(split_mask);
  if (g->routed) {
    pcv_routed_points rp{};
    rp.n = part.n;
    rp.cx = (const uint32_t*)planes[0], rp.cy = (const uint32_t*)planes[1], rp.cz = (const uint32_t*)planes[2];
    rp.oct_rgb = (const uint32_t*)planes[3];
    rp.intensity = g->has_intensity ? (const float*)planes[4] : nullptr;
    return pcv_build_begin_routed(ctx, &pr, &rp, tree);
  }
  pcv_points pts{};
  pts.n = part.n;
  pts.x = (const double*)planes[0], pts.y = (const double*)planes[1], pts.z = (const double*)planes[2];
  pts.color = (const uint8_t*)planes[3];
  pts.color_stride = 3;
  pts.intensity = g->has_intensity ? (const float*)planes[4] : nullptr;
  pts.mem = PCV_MEM_DEVICE;
  return pcv_build_begin(ctx, &pr, &pts, tree);
}

void free_planes(pcv_ctx* ctx, void* planes[5]) {
  (void)hipStreamSynchronize(ctx->stream);
  for (int p = 0; p < 5; ++p)
    if (planes[p]) ctx->dev_free(planes[p]), planes[p] = nullptr;
}

struct TopSpec {
  std::string name;
  uint32_t level, digit, encoding;
  uint64_t num_points, xyz[2], rgb[2], inten[2];  // (offset, bytes) in the accumulator
};

bool write_blob(const std::string& path, const uint8_t* p, uint64_t len) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, len, f) == len;
  return fclose(f) == 0 && ok;
}

int ooc_finish(pcv_ooc* g, const char* directory) {
  pcv_ctx* ctx = g->ctx;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  uint64_t total = 0;
  for (int b = 0; b < 64; ++b) {
    total += g->count[b];
    g->st.largest_bucket = std::max(g->st.largest_bucket, g->count[b]);
    for (int p = 0; p < g->nplanes; ++p) g->st.spill_bytes += g->spill[b][p].size();
  }
  for (int o = 0; o < 8; ++o) g->st.spill_bytes += g->oseq[o].size();
  if (total == 0) {  // an empty stream: meta.pb without nodes, what pcv_octree_write_dir writes for the in-core build of it
    const double t0 = now_ms();
    if (pcv_write_meta(directory, g->params.resolution, g->params.bbox_min, g->params.bbox_max, nullptr, 0))
      return ctx->fail(PCV_E_IO, "pcv_ooc_finish: cannot write meta.pb");
    g->st.write_ms = now_ms() - t0;
    return PCV_OK;
  }
  // plan
  uint32_t part_of[64], nparts = 0, split_mask = 0;
  char err[256] = {};
  const bool can_split = !g->octants_only;
  int rc = pcv_ooc_plan(g->count, (uint32_t)g->cap, can_split ? 1 : 0, g->budget, part_of, &nparts, &split_mask, err, sizeof(err));
  if (rc) return ctx->fail(rc, std::string("pcv_ooc_finish: ") + err);
  g->st.partitions = nparts;
  g->st.split_mask = split_mask;
  std::vector<OocPart> parts(nparts);
  for (int b = 0; b < 64; ++b)
    if (part_of[b] != 0xffffffffu) parts[part_of[b]].buckets.push_back(b), parts[part_of[b]].n += g->count[b];
  // topology pass
  double t0 = now_ms();
  uint64_t l1[8] = {}, l2[64] = {};
  for (const OocPart& part : parts) {
    void* planes[5];
    pcv_octree* t = nullptr;
    rc = ooc_upload_begin(g, part, split_mask, planes, &t);
    pcv_top_streams ts{};
    if (rc == PCV_OK) rc = pcv_build_top_streams(t, &ts);
    if (t) pcv_octree_free(t);
    free_planes(ctx, planes);
    if (rc) return rc;
    for (int c = 0; c < 8; ++c)
      if (!((split_mask >> c) & 1u)) l1[c] += ts.l1[c];  // a split level-1 node's stream is the sum over its level-2 nodes
    for (int b = 0; b < 64; ++b) l2[b] += ts.l2[b];
  }
  pcv_top_layout layout;
  if (pcv_ooc_top_layout(l1, l2, split_mask, &layout)) return ctx->fail(PCV_E_INVALID, "pcv_ooc_finish: the top streams exceed 32-bit offsets");
  g->st.topology_ms = now_ms() - t0;
  // the global-size root / level-1 nodes (distributed.top_nodes)
  const uint64_t bpc[5] = {0, 1, 2, 4, 8};
  std::vector<TopSpec> specs;
  specs.push_back(TopSpec{"r", 0, 0, 0, layout.root_points, {}, {}, {}});
  for (int c = 0; c < 8; ++c) {
    const uint64_t s = layout.l1_stream[c];
    if (s > 0) specs.push_back(TopSpec{"r" + std::to_string(c), 1, (uint32_t)c, 0, s - ceil8(s), {}, {}, {}});
  }
  uint64_t nbytes = 0;
  for (TopSpec& s : specs) {
    s.encoding = (uint32_t)g->enc[s.level];
    const uint64_t xb = s.num_points * 3 * bpc[s.encoding], rb = s.num_points * 3, ib = g->has_intensity ? s.num_points * 4 : 0;
    s.xyz[0] = nbytes, s.xyz[1] = xb, s.rgb[0] = nbytes + xb, s.rgb[1] = rb, s.inten[0] = nbytes + xb + rb, s.inten[1] = ib;
    nbytes = (nbytes + xb + rb + ib + 15) & ~(uint64_t)15;
  }
  nbytes = std::max<uint64_t>(nbytes, 16);
  uint8_t *acc = nullptr, *part_top = nullptr;
  if ((rc = ctx->dev_alloc((void**)&acc, nbytes)) || (rc = ctx->dev_alloc((void**)&part_top, nbytes))) {
    if (acc) ctx->dev_free(acc);
    return rc;
  }
  struct Guard {
    pcv_ctx* ctx;
    uint8_t *a, *b;
    ~Guard() {
      (void)hipStreamSynchronize(ctx->stream);
      ctx->dev_free(a);
      ctx->dev_free(b);
    }
  } guard{ctx, acc, part_top};
  PCV_HIP_CHECK(ctx, hipMemsetAsync(acc, 0, nbytes, ctx->stream));
  // build pass
  std::vector<pcv_node_info> nodes;
  double build_ms = 0, merge_ms = 0, write_ms = 0;
  for (const OocPart& part : parts) {
    t0 = now_ms();
    void* planes[5];
    pcv_octree* t = nullptr;
    rc = ooc_upload_begin(g, part, split_mask, planes, &t);
    if (rc == PCV_OK) rc = pcv_build_finish(t, &layout);
    free_planes(ctx, planes);
    const double t1 = now_ms();
    build_ms += t1 - t0;
    if (rc == PCV_OK) rc = pcv_octree_write_nodes(t, directory, 2);
    const double t2 = now_ms();
    write_ms += t2 - t1;
    std::vector<pcv_node_copy> copies;
    const uint64_t nn = rc == PCV_OK ? pcv_octree_num_nodes(t) : 0;
    for (uint64_t i = 0; i < nn && rc == PCV_OK; ++i) {
      pcv_node_info info;
      if ((rc = pcv_octree_node(t, i, &info))) break;
      if (info.level >= 2) {
        nodes.push_back(info);
        continue;
      }
      const TopSpec* s = nullptr;
      for (const TopSpec& q : specs)
        if (q.level == info.level && q.digit == (info.level ? (uint32_t)info.id_low : 0u)) s = &q;
      if (!s || (uint64_t)info.num_points != s->num_points || info.encoding != s->encoding) {
        rc = ctx->fail(PCV_E_HIP, "pcv_ooc_finish: a partition's top node does not match its slot in the global layout");
        break;
      }
      pcv_node_copy cp{i, {s->xyz[1] ? s->xyz[0] : UINT64_MAX, s->rgb[1] ? s->rgb[0] : UINT64_MAX, s->inten[1] ? s->inten[0] : UINT64_MAX}};
      copies.push_back(cp);
    }
    if (rc == PCV_OK && !copies.empty()) {
      if (hipMemsetAsync(part_top, 0, nbytes, ctx->stream) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "pcv_ooc_finish: hipMemsetAsync");
      if (rc == PCV_OK) rc = pcv_octree_copy_nodes(t, copies.data(), copies.size(), part_top, nbytes, PCV_MEM_DEVICE);
      if (rc == PCV_OK) {
        const uint64_t words = nbytes / 16;
        hipLaunchKernelGGL(ooc_or_kernel, dim3((unsigned)std::min<uint64_t>((words + 255) / 256, 4096)), dim3(256), 0, ctx->stream, (uint4*)acc,
                           (const uint4*)part_top, words);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
          rc = ctx->fail(PCV_E_HIP, "pcv_ooc_finish: folding the top nodes failed");
      }
    }
    if (t) pcv_octree_free(t);
    merge_ms += now_ms() - t2;
    if (rc) return rc;
  }
  g->st.build_ms = build_ms;
  g->st.merge_ms = merge_ms;
  // the root and the level-1 nodes, then meta.pb — last: a failed build never leaves one
  t0 = now_ms();
  std::vector<uint8_t> top(nbytes);
  PCV_HIP_CHECK(ctx, hipMemcpy(top.data(), acc, nbytes, hipMemcpyDeviceToHost));
  g->st.d2h_bytes += nbytes;
  const std::string dir(directory);
  ::mkdir(dir.c_str(), 0777);
  for (const TopSpec& s : specs) {
    pcv_node_info info{};
    info.id_high = (uint64_t)s.level << 56;
    info.id_low = s.digit;
    info.num_points = (int64_t)s.num_points;
    info.level = s.level;
    info.encoding = s.encoding;
    nodes.push_back(info);
    if (!s.num_points) continue;  // node_writer.rs:78-89: empty nodes have no files
    if (!write_blob(dir + "/" + s.name + ".xyz", &top[s.xyz[0]], s.xyz[1]) || !write_blob(dir + "/" + s.name + ".rgb", &top[s.rgb[0]], s.rgb[1]) ||
        (s.inten[1] && !write_blob(dir + "/" + s.name + ".intensity", &top[s.inten[0]], s.inten[1])))
      return ctx->fail(PCV_E_IO, "pcv_ooc_finish: cannot write the files of node " + s.name);
  }
  std::sort(nodes.begin(), nodes.end(), [](const pcv_node_info& a, const pcv_node_info& b) {
    return a.id_high != b.id_high ? a.id_high < b.id_high : a.id_low < b.id_low;  // (level, index)
  });
  if (pcv_write_meta(directory, g->params.resolution, g->params.bbox_min, g->params.bbox_max, nodes.data(), nodes.size()))
    return ctx->fail(PCV_E_IO, "pcv_ooc_finish: cannot write meta.pb");
  g->st.write_ms = write_ms + (now_ms() - t0);
  g->st.nodes = nodes.size();
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_ooc_finish(pcv_ooc* g, const char* directory, pcv_ooc_stats* stats) {
  if (!g) return PCV_E_INVALID;
  pcv_ctx* ctx = g->ctx;
  int rc;
  if (!directory)
    rc = ctx->fail(PCV_E_INVALID, "directory is null");
  else if (g->failed)
    rc = ctx->fail(PCV_E_INVALID, "pcv_ooc_finish after a failed append");
  else
    rc = ooc_finish(g, directory);
  if (stats) *stats = g->st;
  ooc_release(g);
  return rc;
}
