// pcv_las_write.hip — the result of a batched point query as LAS point data records: quantised and bit-packed on the
// device from the query's own tables, returned as they are (pcv_query_batch_las_records, pcv_s2_query_las_records) or streamed
// into a file through two device buffers and two pinned blocks (pcv_query_batch_write_las, pcv_s2_query_write_las). The format
// itself — fields, rules, header, append — is pcv_las_write.h / .cpp; its host-only entry points are at the end of this file.
//
// Tiles of 32 KiB / record_length records, walks and the store are those of pcv_rows_dev.h, the source, the piece pipeline and
// the slice writer those of pcv_result_rows.h. What is this file's: every lane decodes its point with the query's own decode,
// quantises it and lays the 20 - 38-byte record into the tile's image; and the header's reductions: every lane keeps the
// extremes of X, Y, Z and the three counters of its points in registers, a wave counts the returns by ballot, the waves meet in
// LDS behind the image, and the workgroup adds its 24 values to one zeroed block with one vector atomic each (a sum of 0 is
// skipped). The min pass of auto_offset walks whole chunks, not tiles.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "pcv_internal.h"
#include "pcv_las_write.h"
#include "pcv_result_rows.h"
#include "pcv_rows_dev.h"

namespace {

constexpr uint32_t kLasTileBytes = 32u << 10;
inline uint32_t las_tile_records(uint32_t stride) { return kLasTileBytes / stride; }  // 862 (format 8) .. 1638 (format 0)
constexpr uint64_t kLasDefaultChunkPoints = 1ull << 20;
constexpr uint32_t kAccWords = 27;  // 15 returns, 3 counters, 3 hi keys, 3 lo keys, and one pad
// LDS: the image (tile bytes + the phase, rounded to 16), then 4 waves x kAccWords u32 of partial results
inline uint32_t las_image_bytes(uint32_t tile, uint32_t stride) { return (tile * stride + 16 + 15) & ~15u; }

extern __shared__ __attribute__((aligned(16))) uint8_t las_image[];  // the only LDS of these kernels: its base stays 16-byte aligned

// What a lane (counters, extremes) and a wave (returns; uniform) have seen of the header's reductions.
struct LasLaneAcc {
  uint32_t hi[3] = {0, 0, 0}, lo[3] = {0, 0, 0};
  uint32_t out_of_range = 0, clamped = 0, masked = 0;
  uint32_t by_return[15] = {};
};
// one point: its record into the image, its part into the lane's registers; `active` lanes only, but every lane of the wave
// calls (the ballots)
__device__ __forceinline__ void las_take(const PcvLasWritePlan& pl, bool active, uint64_t i, double x, double y, double z, uint8_t* rec, LasLaneAcc& a) {
  uint32_t slot = 15;
  if (active) {
    PcvLasRecord r;
    uint32_t oor, cl, mk;
    pcv_las_make_record(pl, i, x, y, z, &r, &oor, &cl, &mk);
    pcv_las_put(pl.f, r, rec);
    a.out_of_range += oor, a.clamped += cl, a.masked += mk;
    a.hi[0] = max(a.hi[0], pcv_las_hi_key(r.X)), a.hi[1] = max(a.hi[1], pcv_las_hi_key(r.Y)), a.hi[2] = max(a.hi[2], pcv_las_hi_key(r.Z));
    a.lo[0] = max(a.lo[0], pcv_las_lo_key(r.X)), a.lo[1] = max(a.lo[1], pcv_las_lo_key(r.Y)), a.lo[2] = max(a.lo[2], pcv_las_lo_key(r.Z));
    slot = pcv_las_return_slot(pl.f, r);
  }
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k) a.by_return[k] += (uint32_t)__popcll(__ballot(slot == k));  // uniform: scalar registers
}
// The waves' results into LDS at `part` (behind the image), then one atomic per value and workgroup. A tile holds fewer than
// 2^11 records, so u32 partial sums cannot wrap.
__device__ __forceinline__ void las_flush(LasLaneAcc& a, uint32_t* part, PcvLasWriteAcc* acc) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a.out_of_range += __shfl_xor(a.out_of_range, o), a.clamped += __shfl_xor(a.clamped, o), a.masked += __shfl_xor(a.masked, o);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.hi[k] = max(a.hi[k], __shfl_xor(a.hi[k], o)), a.lo[k] = max(a.lo[k], __shfl_xor(a.lo[k], o));
  }
  if (lane == 0) {
    uint32_t* w = part + wave * kAccWords;
#pragma unroll
    for (int k = 0; k < 15; ++k) w[k] = a.by_return[k];
    w[15] = a.out_of_range, w[16] = a.clamped, w[17] = a.masked;
#pragma unroll
    for (int k = 0; k < 3; ++k) w[18 + k] = a.hi[k], w[21 + k] = a.lo[k];
  }
  __syncthreads();
  const uint32_t t = threadIdx.x;
  if (t < 24) {
    const uint32_t v0 = part[t], v1 = part[kAccWords + t], v2 = part[2 * kAccWords + t], v3 = part[3 * kAccWords + t];
    if (t < 18) {
      const uint32_t sum = v0 + v1 + v2 + v3;
      unsigned long long* dst = t < 15 ? acc->by_return + t : t == 15 ? &acc->out_of_range : t == 16 ? &acc->clamped_intensity : &acc->masked_values;
      if (sum) atomicAdd(dst, (unsigned long long)sum);
    } else {
      uint32_t* dst = t < 21 ? acc->hi + (t - 18) : acc->lo + (t - 21);
      atomicMax(dst, max(max(v0, v1), max(v2, v3)));
    }
  }
}

// Records [row0 + blockIdx.x * tile, ...) of the octree batch, `nrows` from row0 on, to out + (row - row0) * stride. The chunks
// [c0, c1) are those of the caller's segment range; chunk_off their scanned kept counts.
__global__ __launch_bounds__(256) void las_records_octree_kernel(const ChunkDesc* __restrict__ desc, uint64_t c0, uint64_t c1,
                                                                 const uint8_t* __restrict__ xyz_blob, const uint8_t* __restrict__ keep,
                                                                 const uint64_t* __restrict__ chunk_off, PcvLasWritePlan pl, uint64_t row0,
                                                                 uint64_t nrows, uint32_t tile, uint32_t part_at, uint8_t* __restrict__ out,
                                                                 PcvLasWriteAcc* __restrict__ acc) {
  const PcvRowsTile t = pcv_rows_tile(row0, nrows, tile, pl.stride, out);
  LasLaneAcc a;
  pcv_walk_octree_rows(desc, c0, c1, xyz_blob, keep, chunk_off, t.g0, t.g1,
                       [&](bool mine, const PointsView& v, uint32_t q, uint64_t attr_index, uint32_t row_in_tile) {
                         V3d p{0.0, 0.0, 0.0};
                         if (mine) p = load_point(v, q);
                         las_take(pl, mine, attr_index, p.x, p.y, p.z, las_image + t.phase + (mine ? row_in_tile * pl.stride : 0u), a);
                       });
  las_flush(a, reinterpret_cast<uint32_t*>(las_image + part_at), acc);  // (its barrier is the one the image needs)
  pcv_store_image(las_image, t.dst, t.phase, t.rows * pl.stride);
}

// The same over an S2 query: positions read as the doubles they are.
__global__ __launch_bounds__(256) void las_records_s2_kernel(const PcvS2Chunk* __restrict__ chunks, uint64_t c0, uint64_t c1,
                                                             const uint8_t* __restrict__ xyz, const uint32_t* __restrict__ flags,
                                                             const uint64_t* __restrict__ offsets, PcvLasWritePlan pl, uint64_t row0, uint64_t nrows,
                                                             uint32_t tile, uint32_t part_at, uint8_t* __restrict__ out,
                                                             PcvLasWriteAcc* __restrict__ acc) {
  const PcvRowsTile t = pcv_rows_tile(row0, nrows, tile, pl.stride, out);
  LasLaneAcc a;
  pcv_walk_s2_rows(chunks, c0, c1, flags, offsets, t.g0, t.g1, [&](bool mine, uint64_t i, uint32_t row_in_tile) {
    double x = 0.0, y = 0.0, z = 0.0;
    if (mine) {
      const double* p = reinterpret_cast<const double*>(xyz) + 3 * i;
      x = p[0], y = p[1], z = p[2];
    }
    las_take(pl, mine, i, x, y, z, las_image + t.phase + (mine ? row_in_tile * pl.stride : 0u), a);
  });
  las_flush(a, reinterpret_cast<uint32_t*>(las_image + part_at), acc);
  pcv_store_image(las_image, t.dst, t.phase, t.rows * pl.stride);
}

// The min pass of auto_offset: one wave per chunk of the range, the kept points' decoded positions as total-order keys under
// min, kept as ~key under max so that the zeroed block is the neutral state. out: 3 u64.
__device__ __forceinline__ void las_min_flush(unsigned long long k[3], unsigned long long* out) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int a = 0; a < 3; ++a) k[a] = max(k[a], (unsigned long long)__shfl_xor((long long)k[a], o));
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (k[a]) atomicMax(out + a, k[a]);
}
__global__ __launch_bounds__(256) void las_min_octree_kernel(const ChunkDesc* __restrict__ desc, uint64_t c0, uint64_t c1,
                                                             const uint8_t* __restrict__ xyz_blob, const uint8_t* __restrict__ keep,
                                                             unsigned long long* __restrict__ out) {
  const uint64_t ci = c0 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long k[3] = {0, 0, 0};
  if (ci < c1) {
    const ChunkDesc& d = desc[ci];
    const PointsView v = points_view_of(d, xyz_blob);
    const uint8_t* kp = keep + d.keep_off;
    for (uint32_t q = lane; q < d.cnt; q += 64) {
      if (!kp[q]) continue;
      const V3d p = load_point(v, q);
      k[0] = max(k[0], (unsigned long long)~pcv_las_order_key((uint64_t)__double_as_longlong(p.x)));
      k[1] = max(k[1], (unsigned long long)~pcv_las_order_key((uint64_t)__double_as_longlong(p.y)));
      k[2] = max(k[2], (unsigned long long)~pcv_las_order_key((uint64_t)__double_as_longlong(p.z)));
    }
  }
  las_min_flush(k, out);
}
__global__ __launch_bounds__(256) void las_min_s2_kernel(const PcvS2Chunk* __restrict__ chunks, uint64_t c0, uint64_t c1,
                                                         const uint8_t* __restrict__ xyz, const uint32_t* __restrict__ flags,
                                                         unsigned long long* __restrict__ out) {
  const uint64_t ci = c0 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long k[3] = {0, 0, 0};
  if (ci < c1) {
    const PcvS2Chunk c = chunks[ci];
    for (uint32_t q = lane; q < c.count; q += 64) {
      if (!flags[c.first + q]) continue;
      const uint64_t* p = reinterpret_cast<const uint64_t*>(xyz) + 3 * (c.src + q);
      for (int a = 0; a < 3; ++a) k[a] = max(k[a], (unsigned long long)~pcv_las_order_key(p[a]));
    }
  }
  las_min_flush(k, out);
}

// ---- what the two kinds of result share on the host -------------------------------------------------------------------------
// The plan with its columns on the device. Loads the used extras of a cloud opened from a directory, and only those.
int resolve_plan(const PcvResultSource& s, const pcv_las_write_params* params, PcvLasWritePlan* plan, pcv_las_write_info* info) {
  pcv_ctx* ctx = s.ctx;
  PcvLasSource src;
  src.has_intensity = s.octree ? s.octree->has_intensity : s.s2->cloud->has_intensity;
  if (s.s2)
    for (const PcvS2Extra& e : s.s2->cloud->extras) src.extra_names.push_back(e.name), src.extra_types.push_back(e.data_type);
  std::vector<int> field_of;
  bool use_color = false, use_intensity = false;
  std::string why;
  if (int rc = pcv_las_write_make_plan(params, src, plan, &field_of, &use_color, &use_intensity, info, &why)) return ctx->fail(rc, why);
  if (use_color) plan->cols.color = s.octree ? s.octree->tree->d_rgb : s.s2->cloud->d_rgb;
  if (use_intensity) plan->cols.intensity = reinterpret_cast<const float*>(s.octree ? s.octree->tree->d_int : s.s2->cloud->d_int);
  for (size_t k = 0; k < field_of.size(); ++k) {
    if (field_of[k] < 0) continue;
    if (int rc = pcv_s2_extra_resident(s.s2->cloud, k)) return rc;
    plan->cols.extra[field_of[k]] = s.s2->cloud->extras[k].d;
  }
  return PCV_OK;
}

// auto_offset: floor(min) per axis over the rows of chunks [c0, c1) into plan->offset; a launch of its own and a wait
int resolve_auto_offset(const PcvResultSource& s, uint64_t c0, uint64_t c1, uint64_t np, PcvLasWritePlan* plan) {
  pcv_ctx* ctx = s.ctx;
  for (int a = 0; a < 3; ++a) plan->offset[a] = 0.0;
  if (np == 0 || c1 == c0) return PCV_OK;
  PcvScratch sc(ctx);
  unsigned long long* d_min = nullptr;
  if (int rc = sc.get(&d_min, 3)) return rc;
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_min, 0, 3 * sizeof(unsigned long long), ctx->stream));
  const uint64_t blocks = (c1 - c0 + 3) / 4;
  if (blocks > 0x7fffffffull) return ctx->fail(PCV_E_INVALID, "too many chunks for one launch");
  {
    PcvProf prof(ctx, PCV_K_LAS_WRITE_MIN);
    if (s.octree) {
      const pcv_query_batch* b = s.octree;
      hipLaunchKernelGGL(las_min_octree_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, (const ChunkDesc*)b->d_desc, c0, c1,
                         (const uint8_t*)b->tree->d_xyz, (const uint8_t*)b->d_keep, d_min);
    } else {
      const pcv_s2_query* q = s.s2;
      hipLaunchKernelGGL(las_min_s2_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, (const PcvS2Chunk*)q->d_chunks, c0, c1,
                         (const uint8_t*)q->cloud->d_xyz, (const uint32_t*)q->d_flags, d_min);
    }
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  unsigned long long h[3];
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(h, d_min, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (int a = 0; a < 3; ++a) {
    const uint64_t bits = pcv_las_order_bits(~(uint64_t)h[a]);
    double d;
    std::memcpy(&d, &bits, 8);
    plan->offset[a] = std::floor(d);
  }
  return PCV_OK;
}

// records [row0, row0 + nrows) of the result, found among the chunks [c0, c1), into d_out (device) on ctx->stream; d_acc accumulates
int launch_records(const PcvResultSource& s, const PcvLasWritePlan& plan, uint64_t c0, uint64_t c1, uint64_t row0, uint64_t nrows, uint8_t* d_out,
                   PcvLasWriteAcc* d_acc) {
  pcv_ctx* ctx = s.ctx;
  const uint32_t tile = las_tile_records(plan.stride);
  const uint64_t blocks = (nrows + tile - 1) / tile;
  if (blocks > 0x7fffffffull) return ctx->fail(PCV_E_INVALID, "too many records for one launch: pack the result in pieces");
  const uint32_t part_at = las_image_bytes(tile, plan.stride);
  const size_t lds = (size_t)part_at + 4 * kAccWords * sizeof(uint32_t);
  const dim3 grid((uint32_t)blocks), block(256);
  PcvProf prof(ctx, PCV_K_LAS_WRITE_RECORDS);
  if (s.octree) {
    const pcv_query_batch* b = s.octree;
    hipLaunchKernelGGL(las_records_octree_kernel, grid, block, lds, ctx->stream, (const ChunkDesc*)b->d_desc, c0, c1, (const uint8_t*)b->tree->d_xyz,
                       (const uint8_t*)b->d_keep, (const uint64_t*)b->d_chunk_off, plan, row0, nrows, tile, part_at, d_out, d_acc);
  } else {
    const pcv_s2_query* q = s.s2;
    hipLaunchKernelGGL(las_records_s2_kernel, grid, block, lds, ctx->stream, (const PcvS2Chunk*)q->d_chunks, c0, c1, (const uint8_t*)q->cloud->d_xyz,
                       (const uint32_t*)q->d_flags, (const uint64_t*)q->d_offsets, plan, row0, nrows, tile, part_at, d_out, d_acc);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

int las_records(const PcvResultSource& s, uint64_t first_segment, uint64_t num_segments, const pcv_las_write_params* params, uint64_t capacity_bytes,
                int mem, void* out, uint32_t* record_length, uint64_t* num_records, pcv_las_write_info* info) {
  pcv_ctx* ctx = s.ctx;
  if (record_length) *record_length = 0;
  if (num_records) *num_records = 0;
  if (info) *info = pcv_las_write_info{};
  if (!params) return ctx->fail(PCV_E_INVALID, "null argument");
  int rc;
  if ((rc = s.check_range(first_segment, num_segments))) return rc;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvLasWritePlan plan{};
  pcv_las_write_info in{};
  if ((rc = resolve_plan(s, params, &plan, &in))) return rc;
  const auto [p0, np, c0, c1] = s.rows_of_segments(first_segment, num_segments);
  if (np >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "LAS: number of point records " + std::to_string(np) + " is 2^32 - 1 or more");
  if (record_length) *record_length = plan.stride;
  if (num_records) *num_records = np;
  if (np > capacity_bytes / plan.stride)
    return ctx->fail(PCV_E_INVALID, "the segments hold " + std::to_string(np) + " records of " + std::to_string(plan.stride) + " bytes, capacity is " +
                                        std::to_string(capacity_bytes) + " bytes");
  if (params->auto_offset && (rc = resolve_auto_offset(s, c0, c1, np, &plan))) return rc;
  std::string why;
  if ((rc = pcv_las_write_check_offset(plan, &why))) return ctx->fail(rc, why);
  PcvLasWriteAcc acc{};
  if (np > 0) {
    if (!out) return ctx->fail(PCV_E_INVALID, "null output");
    PcvScratch sc(ctx);
    uint8_t* d_out = (uint8_t*)out;
    PcvLasWriteAcc* d_acc = nullptr;
    if ((rc = sc.get(&d_acc, 1))) return rc;
    if (mem == PCV_MEM_HOST && (rc = sc.get(&d_out, np * plan.stride))) return rc;
    PCV_HIP_CHECK(ctx, hipMemsetAsync(d_acc, 0, sizeof(PcvLasWriteAcc), ctx->stream));
    if ((rc = launch_records(s, plan, c0, c1, p0, np, d_out, d_acc))) return rc;
    if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, np * plan.stride, hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(&acc, d_acc, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->prof_resolve();
  }
  pcv_las_write_fill_info(plan, acc, np, &in);
  if (info) *info = in;
  return PCV_OK;
}

int write_las(const PcvResultSource& s, uint64_t first_segment, uint64_t num_segments, const char* path, const pcv_las_write_params* params,
              pcv_las_write_info* info) {
  pcv_ctx* ctx = s.ctx;
  if (info) *info = pcv_las_write_info{};
  if (!path || !params) return ctx->fail(PCV_E_INVALID, "null argument");
  int rc;
  if ((rc = s.check_range(first_segment, num_segments))) return rc;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvLasWritePlan plan{};
  pcv_las_write_info in{};
  if ((rc = resolve_plan(s, params, &plan, &in))) return rc;
  const PcvResultSource::Rows r = s.rows_of_segments(first_segment, num_segments);
  const uint64_t np = r.np;
  std::string why;
  bool exists = false;
  PcvLasTotals old;
  std::vector<uint8_t> old_header;
  uint64_t old_size = 0;
  if (params->open_mode == PCV_LAS_APPEND) {
    double fs[3], fo[3];
    if ((rc = pcv_las_append_check(path, plan, !params->auto_offset, &exists, &old, fs, fo, &old_header, &old_size, &why))) return ctx->fail(rc, why);
    if (exists)
      for (int a = 0; a < 3; ++a) plan.scale[a] = fs[a], plan.offset[a] = fo[a];  // (auto_offset is satisfied by the file's)
  }
  if (params->auto_offset && !exists && (rc = resolve_auto_offset(s, r.c0, r.c1, np, &plan))) return rc;
  if ((rc = pcv_las_write_check_offset(plan, &why))) return ctx->fail(rc, why);
  if (np + old.count >= 0xffffffffull)
    return ctx->fail(PCV_E_INVALID, "LAS: number of point records " + std::to_string(np + old.count) + " is 2^32 - 1 or more");
  PcvLasFile file;
  if ((rc = file.begin(path, kLasHeaderSize[plan.version_minor], exists, old, old_header, old_size, &why))) return ctx->fail(rc, why);
  PcvLasWriteAcc acc{};
  if (np == 0) {  // nothing written, no file; an appended file stays as it is
    pcv_las_write_fill_info(plan, acc, 0, &in);
    if (info) *info = in;
    return PCV_OK;
  }
  const uint32_t stride = plan.stride;
  const uint64_t piece = std::min<uint64_t>(np, params->chunk_points ? params->chunk_points : kLasDefaultChunkPoints);
  const uint64_t piece_bytes = ((piece * stride + 255) / 256) * 256;
  PcvScratch sc(ctx);
  uint8_t* d_buf[2];
  PcvLasWriteAcc* d_acc = nullptr;
  PcvPiecePipe pipe;  // the accumulator block lives across the pieces
  if ((rc = sc.get(&d_buf[0], piece_bytes)) || (rc = sc.get(&d_buf[1], piece_bytes)) || (rc = sc.get(&d_acc, 1)) ||
      (rc = ctx->pinned_reserve(2 * piece_bytes)) || (rc = pipe.make(ctx)))
    return rc;
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_acc, 0, sizeof(PcvLasWriteAcc), ctx->stream));
  uint8_t* h_buf[2] = {(uint8_t*)ctx->pinned, (uint8_t*)ctx->pinned + piece_bytes};
  if ((rc = file.open_for_rows(&why))) return ctx->fail(rc, why);
  auto rows_of = [&](uint64_t k) { return std::min(piece, np - k * piece); };
  // the header's reductions once the last piece is written; a point out of range refuses the file
  auto totals = [&]() -> int {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(&acc, d_acc, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    pcv_las_write_fill_info(plan, acc, np, &in);
    if (in.out_of_range != 0) {
      std::string axes;
      for (int a = 0; a < 3; ++a)
        axes += std::string(a ? ", " : "") + "xyz"[a] + " = offset " + std::to_string(plan.offset[a]) + " + [-2147483648, 2147483647] * " +
                std::to_string(plan.scale[a]);
      return ctx->fail(PCV_E_INVALID, "LAS: " + std::to_string(in.out_of_range) + " of " + std::to_string(np) +
                                          " points are out of range of the 32-bit coordinates (" + axes + "); nothing was written");
    }
    return PCV_OK;
  };
  rc = pcv_run_pieces(
      ctx, pipe, (np + piece - 1) / piece,
      [&](uint64_t k, int b) { return launch_records(s, plan, r.c0, r.c1, r.p0 + k * piece, rows_of(k), d_buf[b], d_acc); },
      [&](uint64_t k) { return rows_of(k) * stride; }, d_buf, h_buf,
      [&](uint64_t k, int b) -> int {
        if (hipEventSynchronize(pipe.copied[b]) != hipSuccess) return ctx->fail(PCV_E_HIP, "copying LAS records to the host failed");
        const uint64_t at = k * piece * stride;
        return pcv_write_slices(ctx, rows_of(k) * stride,
                                [&](uint64_t lo, uint64_t len, std::string* w) { return file.write_at(at + lo, h_buf[b] + lo, len, w); });
      });
  if (rc == PCV_OK && (rc = totals()) != PCV_OK) pcv_drain_pieces(ctx);
  if (rc != PCV_OK) {
    file.abandon();
    if (info) *info = in;
    return rc;
  }
  uint8_t header[kLasMaxHeader];
  const uint32_t hs = pcv_las_build_header(params, plan, pcv_las_totals_merge(old, pcv_las_totals_of(in)), header);
  if ((rc = file.commit(header, hs, &why))) return ctx->fail(rc, why);
  ctx->prof_resolve();
  if (info) *info = in;
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_query_batch_las_records(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const pcv_las_write_params* params,
                                           uint64_t capacity_bytes, int mem, void* out, uint32_t* record_length, uint64_t* num_records,
                                           pcv_las_write_info* info) {
  if (!b) return PCV_E_INVALID;
  return las_records(source_of(b), first_segment, num_segments, params, capacity_bytes, mem, out, record_length, num_records, info);
}

extern "C" int pcv_s2_query_las_records(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const pcv_las_write_params* params,
                                        uint64_t capacity_bytes, int mem, void* out, uint32_t* record_length, uint64_t* num_records,
                                        pcv_las_write_info* info) {
  if (!q) return PCV_E_INVALID;
  if (!q->cloud->ctx) return q->cloud->fail(PCV_E_INVALID, "LAS output needs a cloud on a device (this one is host only)");
  return las_records(source_of(q), first_segment, num_segments, params, capacity_bytes, mem, out, record_length, num_records, info);
}

extern "C" int pcv_query_batch_write_las(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const char* path,
                                         const pcv_las_write_params* params, pcv_las_write_info* info) {
  if (!b) return PCV_E_INVALID;
  return write_las(source_of(b), first_segment, num_segments, path, params, info);
}

extern "C" int pcv_s2_query_write_las(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const char* path,
                                      const pcv_las_write_params* params, pcv_las_write_info* info) {
  if (!q) return PCV_E_INVALID;
  if (!q->cloud->ctx) return q->cloud->fail(PCV_E_INVALID, "LAS output needs a cloud on a device (this one is host only)");
  return write_las(source_of(q), first_segment, num_segments, path, params, info);
}

// ---- the format's host-only entry points (pcv_las_write.cpp) -----------------------------------------------------------------
namespace {
int host_source(int has_intensity, const char* const* names, const int32_t* types, uint32_t n, PcvLasSource* src) {
  if (n && (!names || !types)) return pcv_host_fail(PCV_E_INVALID, "LAS: null argument");
  src->has_intensity = has_intensity != 0;
  for (uint32_t k = 0; k < n; ++k) {
    if (!names[k]) return pcv_host_fail(PCV_E_INVALID, "LAS: extra " + std::to_string(k) + " has no name");
    src->extra_names.push_back(names[k]), src->extra_types.push_back(types[k]);
  }
  return PCV_OK;
}
// a plan from an info that a former call filled: format, version, scale, offset
int plan_of_info(const pcv_las_write_info* info, PcvLasWritePlan* plan) {
  const uint32_t f = info->point_format, m = info->version_minor;
  if (f > 8 || f == 4 || f == 5 || (m != 2 && m != 4) || (m == 2 && f > 3)) return pcv_host_fail(PCV_E_INVALID, "LAS: info names no format and version that are written");
  *plan = PcvLasWritePlan{};
  plan->f = pcv_las_format(f), plan->stride = plan->f.min_len, plan->version_minor = m;
  for (int a = 0; a < 3; ++a) plan->scale[a] = info->scale[a], plan->offset[a] = info->offset[a];
  return PCV_OK;
}
}  // namespace

extern "C" int pcv_las_write_check_params_host(const pcv_las_write_params* params, int has_intensity, const char* const* extra_names,
                                               const int32_t* extra_types, uint32_t num_extras, pcv_las_write_info* info) {
  PcvLasSource src;
  if (int rc = host_source(has_intensity, extra_names, extra_types, num_extras, &src)) return rc;
  PcvLasWritePlan plan{};
  std::vector<int> field_of;
  bool uc, ui;
  std::string why;
  if (int rc = pcv_las_write_make_plan(params, src, &plan, &field_of, &uc, &ui, info, &why)) return pcv_host_fail(rc, why);
  if (!params->auto_offset)
    if (int rc = pcv_las_write_check_offset(plan, &why)) return pcv_host_fail(rc, why);
  return PCV_OK;
}

extern "C" int pcv_las_encode_host(const pcv_las_write_params* params, uint64_t n, const double* x, const double* y, const double* z,
                                   const uint8_t* color, const float* intensity, const char* const* extra_names, const int32_t* extra_types,
                                   const void* const* extras, uint32_t num_extras, void* out, uint64_t capacity_bytes, pcv_las_write_info* info) {
  if (info) *info = pcv_las_write_info{};
  PcvLasSource src;
  if (int rc = host_source(intensity != nullptr, extra_names, extra_types, num_extras, &src)) return rc;
  PcvLasWritePlan plan{};
  std::vector<int> field_of;
  bool uc = false, ui = false;
  std::string why;
  pcv_las_write_info in{};
  if (int rc = pcv_las_write_make_plan(params, src, &plan, &field_of, &uc, &ui, &in, &why)) return pcv_host_fail(rc, why);
  if (n && (!x || !y || !z)) return pcv_host_fail(PCV_E_INVALID, "LAS: null positions");
  if (uc) plan.cols.color = color;  // (NULL: zero colour)
  if (ui) plan.cols.intensity = intensity;
  for (size_t k = 0; k < field_of.size(); ++k) {
    if (field_of[k] < 0) continue;
    if (n && (!extras || !extras[k])) return pcv_host_fail(PCV_E_INVALID, "LAS: extra '" + src.extra_names[k] + "' has no column");
    plan.cols.extra[field_of[k]] = extras ? (const uint8_t*)extras[k] : nullptr;
  }
  if (params->auto_offset) plan.offset[0] = pcv_las_floor_min(x, n), plan.offset[1] = pcv_las_floor_min(y, n), plan.offset[2] = pcv_las_floor_min(z, n);
  if (int rc = pcv_las_write_check_offset(plan, &why)) return pcv_host_fail(rc, why);
  if (n >= 0xffffffffull) return pcv_host_fail(PCV_E_INVALID, "LAS: number of point records " + std::to_string(n) + " is 2^32 - 1 or more");
  if (n > capacity_bytes / plan.stride) return pcv_host_fail(PCV_E_INVALID, "LAS: the capacity holds fewer than " + std::to_string(n) + " records");
  if (n && !out) return pcv_host_fail(PCV_E_INVALID, "null output");
  PcvLasWriteAcc acc{};
  pcv_las_encode_records(plan, x, y, z, n, (uint8_t*)out, &acc);
  pcv_las_write_fill_info(plan, acc, n, &in);
  if (info) *info = in;
  return PCV_OK;
}

extern "C" int pcv_las_write_header_host(const pcv_las_write_params* params, const pcv_las_write_info* info, void* buf, uint64_t cap, uint64_t* len) {
  if (len) *len = 0;
  if (!params || !info) return pcv_host_fail(PCV_E_INVALID, "LAS: null argument");
  if (params->struct_size < sizeof(pcv_las_write_params)) return pcv_host_fail(PCV_E_INVALID, "pcv_las_write_params.struct_size is too small");
  PcvLasWritePlan plan;
  if (int rc = plan_of_info(info, &plan)) return rc;
  if (info->num_records >= 0xffffffffull)
    return pcv_host_fail(PCV_E_INVALID, "LAS: number of point records " + std::to_string(info->num_records) + " is 2^32 - 1 or more");
  uint8_t h[kLasMaxHeader];
  const uint32_t size = pcv_las_build_header(params, plan, pcv_las_totals_of(*info), h);
  if (len) *len = size;
  if (buf && cap) std::memcpy(buf, h, (size_t)std::min<uint64_t>(cap, size));
  return PCV_OK;
}

extern "C" int pcv_las_append_check_host(const char* path, const pcv_las_write_params* params, const pcv_las_write_info* info, uint64_t* old_count) {
  if (old_count) *old_count = 0;
  if (!path || !params || !info) return pcv_host_fail(PCV_E_INVALID, "LAS: null argument");
  PcvLasWritePlan plan;
  if (int rc = plan_of_info(info, &plan)) return rc;
  for (int a = 0; a < 3; ++a) plan.scale[a] = params->scale[a], plan.offset[a] = params->offset[a];
  bool exists;
  PcvLasTotals t;
  double s[3], o[3];
  std::vector<uint8_t> h;
  uint64_t size;
  std::string why;
  if (int rc = pcv_las_append_check(path, plan, !params->auto_offset, &exists, &t, s, o, &h, &size, &why)) return pcv_host_fail(rc, why);
  if (old_count) *old_count = t.count;
  return PCV_OK;
}
