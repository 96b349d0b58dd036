// pcv_s2_stream.hip — S2 cell clouds from a stream of batches: S2Splitter as the NodeWriter<PointsBatch> it is (reference
// src/read_write/s2.rs:60-173), `write` once per batch for as long as the input lasts, `get_meta` at the end.
//
//   append   pcv_s2.hip's split of the batch, kept on the device as a pending part: cells ascending, input order inside a cell
//   plan     pcv_s2_merge_plan.h: the merged cells, one segment per (cell, part), the segments cut into output chunks
//   merge    s2_merge_kernel: one launch, one workgroup per output chunk of 2 048 points — every lane finds the segment of its
//            points by binary search over the chunk's segment range (staged in LDS up to 1 024 segments) and copies them
//   flush    directory mode: the merged blobs to pinned host memory, every cell's run appended to its files (pcv_io.cpp)
#include <algorithm>
#include <cstring>
#include <map>
#include <unordered_set>

#include "pcv_internal.h"
#include "pcv_s2_dev.h"
#include "pcv_s2_merge_plan.h"
#include "pcv_s2_obj.h"

namespace {

constexpr uint32_t kMergeLdsSegments = 1024;            // segment offsets of a chunk's range staged in LDS (8 KB); longer ranges are searched in global memory
constexpr uint64_t kMemoryPointCap = 0xffffffffull;     // an in-memory stream holds fewer points than this (pcv_s2_order is u32)
constexpr uint64_t kDefaultFlushPoints = 1ull << 26;    // directory mode, flush_points == 0 (a design constant)
constexpr uint64_t kMaxFlushPoints = 1ull << 31;

struct MergePart {  // device table, one entry per part
  const double* xyz;
  const uint8_t* rgb;
  const float* inten;
  const uint32_t* order;
  uint64_t base;  // points of the stream before this part's batch
};

// One workgroup per output chunk. Nothing depends on scheduling: every output byte has one writer, decided by the plan.
__global__ __launch_bounds__(256) void s2_merge_kernel(uint64_t n, uint64_t num_segments, uint64_t num_chunks,
                                                        const uint64_t* __restrict__ seg_dst, const pcv_s2_merge_segment* __restrict__ segs,
                                                        const uint64_t* __restrict__ chunk_first, const MergePart* __restrict__ parts,
                                                        double* __restrict__ xyz, uint8_t* __restrict__ rgb, float* __restrict__ inten,
                                                        uint32_t* __restrict__ order) {
  __shared__ uint64_t s_dst[kMergeLdsSegments];
  __shared__ uint32_t s_part[kMergeChunkPoints];  // per point of the chunk: its part and its slot in the part's blobs
  __shared__ uint32_t s_src[kMergeChunkPoints];
  const uint64_t chunk = blockIdx.x;
  const uint64_t begin = chunk * kMergeChunkPoints;
  if (chunk >= num_chunks || begin >= n) return;
  const uint32_t m = (uint32_t)(n - begin < (uint64_t)kMergeChunkPoints ? n - begin : (uint64_t)kMergeChunkPoints);
  // the chunk's segments: from the one that holds its first point to the one that holds the next chunk's first point
  const uint64_t lo = chunk_first[chunk];
  const uint64_t hi = chunk + 1 < num_chunks ? chunk_first[chunk + 1] : num_segments - 1;
  const uint64_t span = hi - lo + 1;
  const bool staged = span <= (uint64_t)kMergeLdsSegments;
  if (staged)
    for (uint32_t i = threadIdx.x; i < (uint32_t)span; i += 256u) s_dst[i] = seg_dst[lo + i];
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < m; j += 256u) {
    const uint64_t dst = begin + j;
    uint64_t a = 0, b = span - 1;  // the last segment of the range that starts at or before dst (the first one does)
    while (a < b) {
      const uint64_t mid = (a + b + 1) >> 1;
      const uint64_t at = staged ? s_dst[mid] : seg_dst[lo + mid];
      if (at <= dst) a = mid;
      else b = mid - 1;
    }
    const pcv_s2_merge_segment sg = segs[lo + a];
    const uint32_t src = (uint32_t)(sg.src_offset + (dst - sg.dst_offset));
    s_part[j] = sg.part;
    s_src[j] = src;
    if (inten) inten[dst] = parts[sg.part].inten[src];
    if (order) order[dst] = parts[sg.part].order[src] + (uint32_t)parts[sg.part].base;
  }
  __syncthreads();
  // xyz: the chunk's 3 m doubles, one per lane and step, consecutive lanes on consecutive doubles
  for (uint32_t e = threadIdx.x; e < 3u * m; e += 256u) {
    const uint32_t p = e / 3u, c = e - 3u * p;
    xyz[3u * begin + e] = parts[s_part[p]].xyz[3ull * s_src[p] + c];
  }
  // rgb: the chunk's 3 m bytes start at a multiple of 4 (3 * 2 048 per chunk, the blob's base is aligned): whole words are
  // assembled from byte loads — a source run starts at any byte — and stored once; the last 3 m mod 4 bytes go one by one
  uint8_t* out = rgb + 3u * begin;
  const uint32_t bytes = 3u * m, words = bytes >> 2;
  for (uint32_t w = threadIdx.x; w < words; w += 256u) {
    uint32_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t e = 4u * w + k, p = e / 3u, c = e - 3u * p;
      v |= (uint32_t)parts[s_part[p]].rgb[3ull * s_src[p] + c] << (8u * k);
    }
    reinterpret_cast<uint32_t*>(out)[w] = v;
  }
  for (uint32_t e = 4u * words + threadIdx.x; e < bytes; e += 256u) {
    const uint32_t p = e / 3u, c = e - 3u * p;
    out[e] = parts[s_part[p]].rgb[3ull * s_src[p] + c];
  }
}

}  // namespace

struct pcv_s2_stream {
  pcv_ctx* ctx = nullptr;
  uint32_t level = 0;
  bool dir_mode = false, append_mode = false;
  std::string directory;
  uint64_t flush_points = 0;
  uint64_t memory_cap = kMemoryPointCap;
  bool decided = false, has_intensity = false;  // the first non-empty batch (or the directory appended to) decides
  std::vector<std::pair<std::string, int32_t>> extras;  // ... and the extra attributes, ascending by name
  bool broken = false;                          // a flush failed in the middle of an append: only finish / abort are left
  uint64_t batches = 0, points = 0, pending_points = 0, flushes = 0;
  std::vector<pcv_s2_cloud*> parts;  // pending, non-empty, in batch order
  std::vector<uint64_t> part_base;   // points of the stream before each pending part
  // all that is held between flushes: points per cell (with the cells of the directory appended to), the bounding box, and
  // which cells this stream has written already (their files are appended to from then on, s2.rs:121-136)
  std::map<uint64_t, uint64_t> cell_counts;
  std::unordered_set<uint64_t> written;
  bool have_box = false;
  double bbox_min[3] = {0, 0, 0}, bbox_max[3] = {0, 0, 0};

  void fold_box(const double lo[3], const double hi[3]) {
    for (int a = 0; a < 3; ++a) {
      if (!have_box || lo[a] < bbox_min[a]) bbox_min[a] = lo[a];
      if (!have_box || hi[a] > bbox_max[a]) bbox_max[a] = hi[a];
    }
    have_box = true;
  }
  void drop_parts() {
    for (pcv_s2_cloud* p : parts) pcv_s2_release(p);
    parts.clear();
    part_base.clear();
    pending_points = 0;
  }
};

namespace {

// The pending parts as one cloud (consumed either way). One part is its own merge.
int merge_pending(pcv_s2_stream* s, pcv_s2_cloud** out) {
  pcv_ctx* ctx = s->ctx;
  *out = nullptr;
  const bool with_order = !s->dir_mode;
  if (s->parts.size() == 1 && s->part_base[0] == 0) {  // (its extras come along as they are)
    *out = s->parts[0];
    s->parts.clear();
    s->drop_parts();
    return PCV_OK;
  }
  pcv_s2_cloud* c = new pcv_s2_cloud();
  c->ctx = ctx, c->level = s->level, c->has_intensity = s->has_intensity;
  PcvS2MergePlan plan;
  int rc = PCV_OK;
  {
    std::vector<PcvS2MergePart> in(s->parts.size());
    uint64_t total = 0;
    for (size_t p = 0; p < s->parts.size(); ++p) {
      in[p].ids = s->parts[p]->ids.data(), in[p].counts = s->parts[p]->counts.data(), in[p].num_cells = s->parts[p]->ids.size();
      total += s->parts[p]->n;
    }
    std::string why;
    if (pcv_s2_merge_plan(in.data(), (uint32_t)in.size(), kMergeChunkPoints, &plan, &why)) rc = ctx->fail(PCV_E_HIP, "the merge plan of the stream's parts: " + why);
    else if (plan.n != total || total >= kMemoryPointCap) rc = ctx->fail(PCV_E_HIP, "the merge plan does not cover the stream's parts");
  }
  const uint64_t n = plan.n, num_segments = plan.segments.size(), num_chunks = plan.chunk_first_segment.size();
  if (rc == PCV_OK && n > 0) {
    rc = [&]() -> int {
      PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
      PcvScratch sc(ctx);
      std::vector<MergePart> table(s->parts.size());
      std::vector<uint64_t> seg_dst(num_segments);
      for (size_t p = 0; p < s->parts.size(); ++p) {
        const pcv_s2_cloud* part = s->parts[p];
        table[p] = MergePart{(const double*)part->d_xyz, part->d_rgb, (const float*)part->d_int, part->d_order, s->part_base[p]};
      }
      for (uint64_t k = 0; k < num_segments; ++k) seg_dst[k] = plan.segments[k].dst_offset;
      MergePart* d_parts;
      uint64_t *d_seg_dst, *d_chunk_first;
      pcv_s2_merge_segment* d_segs;
      int r;
      if ((r = sc.get(&d_parts, table.size())) || (r = sc.get(&d_seg_dst, num_segments)) || (r = sc.get(&d_segs, num_segments)) ||
          (r = sc.get(&d_chunk_first, num_chunks)))
        return r;
      if ((with_order && (r = ctx->dev_alloc((void**)&c->d_order, n * 4))) || (r = ctx->dev_alloc((void**)&c->d_xyz, n * 24)) ||
          (r = ctx->dev_alloc((void**)&c->d_rgb, n * 3)) || (c->has_intensity && (r = ctx->dev_alloc((void**)&c->d_int, n * 4))))
        return r;
      if ((uintptr_t)c->d_rgb & 3u) return ctx->fail(PCV_E_HIP, "the merged rgb blob is not word aligned");
      if ((r = ctx->h2d(d_parts, table.data(), table.size() * sizeof(MergePart))) || (r = ctx->h2d(d_seg_dst, seg_dst.data(), num_segments * 8)) ||
          (r = ctx->h2d(d_segs, plan.segments.data(), num_segments * sizeof(pcv_s2_merge_segment))) ||
          (r = ctx->h2d(d_chunk_first, plan.chunk_first_segment.data(), num_chunks * 8)))
        return r;
      {
        PcvProf prof(ctx, PCV_K_S2_MERGE);
        hipLaunchKernelGGL(s2_merge_kernel, dim3((uint32_t)num_chunks), dim3(256), 0, ctx->stream, n, num_segments, num_chunks, d_seg_dst, d_segs,
                           d_chunk_first, d_parts, (double*)c->d_xyz, c->d_rgb, (float*)c->d_int, c->d_order);
      }
      PCV_HIP_CHECK(ctx, hipGetLastError());
      // the extras: one launch each over the same plan (pcv_s2_attr.hip)
      if (!s->extras.empty() && (r = pcv_s2_attr_merge(ctx, sc, n, num_segments, num_chunks, d_seg_dst, d_segs, d_chunk_first, s->parts, c))) return r;
      PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the tables above are host vectors and scratch of this scope)
      ctx->prof_resolve();
      return PCV_OK;
    }();
  }
  if (rc != PCV_OK) (void)hipStreamSynchronize(ctx->stream);
  s->drop_parts();  // after the synchronisation: nothing queued reads them
  if (rc != PCV_OK) {
    pcv_s2_release(c);
    return rc;
  }
  c->n = n;
  c->ids.swap(plan.ids), c->counts.swap(plan.counts), c->offsets.swap(plan.offsets);
  *out = c;
  return PCV_OK;
}

// directory mode: the pending parts merged, downloaded and appended to the cells' files
int flush(pcv_s2_stream* s) {
  pcv_ctx* ctx = s->ctx;
  if (s->parts.empty()) return PCV_OK;
  // (a part standing alone is taken as it is: its base does not matter without an input order)
  if (s->parts.size() == 1) s->part_base[0] = 0;
  pcv_s2_cloud* c;
  int rc = merge_pending(s, &c);
  if (rc != PCV_OK) return rc;
  uint8_t *h_xyz = nullptr, *h_rgb = nullptr, *h_int = nullptr;
  if ((rc = ctx->host_alloc((void**)&h_xyz, c->n * 24)) == PCV_OK && (rc = ctx->host_alloc((void**)&h_rgb, c->n * 3)) == PCV_OK && c->has_intensity)
    rc = ctx->host_alloc((void**)&h_int, c->n * 4);
  if (rc == PCV_OK && (hipMemcpyAsync(h_xyz, c->d_xyz, c->n * 24, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                       hipMemcpyAsync(h_rgb, c->d_rgb, c->n * 3, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                       (h_int && hipMemcpyAsync(h_int, c->d_int, c->n * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
                       hipStreamSynchronize(ctx->stream) != hipSuccess))
    rc = ctx->fail(PCV_E_HIP, "downloading the merged cell blobs failed");
  if (rc == PCV_OK) {
    std::vector<uint8_t> truncate(c->ids.size());
    for (size_t k = 0; k < c->ids.size(); ++k) truncate[k] = !s->append_mode && s->written.insert(c->ids[k]).second ? 1 : 0;
    std::string error;
    rc = pcv_s2_write_cells(s->directory.c_str(), c->ids.size(), c->ids.data(), c->counts.data(), c->offsets.data(), truncate.data(), h_xyz, h_rgb,
                            h_int, &error);
    if (rc != PCV_OK) ctx->fail(rc, error);
    if (rc == PCV_OK && !c->extras.empty()) rc = pcv_s2_attr_write(c, s->directory.c_str(), truncate.data());
  }
  if (h_xyz) ctx->host_release(h_xyz);
  if (h_rgb) ctx->host_release(h_rgb);
  if (h_int) ctx->host_release(h_int);
  (void)hipStreamSynchronize(ctx->stream);
  pcv_s2_release(c);
  if (rc == PCV_OK) s->flushes += 1;
  return rc;
}

void destroy(pcv_s2_stream* s) {
  if (s->ctx) {
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
  }
  s->drop_parts();
  delete s;
}

}  // namespace

extern "C" int pcv_s2_merge_plan_host(uint32_t num_parts, const uint64_t* part_first, const uint64_t* part_ids, const uint64_t* part_counts,
                                      uint32_t chunk_points, uint64_t* num_cells, uint64_t* num_segments, uint64_t* num_chunks,
                                      uint64_t* ids, uint64_t* counts, uint64_t* offsets, pcv_s2_merge_segment* segments,
                                      uint64_t* chunk_first_segment) {
  if (!part_first) return pcv_host_fail(PCV_E_INVALID, "part_first is null");
  if (part_first[0] != 0) return pcv_host_fail(PCV_E_INVALID, "part_first[0] must be 0");
  for (uint32_t p = 0; p < num_parts; ++p)
    if (part_first[p + 1] < part_first[p]) return pcv_host_fail(PCV_E_INVALID, "part_first must not descend");
  if (part_first[num_parts] && (!part_ids || !part_counts)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  std::vector<PcvS2MergePart> parts(num_parts);
  for (uint32_t p = 0; p < num_parts; ++p)
    parts[p] = PcvS2MergePart{part_ids + part_first[p], part_counts + part_first[p], part_first[p + 1] - part_first[p]};
  PcvS2MergePlan plan;
  std::string why;
  if (pcv_s2_merge_plan(parts.data(), num_parts, chunk_points ? chunk_points : kMergeChunkPoints, &plan, &why)) return pcv_host_fail(PCV_E_INVALID, why);
  if (num_cells) *num_cells = plan.ids.size();
  if (num_segments) *num_segments = plan.segments.size();
  if (num_chunks) *num_chunks = plan.chunk_first_segment.size();
  if (ids && !plan.ids.empty()) std::memcpy(ids, plan.ids.data(), plan.ids.size() * 8);
  if (counts && !plan.ids.empty()) std::memcpy(counts, plan.counts.data(), plan.ids.size() * 8);
  if (offsets && !plan.ids.empty()) std::memcpy(offsets, plan.offsets.data(), plan.ids.size() * 8);
  if (segments && !plan.segments.empty()) std::memcpy(segments, plan.segments.data(), plan.segments.size() * sizeof(pcv_s2_merge_segment));
  if (chunk_first_segment && !plan.chunk_first_segment.empty())
    std::memcpy(chunk_first_segment, plan.chunk_first_segment.data(), plan.chunk_first_segment.size() * 8);
  return PCV_OK;
}

extern "C" int pcv_s2_stream_begin(pcv_ctx* ctx, const pcv_s2_stream_params* params, pcv_s2_stream** out) {
  auto fail = [&](int code, const std::string& m) { return ctx ? ctx->fail(code, m) : pcv_host_fail(code, m); };
  if (!params || !out) return fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (params->struct_size < sizeof(pcv_s2_stream_params)) return fail(PCV_E_INVALID, "pcv_s2_stream_params.struct_size is too small");
  if (params->split_level > (uint32_t)s2::kMaxLevel) return fail(PCV_E_INVALID, "an S2 split level is 0 ..= 30");
  if (params->open_mode != PCV_S2_TRUNCATE && params->open_mode != PCV_S2_APPEND) return fail(PCV_E_INVALID, "open_mode must be PCV_S2_TRUNCATE or PCV_S2_APPEND");
  if (!params->directory && params->open_mode == PCV_S2_APPEND) return fail(PCV_E_INVALID, "PCV_S2_APPEND needs a directory");
  if (params->flush_points > kMaxFlushPoints) return fail(PCV_E_INVALID, "flush_points is 2^31 at most");
  pcv_s2_stream* s = new pcv_s2_stream();
  s->ctx = ctx, s->level = params->split_level;
  if (params->directory) {
    s->dir_mode = true;
    s->directory = params->directory;
    s->append_mode = params->open_mode == PCV_S2_APPEND;
    s->flush_points = params->flush_points ? params->flush_points : kDefaultFlushPoints;
  }
  if (s->append_mode) {  // OpenMode::Append: what the directory holds is part of what get_meta will report (a departure)
    PcvS2Dir meta;
    std::string error;
    const int rc = pcv_s2_read_meta(s->directory.c_str(), &meta, &error);
    if (rc != PCV_OK) {
      delete s;
      return fail(rc, error);
    }
    for (size_t k = 0; k < meta.ids.size(); ++k) {
      const uint64_t id = meta.ids[k];
      const uint32_t tz = id ? (uint32_t)__builtin_ctzll(id) : 1u;
      if ((tz & 1u) || tz > 60u || (uint32_t)s2::kMaxLevel - (tz >> 1) != s->level) {
        delete s;
        return fail(PCV_E_INVALID, "PCV_S2_APPEND: cell " + pcv_s2_token(id) + " of " + params->directory + " is not of split level " +
                                       std::to_string(params->split_level));
      }
      s->cell_counts[id] += meta.counts[k];
      s->points += meta.counts[k];
    }
    if (s->points) s->fold_box(meta.bbox_min, meta.bbox_max);
    s->decided = true, s->has_intensity = meta.has_intensity;
    s->extras = meta.extras;
  }
  if (!ctx) {
    delete s;
    return fail(PCV_E_INVALID, "ctx is null");
  }
  *out = s;
  return PCV_OK;
}

extern "C" int pcv_s2_stream_set_memory_cap(pcv_s2_stream* s, uint64_t max_points) {
  if (!s) return PCV_E_INVALID;
  if (max_points == 0 || max_points > kMemoryPointCap) return s->ctx->fail(PCV_E_INVALID, "the cap of an in-memory stream is 1 ..= 2^32 - 1");
  s->memory_cap = max_points;
  return PCV_OK;
}

extern "C" int pcv_s2_stream_append(pcv_s2_stream* s, const pcv_points* batch) { return pcv_s2_stream_append_ex(s, batch, nullptr, 0); }

extern "C" int pcv_s2_stream_append_ex(pcv_s2_stream* s, const pcv_points* batch, const pcv_attribute* attrs, uint32_t num_attrs) {
  if (!s) return PCV_E_INVALID;
  pcv_ctx* ctx = s->ctx;
  if (s->broken) return ctx->fail(PCV_E_INVALID, "this S2 stream failed while flushing; finish or abort it");
  if (!batch) return ctx->fail(PCV_E_INVALID, "points is null");
  const std::string which = " (batch " + std::to_string(s->batches) + " of the stream)";
  std::vector<PcvS2Extra> extras;
  {
    std::string why;
    if (pcv_s2_attr_check(attrs, num_attrs, batch->n, &extras, &why)) return ctx->fail(PCV_E_INVALID, why + which);
  }
  if (batch->n > 0 && batch->n < kMemoryPointCap) {
    if (s->decided && s->has_intensity != (batch->intensity != nullptr))
      return ctx->fail(PCV_E_INVALID, "S2Splitter received incompatible data types for attribute intensity" + which);  // s2.rs:155
    if (s->decided) {  // another type, an unknown name — and a missing one, which the reference lets through
      const char* bad = nullptr;
      for (const PcvS2Extra& e : extras) {
        bool known = false;
        for (const auto& have : s->extras) known = known || (have.first == e.name && have.second == e.data_type);
        if (!known && !bad) bad = e.name.c_str();
      }
      for (const auto& have : s->extras) {
        bool given = false;
        for (const PcvS2Extra& e : extras) given = given || e.name == have.first;
        if (!given && !bad) bad = have.first.c_str();
      }
      if (bad) return ctx->fail(PCV_E_INVALID, std::string("S2Splitter received incompatible data types for attribute ") + bad + which);
    }
    if (!s->dir_mode && batch->n >= s->memory_cap - std::min(s->points, s->memory_cap))
      return ctx->fail(PCV_E_INVALID, "an in-memory S2 stream holds fewer than " + std::to_string(s->memory_cap) +
                                          " points; a stream with a directory has no such limit" + which);
    // a flush handles fewer than 2^32 - 1 points: what is pending goes first where this batch would cross that
    if (s->dir_mode && s->pending_points + batch->n >= kMemoryPointCap) {
      const int rc = flush(s);
      if (rc != PCV_OK) {
        s->broken = true;
        return rc;
      }
    }
  }
  pcv_s2_cloud* part;
  int rc = pcv_s2_split_part(ctx, batch, s->level, !s->dir_mode, &part, &extras);
  if (rc != PCV_OK) return rc == PCV_E_INVALID ? ctx->fail(rc, ctx->last_error + which) : rc;
  s->batches += 1;
  if (part->n == 0) {
    pcv_s2_release(part);
    return PCV_OK;
  }
  if (!s->decided) s->decided = true, s->has_intensity = part->has_intensity, s->extras = pcv_s2_extra_list(part);
  s->fold_box(part->bbox_min, part->bbox_max);
  for (size_t k = 0; k < part->ids.size(); ++k) s->cell_counts[part->ids[k]] += part->counts[k];
  s->parts.push_back(part);
  s->part_base.push_back(s->points);
  s->points += part->n;
  s->pending_points += part->n;
  if (s->dir_mode && s->pending_points >= s->flush_points) {
    rc = flush(s);
    if (rc != PCV_OK) s->broken = true;
  }
  return rc;
}

extern "C" int pcv_s2_stream_info(const pcv_s2_stream* s, uint64_t* batches, uint64_t* points, uint64_t* cells, uint64_t* pending_points,
                                  uint64_t* flushes) {
  if (!s) return PCV_E_INVALID;
  if (batches) *batches = s->batches;
  if (points) *points = s->points;
  if (cells) *cells = s->cell_counts.size();
  if (pending_points) *pending_points = s->pending_points;
  if (flushes) *flushes = s->flushes;
  return PCV_OK;
}

extern "C" int pcv_s2_stream_finish(pcv_s2_stream* s, pcv_s2_cloud** out) {
  if (!s) return PCV_E_INVALID;
  pcv_ctx* ctx = s->ctx;
  if (out) *out = nullptr;
  int rc = PCV_OK;
  if (s->broken) rc = ctx->fail(PCV_E_INVALID, "this S2 stream failed while flushing: " + ctx->last_error);
  if (rc == PCV_OK && !s->dir_mode) {
    if (!out) rc = ctx->fail(PCV_E_INVALID, "out is null");
    pcv_s2_cloud* c = nullptr;
    if (rc == PCV_OK) {
      if (s->parts.empty()) {  // what pcv_s2_split makes of no points
        c = new pcv_s2_cloud();
        c->ctx = ctx, c->level = s->level, c->has_intensity = s->decided && s->has_intensity;
        for (const auto& a : s->extras) {
          PcvS2Extra e;
          e.name = a.first, e.data_type = a.second, e.elem = pcv_s2_attr_size(a.second);
          c->extras.push_back(std::move(e));
        }
      } else {
        rc = merge_pending(s, &c);
      }
    }
    if (rc == PCV_OK) {
      std::memcpy(c->bbox_min, s->bbox_min, 24);
      std::memcpy(c->bbox_max, s->bbox_max, 24);
      *out = c;
    }
  } else if (rc == PCV_OK) {
    rc = flush(s);
    if (rc == PCV_OK) {
      std::vector<uint64_t> ids, counts;
      ids.reserve(s->cell_counts.size()), counts.reserve(s->cell_counts.size());
      for (const auto& kv : s->cell_counts) ids.push_back(kv.first), counts.push_back(kv.second);
      std::string error;
      rc = pcv_s2_write_meta(s->directory.c_str(), s->bbox_min, s->bbox_max, ids.size(), ids.data(), counts.data(), s->decided && s->has_intensity,
                             &error, &s->extras);
      if (rc != PCV_OK) ctx->fail(rc, error);
    }
    if (rc == PCV_OK && out) rc = pcv_s2_open_dir(ctx, s->directory.c_str(), out);
  }
  destroy(s);
  return rc;
}

extern "C" void pcv_s2_stream_abort(pcv_s2_stream* s) {
  if (s) destroy(s);
}
