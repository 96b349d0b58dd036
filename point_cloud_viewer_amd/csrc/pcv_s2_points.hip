// pcv_s2_points.hip — the batched point query over an S2 cell cloud: FilteredIterator over NodeIterator with Encoding::Plain
// (reference src/iterator.rs:96-119, src/s2_cells/mod.rs:171-191) for every (location, listed cell) of one call.
//
//   cells    the lists of pcv_s2_query.hip (pcv_s2_cells_in_location), read back: the counts, then the lists at the longest
//            one's length; one segment per (location, listed cell), locations one after another, cells ascending; the
//            segments' candidates laid out back to back in chunks of 1 024 (pcv_s2_query_dev.h)
//   flags    s2_flags_kernel<KIND>: one workgroup per chunk, an instance per shape kind (PCV_SHAPE_FRUSTUM for both frusta, the
//            web-mercator chain and the cell-union search in instances of their own, so the others keep their registers); the
//            points are the cloud's 24-byte AoS f64, a wave's 64 points one contiguous 1 536-byte run, untouched
//   filter   the intervals on extra attributes (pcv_s2_query_run_ex): launches of their own, pcv_s2_attr.hip, ANDed into the flags
//   scan     flags -> u64 offsets (pcv_batch_scan); a segment's offset is the offset of its first candidate
//   gather   s2_gather_points_kernel: the kept points of a segment range into x / y / z planes, rgb and intensity
#include <algorithm>
#include <cstring>

#include "pcv_internal.h"
#include "pcv_contain_dev.h"
#include "pcv_polygon_dev.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_dev.h"
#include "pcv_s2_query_dev.h"

namespace {

using Chunk = PcvS2Chunk;
constexpr uint32_t kChunkPoints = kS2ChunkPoints;
constexpr int kKindUnion = 100;  // a cell union: not a PCV_SHAPE_*
constexpr int kKindPolygon = 101;  // a web-mercator polygon (the point kind of its shape; its device kind is the bounding rectangle's)

struct Ival {  // ClosedInterval of one location on intensity
  double lo, hi;
  uint32_t used, pad;
};
struct UnionRef {
  uint32_t first, count;
};

template <int KIND>
__global__ __launch_bounds__(256) void s2_flags_kernel(const Chunk* __restrict__ chunks, const uint32_t* __restrict__ which,
                                                        const PcvShapeDev* __restrict__ shapes, uint32_t num_shapes,
                                                        const UnionRef* __restrict__ unions, const uint64_t* __restrict__ union_cells,
                                                        const Ival* __restrict__ ivals, const double* __restrict__ xyz,
                                                        const float* __restrict__ inten, uint32_t* __restrict__ flags) {
  const Chunk c = chunks[which[blockIdx.x]];
  const Ival iv = ivals[c.location];
  ContainParams<KIND == kKindUnion || KIND == kKindPolygon ? PCV_SHAPE_ALL : KIND> shape;
  UnionRef u{0, 0};
  const double* edges = nullptr;  // the polygon's point rule table (workgroup-uniform)
  uint32_t nedges = 0;
  if constexpr (KIND == kKindUnion) u = unions[c.location - num_shapes];
  else if constexpr (KIND == kKindPolygon) edges = shapes[c.location].polygon.edges, nedges = shapes[c.location].polygon.nedges;
  else shape = load_contain<KIND>(shapes + c.location);
  for (uint32_t q = threadIdx.x; q < c.count; q += 256u) {
    const uint64_t i = c.src + q;
    const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    bool k;
    if constexpr (KIND == kKindUnion) {
      k = s2::union_contains(union_cells + u.first, u.count, s2::leaf_from_point(px, py, pz));
    } else if constexpr (KIND == kKindPolygon) {  // the projection once per point, then the edges
      double wu, wv;
      wmr::project(px, py, pz, &wu, &wv);
      k = poly::inside(edges, nedges, wu, wv);
    } else {
      k = shape_contains<KIND>(shape, V3d{px, py, pz});
    }
    if (iv.used) {  // iterator.rs:82-91 + math/mod.rs:86-88
      const double a = (double)inten[i];
      k = k && (iv.lo <= a && a <= iv.hi);
    }
    flags[c.first + q] = k ? 1u : 0u;
  }
}

// the kept points of chunks [first_chunk, first_chunk + gridDim.x) to out index offsets[candidate] - base
__global__ __launch_bounds__(256) void s2_gather_points_kernel(const Chunk* __restrict__ chunks, uint64_t first_chunk,
                                                                const uint32_t* __restrict__ flags, const uint64_t* __restrict__ offsets,
                                                                uint64_t base, const double* __restrict__ xyz, const uint8_t* __restrict__ rgb,
                                                                const float* __restrict__ inten, double* __restrict__ ox,
                                                                double* __restrict__ oy, double* __restrict__ oz, uint8_t* __restrict__ orgb,
                                                                float* __restrict__ ointen) {
  const Chunk c = chunks[first_chunk + blockIdx.x];
  for (uint32_t q = threadIdx.x; q < c.count; q += 256u) {
    if (!flags[c.first + q]) continue;
    const uint64_t i = c.src + q, o = offsets[c.first + q] - base;
    if (ox) ox[o] = xyz[3 * i];
    if (oy) oy[o] = xyz[3 * i + 1];
    if (oz) oz[o] = xyz[3 * i + 2];
    if (orgb) {
      orgb[3 * o] = rgb[3 * i];
      orgb[3 * o + 1] = rgb[3 * i + 1];
      orgb[3 * o + 2] = rgb[3 * i + 2];
    }
    if (ointen) ointen[o] = inten[i];
  }
}

__global__ __launch_bounds__(256) void s2_pick_offsets_kernel(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ at, uint64_t n,
                                                               uint64_t* __restrict__ out) {
  const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (k < n) out[k] = offsets[at[k]];
}

int kind_of(const pcv_shapes* shapes, uint32_t num_shapes, uint32_t location) {
  if (location >= num_shapes) return kKindUnion;
  switch (shapes->kinds[location]) {
    case PCV_SHAPE_AABB: return PCV_SHAPE_AABB;
    case PCV_SHAPE_FRUSTUM:
    case PCV_SHAPE_FRUSTUM_WITH_INVERSE: return PCV_SHAPE_FRUSTUM;
    case PCV_SHAPE_OBB: return PCV_SHAPE_OBB;
    case PCV_SHAPE_WEB_MERCATOR_RECT: return PCV_SHAPE_WEB_MERCATOR_RECT;
    case PCV_SHAPE_S2_CELL_UNION: return kKindUnion;  // a union member of the table: the union location it is
    case PCV_SHAPE_POLYGON: return kKindPolygon;      // (web-mercator: pcv_s2_cells_in_location refuses the xy frame)
    default: return PCV_SHAPE_ALL;
  }
}

void release_query(pcv_s2_query* b) {
  if (!b) return;
  pcv_ctx* ctx = b->cloud->ctx;
  (void)hipSetDevice(ctx->device);
  if (b->d_chunks) ctx->dev_free(b->d_chunks);
  if (b->d_flags) ctx->dev_free(b->d_flags);
  if (b->d_offsets) ctx->dev_free(b->d_offsets);
  delete b;
}

int run_impl(pcv_s2_cloud* c, const pcv_shapes* shapes, uint32_t num_unions, const uint32_t* union_first, const uint64_t* union_cells,
             const double* intervals, const uint8_t* interval_used, pcv_s2_query* b, const std::vector<PcvS2ExtraFilter>* extra_filters = nullptr) {
  pcv_ctx* ctx = c->ctx;
  hipStream_t st = ctx->stream;
  const uint32_t num_shapes = shapes ? shapes->count : 0;
  const uint64_t locations = (uint64_t)num_shapes + num_unions;
  const uint32_t ncells = (uint32_t)c->ids.size();
  b->location_first.assign(locations + 1, 0);
  b->seg_offset.assign(1, 0);
  b->seg_first_chunk.assign(1, 0);
  if (locations == 0 || ncells == 0) return PCV_OK;
  int rc;
  // ---- cell lists, read back: the segments ----
  // the counts first, then the lists at the longest one's length: rows of `cap`, not of every cell of the cloud (many small
  // locations over many cells, xray's leaf tiles, would otherwise cost locations x cells on the host and the device)
  std::vector<uint32_t> counts(locations);
  if ((rc = pcv_s2_cells_in_location(c, shapes, num_unions, union_first, union_cells, 0, counts.data(), nullptr))) return rc;
  const uint32_t cap = *std::max_element(counts.begin(), counts.end());
  std::vector<uint32_t> lists((size_t)locations * cap);
  if (cap && (rc = pcv_s2_cells_in_location(c, shapes, num_unions, union_first, union_cells, cap, counts.data(), lists.data()))) return rc;
  if ((rc = pcv_s2_make_resident(c))) return rc;
  std::vector<Chunk> chunks;
  std::vector<uint64_t> seg_candidate(1, 0);
  std::vector<std::vector<uint32_t>> by_kind(kKindPolygon + 1);
  for (uint64_t l = 0; l < locations; ++l) {
    const int kind = kind_of(shapes, num_shapes, (uint32_t)l);
    for (uint32_t k = 0; k < counts[l]; ++k) {
      const uint32_t cell = lists[l * cap + k];
      b->seg_cell.push_back(cell);
      uint64_t left = c->counts[cell], src = c->offsets[cell];
      while (left) {
        const uint32_t take = (uint32_t)std::min<uint64_t>(left, kChunkPoints);
        by_kind[kind].push_back((uint32_t)chunks.size());
        chunks.push_back(Chunk{src, b->candidates, take, (uint32_t)l});
        src += take, left -= take, b->candidates += take;
      }
      seg_candidate.push_back(b->candidates);
      b->seg_first_chunk.push_back(chunks.size());
    }
    b->location_first[l + 1] = b->seg_cell.size();
  }
  b->nseg = b->seg_cell.size();
  b->seg_offset.assign(b->nseg + 1, 0);
  if (chunks.size() >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "too many candidate points for one S2 query: split the locations");
  if (b->candidates == 0) return PCV_OK;
  // ---- uploads ----
  PcvScratch sc(ctx);
  std::vector<Ival> ivals(locations, Ival{0, 0, 0, 0});
  for (uint64_t l = 0; l < locations && intervals; ++l)
    if (!interval_used || interval_used[l]) ivals[l] = Ival{intervals[2 * l], intervals[2 * l + 1], 1u, 0u};
  // one reference per LOCATION (the union instance is launched with num_shapes = 0): the call's unions, and the table's own
  // union members, whose cells sit behind the call's in d_union
  const uint32_t own_total = num_unions ? union_first[num_unions] : 0;
  const size_t table_total = shapes ? shapes->union_cells.size() : 0;
  std::vector<UnionRef> urefs(locations, UnionRef{0, 0});
  for (uint32_t u = 0; u < num_unions; ++u) urefs[num_shapes + u] = UnionRef{union_first[u], union_first[u + 1] - union_first[u]};
  for (size_t k = 0; shapes && k < shapes->union_shapes.size(); ++k) {
    const uint32_t u = shapes->union_of[k];
    urefs[shapes->union_shapes[k]] = UnionRef{own_total + shapes->union_first[u], shapes->union_first[u + 1] - shapes->union_first[u]};
  }
  const size_t union_total = own_total + table_total;
  std::vector<uint32_t> which;
  for (const auto& v : by_kind) which.insert(which.end(), v.begin(), v.end());
  Ival* d_ivals;
  UnionRef* d_urefs;
  uint64_t *d_union, *d_at, *d_seg_off;
  uint32_t* d_which;
  if ((rc = ctx->dev_alloc((void**)&b->d_chunks, chunks.size() * sizeof(Chunk))) || (rc = ctx->dev_alloc((void**)&b->d_flags, b->candidates * 4)) ||
      (rc = ctx->dev_alloc((void**)&b->d_offsets, (b->candidates + 1) * 8)) || (rc = sc.get(&d_ivals, locations)) ||
      (rc = sc.get(&d_urefs, urefs.size())) || (rc = sc.get(&d_union, (size_t)union_total + 1)) || (rc = sc.get(&d_which, which.size())) ||
      (rc = sc.get(&d_at, b->nseg + 1)) || (rc = sc.get(&d_seg_off, b->nseg + 1)))
    return rc;
  if ((rc = ctx->h2d(b->d_chunks, chunks.data(), chunks.size() * sizeof(Chunk))) || (rc = ctx->h2d(d_ivals, ivals.data(), locations * sizeof(Ival))) ||
      (rc = ctx->h2d(d_urefs, urefs.data(), urefs.size() * sizeof(UnionRef))) || (rc = ctx->h2d(d_which, which.data(), which.size() * 4)) ||
      (rc = ctx->h2d(d_at, seg_candidate.data(), (b->nseg + 1) * 8)) || (own_total && (rc = ctx->h2d(d_union, union_cells, (size_t)own_total * 8))) ||
      (table_total && (rc = ctx->h2d(d_union + own_total, shapes->union_cells.data(), table_total * 8))))
    return rc;
  // ---- flags, one launch per kind that occurs ----
  {
    PcvProf prof(ctx, PCV_K_S2_FLAGS);
    const uint32_t* w = d_which;
    const PcvShapeDev* dev = shapes ? shapes->dev : nullptr;
#define LAUNCH(KIND)                                                                                                                    \
  if (!by_kind[KIND].empty()) {                                                                                                         \
    hipLaunchKernelGGL(s2_flags_kernel<KIND>, dim3((uint32_t)by_kind[KIND].size()), dim3(256), 0, st, b->d_chunks, w, dev,              \
                       KIND == kKindUnion ? 0u : num_shapes,                                                                            \
                       d_urefs, d_union, d_ivals, (const double*)c->d_xyz, (const float*)c->d_int, b->d_flags);                           \
    w += by_kind[KIND].size();                                                                                                          \
  }
    // (the order of by_kind: ascending kind, as `which` was filled)
    LAUNCH(PCV_SHAPE_ALL) LAUNCH(PCV_SHAPE_AABB) LAUNCH(PCV_SHAPE_FRUSTUM) LAUNCH(PCV_SHAPE_OBB) LAUNCH(PCV_SHAPE_WEB_MERCATOR_RECT)
    LAUNCH(kKindUnion) LAUNCH(kKindPolygon)
#undef LAUNCH
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  // ---- the filters on extra attributes: one launch per distinct extra, after the flags and before the scan ----
  if (extra_filters && !extra_filters->empty() && (rc = pcv_s2_attr_filter(ctx, sc, c, b->d_chunks, chunks, locations, *extra_filters, b->d_flags)))
    return rc;
  // ---- scan, the segments' offsets ----
  {
    PcvProf prof(ctx, PCV_K_QUERY_BATCH_SCAN);
    if ((rc = pcv_batch_scan(ctx, sc, b->d_flags, b->candidates, b->d_offsets))) return rc;
    hipLaunchKernelGGL(s2_pick_offsets_kernel, dim3((uint32_t)((b->nseg + 256) / 256)), dim3(256), 0, st, b->d_offsets, d_at, b->nseg + 1, d_seg_off);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(b->seg_offset.data(), d_seg_off, (b->nseg + 1) * 8, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ctx->prof_resolve();
  b->kept = b->seg_offset[b->nseg];
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_s2_query_run(pcv_s2_cloud* c, const pcv_shapes* shapes, uint32_t num_unions, const uint32_t* union_first,
                                const uint64_t* union_cells, const double* intervals, const uint8_t* interval_used, pcv_s2_query** out) {
  if (!c) return PCV_E_INVALID;
  if (!c->ctx) return c->fail(PCV_E_INVALID, "a cloud opened without a context has no device");
  pcv_ctx* ctx = c->ctx;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  const uint64_t locations = (uint64_t)(shapes ? shapes->count : 0) + num_unions;
  for (uint64_t l = 0; l < locations && intervals; ++l)
    if ((!interval_used || interval_used[l]) && !c->has_intensity)
      return ctx->fail(PCV_E_INVALID, "this S2 cell cloud has no intensity attribute to filter on");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  pcv_s2_query* b = new pcv_s2_query();
  b->cloud = c;
  const int rc = run_impl(c, shapes, num_unions, union_first, union_cells, intervals, interval_used, b);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    release_query(b);
    return rc;
  }
  *out = b;
  return PCV_OK;
}

// PointQuery::filter_intervals (iterator.rs:66-119) on any scalar attribute; "intensity" is pcv_s2_query_run's interval
extern "C" int pcv_s2_query_run_ex(pcv_s2_cloud* c, const pcv_shapes* shapes, uint32_t num_unions, const uint32_t* union_first,
                                   const uint64_t* union_cells, const pcv_s2_filter* filters, uint32_t num_filters, pcv_s2_query** out) {
  if (num_filters == 0) return pcv_s2_query_run(c, shapes, num_unions, union_first, union_cells, nullptr, nullptr, out);
  if (!c) return PCV_E_INVALID;
  if (!c->ctx) return c->fail(PCV_E_INVALID, "a cloud opened without a context has no device");
  pcv_ctx* ctx = c->ctx;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  if (!filters) return ctx->fail(PCV_E_INVALID, "filters is null");
  const uint64_t locations = (uint64_t)(shapes ? shapes->count : 0) + num_unions;
  std::vector<double> intervals(2 * locations + 2, 0.0);
  std::vector<uint8_t> used(locations + 1, 0);
  std::vector<PcvS2ExtraFilter> extra;
  bool on_intensity = false;
  for (uint32_t k = 0; k < num_filters; ++k) {
    const pcv_s2_filter& f = filters[k];
    const std::string name(f.attribute ? f.attribute : "");
    if (f.location >= locations)
      return ctx->fail(PCV_E_INVALID, "filter " + std::to_string(k) + " names location " + std::to_string(f.location) + ", the call has " + std::to_string(locations));
    if (name == "color") return ctx->fail(PCV_E_INVALID, "a filter takes a scalar attribute; 'color' is a vector attribute");
    if (name == "intensity") {
      if (!c->has_intensity) return ctx->fail(PCV_E_INVALID, "this S2 cell cloud has no intensity attribute to filter on");
      if (used[f.location]) return ctx->fail(PCV_E_INVALID, "two filters on attribute 'intensity' for location " + std::to_string(f.location));
      intervals[2 * f.location] = f.lo, intervals[2 * f.location + 1] = f.hi, used[f.location] = 1;
      on_intensity = true;
      continue;
    }
    const int e = c->find_extra(name.c_str());
    if (e < 0) return ctx->fail(PCV_E_INVALID, "Data type for attribute '" + name + "' not found.");  // lib.rs:94
    if (c->extras[(size_t)e].elem == 3 || c->extras[(size_t)e].elem == 24)
      return ctx->fail(PCV_E_INVALID, "a filter takes a scalar attribute; '" + name + "' is a vector attribute");
    for (const PcvS2ExtraFilter& o : extra)
      if (o.location == f.location && o.extra == e)
        return ctx->fail(PCV_E_INVALID, "two filters on attribute '" + name + "' for location " + std::to_string(f.location));
    extra.push_back(PcvS2ExtraFilter{f.location, e, f.lo, f.hi});
  }
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  pcv_s2_query* b = new pcv_s2_query();
  b->cloud = c;
  const int rc = run_impl(c, shapes, num_unions, union_first, union_cells, on_intensity ? intervals.data() : nullptr, used.data(), b, &extra);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    release_query(b);
    return rc;
  }
  *out = b;
  return PCV_OK;
}

int pcv_s2_query_run_every(pcv_s2_cloud* c, const pcv_shapes* shapes, const double* intervals, const std::vector<PcvS2ExtraFilter>& filters,
                           pcv_s2_query** out) {
  pcv_ctx* ctx = c->ctx;
  *out = nullptr;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  pcv_s2_query* b = new pcv_s2_query();
  b->cloud = c;
  const int rc = run_impl(c, shapes, 0, nullptr, nullptr, intervals, nullptr, b, &filters);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    release_query(b);
    return rc;
  }
  *out = b;
  return PCV_OK;
}

extern "C" int pcv_s2_query_sizes(const pcv_s2_query* b, uint64_t* num_segments, uint64_t* num_points) {
  if (!b) return PCV_E_INVALID;
  if (num_segments) *num_segments = b->nseg;
  if (num_points) *num_points = b->kept;
  return PCV_OK;
}

extern "C" int pcv_s2_query_segments(const pcv_s2_query* b, uint64_t* location_first_segment, uint32_t* segment_cell, uint64_t* segment_offset) {
  if (!b) return PCV_E_INVALID;
  if (location_first_segment) std::memcpy(location_first_segment, b->location_first.data(), b->location_first.size() * 8);
  if (segment_cell && b->nseg) std::memcpy(segment_cell, b->seg_cell.data(), b->nseg * 4);
  if (segment_offset) std::memcpy(segment_offset, b->seg_offset.data(), b->seg_offset.size() * 8);
  return PCV_OK;
}

extern "C" int pcv_s2_query_points(pcv_s2_query* b, uint64_t first_segment, uint64_t num_segments, uint64_t capacity, int mem, double* x,
                                   double* y, double* z, uint8_t* rgb, float* intensity) {
  if (!b) return PCV_E_INVALID;
  pcv_s2_cloud* c = b->cloud;
  pcv_ctx* ctx = c->ctx;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (first_segment > b->nseg || num_segments > b->nseg - first_segment) return ctx->fail(PCV_E_INVALID, "segment range past the end");
  if (intensity && !c->has_intensity) return ctx->fail(PCV_E_INVALID, "this S2 cell cloud has no intensity attribute");
  const uint64_t base = b->seg_offset[first_segment], count = b->seg_offset[first_segment + num_segments] - base;
  if (count > capacity) return ctx->fail(PCV_E_INVALID, "the segments hold " + std::to_string(count) + " points, capacity is " + std::to_string(capacity));
  const uint64_t chunk0 = b->seg_first_chunk[first_segment], nchunks = b->seg_first_chunk[first_segment + num_segments] - chunk0;
  if (count == 0 || nchunks == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  double *dx = x, *dy = y, *dz = z;
  uint8_t* drgb = rgb;
  float* dint = intensity;
  int rc;
  if (mem == PCV_MEM_HOST) {
    if ((x && (rc = sc.get(&dx, count))) || (y && (rc = sc.get(&dy, count))) || (z && (rc = sc.get(&dz, count))) ||
        (rgb && (rc = sc.get(&drgb, count * 3))) || (intensity && (rc = sc.get(&dint, count))))
      return rc;
  }
  {
    PcvProf prof(ctx, PCV_K_S2_GATHER_POINTS);
    hipLaunchKernelGGL(s2_gather_points_kernel, dim3((uint32_t)nchunks), dim3(256), 0, ctx->stream, b->d_chunks, chunk0, b->d_flags, b->d_offsets,
                       base, (const double*)c->d_xyz, c->d_rgb, (const float*)c->d_int, dx, dy, dz, drgb, dint);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (mem == PCV_MEM_HOST) {
    if (x) PCV_HIP_CHECK(ctx, hipMemcpyAsync(x, dx, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (y) PCV_HIP_CHECK(ctx, hipMemcpyAsync(y, dy, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (z) PCV_HIP_CHECK(ctx, hipMemcpyAsync(z, dz, count * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (rgb) PCV_HIP_CHECK(ctx, hipMemcpyAsync(rgb, drgb, count * 3, hipMemcpyDeviceToHost, ctx->stream));
    if (intensity) PCV_HIP_CHECK(ctx, hipMemcpyAsync(intensity, dint, count * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" void pcv_s2_query_free(pcv_s2_query* b) {
  if (b && b->cloud && b->cloud->ctx) (void)hipStreamSynchronize(b->cloud->ctx->stream);
  release_query(b);
}
