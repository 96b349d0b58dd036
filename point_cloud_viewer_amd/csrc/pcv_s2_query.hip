// pcv_s2_query.hip — S2Cells::nodes_in_location (reference src/s2_cells/mod.rs:160-241) for many locations in one call: the
// cells of a cloud that a shape's covering rect, or a cell union, intersects. The chain is pcv_s2_region_dev.h.
//
//   table      s2_cell_table_kernel: once per cloud, one lane per cell — rect bound, centre, (u, v) bounds, vertices and their
//              lat / lng as SoA planes of one double per cell (240 B per cell), kept on the cloud
//   locations  s2_location_kernel: one lane per shape — the 8 corners' leaf cells, normalize, the union's rect bound
//   pairs      s2_pair_kernel: one wave per location walking the cell table in id order, 64 cells a step — rect against rect
//              bound first (32 B per cell), the precise steps for the survivors, ballot + prefix popcount: every list ascends
//              by cell id without a sort. One pass with a capacity, like pcv_nodes_in_location.
#include <algorithm>
#include <cstring>

#include "pcv_internal.h"
#include "pcv_query_dev.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_region_dev.h"

namespace {

enum : int32_t { kLocNone = 0, kLocAll = 1, kLocRect = 2, kLocUnion = 3 };
struct S2Loc {
  int32_t mode;
  uint32_t union_first, union_count;
  uint32_t pad;
  double rect[4];
};

// AllPoints: every cell; a frustum without an inverse: none (as it has no nodes in an octree); else the corners' rect
__host__ __device__ inline void location_of_shape(int32_t kind, int32_t valid, const double* corners, S2Loc* loc) {
  loc->union_first = loc->union_count = loc->pad = 0;
  s2::rect_set_empty(loc->rect);
  if (kind == PCV_SHAPE_ALL) {
    loc->mode = kLocAll;
  } else if (!valid) {
    loc->mode = kLocNone;
  } else {
    loc->mode = s2::corners_rect(corners, loc->rect) ? kLocRect : kLocNone;
  }
}

using s2::load_geom;  // the layout of the cell table's planes: pcv_s2_region_dev.h
using s2::store_geom;

__global__ __launch_bounds__(256) void s2_cell_table_kernel(const uint64_t* __restrict__ ids, uint32_t n, double* __restrict__ table) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c >= n) return;
  s2::CellGeom g;
  s2::cell_geom(ids[c], &g);
  store_geom(g, table, n, c);
}

__global__ __launch_bounds__(64) void s2_location_kernel(const PcvShapeDev* __restrict__ shapes, uint32_t count, S2Loc* __restrict__ locs) {
  const uint32_t f = blockIdx.x * 64u + threadIdx.x;
  if (f >= count) return;
  S2Loc loc;
  location_of_shape(shapes[f].kind, shapes[f].valid, shapes[f].corners, &loc);
  locs[f] = loc;
}

__global__ __launch_bounds__(64) void s2_pair_kernel(const S2Loc* __restrict__ locs, const uint64_t* __restrict__ ids,
                                                      const double* __restrict__ table, uint32_t n,
                                                      const uint64_t* __restrict__ union_cells, uint32_t capacity,
                                                      uint32_t* __restrict__ counts, uint32_t* __restrict__ out) {
  const S2Loc loc = locs[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  uint32_t* row = out + (size_t)blockIdx.x * capacity;
  uint32_t count = 0;
  if (loc.mode != kLocNone) {
    for (uint32_t base = 0; base < n; base += 64u) {
      const uint32_t c = base + lane;
      bool hit = false;
      if (c < n) {
        if (loc.mode == kLocAll) {
          hit = true;
        } else if (loc.mode == kLocUnion) {
          hit = s2::union_intersects(union_cells + loc.union_first, loc.union_count, ids[c]);
        } else {
          const double bound[4] = {table[c], table[(size_t)n + c], table[2 * (size_t)n + c], table[3 * (size_t)n + c]};
          if (!s2::rect_empty(loc.rect) && s2::rect_intersects(loc.rect, bound)) {
            s2::CellGeom g;
            load_geom(table, n, c, ids[c], &g);
            hit = s2::rect_intersects_cell_after_bound(loc.rect, g);
          }
        }
      }
      const unsigned long long mask = __ballot(hit);
      const uint32_t at = count + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (hit && at < capacity) row[at] = c;
      count += (uint32_t)__popcll(mask);
    }
  }
  if (lane == 0) counts[blockIdx.x] = count;
}

int check_unions(uint32_t num_unions, const uint32_t* union_first, const uint64_t* union_cells, std::string* why) {
  if (num_unions == 0) return PCV_OK;
  if (!union_first) {
    *why = "union_first is null";
    return PCV_E_INVALID;
  }
  if (union_first[0] != 0) {
    *why = "union_first[0] must be 0";
    return PCV_E_INVALID;
  }
  for (uint32_t u = 0; u < num_unions; ++u) {
    if (union_first[u + 1] < union_first[u]) {
      *why = "union_first must not descend";
      return PCV_E_INVALID;
    }
    std::string inner;
    if (pcv_s2_check_union(union_cells ? union_cells + union_first[u] : nullptr, union_first[u + 1] - union_first[u], &inner)) {
      *why = "union " + std::to_string(u) + ": " + inner;
      return PCV_E_INVALID;
    }
    for (uint32_t k = union_first[u]; k < union_first[u + 1]; ++k)
      if (!s2::valid_cell(union_cells[k])) {
        *why = "union " + std::to_string(u) + ": cell " + std::to_string(k - union_first[u]) + " is no S2 cell id";
        return PCV_E_INVALID;
      }
  }
  return PCV_OK;
}

int check_cloud_cells(uint64_t num_cells, const uint64_t* ids, bool geometric, std::string* why) {
  if (num_cells >= 0xffffffffull) {
    *why = "an S2 cell cloud holds fewer than 2^32 - 1 cells";
    return PCV_E_INVALID;
  }
  for (uint64_t k = 0; k < num_cells; ++k) {
    if (!s2::valid_cell(ids[k]) || (k > 0 && ids[k] <= ids[k - 1])) {
      *why = "the cells of a cloud are S2 cell ids that ascend: cell " + std::to_string(k) + " is not";
      return PCV_E_INVALID;
    }
    if (geometric && s2::level_of(ids[k]) == 0u) {
      *why = "a cloud with a cell of level 0 takes no shape locations: Cell::rect_bound of a face is not provided";
      return PCV_E_INVALID;
    }
  }
  return PCV_OK;
}

// the ids and the cell table on the device, once per cloud
int prepare_cloud(pcv_s2_cloud* c, bool geometric) {
  pcv_ctx* ctx = c->ctx;
  const uint32_t n = (uint32_t)c->ids.size();
  if (n == 0) return PCV_OK;
  int rc;
  if (!c->d_ids) {
    if ((rc = ctx->dev_alloc((void**)&c->d_ids, (size_t)n * 8))) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(c->d_ids, c->ids.data(), (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  if (geometric && !c->d_table) {
    if ((rc = ctx->dev_alloc((void**)&c->d_table, (size_t)n * s2::kCellPlanes * 8))) return rc;
    {
      PcvProf prof(ctx, PCV_K_S2_CELL_TABLE);
      hipLaunchKernelGGL(s2_cell_table_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, c->d_ids, n, c->d_table);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  return PCV_OK;
}

}  // namespace

int pcv_s2_check_unions(uint32_t num_unions, const uint32_t* union_first, const uint64_t* union_cells, std::string* why) {
  return check_unions(num_unions, union_first, union_cells, why);
}

// ---- host twins (no context) --------------------------------------------------------------------------------------------
extern "C" int pcv_s2_cell_geometry_host(uint64_t cell, double geometry[30]) {
  if (!geometry) return pcv_host_fail(PCV_E_INVALID, "null argument");
  if (!s2::valid_cell(cell)) return pcv_host_fail(PCV_E_INVALID, "not an S2 cell id");
  if (s2::level_of(cell) == 0u) return pcv_host_fail(PCV_E_INVALID, "the geometry of a level-0 cell (a face) is not provided");
  s2::CellGeom g;
  s2::cell_geom(cell, &g);
  store_geom(g, geometry, 1, 0);
  return PCV_OK;
}

extern "C" int pcv_s2_cell_rect_host(uint64_t cell, double rect[4]) {
  double geometry[30];
  if (!rect) return pcv_host_fail(PCV_E_INVALID, "null argument");
  const int rc = pcv_s2_cell_geometry_host(cell, geometry);
  if (rc == PCV_OK) std::memcpy(rect, geometry, 32);
  return rc;
}

extern "C" int pcv_s2_corners_rect_host(const double corners[24], double rect[4]) {
  if (!corners || !rect) return pcv_host_fail(PCV_E_INVALID, "null argument");
  if (!s2::corners_rect(corners, rect)) return pcv_host_fail(PCV_E_INVALID, "the corners' cells normalize to a level-0 cell");
  return PCV_OK;
}

extern "C" int pcv_s2_rect_intersects_cell_host(const double rect[4], uint64_t cell, int* intersects) {
  if (!rect || !intersects) return pcv_host_fail(PCV_E_INVALID, "null argument");
  if (!s2::valid_cell(cell)) return pcv_host_fail(PCV_E_INVALID, "not an S2 cell id");
  if (s2::level_of(cell) == 0u) return pcv_host_fail(PCV_E_INVALID, "the geometry of a level-0 cell (a face) is not provided");
  s2::CellGeom g;
  s2::cell_geom(cell, &g);
  *intersects = s2::rect_intersects_cell(rect, g) ? 1 : 0;
  return PCV_OK;
}

extern "C" int pcv_s2_union_normalize_host(uint64_t* cells, uint32_t* num_cells) {
  if (!num_cells || (*num_cells && !cells)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  for (uint32_t k = 0; k < *num_cells; ++k)
    if (!s2::valid_cell(cells[k])) return pcv_host_fail(PCV_E_INVALID, "cell " + std::to_string(k) + " is no S2 cell id");
  std::sort(cells, cells + *num_cells);
  *num_cells = s2::normalize_sorted(cells, *num_cells);
  return PCV_OK;
}

extern "C" int pcv_s2_union_intersects_host(const uint64_t* cells, uint32_t num_cells, uint64_t n, const uint64_t* ids, uint8_t* intersects) {
  std::string why;
  if (pcv_s2_check_union(cells, num_cells, &why)) return pcv_host_fail(PCV_E_INVALID, why);
  if (n && (!ids || !intersects)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n; ++i) {
    if (!s2::valid_cell(ids[i])) return pcv_host_fail(PCV_E_INVALID, "id " + std::to_string(i) + " is no S2 cell id");
    intersects[i] = s2::union_intersects(cells, num_cells, ids[i]) ? 1 : 0;
  }
  return PCV_OK;
}

extern "C" int pcv_s2_cells_in_location_host(uint64_t num_cells, const uint64_t* cell_ids, uint32_t num_shapes, const int32_t* kinds,
                                             const int32_t* valid, const double* corners, uint32_t num_unions,
                                             const uint32_t* union_first, const uint64_t* union_cells, uint32_t capacity,
                                             uint32_t* counts, uint32_t* cells) {
  std::string why;
  if (num_cells && !cell_ids) return pcv_host_fail(PCV_E_INVALID, "cell_ids is null");
  if (num_shapes && (!kinds || !valid || !corners)) return pcv_host_fail(PCV_E_INVALID, "kinds, valid and corners are needed for shapes");
  bool geometric = false;
  for (uint32_t f = 0; f < num_shapes; ++f) geometric = geometric || kinds[f] != PCV_SHAPE_ALL;
  if (check_cloud_cells(num_cells, cell_ids, geometric, &why) || check_unions(num_unions, union_first, union_cells, &why))
    return pcv_host_fail(PCV_E_INVALID, why);
  const uint64_t locations = (uint64_t)num_shapes + num_unions;
  if (locations == 0) return PCV_OK;
  if (!counts || (capacity && !cells)) return pcv_host_fail(PCV_E_INVALID, "counts / cells is null");
  std::vector<s2::CellGeom> geom(geometric ? num_cells : 0);
  for (uint64_t c = 0; c < geom.size(); ++c) s2::cell_geom(cell_ids[c], &geom[c]);
  for (uint64_t l = 0; l < locations; ++l) {
    S2Loc loc;
    if (l < num_shapes) {
      location_of_shape(kinds[l], valid[l], corners + 24 * l, &loc);
    } else {
      loc.mode = kLocUnion;
      loc.union_first = union_first[l - num_shapes];
      loc.union_count = union_first[l - num_shapes + 1] - loc.union_first;
    }
    uint32_t count = 0;
    for (uint64_t c = 0; c < num_cells && loc.mode != kLocNone; ++c) {
      bool hit;
      if (loc.mode == kLocAll) hit = true;
      else if (loc.mode == kLocUnion) hit = s2::union_intersects(union_cells + loc.union_first, loc.union_count, cell_ids[c]);
      else hit = s2::rect_intersects_cell(loc.rect, geom[c]);
      if (hit) {
        if (count < capacity) cells[l * capacity + count] = (uint32_t)c;
        ++count;
      }
    }
    counts[l] = count;
  }
  return PCV_OK;
}

// ---- device entry point -------------------------------------------------------------------------------------------------
extern "C" int pcv_s2_cells_in_location(pcv_s2_cloud* c, const pcv_shapes* shapes, uint32_t num_unions, const uint32_t* union_first,
                                        const uint64_t* union_cells, uint32_t capacity, uint32_t* counts, uint32_t* cells) {
  if (!c) return PCV_E_INVALID;
  pcv_ctx* ctx = c->ctx;
  if (!ctx) return c->fail(PCV_E_INVALID, "a cloud opened without a context has no device: pcv_s2_cells_in_location_host takes its cell ids");
  if (shapes && shapes->ctx != ctx) return ctx->fail(PCV_E_INVALID, "the shapes belong to another context");
  const uint32_t num_shapes = shapes ? shapes->count : 0;
  const uint32_t n = (uint32_t)c->ids.size();
  bool geometric = false;  // (a cell union in the table asks for ids only, like the call's own unions)
  for (uint32_t f = 0; f < num_shapes; ++f)
    if (shapes->polygon_frame_of(f) == 0)
      return ctx->fail(PCV_E_INVALID, "shape " + std::to_string(f) + ": a polygon in the xy frame has no meaning over an ECEF cell cloud");
  for (uint32_t f = 0; f < num_shapes; ++f)
    geometric = geometric || (shapes->kinds[f] != PCV_SHAPE_ALL && shapes->kinds[f] != PCV_SHAPE_S2_CELL_UNION);
  std::string why;
  if (check_cloud_cells(c->ids.size(), c->ids.data(), geometric, &why) || check_unions(num_unions, union_first, union_cells, &why))
    return ctx->fail(PCV_E_INVALID, why);
  const uint64_t locations = (uint64_t)num_shapes + num_unions;
  if (locations == 0) return PCV_OK;
  if (locations > 0x7fffffffull) return ctx->fail(PCV_E_INVALID, "too many locations for one call");
  if (!counts || (capacity && !cells)) return ctx->fail(PCV_E_INVALID, "counts / cells is null");
  if (n == 0) {
    std::memset(counts, 0, (size_t)locations * 4);
    return PCV_OK;
  }
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int rc;
  if ((rc = prepare_cloud(c, geometric))) return rc;
  PcvScratch sc(ctx);
  S2Loc* d_locs;
  uint32_t *d_counts, *d_out;
  uint64_t* d_union;
  const uint32_t union_total = num_unions ? union_first[num_unions] : 0;
  // the table's own unions (pcv_shapes_create_ex) sit behind the call's in d_union
  const size_t table_total = shapes ? shapes->union_cells.size() : 0;
  if ((uint64_t)union_total + table_total > 0xffffffffull) return ctx->fail(PCV_E_INVALID, "too many union cells for one call");
  if ((rc = sc.get(&d_locs, (size_t)locations)) || (rc = sc.get(&d_counts, (size_t)locations)) ||
      (rc = sc.get(&d_out, (size_t)locations * capacity + 1)) || (rc = sc.get(&d_union, (size_t)union_total + table_total + 1)))
    return rc;
  if (num_shapes) {
    PcvProf prof(ctx, PCV_K_S2_LOCATIONS);
    hipLaunchKernelGGL(s2_location_kernel, dim3((num_shapes + 63u) / 64u), dim3(64), 0, st, shapes->dev, num_shapes, d_locs);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  // a cell union in the table is the union location it is, at its slot: over what s2_location_kernel wrote for it (none)
  std::vector<S2Loc> t_locs(shapes ? shapes->union_shapes.size() : 0);
  for (size_t k = 0; k < t_locs.size(); ++k) {
    const uint32_t u = shapes->union_of[k];
    S2Loc& loc = t_locs[k];
    loc.mode = kLocUnion;
    loc.union_first = union_total + shapes->union_first[u];
    loc.union_count = shapes->union_first[u + 1] - shapes->union_first[u];
    loc.pad = 0;
    s2::rect_set_empty(loc.rect);
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_locs + shapes->union_shapes[k], &loc, sizeof(S2Loc), hipMemcpyHostToDevice, st));
  }
  if (!t_locs.empty() && table_total)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_union + union_total, shapes->union_cells.data(), table_total * 8, hipMemcpyHostToDevice, st));
  std::vector<S2Loc> h_locs(num_unions);
  if (num_unions) {
    for (uint32_t u = 0; u < num_unions; ++u) {
      S2Loc& loc = h_locs[u];
      loc.mode = kLocUnion;
      loc.union_first = union_first[u];
      loc.union_count = union_first[u + 1] - union_first[u];
      loc.pad = 0;
      s2::rect_set_empty(loc.rect);
    }
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_locs + num_shapes, h_locs.data(), sizeof(S2Loc) * num_unions, hipMemcpyHostToDevice, st));
    if (union_total) PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_union, union_cells, (size_t)union_total * 8, hipMemcpyHostToDevice, st));
  }
  {
    PcvProf prof(ctx, PCV_K_S2_PAIRS);
    hipLaunchKernelGGL(s2_pair_kernel, dim3((uint32_t)locations), dim3(64), 0, st, d_locs, c->d_ids, c->d_table, n, d_union, capacity,
                       d_counts, d_out);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(counts, d_counts, (size_t)locations * 4, hipMemcpyDeviceToHost, st));
  if (capacity) PCV_HIP_CHECK(ctx, hipMemcpyAsync(cells, d_out, (size_t)locations * capacity * 4, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));  // (also: h_locs and the caller's unions may be pageable memory)
  ctx->prof_resolve();
  return PCV_OK;
}
