// pcv_union.hip — cell unions as query locations over the octree for gfx950 (PointLocation::S2Cells; reference
// src/geometry/s2_cell_union.rs, src/octree/mod.rs:309-331, src/octree/octree_iterator.rs).
//
//   rects   union_node_rects_kernel: once per octree, one lane per node — the 8 corners of the node's bounding cube
//           (find_bounding_cube), their leaf cells, normalized, the rect bound: 32 B per node, kept with the tree's query
//           tables. The rect depends on the tree only, never on the union.
//   cells   the CellGeom planes of every union cell of a shape table, once per table (pcv_union_prepare_shapes; the host runs
//           the chain of pcv_s2_region_dev.h, whose results are the device's bit for bit)
//   walk    union_walk_kernel: one wave per location; the lanes are entries of the breadth-first queue, taken 64 at a time.
//           Each lane tests its node's rect against the union's cells (bound rejection, then the precise steps); a ballot and
//           prefix popcounts append the hits, a wave scan their children, in queue order — so the list is NodeIdsIterator's,
//           and, nodes being stored in (level, index) order, it ascends by node index. The queue lives in global scratch.
//
// The per-point test (leaf id, binary search in the union's cells) is pcv_query.hip's: query_flags_union_kernel and
// cull_points_union_kernel. The chain is pcv_s2_dev.h / pcv_s2_region_dev.h: one correctly rounded f64 operation per step, no
// libm, no contraction, so pcv_s2_union_intersects_cubes_host below decides what the device decides.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "pcv_internal.h"
#include "pcv_query_dev.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_region_dev.h"

namespace {

// the rect of cells_intersecting_polyhedron for a node cube: Cube::to_aabb = Aabb::new(min, min + edge) (inf / sup), its corners
// in aabb.rs:114-125 order (corners_rect sorts their cells: the order does not matter), their leaf cells, normalized, the rect
// bound. Eight leaves that normalize to a face have no rect (Cell::rect_bound of a face is not provided): the empty rect, which
// intersects nothing.
__host__ __device__ inline void cube_rect(double mnx, double mny, double mnz, double edge, uint64_t* ids /* 8 working slots */, double* rect) {
  const double ax = mnx + edge, ay = mny + edge, az = mnz + edge;
  const double lx = fmin(mnx, ax), hx = fmax(mnx, ax), ly = fmin(mny, ay), hy = fmax(mny, ay), lz = fmin(mnz, az), hz = fmax(mnz, az);
  const double corners[24] = {lx, ly, lz, hx, ly, lz, lx, hy, lz, hx, hy, lz, lx, ly, hz, hx, ly, hz, lx, hy, hz, hx, hy, hz};
  if (!s2::corners_rect_in(corners, ids, rect)) s2::rect_set_empty(rect);
}

// Rect::intersects_cell of `r` against any of `count` cells whose geometry is columns first .. first + count of the planes
__host__ __device__ inline bool rect_hits_union(const double* r, const uint64_t* cells, uint32_t count, const double* geom, uint32_t stride,
                                                uint32_t first) {
  if (s2::rect_empty(r)) return false;
  for (uint32_t k = 0; k < count; ++k) {
    const size_t c = (size_t)first + k;
    const double bound[4] = {geom[c], geom[(size_t)stride + c], geom[2 * (size_t)stride + c], geom[3 * (size_t)stride + c]};
    if (!s2::rect_intersects(r, bound)) continue;
    s2::CellGeom g;
    s2::load_geom(geom, stride, c, cells[k], &g);
    if (s2::rect_intersects_cell_after_bound(r, g)) return true;
  }
  return false;
}

__global__ __launch_bounds__(256) void union_node_rects_kernel(const double* __restrict__ cubes /* m x 4, find_bounding_cube */, uint32_t m,
                                                                double* __restrict__ rects /* m x 4 */) {
  __shared__ uint64_t ids[256][8];  // the corners' cells of each lane: sorted and normalized in place
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= m) return;
  const double4 c = *reinterpret_cast<const double4*>(cubes + 4 * (size_t)i);
  double r[4];
  cube_rect(c.x, c.y, c.z, c.w, ids[threadIdx.x], r);
  *reinterpret_cast<double4*>(rects + 4 * (size_t)i) = make_double4(r[0], r[1], r[2], r[3]);
}

// One wave (= one workgroup) per location which[first + blockIdx.x]. The queue holds every node whose parent intersects, in
// breadth-first order; each node enters it at most once, so m slots suffice.
__global__ __launch_bounds__(64) void union_walk_kernel(const PcvShapeDev* __restrict__ shapes, const uint32_t* __restrict__ which,
                                                         uint32_t first, uint32_t m, const double* __restrict__ rects,
                                                         const uint32_t* __restrict__ first_child, const uint8_t* __restrict__ child_mask,
                                                         uint32_t* queues, uint32_t capacity, uint32_t* __restrict__ counts,
                                                         uint32_t* __restrict__ out, const uint64_t* __restrict__ rows,
                                                         uint32_t single /* set: the one location's count and list at slot 0 */) {
  const uint32_t lane = threadIdx.x;
  const uint32_t f = which[first + blockIdx.x];
  const PcvShapeDev* s = shapes + f;
  const uint64_t* cells = s->cell_union.cells;
  const double* geom = s->cell_union.geom;
  const uint32_t ncells = s->cell_union.count, col = s->cell_union.first, stride = s->cell_union.stride;
  uint32_t* q = queues + (size_t)blockIdx.x * m;
  const uint32_t slot = single ? 0u : f;
  uint32_t* o = out + (rows ? rows[f] : (uint64_t)slot * capacity);
  if (rows) capacity = (uint32_t)(rows[f + 1] - rows[f]);
  uint32_t head = 0, tail = 0, nout = 0;  // wave-uniform
  if (m > 0 && ncells > 0) {
    if (lane == 0) q[0] = 0;
    tail = 1;
  }
  __syncthreads();  // (one wave: the queue's stores have landed before its loads)
  while (head < tail) {
    const uint32_t n = min(64u, tail - head);
    uint32_t node = 0;
    bool hit = false;
    if (lane < n) {
      node = q[head + lane];
      const double4 r4 = *reinterpret_cast<const double4*>(rects + 4 * (size_t)node);
      const double r[4] = {r4.x, r4.y, r4.z, r4.w};
      hit = rect_hits_union(r, cells, ncells, geom, stride, col);
    }
    const unsigned long long hits = __ballot(hit);
    const uint32_t at = nout + (uint32_t)__popcll(hits & ((1ull << lane) - 1ull));
    if (hit && at < capacity) o[at] = node;  // (entries past `capacity` are dropped, the count is not)
    // the children of the hits, behind the queue's tail in lane order: an exclusive wave scan of the child counts
    const uint32_t mask = hit ? (uint32_t)child_mask[node] : 0u;
    const uint32_t nch = (uint32_t)__popc(mask);
    uint32_t incl = nch;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= (uint32_t)d) incl += t;
    }
    const uint32_t total = (uint32_t)__shfl((int)incl, 63, 64);
    if (nch) {
      uint32_t w = tail + incl - nch, child = first_child[node];
      for (uint32_t k = 0; k < nch; ++k) q[w++] = child++;
    }
    nout += (uint32_t)__popcll(hits);
    head += n;
    tail += total;
    __syncthreads();
  }
  if (lane == 0) counts[slot] = nout;
}

int ensure_node_rects(pcv_ctx* ctx, PcvOctreeQuery* q) {
  if (q->node_rects || q->m == 0) return PCV_OK;
  void* p;
  int rc;
  if ((rc = ctx->dev_alloc(&p, 32 * (size_t)q->m))) return rc;
  {
    PcvProf prof(ctx, PCV_K_UNION_NODE_RECTS);
    hipLaunchKernelGGL(union_node_rects_kernel, dim3((q->m + 255u) / 256u), dim3(256), 0, ctx->stream, q->fb_cubes, q->m, (double*)p);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    ctx->dev_free(p);
    return ctx->fail(PCV_E_HIP, hipGetErrorString(e));
  }
  q->node_rects = (double*)p;
  return PCV_OK;
}

void launch_walk(pcv_ctx* ctx, const pcv_shapes* shapes, const uint32_t* which, uint32_t first, uint32_t nb, const PcvOctreeQuery* q,
                 uint32_t* queues, uint32_t capacity, uint32_t* counts, uint32_t* out, const uint64_t* rows, bool single) {
  hipLaunchKernelGGL(union_walk_kernel, dim3(nb), dim3(64), 0, ctx->stream, shapes->dev, which, first, q->m, q->node_rects, q->first_child,
                     q->child_mask, queues, capacity, counts, out, rows, single ? 1u : 0u);
}

}  // namespace

int pcv_refuse_unions(pcv_ctx* ctx, const pcv_shapes* shapes, const char* what) {
  if (shapes->union_shapes.empty()) return PCV_OK;
  return ctx->fail(PCV_E_INVALID, std::string(what) + ": shape " + std::to_string(shapes->union_shapes[0]) +
                                      " is a cell union, which has no Relation and no clip matrix");
}

int pcv_union_prepare_shapes(pcv_ctx* ctx, pcv_shapes* r, PcvShapeDev* h) {
  const size_t total = r->union_cells.size(), ns = r->union_shapes.size();
  if (ns == 0) return PCV_OK;
  // one block: cells (8 B each), geometry planes (kCellPlanes x total doubles), the union shapes' indices
  const size_t at_geom = 8 * total, at_which = at_geom + 8 * (size_t)s2::kCellPlanes * total, bytes = at_which + 4 * ns;
  std::vector<uint64_t> up((bytes + 7) / 8, 0);
  if (total) std::memcpy(up.data(), r->union_cells.data(), 8 * total);
  double* planes = reinterpret_cast<double*>(up.data()) + total;
  for (size_t c = 0; c < total; ++c) {
    s2::CellGeom g;
    s2::cell_geom(r->union_cells[c], &g);
    s2::store_geom(g, planes, total, c);
  }
  std::memcpy(reinterpret_cast<uint8_t*>(up.data()) + at_which, r->union_shapes.data(), 4 * ns);
  int rc;
  if ((rc = ctx->dev_alloc(&r->d_union, 8 * up.size()))) return rc;
  uint8_t* base = (uint8_t*)r->d_union;
  r->d_union_shapes = (const uint32_t*)(base + at_which);
  for (size_t k = 0; k < ns; ++k) {
    PcvShapeDev& d = h[r->union_shapes[k]];
    const uint32_t u = r->union_of[k];
    d.cell_union.cells = (const uint64_t*)base + r->union_first[u];
    d.cell_union.geom = (const double*)(base + at_geom);
    d.cell_union.count = r->union_first[u + 1] - r->union_first[u];
    d.cell_union.first = r->union_first[u];
    d.cell_union.stride = (uint32_t)total;
    d.cell_union.pad = 0;
  }
  hipError_t e = hipMemcpyAsync(r->d_union, up.data(), 8 * up.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `up` must outlive the copy
  if (e != hipSuccess) return ctx->fail(PCV_E_HIP, hipGetErrorString(e));
  return PCV_OK;
}

int pcv_launch_union_lists(pcv_ctx* ctx, int label, const pcv_shapes* shapes, const pcv_octree* tree, uint32_t capacity, uint32_t* counts,
                           uint32_t* out, uint32_t* queues, uint32_t batch, const uint64_t* rows) {
  const uint32_t nu = (uint32_t)shapes->union_shapes.size();
  if (nu == 0) return PCV_OK;
  PcvOctreeQuery* q = tree->query;
  int rc;
  if ((rc = ensure_node_rects(ctx, q))) return rc;
  for (uint32_t first = 0; first < nu; first += batch) {
    PcvProf prof(ctx, label);
    launch_walk(ctx, shapes, shapes->d_union_shapes, first, std::min(batch, nu - first), q, queues, capacity, counts, out, rows, false);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

int pcv_union_node_list(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_octree* tree, std::vector<uint32_t>* nodes) {
  PcvOctreeQuery* q = tree->query;
  const uint32_t m = q->m;
  nodes->clear();
  if (m == 0) return PCV_OK;
  const auto it = std::lower_bound(shapes->union_shapes.begin(), shapes->union_shapes.end(), shape_index);
  if (it == shapes->union_shapes.end() || *it != shape_index) return ctx->fail(PCV_E_INVALID, "not a cell union");
  const uint32_t k = (uint32_t)(it - shapes->union_shapes.begin());
  int rc;
  if ((rc = ensure_node_rects(ctx, q))) return rc;
  PcvScratch sc(ctx);
  uint32_t *d_counts, *d_out, *d_queue;
  if ((rc = sc.get(&d_counts, 1)) || (rc = sc.get(&d_out, m)) || (rc = sc.get(&d_queue, m))) return rc;
  {
    PcvProf prof(ctx, PCV_K_NODES_IN_LOCATION);
    launch_walk(ctx, shapes, shapes->d_union_shapes, k, 1, q, d_queue, m, d_counts, d_out, nullptr, true);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  nodes->resize(m);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_counts, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(nodes->data(), d_out, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  nodes->resize(*reinterpret_cast<const uint32_t*>(ctx->mailbox));
  return PCV_OK;
}

// ---- host twin (no context) ---------------------------------------------------------------------------------------------
extern "C" int pcv_s2_union_intersects_cubes_host(const uint64_t* cells, uint32_t num_cells, uint64_t n, const double* cubes,
                                                  uint8_t* intersects) {
  std::string why;
  const uint32_t first[2] = {0, num_cells};
  if (pcv_s2_check_unions(1, first, cells, &why)) return pcv_host_fail(PCV_E_INVALID, why.substr(why.rfind("union 0: ", 0) == 0 ? 9 : 0));
  for (uint32_t k = 0; k < num_cells; ++k)
    if (s2::level_of(cells[k]) == 0u) return pcv_host_fail(PCV_E_INVALID, "a union with a level-0 cell has no geometry");
  if (n && (!cubes || !intersects)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  std::vector<double> planes((size_t)s2::kCellPlanes * num_cells);
  for (uint32_t k = 0; k < num_cells; ++k) {
    s2::CellGeom g;
    s2::cell_geom(cells[k], &g);
    s2::store_geom(g, planes.data(), num_cells, k);
  }
  for (uint64_t i = 0; i < n; ++i) {
    double r[4];
    uint64_t ids[8];
    cube_rect(cubes[4 * i], cubes[4 * i + 1], cubes[4 * i + 2], cubes[4 * i + 3], ids, r);
    intersects[i] = rect_hits_union(r, cells, num_cells, planes.data(), num_cells, 0) ? 1 : 0;
  }
  return PCV_OK;
}
