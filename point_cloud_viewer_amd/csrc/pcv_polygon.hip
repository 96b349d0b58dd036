// pcv_polygon.hip — polygons as query locations for gfx950 (PCV_SHAPE_POLYGON): rings of (x, y) vertices under the
// even-odd rule, in the cloud's own xy (a prism polygon x [z_min, z_max]) or in normalized web-mercator coordinates over an ECEF
// cloud.
//
//   tables  once per shape table (pcv_polygon_prepare_shapes, on the host): per polygon the point rule's edge table and the raw
//           edges of the node rule (pcv_polygon_dev.h), one block beside the table
//   walk    polygon_walk_kernel, xy frame: one wave per location, breadth first, one node at a time. The lanes are the polygon's
//           edges, 64 per round: a ballot says whether an edge hits the node's square, a popcount parity whether its corner is
//           inside. The list is in queue order, so it ascends by node index as NodeIdsIterator's does. The queue lives in global
//           scratch, as union_walk_kernel's.
//   wm      a web-mercator polygon has no walk: to every node and cell traversal it is the web-mercator rectangle over its
//           vertices (device kind, corners, axes), prepared here and run by the existing code.
//
// The per-point test is pcv_query.hip's (query_flags_polygon_kernel, cull_points_polygon_kernel) and pcv_s2_points.hip's.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "pcv_internal.h"
#include "pcv_polygon_dev.h"
#include "pcv_query_dev.h"
#include "pcv_wmr_dev.h"

namespace {

// the point rule's table and the raw edges of rings [r0, r1): 4 doubles per entry each
void build_tables(const uint32_t* ring_first, const double* vertices, uint32_t r0, uint32_t r1, std::vector<double>* edges,
                  std::vector<double>* segs) {
  for (uint32_t r = r0; r < r1; ++r) {
    const uint32_t v0 = ring_first[r], nv = ring_first[r + 1] - v0;
    for (uint32_t k = 0; k < nv; ++k) {
      const double* a = vertices + 2 * (size_t)(v0 + k);
      const double* b = vertices + 2 * (size_t)(v0 + (k + 1 == nv ? 0 : k + 1));
      segs->insert(segs->end(), {a[0], a[1], b[0], b[1]});
      if (a[1] == b[1]) continue;  // horizontal: not in the point rule
      const bool up = a[1] < b[1];
      const double lx = up ? a[0] : b[0], ly = up ? a[1] : b[1], ux = up ? b[0] : a[0], uy = up ? b[1] : a[1];
      edges->insert(edges->end(), {lx, ly, uy, (ux - lx) / (uy - ly)});
    }
  }
}

bool finite_f64(double v) { return std::fabs(v) <= 1.7976931348623157e308; }

// one polygon's rings: the checks that do not depend on the frame
bool check_rings(const std::string& who, uint32_t num_rings, const uint32_t* ring_first, const double* vertices, std::string* why) {
  if (num_rings == 0) return *why = who + "has no ring", false;
  for (uint32_t r = 0; r < num_rings; ++r) {
    if (ring_first[r + 1] < ring_first[r]) return *why = who + "ring offsets descend", false;
    if (ring_first[r + 1] - ring_first[r] < 3) return *why = who + "ring " + std::to_string(r) + " has fewer than 3 vertices", false;
  }
  const uint32_t nv = ring_first[num_rings] - ring_first[0];
  if (nv > poly::kMaxVertices) return *why = who + "has more than 65535 vertices", false;
  for (uint32_t v = ring_first[0]; v < ring_first[num_rings]; ++v)
    if (!finite_f64(vertices[2 * (size_t)v]) || !finite_f64(vertices[2 * (size_t)v + 1]))
      return *why = who + "vertex " + std::to_string(v - ring_first[0]) + " is not finite", false;
  return true;
}

// what a shape adds to its polygon's checks: the frame and what the web-mercator frame asks of the vertices and the z range
bool check_frame(const std::string& who, double frame, double z_min, double z_max, uint32_t num_rings, const uint32_t* ring_first,
                 const double* vertices, std::string* why) {
  if (!(frame == 0.0 || frame == 1.0)) return *why = who + "the frame is 0 (xy) or 1 (web-mercator)", false;
  if (frame == 0.0) return true;
  if (!(z_min == -INFINITY && z_max == INFINITY))
    return *why = who + "a web-mercator polygon has no height range: z_min and z_max are -inf and +inf", false;
  for (uint32_t v = ring_first[0]; v < ring_first[num_rings]; ++v)
    for (int a = 0; a < 2; ++a)
      if (!(vertices[2 * (size_t)v + a] >= 0.0 && vertices[2 * (size_t)v + a] < 1.0))
        return *why = who + "vertex " + std::to_string(v - ring_first[0]) + " is outside [0, 1): web-mercator vertices are normalized", false;
  return true;
}

// One wave (= one workgroup) per location which[first + blockIdx.x]; the queue holds every node whose parent was listed, in
// breadth-first order. Each node enters it at most once, so m slots suffice.
__global__ __launch_bounds__(64) void polygon_walk_kernel(const PcvShapeDev* __restrict__ shapes, const uint32_t* __restrict__ which,
                                                           uint32_t first, uint32_t m, const double* __restrict__ cubes /* m x 4 */,
                                                           const uint32_t* __restrict__ first_child, const uint8_t* __restrict__ child_mask,
                                                           uint32_t* queues, uint32_t capacity, uint32_t* __restrict__ counts,
                                                           uint32_t* __restrict__ out, const uint64_t* __restrict__ rows,
                                                           uint32_t single /* set: the one location's count and list at slot 0 */) {
  const uint32_t lane = threadIdx.x;
  const uint32_t f = which[first + blockIdx.x];
  const PcvShapeDev* s = shapes + f;
  const double4* edges = reinterpret_cast<const double4*>(s->polygon.edges);
  const double4* segs = reinterpret_cast<const double4*>(s->polygon.segs);
  const uint32_t nedges = s->polygon.nedges, nsegs = s->polygon.nsegs;
  const double z_min = s->polygon.z_min, z_max = s->polygon.z_max;
  uint32_t* q = queues + (size_t)blockIdx.x * m;
  const uint32_t slot = single ? 0u : f;
  uint32_t* o = out + (rows ? rows[f] : (uint64_t)slot * capacity);
  if (rows) capacity = (uint32_t)(rows[f + 1] - rows[f]);
  uint32_t head = 0, tail = 0, nout = 0;  // wave-uniform
  if (m > 0) {
    if (lane == 0) q[0] = 0;
    tail = 1;
  }
  __syncthreads();  // (one wave: the queue's stores have landed before its loads)
  while (head < tail) {
    const uint32_t node = q[head];  // wave-uniform
    const double4 c = *reinterpret_cast<const double4*>(cubes + 4 * (size_t)node);
    const double hx = c.x + c.w, hy = c.y + c.w, hz = c.z + c.w;
    bool hit = false;  // wave-uniform
    if (z_min <= hz && z_max >= c.z) {
      for (uint32_t k0 = 0; k0 < nsegs && !hit; k0 += 64) {  // an edge hits the square
        bool h = false;
        if (k0 + lane < nsegs) {
          const double4 e = segs[k0 + lane];
          h = poly::edge_hits_square(e.x, e.y, e.z, e.w, c.x, c.y, hx, hy);
        }
        hit = __ballot(h) != 0ull;
      }
      if (!hit) {  // or the square's corner is inside
        uint32_t crossings = 0;
        for (uint32_t k0 = 0; k0 < nedges; k0 += 64) {
          bool x = false;
          if (k0 + lane < nedges) {
            const double4 e = edges[k0 + lane];
            x = poly::crosses(e.x, e.y, e.z, e.w, c.x, c.y);
          }
          crossings += (uint32_t)__popcll(__ballot(x));
        }
        hit = (crossings & 1u) != 0;
      }
    }
    if (hit) {
      if (lane == 0 && nout < capacity) o[nout] = node;  // (entries past `capacity` are dropped, the count is not)
      const uint32_t nch = (uint32_t)__popc((uint32_t)child_mask[node]);
      if (lane < nch) q[tail + lane] = first_child[node] + lane;
      tail += nch;
      ++nout;
    }
    ++head;
    __syncthreads();
  }
  if (lane == 0) counts[slot] = nout;
}

void launch_walk(pcv_ctx* ctx, const pcv_shapes* shapes, const uint32_t* which, uint32_t first, uint32_t nb, const PcvOctreeQuery* q,
                 uint32_t* queues, uint32_t capacity, uint32_t* counts, uint32_t* out, const uint64_t* rows, bool single) {
  hipLaunchKernelGGL(polygon_walk_kernel, dim3(nb), dim3(64), 0, ctx->stream, shapes->dev, which, first, q->m, q->fb_cubes, q->first_child,
                     q->child_mask, queues, capacity, counts, out, rows, single ? 1u : 0u);
}

// a polygon given as the host twins take it: its checks, then its tables
int host_polygon(uint32_t num_rings, const uint32_t* ring_first, const double* vertices, int32_t frame, double z_min, double z_max,
                 std::vector<double>* edges, std::vector<double>* segs) {
  if (!ring_first || !vertices) return pcv_host_fail(PCV_E_INVALID, "null argument");
  std::string why;
  if (ring_first[0] != 0) return pcv_host_fail(PCV_E_INVALID, "ring_first[0] must be 0");
  if (!check_rings("the polygon ", num_rings, ring_first, vertices, &why) ||
      !check_frame("", (double)frame, z_min, z_max, num_rings, ring_first, vertices, &why))
    return pcv_host_fail(PCV_E_INVALID, why);
  if (edges) build_tables(ring_first, vertices, 0, num_rings, edges, segs);
  return PCV_OK;
}

}  // namespace

int pcv_refuse_polygons(pcv_ctx* ctx, const pcv_shapes* shapes, const char* what) {
  if (shapes->polygon_shapes.empty()) return PCV_OK;
  return ctx->fail(PCV_E_INVALID, std::string(what) + ": shape " + std::to_string(shapes->polygon_shapes[0]) +
                                      " is a polygon, which has no Relation and no clip matrix");
}

int pcv_polygon_check_table(uint32_t num_polygons, const uint32_t* polygon_first, const uint32_t* ring_first, const double* vertices,
                            std::string* why) {
  if (num_polygons == 0) return PCV_OK;
  if (!polygon_first || !ring_first || !vertices) return *why = "polygons: null argument", PCV_E_INVALID;
  if (polygon_first[0] != 0 || ring_first[0] != 0) return *why = "polygons: polygon_first[0] and ring_first[0] must be 0", PCV_E_INVALID;
  for (uint32_t p = 0; p < num_polygons; ++p) {
    if (polygon_first[p + 1] < polygon_first[p]) return *why = "polygons: polygon offsets descend", PCV_E_INVALID;
    if (!check_rings("polygon " + std::to_string(p) + ": ", polygon_first[p + 1] - polygon_first[p], ring_first + polygon_first[p], vertices, why))
      return PCV_E_INVALID;
  }
  return PCV_OK;
}

int pcv_polygon_check_shape(double frame, double z_min, double z_max, uint32_t num_rings, const uint32_t* ring_first, const double* vertices,
                            std::string* why) {
  return check_frame("", frame, z_min, z_max, num_rings, ring_first, vertices, why) ? PCV_OK : PCV_E_INVALID;
}

int pcv_polygon_prepare_shapes(pcv_ctx* ctx, pcv_shapes* r, PcvShapeDev* h) {
  const size_t ns = r->polygon_shapes.size();
  if (ns == 0) return PCV_OK;
  const uint32_t np = (uint32_t)r->polygon_first.size() - 1;
  // the tables of every polygon that a shape names, back to back; a polygon's tables do not depend on the shape
  std::vector<double> edges, segs;
  std::vector<size_t> edge_at(np + 1, 0), seg_at(np + 1, 0);
  std::vector<uint8_t> named(np, 0);
  for (size_t k = 0; k < ns; ++k) named[r->polygon_of[k]] = 1;
  for (uint32_t p = 0; p < np; ++p) {
    if (named[p]) build_tables(r->ring_first.data(), r->vertices.data(), r->polygon_first[p], r->polygon_first[p + 1], &edges, &segs);
    edge_at[p + 1] = edges.size() / 4;
    seg_at[p + 1] = segs.size() / 4;
  }
  for (size_t k = 0; k < ns; ++k)
    if (r->polygon_frame[k] == 0) r->xy_polygons.push_back((uint32_t)k);
  // one block: edge tables, raw edges, the xy-frame polygon shapes' indices
  const size_t at_segs = 8 * edges.size(), at_which = at_segs + 8 * segs.size(), bytes = at_which + 4 * r->xy_polygons.size();
  std::vector<uint64_t> up((bytes + 7) / 8 + 1, 0);
  if (!edges.empty()) std::memcpy(up.data(), edges.data(), 8 * edges.size());
  if (!segs.empty()) std::memcpy(reinterpret_cast<uint8_t*>(up.data()) + at_segs, segs.data(), 8 * segs.size());
  uint32_t* which = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(up.data()) + at_which);
  for (size_t j = 0; j < r->xy_polygons.size(); ++j) which[j] = r->polygon_shapes[r->xy_polygons[j]];
  int rc;
  if ((rc = ctx->dev_alloc(&r->d_polygon, 8 * up.size()))) return rc;
  uint8_t* base = (uint8_t*)r->d_polygon;
  r->d_xy_polygon_shapes = (const uint32_t*)(base + at_which);
  for (size_t k = 0; k < ns; ++k) {
    PcvShapeDev& d = h[r->polygon_shapes[k]];
    const uint32_t p = r->polygon_of[k];
    d.polygon.edges = (const double*)base + 4 * edge_at[p];
    d.polygon.segs = (const double*)(base + at_segs) + 4 * seg_at[p];
    d.polygon.nedges = (uint32_t)(edge_at[p + 1] - edge_at[p]);
    d.polygon.nsegs = (uint32_t)(seg_at[p + 1] - seg_at[p]);
    d.polygon.frame = r->polygon_frame[k];
    d.point_kind = PCV_SHAPE_POLYGON;
    if (r->polygon_frame[k] == 1) {
      // the rectangle over the vertices: ("web_mercator_rect", (min x, min y), (max x, max y)), prepared as such a shape is
      const uint32_t v0 = r->ring_first[r->polygon_first[p]], v1 = r->ring_first[r->polygon_first[p + 1]];
      double rect[4] = {r->vertices[2 * (size_t)v0], r->vertices[2 * (size_t)v0 + 1], r->vertices[2 * (size_t)v0], r->vertices[2 * (size_t)v0 + 1]};
      for (uint32_t v = v0; v < v1; ++v) {
        rect[0] = std::fmin(rect[0], r->vertices[2 * (size_t)v]);
        rect[1] = std::fmin(rect[1], r->vertices[2 * (size_t)v + 1]);
        rect[2] = std::fmax(rect[2], r->vertices[2 * (size_t)v]);
        rect[3] = std::fmax(rect[3], r->vertices[2 * (size_t)v + 1]);
      }
      d.kind = PCV_SHAPE_WEB_MERCATOR_RECT;
      d.bmin[0] = rect[0];
      d.bmin[1] = rect[1];
      d.bmax[0] = rect[2];
      d.bmax[1] = rect[3];
      if (pcv_wmr_corners(rect, d.corners) != PCV_OK) return ctx->fail(PCV_E_INVALID, "web-mercator polygon: corners");
    }
  }
  hipError_t e = hipMemcpyAsync(r->d_polygon, up.data(), 8 * up.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `up` must outlive the copy
  if (e != hipSuccess) return ctx->fail(PCV_E_HIP, hipGetErrorString(e));
  return PCV_OK;
}

int pcv_launch_polygon_lists(pcv_ctx* ctx, int label, const pcv_shapes* shapes, const pcv_octree* tree, uint32_t capacity, uint32_t* counts,
                             uint32_t* out, uint32_t* queues, uint32_t batch, const uint64_t* rows) {
  const uint32_t nu = (uint32_t)shapes->xy_polygons.size();
  if (nu == 0) return PCV_OK;
  const PcvOctreeQuery* q = tree->query;
  for (uint32_t first = 0; first < nu; first += batch) {
    PcvProf prof(ctx, label);
    launch_walk(ctx, shapes, shapes->d_xy_polygon_shapes, first, std::min(batch, nu - first), q, queues, capacity, counts, out, rows, false);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

int pcv_polygon_node_list(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_octree* tree, std::vector<uint32_t>* nodes) {
  const PcvOctreeQuery* q = tree->query;
  const uint32_t m = q->m;
  nodes->clear();
  if (m == 0) return PCV_OK;
  uint32_t k = 0;
  while (k < shapes->xy_polygons.size() && shapes->polygon_shapes[shapes->xy_polygons[k]] != shape_index) ++k;
  if (k == shapes->xy_polygons.size()) return ctx->fail(PCV_E_INVALID, "not a polygon in the xy frame");
  PcvScratch sc(ctx);
  uint32_t *d_counts, *d_out, *d_queue;
  int rc;
  if ((rc = sc.get(&d_counts, 1)) || (rc = sc.get(&d_out, m)) || (rc = sc.get(&d_queue, m))) return rc;
  {
    PcvProf prof(ctx, PCV_K_NODES_IN_LOCATION);
    launch_walk(ctx, shapes, shapes->d_xy_polygon_shapes, k, 1, q, d_queue, m, d_counts, d_out, nullptr, true);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  nodes->resize(m);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_counts, 4, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(nodes->data(), d_out, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  nodes->resize(*reinterpret_cast<const uint32_t*>(ctx->mailbox));
  return PCV_OK;
}

// ---- host twins (no device, no context) ------------------------------------------------------------------------------------
extern "C" int pcv_polygon_check_host(uint32_t num_rings, const uint32_t* ring_first, const double* vertices, int32_t frame, double z_min,
                                      double z_max) {
  return host_polygon(num_rings, ring_first, vertices, frame, z_min, z_max, nullptr, nullptr);
}

extern "C" int pcv_polygon_contains_host(uint32_t num_rings, const uint32_t* ring_first, const double* vertices, int32_t frame, double z_min,
                                         double z_max, uint64_t n, const double* x, const double* y, const double* z, uint8_t* keep) {
  std::vector<double> edges, segs;
  const int rc = host_polygon(num_rings, ring_first, vertices, frame, z_min, z_max, &edges, &segs);
  if (rc) return rc;
  if (n && (!x || !y || !z || !keep)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  const uint32_t ne = (uint32_t)(edges.size() / 4);
  for (uint64_t i = 0; i < n; ++i) {
    if (frame == 1) {
      double u, v;
      wmr::project(x[i], y[i], z[i], &u, &v);
      keep[i] = poly::inside(edges.data(), ne, u, v) ? 1 : 0;
    } else {
      keep[i] = (poly::inside(edges.data(), ne, x[i], y[i]) && z_min <= z[i] && z[i] <= z_max) ? 1 : 0;
    }
  }
  return PCV_OK;
}

extern "C" int pcv_polygon_intersects_cubes_host(uint32_t num_rings, const uint32_t* ring_first, const double* vertices, double z_min,
                                                 double z_max, uint64_t m, const double* cubes, uint8_t* intersects) {
  std::vector<double> edges, segs;
  const int rc = host_polygon(num_rings, ring_first, vertices, 0, z_min, z_max, &edges, &segs);
  if (rc) return rc;
  if (m && (!cubes || !intersects)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  const uint32_t ne = (uint32_t)(edges.size() / 4), nsg = (uint32_t)(segs.size() / 4);
  for (uint64_t i = 0; i < m; ++i)
    intersects[i] =
        poly::cube_hits(edges.data(), ne, segs.data(), nsg, z_min, z_max, cubes[4 * i], cubes[4 * i + 1], cubes[4 * i + 2], cubes[4 * i + 3]) ? 1 : 0;
  return PCV_OK;
}
