// pcv_query_dev.h — what the query sources (pcv_shapes.hip, pcv_cull.hip, pcv_query.hip) share with each other and with
// their consumers on the device (pcv_xray.hip, pcv_render.hip): the f64 vector helpers, Isometry3 rotation, the per-point
// decode of a node's bytes, the prepared shapes, the tree's query tables on the device, the chunk descriptor and the batch.
// No kernel is shared across translation units: the point query reaches node culling through the two host functions at the
// end.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "pcv_chain_dev.h"
#include "pcv_query_tables.h"

struct V3d {
  double x, y, z;
};
__host__ __device__ __forceinline__ V3d v_sub(V3d a, V3d b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__host__ __device__ __forceinline__ V3d v_add(V3d a, V3d b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__host__ __device__ __forceinline__ double v_dot(V3d a, V3d b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ __forceinline__ V3d v_cross(V3d a, V3d b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__host__ __device__ __forceinline__ V3d v_scale(V3d a, double s) { return {a.x * s, a.y * s, a.z * s}; }

__host__ __device__ __forceinline__ V3d quat_rotate(const double* q, V3d v) {  // UnitQuaternion * Vector3
  V3d qv = {q[0], q[1], q[2]};
  V3d t = v_scale(v_cross(qv, v), 2.0);
  V3d c = v_cross(qv, t);
  return v_add(v_add(v_scale(t, q[3]), c), v);
}

#define M4(m, r, c) (m)[(c) * 4 + (r)]
// nalgebra Matrix4::transform_point
__device__ __forceinline__ V3d m4_transform_point(const double* m, V3d p) {
  double r0 = ((M4(m, 0, 0) * p.x + M4(m, 0, 1) * p.y) + M4(m, 0, 2) * p.z) + M4(m, 0, 3);
  double r1 = ((M4(m, 1, 0) * p.x + M4(m, 1, 1) * p.y) + M4(m, 1, 2) * p.z) + M4(m, 1, 3);
  double r2 = ((M4(m, 2, 0) * p.x + M4(m, 2, 1) * p.y) + M4(m, 2, 2) * p.z) + M4(m, 2, 3);
  double n = ((M4(m, 3, 0) * p.x + M4(m, 3, 1) * p.y) + M4(m, 3, 2) * p.z) + M4(m, 3, 3);
  if (n != 0.0) return {r0 / n, r1 / n, r2 / n};
  return {r0, r1, r2};
}

// K8: keep mask. Positions either raw f64 SoA or a node's encoded bytes.
struct PointsView {
  uint64_t n;
  const double *x, *y, *z;
  const uint8_t* encoded;  // non-null: node bytes, `enc`, cube
  uint32_t enc;
  double cube_min[3];
  double cube_edge;
  const float* attr;       // optional f32 attribute with closed interval
  double lo, hi;
  int has_interval;
};

__device__ __forceinline__ V3d load_point(const PointsView& v, uint64_t i) {
  if (!v.encoded) return {v.x[i], v.y[i], v.z[i]};
  uint64_t c[3];
  switch (v.enc) {
    case PCV_ENC_UINT8: {
      const uint8_t* p = v.encoded + 3 * i;
      c[0] = p[0];
      c[1] = p[1];
      c[2] = p[2];
      break;
    }
    case PCV_ENC_UINT16: {
      const uint16_t* p = reinterpret_cast<const uint16_t*>(v.encoded) + 3 * i;
      c[0] = p[0];
      c[1] = p[1];
      c[2] = p[2];
      break;
    }
    case PCV_ENC_FLOAT32: {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(v.encoded) + 3 * i;
      c[0] = p[0];
      c[1] = p[1];
      c[2] = p[2];
      break;
    }
    default: {
      const uint64_t* p = reinterpret_cast<const uint64_t*>(v.encoded) + 3 * i;
      c[0] = p[0];
      c[1] = p[1];
      c[2] = p[2];
      break;
    }
  }
  return {pcv_decode_coord(v.enc, c[0], v.cube_min[0], v.cube_edge), pcv_decode_coord(v.enc, c[1], v.cube_min[1], v.cube_edge),
          pcv_decode_coord(v.enc, c[2], v.cube_min[2], v.cube_edge)};
}

// ---- prepared shapes (pcv_shapes_create, pcv_shapes.hip) ------------------------------------------------------------
#define PCV_MAX_AXES 26
struct PcvShapeDev {
  int32_t kind;   // PCV_SHAPE_*
  int32_t valid;  // 0: matrix not invertible (Frustum::from_matrix4 -> None)
  int32_t naxes;  // 0 for a web-mercator rectangle: its axes live in its PcvShapeWide
  int32_t point_kind;  // the kind of the per-point test (ChunkDesc::enc): `kind`, but PCV_SHAPE_POLYGON for a web-mercator polygon
  double clip_from_query[16];
  union {
    double query_from_clip[16];
    struct PcvShapeWide* wide;  // web-mercator rectangle (no matrices): its record beside the table
    struct {                    // cell union (no matrices): its cells and their geometry beside the table (pcv_union.hip)
      const uint64_t* cells;    // the union's own cells, ascending
      const double* geom;       // s2::kCellPlanes planes of `stride` doubles, every union's cells back to back
      uint32_t count, first;    // this union's cells are columns first .. first + count of the planes
      uint32_t stride, pad;
    } cell_union;
    struct {                      // polygon (no matrices): its tables beside the table (pcv_polygon.hip). In the web-mercator
      struct PcvShapeWide* wide;  // frame `kind` is PCV_SHAPE_WEB_MERCATOR_RECT and this is the bounding rectangle's record
      const double* edges;        // the point rule's table: 4 doubles per non-horizontal edge (pcv_polygon_dev.h)
      const double* segs;         // every edge a -> b as given, 4 doubles each: the node rule's
      uint32_t nedges, nsegs;
      double z_min, z_max;
      int32_t frame, pad;
    } polygon;
  };
  double iso[7];   // obb_from_query (translation xyz, quaternion ijkw) for contains()
  double half[3];
  double bmin[3], bmax[3];
  double corners[24];
  double axes[PCV_MAX_AXES * 3];
  double amin[PCV_MAX_AXES];  // projection interval of the shape's own corners on each axis
  double amax[PCV_MAX_AXES];
};

// A web-mercator rectangle has 12 edges and 6 face normals: up to 6 + 3 + 36 = 45 axes (sat.rs:111-143). They live beside the
// shape table, one record per such shape, so that PcvShapeDev keeps its layout and stride for the other kinds. The flat
// kernels' WIDE instances read them (sat_cube<true>); the instances the four older kinds run, and the wave-per-shape walks, whose
// lanes hold at most 32 axes, are what they were: to them such a shape has no axes, and what they write for it is overwritten by
// the WIDE instance launched behind them on the same stream.
#define PCV_WIDE_AXES 45
struct PcvShapeWide {
  int32_t naxes;
  int32_t pad;
  double axes[PCV_WIDE_AXES * 3];
  double amin[PCV_WIDE_AXES];
  double amax[PCV_WIDE_AXES];
};
static_assert(PCV_WIDE_AXES == PCV_MAX_SHAPE_AXES, "pcv_shapes_get_ex's capacity");
static_assert(sizeof(PcvShapeDev) == 1632 && offsetof(PcvShapeDev, iso) == 272, "the union keeps the layout of the four older kinds");

struct pcv_shapes {
  pcv_ctx* ctx;
  uint32_t count;
  PcvShapeDev* dev;
  PcvShapeWide* wide = nullptr;  // one per web-mercator rectangle, in shape order
  std::vector<int32_t> kinds;  // host copy: the point kernels are compiled per shape kind
  // cell unions (pcv_shapes_create_ex). On the device a union shape is `valid == 0` with no axes, so every traversal written
  // for the other kinds reports nothing for it at once; the union walk and the union point instances, launched behind them on
  // the same stream, write its counts, lists and flags.
  std::vector<uint32_t> union_first;   // host copies, as given: U + 1 offsets and the cells
  std::vector<uint64_t> union_cells;
  std::vector<uint32_t> union_shapes;  // the shapes of kind PCV_SHAPE_S2_CELL_UNION, ascending
  std::vector<uint32_t> union_of;      // per union shape (same order): its union
  void* d_union = nullptr;             // one block: the cells, their geometry planes, union_shapes
  const uint32_t* d_union_shapes = nullptr;
  // polygons (pcv_shapes_create_ex2). An xy-frame polygon is, like a union, `valid == 0` with no axes on the device; a
  // web-mercator one is its bounding web-mercator rectangle to every node and cell traversal (device kind, corners, axes) and a
  // polygon to the point kernels (point_kind).
  std::vector<uint32_t> polygon_first;   // host copies, as given: P + 1 offsets in rings, R + 1 in vertices, x y pairs
  std::vector<uint32_t> ring_first;
  std::vector<double> vertices;
  std::vector<uint32_t> polygon_shapes;  // the shapes of kind PCV_SHAPE_POLYGON, ascending
  std::vector<uint32_t> polygon_of;      // per polygon shape (same order): its polygon
  std::vector<int32_t> polygon_frame;    // per polygon shape: 0 xy, 1 web-mercator
  std::vector<uint32_t> xy_polygons;     // positions in polygon_shapes of the xy-frame ones (the walk's locations)
  void* d_polygon = nullptr;             // one block: edge tables, raw edges, the xy-frame polygon shapes' indices
  const uint32_t* d_xy_polygon_shapes = nullptr;
  // -1: shape i is no polygon; otherwise its frame
  int polygon_frame_of(uint32_t i) const {
    const auto it = std::lower_bound(polygon_shapes.begin(), polygon_shapes.end(), i);
    return it == polygon_shapes.end() || *it != i ? -1 : polygon_frame[it - polygon_shapes.begin()];
  }
  // the traversals see shape i as a web-mercator rectangle (its own axes in a PcvShapeWide)
  bool wide_shape(uint32_t i) const { return kinds[i] == PCV_SHAPE_WEB_MERCATOR_RECT || polygon_frame_of(i) == 1; }
};

// Device-resident query view of an octree, built lazily (pcv_octree::query, pcv_octree_prepare_query in pcv_cull.hip): one
// block laid out by PcvQueryLayout, the tables of pcv_query_tables.
struct PcvOctreeQuery {
  uint32_t m = 0;
  double* cubes = nullptr;     // Node::get_child recurrence (the block starts here)
  double* fb_cubes = nullptr;  // NodeId::find_bounding_cube recurrence
  BatchNode* nodes = nullptr;  // what the point query's descriptors need of each node
  uint32_t* first_child = nullptr;
  uint8_t* child_mask = nullptr;
  uint8_t* empty = nullptr;
  double* node_rects = nullptr;  // m x 4, own block, built by the first cell-union query (pcv_union.hip): the rect of fb_cubes[i]'s corners
  std::vector<uint32_t> h_first_child;  // host copies for the host-side walk
  std::vector<uint8_t> h_child_mask;
};
// the node table of a prepared octree on the device (pcv_octree_prepare_query), in node order
const BatchNode* pcv_octree_query_nodes(const pcv_octree* t);
// the tree's blobs (an octree opened from a directory: node files are uploaded on first use) and its query tables on the device
int pcv_octree_ensure_query(pcv_octree* t);

// pass 0 writes one descriptor per chunk, so that pass 1 has a single scalar load between "which chunk" and the
// staging loads
struct ChunkDesc {
  uint64_t src;         // offset of the chunk's first encoded byte in the xyz blob
  uint64_t attr_index;  // index of its first point in the rgb / intensity blobs
  double cube_min[3];
  double cube_edge;
  uint64_t keep_off;  // offset of its first flag
  uint32_t enc;
  uint32_t cnt;  // points
};
static_assert(sizeof(ChunkDesc) == 64, "one descriptor per s_load_dwordx16");
constexpr uint32_t kBatchShapeBits = 24;  // ChunkDesc::enc = encoding | kind << 4 | shape << 8
// the chunk's encoded points as load_point takes them
__device__ __forceinline__ PointsView points_view_of(const ChunkDesc& d, const uint8_t* xyz_blob) {
  PointsView v{};
  v.encoded = xyz_blob + d.src;
  v.enc = d.enc & 15u;
  v.cube_min[0] = d.cube_min[0];
  v.cube_min[1] = d.cube_min[1];
  v.cube_min[2] = d.cube_min[2];
  v.cube_edge = d.cube_edge;
  return v;
}

struct pcv_query_batch {
  pcv_ctx* ctx = nullptr;
  pcv_octree* tree = nullptr;  // read by pcv_query_batch_points, never by pcv_query_batch_free
  bool has_intensity = false;
  uint32_t nshapes = 0;
  uint64_t nseg = 0, npoints = 0, nchunks = 0;
  std::vector<uint64_t> shape_first;  // S + 1
  std::vector<uint64_t> seg_chunk;    // nseg + 1: first chunk of each segment
  std::vector<uint64_t> seg_off;      // nseg + 1: first point of each segment
  uint32_t* d_seg_node = nullptr;
  void* d_desc = nullptr;  // ChunkDesc[nchunks]
  uint8_t* d_keep = nullptr;
  uint64_t* d_chunk_off = nullptr;  // nchunks + 1
};

// ---- cell unions over the octree (pcv_union.hip) --------------------------------------------------------------------
// `what` refused because the table holds a cell union (no Relation, no clip matrix): PCV_E_INVALID naming the first one
int pcv_refuse_unions(pcv_ctx* ctx, const pcv_shapes* shapes, const char* what);
// The block behind pcv_shapes::d_union for the table's unions (geometry of every cell, on the stream) and the union members of
// `h` (the host copy of the shape table, before its upload) pointed at it.
int pcv_union_prepare_shapes(pcv_ctx* ctx, pcv_shapes* r, PcvShapeDev* h);
// The node lists of the table's cell unions, behind pcv_launch_node_lists' other launches and with its arguments: counts[f] and
// the list of every union shape f, breadth first (= ascending by node index). queues: m u32 per location in flight, `batch`
// of them. Builds the tree's rect table on first use.
int pcv_launch_union_lists(pcv_ctx* ctx, int label, const pcv_shapes* shapes, const pcv_octree* tree, uint32_t capacity,
                           uint32_t* counts, uint32_t* out, uint32_t* queues, uint32_t batch, const uint64_t* rows);
// the same for one union shape into `nodes` (host), for the single-location point query
int pcv_union_node_list(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_octree* tree, std::vector<uint32_t>* nodes);

// ---- polygons (pcv_polygon.hip) ---------------------------------------------------------------------------------------
// `what` refused because the table holds a polygon (no Relation, no clip matrix): PCV_E_INVALID naming the first one
int pcv_refuse_polygons(pcv_ctx* ctx, const pcv_shapes* shapes, const char* what);
// pcv_polygon_check_host's checks for polygons given as pcv_shapes_create_ex2 takes them; the message in *why
int pcv_polygon_check_table(uint32_t num_polygons, const uint32_t* polygon_first, const uint32_t* ring_first, const double* vertices,
                            std::string* why);
// what a shape adds to its polygon's checks: the frame (params[2]) and what the web-mercator frame asks of vertices and z range
int pcv_polygon_check_shape(double frame, double z_min, double z_max, uint32_t num_rings, const uint32_t* ring_first, const double* vertices,
                            std::string* why);
// The block behind pcv_shapes::d_polygon (edge tables of every polygon that a shape names) and the polygon members of `h`
// pointed at it; a web-mercator member also gets its bounding rectangle's parameters and corners.
int pcv_polygon_prepare_shapes(pcv_ctx* ctx, pcv_shapes* r, PcvShapeDev* h);
// The node lists of the table's xy-frame polygons, behind pcv_launch_node_lists' other launches and with its arguments, as
// pcv_launch_union_lists.
int pcv_launch_polygon_lists(pcv_ctx* ctx, int label, const pcv_shapes* shapes, const pcv_octree* tree, uint32_t capacity,
                             uint32_t* counts, uint32_t* out, uint32_t* queues, uint32_t batch, const uint64_t* rows);
// the same for one xy-frame polygon shape into `nodes` (host), for the single-location point query
int pcv_polygon_node_list(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_octree* tree, std::vector<uint32_t>* nodes);

// out[0 .. n] = exclusive u64 scan of in[0 .. n), out[n] the total (asynchronous on ctx->stream)
int pcv_batch_scan(pcv_ctx* ctx, PcvScratch& sc, const uint32_t* in, uint64_t n, uint64_t* out);

// ---- node culling for the point query (pcv_cull.hip) ---------------------------------------------------------------
// The Relation of every node cube (find_bounding_cube) to shape `shape_index`, dense, into d_rel[m] on ctx->stream: the
// shape's own instance of cull_nodes_kernel, under the PCV_K_CULL_NODES label.
int pcv_launch_relation_row(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_octree* tree, uint8_t* d_rel);
// PointCloud::nodes_in_location of every shape, on ctx->stream: counts[f] and shape f's list at out + rows[f], of at most
// rows[f + 1] - rows[f] entries (rows null: at out + f * capacity, of at most capacity; entries past the end are dropped,
// the count is not). scratch: pcv_node_lists_scratch(shapes->count, m) u32. Profile brackets carry `label`: one per batch of
// the one-lane walk, and one for the wave walk — its own (walk_bracket) or the first batch's.
size_t pcv_node_lists_scratch(uint32_t nshapes, uint32_t m);
int pcv_launch_node_lists(pcv_ctx* ctx, int label, bool walk_bracket, const pcv_shapes* shapes, const pcv_octree* tree,
                          uint32_t capacity, uint32_t* counts, uint32_t* out, uint32_t* scratch, const uint64_t* rows);
