// pcv_cull.hip — node culling and the tree traversals for gfx950, and the octree's query tables on
// the device.
//
//   K7  cull_nodes       sat() of every (shape, node cube) pair (sat.rs:174-205) + relative_size_on_screen
//                        (src/octree/mod.rs:119-139): dense (pcv_cull_nodes), as lists (pcv_cull_nodes_sparse)
//   K7b visible_nodes    Octree::get_visible_nodes — best-first traversal with Rust's BinaryHeap order
//                        (octree/mod.rs:228-283,360-404), one wave per frustum
//   K7c nodes_in_location  NodeIdsIterator BFS (src/octree/octree_iterator.rs, octree/mod.rs:309-323)
//
// The shapes come prepared from pcv_shapes.hip; the tables are those of pcv_query_tables.h. The point query (pcv_query.hip)
// reaches this file through pcv_launch_relation_row and pcv_launch_node_lists, never through a kernel.
// Arithmetic follows the nalgebra 0.22 formulas restated in DESIGN.md ("query arithmetic"); no fused multiply-add
// (-ffp-contract=off). Bound: K7 is f64-VALU bound (about 1 kflop per pair on 128 B of data).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "pcv_query_dev.h"

namespace {

// sat() of one cube against one prepared shape: Out if any axis separates, else Cross if B sticks out on any axis,
// else In (sat.rs:174-194) — so the walk over the axes stops at the first separating one, like the reference's early
// return, and the Relation does not depend on where it stops.
// The interval of the cube's 8 corners on an axis: each corner is fl(fl(x a_x + y a_y) + z a_z) with x, y, z the low or
// high bound; rounding is monotone, so the least (greatest) corner is the one built from the three least (greatest)
// products — 6 min/max + 4 adds instead of 16 adds + 16 min/max. Only when a bound comes out non-finite (inf / NaN
// inputs) are the 8 corners folded literally, in aabb.rs:114-125 order, so that f64::min / max skip NaNs as they do
// in the reference.
// the interval of the cube [l, h]^3 on one axis (see sat_cube): its three least / greatest products, or — non-finite bounds — its
// eight corners folded literally
__device__ __forceinline__ void sat_axis_interval(double lx, double hx, double ly, double hy, double lz, double hz, double ax, double ay,
                                                  double az, double& bmin, double& bmax, double& magnitude) {
  const double plx = lx * ax, phx = hx * ax, ply = ly * ay, phy = hy * ay, plz = lz * az, phz = hz * az;
  bmin = (fmin(plx, phx) + fmin(ply, phy)) + fmin(plz, phz);
  bmax = (fmax(plx, phx) + fmax(ply, phy)) + fmax(plz, phz);
  magnitude = ((fabs(plx) + fabs(phx)) + (fabs(ply) + fabs(phy))) + (fabs(plz) + fabs(phz));
  if (!(fabs(bmin) <= 1.7976931348623157e308 && fabs(bmax) <= 1.7976931348623157e308)) {
    // corners in aabb.rs:114-125 order: (l,l,l) (h,l,l) (l,h,l) (h,h,l) (l,l,h) (h,l,h) (l,h,h) (h,h,h)
    double c0 = (plx + ply) + plz, c1 = (phx + ply) + plz, c2 = (plx + phy) + plz, c3 = (phx + phy) + plz;
    double c4 = (plx + ply) + phz, c5 = (phx + ply) + phz, c6 = (plx + phy) + phz, c7 = (phx + phy) + phz;
    bmin = fmin(fmin(fmin(fmin(fmin(fmin(fmin(fmin(1.7976931348623157e308, c0), c1), c2), c3), c4), c5), c6), c7);
    bmax = fmax(fmax(fmax(fmax(fmax(fmax(fmax(fmax(-1.7976931348623157e308, c0), c1), c2), c3), c4), c5), c6), c7);
  }
}
template <bool WIDE = false>
__device__ __forceinline__ int sat_cube(const PcvShapeDev* __restrict__ s, double mnx, double mny, double mnz, double edge) {
  if (s->kind == PCV_SHAPE_ALL) return 1;  // AllPoints intersects everything (math/mod.rs:139-160) -> "not Out"
  // Cube::to_aabb: Aabb::new(min, min + edge) (inf / sup)
  const double ax_ = mnx + edge, ay_ = mny + edge, az_ = mnz + edge;
  const double lx = fmin(mnx, ax_), hx = fmax(mnx, ax_);
  const double ly = fmin(mny, ay_), hy = fmax(mny, ay_);
  const double lz = fmin(mnz, az_), hz = fmax(mnz, az_);
  bool cross = false;
  const int na = WIDE ? s->wide->naxes : s->naxes;
  const double* axes = WIDE ? s->wide->axes : s->axes;
  const double* amins = WIDE ? s->wide->amin : s->amin;
  const double* amaxs = WIDE ? s->wide->amax : s->amax;
  for (int a = 0; a < na; ++a) {
    double bmin, bmax, mag;
    sat_axis_interval(lx, hx, ly, hy, lz, hz, axes[3 * a], axes[3 * a + 1], axes[3 * a + 2], bmin, bmax, mag);
    const double amin = amins[a], amax = amaxs[a];
    if (bmin > amax || bmax < amin) return 2;
    cross = cross || (amin > bmin || bmax > amax);
  }
  return cross ? 1 : 0;
}

__device__ __forceinline__ double clamp_num(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// octree/mod.rs:103-139. NaN marks the cases where the reference panics (w == 0).
__device__ double size_on_screen(const double* __restrict__ m, double mnx, double mny, double mnz, double edge) {
  const double mxx = mnx + edge, mxy = mny + edge, mxz = mnz + edge;
  const double px[8] = {mnx, mxx, mxx, mnx, mxx, mnx, mxx, mnx};
  const double py[8] = {mny, mxy, mny, mxy, mxy, mny, mny, mxy};
  const double pz[8] = {mnz, mxz, mnz, mnz, mnz, mxz, mxz, mxz};
  double lox = 0, hix = 0, loy = 0, hiy = 0;
  bool bad = false;
  for (int i = 0; i < 8; ++i) {
    double v[4];
    for (int r = 0; r < 4; ++r) v[r] = ((M4(m, r, 0) * px[i] + M4(m, r, 1) * py[i]) + M4(m, r, 2) * pz[i]) + M4(m, r, 3) * 1.0;
    if (v[3] == 0.0) bad = true;
    const double cx = clamp_num(v[0] / v[3], -1., 1.), cy = clamp_num(v[1] / v[3], -1., 1.);
    if (i == 0) {
      lox = hix = cx;
      loy = hiy = cy;
    } else {
      lox = fmin(lox, cx);
      hix = fmax(hix, cx);
      loy = fmin(loy, cy);
      hiy = fmax(hiy, cy);
    }
  }
  if (bad) return __longlong_as_double(0x7ff8000000000000LL);
  return (hix - lox) * (hiy - loy);
}

// K7: grid.y = shape, grid.x covers the nodes. WIDE: the web-mercator rectangles only, with their own axes.
template <bool WIDE = false>
__global__ __launch_bounds__(256) void cull_nodes_kernel(const PcvShapeDev* __restrict__ shapes, uint32_t m,
                                                          const double* __restrict__ cubes /* m x 4 */,
                                                          uint8_t* __restrict__ relation, double* __restrict__ sizes) {
  const PcvShapeDev* s = shapes + blockIdx.y;
  if (WIDE && s->kind != PCV_SHAPE_WEB_MERCATOR_RECT) return;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double4 c = *reinterpret_cast<const double4*>(cubes + 4 * (uint64_t)i);
  const uint64_t o = (uint64_t)blockIdx.y * m + i;
  relation[o] = s->valid ? (uint8_t)sat_cube<WIDE>(s, c.x, c.y, c.z, c.w) : (uint8_t)2;
  if (sizes) sizes[o] = size_on_screen(s->clip_from_query, c.x, c.y, c.z, c.w);
}

// K7s (round 5): the same relations as a LIST per shape. 99.8 % of the (frustum, node) pairs of BASELINE config 4 are Out; the
// dense matrix spends most of its time on the size on screen of pairs nobody looks at (two IEEE divisions per corner) and
// its 546 MB on the way to the host. One workgroup per shape walks the node table in tiles of 256 and appends the nodes
// that are not Out IN NODE ORDER: {node index, relation, relative_size_on_screen} — the size is computed for those only,
// which is exactly where the reference computes it (octree/mod.rs:261-272: a node is projected when it is pushed).
template <bool WIDE = false>  // WIDE: every web-mercator rectangle (no `redo`), with its own axes
__global__ __launch_bounds__(256) void cull_nodes_sparse_kernel(const PcvShapeDev* __restrict__ shapes, uint32_t m,
                                                                 const double* __restrict__ cubes /* m x 4 */, uint32_t capacity,
                                                                 uint32_t* __restrict__ counts, uint32_t* __restrict__ out_node,
                                                                 uint8_t* __restrict__ out_rel, double* __restrict__ out_size,
                                                                 const uint32_t* __restrict__ redo /* set: only the flagged shapes */) {
  __shared__ uint32_t wave_tot[4];
  if (!WIDE && redo && !redo[blockIdx.x]) return;  // (uniform) the tree walk finished this shape
  const PcvShapeDev* s = shapes + blockIdx.x;
  if (WIDE && s->kind != PCV_SHAPE_WEB_MERCATOR_RECT) return;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t row = (uint64_t)blockIdx.x * capacity;
  uint32_t base = 0;  // entries of this shape so far (uniform)
  const bool valid = s->valid != 0;
  for (uint32_t t0 = 0; t0 < m; t0 += 256) {
    const uint32_t i = t0 + threadIdx.x;
    double4 c = make_double4(0, 0, 0, 0);
    int rel = 2;
    if (i < m && valid) {
      c = *reinterpret_cast<const double4*>(cubes + 4 * (uint64_t)i);
      rel = sat_cube<WIDE>(s, c.x, c.y, c.z, c.w);
    }
    const bool keep = rel != 2;
    const uint64_t b = __ballot(keep);
    if (lane == 0) wave_tot[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t v = wave_tot[w];
      before += w < wave ? v : 0u;
      total += v;
    }
    if (keep) {
      const uint32_t pos = base + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
      if (pos < capacity) {
        out_node[row + pos] = i;
        out_rel[row + pos] = (uint8_t)rel;
        if (out_size) out_size[row + pos] = size_on_screen(s->clip_from_query, c.x, c.y, c.z, c.w);
      }
    }
    base += total;
    __syncthreads();  // wave_tot is rewritten by the next tile
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = base;
}

// K7t (round 6): the same lists, descending the tree like the reference's own traversals do (octree_iterator.rs:30-43,
// octree/mod.rs:261-272: children are only tested under a parent that is not Out). 99.76 % of the pairs of BASELINE config 4 are
// Out and nearly all of them sit under an Out ancestor. One WAVE per shape walks the tree breadth first — node order is
// (level, index), so the breadth-first order of the kept nodes IS the list's order.
//   * The wave's lanes are the shape's AXES, not the children: lane l holds axis l mod 32 of the shape (<= 26) in registers for
//     the whole walk, lanes 0-31 test one child of the popped node, lanes 32-63 the next, and three ballots give both Relations
//     (Out if any axis separates, else Cross if the cube sticks out on any axis, else In: sat.rs:174-194 does not depend on the
//     order of the axes). A first form with one child per lane and the loop over the axes inside ran 286-370 us for the 10 000
//     frusta: every round paid all 26 axes for a handful of busy lanes; the flat kernel needed 431.
//   * The queue (LDS) holds the kept INNER nodes only (87 % of a tree's nodes are leaves: listed, never expanded), each with its
//     cube, first child and child mask, so a popped node costs no dependent global load: its children's cubes are the recurrence
//     step NodeId::find_bounding_cube takes (node.rs:160-170: edge /= 2; min += bit * edge) — how the table's own cubes were
//     made (tests/test_gpu_query.py checks it on the node table) — and the children's own masks are requested (lanes 0-7) before
//     the tests and used after them.
//   * relative_size_on_screen of a popped node's kept children: eight lanes per child, one corner each (size_on_screen_by_corner).
// A subtree is skipped only under a node that is Out BY A MARGIN: some axis separates it by more than 1e-9 of the magnitudes
// involved — ~10^6 times the rounding error of any cube inside this one (a descendant's bounds lie within a few ulps of its
// ancestor's: min += bit * edge only adds, max = min + edge) — so every descendant is Out for the flat evaluation too. A shape
// that meets an Out node without that margin (a face within an ulp of a cube face, non-finite bounds), whose frontier outgrows
// the queue, or that is AllPoints, is flagged and redone by the flat kernel (cull_nodes_sparse_kernel with `redo`): the lists
// are the flat kernel's in every case.
__device__ __forceinline__ double size_on_screen_by_corner(const double* __restrict__ m, double mnx, double mny, double mnz, double edge,
                                                           uint32_t corner) {
  // lanes 8 g .. 8 g + 7 take the eight corners of cube g (size_on_screen's order), each its own projection and its two divisions;
  // the corners' clamped x / y are folded with min / max across the eight lanes (a min / max over a set: the order of the fold only
  // decides the sign of a zero)
  const double px = ((0x56u >> corner) & 1u) ? mnx + edge : mnx, py = ((0x9au >> corner) & 1u) ? mny + edge : mny,
               pz = ((0xe2u >> corner) & 1u) ? mnz + edge : mnz;
  double v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = ((M4(m, r, 0) * px + M4(m, r, 1) * py) + M4(m, r, 2) * pz) + M4(m, r, 3) * 1.0;
  bool bad = v[3] == 0.0;
  double lox = clamp_num(v[0] / v[3], -1., 1.), loy = clamp_num(v[1] / v[3], -1., 1.);
  double hix = lox, hiy = loy;
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    lox = fmin(lox, __shfl_xor(lox, o, 64));
    hix = fmax(hix, __shfl_xor(hix, o, 64));
    loy = fmin(loy, __shfl_xor(loy, o, 64));
    hiy = fmax(hiy, __shfl_xor(hiy, o, 64));
    // the exchange first, on every lane: under `bad ||` a lane that is already bad would sit the shuffle out and its partner
    // would read nothing, so a w == 0 on any corner but the first never reached the lane whose result is used
    const int theirs = __shfl_xor((int)bad, o, 64);
    bad = bad || theirs != 0;
  }
  if (bad) return __longlong_as_double(0x7ff8000000000000LL);
  return (hix - lox) * (hiy - loy);
}
struct CullEntry {
  double mnx, mny, mnz, edge;
  uint32_t first_child, mask;
};
constexpr uint32_t kCullQueue = 128;  // kept inner nodes waiting for their children to be tested, per wave (5 KiB: LDS does not bound the occupancy)
// this lane's axis against the cube (mn, mn + edge): does it separate (Out), does the cube stick out (Cross), does it separate by
// the margin
struct AxisTest {
  bool sep, cross, robust;
};
__device__ __forceinline__ AxisTest cull_axis_test(bool on, double ax, double ay, double az, double amin, double amax, double mnx,
                                                   double mny, double mnz, double edge) {
  const double ax_ = mnx + edge, ay_ = mny + edge, az_ = mnz + edge;  // Cube::to_aabb, as sat_cube
  const double lx = fmin(mnx, ax_), hx = fmax(mnx, ax_), ly = fmin(mny, ay_), hy = fmax(mny, ay_), lz = fmin(mnz, az_), hz = fmax(mnz, az_);
  double bmin, bmax, mag;
  sat_axis_interval(lx, hx, ly, hy, lz, hz, ax, ay, az, bmin, bmax, mag);
  AxisTest t;
  t.sep = on && (bmin > amax || bmax < amin);
  t.cross = on && (amin > bmin || bmax > amax);
  const double scale = mag + (fabs(amin) + fabs(amax));
  t.robust = on && fmax(bmin - amax, amin - bmax) > 1e-9 * scale && scale <= 1.7976931348623157e308;  // (NaN / inf anywhere: no)
  return t;
}
// HIER: the walk IS the answer — PointCloud::nodes_in_location (octree/mod.rs:309-323, NodeIdsIterator: a node's children are
// visited iff the node is not Out): every Out node prunes its subtree, margin or not; node indices only.
template <bool SIZES, bool HIER = false>
__global__ __launch_bounds__(256) void cull_nodes_tree_kernel(const PcvShapeDev* __restrict__ shapes, uint32_t nshapes, uint32_t m,
                                                               const double* __restrict__ cubes /* m x 4, find_bounding_cube */,
                                                               const uint32_t* __restrict__ first_child, const uint8_t* __restrict__ child_mask,
                                                               uint32_t capacity, uint32_t* __restrict__ counts, uint32_t* __restrict__ out_node,
                                                               uint8_t* __restrict__ out_rel, double* __restrict__ out_size,
                                                               uint32_t* __restrict__ redo,
                                                               const uint64_t* __restrict__ rows /* set: shape f's list at rows[f] .. rows[f + 1] */) {
  __shared__ CullEntry queue[4][kCullQueue];
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint32_t f = blockIdx.x * 4 + wave;
  if (f >= nshapes) return;  // wave-uniform
  const PcvShapeDev* s = shapes + f;
  const uint64_t row = rows ? rows[f] : (uint64_t)f * capacity;
  if (rows) capacity = (uint32_t)(rows[f + 1] - rows[f]);
  CullEntry* q = queue[wave];
  uint32_t head = 0, tail = 0;  // queue of kept inner nodes
  uint32_t nout = 0;            // listed nodes
  const int na = s->naxes;
  bool again = s->kind == PCV_SHAPE_ALL;  // (every node: the flat kernel lists them as fast)
  // this lane's axis, for the whole walk
  const uint32_t axis = lane & 31u;
  const bool on = (int)axis < na;
  double ax = 0, ay = 0, az = 0, amin = 0, amax = 0;
  if (on) {
    ax = s->axes[3 * axis], ay = s->axes[3 * axis + 1], az = s->axes[3 * axis + 2];
    amin = s->amin[axis], amax = s->amax[axis];
  }
  if (s->valid && !again) {
    {  // the root (both halves of the wave test it: the lower one's ballot bits are read)
      const double4 c = *reinterpret_cast<const double4*>(cubes);
      const AxisTest t = cull_axis_test(on, ax, ay, az, amin, amax, c.x, c.y, c.z, c.w);
      const uint32_t sep = (uint32_t)__ballot(t.sep), cross = (uint32_t)__ballot(t.cross), rob = (uint32_t)__ballot(t.robust);
      if (sep == 0u) {
        const uint32_t cm = child_mask[0];
        if (lane == 0) {
          if (capacity) {  // (entries past `capacity` are dropped, the count is not: capacity 0 only counts)
            out_node[row] = 0;
            if (!HIER) out_rel[row] = (uint8_t)(cross ? 1 : 0);
            if (SIZES) out_size[row] = size_on_screen(s->clip_from_query, c.x, c.y, c.z, c.w);
          }
          q[0] = CullEntry{c.x, c.y, c.z, c.w, first_child[0], cm};
        }
        nout = 1;
        tail = cm ? 1u : 0u;
      } else {
        again = !HIER && rob == 0u;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    while (head < tail && !again) {
      const CullEntry e = q[head & (kCullQueue - 1u)];  // (one address: a broadcast)
      const uint32_t pmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.mask);
      const uint32_t pfirst = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.first_child);
      // the children's own masks / first children: requested now (lanes 0-7), used after the tests
      uint32_t cm = 0, cf = 0;
      const uint32_t mychild = pfirst + (uint32_t)__popc(pmask & ((1u << (lane & 7u)) - 1u));
      if (lane < 8u && ((pmask >> lane) & 1u)) {
        cm = child_mask[mychild];
        cf = first_child[mychild];
      }
      const double half = e.edge / 2.0;  // node.rs:160-170
      uint32_t kept_mask = 0, cross_mask = 0;  // per digit (wave-uniform)
      for (uint32_t rest = pmask; rest != 0u && !again;) {
        const uint32_t d0 = (uint32_t)__builtin_ctz(rest);
        rest &= rest - 1u;
        const uint32_t d1 = rest ? (uint32_t)__builtin_ctz(rest) : 8u;
        rest &= rest - 1u;  // (0 & anything stays 0)
        const uint32_t digit = lane < 32u ? d0 : d1;
        const bool lane_on = on && digit < 8u;
        const double cx = e.mnx + ((digit & 4u) ? half : 0.0), cy = e.mny + ((digit & 2u) ? half : 0.0), cz = e.mnz + ((digit & 1u) ? half : 0.0);
        const AxisTest t = cull_axis_test(lane_on, ax, ay, az, amin, amax, cx, cy, cz, half);
        const uint64_t sep = __ballot(t.sep), cross = __ballot(t.cross), rob = __ballot(t.robust);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const uint32_t d = h ? d1 : d0;
          if (d >= 8u) continue;
          const uint32_t sp = (uint32_t)(sep >> (32 * h)), cr = (uint32_t)(cross >> (32 * h)), rb = (uint32_t)(rob >> (32 * h));
          if (sp == 0u) {
            kept_mask |= 1u << d;
            if (cr) cross_mask |= 1u << d;
          } else if (!HIER && rb == 0u) {
            again = true;  // Out without the margin: its subtree cannot be skipped
          }
        }
      }
      const uint32_t kept = (uint32_t)__popc(kept_mask);
      if (again) break;
      const bool mine = lane < 8u && ((kept_mask >> lane) & 1u);
      const uint32_t k = (uint32_t)__popc(kept_mask & ((1u << (lane & 7u)) - 1u));
      if (mine && nout + k < capacity) {  // (entries past `capacity` are dropped, the count is not)
        out_node[row + nout + k] = mychild;
        if (!HIER) out_rel[row + nout + k] = (uint8_t)((cross_mask >> lane) & 1u);
      }
      if (SIZES && kept && nout < capacity) {  // lanes 8 g .. 8 g + 7: the eight corners of the g-th kept child
        const uint32_t g = lane >> 3;
        uint32_t mk = kept_mask;
        for (uint32_t i = 0; i < g && mk; ++i) mk &= mk - 1u;  // drop the g lowest set bits
        const uint32_t d = mk ? (uint32_t)__builtin_ctz(mk) : (uint32_t)__builtin_ctz(kept_mask);  // (idle groups redo the first: no divergence)
        const double cx = e.mnx + ((d & 4u) ? half : 0.0), cy = e.mny + ((d & 2u) ? half : 0.0), cz = e.mnz + ((d & 1u) ? half : 0.0);
        const double sz = size_on_screen_by_corner(s->clip_from_query, cx, cy, cz, half, lane & 7u);
        if (g < kept && nout + g < capacity && (lane & 7u) == 0u) out_size[row + nout + g] = sz;
      }
      const bool inner = mine && cm != 0u;
      const uint32_t inner_mask = (uint32_t)__ballot(inner);
      const uint32_t pushed = (uint32_t)__popc(inner_mask);
      if (tail + pushed - (head + 1u) > kCullQueue) {  // a frontier wider than the queue: the flat kernel
        again = true;
        break;
      }
      if (inner) {
        const double cx = e.mnx + ((lane & 4u) ? half : 0.0), cy = e.mny + ((lane & 2u) ? half : 0.0), cz = e.mnz + ((lane & 1u) ? half : 0.0);
        q[(tail + (uint32_t)__popc(inner_mask & ((1u << lane) - 1u))) & (kCullQueue - 1u)] = CullEntry{cx, cy, cz, half, cf, cm};
      }
      nout += kept;
      tail += pushed;
      head += 1u;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  if (lane == 0) {
    counts[f] = nout;
    redo[f] = again ? 1u : 0u;
  }
}

struct QTree {
  uint32_t m;
  const double* cubes;         // get_child-style cubes (min xyz, edge), node order = (level, index)
  const uint32_t* first_child;
  const uint8_t* child_mask;
  const uint8_t* empty;        // num_points == 0
};

// K7b: one wave per frustum. Lanes 0..7 run the SAT + size_on_screen of the popped node's children side by side;
// lane 0 owns the BinaryHeap (std's pop / push sift order restated, so the pop order is the reference's). The first
// kHeapLds heap slots live in LDS, anything deeper in the frustum's global scratch (m entries).
// Round 6: an entry carries what popping it needs — the node's first child, its child mask, whether it holds points — fetched
// when the node was PUSHED (beside the SAT / size arithmetic of its siblings), so a pop is followed by ONE global load (the node's
// cube; its children's cubes are Node::get_child steps from it, node.rs:190-211) instead of two dependent rounds of them.
struct HeapEntry {
  double size;
  uint32_t node;
  uint32_t first_child;
  uint32_t bits;  // child mask in bits 0..7, bit 8: Relation::Cross (else In), bit 9: the node holds no points
  uint32_t pad;
};
constexpr uint32_t kHeapLds = 256;  // 24 B entries: 4 waves x 6 KiB per workgroup
struct WaveHeap {
  HeapEntry* lds;
  HeapEntry* glb;  // indexed by heap slot too (its first kHeapLds slots stay unused)
  __device__ __forceinline__ HeapEntry get(uint32_t i) const { return i < kHeapLds ? lds[i] : glb[i]; }
  __device__ __forceinline__ void set(uint32_t i, const HeapEntry& e) const {
    if (i < kHeapLds) lds[i] = e;
    else glb[i] = e;
  }
};
__device__ __forceinline__ void heap_sift_up(const WaveHeap& d, uint32_t start, uint32_t pos) {
  HeapEntry elt = d.get(pos);
  while (pos > start) {
    uint32_t parent = (pos - 1) / 2;
    HeapEntry pe = d.get(parent);
    if (elt.size <= pe.size) break;
    d.set(pos, pe);
    pos = parent;
  }
  d.set(pos, elt);
}
// BinaryHeap::pop: swap the last element in, sift_down_to_bottom, sift_up
__device__ __forceinline__ HeapEntry heap_pop(const WaveHeap& d, uint32_t& len) {
  HeapEntry item = d.get(len - 1);
  --len;
  if (len > 0) {
    HeapEntry top = d.get(0);
    d.set(0, item);
    item = top;
    const uint32_t end = len;
    uint32_t pos = 0, child = 1;
    HeapEntry elt = d.get(0);
    while (child + 1 < end) {
      HeapEntry l = d.get(child), r = d.get(child + 1);
      const bool right = l.size <= r.size;
      child += right ? 1u : 0u;
      d.set(pos, right ? r : l);
      pos = child;
      child = 2 * pos + 1;
    }
    if (child == end - 1) {
      d.set(pos, d.get(child));
      pos = child;
    }
    d.set(pos, elt);
    heap_sift_up(d, 0, pos);
  }
  return item;
}
__global__ __launch_bounds__(256) void visible_nodes_kernel(const PcvShapeDev* __restrict__ shapes, uint32_t first_shape,
                                                             uint32_t nshapes, QTree t, HeapEntry* __restrict__ heaps,
                                                             uint32_t capacity, uint32_t* __restrict__ counts,
                                                             uint32_t* __restrict__ out, int32_t* __restrict__ status) {
  __shared__ HeapEntry lds_heap[4][kHeapLds];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t li = blockIdx.x * 4 + wave;
  if (li >= nshapes) return;  // wave-uniform
  const uint32_t f = first_shape + li;
  const PcvShapeDev* s = shapes + f;
  const WaveHeap d{lds_heap[wave], heaps + (uint64_t)li * t.m};
  uint32_t* o = out + (uint64_t)f * capacity;
  uint32_t len = 0, nout = 0;  // lane 0's
  int32_t st = 0;
  // this lane's axis of the shape, for the whole traversal (lanes 0-31 and 32-63 hold the same axes)
  const bool on = (int)(lane & 31u) < s->naxes;
  double ax = 0, ay = 0, az = 0, amin = 0, amax = 0;
  if (on) {
    ax = s->axes[3 * (lane & 31u)], ay = s->axes[3 * (lane & 31u) + 1], az = s->axes[3 * (lane & 31u) + 2];
    amin = s->amin[lane & 31u], amax = s->amax[lane & 31u];
  }
  if (!s->valid) {  // .expect("Invalid projection matrix.")
    if (lane == 0) {
      counts[f] = 0;
      status[f] = 1;
    }
    return;
  }
  if (t.m > 0 && lane == 0) {  // maybe_push_node(root, Cross)
    double sz = size_on_screen(s->clip_from_query, t.cubes[0], t.cubes[1], t.cubes[2], t.cubes[3]);
    if (sz != sz) st = 2;
    d.set(0, HeapEntry{sz, 0u, t.first_child[0], (uint32_t)t.child_mask[0] | 0x100u | (t.empty[0] ? 0x200u : 0u), 0u});
    len = 1;
  }
  const bool all_points = s->kind == PCV_SHAPE_ALL;
  for (;;) {
    if (!__shfl((int)(len > 0 && st == 0), 0)) break;
    uint32_t node = 0, first = 0, bits = 0;
    if (lane == 0) {
      const HeapEntry item = heap_pop(d, len);
      node = item.node;
      first = item.first_child;
      bits = item.bits;
    }
    node = (uint32_t)__builtin_amdgcn_readfirstlane((int)node);  // (lane 0 is the first active lane)
    first = (uint32_t)__builtin_amdgcn_readfirstlane((int)first);
    bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)bits);
    const uint32_t mask = bits & 0xffu;
    const bool cross_parent = (bits & 0x100u) != 0u;
    // the popped node's cube (one address for the wave) — the only load a pop waits for
    const double4 pc = *reinterpret_cast<const double4*>(t.cubes + 4 * (uint64_t)node);
    // what the children's own entries will need, requested now (lanes 0-7), used when they are pushed
    const uint32_t c = first + (uint32_t)__popc(mask & ((1u << (lane & 7)) - 1u));
    uint32_t cbits = 0, cfirst = 0;
    if (lane < 8 && ((mask >> lane) & 1u)) {
      cbits = (uint32_t)t.child_mask[c] | (t.empty[c] ? 0x200u : 0u);
      cfirst = t.first_child[c];
    }
    const double half = pc.w / 2.;  // Node::get_child (node.rs:190-211): min += half only where the bit is set
    // maybe_push_node on the children that exist: the wave's lanes are the shape's AXES — lanes 0-31 test one child, lanes 32-63
    // the next, two ballots give both Relations — and a kept child's size on screen is computed by eight lanes, one corner each
    // (one lane per child with the 26 axes and the 8 corners in loops left 56 lanes idle for ~3 000 instructions per pop)
    uint32_t kept_mask = mask, cross_mask = 0;  // children of an In node are In without a test (octree/mod.rs:261-272)
    if (cross_parent && all_points) {
      cross_mask = mask;  // sat_cube: AllPoints is "not Out" of everything, reported as Cross
    } else if (cross_parent) {
      kept_mask = 0;
      for (uint32_t rest = mask; rest != 0u;) {
        const uint32_t d0 = (uint32_t)__builtin_ctz(rest);
        rest &= rest - 1u;
        const uint32_t d1 = rest ? (uint32_t)__builtin_ctz(rest) : 8u;
        rest &= rest - 1u;
        const uint32_t digit = lane < 32u ? d0 : d1;
        const double cx = (digit & 4u) ? pc.x + half : pc.x, cy = (digit & 2u) ? pc.y + half : pc.y, cz = (digit & 1u) ? pc.z + half : pc.z;
        const AxisTest at = cull_axis_test(on && digit < 8u, ax, ay, az, amin, amax, cx, cy, cz, half);
        const uint64_t sep = __ballot(at.sep), cross = __ballot(at.cross);
        if ((uint32_t)sep == 0u) {
          kept_mask |= 1u << d0;
          if ((uint32_t)cross) cross_mask |= 1u << d0;
        }
        if (d1 < 8u && (uint32_t)(sep >> 32) == 0u) {
          kept_mask |= 1u << d1;
          if ((uint32_t)(cross >> 32)) cross_mask |= 1u << d1;
        }
      }
    }
    double sz = 0.0;  // lane 8 g: the size of the g-th kept child
    if (kept_mask) {
      const uint32_t g = lane >> 3;
      uint32_t mk = kept_mask;
      for (uint32_t i = 0; i < g && mk; ++i) mk &= mk - 1u;
      const uint32_t dg = (uint32_t)(mk ? __builtin_ctz(mk) : __builtin_ctz(kept_mask));  // (idle groups redo the first: no divergence)
      const double cx = (dg & 4u) ? pc.x + half : pc.x, cy = (dg & 2u) ? pc.y + half : pc.y, cz = (dg & 1u) ? pc.z + half : pc.z;
      sz = size_on_screen_by_corner(s->clip_from_query, cx, cy, cz, half, lane & 7u);
    }
    uint32_t g = 0;
    for (int ci = 0; ci < 8; ++ci) {  // pushes in child order, like the reference's loop
      if (!((kept_mask >> ci) & 1u)) continue;  // (wave-uniform)
      const double z = __shfl(sz, (int)(8u * g));
      const uint32_t cc = (uint32_t)__shfl((int)c, ci), cf = (uint32_t)__shfl((int)cfirst, ci), cb = (uint32_t)__shfl((int)cbits, ci);
      ++g;
      if (lane == 0) {
        if (z != z) st = 2;
        d.set(len, HeapEntry{z, cc, cf, cb | (((cross_mask >> ci) & 1u) << 8), 0u});
        heap_sift_up(d, 0, len);
        ++len;
      }
    }
    if (lane == 0 && !(bits & 0x200u)) {
      if (nout < capacity) o[nout] = node;
      ++nout;
    }
  }
  if (lane == 0) {
    counts[f] = nout;
    status[f] = st;
  }
}

// K7c: BFS of NodeIdsIterator; queue in global scratch. WIDE: every web-mercator rectangle (no `redo`), with its own axes.
template <bool WIDE = false>
__global__ __launch_bounds__(64) void nodes_in_location_kernel(const PcvShapeDev* __restrict__ shapes, uint32_t first_shape,
                                                                uint32_t nshapes, QTree t, const double* __restrict__ fb_cubes,
                                                                uint32_t* __restrict__ queues, uint32_t capacity,
                                                                uint32_t* __restrict__ counts, uint32_t* __restrict__ out,
                                                                const uint32_t* __restrict__ redo /* set: only the flagged shapes */,
                                                                const uint64_t* __restrict__ rows /* set: shape f's list at rows[f] .. rows[f + 1] */) {
  const uint32_t li = blockIdx.x * 64 + threadIdx.x;
  if (li >= nshapes) return;
  const uint32_t f = first_shape + li;
  if (!WIDE && redo && !redo[f]) return;  // the wave-per-shape walk finished this one
  const PcvShapeDev* s = shapes + f;
  if (WIDE && s->kind != PCV_SHAPE_WEB_MERCATOR_RECT) return;
  uint32_t* q = queues + (uint64_t)li * t.m;
  uint32_t* o = out + (rows ? rows[f] : (uint64_t)f * capacity);
  if (rows) capacity = (uint32_t)(rows[f + 1] - rows[f]);
  uint32_t head = 0, tail = 0, nout = 0;
  if (t.m > 0 && s->valid) q[tail++] = 0;
  while (head < tail) {
    const uint32_t cur = q[head++];
    const double* cb = fb_cubes + 4 * (uint64_t)cur;  // NodeMeta::bounding_cube = find_bounding_cube (octree/mod.rs:205)
    if (sat_cube<WIDE>(s, cb[0], cb[1], cb[2], cb[3]) == 2) continue;
    const uint32_t mask = t.child_mask[cur];
    uint32_t cidx = t.first_child[cur];
    for (uint32_t ci = 0; ci < 8; ++ci)
      if ((mask >> ci) & 1u) q[tail++] = cidx++;
    if (nout < capacity) o[nout] = cur;
    ++nout;
  }
  counts[f] = nout;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// the octree's query tables on the device
// ---------------------------------------------------------------------------------------------
const BatchNode* pcv_octree_query_nodes(const pcv_octree* t) { return t->query ? t->query->nodes : nullptr; }

int pcv_octree_prepare_query(pcv_octree* t) {
  if (t->query) return PCV_OK;
  pcv_ctx* ctx = t->ctx;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint32_t m = (uint32_t)t->nodes.size();
  const PcvQueryTables h = pcv_query_tables(t->nodes.data(), m, t->bbox_min, t->bbox_max);
  const PcvQueryLayout at(m);
  void* p;
  int rc;
  if ((rc = ctx->dev_alloc(&p, at.bytes))) return rc;
  uint8_t* base = (uint8_t*)p;
  PcvOctreeQuery* q = new PcvOctreeQuery();
  q->m = m;
  q->cubes = (double*)(base + at.cubes);
  q->fb_cubes = (double*)(base + at.fb_cubes);
  q->nodes = (BatchNode*)(base + at.nodes);
  q->first_child = (uint32_t*)(base + at.first_child);
  q->child_mask = base + at.child_mask;
  q->empty = base + at.empty;
  hipError_t e = hipMemcpy(q->cubes, h.cubes.data(), 32 * (size_t)m, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(q->fb_cubes, h.fb_cubes.data(), 32 * (size_t)m, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(q->nodes, h.nodes.data(), sizeof(BatchNode) * (size_t)m, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(q->first_child, h.first_child.data(), 4 * (size_t)m, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(q->child_mask, h.child_mask.data(), (size_t)m, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(q->empty, h.empty.data(), (size_t)m, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    ctx->dev_free(p);
    delete q;
    return ctx->fail(PCV_E_HIP, hipGetErrorString(e));
  }
  q->h_first_child = h.first_child;
  q->h_child_mask = h.child_mask;
  t->query = q;
  return PCV_OK;
}

void pcv_octree_release_query(pcv_octree* t) {
  if (!t->query) return;
  if (t->query->node_rects) t->ctx->dev_free(t->query->node_rects);
  t->ctx->dev_free(t->query->cubes);
  delete t->query;
  t->query = nullptr;
}

int pcv_octree_ensure_query(pcv_octree* t) {
  if (!t->d_xyz) {  // an octree opened from a directory: node files are uploaded on first use
    int rc = pcv_octree_load_device(t);
    if (rc) return rc;
  }
  return pcv_octree_prepare_query(t);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
extern "C" int pcv_cull_nodes(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, uint8_t* relation,
                              double* size_on_screen_out) {
  if (!ctx) return PCV_E_INVALID;
  if (!shapes || !tree || !relation) return ctx->fail(PCV_E_INVALID, "null argument");
  int rc = pcv_refuse_unions(ctx, shapes, "pcv_cull_nodes");
  if (rc) return rc;
  if ((rc = pcv_refuse_polygons(ctx, shapes, "pcv_cull_nodes"))) return rc;
  rc = pcv_octree_prepare_query(tree);
  if (rc) return rc;
  const uint32_t m = tree->query->m, f = shapes->count;
  if (m == 0 || f == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  uint8_t* d_rel;
  double* d_sz = nullptr;
  if ((rc = sc.get(&d_rel, (size_t)f * m))) return rc;
  if (size_on_screen_out && (rc = sc.get(&d_sz, (size_t)f * m))) return rc;
  {
    PcvProf prof(ctx, PCV_K_CULL_NODES);
    // cull against NodeMeta cubes (find_bounding_cube), as nodes_in_location does; get_visible_nodes' own
    // get_child cubes differ at most in the sign of zero
    hipLaunchKernelGGL(cull_nodes_kernel<false>, dim3((m + 255) / 256, f), dim3(256), 0, ctx->stream, shapes->dev, m,
                       tree->query->fb_cubes, d_rel, d_sz);
    if (shapes->wide)  // the web-mercator rectangles' rows, over what the launch above wrote for them
      hipLaunchKernelGGL(cull_nodes_kernel<true>, dim3((m + 255) / 256, f), dim3(256), 0, ctx->stream, shapes->dev, m,
                         tree->query->fb_cubes, d_rel, d_sz);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(relation, d_rel, (size_t)f * m, hipMemcpyDeviceToHost, ctx->stream));
  if (d_sz) PCV_HIP_CHECK(ctx, hipMemcpyAsync(size_on_screen_out, d_sz, (size_t)f * m * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

int pcv_launch_relation_row(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_octree* tree, uint8_t* d_rel) {
  const uint32_t m = tree->query->m;
  const auto kernel = shapes->wide_shape(shape_index) ? cull_nodes_kernel<true> : cull_nodes_kernel<false>;
  {
    PcvProf prof(ctx, PCV_K_CULL_NODES);
    hipLaunchKernelGGL(kernel, dim3((m + 255) / 256, 1), dim3(256), 0, ctx->stream, shapes->dev + shape_index, m, tree->query->fb_cubes,
                       d_rel, (double*)nullptr);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

extern "C" int pcv_cull_nodes_sparse(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, uint32_t capacity, uint32_t* counts,
                                     uint32_t* node_indices, uint8_t* relation, double* size_on_screen_out) {
  if (!ctx) return PCV_E_INVALID;
  if (!shapes || !tree || !counts || (capacity && (!node_indices || !relation))) return ctx->fail(PCV_E_INVALID, "null argument");
  int rc = pcv_refuse_unions(ctx, shapes, "pcv_cull_nodes_sparse");
  if (rc) return rc;
  if ((rc = pcv_refuse_polygons(ctx, shapes, "pcv_cull_nodes_sparse"))) return rc;
  rc = pcv_octree_prepare_query(tree);
  if (rc) return rc;
  const PcvOctreeQuery* q = tree->query;
  const uint32_t m = q->m, f = shapes->count;
  if (f == 0) return PCV_OK;
  if (m == 0) {
    std::memset(counts, 0, (size_t)f * 4);
    return PCV_OK;
  }
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  const size_t rows = (size_t)f * (capacity ? capacity : 1);
  uint32_t *d_cnt, *d_node;
  uint8_t* d_rel;
  double* d_sz = nullptr;
  if ((rc = sc.get(&d_cnt, f)) || (rc = sc.get(&d_node, rows)) || (rc = sc.get(&d_rel, rows))) return rc;
  if (size_on_screen_out && (rc = sc.get(&d_sz, rows))) return rc;
  uint32_t* d_redo;
  if ((rc = sc.get(&d_redo, f))) return rc;
  {
    PcvProf prof(ctx, PCV_K_CULL_NODES_SPARSE);
    const auto tree_walk = d_sz ? cull_nodes_tree_kernel<true> : cull_nodes_tree_kernel<false>;
    hipLaunchKernelGGL(tree_walk, dim3((f + 3) / 4), dim3(256), 0, ctx->stream, shapes->dev, f, m, q->fb_cubes, q->first_child, q->child_mask,
                       capacity, d_cnt, d_node, d_rel, d_sz, d_redo, (const uint64_t*)nullptr);
    hipLaunchKernelGGL(cull_nodes_sparse_kernel<false>, dim3(f), dim3(256), 0, ctx->stream, shapes->dev, m, q->fb_cubes, capacity, d_cnt,
                       d_node, d_rel, d_sz, (const uint32_t*)d_redo);
    if (shapes->wide)  // the web-mercator rectangles' lists and counts, over what the launches above wrote for them
      hipLaunchKernelGGL(cull_nodes_sparse_kernel<true>, dim3(f), dim3(256), 0, ctx->stream, shapes->dev, m, q->fb_cubes, capacity, d_cnt,
                         d_node, d_rel, d_sz, (const uint32_t*)nullptr);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(counts, d_cnt, (size_t)f * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (capacity) {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(node_indices, d_node, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(relation, d_rel, rows, hipMemcpyDeviceToHost, ctx->stream));
    if (d_sz) PCV_HIP_CHECK(ctx, hipMemcpyAsync(size_on_screen_out, d_sz, rows * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

// Shapes per launch of a traversal that keeps `per_shape` bytes of scratch per shape in flight (m heap entries, m queue
// slots): ~256 MiB per launch, 64 shapes at least.
static uint32_t traversal_batch(uint32_t f, size_t per_shape) {
  return (uint32_t)std::min<size_t>(f, std::max<size_t>(64, ((size_t)256 << 20) / per_shape));
}
static size_t queue_bytes(uint32_t m) { return 4 * (size_t)(m ? m : 1); }  // nodes_in_location_kernel's queue of one shape

size_t pcv_node_lists_scratch(uint32_t f, uint32_t m) { return f + queue_bytes(m) / 4 * traversal_batch(f, queue_bytes(m)); }

// Round 6: one WAVE per shape walks the tree with the lanes as the shape's axes (cull_nodes_tree_kernel<.., HIER>): the
// one-lane-per-shape walk took 3.1 ms for 10 000 frusta; it stays for the shapes the wave walk hands back (a frontier that
// outgrows the wave's queue, AllPoints), batch by batch, and its WIDE instance, behind it in every batch, writes the
// web-mercator rectangles' lists and counts over what the launches before it wrote for them. Cell unions have a walk of their
// own behind all of these (pcv_union.hip), a wave per location, which reuses the queues; so have the xy-frame polygons
// (pcv_polygon.hip). A web-mercator polygon is a web-mercator rectangle here.
int pcv_launch_node_lists(pcv_ctx* ctx, int label, bool walk_bracket, const pcv_shapes* shapes, const pcv_octree* tree,
                          uint32_t capacity, uint32_t* counts, uint32_t* out, uint32_t* scratch, const uint64_t* rows) {
  const PcvOctreeQuery* q = tree->query;
  const uint32_t m = q->m, f = shapes->count;
  const QTree qt{m, q->cubes, q->first_child, q->child_mask, q->empty};
  uint32_t* redo = m ? scratch : nullptr;  // an empty table: the one-lane walk reports no node for every shape
  uint32_t* queues = scratch + f;
  const uint32_t batch = traversal_batch(f, queue_bytes(m));
  auto wave_walk = [&] {
    if (m)
      hipLaunchKernelGGL((cull_nodes_tree_kernel<false, true>), dim3((f + 3) / 4), dim3(256), 0, ctx->stream, shapes->dev, f, m, q->fb_cubes,
                         q->first_child, q->child_mask, capacity, counts, out, (uint8_t*)nullptr, (double*)nullptr, redo, rows);
  };
  if (walk_bracket) {
    PcvProf prof(ctx, label);
    wave_walk();
  }
  for (uint32_t first = 0; first < f; first += batch) {
    const uint32_t nb = std::min(batch, f - first);
    PcvProf prof(ctx, label);
    if (!walk_bracket && first == 0) wave_walk();
    hipLaunchKernelGGL(nodes_in_location_kernel<false>, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, shapes->dev, first, nb, qt,
                       q->fb_cubes, queues, capacity, counts, out, (const uint32_t*)redo, rows);
    if (shapes->wide)
      hipLaunchKernelGGL(nodes_in_location_kernel<true>, dim3((nb + 63) / 64), dim3(64), 0, ctx->stream, shapes->dev, first, nb, qt,
                         q->fb_cubes, queues, capacity, counts, out, (const uint32_t*)nullptr, rows);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  // the cell unions' and the xy-frame polygons' counts and lists, over the zeroes the launches above wrote for them (to those
  // neither is valid)
  const int rc = pcv_launch_union_lists(ctx, label, shapes, tree, capacity, counts, out, queues, batch, rows);
  return rc ? rc : pcv_launch_polygon_lists(ctx, label, shapes, tree, capacity, counts, out, queues, batch, rows);
}

// What the two traversals share. Before their launches: the arguments, the tree's tables, counts and lists on the device
// (*f == 0: nothing to do). After them: counts, lists and — set — the status words to the host.
static int traversal_begin(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, uint32_t capacity, const uint32_t* counts,
                           const uint32_t* node_indices, PcvScratch& sc, uint32_t* f, uint32_t** d_counts, uint32_t** d_out) {
  *f = 0;
  if (!shapes || !tree || !counts || (capacity && !node_indices)) return ctx->fail(PCV_E_INVALID, "null argument");
  int rc = pcv_octree_prepare_query(tree);
  if (rc) return rc;
  if (shapes->count == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if ((rc = sc.get(d_counts, shapes->count)) || (rc = sc.get(d_out, (size_t)shapes->count * (capacity ? capacity : 1)))) return rc;
  *f = shapes->count;
  return PCV_OK;
}
static int traversal_end(pcv_ctx* ctx, uint32_t f, uint32_t capacity, uint32_t* counts, uint32_t* node_indices, int32_t* status,
                         const uint32_t* d_counts, const uint32_t* d_out, const int32_t* d_status) {
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(counts, d_counts, 4 * (size_t)f, hipMemcpyDeviceToHost, ctx->stream));
  if (capacity) PCV_HIP_CHECK(ctx, hipMemcpyAsync(node_indices, d_out, 4 * (size_t)f * capacity, hipMemcpyDeviceToHost, ctx->stream));
  if (status) PCV_HIP_CHECK(ctx, hipMemcpyAsync(status, d_status, 4 * (size_t)f, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_visible_nodes(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, uint32_t capacity,
                                 uint32_t* counts, uint32_t* node_indices, int32_t* status) {
  if (!ctx) return PCV_E_INVALID;
  PcvScratch sc(ctx);
  uint32_t f, *d_counts, *d_out;
  int rc = frusta ? pcv_refuse_unions(ctx, frusta, "pcv_visible_nodes") : PCV_OK;
  if (rc) return rc;
  if (frusta && (rc = pcv_refuse_polygons(ctx, frusta, "pcv_visible_nodes"))) return rc;
  rc = traversal_begin(ctx, frusta, tree, capacity, counts, node_indices, sc, &f, &d_counts, &d_out);
  if (rc || f == 0) return rc;
  const PcvOctreeQuery* q = tree->query;
  const QTree qt{q->m, q->cubes, q->first_child, q->child_mask, q->empty};
  // the heap slots past the wave's LDS: m entries per frustum in flight
  const size_t per = sizeof(HeapEntry) * (size_t)(q->m ? q->m : 1);
  const uint32_t batch = traversal_batch(f, per);
  int32_t* d_status;
  HeapEntry* d_heaps;
  if ((rc = sc.get(&d_status, f)) || (rc = sc.get(&d_heaps, per / sizeof(HeapEntry) * batch))) return rc;
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_status, 0, 4 * (size_t)f, ctx->stream));
  for (uint32_t first = 0; first < f; first += batch) {
    const uint32_t nb = std::min(batch, f - first);
    PcvProf prof(ctx, PCV_K_VISIBLE_NODES);
    hipLaunchKernelGGL(visible_nodes_kernel, dim3((nb + 3) / 4), dim3(256), 0, ctx->stream, frusta->dev, first, nb, qt, d_heaps, capacity,
                       d_counts, d_out, d_status);
  }
  return traversal_end(ctx, f, capacity, counts, node_indices, status, d_counts, d_out, d_status);
}

extern "C" int pcv_nodes_in_location(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, uint32_t capacity,
                                     uint32_t* counts, uint32_t* node_indices) {
  if (!ctx) return PCV_E_INVALID;
  PcvScratch sc(ctx);
  uint32_t f, *d_counts, *d_out, *d_scratch;
  int rc = traversal_begin(ctx, shapes, tree, capacity, counts, node_indices, sc, &f, &d_counts, &d_out);
  if (rc || f == 0) return rc;
  if ((rc = sc.get(&d_scratch, pcv_node_lists_scratch(f, tree->query->m)))) return rc;
  if ((rc = pcv_launch_node_lists(ctx, PCV_K_NODES_IN_LOCATION, true, shapes, tree, capacity, d_counts, d_out, d_scratch, nullptr))) return rc;
  return traversal_end(ctx, f, capacity, counts, node_indices, nullptr, d_counts, d_out, nullptr);
}
