// pcv_xray_inpaint.hip — inpaint_xray_quadtree (xray/src/bin/inpaint_xray_quadtree.rs, xray/src/inpaint.rs) for the leaf
// tiles of a quadtree, on the device. Every step but the fill restates the reference; the fill is this project's own
// (DESIGN 9a): the reference hands the target pixels to the texture-synthesis crate, whose result is not reproducible here.
//
//   host   check, plan     the neighbour quadtrees by the direction of their roots, their adjacent leaves
//                          (get_adjacent_leaf_node_ids :41-71) and nine source slots per leaf (stitched_image :90-121)
//   host   groups          consecutive leaves whose enlarged tiles (their own and those of the neighbours they blend with)
//                          fit the context's xray chunk; one set of work buffers serves every group
//   K_st   stitch          per enlarged tile (2W x 2W): a gather through its nine slots, absent ones transparent; known = alpha != 0
//   K_row  row pass        per 64 rows, staged through LDS in 64-column chunks: the distance to the nearest feature along the
//   K_col  column pass     row (column), capped at 255, one sweep each way; dilate = distance to a set pixel <= d, erode =
//                          distance to a clear pixel > d, windows clipped to the image. Cost does not depend on d.
//                          close = rows, columns (dilate), rows, columns (erode); the last pass leaves closed & !known
//   K_ls   list            the target pixels of the group, compacted (order is free: a target pixel reads known pixels only)
//   K_fl   fill            one thread per target pixel: the smallest ring r that holds a known pixel, then the weighted mean
//                          of the known pixels within 2 r, integer sums in u64
//   K_bl   blend           per final pixel: the horizontal blend of the enlarged tiles, the vertical blend of those results
//                          (interpolate_inpaint_image_with :132-161, f32, every operation rounded on its own), the crop, the
//                          background (alpha < 128) and the three counters
// then create_non_leaf_nodes through xray_build_levels (pcv_xray_pyramid.hip).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "pcv_xray_obj.h"

namespace {

constexpr uint32_t kAbsent = 0xffffffffu;
constexpr uint32_t kTransparentPx = 0x00ffffffu;  // TRANSPARENT.to_u8() = (255, 255, 255, 0), packed
constexpr uint32_t kWhitePx = 0xffffffffu;
constexpr uint32_t kRowChunk = 64;                 // rows per workgroup and columns per LDS chunk of the row pass
constexpr uint32_t kRowStride = kRowChunk / 4 + 1;  // words per staged row: 17, so that 32 rows hit 32 banks

// ---- quadtree ids (quadtree/src/lib.rs:290-349) ---------------------------------------------------------------------------
void spatial_of(uint32_t level, uint64_t index, uint64_t* x, uint64_t* y) {
  *x = *y = 0;
  for (uint32_t b = 0; b < level; ++b) {
    if ((index >> (2 * b)) & 1u) *y |= (uint64_t)1 << b;
    if ((index >> (2 * b + 1)) & 1u) *x |= (uint64_t)1 << b;
  }
}
uint64_t index_of(uint32_t level, uint64_t x, uint64_t y) {
  uint64_t index = 0;
  for (uint32_t b = 0; b < level; ++b) index |= ((y >> b) & 1u) << (2 * b) | ((x >> b) & 1u) << (2 * b + 1);
  return index;
}
// SpatialNodeId::neighbor: (dx, dy) with Top = y + 1; false outside the level's grid
bool neighbor_of(uint32_t level, uint64_t x, uint64_t y, int dx, int dy, uint64_t* nx, uint64_t* ny) {
  const int64_t dim = (int64_t)1 << level, ax = (int64_t)x + dx, ay = (int64_t)y + dy;
  if (ax < 0 || ax >= dim || ay < 0 || ay >= dim) return false;
  *nx = (uint64_t)ax;
  *ny = (uint64_t)ay;
  return true;
}

// Left, Top, Right, Bottom (get_adjacent_leaf_node_ids' order)
constexpr int kDirX[4] = {-1, 0, 1, 0};
constexpr int kDirY[4] = {0, 1, 0, -1};
const char* const kDirName[4] = {"Left", "Top", "Right", "Bottom"};
// the nine slots of a stitched image, rows top to bottom: TopLeft, Top, TopRight, Left, the leaf, Right, BottomLeft, ...
constexpr int kSlotX[9] = {-1, 0, 1, -1, 0, 1, -1, 0, 1};
constexpr int kSlotY[9] = {1, 1, 1, 0, 0, 0, -1, -1, -1};

struct InpaintPlan {
  uint32_t W = 0, deepest = 0, root_level = 0;
  uint64_t root_index = 0;
  std::vector<uint64_t> leaf;            // x's leaves: node index at `deepest`, in x's node order
  int dir_of[4] = {-1, -1, -1, -1};      // neighbour argument per direction
  std::vector<uint32_t> slots;           // 18 per leaf: (part, node) per slot, part 0 = x, k + 1 = neighbours[k]
  std::vector<std::pair<uint32_t, uint32_t>> adjacent;  // the taken leaves of the neighbours, ascending (part, node)
};

bool is_pow2(uint32_t v) { return v && !(v & (v - 1)); }

// the leaves of a part are its nodes 0 .. created.size() - 1 (built, inpainted: created order; opened: descending level)
uint64_t part_leaf_index(const pcv_xray* p, uint64_t c) { return p->geo.index[p->created[c]]; }

int part_root(const pcv_xray* p, const std::string& who, uint32_t* level, uint64_t* index, std::string* err) {
  if (xray_owns_tiles(p)) {
    *level = p->root_level;
    *index = p->root_index;
    return PCV_OK;
  }
  const uint64_t n = p->node_index.size();
  if (n == 0) {
    *err = "xray inpaint: " + who + " has no nodes";
    return PCV_E_INVALID;
  }
  uint64_t at = 0, count = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (p->node_level[i] < p->node_level[at]) at = i, count = 0;
    if (p->node_level[i] == p->node_level[at]) ++count;
  }
  if (count != 1) {
    *err = "xray inpaint: " + who + " has " + std::to_string(count) + " nodes at its minimum level: its root is not defined";
    return PCV_E_INVALID;
  }
  *level = p->node_level[at];
  *index = p->node_index[at];
  return PCV_OK;
}

int check_part(const pcv_xray* p, const std::string& who, std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = "xray inpaint: " + who + m;
    return PCV_E_INVALID;
  };
  if (!p) return bad(" is null");
  if (!xray_is_live(p)) return bad(" is not a live pcv_xray");
  if (p->kind == kXrayMerged) return bad(" is a merged quadtree (inpaint its parts, or write it and open the directory)");
  if (xray_owns_tiles(p) && p->bg != kTransparentPx)
    return bad(" was built with the white background: its holes are gone (build it with PCV_XRAY_BG_TRANSPARENT)");
  return PCV_OK;
}

int inpaint_check(const pcv_xray* x, pcv_xray* const* nb, uint32_t num_nb, uint32_t d, InpaintPlan* plan, std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = m;
    return PCV_E_INVALID;
  };
  if (int rc = check_part(x, "the quadtree", err)) return rc;
  if (d == 255)
    return bad("xray inpaint: inpaint_distance_px 255 is not offered: imageproc's distance transform saturates there and its close is "
               "no longer the morphological one");
  if (d > 255) return bad("xray inpaint: inpaint_distance_px is a u8");
  if (!is_pow2(x->W) || x->W < 2) return bad("xray inpaint: the tile size " + std::to_string(x->W) + " is not a power of two >= 2");
  if (x->W > PCV_XRAY_INPAINT_MAX_TILE)
    return bad("xray inpaint: tiles are at most " + std::to_string(PCV_XRAY_INPAINT_MAX_TILE) + " pixels wide");
  if (num_nb > 4) return bad("xray inpaint: more than 4 neighbour quadtrees");
  if (num_nb && !nb) return bad("xray inpaint: null argument");
  plan->W = x->W;
  plan->deepest = x->geo.deepest_level;
  if (int rc = part_root(x, "the quadtree", &plan->root_level, &plan->root_index, err)) return rc;
  if (plan->root_level > plan->deepest) return bad("xray inpaint: the root's level is above deepest_level");
  uint64_t rx, ry;
  spatial_of(plan->root_level, plan->root_index, &rx, &ry);
  for (uint32_t k = 0; k < num_nb; ++k) {
    const std::string who = "neighbour " + std::to_string(k);
    if (int rc = check_part(nb[k], who, err)) return rc;
    if (nb[k]->W != x->W) return bad("xray inpaint: " + who + " has tile size " + std::to_string(nb[k]->W) + ", not " + std::to_string(x->W));
    if (nb[k]->geo.deepest_level != plan->deepest)
      return bad("xray inpaint: " + who + " has deepest level " + std::to_string(nb[k]->geo.deepest_level) + ", not " + std::to_string(plan->deepest));
    uint32_t level;
    uint64_t index;
    if (int rc = part_root(nb[k], who, &level, &index, err)) return rc;
    int dir = -1;
    for (int t = 0; t < 4 && level == plan->root_level; ++t) {
      uint64_t nx, ny;
      if (neighbor_of(level, rx, ry, kDirX[t], kDirY[t], &nx, &ny) && index_of(level, nx, ny) == index) dir = t;
    }
    if (dir < 0)
      return bad("xray inpaint: the root of " + who + " (" + quad_name(level, index) + ") is not the Left, Top, Right or Bottom neighbour of " +
                 quad_name(plan->root_level, plan->root_index));
    if (plan->dir_of[dir] >= 0) return bad("xray inpaint: two " + std::string(kDirName[dir]) + " neighbours");
    plan->dir_of[dir] = (int)k;
  }
  return PCV_OK;
}

// steps 1 and 2 as a table
void inpaint_plan(const pcv_xray* x, pcv_xray* const* nb, InpaintPlan* plan) {
  const uint32_t D = plan->deepest;
  const uint64_t nc = x->created.size();
  plan->leaf.resize(nc);
  std::unordered_map<uint64_t, uint32_t> own;  // leaf index -> node
  own.reserve(nc * 2);
  for (uint64_t c = 0; c < nc; ++c) own[plan->leaf[c] = part_leaf_index(x, c)] = (uint32_t)c;
  // get_adjacent_leaf_node_ids: a leaf of the neighbour in direction t whose neighbour in the opposite direction is a leaf of x
  std::unordered_map<uint64_t, std::pair<uint32_t, uint32_t>> foreign;  // leaf index -> (part, node)
  for (int t = 0; t < 4; ++t) {
    if (plan->dir_of[t] < 0) continue;
    const pcv_xray* p = nb[plan->dir_of[t]];
    for (uint64_t c = 0; c < p->created.size(); ++c) {
      const uint64_t idx = part_leaf_index(p, c);
      uint64_t px, py, ox, oy;
      spatial_of(D, idx, &px, &py);
      if (!neighbor_of(D, px, py, -kDirX[t], -kDirY[t], &ox, &oy) || !own.count(index_of(D, ox, oy))) continue;
      if (foreign.emplace(idx, std::make_pair((uint32_t)plan->dir_of[t] + 1, (uint32_t)c)).second)
        plan->adjacent.emplace_back((uint32_t)plan->dir_of[t] + 1, (uint32_t)c);
    }
  }
  std::sort(plan->adjacent.begin(), plan->adjacent.end());
  plan->slots.assign(18 * nc, kAbsent);
  for (uint64_t c = 0; c < nc; ++c) {
    uint64_t lx, ly;
    spatial_of(D, plan->leaf[c], &lx, &ly);
    for (int s = 0; s < 9; ++s) {
      uint64_t nx, ny;
      if (!neighbor_of(D, lx, ly, kSlotX[s], kSlotY[s], &nx, &ny)) continue;
      const uint64_t idx = index_of(D, nx, ny);
      auto o = own.find(idx);
      if (o != own.end()) {
        plan->slots[18 * c + 2 * s] = 0;
        plan->slots[18 * c + 2 * s + 1] = o->second;
        continue;
      }
      auto f = foreign.find(idx);
      if (f != foreign.end()) {
        plan->slots[18 * c + 2 * s] = f->second.first;
        plan->slots[18 * c + 2 * s + 1] = f->second.second;
      }
    }
  }
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
struct StitchArgs {
  const uint32_t* leaves;  // x's leaf images, W x W each
  const uint32_t* adj;     // the adjacent leaves of the neighbours, in the plan's order
  uint32_t nleaves;
  const int32_t* slots;    // 9 per enlarged tile: < 0 absent, < nleaves a leaf of x, else nleaves + adjacent position
  uint32_t* rgba;          // 2W x 2W per enlarged tile
  uint8_t* known;
  uint64_t quads;          // tiles x 2W x 2W / 4
  uint32_t W;
};

// one thread per four pixels of a row of an enlarged tile
__global__ __launch_bounds__(256) void xray_inpaint_stitch_kernel(StitchArgs a) {
  const uint32_t W = a.W, n = 2 * W, w = W / 2, qrow = n / 4;
  const uint64_t per_tile = (uint64_t)n * qrow;
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < a.quads; id += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t e = id / per_tile;
    const uint32_t q = (uint32_t)(id % per_tile), Y = q / qrow, X0 = (q % qrow) * 4;
    const uint32_t cy = Y < w ? 0u : (Y < 3 * w ? 1u : 2u);
    const uint32_t sy = cy == 0 ? Y + w : (cy == 1 ? Y - w : Y - 3 * w);
    uint32_t px[4], kn = 0;
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t X = X0 + j;
      const uint32_t cx = X < w ? 0u : (X < 3 * w ? 1u : 2u);
      const uint32_t sx = cx == 0 ? X + w : (cx == 1 ? X - w : X - 3 * w);
      const int32_t s = a.slots[e * 9 + cy * 3 + cx];
      uint32_t p = kTransparentPx;
      if (s >= 0) {
        const uint32_t* img = (uint32_t)s < a.nleaves ? a.leaves + (uint64_t)s * W * W : a.adj + (uint64_t)((uint32_t)s - a.nleaves) * W * W;
        p = img[(uint64_t)sy * W + sx];
      }
      px[j] = p;
      kn |= ((p >> 24) != 0 ? 1u : 0u) << (8 * j);
    }
    const uint64_t at = e * n * n + (uint64_t)Y * n + X0;
    *reinterpret_cast<uint4*>(a.rgba + at) = make_uint4(px[0], px[1], px[2], px[3]);
    *reinterpret_cast<uint32_t*>(a.known + at) = kn;
  }
}

// The two sweeps of a line pass share one step: the distance to the nearest feature so far, capped at 255 (> any d)
__device__ __forceinline__ uint32_t step_dist(uint32_t dist, bool feature) { return feature ? 0u : min(dist + 1u, 255u); }

// Row pass over `rows` rows of n bytes (the tiles' rows back to back): 64 threads per 64 rows, one row each, the row chunks
// staged through LDS so that global accesses are whole words of consecutive lanes. in != out.
__global__ __launch_bounds__(64) void xray_inpaint_row_kernel(const uint8_t* in, uint8_t* out, uint64_t rows, uint32_t n, uint32_t d, int erode) {
  __shared__ uint32_t sm[kRowChunk * kRowStride];
  __shared__ uint32_t sd[kRowChunk * kRowStride];
  const uint32_t lane = threadIdx.x;
  const uint32_t cw = min(n, kRowChunk), wq = cw / 4;
  const uint64_t blocks = (rows + kRowChunk - 1) / kRowChunk;
  for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
    const uint64_t row0 = b * kRowChunk;
    const uint32_t nrows = (uint32_t)min((uint64_t)kRowChunk, rows - row0);
    uint32_t dist = 255;
    for (uint32_t c0 = 0; c0 < n; c0 += cw) {  // left to right: the distance to the nearest feature on the left
      for (uint32_t i = lane; i < nrows * wq; i += 64) {
        const uint32_t r = i / wq, q = i % wq;
        sm[r * kRowStride + q] = *reinterpret_cast<const uint32_t*>(in + (row0 + r) * n + c0 + 4 * q);
      }
      __syncthreads();
      if (lane < nrows)
        for (uint32_t q = 0; q < wq; ++q) {
          const uint32_t m = sm[lane * kRowStride + q];
          uint32_t o = 0;
          for (uint32_t j = 0; j < 4; ++j) {
            dist = step_dist(dist, (((m >> (8 * j)) & 255u) != 0) != (erode != 0));
            o |= dist << (8 * j);
          }
          sm[lane * kRowStride + q] = o;
        }
      __syncthreads();
      for (uint32_t i = lane; i < nrows * wq; i += 64) {
        const uint32_t r = i / wq, q = i % wq;
        *reinterpret_cast<uint32_t*>(out + (row0 + r) * n + c0 + 4 * q) = sm[r * kRowStride + q];
      }
      __syncthreads();
    }
    dist = 255;
    for (uint32_t c1 = n; c1 > 0; c1 -= cw) {  // right to left, joined with the left distances
      const uint32_t c0 = c1 - cw;
      for (uint32_t i = lane; i < nrows * wq; i += 64) {
        const uint32_t r = i / wq, q = i % wq;
        sm[r * kRowStride + q] = *reinterpret_cast<const uint32_t*>(in + (row0 + r) * n + c0 + 4 * q);
        sd[r * kRowStride + q] = *reinterpret_cast<const uint32_t*>(out + (row0 + r) * n + c0 + 4 * q);
      }
      __syncthreads();
      if (lane < nrows)
        for (uint32_t q = wq; q-- > 0;) {
          const uint32_t m = sm[lane * kRowStride + q], l = sd[lane * kRowStride + q];
          uint32_t o = 0;
          for (uint32_t j = 4; j-- > 0;) {
            dist = step_dist(dist, (((m >> (8 * j)) & 255u) != 0) != (erode != 0));
            const bool near = min(dist, (l >> (8 * j)) & 255u) <= d;
            o |= (near != (erode != 0) ? 1u : 0u) << (8 * j);
          }
          sd[lane * kRowStride + q] = o;
        }
      __syncthreads();
      for (uint32_t i = lane; i < nrows * wq; i += 64) {
        const uint32_t r = i / wq, q = i % wq;
        *reinterpret_cast<uint32_t*>(out + (row0 + r) * n + c0 + 4 * q) = sd[r * kRowStride + q];
      }
      __syncthreads();
    }
  }
}

// Column pass: one thread per four adjacent columns of a tile, down and then up. known != null (the last pass of the
// close): the result is cleared where the pixel is known, which leaves the target mask. in != out.
__global__ __launch_bounds__(256) void xray_inpaint_col_kernel(const uint8_t* in, uint8_t* out, const uint8_t* known, uint64_t tiles, uint32_t n,
                                                               uint32_t d, int erode) {
  const uint32_t qrow = n / 4;
  const uint64_t total = tiles * qrow;
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t base = (id / qrow) * n * n + (id % qrow) * 4;
    uint32_t dist[4] = {255, 255, 255, 255};
    for (uint32_t y = 0; y < n; ++y) {
      const uint32_t m = *reinterpret_cast<const uint32_t*>(in + base + (uint64_t)y * n);
      uint32_t o = 0;
      for (uint32_t j = 0; j < 4; ++j) {
        dist[j] = step_dist(dist[j], (((m >> (8 * j)) & 255u) != 0) != (erode != 0));
        o |= dist[j] << (8 * j);
      }
      *reinterpret_cast<uint32_t*>(out + base + (uint64_t)y * n) = o;
    }
    for (uint32_t j = 0; j < 4; ++j) dist[j] = 255;
    for (uint32_t y = n; y-- > 0;) {
      const uint32_t m = *reinterpret_cast<const uint32_t*>(in + base + (uint64_t)y * n);
      const uint32_t l = *reinterpret_cast<const uint32_t*>(out + base + (uint64_t)y * n);
      const uint32_t k = known ? *reinterpret_cast<const uint32_t*>(known + base + (uint64_t)y * n) : 0u;
      uint32_t o = 0;
      for (uint32_t j = 0; j < 4; ++j) {
        dist[j] = step_dist(dist[j], (((m >> (8 * j)) & 255u) != 0) != (erode != 0));
        const bool near = min(dist[j], (l >> (8 * j)) & 255u) <= d;
        const bool v = (near != (erode != 0)) && ((k >> (8 * j)) & 255u) == 0;
        o |= (v ? 1u : 0u) << (8 * j);
      }
      *reinterpret_cast<uint32_t*>(out + base + (uint64_t)y * n) = o;
    }
  }
}

// the set bytes of the target masks as pixel numbers (tile * 4 W W + pixel), in no particular order
__global__ __launch_bounds__(256) void xray_inpaint_list_kernel(const uint8_t* target, uint64_t quads, uint32_t* list, unsigned long long* count) {
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < quads; id += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t m = *reinterpret_cast<const uint32_t*>(target + 4 * id);
    for (uint32_t j = 0; j < 4; ++j)
      if ((m >> (8 * j)) & 255u) list[atomicAdd(count, 1ull)] = (uint32_t)(4 * id + j);
  }
}

// Step 4 for one target pixel per thread. Sources are pixels of the known mask only, and those are never written here.
__global__ __launch_bounds__(256) void xray_inpaint_fill_kernel(uint32_t* rgba, const uint8_t* known, const uint32_t* list,
                                                                const unsigned long long* count, uint32_t n, uint32_t d) {
  const uint64_t total = *count, per_tile = (uint64_t)n * n;
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t pix = list[id];
    const uint64_t tile = pix / per_tile * per_tile;
    const uint32_t p = (uint32_t)(pix - tile);
    const int32_t py = (int32_t)(p / n), px = (int32_t)(p % n), last = (int32_t)n - 1;
    const uint8_t* kn = known + tile;
    const uint32_t* img = rgba + tile;
    uint32_t r = 0;
    for (int32_t t = 1; t <= (int32_t)d && r == 0; ++t) {  // the ring at Chebyshev distance t, clipped
      const int32_t x0 = max(px - t, 0), x1 = min(px + t, last), y0 = max(py - t, 0), y1 = min(py + t, last);
      bool hit = false;
      if (py - t >= 0)
        for (int32_t x = x0; x <= x1; ++x) hit |= kn[(uint32_t)(py - t) * n + x] != 0;
      if (py + t <= last)
        for (int32_t x = x0; x <= x1; ++x) hit |= kn[(uint32_t)(py + t) * n + x] != 0;
      if (px - t >= 0)
        for (int32_t y = y0; y <= y1; ++y) hit |= kn[(uint32_t)y * n + (px - t)] != 0;
      if (px + t <= last)
        for (int32_t y = y0; y <= y1; ++y) hit |= kn[(uint32_t)y * n + (px + t)] != 0;
      if (hit) r = (uint32_t)t;
    }
    if (r == 0) continue;  // not reached: a target pixel lies in dilate(known, d)
    const int32_t R = 2 * (int32_t)r;
    const int32_t x0 = max(px - R, 0), x1 = min(px + R, last), y0 = max(py - R, 0), y1 = min(py + R, last);
    uint64_t sr = 0, sg = 0, sb = 0, sw = 0;
    for (int32_t y = y0; y <= y1; ++y)
      for (int32_t x = x0; x <= x1; ++x) {
        if (!kn[(uint32_t)y * n + x]) continue;
        const uint64_t wgt = (uint64_t)(R + 1 - max(abs(x - px), abs(y - py)));
        const uint32_t c = img[(uint32_t)y * n + x];
        sr += wgt * (c & 255u);
        sg += wgt * ((c >> 8) & 255u);
        sb += wgt * ((c >> 16) & 255u);
        sw += wgt;
      }
    rgba[tile + p] = (uint32_t)((sr + sw / 2) / sw) | (uint32_t)((sg + sw / 2) / sw) << 8 | (uint32_t)((sb + sw / 2) / sw) << 16 | 0xff000000u;
  }
}

struct BlendArgs {
  const uint32_t* rgba;   // the group's enlarged tiles after the fill
  const uint8_t* known;
  const uint8_t* target;
  const int32_t* tbl;     // 9 per leaf of the group: the enlarged tile of the slot's leaf of x, < 0 where it takes no part
  uint32_t* out;          // the group's first final tile
  unsigned long long* counts;  // 3 per leaf of the group: target, filled, blended
  uint32_t W, bg, blocks_per_leaf;
};

// interpolate_pixels (utils.rs:46-60): per channel (this * wt + other * (1 - wt)).round() as u8, f32, nothing fused
__device__ __forceinline__ uint32_t blend_px(uint32_t self, uint32_t other, float wt) {
  const float rest = 1.0f - wt;
  uint32_t o = 0;
  for (uint32_t c = 0; c < 4; ++c) {
    const float a = (float)((self >> (8 * c)) & 255u) * wt;
    const float b = (float)((other >> (8 * c)) & 255u) * rest;
    const float v = roundf(a + b);
    o |= (v >= 255.0f ? 255u : (uint32_t)v) << (8 * c);
  }
  return o;
}

// an enlarged tile after the horizontal phase: its right half against the left half of its Right neighbour (the neighbour
// is `this`), its left half against the right half of its Left neighbour (the tile itself is `this`)
__device__ __forceinline__ uint32_t blend_h(const uint32_t* rgba, uint32_t n, int32_t self, int32_t left, int32_t right, uint32_t X, uint32_t Y) {
  const uint64_t per_tile = (uint64_t)n * n;
  const uint32_t half = n / 2;
  const uint32_t cur = rgba[(uint64_t)self * per_tile + (uint64_t)Y * n + X];
  if (X >= half) {
    if (right < 0) return cur;
    const uint32_t i = X - half;
    return blend_px(rgba[(uint64_t)right * per_tile + (uint64_t)Y * n + i], cur, (float)i / (float)(half - 1));
  }
  if (left < 0) return cur;
  return blend_px(cur, rgba[(uint64_t)left * per_tile + (uint64_t)Y * n + X + half], (float)X / (float)(half - 1));
}

// 256 threads per (leaf of the group, 256 final pixels)
__global__ __launch_bounds__(256) void xray_inpaint_blend_kernel(BlendArgs a) {
  const uint32_t W = a.W, n = 2 * W, half = W, w = W / 2;
  const uint32_t leaf = blockIdx.x / a.blocks_per_leaf;
  const uint32_t p = (blockIdx.x % a.blocks_per_leaf) * 256 + threadIdx.x;
  const int32_t* t = a.tbl + 9 * (uint64_t)leaf;
  bool is_target = false, is_filled = false, is_blended = false;
  if (p < W * W) {
    const uint32_t X = p % W + w, Y = p / W + w;
    const int32_t self = t[4];
    const uint64_t at = (uint64_t)self * n * n + (uint64_t)Y * n + X;
    const uint32_t before = a.rgba[at];
    uint32_t v = blend_h(a.rgba, n, self, t[3], t[5], X, Y);
    if (Y >= half) {
      if (t[7] >= 0) {  // Bottom (y - 1) is `this`
        const uint32_t j = Y - half;
        v = blend_px(blend_h(a.rgba, n, t[7], t[6], t[8], X, j), v, (float)j / (float)(half - 1));
      }
    } else if (t[1] >= 0) {  // this tile is the Bottom neighbour of Top
      v = blend_px(v, blend_h(a.rgba, n, t[1], t[0], t[2], X, Y + half), (float)Y / (float)(half - 1));
    }
    is_target = a.target[at] != 0;
    is_filled = (v >> 24) >= 128 && a.known[at] == 0;
    is_blended = v != before;
    a.out[(uint64_t)leaf * W * W + p] = (v >> 24) < 128 ? a.bg : v;  // assign_background_color
  }
  const unsigned long long mt = __ballot(is_target), mf = __ballot(is_filled), mb = __ballot(is_blended);
  if ((threadIdx.x & 63u) == 0) {
    unsigned long long* c = a.counts + 3 * (uint64_t)leaf;
    if (mt) atomicAdd(c, (unsigned long long)__popcll(mt));
    if (mf) atomicAdd(c + 1, (unsigned long long)__popcll(mf));
    if (mb) atomicAdd(c + 2, (unsigned long long)__popcll(mb));
  }
}

// d == 0: assign_background_color alone
__global__ __launch_bounds__(256) void xray_inpaint_background_kernel(const uint32_t* in, uint32_t* out, uint64_t pixels, uint32_t bg) {
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < pixels; id += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = in[id];
    out[id] = (v >> 24) < 128 ? bg : v;
  }
}

uint32_t grid_for(uint64_t threads, uint32_t block) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((threads + block - 1) / block, 8192)); }

// the tile of leaf `node` of a built or inpainted part, or the decoded file of an opened one, on its way into dst
struct TileStage {
  pcv_ctx* ctx;
  uint64_t tile_bytes, cap = 0, used = 0;
  uint8_t* host = nullptr;
  int open(uint64_t opened_tiles) {
    if (opened_tiles == 0) return PCV_OK;
    cap = std::max<uint64_t>(1, std::min(opened_tiles, ctx->xray_chunk_bytes / tile_bytes));
    return ctx->host_alloc((void**)&host, cap * tile_bytes);
  }
  int flush() {  // the pinned block is free again once its uploads have completed
    if (used && hipStreamSynchronize(ctx->stream) != hipSuccess) return ctx->fail(PCV_E_HIP, "xray inpaint: tile upload");
    used = 0;
    return PCV_OK;
  }
  int add(pcv_xray* part, uint64_t node, uint8_t* dst) {
    if (xray_owns_tiles(part)) return queue_node_images(part, node, 1, dst, hipMemcpyDeviceToDevice);
    if (used == cap)
      if (int rc = flush()) return rc;
    uint8_t* h = host + used * tile_bytes;
    if (int rc = opened_node_to_host(part, node, h)) return part->ctx ? rc : ctx->fail(rc, pcv_host_last_error());
    ++used;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst, h, tile_bytes, hipMemcpyHostToDevice, ctx->stream));
    return PCV_OK;
  }
  void close() {
    if (host) ctx->host_release(host);
    host = nullptr;
  }
};

void copy_err(const std::string& m, char* err, uint64_t errcap) {
  if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
}

}  // namespace

extern "C" int pcv_xray_inpaint_check(const pcv_xray* x, pcv_xray* const* neighbours, uint32_t num_neighbours, uint32_t distance_px, char* err,
                                      uint64_t errcap) {
  InpaintPlan plan;
  std::string m;
  const int rc = inpaint_check(x, neighbours, num_neighbours, distance_px, &plan, &m);
  if (rc) copy_err(m, err, errcap);
  return rc;
}

extern "C" int pcv_xray_inpaint_plan(const pcv_xray* x, pcv_xray* const* neighbours, uint32_t num_neighbours, uint64_t capacity, uint32_t* slots,
                                     uint64_t* num_adjacent, char* err, uint64_t errcap) {
  InpaintPlan plan;
  std::string m;
  const int rc = inpaint_check(x, neighbours, num_neighbours, 0, &plan, &m);
  if (rc) {
    copy_err(m, err, errcap);
    return rc;
  }
  inpaint_plan(x, neighbours, &plan);
  if (num_adjacent) *num_adjacent = plan.adjacent.size();
  if (slots) std::memcpy(slots, plan.slots.data(), 4 * 18 * std::min<uint64_t>(capacity, plan.leaf.size()));
  return PCV_OK;
}

extern "C" int pcv_xray_inpaint(pcv_ctx* ctx, pcv_xray* xin, pcv_xray* const* neighbours, uint32_t num_neighbours, uint32_t distance_px,
                                uint32_t background, pcv_xray** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (background > PCV_XRAY_BG_TRANSPARENT) return ctx->fail(PCV_E_INVALID, "xray: unknown background");
  InpaintPlan plan;
  std::string m;
  int rc = inpaint_check(xin, neighbours, num_neighbours, distance_px, &plan, &m);
  if (rc) return ctx->fail(rc, m);
  if (xin->ctx && xin->ctx != ctx) return ctx->fail(PCV_E_INVALID, "xray inpaint: the quadtree belongs to another context");
  for (uint32_t k = 0; k < num_neighbours; ++k)
    if (neighbours[k]->ctx && neighbours[k]->ctx != ctx)
      return ctx->fail(PCV_E_INVALID, "xray inpaint: neighbour " + std::to_string(k) + " belongs to another context");
  inpaint_plan(xin, neighbours, &plan);
  const uint32_t W = plan.W, n = 2 * W, d = distance_px;
  const uint64_t nc = plan.leaf.size(), na = d ? plan.adjacent.size() : 0, tile_px = (uint64_t)W * W, tile_bytes = 4 * tile_px, big_px = 4 * tile_px;
  const uint32_t bg = background == PCV_XRAY_BG_TRANSPARENT ? kTransparentPx : kWhitePx;

  // groups of consecutive leaves and the enlarged tiles each needs: the leaf's own, Left / Right, Top / Bottom and, where
  // Top or Bottom is there, that one's Left / Right
  struct Group {
    uint64_t first, count, efirst, ecount;
  };
  std::vector<Group> groups;
  std::vector<uint32_t> etile;  // per enlarged tile of every group: the leaf of x
  std::vector<int32_t> tbl(9 * nc, -1);
  uint64_t max_e = 0;
  if (d) {
    const uint64_t fit = std::min<uint64_t>(ctx->xray_chunk_bytes / PCV_XRAY_INPAINT_WORK_BYTES(W), 0xffffffffull / big_px);
    const uint64_t cap_e = std::max<uint64_t>(9, fit);
    std::vector<int32_t> eslot(nc, -1);
    Group g{0, 0, 0, 0};
    auto close_group = [&]() {
      for (uint64_t e = g.efirst; e < g.efirst + g.ecount; ++e) eslot[etile[e]] = -1;
      max_e = std::max(max_e, g.ecount);
      groups.push_back(g);
      g = Group{g.first + g.count, 0, etile.size(), 0};
    };
    for (uint64_t c = 0; c < nc; ++c) {
      const uint32_t* s = plan.slots.data() + 18 * c;
      auto own = [&](int k) { return s[2 * k] == 0; };
      bool need[9] = {own(1) && own(0), own(1), own(1) && own(2), own(3), true, own(5), own(7) && own(6), own(7), own(7) && own(8)};
      uint64_t fresh = 0;
      for (int k = 0; k < 9; ++k) fresh += need[k] && eslot[s[2 * k + 1]] < 0;
      if (g.count && g.ecount + fresh > cap_e) {
        close_group();
      }
      for (int k = 0; k < 9; ++k) {
        if (!need[k]) continue;
        const uint32_t leaf = s[2 * k + 1];
        if (eslot[leaf] < 0) {
          eslot[leaf] = (int32_t)g.ecount++;
          etile.push_back(leaf);
        }
        tbl[9 * c + k] = eslot[leaf];
      }
      ++g.count;
    }
    if (g.count) close_group();
  }
  const uint64_t ne = etile.size();
  // the stitch table of every enlarged tile: the plan's slots as positions in [x's leaves, adjacent leaves]
  std::vector<int32_t> st(9 * ne, -1);
  for (uint64_t e = 0; e < ne; ++e)
    for (int k = 0; k < 9; ++k) {
      const uint32_t part = plan.slots[18 * (uint64_t)etile[e] + 2 * k], node = plan.slots[18 * (uint64_t)etile[e] + 2 * k + 1];
      if (part == kAbsent) continue;
      if (part == 0) st[9 * e + k] = (int32_t)node;
      else st[9 * e + k] = (int32_t)(nc + (uint64_t)(std::lower_bound(plan.adjacent.begin(), plan.adjacent.end(), std::make_pair(part, node)) - plan.adjacent.begin()));
    }
  if (nc + na > 0x7fffffffull) return ctx->fail(PCV_E_INVALID, "xray inpaint: more than 2^31 source tiles");

  // the result's node list: x's leaves in x's order, then create_non_leaf_nodes' levels
  pcv_xray* x = new pcv_xray();
  x->ctx = ctx;
  x->kind = kXrayInpainted;
  x->W = W;
  x->bg = bg;
  x->root_level = plan.root_level;
  x->root_index = plan.root_index;
  x->geo.deepest_level = plan.deepest;
  if (xin->kind == kXrayBuilt) built_root_rect(xin, x->geo.rect);
  else std::memcpy(x->geo.rect, xin->geo.rect, sizeof(x->geo.rect));
  x->geo.index = plan.leaf;
  x->created.resize(nc);
  for (uint64_t c = 0; c < nc; ++c) x->created[c] = c;
  x->kept.assign(nc, 0);
  x->drawn.assign(nc, 0);
  x->negative.assign(nc, 0);
  x->inpaint_target.assign(nc, 0);
  x->inpaint_filled.assign(nc, 0);
  x->inpaint_blended.assign(nc, 0);
  x->parents_built = true;
  auto finish_nodes = [&]() {
    x->node_level.assign(nc, plan.deepest);
    x->node_index = plan.leaf;
    x->node_level.insert(x->node_level.end(), x->parent_level.begin(), x->parent_level.end());
    x->node_index.insert(x->node_index.end(), x->parent_index.begin(), x->parent_index.end());
  };
  if (nc == 0) {
    finish_nodes();
    *out = x;
    return PCV_OK;
  }

  // ---- everything is allocated here, before the first launch ---------------------------------------------------------
  PcvScratch sc(ctx);
  TileStage stage{ctx, tile_bytes};
  auto undo = [&](int code) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    stage.close();
    pcv_xray_free(x);
    return code;
  };
  if (hipSetDevice(ctx->device) != hipSuccess) return undo(ctx->fail(PCV_E_HIP, "hipSetDevice"));
  const uint64_t np = xray_count_levels(plan.leaf, plan.deepest, plan.root_level);
  const bool x_opened = xin->kind == kXrayOpened;
  uint32_t *d_src = nullptr, *d_adj = nullptr, *d_rgba = nullptr, *d_list = nullptr;
  uint8_t *d_known = nullptr, *d_ma = nullptr, *d_mb = nullptr;
  int32_t *d_st = nullptr, *d_tbl = nullptr;
  unsigned long long *d_counts = nullptr, *d_fill = nullptr;
  auto oom = [&](int code) {
    return undo(ctx->fail(code == PCV_E_HIP ? code : PCV_E_OOM, "xray inpaint: no device memory for " + std::to_string(nc) + " leaves, " + std::to_string(np) +
                                                                    " parents and the work of " + std::to_string(max_e) + " enlarged tiles (" +
                                                                    ctx->last_error + ")"));
  };
  if ((rc = ctx->dev_alloc((void**)&x->d_images, nc * tile_bytes))) return oom(rc);
  if (np && (rc = ctx->dev_alloc((void**)&x->d_parents, np * tile_bytes))) return oom(rc);
  if (x_opened && (rc = sc.get(&d_src, nc * tile_px))) return oom(rc);
  if (d) {
    if ((na && (rc = sc.get(&d_adj, na * tile_px))) || (rc = sc.get(&d_rgba, max_e * big_px)) || (rc = sc.get(&d_known, max_e * big_px)) ||
        (rc = sc.get(&d_ma, max_e * big_px)) || (rc = sc.get(&d_mb, max_e * big_px)) || (rc = sc.get(&d_list, max_e * big_px)) ||
        (rc = sc.get(&d_st, 9 * ne)) || (rc = sc.get(&d_tbl, 9 * nc)) || (rc = sc.get(&d_counts, 3 * nc)) || (rc = sc.get(&d_fill, groups.size())))
      return oom(rc);
  }
  uint64_t opened_tiles = x_opened ? nc : 0;
  for (uint64_t i = 0; i < na; ++i) opened_tiles += neighbours[plan.adjacent[i].first - 1]->kind == kXrayOpened;
  if ((rc = stage.open(opened_tiles))) return undo(rc);

  // ---- sources: x's leaves (in place when they live on the device) and the adjacent leaves -------------------------
  for (uint64_t c = 0; !rc && x_opened && c < nc; ++c) rc = stage.add(xin, c, reinterpret_cast<uint8_t*>(d_src) + c * tile_bytes);
  for (uint64_t i = 0; !rc && i < na; ++i)
    rc = stage.add(neighbours[plan.adjacent[i].first - 1], plan.adjacent[i].second, reinterpret_cast<uint8_t*>(d_adj) + i * tile_bytes);
  if (rc) return undo(rc);
  const uint32_t* src = x_opened ? d_src : xin->d_images;
  auto launched = [&](const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? PCV_OK : ctx->fail(PCV_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  if (d == 0) {
    hipLaunchKernelGGL(xray_inpaint_background_kernel, dim3(grid_for(nc * tile_px, 256)), dim3(256), 0, ctx->stream, src, x->d_images, nc * tile_px, bg);
    if ((rc = launched("xray_inpaint_background_kernel"))) return undo(rc);
  } else {
    if (hipMemcpyAsync(d_st, st.data(), 4 * st.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(d_tbl, tbl.data(), 4 * tbl.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemsetAsync(d_counts, 0, 8 * 3 * nc, ctx->stream) != hipSuccess || hipMemsetAsync(d_fill, 0, 8 * groups.size(), ctx->stream) != hipSuccess)
      return undo(ctx->fail(PCV_E_HIP, "xray inpaint: table upload"));
    for (size_t gi = 0; gi < groups.size(); ++gi) {
      const Group& g = groups[gi];
      const uint64_t quads = g.ecount * big_px / 4, rows = g.ecount * n;
      StitchArgs sa{src, d_adj, (uint32_t)nc, d_st + 9 * g.efirst, d_rgba, d_known, quads, W};
      {
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_STITCH);
        hipLaunchKernelGGL(xray_inpaint_stitch_kernel, dim3(grid_for(quads, 256)), dim3(256), 0, ctx->stream, sa);
      }
      const uint32_t row_grid = grid_for((rows + kRowChunk - 1) / kRowChunk, 1), col_grid = grid_for(g.ecount * (n / 4), 256);
      {  // dilate: rows, columns
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_ROWS);
        hipLaunchKernelGGL(xray_inpaint_row_kernel, dim3(row_grid), dim3(64), 0, ctx->stream, d_known, d_ma, rows, n, d, 0);
      }
      {
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_COLS);
        hipLaunchKernelGGL(xray_inpaint_col_kernel, dim3(col_grid), dim3(256), 0, ctx->stream, d_ma, d_mb, (const uint8_t*)nullptr, g.ecount, n, d, 0);
      }
      {  // erode: rows, columns; the last pass leaves closed & !known
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_ROWS);
        hipLaunchKernelGGL(xray_inpaint_row_kernel, dim3(row_grid), dim3(64), 0, ctx->stream, d_mb, d_ma, rows, n, d, 1);
      }
      {
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_COLS);
        hipLaunchKernelGGL(xray_inpaint_col_kernel, dim3(col_grid), dim3(256), 0, ctx->stream, d_ma, d_mb, (const uint8_t*)d_known, g.ecount, n, d, 1);
      }
      {
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_LIST);
        hipLaunchKernelGGL(xray_inpaint_list_kernel, dim3(grid_for(quads, 256)), dim3(256), 0, ctx->stream, d_mb, quads, d_list, d_fill + gi);
      }
      {
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_FILL);
        hipLaunchKernelGGL(xray_inpaint_fill_kernel, dim3(grid_for(g.ecount * big_px / 16, 256)), dim3(256), 0, ctx->stream, d_rgba, d_known, d_list,
                           d_fill + gi, n, d);
      }
      BlendArgs ba{d_rgba, d_known, d_mb, d_tbl + 9 * g.first, x->d_images + g.first * tile_px, d_counts + 3 * g.first, W, bg,
                   (uint32_t)((tile_px + 255) / 256)};
      {
        PcvProf prof(ctx, PCV_K_XRAY_INPAINT_BLEND);
        hipLaunchKernelGGL(xray_inpaint_blend_kernel, dim3((uint32_t)(g.count * ba.blocks_per_leaf)), dim3(256), 0, ctx->stream, ba);
      }
      if ((rc = launched("xray inpaint kernels"))) return undo(rc);
    }
    std::vector<unsigned long long> counts(3 * nc);
    if (hipMemcpyAsync(counts.data(), d_counts, 8 * counts.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
      return undo(ctx->fail(PCV_E_HIP, "xray inpaint: kernels failed"));
    for (uint64_t c = 0; c < nc; ++c) {
      x->inpaint_target[c] = counts[3 * c];
      x->inpaint_filled[c] = counts[3 * c + 1];
      x->inpaint_blended[c] = counts[3 * c + 2];
    }
  }
  // create_non_leaf_nodes up to x's root, into the images allocated above (returns after a stream sync)
  XrayLevels lv;
  if ((rc = xray_build_levels(ctx, W, bg, plan.leaf, plan.deepest, plan.root_level, x->d_images, PCV_K_XRAY_PARENT, x->d_parents, &lv))) return undo(rc);
  if (np == 0 && hipStreamSynchronize(ctx->stream) != hipSuccess) return undo(ctx->fail(PCV_E_HIP, "xray inpaint: kernels failed"));
  stage.close();
  x->parent_level.swap(lv.plevel);
  x->parent_index.swap(lv.pindex);
  x->level_first.swap(lv.first);
  finish_nodes();
  ctx->prof_resolve();
  *out = x;
  return PCV_OK;
}

extern "C" int pcv_xray_inpaint_info(const pcv_xray* x, uint64_t* target_pixels, uint64_t* filled_pixels, uint64_t* blended_pixels) {
  if (!x) return PCV_E_INVALID;
  if (x->kind != kXrayInpainted) return xray_fail(x, PCV_E_INVALID, "xray: pcv_xray_inpaint_info needs the result of pcv_xray_inpaint");
  const uint64_t bytes = 8 * x->created.size();
  if (target_pixels) std::memcpy(target_pixels, x->inpaint_target.data(), bytes);
  if (filled_pixels) std::memcpy(filled_pixels, x->inpaint_filled.data(), bytes);
  if (blended_pixels) std::memcpy(blended_pixels, x->inpaint_blended.data(), bytes);
  return PCV_OK;
}
