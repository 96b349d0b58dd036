// pcv_xray_pyramid.hip — the levels above a set of xray tiles: create_non_leaf_nodes (xray/src/generation.rs:656-682),
// build_node (:726-759), build_parent (:410-450) for the parents of a built quadtree's leaves (pcv_xray.hip) and, behind a
// staging step, for the levels merge_xray_quadtrees puts above the roots of partial quadtrees.
//
//   host   parent sets     parent_id of the level below, from deepest - 1 up to root_level (create_non_leaf_nodes)
//   host   2:1 Lanczos3    the taps of image 0.23.10 imageops::resize(FilterType::Lanczos3) for a square 2W -> W resize,
//                          as DynamicImage::resize reaches it (sample.rs vertical_sample, then horizontal_sample): a
//                          restatement of the pinned crate version, computed once per W with libm's sinf
//   K_xp   xray_parent     per (parent, 32 x 32 output block): the virtual 2W x 2W image of build_parent (children 1, 0,
//                          3, 2 at (0, 0), (0, W), (W, 0), (W, W); a missing child is the background) over the block's
//                          window into LDS, the vertical pass into LDS as f32, the horizontal pass, clamp, round, u8
//
// Every output pixel is a fixed sequence of f32 multiplies and adds (no FMA: -ffp-contract=off), so the images do not
// depend on scheduling and equal a host evaluation of the same sequence bit for bit.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pcv_xray_obj.h"

namespace {

constexpr uint32_t kTaps = 12;        // 2 x support 6: taps of an interior output index
constexpr uint32_t kWin = 2 * (kBlk - 1) + kTaps;  // 74: input rows / columns a 32-pixel output block reads

struct LanczosTap {  // one output index o: input [left, left + count), normalised weights
  uint32_t left, count;
  float w[kTaps];
};

// image::imageops::sample sinc / lanczos3: f32 throughout, sin = libm sinf (what f32::sin calls on linux-gnu)
float sinc_f32(float t) {
  if (t == 0.0f) return 1.0f;
  const float a = t * 3.14159265358979323846264338327950288f;  // f32::consts::PI
  return ::sinf(a) / a;
}
float lanczos3_f32(float x) { return std::fabs(x) < 3.0f ? sinc_f32(x) * sinc_f32(x / 3.0f) : 0.0f; }

// vertical_sample / horizontal_sample's filter table for 2W -> W: ratio 2, support 3 x 2 = 6
void lanczos_taps(uint32_t W, std::vector<LanczosTap>& taps) {
  taps.assign(W, LanczosTap{});
  const float ratio = 2.0f, sratio = 2.0f, support = 3.0f * sratio;
  const int64_t n = 2 * (int64_t)W;
  for (uint32_t o = 0; o < W; ++o) {
    const float c = ((float)o + 0.5f) * ratio;
    const int64_t left = std::min<int64_t>(std::max<int64_t>((int64_t)std::floor(c - support), 0), n - 1);
    const int64_t right = std::min<int64_t>(std::max<int64_t>((int64_t)std::ceil(c + support), left + 1), n);
    const float ci = c - 0.5f;
    LanczosTap& t = taps[o];
    t.left = (uint32_t)left;
    t.count = (uint32_t)(right - left);
    float sum = 0.0f;
    for (int64_t i = left; i < right; ++i) {
      const float w = lanczos3_f32(((float)i - ci) / sratio);
      t.w[i - left] = w;
      sum += w;
    }
    for (uint32_t k = 0; k < t.count; ++k) t.w[k] /= sum;
  }
}

struct XrayParentArgs {
  const uint32_t* leaves;   // created leaf images, node positions [0, nleaves)
  const uint32_t* parents;  // parent images, node positions [nleaves, ...)
  uint64_t nleaves;
  const int64_t* slots;     // 4 per parent of the level: node position of child c, -1 where it is missing
  uint32_t* out;            // the level's first parent image
  uint64_t nparents;
  const LanczosTap* taps;   // W entries, rows and columns alike
  uint32_t W, nbx, bg;
};

__device__ __forceinline__ float4 unpack_f4(uint32_t p) {
  return make_float4((float)(p & 255u), (float)((p >> 8) & 255u), (float)((p >> 16) & 255u), (float)(p >> 24));
}
// horizontal_sample's store: clamp(t, 0, 255) then FloatNearest (round half away from zero) as u8
__device__ __forceinline__ uint32_t to_u8_round(float t) {
  t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
  return (uint32_t)roundf(t);
}

// 256 threads per (parent, output block); the grid strides over parents x blocks
__global__ __launch_bounds__(256) void xray_parent_kernel(XrayParentArgs a) {
  __shared__ uint32_t win[kWin * kWin];   // input window of the virtual image, RGBA8
  __shared__ float4 mid[kBlk * kWin];     // vertical pass: block rows x window columns, f32 RGBA
  const uint32_t nblocks = a.nbx * a.nbx;
  const uint64_t total = a.nparents * nblocks;
  const uint32_t W = a.W;
  for (uint64_t b = blockIdx.x; b < total; b += gridDim.x) {
    const uint64_t parent = b / nblocks;
    const uint32_t blk = (uint32_t)(b % nblocks), by = blk / a.nbx, bx = blk % a.nbx;
    const uint32_t oy0 = by * kBlk, ox0 = bx * kBlk;
    const uint32_t oy1 = min(oy0 + kBlk, W), ox1 = min(ox0 + kBlk, W);  // exclusive
    const LanczosTap& ty0 = a.taps[oy0];
    const LanczosTap& ty1 = a.taps[oy1 - 1];
    const LanczosTap& tx0 = a.taps[ox0];
    const LanczosTap& tx1 = a.taps[ox1 - 1];
    const uint32_t row0 = ty0.left, nrow = ty1.left + ty1.count - row0;  // <= kWin: left and right never decrease
    const uint32_t col0 = tx0.left, ncol = tx1.left + tx1.count - col0;
    const int64_t* slot = a.slots + 4 * parent;
    // the window: child pixel or background (build_parent's from_pixel + copy_from)
    for (uint32_t i = threadIdx.x; i < nrow * ncol; i += blockDim.x) {
      const uint32_t vy = row0 + i / ncol, vx = col0 + i % ncol;
      const uint32_t top = vy < W, lft = vx < W;
      const uint32_t child = lft ? (top ? 1u : 0u) : (top ? 3u : 2u);
      const int64_t s = slot[child];
      uint32_t px = a.bg;
      if (s >= 0) {
        const uint32_t* img = (uint64_t)s < a.nleaves ? a.leaves + (uint64_t)s * W * W : a.parents + ((uint64_t)s - a.nleaves) * W * W;
        px = img[(uint64_t)(vy - (top ? 0u : W)) * W + (vx - (lft ? 0u : W))];
      }
      win[(i / ncol) * kWin + i % ncol] = px;
    }
    __syncthreads();
    // vertical pass: t = t + p * w in tap order, f32, neither clamped nor rounded
    for (uint32_t i = threadIdx.x; i < (oy1 - oy0) * ncol; i += blockDim.x) {
      const uint32_t r = i / ncol, c = i % ncol;
      const LanczosTap& t = a.taps[oy0 + r];
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const uint32_t* src = win + (t.left - row0) * kWin + c;
      for (uint32_t k = 0; k < t.count; ++k) {
        const float4 p = unpack_f4(src[k * kWin]);
        const float w = t.w[k];
        acc.x = acc.x + p.x * w;
        acc.y = acc.y + p.y * w;
        acc.z = acc.z + p.z * w;
        acc.w = acc.w + p.w * w;
      }
      mid[r * kWin + c] = acc;
    }
    __syncthreads();
    // horizontal pass over the intermediate, then clamp, round, u8
    uint32_t* out = a.out + parent * W * W;
    for (uint32_t i = threadIdx.x; i < kBlk * kBlk; i += blockDim.x) {
      const uint32_t r = i / kBlk, c = i % kBlk;
      const uint32_t oy = oy0 + r, ox = ox0 + c;
      if (oy >= oy1 || ox >= ox1) continue;
      const LanczosTap& t = a.taps[ox];
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float4* src = mid + r * kWin + (t.left - col0);
      for (uint32_t k = 0; k < t.count; ++k) {
        const float4 p = src[k];
        const float w = t.w[k];
        acc.x = acc.x + p.x * w;
        acc.y = acc.y + p.y * w;
        acc.z = acc.z + p.z * w;
        acc.w = acc.w + p.w * w;
      }
      out[(uint64_t)oy * W + ox] = to_u8_round(acc.x) | to_u8_round(acc.y) << 8 | to_u8_round(acc.z) << 16 | to_u8_round(acc.w) << 24;
    }
    __syncthreads();  // the next block overwrites the window and the intermediate
  }
}

}  // namespace

extern "C" int pcv_xray_lanczos_taps(uint32_t tile_size_px, uint32_t* left, uint32_t* count, float* weights) {
  if (tile_size_px == 0 || tile_size_px > kMaxTilePx) return PCV_E_INVALID;
  std::vector<LanczosTap> taps;
  lanczos_taps(tile_size_px, taps);
  for (uint32_t o = 0; o < tile_size_px; ++o) {
    if (left) left[o] = taps[o].left;
    if (count) count[o] = taps[o].count;
    if (weights)
      for (uint32_t k = 0; k < kTaps; ++k) weights[(uint64_t)o * kTaps + k] = k < taps[o].count ? taps[o].w[k] : 0.0f;
  }
  return PCV_OK;
}

uint64_t xray_count_levels(const std::vector<uint64_t>& base, uint32_t from, uint32_t to) {
  uint64_t n = 0;
  std::vector<uint64_t> below(base);
  for (uint32_t level = from; !below.empty() && level > to; --level) {
    for (uint64_t& i : below) i >>= 2;
    std::sort(below.begin(), below.end());
    below.erase(std::unique(below.begin(), below.end()), below.end());
    n += below.size();
  }
  return n;
}

// the parent levels of a built quadtree (base = the created leaves), the upper levels of a merged one (base = the parts'
// roots) and the parents of an inpainted one (base = its leaves)
int xray_build_levels(pcv_ctx* ctx, uint32_t W, uint32_t bg, const std::vector<uint64_t>& base, uint32_t from, uint32_t to,
                      const uint32_t* d_base, int prof_id, uint32_t* images, XrayLevels* out) {
  const uint64_t nc = base.size();
  std::vector<uint32_t> plevel;
  std::vector<uint64_t> pindex, first;
  // create_non_leaf_nodes: the parent ids of the level below, to ..= from - 1 (ascending index per level)
  std::vector<uint64_t> below(base);
  for (uint32_t level = from; nc && level > to; --level) {
    std::vector<uint64_t> up(below.size());
    for (size_t i = 0; i < below.size(); ++i) up[i] = below[i] >> 2;
    std::sort(up.begin(), up.end());
    up.erase(std::unique(up.begin(), up.end()), up.end());
    first.push_back(pindex.size());
    for (uint64_t i : up) {
      plevel.push_back(level - 1);
      pindex.push_back(i);
    }
    below.swap(up);
  }
  first.push_back(pindex.size());
  const uint64_t np = pindex.size();
  if (np == 0) return PCV_OK;
  // child slots: node positions of (index << 2) + c one level down, -1 where that child was not created
  std::vector<std::pair<uint64_t, uint64_t>> leaf_pos(nc);  // (leaf index, node position)
  for (uint64_t c = 0; c < nc; ++c) leaf_pos[c] = {base[c], c};
  std::sort(leaf_pos.begin(), leaf_pos.end());
  std::vector<int64_t> slots(4 * np, -1);
  for (size_t k = 0; k + 1 < first.size(); ++k) {
    for (uint64_t p = first[k]; p < first[k + 1]; ++p)
      for (uint64_t c = 0; c < 4; ++c) {
        const uint64_t child = (pindex[p] << 2) + c;
        if (k == 0) {
          auto it = std::lower_bound(leaf_pos.begin(), leaf_pos.end(), std::make_pair(child, (uint64_t)0));
          if (it != leaf_pos.end() && it->first == child) slots[4 * p + c] = (int64_t)it->second;
        } else {
          auto b = pindex.begin() + (ptrdiff_t)first[k - 1], e = pindex.begin() + (ptrdiff_t)first[k];
          auto it = std::lower_bound(b, e, child);
          if (it != e && *it == child) slots[4 * p + c] = (int64_t)(nc + (uint64_t)(it - pindex.begin()));
        }
      }
  }
  std::vector<LanczosTap> taps;
  lanczos_taps(W, taps);
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int rc;
  uint32_t* d_parents = images;
  if (!images && (rc = ctx->dev_alloc((void**)&d_parents, 4ull * W * W * np)))  // every parent image before any launch
    return ctx->fail(PCV_E_OOM, "xray: no device memory for " + std::to_string(np) + " parent images (" + ctx->last_error + ")");
  PcvScratch sc(ctx);
  int64_t* d_slots;
  LanczosTap* d_taps;
  if ((rc = sc.get(&d_slots, 4 * np)) || (rc = sc.get(&d_taps, W))) {
    if (!images) ctx->dev_free(d_parents);
    return rc;
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_slots, slots.data(), 8 * slots.size(), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_taps, taps.data(), sizeof(LanczosTap) * W, hipMemcpyHostToDevice, ctx->stream));
  int cus = 0, per_cu = 0;
  PCV_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, xray_parent_kernel, 256, 0));
  const uint64_t resident = (uint64_t)std::max(cus, 1) * (uint64_t)std::max(per_cu, 1);
  XrayParentArgs a{};
  a.leaves = d_base;
  a.parents = d_parents;
  a.nleaves = nc;
  a.taps = d_taps;
  a.W = W;
  a.nbx = (W + kBlk - 1) / kBlk;
  a.bg = bg;
  for (size_t k = 0; k + 1 < first.size(); ++k) {  // a level reads the one below: one launch each, in order
    a.slots = d_slots + 4 * first[k];
    a.out = d_parents + first[k] * W * W;
    a.nparents = first[k + 1] - first[k];
    const uint64_t work = a.nparents * a.nbx * a.nbx;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(work, 4 * resident);
    {
      PcvProf prof(ctx, prof_id);
      hipLaunchKernelGGL(xray_parent_kernel, dim3(grid), dim3(256), 0, ctx->stream, a);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(ctx->stream);
      if (!images) ctx->dev_free(d_parents);
      return ctx->fail(PCV_E_HIP, std::string("xray_parent_kernel: ") + hipGetErrorString(e));
    }
  }
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
    if (!images) ctx->dev_free(d_parents);
    return ctx->fail(PCV_E_HIP, "xray: parent levels failed");
  }
  out->d_parents = d_parents;
  out->plevel.swap(plevel);
  out->pindex.swap(pindex);
  out->first.swap(first);
  return PCV_OK;
}

static int xray_build_parents(pcv_xray* x) {
  const uint64_t nc = x->created.size();
  std::vector<uint64_t> leaves(nc);
  for (uint64_t c = 0; c < nc; ++c) leaves[c] = x->geo.index[x->created[c]];
  XrayLevels lv;
  const int rc = xray_build_levels(x->ctx, x->W, x->bg, leaves, x->geo.deepest_level, x->root_level, x->d_images, PCV_K_XRAY_PARENT, nullptr, &lv);
  if (rc) return rc;
  x->d_parents = lv.d_parents;
  x->parent_level.swap(lv.plevel);
  x->parent_index.swap(lv.pindex);
  x->level_first.swap(lv.first);
  return PCV_OK;
}

extern "C" int pcv_xray_build_parents(pcv_xray* x) {
  if (!x) return PCV_E_INVALID;
  if (x->kind != kXrayBuilt) return xray_not_built(x, "pcv_xray_build_parents");
  if (x->parents_built) return PCV_OK;
  const int rc = xray_build_parents(x);
  if (rc) return rc;
  x->parents_built = true;
  x->ctx->prof_resolve();
  return PCV_OK;
}

// ---- merge_xray_quadtrees (xray/src/bin/merge_xray_quadtrees.rs:129-205) ---------------------------------------------
namespace {

struct MergePlan {
  uint32_t L = 0, deepest = 0, W = 0;
  double rect[3] = {0, 0, 0};
  std::vector<int64_t> root_pos;    // per part: position of its root in its own node list, -1 for an empty part
  std::vector<uint64_t> root_index;  // per part: index of its root at level L
};

int merge_plan(pcv_xray* const* parts, uint32_t num_parts, MergePlan* plan, std::string* err) {
  auto bad = [&](const std::string& m) {
    *err = m;
    return PCV_E_INVALID;
  };
  if (num_parts == 0) return bad("No subquadtrees meta files found.");
  if (!parts) return bad("xray merge: null argument");
  struct Root {
    uint32_t level;
    uint64_t index;
  };
  std::vector<Root> roots;
  int first_part = -1;
  plan->root_pos.assign(num_parts, -1);
  plan->root_index.assign(num_parts, 0);
  for (uint32_t k = 0; k < num_parts; ++k) {
    const pcv_xray* x = parts[k];
    if (!x) return bad("xray merge: part " + std::to_string(k) + " is null");
    if (!xray_is_live(x)) return bad("xray merge: part " + std::to_string(k) + " is not a live pcv_xray");
    if (x->kind == kXrayBuilt && !x->parents_built && !x->created.empty() && x->root_level < x->geo.deepest_level)
      return bad("xray merge: the parent levels of part " + std::to_string(k) + " are not built (pcv_xray_build_parents)");
    const uint64_t n = xray_num_nodes(x);
    std::vector<uint32_t> level(n);
    std::vector<uint64_t> index(n);
    pcv_xray_nodes(x, nullptr, n, level.data(), index.data());
    if (n == 0) continue;  // get_root_nodes skips it; it still takes part in the deepest_level and tile_size checks
    uint64_t at = 0, count = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (level[i] < level[at]) at = i, count = 0;
      if (level[i] == level[at]) ++count;
    }
    if (count != 1)
      return bad("xray merge: part " + std::to_string(k) + " has " + std::to_string(count) + " nodes at its minimum level " +
                 std::to_string(level[at]) + ": its root is not defined");
    plan->root_pos[k] = (int64_t)at;
    plan->root_index[k] = index[at];
    roots.push_back(Root{level[at], index[at]});
    if (first_part < 0) first_part = (int)k;
  }
  if (roots.empty()) return bad("All subquadtress are empty.");
  for (size_t a = 0; a < roots.size(); ++a)
    for (size_t b = a + 1; b < roots.size(); ++b)
      if (roots[a].level == roots[b].level && roots[a].index == roots[b].index) return bad("Not all roots are unique.");
  for (const Root& r : roots)
    if (r.level != roots[0].level) return bad("Not all roots have the same level.");
  for (uint32_t k = 1; k < num_parts; ++k)
    if (parts[k]->geo.deepest_level != parts[0]->geo.deepest_level) return bad("Not all meta files have the same deepest level.");
  for (uint32_t k = 1; k < num_parts; ++k)
    if (parts[k]->W != parts[0]->W) return bad("Not all meta files have the same tile size.");
  plan->L = roots[0].level;
  plan->deepest = parts[0]->geo.deepest_level;
  plan->W = parts[0]->W;
  if (plan->L > plan->deepest) return bad("xray merge: the roots' level is above deepest_level");
  // the first root's rect under Node::parent until level 0
  const pcv_xray* x = parts[first_part];
  if (x->kind == kXrayBuilt) built_root_rect(x, plan->rect);
  else std::memcpy(plan->rect, x->geo.rect, sizeof(plan->rect));
  uint64_t idx = roots[0].index;
  for (uint32_t l = plan->L; l > 0; --l, idx >>= 2) {
    const uint32_t ci = (uint32_t)idx & 3u;
    if (ci & 1u) plan->rect[1] -= plan->rect[2];
    if (ci & 2u) plan->rect[0] -= plan->rect[2];
    plan->rect[2] *= 2.0;
  }
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_xray_merge_check(pcv_xray* const* parts, uint32_t num_parts, uint32_t* root_level, double rect[3], char* err,
                                    uint64_t errcap) {
  MergePlan plan;
  std::string m;
  const int rc = merge_plan(parts, num_parts, &plan, &m);
  if (rc) {
    if (err && errcap) std::snprintf(err, errcap, "%s", m.c_str());
    return rc;
  }
  if (root_level) *root_level = plan.L;
  if (rect) std::memcpy(rect, plan.rect, sizeof(plan.rect));
  return PCV_OK;
}

extern "C" int pcv_xray_merge(pcv_ctx* ctx, pcv_xray* const* parts, uint32_t num_parts, uint32_t background, pcv_xray** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (background > PCV_XRAY_BG_TRANSPARENT) return ctx->fail(PCV_E_INVALID, "xray: unknown background");
  MergePlan plan;
  std::string m;
  int rc = merge_plan(parts, num_parts, &plan, &m);
  if (rc) return ctx->fail(rc, m);
  for (uint32_t k = 0; k < num_parts; ++k)
    if (parts[k]->ctx && parts[k]->ctx != ctx) return ctx->fail(PCV_E_INVALID, "xray merge: part " + std::to_string(k) + " belongs to another context");
  const uint32_t W = plan.W;
  const uint64_t tile_bytes = 4ull * W * W;
  pcv_xray* x = new pcv_xray();
  x->ctx = ctx;
  x->kind = kXrayMerged;
  x->W = W;
  x->bg = background == PCV_XRAY_BG_TRANSPARENT ? 0x00ffffffu : 0xffffffffu;
  x->geo.deepest_level = plan.deepest;
  std::memcpy(x->geo.rect, plan.rect, sizeof(plan.rect));
  for (uint32_t k = 0; k < num_parts; ++k) {
    uint64_t n = 0;
    pcv_xray_nodes(parts[k], &n, 0, nullptr, nullptr);
    const uint64_t at = x->node_index.size();
    x->parts.push_back(XrayPartRef{parts[k], parts[k]->serial, at, n});
    x->node_level.resize(at + n);
    x->node_index.resize(at + n);
    pcv_xray_nodes(parts[k], &n, n, x->node_level.data() + at, x->node_index.data() + at);
  }
  // the level array of the roots: those of built parts first (device to device), then those of opened parts (decoded
  // into one pinned block, one upload)
  std::vector<uint32_t> order;
  for (int opened = 0; opened < 2; ++opened)
    for (uint32_t k = 0; k < num_parts; ++k)
      if (plan.root_pos[k] >= 0 && (parts[k]->kind == kXrayOpened) == (opened == 1)) order.push_back(k);
  uint64_t num_opened = 0;
  std::vector<uint64_t> base;
  for (uint32_t k : order) {
    base.push_back(plan.root_index[k]);
    num_opened += parts[k]->kind == kXrayOpened;
  }
  auto undo = [&](int code) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipGetLastError();
    pcv_xray_free(x);
    return code;
  };
  if (plan.L > 0) {
    if (hipSetDevice(ctx->device) != hipSuccess) return undo(ctx->fail(PCV_E_HIP, "hipSetDevice"));
    PcvScratch sc(ctx);
    uint8_t* d_stage = nullptr;
    uint8_t* host = nullptr;
    if ((rc = sc.get(&d_stage, base.size() * tile_bytes)))
      return undo(ctx->fail(PCV_E_OOM, "xray merge: no device memory for " + std::to_string(base.size()) + " root tiles"));
    if (num_opened && (rc = ctx->host_alloc((void**)&host, num_opened * tile_bytes))) return undo(rc);
    const uint64_t num_built = base.size() - num_opened;
    for (uint64_t i = 0; !rc && i < num_opened; ++i) {
      pcv_xray* part = parts[order[num_built + i]];
      rc = opened_node_to_host(part, (uint64_t)plan.root_pos[order[num_built + i]], host + i * tile_bytes);
      if (rc && !part->ctx) ctx->fail(rc, pcv_host_last_error());
    }
    if (!rc) {
      PcvProf prof(ctx, PCV_K_XRAY_MERGE_STAGE);
      for (uint64_t i = 0; !rc && i < num_built; ++i) {
        pcv_xray* part = parts[order[i]];
        if (xray_owns_tiles(part)) {
          rc = queue_node_images(part, (uint64_t)plan.root_pos[order[i]], 1, d_stage + i * tile_bytes, hipMemcpyDeviceToDevice);
        } else {  // a merged part: through its own parts
          rc = xray_node_images(part, (uint64_t)plan.root_pos[order[i]], 1, PCV_MEM_DEVICE, d_stage + i * tile_bytes);
        }
      }
      if (!rc && num_opened &&
          hipMemcpyAsync(d_stage + num_built * tile_bytes, host, num_opened * tile_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = ctx->fail(PCV_E_HIP, "xray merge: root tile upload");
    }
    XrayLevels lv;
    if (!rc)
      rc = xray_build_levels(ctx, W, x->bg, base, plan.L, 0, reinterpret_cast<const uint32_t*>(d_stage), PCV_K_XRAY_MERGE_PARENT, nullptr, &lv);
    else
      (void)hipStreamSynchronize(ctx->stream);
    if (host) ctx->host_release(host);  // the upload has completed: xray_build_levels returns after a stream sync
    if (rc) return undo(rc);
    x->d_parents = lv.d_parents;
    x->parent_level.swap(lv.plevel);
    x->parent_index.swap(lv.pindex);
    x->level_first.swap(lv.first);
    x->node_level.insert(x->node_level.end(), x->parent_level.begin(), x->parent_level.end());
    x->node_index.insert(x->node_index.end(), x->parent_index.begin(), x->parent_index.end());
  }
  x->parents_built = true;
  for (size_t i = 0; i < x->node_index.size(); ++i)
    if (x->node_level[i] == plan.deepest) {
      x->created.push_back(x->geo.index.size());
      x->geo.index.push_back(x->node_index[i]);
    }
  ctx->prof_resolve();
  *out = x;
  return PCV_OK;
}
