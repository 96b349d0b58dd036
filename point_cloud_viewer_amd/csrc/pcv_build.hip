// pcv_build.hip — host orchestration of the device-resident octree build behind the C ABI (include/pcv_hip.h).
//
// Replaces build_octree (reference src/octree/generation.rs:289-403). The reference streams every point
// through one file per node per level; here the tree is derived from a stable sort of chain-exact path keys:
//
//   K1 aabb_reduce (optional)            find_bounding_box                   generation.rs:256-270
//   K2 chain_keys                        per-level octant digits             generation.rs:78-83 + codec.rs
//   K3 sort keys                         (groups points by path)             generation.rs:84-101
//   K4 node_split                        should_split_node / recursion       generation.rs:110-193
//   host: node table finalize            counts of the promotion pyramid     generation.rs:195-253 (closed form)
//   K5 leaf_encode                       leaf-level quantisation             node_writer.rs:281-316
//   K3 sort records by leaf rank         stable => per-node input order      SURVEY F11
//   K6 promote_encode                    every-8th promotion + rewrites      generation.rs:222-238
//
// Everything between the first and last kernel stays in HBM; the only host round trip is the (small) node
// table. No CPU fallback exists: if HIP fails the call fails.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pcv_build_state.h"
#include "pcv_internal.h"
#include "pcv_spec.h"
#include "pcv_tables.h"

// ------------------------------------------------------------------------------------------------
// input staging
// ------------------------------------------------------------------------------------------------
int pcv_validate_points(pcv_ctx* ctx, const pcv_points* p, bool need_color) {
  if (!p) return ctx->fail(PCV_E_INVALID, "points is null");
  if (p->mem != PCV_MEM_HOST && p->mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "points.mem must be PCV_MEM_HOST or PCV_MEM_DEVICE");
  if (p->n >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "at most 2^32 - 2 points per call");
  if (p->n > 0 && (!p->x || !p->y || !p->z)) return ctx->fail(PCV_E_INVALID, "x/y/z must be non-null");
  if (need_color) {
    if (p->n > 0 && !p->color) return ctx->fail(PCV_E_INVALID, "color is required (on_disk.rs:20-22: colour is always present)");
    if (p->color_stride != 3 && p->color_stride != 4) return ctx->fail(PCV_E_INVALID, "color_stride must be 3 or 4");
  }
  return PCV_OK;
}

int pcv_stage_points(pcv_ctx* ctx, PcvScratch& sc, const pcv_points* p, bool with_attrs, DevPoints* d) {
  d->n = p->n;
  d->color_stride = p->color_stride;
  if (p->mem == PCV_MEM_DEVICE || p->n == 0) {
    d->x = p->x;
    d->y = p->y;
    d->z = p->z;
    d->color = p->color;
    d->intensity = p->intensity;
    return PCV_OK;
  }
  double *x, *y, *z;
  int rc;
  if ((rc = sc.get(&x, p->n)) || (rc = sc.get(&y, p->n)) || (rc = sc.get(&z, p->n))) return rc;
  if ((rc = ctx->h2d(x, p->x, p->n * 8)) || (rc = ctx->h2d(y, p->y, p->n * 8)) || (rc = ctx->h2d(z, p->z, p->n * 8))) return rc;
  d->x = x;
  d->y = y;
  d->z = z;
  if (with_attrs) {
    uint8_t* c;
    if ((rc = sc.get(&c, p->n * p->color_stride))) return rc;
    if ((rc = ctx->h2d(c, p->color, p->n * p->color_stride))) return rc;
    d->color = c;
    if (p->intensity) {
      float* f;
      if ((rc = sc.get(&f, p->n))) return rc;
      if ((rc = ctx->h2d(f, p->intensity, p->n * 4))) return rc;
      d->intensity = f;
    }
  }
  return PCV_OK;
}

// K1 in two halves, so that the caller can do host work (allocations) while the reduction runs.
// The final kernel stores the six doubles straight into the pinned mailbox (host memory the device can write), which holds a
// sentinel until then: the host polls the mailbox instead of waiting for the stream — the blocked wait of a stream synchronize
// wakes up 20-30 us after a 0.4 ms kernel has ended, the poll sees the stores within a few.
static const uint64_t kAabbSentinel = 0x7ff8dead0badbeefull;  // a NaN no fmin / fmax reduction of the kernel can produce
int pcv_device_aabb_launch(pcv_ctx* ctx, PcvScratch& sc, const DevPoints& d) {
  double* partial;
  int rc = sc.get(&partial, (size_t)2048 * 6 + 6);
  if (rc) return rc;
  for (int a = 0; a < 6; ++a) ctx->mailbox[a] = kAabbSentinel;  // nothing queued on the stream writes these slots before the kernel does
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  double* out6 = (double*)ctx->mailbox_dev;
  // the 16-byte vector loads need aligned bases; fall back to staging when the caller's views are not
  if (((uintptr_t)d.x | (uintptr_t)d.y | (uintptr_t)d.z) & 15) {
    double *x, *y, *z;
    if ((rc = sc.get(&x, d.n)) || (rc = sc.get(&y, d.n)) || (rc = sc.get(&z, d.n))) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(x, d.x, d.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(y, d.y, d.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(z, d.z, d.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    pcv_launch_aabb(ctx, d.n, x, y, z, partial, out6);
  } else {
    pcv_launch_aabb(ctx, d.n, d.x, d.y, d.z, partial, out6);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}
int pcv_device_aabb_wait(pcv_ctx* ctx, double bmin[3], double bmax[3]) {
  volatile uint64_t* box = ctx->mailbox;
  bool seen = false;
  for (uint32_t spin = 0; !seen; ++spin) {
    seen = true;
    for (int a = 0; a < 6; ++a) seen = seen && box[a] != kAabbSentinel;
    // every few thousand reads: is the stream still alive? (a failed launch would never deliver)
    if (!seen && (spin & 0xfff) == 0xfff && hipStreamQuery(ctx->stream) != hipErrorNotReady) break;
  }
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  if (!seen) PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  double h[6];
  std::memcpy(h, ctx->mailbox, sizeof(h));
  for (int a = 0; a < 3; ++a) {
    bmin[a] = h[a];
    bmax[a] = h[3 + a];
  }
  return PCV_OK;
}
int pcv_device_aabb(pcv_ctx* ctx, PcvScratch& sc, const DevPoints& d, double bmin[3], double bmax[3]) {
  if (d.n == 0) {  // Aabb::zero() (generation.rs:269)
    for (int a = 0; a < 3; ++a) bmin[a] = bmax[a] = 0.;
    return PCV_OK;
  }
  int rc = pcv_device_aabb_launch(ctx, sc, d);
  return rc ? rc : pcv_device_aabb_wait(ctx, bmin, bmax);
}

// ------------------------------------------------------------------------------------------------
// the build
// ------------------------------------------------------------------------------------------------
extern "C" int pcv_build_begin(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points,
                               pcv_octree** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  if (!params) return ctx->fail(PCV_E_INVALID, "params is null");
  int rc = pcv_validate_points(ctx, points, true);
  if (rc) return rc;
  return pcv_build_begin_impl(ctx, params, points, nullptr, out);
}
extern "C" int pcv_build_begin_routed(pcv_ctx* ctx, const pcv_build_params* params, const pcv_routed_points* routed,
                                      pcv_octree** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  if (!params || !routed) return ctx->fail(PCV_E_INVALID, "null argument");
  if (routed->n >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "at most 2^32 - 2 points per call");
  if (routed->n > 0 && (!routed->oct_rgb || !routed->cx || !routed->cy || !routed->cz))
    return ctx->fail(PCV_E_INVALID, "cx, cy, cz and oct_rgb must be non-null");
  if (params->flags & PCV_BUILD_COMPUTE_BBOX) return ctx->fail(PCV_E_INVALID, "routed points need the global bounding box");
  return pcv_build_begin_impl(ctx, params, nullptr, routed, out);
}

// Scratch for a device node table of n points: capacity for every level down to `deepest`; a level may have up to `max_open`
// open nodes (at most 2^22) as far as the scratch of the two-levels-per-launch kernels goes.
int pcv_alloc_node_table(PcvScratch& sc, uint64_t n, uint32_t max_points, int deepest, uint64_t max_open, PcvNodeTableDev* out) {
  int rc;
  PcvNodeTableDev& nt = *out;
  uint64_t cap64 = 8ull * (uint64_t)(deepest + 1) * (n / max_points + 1) + 64;
  if (cap64 > (1ull << 26)) cap64 = 1ull << 26;
  const uint32_t cap = (uint32_t)cap64;
  nt.capacity = cap;
  nt.prefix_lo = nullptr;
  if ((rc = sc.get(&nt.prefix, cap)) || (rc = sc.get(&nt.lo, cap)) || (rc = sc.get(&nt.hi, cap)) ||
      (rc = sc.get(&nt.parent, cap)) || (rc = sc.get(&nt.first_child, cap)) || (rc = sc.get(&nt.level, cap)) ||
      (rc = sc.get(&nt.child_mask, cap)) || (rc = sc.get(&nt.open, cap)) ||
      (rc = sc.get(&nt.counters, 64)))
    return rc;
  nt.max_open = (uint32_t)std::min<uint64_t>(max_open, 1u << 22);
  return sc.get(&nt.bounds, std::max((size_t)cap * 9, (size_t)nt.max_open * 85));
}

// Depth speculation of the exact build: full-depth keys of a strided sample (2^18 points), sorted; *levels = the key levels the
// main pass needs if the sample is right (K4 verifies), left alone when that is the full depth.
static int probe_depth(pcv_ctx* ctx, PcvBuild* bs, uint32_t max_points, int full_levels, int* levels) {
  int rc;
  hipStream_t st = ctx->stream;
  const DevPoints& d = bs->d;
  const uint64_t n = bs->n;
  const uint32_t ns = 1u << 18;
  const uint64_t stride = n / ns;
  uint32_t* d_max;
  if ((rc = bs->sc.get(&d_max, 64))) return rc;
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_max, 0, 4, st));
  pcv_launch_chain_keys(ctx, bs->lv, ns, stride, d.x, d.y, d.z, bs->keys_a, false, d.routed);
  bool s_in_a = true;
  // the probe only has to tell depths up to kProbeLevels apart (deeper -> no speculation): sort those digits only
  const int kProbeLevels = 14;
  const int probe_levels = full_levels < kProbeLevels ? full_levels : kProbeLevels;
  if ((rc = pcv_radix_sort_u64(ctx, bs->keys_a, bs->keys_b, ns, 3 * (PCV_MAX_KEY_LEVELS - probe_levels), 3 * PCV_MAX_KEY_LEVELS,
                               nullptr, bs->sort_scratch, &s_in_a)))
    return rc;
  double gapd = 0.6 * (double)max_points * (double)ns / (double)n;
  uint32_t gap = gapd < 1.0 ? 1u : (uint32_t)gapd;
  pcv_launch_depth_probe(ctx, s_in_a ? bs->keys_a : bs->keys_b, ns, gap, d_max);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_max, 4, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const uint32_t shared = *(const uint32_t*)ctx->mailbox;
  // a level-`shared` node is (probably) split -> nodes of level shared + 1 exist -> that many digits are needed;
  // a prefix shared down to the last sorted level says nothing about the levels below it
  int want = (int)shared >= probe_levels ? full_levels : (int)shared + 1;
  if (want < 3) want = 3;
  if (want < full_levels) *levels = want;
  return PCV_OK;
}

// Deep tree: a second key word for levels 22..40 (heavy duplicates in a cube with edge/resolution > 2^21). Rare path, built
// from existing pieces: digits as four 32-bit words, four stable LSD sorts (one per word, least significant first, the other
// three travel as payload planes), then the split with both words.
static int split_deep_tree(pcv_ctx* ctx, PcvBuild* bs, const pcv_build_params* params, uint32_t max_points, int deep_levels,
                           PcvNodeTableDev* nt) {
  int rc;
  PcvScratch& sc = bs->sc;
  const DevPoints& d = bs->d;
  const uint64_t n = bs->n;
  bs->deep = true;
  bs->lv.nlevels = deep_levels;
  uint32_t* W[4][2];
  for (int j = 0; j < 4; ++j)
    for (int sd = 0; sd < 2; ++sd)
      if ((rc = sc.get(&W[j][sd], n))) return rc;
  uint32_t* first[4] = {W[0][0], W[1][0], W[2][0], W[3][0]};
  pcv_launch_chain_keys_deep(ctx, bs->lv, n, d.x, d.y, d.z, d.routed, first);
  int side = 0;
  for (int j = 3; j >= 0; --j) {
    PcvSortPayload pl;
    pl.nwords = 3;
    int w = 0;
    for (int o = 0; o < 4; ++o) {
      if (o == j) continue;
      pl.in[w] = W[o][side];
      pl.out[w] = W[o][1 - side];
      ++w;
    }
    bool in_a = true;
    if ((rc = pcv_radix_sort_u32(ctx, W[j][side], W[j][1 - side], n, 0, 32, &pl, bs->sort_scratch, &in_a))) return rc;
    if (!in_a) side = 1 - side;
  }
  const uint32_t* sorted_words[4] = {W[0][side], W[1][side], W[2][side], W[3][side]};
  pcv_launch_combine_words(ctx, n, sorted_words, bs->keys_a, bs->keys_b);  // keys_a = first word, keys_b = second word
  if ((rc = sc.get(&nt->prefix_lo, nt->capacity))) return rc;
  bs->d_prefix_lo = nt->prefix_lo;
  pcv_launch_node_split(ctx, *nt, bs->keys_a, false, (uint32_t)n, bs->lv, params->resolution, max_points,
                        (params->flags >> 8) & 0xffu, bs->keys_b);
  ctx->stage_end(PCV_STAGE_NODE_SPLIT);
  ctx->stage_begin(PCV_STAGE_TABLE);
  return PCV_OK;
}

// What the node split left in its counters ([0] nodes, [1] bit 0: a node at the last key level would still be split), through
// the pinned mailbox; a full node table is an error here.
static int read_split_counters(pcv_ctx* ctx, const PcvNodeTableDev& nt, uint32_t counters[64]) {
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, nt.counters, 64 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(counters, ctx->mailbox, 64 * sizeof(uint32_t));
  if (counters[1] & 2u) return ctx->fail(PCV_E_OOM, "node table capacity exceeded");
  return PCV_OK;
}

// The tree's node table into the context's pinned block (pcv_tables.h), reserved here for everything pcv_build_finish will put
// behind it: downloaded from the device table, or copied from the true tree the single-chain build derived on the host.
static int stage_node_table(pcv_ctx* ctx, const PcvBuild* bs, const PcvNodeTableDev& nt, const PcvTrueTree* tt) {
  int rc;
  const uint32_t M = bs->M;
  if ((rc = ctx->pinned_reserve(pcv_table_pinned_bytes(M, bs->n, bs->deep)))) return rc;
  const PcvStagedTable tb = pcv_staged_table(ctx->pinned, M, bs->deep);
  if (tt) {
    std::memcpy(tb.prefix, tt->prefix.data(), (size_t)M * 8);
    std::memcpy(tb.lo, tt->lo.data(), (size_t)M * 4);
    std::memcpy(tb.hi, tt->hi.data(), (size_t)M * 4);
    std::memcpy(tb.first_child, tt->first_child.data(), (size_t)M * 4);
    std::memcpy(tb.level, tt->level.data(), (size_t)M);
    std::memcpy(tb.child_mask, tt->child_mask.data(), (size_t)M);
    std::memcpy(tb.open, tt->open.data(), (size_t)M);
    return PCV_OK;
  }
  hipStream_t st = ctx->stream;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.prefix, nt.prefix, (size_t)M * 8, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.lo, nt.lo, (size_t)M * 4, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.hi, nt.hi, (size_t)M * 4, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.first_child, nt.first_child, (size_t)M * 4, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.level, nt.level, (size_t)M, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.child_mask, nt.child_mask, (size_t)M, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.open, nt.open, (size_t)M, hipMemcpyDeviceToHost, st));
  if (bs->deep) PCV_HIP_CHECK(ctx, hipMemcpyAsync(tb.prefix_lo, nt.prefix_lo, (size_t)M * 8, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  return PCV_OK;
}

int pcv_build_begin_impl(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, const pcv_routed_points* routed,
                         pcv_octree** out, const PcvTrueTree* given_tree) {
  int rc;
  if (!(params->resolution > 0.0) || !std::isfinite(params->resolution)) return ctx->fail(PCV_E_INVALID, "resolution must be a positive finite number");
  const uint32_t max_points = params->max_points_per_node ? params->max_points_per_node : PCV_DEFAULT_MAX_POINTS_PER_NODE;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint64_t n = routed ? routed->n : points->n;

  PcvBuild* bs = new PcvBuild(ctx);
  pcv_octree* t = new pcv_octree();
  t->pending = bs;  // owned by the tree from here on
  t->ctx = ctx;
  PcvScratch& sc = bs->sc;
  DevPoints& d = bs->d;
  bs->n = n;
  t->resolution = params->resolution;
  t->has_intensity = (routed ? routed->intensity : points->intensity) != nullptr;
  struct Guard {
    pcv_octree* t;
    ~Guard() {
      if (t) pcv_octree_free(t);
    }
  } guard{t};
  PCV_HIP_CHECK(ctx, hipEventRecord(ctx->ev[0], st));
  // (input placement and box stay inline: they hand on the staged points, the box, both key buffers and the sort scratch, and
  // take three of those while K1 runs — too wide an interface for a function of its own)
  for (bool& on : ctx->stage_on) on = false;
  for (bool& open : ctx->stage_open) open = false;
  ctx->stage_times = bs->stage_times = (params->flags & PCV_BUILD_STAGE_TIMES) != 0;
  ctx->stage_begin(PCV_STAGE_AABB);
  if (routed) {  // device-resident by contract
    d.n = n;
    d.routed.oct = reinterpret_cast<const uint8_t*>(routed->oct_rgb);  // byte 0 of every packed word
    d.routed.oct_stride = 4;
    d.routed.cx = routed->cx;
    d.routed.cy = routed->cy;
    d.routed.cz = routed->cz;
    d.color = reinterpret_cast<const uint8_t*>(routed->oct_rgb) + 1;  // r, g, b follow the digit
    d.color_stride = 4;
    d.intensity = routed->intensity;
  } else if ((rc = pcv_stage_points(ctx, sc, points, true, &d))) {
    return rc;
  }

  double bmin[3], bmax[3];
  if ((params->flags & PCV_BUILD_COMPUTE_BBOX) && n > 0) {
    // K1 is queued; the build's three big scratch blocks are taken from the pool while it runs (the host has nothing else to do
    // for 0.4 ms at 100 M points, and these calls are the slow ones of what follows the box)
    if ((rc = pcv_device_aabb_launch(ctx, sc, d))) return rc;
    // a return while K1 is in flight (a failed allocation below) drains the stream: K1 stores its box into the context's
    // mailbox when it ends, and a retry on this context could take that late store for its own box
    struct DrainK1 {
      pcv_ctx* ctx;
      bool in_flight = true;
      ~DrainK1() {
        if (in_flight) (void)hipStreamSynchronize(ctx->stream);
      }
    } k1{ctx};
    if ((rc = sc.get(&bs->keys_a, n)) || (rc = sc.get(&bs->keys_b, n))) return rc;
    if ((rc = ctx->dev_alloc(&bs->sort_scratch, pcv_sort_scratch_bytes(n)))) return rc;
    sc.ptrs.push_back(bs->sort_scratch);
    k1.in_flight = false;  // the wait itself ends with the box delivered or the stream drained
    if ((rc = pcv_device_aabb_wait(ctx, bmin, bmax))) return rc;
  } else if (params->flags & PCV_BUILD_COMPUTE_BBOX) {
    if ((rc = pcv_device_aabb(ctx, sc, d, bmin, bmax))) return rc;
  } else {
    for (int a = 0; a < 3; ++a) {
      bmin[a] = params->bbox_min[a];
      bmax[a] = params->bbox_max[a];
    }
  }
  for (int a = 0; a < 3; ++a) {
    t->bbox_min[a] = bmin[a];
    t->bbox_max[a] = bmax[a];
  }
  ctx->stage_end(PCV_STAGE_AABB);
  if (n == 0) {  // generation.rs:325-330: no leaves, no finished nodes, meta without nodes
    delete t->pending;
    t->pending = nullptr;
    *out = t;
    guard.t = nullptr;
    return PCV_OK;
  }

  PcvLevels& lv = bs->lv;
  int max_level = 0;
  pcv_make_levels(bmin, bmax, params->resolution, 64, &lv, &max_level, nullptr, nullptr);
  if (routed && (lv.nlevels < 1 || lv.enc[1] != PCV_ENC_FLOAT32))
    return ctx->fail(PCV_E_INVALID, "routed points carry Float32 level-1 codes, but level 1 of this cube is not Float32-encoded");

  ctx->stage_begin(PCV_STAGE_CHAIN_KEYS);
  // ---- K2 keys, K3 sort, K4 node split — with depth speculation ----
  // The keys only have to cover the levels the tree really uses. A strided sample (2^18 points) gets full-depth
  // keys, is sorted, and depth_probe measures the deepest prefix still shared by sample keys `gap` apart
  // (gap = 0.6 x the sample-scaled node capacity, i.e. biased towards deeper). The main pass then computes and
  // sorts only that many levels (+1), with 32-bit keys when 10 levels suffice. K4 verifies: if any node at the last
  // key level would still have to be split, everything is redone at full depth — speculation can cost time, never
  // correctness.
  uint64_t*& keys_a = bs->keys_a;
  uint64_t*& keys_b = bs->keys_b;
  void*& sort_scratch = bs->sort_scratch;
  if (!keys_a) {  // (taken while K1 ran when the build computes its own box)
    if ((rc = sc.get(&keys_a, n)) || (rc = sc.get(&keys_b, n))) return rc;
    if ((rc = ctx->dev_alloc(&sort_scratch, pcv_sort_scratch_bytes(n)))) return rc;
    sc.ptrs.push_back(sort_scratch);
  }
  const int full_levels = lv.nlevels;
  int spec_levels = full_levels;

  // device node table (the sample tree of the single-chain build, the tree itself in the exact build)
  PcvNodeTableDev nt;
  // every level down to max_level (incl. the deep retry); the sample tree of the single-chain build splits at a LOWERED
  // threshold: twice the open nodes the capacity allows
  if ((rc = pcv_alloc_node_table(sc, n, max_points, max_level < PCV_MAX_LEVELS ? max_level : PCV_MAX_LEVELS,
                                 2 * (n / max_points + 1) + 64, &nt)))
    return rc;
  uint32_t counters[64];
  bool keys32 = false;
  int attempts = 0;

  // ---- single-chain build (pcv_spec.h): ONE chain pass, topology from a sample + exact per-leaf counts ----
  bool spec_used = false;
  PcvTrueTree true_tree;
  if (given_tree) {  // pcv_gather_encode: the topology is an input; K5 / K6 run on it as they do after K4
    true_tree = *given_tree;
    spec_used = true;
    counters[0] = (uint32_t)true_tree.prefix.size();
    ctx->stage_begin(PCV_STAGE_TABLE);
  } else {
    bool wide_level = false;  // a Float64-encoded level needs the high code words: left to the exact pipeline
    for (int k = 0; k <= full_levels; ++k) wide_level = wide_level || lv.enc[k] == PCV_ENC_FLOAT64;
    const bool forced = (params->flags & PCV_BUILD_FORCE_SINGLE_CHAIN) != 0;
    const bool want = !(params->flags & (PCV_BUILD_NO_SPECULATION | PCV_BUILD_NO_SINGLE_CHAIN)) && (forced || n >= (1ull << 22));
    if (want && !wide_level && full_levels >= 1) {
      if ((rc = pcv_single_chain_topology(ctx, bs, t, params, max_points, full_levels, nt, &true_tree, &spec_used))) return rc;
      if (spec_used) counters[0] = (uint32_t)true_tree.prefix.size();
      else ++attempts;  // the prediction was too shallow somewhere: the exact pipeline redoes the build
    }
  }

  if (!spec_used && n >= (1ull << 22) && full_levels > 4 && !(params->flags & PCV_BUILD_NO_SPECULATION) &&
      (rc = probe_depth(ctx, bs, max_points, full_levels, &spec_levels)))
    return rc;

  for (; !spec_used;) {
    ++attempts;
    lv.nlevels = spec_levels;
    keys32 = spec_levels <= 10;
    pcv_launch_chain_keys(ctx, lv, n, 1, d.x, d.y, d.z, keys_a, keys32, d.routed);
    ctx->stage_end(PCV_STAGE_CHAIN_KEYS);
    ctx->stage_begin(PCV_STAGE_SORT_KEYS);
    bool in_a = true;
    if (keys32)
      rc = pcv_radix_sort_u32(ctx, (uint32_t*)keys_a, (uint32_t*)keys_b, n, 3 * (10 - spec_levels), 30, nullptr,
                              sort_scratch, &in_a);
    else
      rc = pcv_radix_sort_u64(ctx, keys_a, keys_b, n, 3 * (PCV_MAX_KEY_LEVELS - spec_levels), 3 * PCV_MAX_KEY_LEVELS,
                              nullptr, sort_scratch, &in_a);
    if (rc) return rc;
    const void* sorted_keys = in_a ? (const void*)keys_a : (const void*)keys_b;
    ctx->stage_end(PCV_STAGE_SORT_KEYS);
    ctx->stage_begin(PCV_STAGE_NODE_SPLIT);

    // K4: every open node holds > max_points points and open nodes of one level are disjoint
    pcv_launch_node_split(ctx, nt, sorted_keys, keys32, (uint32_t)n, lv, params->resolution, max_points,
                          (params->flags >> 8) & 0xffu);
    ctx->stage_end(PCV_STAGE_NODE_SPLIT);
    ctx->stage_begin(PCV_STAGE_TABLE);

    if ((rc = read_split_counters(ctx, nt, counters))) return rc;
    if (counters[1] & 1u) {
      if (spec_levels < full_levels) {  // speculation too shallow: redo at full depth
        spec_levels = full_levels;
        continue;
      }
      if (max_level > PCV_MAX_KEY_LEVELS) {
        ++attempts;  // deep tree: a second key word for levels 22..40
        const int deep_levels = max_level < PCV_MAX_LEVELS ? max_level : PCV_MAX_LEVELS;
        if ((rc = split_deep_tree(ctx, bs, params, max_points, deep_levels, &nt))) return rc;
        if ((rc = read_split_counters(ctx, nt, counters))) return rc;
        if (!(counters[1] & 1u)) {
          spec_levels = deep_levels;
          break;
        }
      }
      return ctx->fail(PCV_E_DEPTH, "a node at level " + std::to_string(lv.nlevels) +
                                        " still holds more than max_points_per_node points and is larger than the "
                                        "resolution; the reference's NodeId cannot name deeper nodes either");
    }
    break;
  }
  t->key_levels = spec_levels;
  t->key_attempts = attempts;
  bs->levels = bs->deep ? lv.nlevels : full_levels;
  lv.nlevels = bs->levels;  // K5/K6 index the level tables by node level; the walk stops at leaves anyway
  const uint32_t M = counters[0];
  bs->M = M;
  if ((rc = stage_node_table(ctx, bs, nt, spec_used ? &true_tree : nullptr))) return rc;
  bs->pre.resize(M);
  pcv_table_stream_lengths(pcv_staged_table(ctx->pinned, M, bs->deep), bs->pre.data());
  *out = t;
  guard.t = nullptr;
  return PCV_OK;
}

extern "C" int pcv_build_top_streams(const pcv_octree* t, pcv_top_streams* out) {
  if (!t || !out) return PCV_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  const PcvBuild* bs = t->pending;
  if (!bs) return t->nodes.empty() ? PCV_OK : t->ctx->fail(PCV_E_INVALID, "pcv_build_top_streams needs a tree between pcv_build_begin and pcv_build_finish");
  pcv_table_top_streams(pcv_staged_table(t->ctx->pinned, bs->M, bs->deep), bs->pre.data(), out);  // the table staged by pcv_build_begin
  return PCV_OK;
}

// The node-contiguous blobs K6 writes. Global-size top nodes (multi-GPU build: the first top_nodes nodes) are only partly
// filled by this rank: the rest must read as zero.
static int alloc_blobs(pcv_ctx* ctx, pcv_octree* t, const PcvStagedTable& tb, uint32_t top_nodes) {
  int rc;
  void *bx, *br, *bi = nullptr;
  if ((rc = ctx->dev_alloc(&bx, t->xyz_bytes))) return rc;
  t->d_xyz = (uint8_t*)bx;
  if ((rc = ctx->dev_alloc(&br, t->rgb_bytes))) return rc;
  t->d_rgb = (uint8_t*)br;
  if (t->has_intensity) {
    if ((rc = ctx->dev_alloc(&bi, t->int_bytes))) return rc;
    t->d_int = (uint8_t*)bi;
  }
  if (top_nodes) {
    const uint64_t tx = top_nodes < tb.M ? tb.xyz_off[top_nodes] : t->xyz_bytes;
    const uint64_t tp = top_nodes < tb.M ? tb.point_off[top_nodes] : t->num_points;
    if (tx) PCV_HIP_CHECK(ctx, hipMemsetAsync(t->d_xyz, 0, tx, ctx->stream));
    if (tp) PCV_HIP_CHECK(ctx, hipMemsetAsync(t->d_rgb, 0, tp * 3, ctx->stream));
    if (tp && t->d_int) PCV_HIP_CHECK(ctx, hipMemsetAsync(t->d_int, 0, tp * 4, ctx->stream));
  }
  return PCV_OK;
}

// Where `settle` leaves the compact climber records for `climb`: in the payload buffer the sort left unused
// (32 B x n / 8 < 16 B x n) unless that buffer is taken or too small.
static int place_climbers(pcv_ctx* ctx, PcvBuild* bs, const pcv_octree* t, bool fuse_sort, uint64_t num_climbers, void** out) {
  int rc;
  const uint64_t n = bs->n;
  void* climbers = bs->rec_in_a ? bs->pay_b : bs->pay_a;
  if (fuse_sort) {  // that buffer is the held-back pass's SOURCE: the (16-byte) climbers go to the free half of a key buffer — with
                    // an intensity plane that half carries the plane, and the (32-byte) climbers get a block of their own
    const size_t half = ((size_t)n * 4 + 15) & ~(size_t)15;
    climbers = (void*)((uint8_t*)(bs->rec_in_a ? bs->keys_b : bs->keys_a) + half);
    const size_t need = t->has_intensity ? pcv_climber_bytes(num_climbers) : (size_t)(num_climbers + 1) * 16;
    if (t->has_intensity || half + need > (uint64_t)n * 8) {
      if ((rc = ctx->dev_alloc(&climbers, need))) return rc;
      bs->sc.ptrs.push_back(climbers);
    }
  } else if (pcv_climber_bytes(num_climbers) > (size_t)n * (bs->spec_wide ? 8 : 16)) {
    if ((rc = ctx->dev_alloc(&climbers, pcv_climber_bytes(num_climbers)))) return rc;
    bs->sc.ptrs.push_back(climbers);
  }
  *out = climbers;
  return PCV_OK;
}

// single-chain build: the record sort ran on the device's rank map, the node tables come from the host's resolve. Both apply
// the same integer rules to the same counts, so a difference is a bug — reported. Call with the stream drained.
static int check_device_resolve(pcv_ctx* ctx, const PcvBuild* bs) {
  if (!bs->spec || !bs->resolve_on_device) return PCV_OK;
  uint32_t dev[2];
  std::memcpy(dev, ctx->mailbox + kPcvMailboxResolve, sizeof(dev));
  if (dev[0] == 0xffffffffu && dev[1] == 0xffffffffu)  // the sentinel: the resolve kernel never delivered a verdict
    return ctx->fail(PCV_E_HIP, "single-chain build: the device's resolve kernel wrote no verdict");
  bool same = dev[0] == bs->resolve_host_leaves && dev[1] == 0u;
  if (same && bs->resolve_check_map && !bs->resolve_host_map.empty()) {
    std::vector<uint32_t> dm(bs->resolve_host_map.size());
    PCV_HIP_CHECK(ctx, hipMemcpy(dm.data(), bs->spec_map_dev, dm.size() * 4, hipMemcpyDeviceToHost));
    for (size_t k = 0; same && k < dm.size(); ++k) same = bs->resolve_host_inner[k] || dm[k] == bs->resolve_host_map[k];
  }
  if (!same) return ctx->fail(PCV_E_HIP, "single-chain build: the device's resolve of the predicted tree disagrees with the host's");
  return PCV_OK;
}

extern "C" int pcv_build_finish(pcv_octree* t, const pcv_top_layout* top) {
  if (!t) return PCV_E_INVALID;
  PcvBuild* bs = t->pending;
  if (!bs) return t->nodes.empty() && t->num_points == 0 ? PCV_OK : t->ctx->fail(PCV_E_INVALID, "pcv_build_finish: nothing pending");
  pcv_ctx* ctx = t->ctx;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int rc;
  struct Done {  // the build state is released on every exit path; on failure the tree stays valid but empty
    pcv_octree* t;
    ~Done() {
      delete t->pending;
      t->pending = nullptr;
    }
  } done{t};
  PcvLevels& lv = bs->lv;
  const uint64_t n = bs->n;
  const uint32_t M = bs->M;
  ctx->stage_times = bs->stage_times;  // the flag of this build, whatever the context has begun since

  uint64_t* keys_a = bs->keys_a;
  uint64_t* keys_b = bs->keys_b;
  std::vector<uint64_t>& pre = bs->pre;
  const PcvStagedTable tb = pcv_staged_table(ctx->pinned, M, bs->deep);  // the node table staged by pcv_build_begin
  // nodes of level <= 1 hold GLOBAL streams when a layout is given (multi-GPU build)
  const uint32_t top_nodes = top ? pcv_table_apply_top_layout(tb, *top, pre.data()) : 0u;
  std::vector<uint32_t> rank_of(M);
  bool wide = false;
  const uint32_t num_leaves = pcv_table_leaf_order(tb, lv, rank_of.data(), &wide);
  // The single-chain build queued its record sort as soon as the rank map was on the device (pcv_queue_record_sort): the
  // host work from here to K6 — node tables and their upload — hides behind the two sort passes.
  const int w_int = t->has_intensity ? 0 : -1;
  const int w_hi = wide ? (t->has_intensity ? 1 : 0) : -1;
  PcvWalkTables wt;
  if (bs->spec && !bs->sort_queued) {
    ctx->stage_end(PCV_STAGE_TABLE);
    if ((rc = pcv_queue_record_sort(ctx, bs, t, nullptr, num_leaves, wide))) return rc;
  }
  t->nodes.resize(M);
  pcv_table_node_infos(tb, lv, t->bbox_min, pre.data(), rank_of.data(), t->nodes.data(), &t->num_points, &t->xyz_bytes);
  t->rgb_bytes = t->num_points * 3;
  t->int_bytes = t->has_intensity ? t->num_points * 4 : 0;

  // device tables: walk records for K5, 64-byte node / leaf records and the work lists for K6 (pcv_tables.h). settle_by_leaf
  // off: the slot-wise settle kernel and the flat climb launch, experiments
  const bool by_leaf = pcv_switches().settle_by_leaf;
  const bool fuse_sort = bs->spec && bs->sort_second.pending &&
                         pcv_sort_second_settles(bs->sort_second.nbits, bs->sort_second.plane_src != nullptr, t->has_intensity) && by_leaf && !wide && bs->spec_wide;
  const uint32_t num_cont = bs->spec ? (uint32_t)bs->cont_nodes.size() : 0u;
  PcvWorkLists work;
  pcv_table_plan_work(tb, lv, num_leaves, rank_of.data(), by_leaf, fuse_sort, bs->cont_nodes.data(), num_cont, bs->fix_ranges.data(),
                      bs->fix_ranges.size(), &work);
  const PcvRecordBlock rec = pcv_record_block(tb.records, work.counts);
  // (the block cannot grow here: that would free the staged table)
  if ((size_t)(tb.records - (uint8_t*)ctx->pinned) + rec.bytes > ctx->pinned_bytes)
    return ctx->fail(PCV_E_OOM, "node tables: the record block of " + std::to_string(rec.bytes) + " bytes does not fit the pinned reservation");
  pcv_table_fill_records(tb, lv, rank_of.data(), bs->cont_nodes.data(), bs->cont_from.data(), rec, &work);
  const uint32_t num_items = work.counts.num_items, num_citems = by_leaf ? work.counts.num_citems : 0u;
  const uint32_t num_cont_items = work.counts.num_cont_items;
  const uint64_t num_climbers = work.num_climbers;
  // the tables live in a context-owned block; with the record sort already running they go up on the side stream (the
  // copy would otherwise queue behind the sort and sit, with its hand-over, between the sort and K6)
  const size_t walk_bytes = pcv_table_dev_walk_bytes(M);
  if ((rc = ctx->table_dev_reserve(walk_bytes + rec.bytes + 256))) return rc;
  uint8_t* d_up = (uint8_t*)ctx->table_dev;
  const PcvRecordBlock d_rec = pcv_record_block(d_up + walk_bytes, work.counts);
  const bool up_side = bs->spec && bs->sort_queued;
  hipStream_t up_st = up_side ? ctx->side : st;
  if (!bs->spec) PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_up, tb.walk, (size_t)M * 8, hipMemcpyHostToDevice, up_st));  // K5 only
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_rec.node_rec, rec.node_rec, rec.bytes, hipMemcpyHostToDevice, up_st));
  if (up_side && (rc = ctx->side_end())) return ctx->fail(rc, "side stream");
  // (the side stream is in order: this join also covers the layout of the record sort's held-back pass, queued there before the
  // tables — one cross-stream wait in front of that pass instead of two, each ~10 us of idle stream)
  if (up_side) bs->sort_second.join_side = false;
  wt.walk = (const uint64_t*)d_up;
  wt.num_nodes = M;
  PcvPromoteTables pt;
  pt.node_rec = d_rec.node_rec;
  pt.leaf_rec = d_rec.leaf_rec;
  ctx->stage_end(PCV_STAGE_TABLE);  // single-chain build: what is left of the table work once the sort has drained

  if (!bs->spec && (rc = pcv_queue_record_sort(ctx, bs, t, &wt, num_leaves, wide))) return rc;
  const bool rec_in_a = bs->rec_in_a;
  uint4 *pay_a = (uint4*)bs->pay_a, *pay_b = (uint4*)bs->pay_b;
  PcvSortPayload& pl = bs->pl;
  uint32_t* s_rank = rec_in_a ? (uint32_t*)keys_a : (uint32_t*)keys_b;
  const void* s_pay = rec_in_a ? (const void*)pay_a : (const void*)pay_b;
  uint32_t** s_plane = rec_in_a ? pl.in : pl.out;
  ctx->stage_begin(PCV_STAGE_PROMOTE_ENCODE);

  // ---- K6 promotion + final encode into node-contiguous blobs ----
  if ((rc = alloc_blobs(ctx, t, tb, top_nodes))) return rc;
  void* climbers = nullptr;
  if ((rc = place_climbers(ctx, bs, t, fuse_sort, num_climbers, &climbers))) return rc;
  t->settled_in_sort = work.settled_points;
  if (bs->sort_second.pending) {  // the second pass of the record sort, now that tables and blobs exist
    PcvSortFuse fz;
    fz.leaf_rec = d_rec.leaf_rec;
    fz.leaf_fused = d_rec.fused;
    fz.climb_base = d_rec.climb_base;
    fz.climbers = climbers;
    fz.xyz_blob = t->d_xyz;
    fz.rgb_blob = t->d_rgb;
    fz.inten_blob = t->d_int;
    fz.num_leaves = num_leaves;
    ctx->stage_begin(PCV_STAGE_SORT_SECOND);  // (nested in PROMOTE_ENCODE: the sort's pass is accounted on its own)
    rc = pcv_radix_sort_records_second(ctx, &bs->sort_second, fuse_sort ? &fz : nullptr);
    ctx->stage_end(PCV_STAGE_SORT_SECOND);
    if (rc) return rc;
    if ((rc = pcv_queue_replay(ctx, bs))) return rc;  // (held back with the pass: replayed leaves rewrite their sorted records)
  }
  // leaves below a split first candidate: the leaf-wise settle kernel continues their chain itself (its items name the
  // range); the slot-wise kernel (experiments) gets the codes rewritten by a pass of its own first
  const bool cont_in_settle = by_leaf && num_cont_items > 0;
  if (num_cont_items && !cont_in_settle)
    pcv_launch_spec_continue(ctx, lv, d_rec.cont_ranges, d_rec.cont_items, num_cont_items, (void*)s_pay, bs->spec_wide);
  pcv_launch_promote_encode(ctx, lv, pt, n, s_rank, s_pay, wide ? s_plane[w_hi] : nullptr,
                            wide ? s_plane[w_hi + 1] : nullptr, wide ? s_plane[w_hi + 2] : nullptr,
                            w_int >= 0 ? s_plane[w_int] : nullptr, d_rec.climb_base, (uint32_t)num_climbers, climbers, t->d_xyz,
                            t->d_rgb, t->d_int, bs->spec_wide, by_leaf ? d_rec.items : nullptr, num_items,
                            by_leaf ? d_rec.citems : nullptr, num_citems, cont_in_settle ? d_rec.cont_ranges : nullptr);
  ctx->stage_end(PCV_STAGE_PROMOTE_ENCODE);
  PCV_HIP_CHECK(ctx, hipEventRecord(ctx->ev[8], st));
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if ((rc = check_device_resolve(ctx, bs))) {  // never handed out as an octree
    t->nodes.clear();
    t->num_points = 0;
    return rc;
  }
  ctx->prof_resolve();
  for (int sidx = 0; sidx < PCV_STAGE_TOTAL; ++sidx) {
    t->stage_ms[sidx] = 0.f;
    if (ctx->stage_on[sidx]) (void)hipEventElapsedTime(&t->stage_ms[sidx], ctx->stage_b[sidx], ctx->stage_e[sidx]);
  }
  (void)hipEventElapsedTime(&t->stage_ms[PCV_STAGE_TOTAL], ctx->ev[0], ctx->ev[8]);
  return PCV_OK;
}

extern "C" int pcv_build_octree(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points,
                                pcv_octree** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  pcv_octree* t = nullptr;
  int rc = pcv_build_begin(ctx, params, points, &t);
  if (rc == PCV_OK && (rc = pcv_build_finish(t, nullptr)) != PCV_OK) {
    pcv_octree_free(t);
    t = nullptr;
  }
  *out = t;
  return rc;
}

