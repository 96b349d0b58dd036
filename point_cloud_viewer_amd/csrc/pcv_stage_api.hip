// pcv_stage_api.hip — the stage-level entry points of the build: every stage of pcv_build.hip's K1...K6 map on
// its own, for tests and for callers that hold the intermediate arrays themselves. Host code only.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pcv_build_state.h"
#include "pcv_internal.h"
#include "pcv_sort_records_check.h"
#include "pcv_tables.h"

// ------------------------------------------------------------------------------------------------
// stage-level entry points
// ------------------------------------------------------------------------------------------------
extern "C" int pcv_aabb_reduce(pcv_ctx* ctx, const pcv_points* points, double bbox_min[3], double bbox_max[3]) {
  if (!ctx) return PCV_E_INVALID;
  int rc = pcv_validate_points(ctx, points, false);
  if (rc) return rc;
  if (!bbox_min || !bbox_max) return ctx->fail(PCV_E_INVALID, "null output");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  DevPoints d;
  if ((rc = pcv_stage_points(ctx, sc, points, false, &d))) return rc;
  return pcv_device_aabb(ctx, sc, d, bbox_min, bbox_max);
}

extern "C" int pcv_chain_keys(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, int nlevels,
                              uint64_t* keys) {
  if (!ctx) return PCV_E_INVALID;
  int rc = pcv_validate_points(ctx, points, false);
  if (rc) return rc;
  if (!params || !keys) return ctx->fail(PCV_E_INVALID, "null argument");
  if (!(params->resolution > 0.0)) return ctx->fail(PCV_E_INVALID, "resolution must be positive");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  DevPoints d;
  if ((rc = pcv_stage_points(ctx, sc, points, false, &d))) return rc;
  PcvLevels lv;
  int max_level;
  pcv_make_levels(params->bbox_min, params->bbox_max, params->resolution, 64, &lv, &max_level, nullptr, nullptr);
  if (nlevels > 0 && nlevels < lv.nlevels) lv.nlevels = nlevels;
  if (points->n == 0) return PCV_OK;
  uint64_t* dk = keys;
  if (points->mem == PCV_MEM_HOST && (rc = sc.get(&dk, points->n))) return rc;
  pcv_launch_chain_keys(ctx, lv, points->n, 1, d.x, d.y, d.z, dk, false);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (points->mem == PCV_MEM_HOST)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(keys, dk, points->n * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

template <typename KeyT>
static int sort_api(pcv_ctx* ctx, KeyT* keys, uint32_t* values, uint64_t n, int begin_bit, int end_bit, int mem) {
  if (!ctx) return PCV_E_INVALID;
  if (n == 0) return PCV_OK;
  if (!keys) return ctx->fail(PCV_E_INVALID, "keys is null");
  if (begin_bit < 0 || end_bit > (int)sizeof(KeyT) * 8 || begin_bit > end_bit) return ctx->fail(PCV_E_INVALID, "bad bit range");
  if (n >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "n must be < 2^32 - 1");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  KeyT *a, *b;
  uint32_t *va = nullptr, *vb = nullptr;
  void* scratch;
  int rc;
  if ((rc = sc.get(&a, n)) || (rc = sc.get(&b, n))) return rc;
  if (values && ((rc = sc.get(&va, n)) || (rc = sc.get(&vb, n)))) return rc;
  if ((rc = ctx->dev_alloc(&scratch, pcv_sort_scratch_bytes(n)))) return rc;
  sc.ptrs.push_back(scratch);
  hipMemcpyKind in = mem == PCV_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  hipMemcpyKind outk = mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(a, keys, n * sizeof(KeyT), in, ctx->stream));
  if (values) PCV_HIP_CHECK(ctx, hipMemcpyAsync(va, values, n * 4, in, ctx->stream));
  PcvSortPayload pl;
  pl.nwords = values ? 1 : 0;
  pl.in[0] = va;
  pl.out[0] = vb;
  bool in_a = true;
  if constexpr (sizeof(KeyT) == 8) rc = pcv_radix_sort_u64(ctx, (uint64_t*)a, (uint64_t*)b, n, begin_bit, end_bit, &pl, scratch, &in_a);
  else rc = pcv_radix_sort_u32(ctx, (uint32_t*)a, (uint32_t*)b, n, begin_bit, end_bit, &pl, scratch, &in_a);
  if (rc) return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(keys, in_a ? a : b, n * sizeof(KeyT), outk, ctx->stream));
  if (values) PCV_HIP_CHECK(ctx, hipMemcpyAsync(values, in_a ? va : vb, n * 4, outk, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_sort_keys64(pcv_ctx* ctx, uint64_t* keys, uint64_t n, int begin_bit, int end_bit, int mem) {
  return sort_api<uint64_t>(ctx, keys, nullptr, n, begin_bit, end_bit, mem);
}
extern "C" int pcv_sort_keys32(pcv_ctx* ctx, uint32_t* keys, uint64_t n, int begin_bit, int end_bit, int mem) {
  return sort_api<uint32_t>(ctx, keys, nullptr, n, begin_bit, end_bit, mem);
}
extern "C" int pcv_sort_pairs32(pcv_ctx* ctx, uint32_t* keys, uint32_t* values, uint64_t n, int begin_bit, int end_bit,
                                int mem) {
  if (ctx && !values) return ctx->fail(PCV_E_INVALID, "values is null");
  return sort_api<uint32_t>(ctx, keys, values, n, begin_bit, end_bit, mem);
}

// The build's record sort on the caller's arrays: the payload set up as pcv_queue_record_sort sets it up, the rows counted as
// count_and_queue_sort counts them, the sort and its held-back second pass called as the build calls them. The checks and the
// plan handed back are pcv_sort_records_check.cpp's (host only).
extern "C" int pcv_sort_records(pcv_ctx* ctx, const pcv_sort_records_args* args, pcv_sort_plan_info* plan_out) {
  if (!ctx) return PCV_E_INVALID;
  PcvSortRecordsSwitches sw;
  sw.sort_rows2 = pcv_switches().sort_rows2, sw.sort_msd = pcv_switches().sort_msd, sw.rows_true_bins = pcv_switches().rows_true_bins;
  PcvSortFacts facts;
  PcvSortPlan plan;
  if (const char* why = pcv_sort_records_check(args, sw, &facts, &plan)) return ctx->fail(PCV_E_INVALID, why);
  const pcv_sort_records_args& a = *args;
  const uint64_t n = a.n;
  const bool host = a.mem == PCV_MEM_HOST;
  const bool packed = (a.flags & PCV_SORT_RECORDS_PACKED) != 0;
  if (n && a.map && (a.flags & PCV_SORT_RECORDS_CHECK_KEYS)) {
    std::vector<uint32_t> copy;
    const uint32_t* hk = packed ? (const uint32_t*)a.vec : a.keys;  // (packed: the ranks are in the records)
    const size_t words = packed ? 2 * n : n;
    if (!host) {
      copy.resize(words);
      PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
      PCV_HIP_CHECK(ctx, hipMemcpy(copy.data(), hk, words * 4, hipMemcpyDeviceToHost));
      hk = copy.data();
    }
    if (const char* why = packed ? pcv_sort_records_check_packed(hk, n, a.map_entries) : pcv_sort_records_check_keys(hk, n, a.vec_bytes, a.map_entries))
      return ctx->fail(PCV_E_INVALID, why);
  }
  if (plan_out) pcv_sort_records_plan_info(plan, plan_out);
  if (n == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const hipMemcpyKind outk = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  PcvScratch sc(ctx);
  int rc;
  // a host array on the device in an allocation of its own; a device array is read where it lies
  auto staged = [&](const void* src, size_t bytes, const void** dev) -> int {
    *dev = src;
    if (!host || !src) return PCV_OK;
    uint8_t* d;
    if (int r = sc.get(&d, bytes)) return r;
    if (hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) return ctx->fail(PCV_E_HIP, "pcv_sort_records: upload");
    *dev = d;
    return PCV_OK;
  };
  uint32_t *ka, *kb;
  if ((rc = sc.get(&ka, n)) || (rc = sc.get(&kb, n))) return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ka, a.keys, n * 4, in, st));
  PcvSortPayload pl;
  const size_t vec_bytes = (size_t)a.vec_bytes;
  if (vec_bytes) {
    uint8_t *va, *vb;
    if ((rc = sc.get(&va, n * vec_bytes)) || (rc = sc.get(&vb, n * vec_bytes))) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(va, a.vec, n * vec_bytes, in, st));
    pl.vec_in = va, pl.vec_out = vb, pl.vec_bytes = a.vec_bytes;
  }
  pl.nwords = a.nwords;
  for (int w = 0; w < a.nwords; ++w) {
    if ((rc = sc.get(&pl.in[w], n)) || (rc = sc.get(&pl.out[w], n))) return rc;
    if (w == 0 && a.plane0_in) continue;  // (the first pass reads the caller's array)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(pl.in[w], a.planes[w], n * 4, in, st));
  }
  const void* dev;
  if ((rc = staged(a.plane0_in, n * 4, &dev))) return rc;
  pl.first_in0 = (const uint32_t*)dev;
  if ((rc = staged(a.color_in, n * a.color_stride, &dev))) return rc;
  pl.color_in = (const uint8_t*)dev, pl.color_stride = a.color_in ? a.color_stride : 3;
  pl.packed = packed;
  if ((rc = staged(a.map, (size_t)a.map_entries * 4, &dev))) return rc;
  const uint32_t* map = (const uint32_t*)dev;
  const uint32_t* rows = nullptr;
  const size_t rows_words = (size_t)plan.geom.groups * a.map_entries;
  if (a.rows_mode == PCV_SORT_ROWS_GIVEN) {
    if ((rc = staged(a.rows, rows_words * 4, &dev))) return rc;
    rows = (const uint32_t*)dev;
  } else if (a.rows_mode == PCV_SORT_ROWS_DEVICE) {
    int sgroups;
    uint64_t schunk;
    pcv_sort_rec12_geometry(n, &sgroups, &schunk);
    uint32_t *counted, *counts;
    if ((rc = sc.get(&counted, rows_words)) || (rc = sc.get(&counts, a.map_entries))) return rc;
    PCV_HIP_CHECK(ctx, hipMemsetAsync(counts, 0, (size_t)a.map_entries * 4, st));
    pcv_launch_rank_hist_rows(ctx, ka, n, a.map_entries, counts, packed ? 0 : 8, sgroups, schunk, counted, packed);
    PCV_HIP_CHECK(ctx, hipGetLastError());
    if (a.rows) PCV_HIP_CHECK(ctx, hipMemcpyAsync(a.rows, counted, rows_words * 4, outk, st));
    rows = counted;
  }
  void* scratch;
  if ((rc = ctx->dev_alloc(&scratch, pcv_sort_scratch_bytes(n)))) return rc;
  sc.ptrs.push_back(scratch);
  bool in_a = true;
  PcvSortSecond second;
  if (map) {
    rc = pcv_radix_sort_records_mapped(ctx, ka, kb, n, a.key_bits, &pl, scratch, map, a.map_entries, &in_a, rows,
                                       a.hold_second ? &second : nullptr);
    if (rc == PCV_OK && second.pending) {
      if (plan_out) plan_out->second_ran = 1;
      rc = pcv_radix_sort_records_second(ctx, &second, nullptr);
    }
  } else {
    rc = pcv_radix_sort_u32(ctx, ka, kb, n, facts.begin_bit, facts.end_bit, &pl, scratch, &in_a);
  }
  if (rc) {
    (void)hipStreamSynchronize(st);  // (the arrays of `sc` are released on return)
    return rc;
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(a.keys, in_a ? ka : kb, n * 4, outk, st));
  if (vec_bytes) PCV_HIP_CHECK(ctx, hipMemcpyAsync(a.vec, in_a ? pl.vec_in : pl.vec_out, n * vec_bytes, outk, st));
  for (int w = 0; w < a.nwords; ++w) PCV_HIP_CHECK(ctx, hipMemcpyAsync(a.planes[w], in_a ? pl.in[w] : pl.out[w], n * 4, outk, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  return PCV_OK;
}

extern "C" void pcv_sort_records_geometry(uint64_t n, int32_t* groups, uint64_t* chunk) {
  int g;
  pcv_sort_rec12_geometry(n, &g, chunk);
  *groups = g;
}

// ------------------------------------------------------------------------------------------------
// stage-level entry points of the topology / promotion / encode stages
// ------------------------------------------------------------------------------------------------
extern "C" int pcv_node_split(pcv_ctx* ctx, const pcv_build_params* params, const uint64_t* sorted_keys, uint64_t n, int mem,
                              pcv_split_node* nodes, uint64_t capacity, uint64_t* num_nodes) {
  if (!ctx) return PCV_E_INVALID;
  if (!params || !num_nodes || (capacity && !nodes)) return ctx->fail(PCV_E_INVALID, "null argument");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (!(params->resolution > 0.0)) return ctx->fail(PCV_E_INVALID, "resolution must be positive");
  if (n >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "at most 2^32 - 2 keys per call");
  *num_nodes = 0;
  if (n == 0) return PCV_OK;
  if (!sorted_keys) return ctx->fail(PCV_E_INVALID, "sorted_keys is null");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t max_points = params->max_points_per_node ? params->max_points_per_node : PCV_DEFAULT_MAX_POINTS_PER_NODE;
  PcvLevels lv;
  int max_level = 0;
  pcv_make_levels(params->bbox_min, params->bbox_max, params->resolution, 64, &lv, &max_level, nullptr, nullptr);
  PcvScratch sc(ctx);
  int rc;
  const uint64_t* dk = sorted_keys;
  if (mem == PCV_MEM_HOST) {
    uint64_t* tmp;
    if ((rc = sc.get(&tmp, n))) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(tmp, sorted_keys, n * 8, hipMemcpyHostToDevice, st));
    dk = tmp;
  }
  PcvNodeTableDev nt;  // one key word's levels; the split runs at the capacity itself: as many open nodes as it allows
  if ((rc = pcv_alloc_node_table(sc, n, max_points, lv.nlevels, n / max_points + 64, &nt))) return rc;
  uint8_t* d_pack;
  if ((rc = sc.get(&d_pack, kPcvPackHeader + ((size_t)nt.capacity + 8) * sizeof(PcvPackedNode)))) return rc;
  pcv_launch_node_split(ctx, nt, dk, false, (uint32_t)n, lv, params->resolution, max_points, (params->flags >> 8) & 0xffu);
  pcv_launch_pack_node_table(ctx, nt, d_pack);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_pack, 256, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  uint32_t counters[64];
  std::memcpy(counters, ctx->mailbox, sizeof(counters));
  if (counters[1] & 2u) return ctx->fail(PCV_E_OOM, "node table capacity exceeded");
  if (counters[1] & 1u) return ctx->fail(PCV_E_DEPTH, "a node at the last key level would still have to be split");
  const uint32_t m = counters[0];
  *num_nodes = m;
  std::vector<PcvPackedNode> pk(m);
  if (m) PCV_HIP_CHECK(ctx, hipMemcpy(pk.data(), d_pack + kPcvPackHeader, (size_t)m * sizeof(PcvPackedNode), hipMemcpyDeviceToHost));
  std::vector<uint32_t> parent(m, 0xffffffffu);
  for (uint32_t i = 0; i < m; ++i)
    if (pk[i].open) {
      const uint32_t nchild = (uint32_t)__builtin_popcount(pk[i].child_mask);
      for (uint32_t c = 0; c < nchild; ++c) parent[pk[i].first_child + c] = i;
    }
  for (uint32_t i = 0; i < m && i < capacity; ++i) {
    pcv_split_node& o = nodes[i];
    const int level = pk[i].level;
    const unsigned __int128 index = level ? (unsigned __int128)(pk[i].prefix >> (3 * (PCV_MAX_KEY_LEVELS - level))) : 0;
    o.id_high = ((uint64_t)level << 56) | (uint64_t)(index >> 64);
    o.id_low = (uint64_t)index;
    o.first = pk[i].lo;
    o.count = (uint64_t)pk[i].hi - pk[i].lo;
    o.level = (uint32_t)level;
    o.parent = parent[i];
    o.first_child = pk[i].open ? pk[i].first_child : 0u;
    o.child_mask = pk[i].child_mask;
    o.is_leaf = pk[i].open ? 0u : 1u;
    o.reserved = 0;
  }
  return PCV_OK;
}

extern "C" int pcv_gather_encode(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points,
                                 const pcv_split_node* nodes, uint64_t num_nodes, pcv_octree** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  if (!params) return ctx->fail(PCV_E_INVALID, "params is null");
  int rc = pcv_validate_points(ctx, points, true);
  if (rc) return rc;
  if (params->flags & PCV_BUILD_COMPUTE_BBOX) return ctx->fail(PCV_E_INVALID, "the topology was built for a given bounding box: pass it");
  if (points->n && (!nodes || num_nodes == 0)) return ctx->fail(PCV_E_INVALID, "no topology");
  if (num_nodes > (1ull << 26)) return ctx->fail(PCV_E_INVALID, "too many nodes");
  PcvTrueTree tt;
  const uint32_t m = (uint32_t)num_nodes;
  for (uint32_t i = 0; i < m && points->n; ++i) {
    const pcv_split_node& nd = nodes[i];
    if (nd.level > PCV_MAX_KEY_LEVELS) return ctx->fail(PCV_E_INVALID, "pcv_gather_encode takes trees of up to 21 levels");
    if (nd.first + nd.count > points->n) return ctx->fail(PCV_E_INVALID, "node range outside the points");
    const uint32_t nchild = (uint32_t)__builtin_popcount(nd.child_mask & 0xffu);
    if (!nd.is_leaf && (nchild == 0 || nd.first_child <= i || (uint64_t)nd.first_child + nchild > m))
      return ctx->fail(PCV_E_INVALID, "node table is not breadth first with consecutive children");
    const unsigned __int128 index = ((unsigned __int128)(nd.id_high & 0x00ffffffffffffffull) << 64) | nd.id_low;
    tt.prefix.push_back(nd.level ? (uint64_t)(index << (3 * (PCV_MAX_KEY_LEVELS - nd.level))) : 0ull);
    tt.lo.push_back((uint32_t)nd.first);
    tt.hi.push_back((uint32_t)(nd.first + nd.count));
    tt.first_child.push_back(nd.is_leaf ? 0u : nd.first_child);
    tt.level.push_back((uint8_t)nd.level);
    tt.child_mask.push_back((uint8_t)nd.child_mask);
    tt.open.push_back(nd.is_leaf ? 0 : 1);
  }
  if (points->n && (tt.lo[0] != 0 || tt.hi[0] != points->n || tt.level[0] != 0))
    return ctx->fail(PCV_E_INVALID, "the first node must be the root and span all points");
  pcv_octree* t = nullptr;
  rc = pcv_build_begin_impl(ctx, params, points, nullptr, &t, &tt);
  if (rc == PCV_OK && (rc = pcv_build_finish(t, nullptr)) != PCV_OK) {
    pcv_octree_free(t);
    t = nullptr;
  }
  *out = t;
  return rc;
}
