// pcv_single_chain.hip — the single-chain build's host side (pcv_spec.h): the record sort and the replay it
// queues, and the topology found from a sample in named steps. Host code only: the kernels are in pcv_chain.hip,
// pcv_topology.hip, pcv_sort.hip, pcv_sort_rec12.hip and pcv_encode.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pcv_build_state.h"
#include "pcv_internal.h"
#include "pcv_spec.h"
#include "pcv_tables.h"

// The record sort's second pass settles the leaves' points itself (PcvSortFuse) where it can: the pass is held back until the
// node tables are on the device. Otherwise the sort runs to its end and `settle` reads the records.
static bool pcv_settle_in_sort() { return pcv_switches().settle_in_sort && pcv_switches().settle_by_leaf; }

// K5 (exact pipeline only: `wt` set) + K3 stable record sort by leaf rank, queued on the stream; the outcome is left in
// the build state for K6. num_leaves only sizes the digits: any upper bound of the number of true leaves will do.
// record = rank (u32) + one 16-byte payload {code x, code y, code z, rgba}; optional 4-byte planes for the intensity
// and, when some leaf level is Float64-encoded, the high words of the codes. The key buffers are dead by now: each
// (8n bytes) hosts one rank array; payloads get their own buffers.
int pcv_queue_record_sort(pcv_ctx* ctx, PcvBuild* bs, pcv_octree* t, const PcvWalkTables* wt, uint32_t num_leaves, bool wide) {
  PcvScratch& sc = bs->sc;
  DevPoints& d = bs->d;
  PcvLevels& lv = bs->lv;
  const uint64_t n = bs->n;
  int rc;
  uint32_t* rank_a = (uint32_t*)bs->keys_a;
  uint32_t* rank_b = (uint32_t*)bs->keys_b;
  const bool compact = bs->spec_wide != nullptr;  // 12-byte records: uint2 payloads
  uint4 *pay_a = (uint4*)bs->spec_payload, *pay_b;
  if (compact) {
    uint2* b2;
    if ((rc = sc.get(&b2, n))) return rc;
    pay_b = (uint4*)b2;
  } else if ((!pay_a && (rc = sc.get(&pay_a, n))) || (rc = sc.get(&pay_b, n))) {
    return rc;
  }
  PcvSortPayload& pl = bs->pl;
  pl = PcvSortPayload();
  pl.vec_in = pay_a;
  pl.vec_out = pay_b;
  pl.vec_bytes = compact ? 8 : 16;
  t->record_bytes = compact ? 12 : 20;
  t->packed_handover = 0;
  pl.nwords = (t->has_intensity ? 1 : 0) + (wide ? 3 : 0);
  for (int w = 0; w < pl.nwords; ++w) {
    if (w == 0) {  // first plane fits in the second half of the key buffers
      pl.in[0] = (uint32_t*)bs->keys_a + n;
      pl.out[0] = (uint32_t*)bs->keys_b + n;
    } else if ((rc = sc.get(&pl.in[w], n)) || (rc = sc.get(&pl.out[w], n))) {
      return rc;
    }
  }
  if (bs->spec && t->has_intensity) pl.first_in0 = reinterpret_cast<const uint32_t*>(d.intensity);  // float bits, record order
  const int w_int = t->has_intensity ? 0 : -1;
  const int w_hi = wide ? (t->has_intensity ? 1 : 0) : -1;
  if (!bs->spec) {  // the single-chain build wrote (true-leaf rank, leaf codes, rgb[, intensity]) while it found the topology
    ctx->stage_begin(PCV_STAGE_LEAF_ENCODE);
    pcv_launch_leaf_encode(ctx, lv, *wt, n, d.x, d.y, d.z, d.routed, d.color, d.color_stride, d.intensity, rank_a, pay_a,
                           wide ? pl.in[w_hi] : nullptr, wide ? pl.in[w_hi + 1] : nullptr, wide ? pl.in[w_hi + 2] : nullptr,
                           w_int >= 0 ? pl.in[w_int] : nullptr);
    ctx->stage_end(PCV_STAGE_LEAF_ENCODE);
  }
  ctx->stage_begin(PCV_STAGE_SORT_RECORDS);
  int rank_bits = 1;
  while ((1ull << rank_bits) < num_leaves) ++rank_bits;
  bool rec_in_a = true;
  if (bs->spec && bs->color_late) {
    // the first pass of the rows form reads the colour as it loads the records; any other form of the sort (the rank-count rows
    // did not fit, experiments) gets it joined in place first
    const bool first_pass_joins = bs->spec_map_dev && compact && pl.nwords <= 1 && bs->spec_rows;
    if (first_pass_joins) {
      pl.color_in = d.color;
      pl.color_stride = d.color_stride;
      pl.packed = bs->packed;  // (no plane: the packed hand-over is not tried with an intensity)
      t->packed_handover = bs->packed ? 1 : 0;
    } else if (bs->packed) {
      pcv_launch_unpack_records(ctx, n, d.color, d.color_stride, rank_a, pay_a);
      t->packed_handover = 2;
    } else {
      pcv_launch_join_color(ctx, n, d.color, d.color_stride, rank_a, pay_a);
    }
  }
  if (bs->spec_map_dev)
    rc = pcv_radix_sort_records_mapped(ctx, rank_a, rank_b, n, rank_bits, &pl, bs->sort_scratch, bs->spec_map_dev,
                                       bs->spec_map_entries, &rec_in_a, compact && pl.nwords <= 1 ? bs->spec_rows : nullptr,
                                       compact && pl.nwords <= 1 && !wide && pcv_settle_in_sort() ? &bs->sort_second : nullptr);
  else
    rc = pcv_radix_sort_u32(ctx, rank_a, rank_b, n, 0, rank_bits, &pl, bs->sort_scratch, &rec_in_a);
  if (rc) return rc;
  ctx->stage_end(PCV_STAGE_SORT_RECORDS);
  bs->sort_queued = true;
  bs->rec_in_a = rec_in_a;
  bs->pay_a = pay_a;
  bs->pay_b = pay_b;
  return PCV_OK;
}

// single-chain build: the few leaves whose records hold no usable codes (bs->fix_ranges, PCV_SPEC_MAP_REPLAY) replay their
// chain from the coordinates now that the record sort has made them contiguous; queued behind the sort.
int pcv_queue_replay(pcv_ctx* ctx, PcvBuild* bs) {
  if (!bs->spec || bs->fix_ranges.empty()) return PCV_OK;
  hipStream_t st = ctx->stream;
  DevPoints& d = bs->d;
  int rc;
  const void* s_pay = bs->rec_in_a ? (const void*)bs->pay_a : (const void*)bs->pay_b;
  const uint32_t nr = (uint32_t)bs->fix_ranges.size();
  uint32_t* d_ranges;
  if ((rc = bs->sc.get(&d_ranges, (size_t)nr * 4 + 4))) return rc;
  // staging: the second half of the pinned mailbox block is reserved for these ranges (kMaxMailboxRanges of them) — the upload is
  // queued behind the record sort and the caller gets control back before it has run, so the slot must not be one that
  // other entry points of the context write (they use the first half); more ranges (tiny capacities in tests) wait
  // for the queued work and take the big block
  constexpr uint32_t kMaxMailboxRanges = (kPcvMailboxResolve - kPcvMailboxReplay) * sizeof(uint64_t) / 16;  // 16 bytes per range
  uint32_t* h_ranges = (uint32_t*)(ctx->mailbox + kPcvMailboxReplay);
  if (nr > kMaxMailboxRanges) {
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if ((rc = ctx->pinned_spec_reserve((size_t)nr * 16 + 64))) return rc;
    h_ranges = (uint32_t*)ctx->pinned_spec;
  }
  uint32_t before = 0;
  for (uint32_t k = 0; k < nr; ++k) {
    h_ranges[4 * k + 0] = bs->fix_ranges[k].lo;
    h_ranges[4 * k + 1] = before;
    h_ranges[4 * k + 2] = bs->fix_ranges[k].level;
    h_ranges[4 * k + 3] = 0;
    before += bs->fix_ranges[k].count;
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_ranges, h_ranges, (size_t)nr * 16, hipMemcpyHostToDevice, st));
  pcv_launch_spec_replay(ctx, bs->lv, d_ranges, nr, before, d.x, d.y, d.z, d.routed, (void*)s_pay, bs->spec_wide,
                         (uint32_t)pcv_pool_region_entries(bs->n));
  return PCV_OK;
}

// ------------------------------------------------------------------------------------------------
// the single-chain topology (pcv_spec.h), step by step: plan_sample -> allocate_attempt -> sample_round (at most twice) ->
// count_and_queue_sort -> settle_verdict
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kFirst = 16384;  // T'' nodes mirrored by the first copy (a 100 M-point tree has ~7 500)
// where that first mirror lands in the context's pinned_spec block: info at 0, then walk / parent / level of kFirst nodes
constexpr size_t kHostWalk = 256, kHostParent = kHostWalk + (size_t)kFirst * 4, kHostLevel = kHostParent + (size_t)kFirst * 4;
constexpr size_t kHostFirstBytes = kHostLevel + kFirst;

// What the steps hand to one another: each step reads the groups above its own and fills its own.
struct SingleChain {
  // the call
  pcv_ctx* ctx;
  PcvBuild* bs;
  pcv_octree* t;
  const pcv_build_params* params;
  uint32_t max_points;
  int full_levels;
  PcvNodeTableDev& nt;  // the sample tree's node table (its capacity bounds T'')
  // plan_sample
  uint64_t stride = 64, ns = 0;
  PcvSpecParams sp;
  double upper = 0.0;      // the candidate band's upper end, in sample points
  int sample_levels = 0;   // levels the sample keys cover in the coming round
  size_t tcap = 0;         // T'' nodes at most
  bool tree_by_split = false, table_tree = false;
  uint64_t pool_cap = 0, pool_entries = 0;
  bool compact = false;    // 12-byte records
  uint64_t wide_levels = 0;
  // allocate_attempt
  uint64_t* d_open = nullptr;  // the open sample nodes (at most nt.capacity: T'' holds 1 + 8 x that many nodes)
  uint32_t *d_ord = nullptr, *d_walk = nullptr, *d_sparent = nullptr, *d_info = nullptr, *d_counts = nullptr, *d_map = nullptr,
           *d_pool_ctr = nullptr;
  uint8_t* d_slevel = nullptr;
  uint32_t* rank = nullptr;  // the chain pass's rank array: keys_a
  uint4* payload = nullptr;
  uint4* wide = nullptr;
  uint8_t* depth_grid = nullptr;
  // sample_round (scratch that outlives a round, then the host's mirror of T'')
  uint64_t* small_partner = nullptr;
#ifdef PCV_EXPERIMENTS
  uint32_t* d_sample_counts = nullptr;
#endif
  PcvSpecTree tree;
  // count_and_queue_sort: the pool counters and the exact counts as they arrive in pinned_spec
  uint32_t *h_pool = nullptr, *h_counts = nullptr;
};

// plan: sample stride, PcvSpecParams, the levels of the first round's keys, the record form. Host arithmetic only.
// false: the cloud is too small to sample.
static bool plan_sample(SingleChain& s) {
  const PcvLevels& lv = s.bs->lv;
  const uint64_t n = s.bs->n;
  const uint32_t max_points = s.max_points;
  const int full_levels = s.full_levels;
  // the stride and the band rule: pcv_spec_sample_plan (pcv_spec.cpp), which the tests ask as well
  uint32_t stride;
  double delta;
  pcv_spec_sample_plan(n, max_points, &stride, &delta);
  s.stride = stride;
  s.ns = n / stride;
  if (s.ns == 0) return false;
  PcvSpecParams& sp = s.sp;
  sp.cap = max_points;
  sp.resolution = s.params->resolution;
  sp.edge = lv.edge;
  sp.nlevels = full_levels;
  sp.force_mask = (s.params->flags >> 8) & 0xffu;
  sp.scale = (double)stride;
  sp.delta = delta;
  s.upper = (double)sp.cap * (1.0 + sp.delta) / sp.scale;
  // T'' nodes at most (at least 4 096 records: the chain pass may mirror the table's first 2 048 in LDS without asking how many exist)
  s.tcap = std::max<size_t>(1 + 8 * (size_t)s.nt.capacity, 4096);
  // the sample tree straight from the sorted sample keys (pcv_launch_spec_sample_tree: two launches); the split into a node
  // table + spec_tree_scan / emit (fifteen launches for the 100 M bench cloud) stays in the experiment library
  // (sample_tree_split, or the one-level split kernels) — same T'' either way
  s.tree_by_split = pcv_switches().sample_tree_split || !pcv_switches().split2;
  s.table_tree = s.tree_by_split || pcv_switches().sample_counts;  // (the sample tree by counting builds a node table as well)
  // 12-byte records (pcv_internal.h) unless switched off (experiments) or the predicted tree could outgrow the 24 rank
  // bits of the key
  // ... or the pool of Float32 codes (kPcvPoolRegions regions, pcv_internal.h) could outgrow 32-bit entry numbers
  s.pool_cap = pcv_pool_region_entries(n);
  s.pool_entries = s.pool_cap * kPcvPoolRegions;
  s.compact = pcv_switches().compact_records && s.tcap <= (1u << 24) && s.pool_entries <= 0xffffffffull;
  for (int k = 0; k <= full_levels && k < 64; ++k)
    if (lv.enc[k] > PCV_ENC_UINT16) s.wide_levels |= 1ull << k;
  // Levels the sample keys cover first: a uniform cloud reaches the capacity at level log8(n / capacity); clustered clouds
  // go deeper, so eight levels on top (12 levels for the 100 M bench cloud whose deepest leaf sits at level 10, 13 for
  // 1 B points), at most 14. Every level less is a tenth of the sample's chain, three bits of its key sort and two
  // launches of its split; a sample tree that wants to go deeper is keyed again at full depth (pcv_single_chain_topology).
  int uniform = 0;
  for (uint64_t per_node = n / (uint64_t)max_points + 1; per_node > 1; per_node = (per_node + 7) / 8) ++uniform;
  s.sample_levels = std::min(14, std::max(10, uniform + 8));
  if (s.sample_levels > full_levels) s.sample_levels = full_levels;
  return true;
}

// allocate: everything the attempt takes from the pool (and the pinned block of the first mirror) before the first round.
static int allocate_attempt(SingleChain& s) {
  pcv_ctx* ctx = s.ctx;
  PcvScratch& sc = s.bs->sc;
  const uint64_t n = s.bs->n;
  const size_t tcap = s.tcap;
  int rc;
  // The predicted tree is built on the device (from the sorted sample keys, pcv_launch_spec_sample_tree): the one chain pass starts without a
  // host round trip, and the host mirrors the tree (one small asynchronous copy) while that pass runs.
  if ((!s.tree_by_split && (rc = sc.get(&s.d_open, s.nt.capacity))) || (s.table_tree && (rc = sc.get(&s.d_ord, s.nt.capacity)))) return rc;
  if ((rc = sc.get(&s.d_walk, tcap)) || (rc = sc.get(&s.d_sparent, tcap)) ||
      (rc = sc.get(&s.d_slevel, tcap)) || (rc = sc.get(&s.d_info, 64)) || (rc = sc.get(&s.d_pool_ctr, kPcvPoolRegions + tcap + 4)) ||
      (rc = sc.get(&s.d_map, tcap)))
    return rc;
  s.d_counts = s.d_pool_ctr + kPcvPoolRegions;  // the pool counters and the exact counts travel to the host in ONE copy
  s.rank = (uint32_t*)s.bs->keys_a;
  if (s.compact) {
    uint2* p2;
    if ((rc = sc.get(&p2, n)) || (rc = sc.get(&s.wide, s.pool_entries))) return rc;
    s.payload = (uint4*)p2;
  } else if ((rc = sc.get(&s.payload, n))) {
    return rc;
  }
  if (n >= (1u << 20) && (rc = sc.get(&s.depth_grid, pcv_spec_depth_grid_bytes()))) return rc;  // small builds: not worth a 2 MiB fill
  return ctx->pinned_spec_reserve(kHostFirstBytes + 256);
}

enum class SampleRound {
  kTreeMirrored,  // s.tree is the host's copy of T''; the chain pass down T'' is queued
  kKeyAgain,      // the sample tree wants to go deeper than the sample keys: key the sample again at full depth
  kLeaveToExact   // the prediction cannot be used (table capacity, deeper than one key word): the exact pipeline takes the build
};

// The end of a sample round: wait for the mirror of T'' (fed to the side stream by sample_round) and read it.
static int read_mirror(SingleChain& s, SampleRound* out) {
  pcv_ctx* ctx = s.ctx;
  hipStream_t st = ctx->stream;
  const uint8_t* hs = (const uint8_t*)ctx->pinned_spec;
  const size_t first = s.tcap < kFirst ? s.tcap : kFirst;
  *out = SampleRound::kLeaveToExact;
  PCV_HIP_CHECK(ctx, hipEventSynchronize(ctx->spec_ev));
  uint32_t info[4] = {0, 0, 0, 0};
  std::memcpy(info, hs, sizeof(info));
  if (info[1] & 2u) return PCV_OK;  // table capacity: let the exact pipeline report it
  if (info[1] & 1u) {               // deeper than the sample keys
    if (s.sample_levels < s.full_levels) *out = SampleRound::kKeyAgain;
    return PCV_OK;  // (at full depth already: deeper than one key word: the exact pipeline (deep path) takes it)
  }
  const uint32_t tn = info[0];
  if (tn <= first) {
    if (!pcv_spec_tree_from_walk((const uint32_t*)(hs + kHostWalk), (const uint32_t*)(hs + kHostParent), hs + kHostLevel, tn, &s.tree))
      return ctx->fail(PCV_E_HIP, "single-chain build: inconsistent predicted tree");
  } else {  // a big tree: fetch all of it (queued behind the chain pass; 500 M+ points)
    std::vector<uint32_t> w(tn), pr(tn);
    std::vector<uint8_t> lvl(tn);
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(w.data(), s.d_walk, (size_t)tn * 4, hipMemcpyDeviceToHost, st));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(pr.data(), s.d_sparent, (size_t)tn * 4, hipMemcpyDeviceToHost, st));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(lvl.data(), s.d_slevel, (size_t)tn, hipMemcpyDeviceToHost, st));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (!pcv_spec_tree_from_walk(w.data(), pr.data(), lvl.data(), tn, &s.tree))
      return ctx->fail(PCV_E_HIP, "single-chain build: inconsistent predicted tree");
  }
  *out = SampleRound::kTreeMirrored;
  return PCV_OK;
}

// One sample round: key the sample at s.sample_levels levels, sort (or count) the keys, build T'' on the device, record the
// fork, queue the ONE chain pass down T'', feed the side stream with the mirror of T'', wait for the mirror (read_mirror).
// The sample keys cover `sample_levels` levels first (plan_sample); a sample tree that wants to go deeper is keyed again at
// full depth.
static int sample_round(SingleChain& s, SampleRound* out) {
  *out = SampleRound::kLeaveToExact;
  pcv_ctx* ctx = s.ctx;
  PcvBuild* bs = s.bs;
  hipStream_t st = ctx->stream;
  PcvScratch& sc = bs->sc;
  DevPoints& d = bs->d;
  PcvLevels& lv = bs->lv;
  const PcvSpecParams& sp = s.sp;
  const PcvNodeTableDev& nt = s.nt;
  const uint64_t n = bs->n, ns = s.ns, stride = s.stride;
  const int sample_levels = s.sample_levels, full_levels = s.full_levels;
  const size_t tcap = s.tcap;
  int rc;
  lv.nlevels = sample_levels;
  // keys_a doubles as the rank array of the chain pass below: a second round must not start before the first
  // round's pass is done with it — same stream, so it is ordered
  uint64_t* skeys_a = bs->keys_b;  // the sample keys (and their sort partner) live in keys_b: 2 x n / 32 x 8 B of its 8 n
  const uint64_t soff = ((ns + 31) & ~31ull) + 32;  // keeps the partner 256-byte aligned
  uint64_t* skeys_b = bs->keys_b + soff;
  if (soff + ns > n) {  // tiny forced builds sample every point: the partner gets its own buffer
    if (!s.small_partner && (rc = sc.get(&s.small_partner, ns + 32))) return rc;
    skeys_b = s.small_partner;
  }
  // The sample is taken in clumps of 8 consecutive points (one clump every 8 x stride): read one by one, every
  // sampled coordinate costs a full cache line (1.2 GB and 0.23 ms for the 3.1 M sample points of a 100 M cloud)
  constexpr uint32_t clump_shift = 3;
  // cleared by the chain-keys launch on its way: 64 words, the counters of the sample tree kernels
  uint32_t* zero;
  if ((rc = sc.get(&zero, 64))) return rc;
  pcv_launch_chain_keys(ctx, lv, ns, stride, d.x, d.y, d.z, skeys_a, false, d.routed, stride > 1 ? clump_shift : 0u, zero, 64);
  bool in_a = true;
  // sample_counts (libpcv_hip_exp.so only): the sample tree by COUNTING the keys, three levels per launch pair
  // (pcv_topology.hip): 9 launches instead of 27 and no sort — and 2-3 x SLOWER, measured: the 1.5 M keys cost 4.7 M
  // device-scope atomics per group of levels and this part retires ~9 G of those per second (0.54 + 0.38 ms for the two
  // middle groups against 0.28 ms for the whole key sort + split; profiles/r05_ab_sample_tree_by_counting_dropped.json)
  const uint32_t thr_s = pcv_spec_sample_threshold(sp);
  bool counted = false;
#ifdef PCV_EXPERIMENTS
  if (pcv_switches().sample_counts && thr_s > 0 && nt.max_open >= ns / thr_s + 16 && sample_levels <= PCV_MAX_KEY_LEVELS) {
    if (!s.d_sample_counts && (rc = sc.get(&s.d_sample_counts, pcv_sample_count_scratch_words(nt.capacity, nt.max_open, full_levels)))) return rc;
    // (a count only matters up to the larger of the split threshold and the candidate band's upper end)
    const double sat_d = std::fmax((double)thr_s, std::ceil(s.upper)) + 2.0;
    const uint32_t sat = sat_d >= 4294967000.0 ? 0xfffffff0u : (uint32_t)sat_d;
    pcv_launch_sample_tree_counts(ctx, nt, skeys_a, (uint32_t)ns, lv, s.params->resolution, thr_s, sp.force_mask, s.d_sample_counts, sat);
    counted = true;
  }
#endif
  if (!counted && (rc = pcv_radix_sort_u64(ctx, skeys_a, skeys_b, ns, 3 * (PCV_MAX_KEY_LEVELS - sample_levels), 3 * PCV_MAX_KEY_LEVELS,
                                           nullptr, bs->sort_scratch, &in_a)))
    return rc;
  if (!counted && !s.tree_by_split) {
    if ((rc = pcv_launch_spec_sample_tree(ctx, in_a ? skeys_a : skeys_b, (uint32_t)ns, lv, s.params->resolution, thr_s, s.upper, sp.force_mask,
                                          s.d_open, nt.capacity, zero, s.d_walk, s.d_sparent, s.d_slevel, s.d_info, s.d_pool_ctr)))
      return rc;
  } else {
    if (!counted) {
      pcv_launch_node_split(ctx, nt, in_a ? skeys_a : skeys_b, false, (uint32_t)ns, lv, s.params->resolution, thr_s, sp.force_mask);
    }
    pcv_launch_spec_tree(ctx, nt, s.upper, sp.force_mask, s.d_ord, s.d_walk, s.d_sparent, s.d_slevel, s.d_info, s.d_pool_ctr);
  }
  uint8_t* hs = (uint8_t*)ctx->pinned_spec;
  const size_t first = tcap < kFirst ? tcap : kFirst;
  // The host's mirror of the tree and the zeroed counters travel on the side stream: on `stream` each of these small
  // operations would sit (with its ~12 us hand-over) between the tree kernels and the chain pass. The fork point is
  // recorded now, the chain pass is queued next (the GPU has caught up with the host by here, so every API call
  // before that launch is idle GPU time), and only then is the side stream fed.
  PCV_HIP_CHECK(ctx, hipEventRecord(ctx->side_fork, st));
  ctx->stage_end(PCV_STAGE_CHAIN_KEYS);

  // ---- the one chain pass (queued before the host has seen the tree) ----
  ctx->stage_begin(PCV_STAGE_LEAF_ENCODE);
  lv.nlevels = full_levels;
  // round 6, measured and NOT shipped (color_late, libpcv_hip_exp.so; profiles/r06_ab_colour_joins_in_the_sort_dropped.json):
  // the 12-byte records leave the pass without their colour and the record sort's first pass — which reads every record in
  // input order anyway — fetches it from the caller's array. The chain pass gains 0.13 ms (1.86 -> 1.73 at 100 M points), the
  // sort's first pass loses 0.31 (0.59 -> 0.90): eight more (unaligned) loads per lane on top of its sixteen — that pass is
  // bound by the issue of its vector-memory instructions, not by bytes. Same octree either way.
  bs->color_late = pcv_switches().color_late && s.compact;
  // The packed hand-over (ships; packed_handover off: the 12-byte records with their colour): single-chain build with 12-byte
  // records, raw input, no intensity plane. Where T'' has at most 65 536 nodes — which the device knows now and the host once it
  // has mirrored the tree (count_and_queue_sort) — the pass leaves the colour to the sort's first pass and writes 8-byte
  // records and the ranks as a plane of half words; a bigger tree gets today's 12-byte records with their colour. Whether the
  // sort can take packed records is settled when it is queued (pcv_queue_record_sort): the rows form's first pass loads them
  // as they are, any other sort gets them unpacked first. (rec_wc bit 0, experiments: the write-combining first pass takes
  // 12-byte records with their colour: the old hand-over.)
  bs->pack_tried = pcv_packed_handover_tried(pcv_switches().packed_handover && !bs->color_late && !(pcv_switches().rec_wc & 1), s.compact,
                                             d.routed.oct != nullptr,
                                             d.intensity != nullptr || s.t->has_intensity);
  bs->packed = false;
  // the exact counters (d_counts) are cleared by the depth-grid kernel in front of the pass where there is one; small builds
  // clear them with a fill on `stream`
  const size_t counts_words = (tcap + 3) & ~(size_t)3;
  const bool zero_in_grid = s.depth_grid && (((uintptr_t)s.d_counts & 15) == 0);
  if (!zero_in_grid) PCV_HIP_CHECK(ctx, hipMemsetAsync(s.d_counts, 0, tcap * 4, st));
  // the intensity plane needs no copy: the chain pass leaves its records in input order, so the record sort's first pass
  // reads the caller's own array (PcvSortPayload::first_in0, pcv_queue_record_sort) — 8 bytes per point less in the chain pass
  uint32_t* inten_bits = nullptr;
  pcv_launch_spec_encode(ctx, lv, s.d_walk, n, d.x, d.y, d.z, d.routed, d.color, d.color_stride, d.intensity, s.rank, s.payload,
                         inten_bits, s.depth_grid, s.wide, s.d_pool_ctr /* zeroed by the spec_tree kernels */, s.d_info, bs->color_late,
                         zero_in_grid ? s.d_counts : nullptr, zero_in_grid ? counts_words : 0, bs->pack_tried);
  ctx->stage_end(PCV_STAGE_LEAF_ENCODE);

  PCV_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_fork, 0));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(hs, s.d_info, 16, hipMemcpyDeviceToHost, ctx->side));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(hs + kHostWalk, s.d_walk, first * 4, hipMemcpyDeviceToHost, ctx->side));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(hs + kHostParent, s.d_sparent, first * 4, hipMemcpyDeviceToHost, ctx->side));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(hs + kHostLevel, s.d_slevel, first, hipMemcpyDeviceToHost, ctx->side));
  PCV_HIP_CHECK(ctx, hipEventRecord(ctx->spec_ev, ctx->side));

  // ---- meanwhile: the host's view of the tree ----
  return read_mirror(s, out);
}

// count and queue: exact counts -> rank map (device); the counts' copy for the host's resolve on the side stream; the record
// sort queued behind the device's resolve, ahead of the verdict.
static int count_and_queue_sort(SingleChain& s) {
  pcv_ctx* ctx = s.ctx;
  PcvBuild* bs = s.bs;
  PcvScratch& sc = bs->sc;
  const PcvLevels& lv = bs->lv;
  const PcvSpecTree& tree = s.tree;
  const uint64_t n = bs->n;
  int rc;
  // ---- exact counts -> rank map (device) and true tree (host) ----
  ctx->stage_begin(PCV_STAGE_NODE_SPLIT);
  // 12-byte records and a predicted tree whose counters fit one LDS histogram and whose map fits beside the sort's staging
  // (up to 16 384 nodes: clouds of up to ~250 M points at the default capacity):
  // the count runs over the record sort's own workgroups and keeps every workgroup's histogram, from which the sort's first
  // pass derives its digit histogram (the keys are then read by its downsweep only, which applies the map itself).
  // sort_rows off (libpcv_hip_exp.so): the first pass counts (and maps) the keys in a pass of its own.
  bs->spec_rows = nullptr;
  // (a predicted leaf is named by its node index: tree.num_leaves is the number of T'' nodes the chain pass decided by)
  bs->packed = bs->pack_tried && pcv_packed_handover(tree.num_leaves);
  if (bs->packed) bs->color_late = true;  // (packed records come without their colour)
  const int rank_shift = bs->packed ? 0 : s.compact ? 8 : 0;
  if (pcv_switches().sort_rows && s.compact && tree.num_leaves <= pcv_rank_hist_max_bins()) {
    int sgroups;
    uint64_t schunk;
    pcv_sort_rec12_geometry(n, &sgroups, &schunk);
    uint32_t* rows = nullptr;
    // the rows are an optimisation (up to ~1 GB beside the records for the biggest trees): a failed allocation falls
    // back to the plain count, whose sort takes a counting pass instead
    if (sc.get(&rows, (size_t)sgroups * tree.num_leaves) == PCV_OK) {
      pcv_launch_rank_hist_rows(ctx, s.rank, n, tree.num_leaves, s.d_counts, rank_shift, sgroups, schunk, rows, bs->packed);
      bs->spec_rows = rows;
    }
  }
  if (!bs->spec_rows) pcv_launch_rank_hist(ctx, s.rank, n, tree.num_leaves, s.d_counts, rank_shift, bs->packed);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = ctx->pinned_spec_reserve((size_t)tree.num_leaves * 8 + 512 + kPcvPoolRegions * 4))) return rc;
  uint8_t* hp = (uint8_t*)ctx->pinned_spec;
  // the number of `wide` pool entries the chain pass handed out per region (the record epilogue of chain_pass_kernel), then the exact counts: one
  // block on the device, one copy (every small operation on `stream` costs a hand-over of ~10 us between two kernels)
  s.h_pool = (uint32_t*)hp;
  s.h_counts = s.h_pool + kPcvPoolRegions;
  // (the copy travels on the side stream, behind an event of `stream`: a copy command between the count and the resolve kernel costs
  // `stream` two hand-overs of ~10 us; nothing queued on `stream` later writes these counters)
  if (ctx->side_begin() != PCV_OK) return ctx->fail(PCV_E_HIP, "single-chain build: side stream");
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(s.h_pool, s.d_pool_ctr, ((size_t)kPcvPoolRegions + tree.num_leaves) * 4, hipMemcpyDeviceToHost, ctx->side));
  PCV_HIP_CHECK(ctx, hipEventRecord(ctx->spec_ev, ctx->side));  // the counts are on their way to the host
  // The map the record sort needs is computed on the device (spec_resolve_kernel), and the sort is queued behind it right
  // away: the counts' trip to the host, the host's own resolve and the table building all happen beside the sort instead
  // of in front of it. The sort's digit widths come from the number of PREDICTED leaves (an upper bound of the true
  // leaves, known since the host mirrored T'').
  bs->spec_wide = s.wide;
  bs->wide_levels = s.wide_levels;
  bs->spec_map_dev = s.d_map;
  bs->spec_map_entries = tree.num_leaves;
  bs->spec = true;
  bs->spec_payload = s.payload;
  bs->fix_ranges.clear();
  uint32_t *d_nst, *d_base, *d_out;
  const uint32_t tn = (uint32_t)tree.prefix.size();
  if ((rc = sc.get(&d_nst, tn)) || (rc = sc.get(&d_base, tn))) return rc;
  // the kernel stores its verdict straight into the pinned mailbox (host memory the device can write): no copy between
  // the resolve kernel and the sort
  d_out = (uint32_t*)(ctx->mailbox_dev + kPcvMailboxResolve);
  // the sentinel goes in BEFORE the launch: nothing queued on the stream writes this slot until the kernel does, and a
  // store after the launch could overwrite a verdict the kernel had already delivered
  ctx->mailbox[kPcvMailboxResolve] = ~0ull;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  pcv_launch_spec_resolve(ctx, lv, s.params->resolution, s.sp.cap, s.sp.force_mask, s.d_walk, s.d_slevel, tn, s.d_counts, d_nst, d_base, s.d_map, d_out);
  PCV_HIP_CHECK(ctx, hipGetLastError());  // before the sort is queued behind it
  // {true leaves, too shallow} as the device sees them: read by pcv_build_finish (which synchronises anyway) and held
  // against the host's resolve — the device map drives the sort, the host's tree the tables
  bs->resolve_on_device = true;
  ctx->stage_end(PCV_STAGE_NODE_SPLIT);
  const uint32_t predicted_leaves = (uint32_t)std::count(tree.inner.begin(), tree.inner.end(), (uint8_t)0);
  return pcv_queue_record_sort(ctx, bs, s.t, nullptr, predicted_leaves, false);
}

// verdict: the host's resolve of the exact counts. Held (*used): `tt` is the true tree, the build state names the leaves that
// continue or replay their chain, the replay is queued (or left to pcv_build_finish with the sort's held-back pass). Not
// held: PcvBuild::drop_single_chain and *used stays false.
static int settle_verdict(SingleChain& s, PcvTrueTree* tt, bool* used) {
  pcv_ctx* ctx = s.ctx;
  PcvBuild* bs = s.bs;
  pcv_octree* t = s.t;
  const PcvSpecTree& tree = s.tree;
  int rc;
  PCV_HIP_CHECK(ctx, hipEventSynchronize(ctx->spec_ev));
  const PcvSpecStatus resolved = pcv_spec_resolve(s.sp, tree, s.h_counts, tt);
  if (resolved != PCV_SPEC_OK) {
    bs->drop_single_chain(s.payload, s.wide);
    return PCV_OK;  // *used stays false
  }
  // the rare replay takes its pool entries from the TOPS of the pool regions (spec_replay_kernel: slot j of the flattened
  // replay list -> region j % regions): they must not reach down to what the chain pass filled from the bottoms. A point
  // has at most one live entry, but a replayed point may have used one in the chain pass already — on an adversarial
  // cloud a region can run out: the exact pipeline takes the build
  if (s.wide) {
    uint64_t replay_slots = 0, used_entries = 0, most = 0;
    for (uint32_t k : tt->fix_nodes) replay_slots += tt->hi[k] - tt->lo[k];
    for (uint32_t r = 0; r < kPcvPoolRegions; ++r) {
      used_entries += s.h_pool[r];
      most = std::max<uint64_t>(most, s.h_pool[r]);
    }
    if (most + (replay_slots + kPcvPoolRegions - 1) / kPcvPoolRegions > s.pool_cap) {
      bs->drop_single_chain(s.payload, s.wide);
      return PCV_OK;
    }
    t->wide_pool_entries = used_entries;
  }
  bs->resolve_host_leaves = tt->num_leaves;
  bs->resolve_check_map = (s.params->flags & PCV_BUILD_CHECK_RESOLVE) != 0;
  if (bs->resolve_check_map) {
    bs->resolve_host_map = tt->spec_map;
    bs->resolve_host_inner = tree.inner;
  }
  if (tt->prefix.size() > (size_t)s.nt.capacity) return ctx->fail(PCV_E_OOM, "node table capacity exceeded");
  bs->cont_nodes = tt->cont_nodes;
  bs->cont_from = tt->cont_from;
  // leaves whose points still have to replay the chain: contiguous once the records are sorted ([lo, hi) of the leaf)
  for (uint32_t k : tt->fix_nodes) bs->fix_ranges.push_back({tt->lo[k], tt->hi[k] - tt->lo[k], (uint32_t)tt->level[k]});
  // replayed leaves rewrite their SORTED records: with the sort's second pass held back (PcvSortSecond) the replay is queued
  // behind that pass, in pcv_build_finish
  if (!bs->sort_second.pending && (rc = pcv_queue_replay(ctx, bs))) return rc;
  ctx->stage_begin(PCV_STAGE_TABLE);
  t->spec_stats[0] = tree.prefix.size();
  t->spec_stats[1] = (uint64_t)std::count(tree.inner.begin(), tree.inner.end(), (uint8_t)0);
  t->spec_stats[2] = tt->kept_points;
  t->spec_stats[3] = tt->fix_points;
  t->spec_continued = tt->cont_points;
  *used = true;
  return PCV_OK;
}

// The single-chain topology (pcv_spec.h): sample -> predicted tree T'' -> ONE chain pass for all points -> exact counts
// per predicted leaf -> true tree on the host. On success (*used) the records (true-leaf rank in the first half of
// keys_a, payload in bs->spec_payload, intensity bits in the second half of keys_a) are what K5 would have produced and
// `tt` is the node table K4 would have produced. *used == false: the prediction did not cover the tree (or the sample
// says the tree is deeper than one key word): the caller runs the exact pipeline; nothing of this attempt is kept.
int pcv_single_chain_topology(pcv_ctx* ctx, PcvBuild* bs, pcv_octree* t, const pcv_build_params* params, uint32_t max_points,
                              int full_levels, PcvNodeTableDev& nt, PcvTrueTree* tt, bool* used) {
  *used = false;
  SingleChain s{ctx, bs, t, params, max_points, full_levels, nt};
  int rc;
  if (!plan_sample(s)) return PCV_OK;
  ctx->stage_begin(PCV_STAGE_CHAIN_KEYS);
  if ((rc = allocate_attempt(s))) return rc;
  // two rounds at most: the second one keys the sample at full depth and cannot ask for more
  SampleRound round;
  if ((rc = sample_round(s, &round))) return rc;
  if (round == SampleRound::kKeyAgain) {
    s.sample_levels = full_levels;
    ctx->stage_begin(PCV_STAGE_CHAIN_KEYS);
    if ((rc = sample_round(s, &round))) return rc;
  }
  if (round != SampleRound::kTreeMirrored) return PCV_OK;  // *used stays false: the caller runs the exact pipeline
  s.sp.nlevels = s.sample_levels;
  if ((rc = count_and_queue_sort(s))) return rc;
  return settle_verdict(s, tt, used);
}
