// pcv_sort.hip — K3: stable LSD radix sort for gfx950 (wave64), 8-bit digits, LDS histograms.
//
// The reference never sorts: it partitions every node's stream into 8 child files level by level
// (src/octree/generation.rs:58-126: 8 clones + 8 `retain`s per batch). On the GPU the same *stable* grouping
// is one radix sort of the path keys (and later of leaf-rank records), SURVEY.md §8a R7 / F11.
//
// Structure per 8-bit pass (reduce-then-scan, no inter-workgroup spinning):
//   upsweep   : G workgroups, each counts the digits of its contiguous chunk in per-wave LDS histograms
//   scan      : one workgroup per digit scans that digit's G counts; digit totals are scanned in the downsweep
//   downsweep : the same G workgroups walk their chunk tile by tile; inside a tile each wave ranks its keys
//               with ballot-built peer masks (64-lane match-any), a 256-entry LDS scan orders the digits,
//               keys (and the record payload) are staged through LDS so global stores go out as runs.
// Two downsweep kernels: keys only (u32/u64, 16 keys per lane, next tile prefetched into registers) and records
// (u32 key + one 16-byte payload word per key, 8 per lane, + optional extra 4-byte planes).
// HBM traffic per pass and key: sizeof(key) (upsweep) + 2 * sizeof(key) + 2 * payload bytes.
// This file: the upsweeps, the scan, the two downsweeps and the generic pass loop over a plan (pcv_sort_plan.h). The 12-byte
// records of the single-chain build — their downsweep, the rows form, the settling pass — are pcv_sort_rec12.hip.
#include "pcv_sort_dev.h"

namespace {

// kPlain: one LDS add per key instead of the ballot match — for digits that are spread evenly over the wave (the upper
// digit of the record sort after the pass on the lower one: 0.132 -> 0.115 ms at 100 M records; the match wins on the
// skewed digits of the first pass and of the path keys)
template <typename KeyT, bool kPlain = false>
__global__ __launch_bounds__(kBlock) void upsweep_kernel(const KeyT* __restrict__ keys, uint64_t n, uint64_t chunk,
                                                          int groups, int shift, uint32_t mask,
                                                          uint32_t* __restrict__ hist /* [256][groups] */) {
  __shared__ uint32_t wh[kWaves][kRadix];
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kWaves * kRadix; i += kBlock) (&wh[0][0])[i] = 0;
  __syncthreads();
  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  uint64_t end = begin + chunk;
  if (end > n) end = n;
  constexpr int kVec = 16 / sizeof(KeyT);  // keys per 16-byte load
  typedef KeyT VecT __attribute__((ext_vector_type(kVec)));
  // chunk is a multiple of the tile and buffers come from the pool (256-B aligned) => 16-byte loads are aligned
  uint64_t i = begin + (uint64_t)threadIdx.x * kVec;
  constexpr uint64_t kStep = (uint64_t)kBlock * kVec;
  // four 16-byte loads in flight per lane: the loop is latency bound otherwise
  for (; i + 3 * kStep + kVec <= end; i += 4 * kStep) {
    VecT v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const VecT*>(keys + i + u * kStep);
    // the loop condition is not wave-uniform in the last iterations of a chunk: match only the lanes that are here
    const uint64_t here = __builtin_amdgcn_ballot_w64(true);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int k = 0; k < kVec; ++k) {
        if (kPlain) atomicAdd(&wh[wave][(uint32_t)(v[u][k] >> shift) & mask], 1u);
        else count_digit(wh[wave], (uint32_t)(v[u][k] >> shift) & mask, here, true);
      }
  }
  for (; i + kVec <= end; i += kStep) {
    VecT v = *reinterpret_cast<const VecT*>(keys + i);
    const uint64_t here = __builtin_amdgcn_ballot_w64(true);
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
      if (kPlain) atomicAdd(&wh[wave][(uint32_t)(v[k] >> shift) & mask], 1u);
      else count_digit(wh[wave], (uint32_t)(v[k] >> shift) & mask, here, true);
    }
  }
  for (; i < end; ++i) atomicAdd(&wh[wave][(uint32_t)(keys[i] >> shift) & mask], 1u);  // ragged tail (< kVec keys)
  __syncthreads();
  for (int d = threadIdx.x; d < kRadix; d += kBlock) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += wh[w][d];
    hist[(uint64_t)d * groups + blockIdx.x] = s;
  }
}

// First record pass of the single-chain build: the upsweep reads every rank anyway, so it also translates it on the way
// — rank := map[rank], written back in place — and counts the digits of the MAPPED ranks: one pass over the ranks
// instead of two; the downsweep is the ordinary one. The payloads are not touched: a record already carries the codes
// its true leaf needs (pcv_spec.h), except for the rare leaves the map flags PCV_SPEC_MAP_REPLAY (bit 30), whose points
// leave their input index in the first payload word for the replay after the sort.
// kMapLds: the map (one entry per predicted leaf; 30 KB for a 100 M-point tree) is copied into LDS first — eight
// dependent lookups per lane and iteration then cost LDS latency instead of a trip to the vector L1 / L2 that the
// streaming keys keep evicting it from. Static + dynamic LDS stay inside the 64 KB a kernel gets without opting in.
// (kPcvSortUpsweepMapLdsEntries, pcv_sort_plan.h: 60 000 bytes next to the 4 KB of counters)
// kCompact (12-byte records, pcv_internal.h): key = rank << 8 | blue, payload = uint2; `shift` is the digit's position
// inside the KEY (8 + its position inside the rank).
template <bool kMapLds, bool kCompact>
__global__ __launch_bounds__(kBlock) void upsweep_map_kernel(uint32_t* __restrict__ keys, uint64_t n, uint64_t chunk, int groups,
                                                              int shift, uint32_t mask, uint32_t* __restrict__ hist,
                                                              const uint32_t* __restrict__ gmap, uint32_t map_entries,
                                                              void* __restrict__ payload_v) {
  __shared__ uint32_t wh[kWaves][kRadix];
  extern __shared__ uint32_t smap[];  // kMapLds: map_entries words (dynamic, so small maps keep the occupancy)
  const int wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kWaves * kRadix; i += kBlock) (&wh[0][0])[i] = 0;
  if (kMapLds)
    for (uint32_t i = threadIdx.x; i < map_entries; i += kBlock) smap[i] = gmap[i];
  const uint32_t* map = kMapLds ? smap : gmap;
  __syncthreads();
  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  uint64_t end = begin + chunk;
  if (end > n) end = n;
  auto one = [&](uint64_t idx, uint32_t old, uint32_t m) -> uint32_t {
    if (__builtin_expect((m & (1u << 30)) != 0u, 0)) {  // replay: the first payload word becomes the input index
      if (kCompact) reinterpret_cast<uint32_t*>(reinterpret_cast<uint2*>(payload_v) + idx)[0] = (uint32_t)idx;
      else reinterpret_cast<uint32_t*>(reinterpret_cast<uint4*>(payload_v) + idx)[0] = (uint32_t)idx;
    }
    return kCompact ? (((m & PCV_SPEC_INDEX_MASK) << 8) | (old & 0xffu)) : (m & PCV_SPEC_INDEX_MASK);
  };
  constexpr int kKeyShift = kCompact ? 8 : 0;  // position of the predicted-leaf rank inside the key
  uint64_t i = begin + (uint64_t)threadIdx.x * 4;
  constexpr uint64_t kStep = (uint64_t)kBlock * 4;
  for (; i + 3 * kStep + 4 <= end; i += 4 * kStep) {  // four 16-byte loads and their sixteen map lookups in flight per lane
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const uint4*>(keys + i + u * kStep);
    uint32_t r[16];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t o[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
      uint32_t m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = map[o[k] >> kKeyShift];
#pragma unroll
      for (int k = 0; k < 4; ++k) r[4 * u + k] = one(i + u * kStep + k, o[k], m[k]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      *reinterpret_cast<uint4*>(keys + i + u * kStep) = make_uint4(r[4 * u], r[4 * u + 1], r[4 * u + 2], r[4 * u + 3]);
    const uint64_t here = __builtin_amdgcn_ballot_w64(true);
#pragma unroll
    for (int k = 0; k < 16; ++k) count_digit(wh[wave], (r[k] >> shift) & mask, here, true);
  }
  for (; i + 4 <= end; i += kStep) {
    const uint4 v = *reinterpret_cast<const uint4*>(keys + i);
    const uint32_t o[4] = {v.x, v.y, v.z, v.w};
    uint32_t m[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = map[o[k] >> kKeyShift];
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = one(i + k, o[k], m[k]);
    *reinterpret_cast<uint4*>(keys + i) = make_uint4(r[0], r[1], r[2], r[3]);
    const uint64_t here = __builtin_amdgcn_ballot_w64(true);
#pragma unroll
    for (int k = 0; k < 4; ++k) count_digit(wh[wave], (r[k] >> shift) & mask, here, true);
  }
  for (; i < end; ++i) {  // ragged tail (< 4 keys per lane)
    const uint32_t o = keys[i];
    const uint32_t r = one(i, o, map[o >> kKeyShift]);
    keys[i] = r;
    atomicAdd(&wh[wave][(r >> shift) & mask], 1u);
  }
  __syncthreads();
  for (int d = threadIdx.x; d < kRadix; d += kBlock) {
    uint32_t s2 = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s2 += wh[w][d];
    hist[(uint64_t)d * groups + blockIdx.x] = s2;
  }
}

// One workgroup per digit: exclusive scan of that digit's `groups` counters in place (groups <= 1024) and the
// digit's total. The scan across digits is folded into the downsweep prologue (256 values).
__global__ __launch_bounds__(256) void scan_kernel(uint32_t* __restrict__ hist, int groups,
                                                    uint32_t* __restrict__ totals) {
  __shared__ uint32_t wave_tot[4];
  uint32_t* row = hist + (uint64_t)blockIdx.x * groups;
  constexpr int kPerMax = (kMaxGroups + 255) / 256;
  const int per = (groups + 255) / 256;  // <= kPerMax
  const int begin = threadIdx.x * per;
  uint32_t v[kPerMax];
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < kPerMax; ++i) v[i] = 0;
#pragma unroll
  for (int i = 0; i < kPerMax; ++i)
    if (i < per && begin + i < groups) {
      v[i] = row[begin + i];
      sum += v[i];
    }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t woff = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    woff += (w < wave) ? wave_tot[w] : 0u;
    total += wave_tot[w];
  }
  uint32_t run = woff + inc - sum;
#pragma unroll
  for (int i = 0; i < kPerMax; ++i)
    if (i < per && begin + i < groups) {
      row[begin + i] = run;
      run += v[i];
    }
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// ---- keys only ------------------------------------------------------------------------------------
template <typename KeyT>
__global__ __launch_bounds__(kBlock, kKeysWaves) void downsweep_keys_kernel(const KeyT* __restrict__ keys_in,
                                                                   KeyT* __restrict__ keys_out, uint64_t n, uint64_t chunk,
                                                                   int groups, int shift, int nbits,
                                                                   const uint32_t* __restrict__ offsets,
                                                                   const uint32_t* __restrict__ totals) {
  constexpr int kKpt = kKptKeys, kTile = kBlock * kKpt;
  __shared__ KeyT skeys[kTile];
  __shared__ DigitState<kRadix> S;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t mask = (1u << nbits) - 1u;
  init_digit_base(S, offsets, totals, groups, t, lane, wave);

  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  uint64_t end = begin + chunk;
  if (end > n) end = n;
  const uint32_t wbase = wave * 64 * kKpt + lane;

  KeyT key[kKpt];
  {  // first tile
    const uint32_t tile_n = (uint32_t)((end - begin) < (uint64_t)kTile ? (end - begin) : (uint64_t)kTile);
#pragma unroll
    for (int i = 0; i < kKpt; ++i) {
      const uint32_t li = wbase + i * 64;
      key[i] = li < tile_n ? keys_in[begin + li] : (KeyT)0;
    }
  }
  for (uint64_t base = begin; base < end; base += kTile) {
    const uint32_t tile_n = (uint32_t)((end - base) < (uint64_t)kTile ? (end - base) : (uint64_t)kTile);
    uint16_t lpos[kKpt];
    if (tile_n == (uint32_t)kTile)
      wave_rank_all<kKpt, KeyT, true, kRadix>(S, wave, wbase, tile_n, key, shift, mask, lpos);
    else
      wave_rank_all<kKpt, KeyT, false, kRadix>(S, wave, wbase, tile_n, key, shift, mask, lpos);
    digit_scan(S, t, lane, wave);
#pragma unroll
    for (int i = 0; i < kKpt; ++i) {
      if (wbase + i * 64 < tile_n) {
        const uint32_t d = (uint32_t)(key[i] >> shift) & mask;
        skeys[S.whist[wave][d] + lpos[i]] = key[i];
      }
    }
    // the key registers are free now: fetch the next tile while this one drains through LDS
    const uint64_t nbase = base + kTile;
    if (nbase < end) {
      const uint32_t next_n = (uint32_t)((end - nbase) < (uint64_t)kTile ? (end - nbase) : (uint64_t)kTile);
#pragma unroll
      for (int i = 0; i < kKpt; ++i) {
        const uint32_t li = wbase + i * 64;
        key[i] = li < next_n ? keys_in[nbase + li] : (KeyT)0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kKpt; ++j) {
      const uint32_t p = j * kBlock + t;
      if (p < tile_n) {
        const KeyT k = skeys[p];
        const uint32_t d = (uint32_t)(k >> shift) & mask;
        keys_out[S.delta[d] + p] = k;
      }
    }
#pragma unroll
    for (int w = 0; w < kWaves; ++w) S.whist[w][t] = 0;  // last read before the barrier above
    __syncthreads();
  }
}

// ---- records: u32 key + optional 16-byte payload + extra 4-byte planes -----------------------------
struct RecPtrs {
  const void* vec_in;  // may be null; uint4 (20-byte records) or uint2 (12-byte records) per key
  void* vec_out;
  int nplanes;          // extra u32 planes (0..8)
  const uint32_t* plane_in[8];
  uint32_t* plane_out[8];
};

// kPrefetch: the next tile's keys and payloads are loaded into the registers the LDS staging just freed, so that the
// loads are in flight while this tile drains through LDS to memory (as the keys-only kernel does).
template <bool kHasVec, bool kPrefetch = false, typename VecT = uint4, int R = kRadix>
__global__ __launch_bounds__(kBlock, kHasVec ? kRecWaves : 4) void downsweep_rec_kernel(const uint32_t* __restrict__ keys_in,
                                                                  uint32_t* __restrict__ keys_out, uint64_t n,
                                                                  uint64_t chunk, int groups, int shift, int nbits,
                                                                  const uint32_t* __restrict__ offsets,
                                                                  const uint32_t* __restrict__ totals, RecPtrs rp) {
  constexpr int kKpt = kKptRec, kTile = kBlock * kKpt;
  __shared__ uint32_t skeys[kTile];
  __shared__ VecT svec[kHasVec ? kTile : 1];
  __shared__ DigitState<R> S;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t mask = (1u << nbits) - 1u;
  init_digit_base(S, offsets, totals, groups, t, lane, wave);
  const VecT* __restrict__ vec_in = reinterpret_cast<const VecT*>(rp.vec_in);
  VecT* __restrict__ vec_out = reinterpret_cast<VecT*>(rp.vec_out);

  const uint64_t begin = (uint64_t)blockIdx.x * chunk;
  uint64_t end = begin + chunk;
  if (end > n) end = n;
  const uint32_t wbase = wave * 64 * kKpt + lane;

  uint32_t key[kKpt];
  VecT vec[kHasVec ? kKpt : 1];
  auto load_tile = [&](uint64_t base, uint32_t tile_n) {
#pragma unroll
    for (int i = 0; i < kKpt; ++i) {
      const uint32_t li = wbase + i * 64;
      const bool valid = li < tile_n;
      key[i] = valid ? keys_in[base + li] : 0u;
      if (kHasVec) vec[i] = valid ? vec_in[base + li] : VecT{};
    }
  };
  if (kPrefetch && begin < end) load_tile(begin, (uint32_t)((end - begin) < (uint64_t)kTile ? (end - begin) : (uint64_t)kTile));
  for (uint64_t base = begin; base < end; base += kTile) {
    const uint32_t tile_n = (uint32_t)((end - base) < (uint64_t)kTile ? (end - base) : (uint64_t)kTile);
    if (!kPrefetch) load_tile(base, tile_n);
    uint16_t lpos[kKpt];
    if (tile_n == (uint32_t)kTile)
      wave_rank_all<kKpt, uint32_t, true, R>(S, wave, wbase, tile_n, key, shift, mask, lpos, nbits);
    else
      wave_rank_all<kKpt, uint32_t, false, R>(S, wave, wbase, tile_n, key, shift, mask, lpos, nbits);
    digit_scan(S, t, lane, wave);
#pragma unroll
    for (int i = 0; i < kKpt; ++i) {
      if (wbase + i * 64 < tile_n) {
        const uint32_t d = (key[i] >> shift) & mask;
        const uint32_t p = S.whist[wave][d] + lpos[i];
        lpos[i] = (uint16_t)p;
        skeys[p] = key[i];
        if (kHasVec) svec[p] = vec[i];
      }
    }
    if (kPrefetch) {  // the key / payload registers are free: fetch the next tile while this one drains
      const uint64_t nbase = base + kTile;
      if (nbase < end) load_tile(nbase, (uint32_t)((end - nbase) < (uint64_t)kTile ? (end - nbase) : (uint64_t)kTile));
    }
    __syncthreads();
    uint32_t gidx[kKpt];
#pragma unroll
    for (int j = 0; j < kKpt; ++j) {
      const uint32_t p = j * kBlock + t;
      if (p < tile_n) {
        const uint32_t k = skeys[p];
        const uint32_t d = (k >> shift) & mask;
        const uint32_t g = S.delta[d] + p;
        gidx[j] = g;
        keys_out[g] = k;
        if (kHasVec) vec_out[g] = svec[p];
      }
    }
    for (int w = 0; w < rp.nplanes; ++w) {  // rare: intensity / Float64 high words / generic pairs API
      const uint32_t* __restrict__ src = rp.plane_in[w];
      uint32_t* __restrict__ dst = rp.plane_out[w];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kKpt; ++i) {
        const uint32_t li = wbase + i * 64;
        if (li < tile_n) skeys[lpos[i]] = src[base + li];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < kKpt; ++j) {
        const uint32_t p = j * kBlock + t;
        if (p < tile_n) dst[gidx[j]] = skeys[p];
      }
    }
    if (t < R) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) S.whist[w][t] = 0;  // last read before the barrier after the LDS scatter
    }
    __syncthreads();
  }
}

// ---- the generic pass: upsweep -> scan -> downsweep, as the plan's pass k says ----------------------------------------
template <typename KeyT>
void launch_upsweep(pcv_ctx* ctx, const PcvSortPlan& plan, const PcvSortPass& p, const PcvSortSides& s, uint32_t* hist,
                    const uint32_t* map, uint32_t map_entries) {
  const PcvSortGeom& g = plan.geom;
  const uint32_t mask = (1u << p.nbits) - 1u;
  if (p.hist == PCV_HIST_UPSWEEP_MAP) {
    PcvProf prof(ctx, PCV_K_SORT_UPSWEEP_MAP);  // finalize fused into the first upsweep
    const auto kernel = p.map_lds ? (plan.compact ? upsweep_map_kernel<true, true> : upsweep_map_kernel<true, false>)
                                  : (plan.compact ? upsweep_map_kernel<false, true> : upsweep_map_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(g.groups), dim3(kBlock), p.map_lds ? (size_t)map_entries * 4 : 0, ctx->stream, (uint32_t*)s.src,
                       g.n, g.chunk, g.groups, p.shift, mask, hist, map, map_entries, s.vec_in);
    return;
  }
  PcvProf prof(ctx, sizeof(KeyT) == 8 ? PCV_K_SORT_UPSWEEP64 : PCV_K_SORT_UPSWEEP32);
  const auto kernel = p.plain_add ? upsweep_kernel<KeyT, true> : upsweep_kernel<KeyT, false>;
  hipLaunchKernelGGL(kernel, dim3(g.groups), dim3(kBlock), 0, ctx->stream, (const KeyT*)s.src, g.n, g.chunk, g.groups, p.shift, mask,
                     hist);
}

template <typename KeyT>
void launch_downsweep(pcv_ctx* ctx, const PcvSortPlan& plan, int k, const PcvSortSides& s, const PcvSortPayload* payload,
                      const uint32_t* hist, const uint32_t* totals) {
  const PcvSortGeom& g = plan.geom;
  const PcvSortPass& p = plan.pass[k];
  if (p.down == PCV_DOWN_KEYS) {
    PcvProf prof(ctx, sizeof(KeyT) == 8 ? PCV_K_SORT_DOWNSWEEP64 : PCV_K_SORT_DOWNSWEEP32);
    hipLaunchKernelGGL(downsweep_keys_kernel<KeyT>, dim3(g.groups), dim3(kBlock), 0, ctx->stream, (const KeyT*)s.src, (KeyT*)s.dst, g.n,
                       g.chunk, g.groups, p.shift, p.nbits, hist, totals);
    return;
  }
  if (p.down == PCV_DOWN_REC12_CHUNKS) {
    PcvSortRec12Args r;
    r.R = p.R, r.PL = p.PL, r.grid = g.groups;
    r.src = (const uint32_t*)s.src, r.dst = (uint32_t*)s.dst, r.n = g.n, r.chunk = g.chunk, r.shift = p.shift, r.nbits = p.nbits;
    r.hist = hist, r.totals = totals, r.vec_in = s.vec_in, r.vec_out = s.vec_out;
    r.plane_in = s.plane_in, r.plane_out = s.plane_out;
    pcv_sort_launch_rec12(ctx, r);
    return;
  }
  RecPtrs rp{};
  rp.vec_in = s.vec_in, rp.vec_out = s.vec_out;
  rp.nplanes = payload->nwords;
  for (int w = 0; w < payload->nwords; ++w) {
    rp.plane_in[w] = k % 2 == 0 ? payload->in[w] : payload->out[w];
    rp.plane_out[w] = k % 2 == 0 ? payload->out[w] : payload->in[w];
  }
  if (payload->nwords > 0) rp.plane_in[0] = s.plane_in;  // (pass 0: PcvSortPayload::first_in0)
  PcvProf prof(ctx, PCV_K_SORT_DOWNSWEEP_REC);
  const auto kernel = p.down == PCV_DOWN_REC_UINT2   ? downsweep_rec_kernel<true, true, uint2>
                      : p.down == PCV_DOWN_REC_UINT4 ? downsweep_rec_kernel<true, true>
                                                     : downsweep_rec_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(g.groups), dim3(kBlock), 0, ctx->stream, (const uint32_t*)s.src, (uint32_t*)s.dst, g.n, g.chunk,
                     g.groups, p.shift, p.nbits, hist, totals, rp);
}

template <typename KeyT>
void generic_passes(pcv_ctx* ctx, const PcvSortPlan& plan, int first, KeyT* a, KeyT* b, PcvSortPayload* payload, void* scratch,
                    const uint32_t* map, uint32_t map_entries) {
  const PcvSortScratch lay = pcv_sort_scratch(plan.geom.n, pcv_switches().rows_true_bins);
  uint32_t* hist = pcv_sort_scratch_at<uint32_t>(scratch, lay.hist);
  uint32_t* totals = pcv_sort_scratch_at<uint32_t>(scratch, lay.totals);
  for (int k = first; k < plan.npasses; ++k) {
    const PcvSortSides s = pcv_sort_sides(a, b, payload, k);
    launch_upsweep<KeyT>(ctx, plan, plan.pass[k], s, hist, map, map_entries);
    pcv_sort_launch_scan(ctx, hist, plan.geom.groups, totals);
    launch_downsweep<KeyT>(ctx, plan, k, s, payload, hist, totals);
  }
}

template <typename KeyT>
int radix_sort(pcv_ctx* ctx, KeyT* a, KeyT* b, uint64_t n, int begin_bit, int end_bit, PcvSortPayload* payload, void* scratch,
               bool* result_in_a) {
  *result_in_a = true;
  PcvSortPlan plan;
  if (const char* why = pcv_sort_plan(pcv_sort_facts(n, (int)sizeof(KeyT), begin_bit, end_bit, payload), &plan))
    return ctx->fail(PCV_E_INVALID, why);
  if (plan.npasses == 0) return PCV_OK;
  generic_passes<KeyT>(ctx, plan, 0, a, b, payload, scratch, nullptr, 0);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  *result_in_a = plan.result_in_a;
  return PCV_OK;
}

}  // namespace

size_t pcv_sort_scratch_bytes(uint64_t n) { return pcv_sort_scratch(n, pcv_switches().rows_true_bins).end + kPcvSortScratchSlack; }

void pcv_sort_launch_scan(pcv_ctx* ctx, uint32_t* hist, int groups, uint32_t* totals) {
  PcvProf prof(ctx, PCV_K_SORT_SCAN);
  hipLaunchKernelGGL(scan_kernel, dim3(kRadix), dim3(256), 0, ctx->stream, hist, groups, totals);
}
void pcv_sort_generic_passes_u32(pcv_ctx* ctx, const PcvSortPlan& plan, int first, uint32_t* keys_a, uint32_t* keys_b,
                                 PcvSortPayload* payload, void* scratch, const uint32_t* map, uint32_t map_entries) {
  generic_passes<uint32_t>(ctx, plan, first, keys_a, keys_b, payload, scratch, map, map_entries);
}

int pcv_radix_sort_u64(pcv_ctx* ctx, uint64_t* keys_a, uint64_t* keys_b, uint64_t n, int begin_bit, int end_bit,
                       PcvSortPayload* payload, void* scratch, bool* result_in_a) {
  return radix_sort<uint64_t>(ctx, keys_a, keys_b, n, begin_bit, end_bit, payload, scratch, result_in_a);
}
int pcv_radix_sort_u32(pcv_ctx* ctx, uint32_t* keys_a, uint32_t* keys_b, uint64_t n, int begin_bit, int end_bit,
                       PcvSortPayload* payload, void* scratch, bool* result_in_a) {
  return radix_sort<uint32_t>(ctx, keys_a, keys_b, n, begin_bit, end_bit, payload, scratch, result_in_a);
}
