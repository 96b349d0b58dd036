// pcv_sort_dev.h — the device pieces shared by the sort's two sources (pcv_sort.hip, pcv_sort_rec12.hip): the constants of the
// kernels' geometry, the ballot-matched digit count and the digit state, ranking and scan of a downsweep tile. Every kernel is
// compiled in one of the two sources only; the host side of the same constants is pcv_sort_plan.h.
#pragma once
#include "pcv_internal.h"

namespace {

constexpr int kBlock = 256;  // 4 waves
constexpr int kWaves = kBlock / 64;
constexpr int kRadix = kPcvSortRadix;
constexpr int kMaxGroups = kPcvSortMaxGroups;
// records per lane and tile of the record kernel: 16 = tiles of 4 096 records (86 KB of LDS, one workgroup per CU) beat 8
// (three workgroups per CU) by 0.1-0.15 ms per pass at 100 M records — twice as long write runs per digit, a third of
// the concurrent write streams
constexpr int kKptKeys = 16;  // keys-only kernel: keys per lane per tile
constexpr int kKptRec = 16;   // record kernel
constexpr int kKeysWaves = 4;  // waves per SIMD the keys-only kernel / the record kernel with a payload word ask for
constexpr int kRecWaves = 3;
constexpr int lcm_kpt(int a, int b) {
  int x = a, y = b;
  while (y) {
    const int t = x % y;
    x = y;
    y = t;
  }
  return a / x * b;
}
constexpr int kTileUnit = kBlock * lcm_kpt(kKptKeys, kKptRec);  // chunk granularity (multiple of both tile sizes)
static_assert(kTileUnit == kPcvSortTileUnit && kRadix == 256, "pcv_sort_plan.h states the kernels' geometry");

// One histogram update per group of lanes holding the same digit: the lanes are matched with ballots (as in the
// downsweep ranking) and only the first of each group issues the LDS add, with the group size. Plain per-lane LDS
// atomics serialise on equal addresses, and the digits of path keys / leaf ranks are heavily skewed (the upper
// digits take a few dozen values), which cost up to 60 % over uniform keys.
__device__ __forceinline__ void count_digit(uint32_t* __restrict__ wh, uint32_t d, uint64_t valid_mask, bool valid) {
  uint32_t plo = (uint32_t)valid_mask, phi = (uint32_t)(valid_mask >> 32);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    int m;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(d), "n"(b));
    const uint64_t bal = __builtin_amdgcn_ballot_w64(m != 0);
    plo = __builtin_amdgcn_bitop3_b32(plo, (uint32_t)bal, (uint32_t)m, 0x90);  // p & ~(ballot ^ m)
    phi = __builtin_amdgcn_bitop3_b32(phi, (uint32_t)(bal >> 32), (uint32_t)m, 0x90);
  }
  const uint32_t below = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
  if (valid && below == 0) atomicAdd(&wh[d], (uint32_t)(__popc(plo) + __popc(phi)));
}

// ---- shared pieces of the two downsweep kernels -------------------------------------------------

// R: digit values the pass can produce (256, or 128 for digits of <= 7 bits: 3 KB less LDS, which is what lets three
// workgroups of the 12-byte record kernel share a CU); thread t serves digit t, threads >= R only keep the barriers
template <int R = kRadix>
struct DigitState {
  uint32_t whist[kWaves][R];  // per-wave digit counters, then exclusive prefix over the waves
  uint32_t digit_base[R];     // global position of the next key of each digit for this workgroup
  uint32_t delta[R];          // digit_base - (digit's start inside the tile): LDS slot p goes to delta[digit] + p
  uint32_t wave_tot[kWaves];
};

// global base of digit t for this workgroup = (keys with a smaller digit) + (same digit, earlier workgroups)
template <int R>
__device__ __forceinline__ void init_digit_base(DigitState<R>& S, const uint32_t* __restrict__ offsets,
                                                const uint32_t* __restrict__ totals, int groups, int t, int lane, int wave) {
  const uint32_t tot = t < R ? totals[t] : 0u;  // kBlock == kRadix >= R
  uint32_t inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) S.wave_tot[wave] = inc;
  __syncthreads();
  uint32_t woff = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) woff += (w < wave) ? S.wave_tot[w] : 0u;
  if (t < R) {
    S.digit_base[t] = woff + inc - tot + offsets[(uint64_t)t * groups + blockIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) S.whist[w][t] = 0;
  }
  __syncthreads();
}

// Rank of every key of this lane among the earlier keys of the same digit inside the wave's slice of the tile
// (stable: iteration-major, lane-minor == input order). Per key, 8 ballots build the mask of lanes holding the same
// digit; every lane reads the wave's digit counter, then the first lane of the group bumps it by the group size
// (non-returning LDS add). A wave's LDS operations retire in issue order, so the reads and adds of all kKpt
// iterations are issued back to back — no round trip per key — and every read still sees exactly the counts of the
// earlier iterations.
// The kernel is VALU-issue bound (a wave64 op takes 4 clocks on a 16-lane SIMD), so the mask arithmetic is written
// on 32-bit halves in the shape the ISA has single instructions for: one sign-extracting bit-field op per digit bit,
// one compare (the ballot), one three-input bit op per half (p & ~(ballot ^ m)), mbcnt for the lanes below.
template <int kKpt, typename KeyT, bool kFull, int R>
__device__ __forceinline__ void wave_rank_all(DigitState<R>& S, int wave, uint32_t wbase, uint32_t tile_n,
                                              const KeyT (&key)[kKpt], int shift, uint32_t mask, uint16_t (&lpos)[kKpt],
                                              int nbits = 8) {
  constexpr int kBatch = 8;  // adds in flight; more costs registers the 16-keys-per-lane kernel does not have
  static_assert(kKpt % kBatch == 0, "keys per lane must be a multiple of the batch");
#pragma unroll
  for (int i0 = 0; i0 < kKpt; i0 += kBatch) {
    uint32_t pre[kBatch], rank_in[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) {
      const int i = i0 + j;
      const bool valid = kFull || wbase + i * 64 < tile_n;
      const uint32_t d = (uint32_t)(key[i] >> shift) & mask;
      uint32_t plo = 0xffffffffu, phi = 0xffffffffu;
      if (!kFull) {
        const uint64_t vm = __ballot(valid);
        plo = (uint32_t)vm;
        phi = (uint32_t)(vm >> 32);
      }
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        if (b >= 5 && b >= nbits) break;  // narrow digits (wave-uniform): the upper bits are zero in every lane
        int m;  // all ones when bit b of the digit is set (asm: keep the optimiser from re-deriving it the long way)
        asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(d), "n"(b));
        const uint64_t bal = __builtin_amdgcn_ballot_w64(m != 0);
        plo = __builtin_amdgcn_bitop3_b32(plo, (uint32_t)bal, (uint32_t)m, 0x90);  // p & ~(ballot ^ m)
        phi = __builtin_amdgcn_bitop3_b32(phi, (uint32_t)(bal >> 32), (uint32_t)m, 0x90);
      }
      rank_in[j] = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
      uint32_t* slot = &S.whist[wave][d];
      pre[j] = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (valid && rank_in[j] == 0)
        (void)__hip_atomic_fetch_add(slot, (uint32_t)(__popc(plo) + __popc(phi)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#pragma unroll
    for (int j = 0; j < kBatch; ++j) lpos[i0 + j] = (uint16_t)(pre[j] + rank_in[j]);
  }
}

// After all waves ranked their slices: per digit t the exclusive prefix over the waves (folded together with the
// digit's start inside the tile, so the LDS slot of a key is whist[wave][d] + its rank), the global position of the
// digit's run (delta) and the advance of digit_base. Starts and ends with a barrier.
template <int R>
__device__ __forceinline__ void digit_scan(DigitState<R>& S, int t, int lane, int wave) {
  __syncthreads();
  uint32_t pre[kWaves];
  uint32_t acc = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    pre[w] = acc;
    acc += t < R ? S.whist[w][t] : 0u;
  }
  uint32_t inc = acc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t v = __shfl_up(inc, o, 64);
    if (lane >= o) inc += v;
  }
  if (lane == 63) S.wave_tot[wave] = inc;
  __syncthreads();
  uint32_t woff = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) woff += (w < wave) ? S.wave_tot[w] : 0u;
  const uint32_t start = woff + inc - acc;
  if (t < R) {
#pragma unroll
    for (int w = 0; w < kWaves; ++w) S.whist[w][t] = start + pre[w];
    const uint32_t base = S.digit_base[t];
    S.delta[t] = base - start;
    S.digit_base[t] = base + acc;
  }
  __syncthreads();
}

}  // namespace
