// pcv_sort_rec12.hip — the record sort of the single-chain build: 12-byte records (u32 key = rank << 8 | blue, uint2 payload,
// optionally one 4-byte plane) in tiles of 8 192. The downsweep in all its forms (plain, with the rank map applied on the way, in
// pieces of whole first-pass runs, settling the leaves' points itself), the histograms taken from the rank counts instead of the
// keys (the rows form, one pass or two), the one launcher of the downsweep, and the entry points pcv_radix_sort_records_mapped /
// _second. What is launched is planned in pcv_sort_plan.h; scan_kernel and the generic passes are pcv_sort.hip's.
#include <algorithm>

#include "pcv_sort_dev.h"
// (after pcv_internal.h)
#include "pcv_color_stage.h"
#include "pcv_settle_dev.h"

#ifndef PCV_FUSE_DIAG
#define PCV_FUSE_DIAG 0
#endif

namespace {

// ---- 12-byte records, generalised geometry ---------------------------------------------------------------------------
// The same reduce-then-scan downsweep for the packed records of the single-chain build (u32 key + uint2 payload), with
// the workgroup size, the records per lane and the digit-state size as template parameters, so that the occupancy can
// be chosen: the 256-lane / 16-per-lane kernel of pcv_sort.hip needs 235 VGPRs and 54 KB of LDS (two workgroups = 8 waves per CU).
//   BLOCK x KPT = tile (records staged through LDS per round); R = digit values (128 for digits of <= 7 bits);
//   WPE = waves per SIMD the register allocation is asked to admit; NT (unused): non-temporal stores cost 35 %.
// The output phase runs in groups of four LDS reads + four stores (a scheduling barrier between the groups keeps the
// compiler from hoisting all reads of the tile into registers), with the next tile's loads already in flight.
template <int NW, int R>
struct DigitStateN {
  uint32_t whist[NW][R];
  uint32_t digit_base[R];
  uint32_t delta[R];
  uint32_t wave_tot[NW];
};

// MAP (first pass of the single-chain build's record sort when the histogram came from the rank counts, hist_from_rows_kernel):
// the keys still carry PREDICTED leaf ranks; they are translated through the rank map (a copy in dynamic LDS) as they are
// loaded — rank := map[rank], and where the map flags a replayed leaf (bit 30) the record's first payload word becomes its
// input index — which is what upsweep_map_kernel does in a pass of its own otherwise.
// PL (round 5): ONE extra 4-byte plane travels with the record (the intensity of the reference binary's default payload,
// src/bin/build_octree.rs:47-52): 16 bytes per record through the same tiles, 32 KB more LDS.
// WC (round 5, experiment behind PCV_REC_WC in libpcv_hip_exp.so): whole-line write combining. A digit's records leave a tile
// only in 32-record blocks aligned to 32 records of the OUTPUT array (128 bytes of keys, 256 bytes of payloads); what is left
// of a digit's run (< 32 records) waits in a carry buffer in LDS for the next tile of the piece (tools/scatter_probe.hip: runs
// that start on 256-byte boundaries move the same bytes 20-26 % faster than runs at odd record offsets). 128 digit values only
// (48 KB of carry next to the 107 KB of the tile), no plane, no map copy in LDS.
// the settling pass's view of a leaf (one entry per digit value of the piece, in LDS)
struct alignas(16) FuseLeaf {  // 80 bytes: with the intensity plane two workgroups' tables, tiles and digit state fill the CU's LDS
  uint32_t lo, climb_base, flags;
  uint32_t count;      // points of the leaf as the HOST's tree has it: a record outside [lo, lo + count) is never settled here
  uint64_t xyz_off;    // byte offset of the leaf's .xyz content in the xyz blob
  uint64_t point_off;  // point offset of the leaf in the rgb / intensity blobs
  double mn[3], edge, inv_edge, inv_edge_lo;
};
static_assert(sizeof(FuseLeaf) == 80, "leaf table entry");
constexpr uint32_t kFuseSettles = 1u, kFuseU8 = 2u;
// FUSE (PcvSortFuse, pcv_internal.h): the pass is the LAST one of a two-pass sort whose pieces hold one value of the rank's lower
// digit each: a digit's run inside a tile is then ONE leaf's records at consecutive sorted slots. Waves take whole runs: the leaf's
// record comes through the scalar cache, and the run's records leave as final bytes / climber records (flagged leaves) or as
// 12-byte records like in the plain pass (the others: `settle` finishes those).
// PK (first pass of the rows form, no plane): the records are the chain pass's PACKED 8-byte ones — {codes x | y << 16 or the
// pool entry, code z | predicted rank << 16}, no key array — and the colour joins here.
// Its colours are staged: a tile's colours are contiguous bytes of the caller's array, fetched by the whole workgroup as aligned
// 16-byte pieces in front of the NEXT tile's records (pcv_color_stage.h: at most two pieces per lane instead of eight unaligned
// dwords), parked in dynamic LDS behind the map at the end of the iteration, and merged into the records after the ranking's
// barriers, at the LDS scatter.
// !PK: every other form compiles exactly as before the packed form existed (12-byte records with color_in keep their colour loads
// per lane: with the plan they have, a map of 16 384 entries in LDS leaves no room for the colours' buffer).
template <int BLOCK, int KPT, int R, int WPE, bool NT, int MAP, bool PL, bool WC, bool FUSE, bool PK = false>
__device__ __forceinline__ void downsweep_rec12_body(const uint32_t* __restrict__ keys_in, uint32_t* __restrict__ keys_out, uint64_t n,
                                                     uint64_t chunk, int groups, int shift, int nbits, const uint32_t* __restrict__ offsets,
                                                     const uint32_t* __restrict__ totals, const uint2* __restrict__ vec_in,
                                                     uint2* __restrict__ vec_out, const uint32_t* __restrict__ gmap, uint32_t map_entries,
                                                     const uint2* __restrict__ ranges, const uint32_t* __restrict__ order,
                                                     const uint32_t* __restrict__ plane_in, uint32_t* __restrict__ plane_out,
                                                     const PcvSortFuse& fuse, const uint8_t* __restrict__ color_in = nullptr,
                                                     uint32_t color_stride = 3) {
  constexpr int NW = BLOCK / 64, kTile = BLOCK * KPT, RW = R / 64;
  static_assert(!FUSE || (!WC && MAP == 0), "the settling pass: second pass of 12-byte records (+ the intensity plane)");
  constexpr bool kStage = PK, staged = PK;
  static_assert(!kStage || (MAP != 0 && !PL && !WC && !FUSE), "staged colours: first pass of the rows form, no plane");
  // two pieces per lane cover a tile; the one piece more that a full stride-4 tile behind a skewed start needs (the 2 049th)
  // is fetched as sixteen single bytes by sixteen lanes when the pieces are parked: no third piece's four registers
  constexpr int kColRounds = kStage ? 2 : 1;
  static_assert(!kStage || pcv_color_stage_pieces(kTile, 4) <= (uint32_t)(kColRounds * BLOCK + 1), "one piece beyond the rounds at most");
  // the LDS rule of pcv_sort_plan.h rests on this static part
  static_assert(!kStage || sizeof(uint32_t) * kTile + sizeof(uint2) * kTile + sizeof(DigitStateN<NW, R>) == pcv_sort_rec12_static_lds(false, R),
                "pcv_sort_rec12_static_lds");
  __shared__ FuseLeaf sleaf[FUSE ? R : 1];  // FUSE: the leaf of digit value d in this piece: rank = d << low_bits | the piece's lower digit
  const uint32_t piece = order ? order[blockIdx.x] : blockIdx.x;
  static_assert(BLOCK >= R && R % 64 == 0 && KPT % 8 == 0, "geometry");
  __shared__ uint32_t skeys[kTile];
  __shared__ uint2 svec[kTile];
  __shared__ uint32_t splane[PL ? kTile : 1];
  static_assert(!WC || (R == 128 && BLOCK == 1024 && !PL && MAP != 1), "write combining: 128 digit values, 1 024 lanes, no plane, no LDS map");
  __shared__ uint32_t wc_key[WC ? R * 32 : 1];  // carry: the records of digit d at output positions [W_d, W_d + count_d)
  __shared__ uint2 wc_vec[WC ? R * 32 : 1];
  __shared__ uint32_t wc_count[WC ? R : 1], wc_W[WC ? R : 1], wc_gb[WC ? R : 1], wc_A[WC ? R : 1], wc_ts[WC ? R : 1], wc_cnt[WC ? R : 1];
  __shared__ uint32_t wc_seg[WC ? R + 1 : 1];  // exclusive prefix of the digits' block counts of this tile; [R] = their sum
  __shared__ DigitStateN<NW, R> S;
  extern __shared__ __attribute__((aligned(16))) uint16_t smap_dyn[];  // MAP: map_entries half words: true rank (< 2^15) | replay mark << 15
  // the staged colours' buffer behind the map (MAP == 2: there is no map in LDS)
  uint32_t* const scol = reinterpret_cast<uint32_t*>(smap_dyn) + (MAP == 1 ? ((map_entries * 2u + 15u) & ~15u) / 4u : 0u);
  const uint32_t color_low4 = (uint32_t)reinterpret_cast<uintptr_t>(color_in) & 15u;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const uint32_t mask = (1u << nbits) - 1u;
  if (FUSE && t < R) {  // visible after the first barrier below
    const uint32_t r = ((uint32_t)t << fuse.low_bits) | (piece / fuse.blocks);
    FuseLeaf L{};
    if ((uint32_t)t <= mask && r < fuse.num_leaves) {
      const PcvNodeRec c = fuse.leaf_rec[r];
      L.lo = c.lo, L.climb_base = fuse.climb_base[r];
      L.flags = (fuse.leaf_fused[r] ? kFuseSettles : 0u) | (c.enc == PCV_ENC_UINT8 ? kFuseU8 : 0u);
      L.count = (r + 1u < fuse.num_leaves ? fuse.leaf_rec[r + 1u].lo : (uint32_t)n) - c.lo;  // leaves lie in rank order
      L.xyz_off = c.xyz_off, L.point_off = c.point_off;
      L.mn[0] = c.mn[0], L.mn[1] = c.mn[1], L.mn[2] = c.mn[2];
      L.edge = c.edge, L.inv_edge = c.inv_edge, L.inv_edge_lo = c.inv_edge_lo;
    }
    sleaf[t] = L;
  }
  if (MAP == 1)
    for (uint32_t i = t; i < map_entries; i += BLOCK) {  // visible after the first barrier below
      const uint32_t m = gmap[i];
      smap_dyn[i] = (uint16_t)((m & 0x7fffu) | (((m >> 30) & 1u) << 15));
    }
  {  // global base of digit t for this workgroup = (keys with a smaller digit) + (same digit, earlier workgroups)
    const uint32_t tot = t < R ? totals[t] : 0u;
    uint32_t inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o, 64);
      if (lane >= o) inc += v;
    }
    if (lane == 63 && wave < RW) S.wave_tot[wave] = inc;
    __syncthreads();
    uint32_t woff = 0;
#pragma unroll
    for (int w = 0; w < RW; ++w) woff += (w < wave) ? S.wave_tot[w] : 0u;
    if (t < R) S.digit_base[t] = woff + inc - tot + offsets[(uint64_t)t * groups + piece];
    if (WC && t < R) wc_count[t] = 0;
    for (int k = t; k < NW * R; k += BLOCK) (&S.whist[0][0])[k] = 0;
    __syncthreads();
  }
  uint64_t begin = (uint64_t)piece * chunk;
  uint64_t end = begin + chunk;
  if (end > n) end = n;
  if (ranges) {
    begin = ranges[piece].x;
    end = ranges[piece].y;
  }
  const uint32_t wbase = wave * 64 * KPT + lane;

  uint32_t key[KPT];
  uint2 vec[KPT];
  uint32_t pln[PL ? KPT : 1];
  uint4 col[kColRounds];  // staged colours: piece k x BLOCK + t of the tile in flight
  auto load_tile = [&](uint64_t base, uint32_t tile_n) {
    if (kStage && staged) {  // the tile's colour bytes first (they are parked in LDS while the records are still on their way), 16 at a
      // time; only bytes inside the caller's array are touched
      const PcvColorTile ct = pcv_color_tile(color_low4, color_stride, base, tile_n);
#pragma unroll
      for (int k = 0; k < kColRounds; ++k) {
        const uint32_t piece = (uint32_t)(k * BLOCK + t);
        col[k] = make_uint4(0u, 0u, 0u, 0u);
        if (piece < ct.npieces) {
          const PcvColorSpan sp = pcv_color_piece(ct, piece, n, color_stride);
          if (sp.lo == 0u && sp.hi == kPcvColorPiece) {
            col[k] = *reinterpret_cast<const uint4*>(color_in + sp.at);
          } else {  // the array's first / last bytes: one by one
            uint64_t lo8 = 0, hi8 = 0;  // (a short loop, not unrolled: one lane of the grid's first and last tile runs it)
#pragma unroll 1
            for (uint32_t b = sp.lo; b < sp.hi; ++b) {
              const uint64_t v = (uint64_t)color_in[sp.at + (int64_t)b] << (8u * (b & 7u));
              if (b < 8u) lo8 |= v;
              else hi8 |= v;
            }
            col[k] = make_uint4((uint32_t)lo8, (uint32_t)(lo8 >> 32), (uint32_t)hi8, (uint32_t)(hi8 >> 32));
          }
        }
      }
    }
    const uint32_t* __restrict__ kp = PK ? nullptr : keys_in + base + wbase;
    const uint2* __restrict__ vp = vec_in + base + wbase;
    const uint32_t* __restrict__ pp = PL ? plane_in + base + wbase : nullptr;
    if (tile_n == (uint32_t)kTile) {  // full tile: straight-line loads off one base address each
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        if (!PK) key[i] = kp[i * 64];
        vec[i] = vp[i * 64];
        if (PL) pln[i] = pp[i * 64];
      }
    } else {
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const bool valid = wbase + i * 64 < tile_n;
        if (!PK) key[i] = valid ? kp[i * 64] : 0u;
        vec[i] = valid ? vp[i * 64] : make_uint2(0u, 0u);
        if (PL) pln[i] = valid ? pp[i * 64] : 0u;
      }
    }
    if constexpr (PK) {
      // packed records keep their rank where it is, in the upper half of vec.y — the true rank once it has been through the map
      // (< 2^16: the map has at most 65 536 entries) — until the LDS scatter, where the key is made and the red and green bytes
      // take its place: eight registers less across the ranking than a key array
      uint32_t m[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const uint32_t pr = vec[i].y >> 16;
        m[i] = MAP == 1 ? (uint32_t)smap_dyn[pr < map_entries ? pr : 0u] : gmap[pr < map_entries ? pr : 0u];
      }
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const bool replay = MAP == 1 ? (m[i] & 0x8000u) != 0u : (m[i] & (1u << 30)) != 0u;
        if (__builtin_expect(replay, 0)) vec[i].x = (uint32_t)(base + wbase + i * 64);  // replay: the input index
        vec[i].y = (vec[i].y & 0xffffu) | ((MAP == 1 ? (m[i] & 0x7fffu) : (m[i] & PCV_SPEC_INDEX_MASK)) << 16);
      }
      return;
    }
    if (MAP != 0 && color_in && !staged) {  // (wave-uniform) the first pass of records that left the chain pass without their colour
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const uint64_t idx = base + wbase + (uint32_t)(i * 64);
        if (tile_n == (uint32_t)kTile || wbase + i * 64 < tile_n) {
          const uint8_t* c = color_in + idx * color_stride;
          uint32_t rgb;  // r | g << 8 | b << 16 (pcv_load_rgb: one unaligned dword where a fourth byte exists behind the colour)
          if (idx + 1 < n) {
            __builtin_memcpy(&rgb, c, 4);
            rgb &= 0xffffffu;
          } else {
            rgb = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
          }
          key[i] |= rgb >> 16;
          vec[i].y |= (rgb & 0xffffu) << 16;
        }
      }
    }
    if (MAP == 1) {
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const uint32_t pr = key[i] >> 8;
        const uint32_t m = smap_dyn[pr < map_entries ? pr : 0u];
        if (__builtin_expect((m & 0x8000u) != 0u, 0)) vec[i].x = (uint32_t)(base + wbase + i * 64);  // replay: the input index
        key[i] = ((m & 0x7fffu) << 8) | (key[i] & 0xffu);
      }
    }
    if (MAP == 2) {  // trees of more than 16 384 predicted nodes: the map (4 bytes per node, L2-resident) is gathered as it is
      uint32_t m[KPT];
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        const uint32_t pr = key[i] >> 8;
        m[i] = gmap[pr < map_entries ? pr : 0u];
      }
#pragma unroll
      for (int i = 0; i < KPT; ++i) {
        if (__builtin_expect((m[i] & (1u << 30)) != 0u, 0)) vec[i].x = (uint32_t)(base + wbase + i * 64);  // replay: the input index
        key[i] = ((m[i] & PCV_SPEC_INDEX_MASK) << 8) | (key[i] & 0xffu);
      }
    }
  };
  // Staged colours: the pieces in `col` go to the LDS buffer. The first tile's before its ranking; the next tile's at the end of
  // the iteration that requested them, behind that iteration's output phase — the records that read the buffer did so before the
  // LDS scatter, a barrier ago, and the next readers come behind the ranking's barriers: no barrier of their own, and the
  // pieces' registers are free while the ranking needs them.
  auto park_colors = [&](uint64_t base, uint32_t tile_n) {
    const PcvColorTile ct = pcv_color_tile(color_low4, color_stride, base, tile_n);
#pragma unroll
    for (int k = 0; k < kColRounds; ++k) {
      const uint32_t piece = (uint32_t)(k * BLOCK + t);
      if (piece < ct.npieces) reinterpret_cast<uint4*>(scol)[piece] = col[k];
    }
    // (that one piece more: loaded here, where it is parked — sixteen lanes of one wave wait for a byte each, and only for
    // 4-byte colours in an array that is not 16-byte aligned)
    if ((uint32_t)(kColRounds * BLOCK) < ct.npieces && t < (int)kPcvColorPiece) {
      const PcvColorSpan sp = pcv_color_piece(ct, (uint32_t)(kColRounds * BLOCK), n, color_stride);
      const uint32_t b = ((uint32_t)t >= sp.lo && (uint32_t)t < sp.hi) ? (uint32_t)color_in[sp.at + (int64_t)t] : 0u;
      reinterpret_cast<uint8_t*>(scol)[(uint32_t)(kColRounds * BLOCK) * kPcvColorPiece + (uint32_t)t] = (uint8_t)b;
    }
  };
  // the record's digit (PK: out of the rank in the upper half of vec.y; the first pass's shift counts from the key's bit 0)
  auto digit_of = [&](int i) -> uint32_t { return PK ? ((vec[i].y >> 16) >> (shift - 8)) & mask : (key[i] >> shift) & mask; };
  // (MAP: the copy of the map above is complete: the digit-base prologue ended with a barrier)
  if (begin < end) {
    const uint32_t first_n = (uint32_t)((end - begin) < (uint64_t)kTile ? (end - begin) : (uint64_t)kTile);
    load_tile(begin, first_n);
    if (kStage && staged) park_colors(begin, first_n);
  }
  for (uint64_t base = begin; base < end; base += kTile) {
    const uint32_t tile_n = (uint32_t)((end - base) < (uint64_t)kTile ? (end - base) : (uint64_t)kTile);
    const bool full = tile_n == (uint32_t)kTile;
    const uint32_t col_skew = (kStage && staged) ? pcv_color_tile(color_low4, color_stride, base, tile_n).skew : 0u;
    // rank of every record among the earlier records of the same digit inside the wave's slice (see wave_rank_all)
    uint16_t lpos[KPT];
#pragma unroll
    for (int i0 = 0; i0 < KPT; i0 += 8) {
      uint32_t pre[8], rank_in[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = i0 + j;
        const bool valid = full || wbase + i * 64 < tile_n;
        const uint32_t d = digit_of(i);
        uint32_t plo = 0xffffffffu, phi = 0xffffffffu;
        if (!full) {
          const uint64_t vm = __ballot(valid);
          plo = (uint32_t)vm;
          phi = (uint32_t)(vm >> 32);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          if (b >= 5 && b >= nbits) break;
          int m;
          asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(m) : "v"(d), "n"(b));
          const uint64_t bal = __builtin_amdgcn_ballot_w64(m != 0);
          plo = __builtin_amdgcn_bitop3_b32(plo, (uint32_t)bal, (uint32_t)m, 0x90);
          phi = __builtin_amdgcn_bitop3_b32(phi, (uint32_t)(bal >> 32), (uint32_t)m, 0x90);
        }
        rank_in[j] = __builtin_amdgcn_mbcnt_hi(phi, __builtin_amdgcn_mbcnt_lo(plo, 0u));
        uint32_t* slot = &S.whist[wave][d];
        pre[j] = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (valid && rank_in[j] == 0)
          (void)__hip_atomic_fetch_add(slot, (uint32_t)(__popc(plo) + __popc(phi)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) lpos[i0 + j] = (uint16_t)(pre[j] + rank_in[j]);
    }
    // per digit: exclusive prefix over the waves + the digit's start inside the tile; global position of the digit's run
    __syncthreads();
    {
      uint32_t pre[NW];
      uint32_t acc = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        pre[w] = acc;
        acc += t < R ? S.whist[w][t] : 0u;
      }
      // WC: the digit's aligned blocks of this tile are scanned in the upper half word of the same prefix (<= 8 192 records
      // and <= 384 blocks per tile)
      uint32_t wcW = 0, wcA = 0, nseg = 0, gb0 = 0;
      if (WC && t < R) {
        gb0 = S.digit_base[t];
        wcW = gb0 - wc_count[t];
        wcA = (gb0 + acc) & ~31u;
        nseg = wcA > wcW ? (wcA >> 5) - (wcW >> 5) : 0u;
      }
      const uint32_t val = WC ? (acc | (nseg << 16)) : acc;
      uint32_t inc = val;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o, 64);
        if (lane >= o) inc += v;
      }
      if (lane == 63 && wave < RW) S.wave_tot[wave] = inc;
      __syncthreads();
      uint32_t woff = 0;
#pragma unroll
      for (int w = 0; w < RW; ++w) woff += (w < wave) ? S.wave_tot[w] : 0u;
      const uint32_t excl = woff + inc - val;
      const uint32_t start = WC ? (excl & 0xffffu) : excl;
      if (t < R) {
#pragma unroll
        for (int w = 0; w < NW; ++w) S.whist[w][t] = start + pre[w];
        const uint32_t gb = S.digit_base[t];
        S.delta[t] = gb - start;
        S.digit_base[t] = gb + acc;
        if (WC) {
          wc_W[t] = wcW, wc_gb[t] = gb0, wc_A[t] = wcA, wc_ts[t] = start, wc_cnt[t] = acc;
          wc_seg[t] = excl >> 16;
          if (t == R - 1) wc_seg[R] = (excl >> 16) + nseg;
        }
      }
      __syncthreads();
    }
    // red, green, blue of a record out of the parked bytes: the two aligned words around them
    auto staged_rgb = [&](int i) -> uint32_t {
      const uint32_t at = col_skew + (wbase + (uint32_t)(i * 64)) * color_stride;  // pcv_color_record_at
      const uint32_t w0 = scol[at >> 2], w1 = scol[(at >> 2) + 1u];
      return __builtin_amdgcn_alignbyte(w1, w0, at & 3u) & 0xffffffu;  // r | g << 8 | b << 16
    };
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      if (full || wbase + i * 64 < tile_n) {
        const uint32_t d = digit_of(i);
        const uint32_t p = S.whist[wave][d] + lpos[i];
        if constexpr (PK) {
          const uint32_t rgb = staged_rgb(i);
          skeys[p] = ((vec[i].y >> 16) << 8) | (rgb >> 16);
          svec[p] = make_uint2(vec[i].x, (vec[i].y & 0xffffu) | ((rgb & 0xffffu) << 16));
        } else {
          skeys[p] = key[i];
          svec[p] = vec[i];
        }
        if (PL) splane[p] = pln[i];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // the loads below must not be hoisted over the LDS scatter (twice the registers)
    {  // the key / payload registers are free: fetch the next tile while this one drains
      const uint64_t nbase = base + kTile;
      if (nbase < end) load_tile(nbase, (uint32_t)((end - nbase) < (uint64_t)kTile ? (end - nbase) : (uint64_t)kTile));
    }
    __syncthreads();
    if constexpr (WC) {
      // every half wave writes whole 32-record blocks: 128 contiguous, aligned bytes of keys and 256 of payloads
      const uint32_t ns = wc_seg[R];
      const uint32_t l32 = (uint32_t)t & 31u;
      for (uint32_t q = (uint32_t)t >> 5; q < ns; q += BLOCK / 32) {
        uint32_t lo = 0, hi = R;  // the digit of block q: the last one whose prefix is <= q
#pragma unroll
        for (int it = 0; it < 7; ++it) {
          const uint32_t mid = (lo + hi) >> 1;
          if (wc_seg[mid] <= q) lo = mid;
          else hi = mid;
        }
        const uint32_t W = wc_W[lo], gb = wc_gb[lo];
        const uint32_t P = (((W >> 5) + (q - wc_seg[lo])) << 5) + l32;
        if (P >= W) {  // (the first block of a piece's digit may begin inside a line)
          uint32_t k;
          uint2 v;
          if (P < gb) {
            k = wc_key[lo * 32 + (P - W)];
            v = wc_vec[lo * 32 + (P - W)];
          } else {
            const uint32_t src = wc_ts[lo] + (P - gb);
            k = skeys[src];
            v = svec[src];
          }
          keys_out[P] = k;
          vec_out[P] = v;
        }
      }
      __syncthreads();
      {  // what is left of every digit's run goes to (or stays in) its carry: lanes 8 d .. 8 d + 7 serve digit d
        const uint32_t d = (uint32_t)t >> 3;
        const uint32_t c = wc_count[d], W = wc_W[d], gb = wc_gb[d], A = wc_A[d], cnt = wc_cnt[d], ts = wc_ts[d];
        const bool wrote = A > W;
        const uint32_t newc = wrote ? gb + cnt - A : c + cnt;
#pragma unroll
        for (uint32_t k8 = 0; k8 < 4; ++k8) {
          const uint32_t sl = ((uint32_t)t & 7u) + 8u * k8;
          if (wrote ? sl < newc : (sl >= c && sl < newc)) {
            const uint32_t src = wrote ? ts + (A - gb) + sl : ts + (sl - c);
            wc_key[d * 32 + sl] = skeys[src];
            wc_vec[d * 32 + sl] = svec[src];
          }
        }
        if (((uint32_t)t & 7u) == 0u) wc_count[d] = newc;
      }
    } else if constexpr (FUSE) {
      // every lane finishes the records at its own tile positions (consecutive lanes = consecutive sorted slots of a run): the run's
      // leaf comes out of the piece's table in LDS (lanes of one run read one address: a broadcast)
#pragma unroll 2
      for (int i = 0; i < KPT; ++i) {
        const uint32_t p = (uint32_t)i * BLOCK + (uint32_t)t;
        if (!(full || p < tile_n)) continue;
        const uint32_t k = skeys[p];
        const uint2 q = svec[p];
        const uint32_t d = (k >> shift) & mask;
        const FuseLeaf& L = sleaf[d];
        const uint32_t g = S.delta[d] + p;  // sorted slot
        const uint32_t flags = L.flags;
        const uint32_t inten = PL ? splane[p] : 0u;
        // (g - lo < count always holds when the device's rank map and the host's tree agree — the build checks that they do,
        // but only at its end: a record that falls outside its leaf keeps its 12 bytes instead of being written anywhere)
        if (!(flags & kFuseSettles) || g - L.lo >= L.count) {  // `settle` finishes this leaf: the record as in the plain pass
          keys_out[g] = k;
          vec_out[g] = q;
          if (PL) plane_out[g] = inten;
          continue;
        }
        const uint32_t j = g - L.lo;  // position in the leaf's stream
        const uint32_t rgb = (q.y >> 16) | ((k & 0xffu) << 16);
        const uint32_t c0 = q.x & 0xffffu, c1 = q.x >> 16, c2 = q.y & 0xffffu;
        if ((j & 7u) == 0) {  // every eighth point climbs: its record for `climb`, dense per leaf
          if (PL)  // (the leaf's rank: this digit above the piece's lower digit)
            reinterpret_cast<PcvClimber*>(fuse.climbers)[L.climb_base + (j >> 3)] =
                PcvClimber{make_uint4(c0, c1, c2, rgb), (d << fuse.low_bits) | (piece / fuse.blocks), g, inten, 0u};
          else reinterpret_cast<uint4*>(fuse.climbers)[L.climb_base + (j >> 3)] = make_uint4(c0, c1, c2, rgb);
          continue;
        }
        // final rewrite encode(decode(code)) at the leaf's own level (promote_final, pcv_settle_dev.h) with the
        // encoding's constants as per-lane values: the same operations in the same order for u8 and u16
        const bool u8 = (flags & kFuseU8) != 0;
        const double maxval = u8 ? 255.0 : 65535.0;
        const PcvRecip rm = u8 ? PCV_RECIP_255 : PCV_RECIP_65535;
        uint32_t out[3];
        const uint32_t cin[3] = {c0, c1, c2};
#if PCV_FUSE_DIAG == 2
        out[0] = c0, out[1] = c1, out[2] = c2;
        if (L.inv_edge == 123.0) {
#else
        if (__builtin_expect(L.inv_edge != 0.0, 1)) {
#endif
          const PcvRecip ie{L.inv_edge, L.inv_edge_lo};
#pragma unroll
          for (int a = 0; a < 3; ++a)
            out[a] = pcv_fix_encode<false>(__fma_rn(pcv_div_code((double)cin[a], rm), L.edge, L.mn[a]), L.mn[a], L.edge, ie, maxval);
#if PCV_FUSE_DIAG == 2
        } else if (L.inv_edge == 124.0) {
#else
        } else {
#endif
          const uint32_t enc = u8 ? PCV_ENC_UINT8 : PCV_ENC_UINT16;
#pragma unroll
          for (int a = 0; a < 3; ++a)
            out[a] = (uint32_t)pcv_encode_coord(enc, pcv_decode_coord(enc, cin[a], L.mn[a], L.edge), L.mn[a], L.edge, PcvRecip{0.0, 0.0});
        }
        const uint32_t slot = j - (j >> 3) - 1u;
        const bool odd = (slot & 1u) != 0;
#if PCV_FUSE_DIAG == 1  // (timing experiments, tools/build_variants.sh: 1 = no final stores, 2 = no rewrite; never shipped)
        if (out[0] != 0x7fffffffu) continue;
#endif
        const uint64_t pidx = L.point_off + slot;
        if (PL) reinterpret_cast<uint32_t*>(fuse.inten_blob)[pidx] = inten;
        // 3 bytes at 3 x pidx: one 2-byte store at the EVEN address of the three + one byte. The parity is the address's, i.e.
        // pidx's, not slot's: a leaf's point_off may be odd (the .xyz stores below may use slot's, xyz_off is
        // 16-byte aligned)
        uint8_t* cd = fuse.rgb_blob + pidx * 3;
        const bool odd_rgb = (pidx & 1u) != 0;
        *reinterpret_cast<uint16_t*>(cd + (odd_rgb ? 1 : 0)) = (uint16_t)(odd_rgb ? rgb >> 8 : rgb);
        cd[odd_rgb ? 0 : 2] = (uint8_t)(odd_rgb ? rgb : rgb >> 16);
        if (u8) {
          uint8_t* x = fuse.xyz_blob + L.xyz_off + (uint64_t)slot * 3;
          *reinterpret_cast<uint16_t*>(x + (odd ? 1 : 0)) = (uint16_t)(odd ? out[1] | (out[2] << 8) : out[0] | (out[1] << 8));
          x[odd ? 0 : 2] = (uint8_t)(odd ? out[0] : out[2]);
        } else {  // 6 bytes at 6 x slot: one 4-byte store at the 4-aligned address of the six + one 2-byte store
          uint8_t* x = fuse.xyz_blob + L.xyz_off + (uint64_t)slot * 6;
          *reinterpret_cast<uint32_t*>(x + (odd ? 2 : 0)) = odd ? out[1] | (out[2] << 16) : out[0] | (out[1] << 16);
          *reinterpret_cast<uint16_t*>(x + (odd ? 0 : 4)) = (uint16_t)(odd ? out[0] : out[2]);
        }
      }
    } else {
#pragma unroll
    for (int j0 = 0; j0 < KPT; j0 += 4) {
      uint32_t k4[4];
      uint2 v4[4];
      uint32_t p4[PL ? 4 : 1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p = (j0 + j) * BLOCK + t;
        k4[j] = skeys[p];
        v4[j] = svec[p];
        if (PL) p4[j] = splane[p];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p = (j0 + j) * BLOCK + t;
        if (full || p < tile_n) {
          const uint32_t g = S.delta[(k4[j] >> shift) & mask] + p;
          keys_out[g] = k4[j];
          vec_out[g] = v4[j];
          if (PL) plane_out[g] = p4[j];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    }
    if (kStage && staged) {
      const uint64_t nbase = base + kTile;
      if (nbase < end) park_colors(nbase, (uint32_t)((end - nbase) < (uint64_t)kTile ? (end - nbase) : (uint64_t)kTile));
    }
    for (int k = t; k < NW * R; k += BLOCK) (&S.whist[0][0])[k] = 0;  // last read before the barrier above
    __syncthreads();
  }
  if constexpr (WC) {  // end of the piece: the carries leave as they are (the tail of every digit's run)
    const uint32_t d = (uint32_t)t >> 3;
    const uint32_t c = wc_count[d], W = S.digit_base[d] - c;
#pragma unroll
    for (uint32_t k8 = 0; k8 < 4; ++k8) {
      const uint32_t sl = ((uint32_t)t & 7u) + 8u * k8;
      if (sl < c) {
        keys_out[W + sl] = wc_key[d * 32 + sl];
        vec_out[W + sl] = wc_vec[d * 32 + sl];
      }
    }
  }
}


template <int BLOCK, int KPT, int R, int WPE, bool NT, int MAP = 0 /* 1: the map in LDS (half words), 2: in global memory */, bool PL = false,
          bool WC = false, bool PK = false /* packed 8-byte records in vec_in, keys_in unused; the colours staged through LDS */>
__global__ __launch_bounds__(BLOCK, WPE) void downsweep_rec12_kernel(const uint32_t* __restrict__ keys_in,
                                                                     uint32_t* __restrict__ keys_out, uint64_t n, uint64_t chunk,
                                                                     int groups, int shift, int nbits,
                                                                     const uint32_t* __restrict__ offsets,
                                                                     const uint32_t* __restrict__ totals,
                                                                     const uint2* __restrict__ vec_in, uint2* __restrict__ vec_out,
                                                                     const uint32_t* __restrict__ gmap = nullptr, uint32_t map_entries = 0,
                                                                     const uint2* __restrict__ ranges = nullptr /* set: piece k
                                                                     = the records [ranges[k].x, ranges[k].y) instead of chunk k */,
                                                                     const uint32_t* __restrict__ order = nullptr /* set: workgroup
                                                                     b takes piece order[b] (largest pieces first) */,
                                                                     const uint32_t* __restrict__ plane_in = nullptr,
                                                                     uint32_t* __restrict__ plane_out = nullptr,
                                                                     const uint8_t* __restrict__ color_in = nullptr /* MAP != 0: the
                                                                     records come without colour, record i's is here */,
                                                                     uint32_t color_stride = 3) {
  downsweep_rec12_body<BLOCK, KPT, R, WPE, NT, MAP, PL, WC, false, PK>(keys_in, keys_out, n, chunk, groups, shift, nbits, offsets, totals,
                                                                       vec_in, vec_out, gmap, map_entries, ranges, order, plane_in, plane_out,
                                                                       PcvSortFuse(), color_in, color_stride);
}
// the settling form of the second pass (FUSE above): a kernel of its own name for the profiles
// (R = 128 digit values: the second digit of a rank of <= 15 bits has <= 7 bits; 256 for ranks of 16 bits)
template <bool PL, int BLOCK = 1024, int R = 128>
__global__ __launch_bounds__(BLOCK, 4) void downsweep_settle_kernel(const uint32_t* __restrict__ keys_in, uint32_t* __restrict__ keys_out,
                                                                   uint64_t n, uint64_t chunk, int groups, int shift, int nbits,
                                                                   const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ totals,
                                                                   const uint2* __restrict__ vec_in, uint2* __restrict__ vec_out,
                                                                   const uint2* __restrict__ ranges, const uint32_t* __restrict__ order,
                                                                   const uint32_t* __restrict__ plane_in, uint32_t* __restrict__ plane_out,
                                                                   PcvSortFuse fuse) {
  downsweep_rec12_body<BLOCK, 8, R, 4, false, 0, PL, false, true>(keys_in, keys_out, n, chunk, groups, shift, nbits, offsets, totals, vec_in,
                                                                   vec_out, nullptr, 0u, ranges, order, plane_in, plane_out, fuse);
}

// First-pass histogram of the record sort from the per-workgroup rank counts (rank_hist rows, pcv_encode.hip) and the rank map:
// workgroup g's count of digit d = sum over the predicted leaves b whose TRUE rank has digit d of rows[g][b]. One workgroup
// per sort workgroup; the keys are not read.
__global__ __launch_bounds__(256) void hist_from_rows_kernel(const uint32_t* __restrict__ rows, uint32_t nbins,
                                                              const uint32_t* __restrict__ map, int rank_shift, uint32_t mask, int groups,
                                                              uint32_t* __restrict__ hist /* [digit][groups] */) {
  __shared__ uint32_t h[kRadix];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t* row = rows + (uint64_t)blockIdx.x * nbins;
  for (uint32_t b = threadIdx.x; b < nbins; b += 256) {
    const uint32_t c = row[b];
    if (c) atomicAdd(&h[((map[b] & PCV_SPEC_INDEX_MASK) >> rank_shift) & mask], c);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * groups + blockIdx.x] = threadIdx.x <= mask ? h[threadIdx.x] : 0u;  // all kRadix rows are scanned
}

// Two-pass sorts: BOTH histograms from the rank counts. Per sort workgroup g the counts are re-indexed by TRUE rank, lower
// digit major — tr[d1 * D2 + d2] — and kept (rows_true[g][.]); the first pass's histogram is their sum over d2. The first
// pass writes its output ordered by (d1, g); the second pass cuts THAT sequence into pieces of whole runs — piece k = digit
// d1 = k / blocks, workgroups [blk * gpb, (blk + 1) * gpb) of the first pass — so a piece's digit counts are sums of
// rows_true entries and its record range follows from the first pass's offsets: the second pass needs no counting pass over
// the keys either (pass2_layout_kernel). Pieces differ in size (by the popularity of d1) instead of being equal chunks.
__global__ __launch_bounds__(256) void hist12_from_rows_kernel(const uint32_t* __restrict__ rows, uint32_t nbins,
                                                                const uint32_t* __restrict__ map, int nbits1, int nbits2, int groups,
                                                                uint32_t* __restrict__ hist1 /* [d1][groups] */,
                                                                uint32_t* __restrict__ rows_true /* [groups][D1 * D2] */,
                                                                int msd /* experiments: the FIRST pass takes the rank's upper nbits1 bits */) {
  extern __shared__ uint32_t tr[];  // D1 x D2 counters: 64 KB for ranks of 14 bits, 128 KB for 15; 16 bits: two rounds of 128 KB
  const uint32_t D1 = 1u << nbits1, D2 = 1u << nbits2, TB = D1 * D2;
  const int sh1 = msd ? nbits2 : 0, sh2 = msd ? 0 : nbits1;
  const uint32_t rounds = TB > 32768u ? TB / 32768u : 1u, D1r = D1 / rounds, TBr = D1r * D2;  // a round takes D1r values of the first digit
  const uint32_t* row = rows + (uint64_t)blockIdx.x * nbins;
  uint32_t* out = rows_true + (uint64_t)blockIdx.x * TB;
  hist1[(uint64_t)threadIdx.x * groups + blockIdx.x] = 0;  // all kRadix rows are scanned (digit values >= D1 stay empty)
  for (uint32_t rd = 0; rd < rounds; ++rd) {
    const uint32_t d1_lo = rd * D1r;
    for (uint32_t i = threadIdx.x; i < TBr; i += 256) tr[i] = 0;
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < nbins; b += 256) {
      const uint32_t c = row[b];
      if (c) {
        const uint32_t r = map[b] & PCV_SPEC_INDEX_MASK;
        const uint32_t d1 = ((r >> sh1) & (D1 - 1u)) - d1_lo;
        if (d1 < D1r) atomicAdd(&tr[d1 * D2 + ((r >> sh2) & (D2 - 1u))], c);
      }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TBr; i += 256) out[(uint64_t)d1_lo * D2 + i] = tr[i];
    if (threadIdx.x < D1r) {
      uint32_t s = 0;
      for (uint32_t d2 = 0; d2 < D2; ++d2) s += tr[threadIdx.x * D2 + ((d2 + threadIdx.x) & (D2 - 1u))];  // skewed: no bank conflict
      hist1[(uint64_t)(d1_lo + threadIdx.x) * groups + blockIdx.x] = s;
    }
    __syncthreads();
  }
}
// piece k of the second pass (see above): its digit counts and its record range. offsets1 / totals1: the first pass's scanned
// histogram. One workgroup of 256 lanes per piece.
__global__ __launch_bounds__(256) void pass2_layout_kernel(const uint32_t* __restrict__ rows_true, int nbits1, int nbits2, int groups,
                                                            int blocks, int gpb, const uint32_t* __restrict__ offsets1,
                                                            const uint32_t* __restrict__ totals1, int pieces,
                                                            uint32_t* __restrict__ hist2 /* [d2][pieces] */, uint2* __restrict__ ranges,
                                                            uint32_t* __restrict__ order /* pieces by falling size of their digit */) {
  __shared__ uint32_t part[4][256];
  const uint32_t D1 = 1u << nbits1, D2 = 1u << nbits2, TB = D1 * D2;
  const int k = blockIdx.x, d1 = k / blocks, blk = k % blocks;
  const int g_lo = blk * gpb, g_hi = (g_lo + gpb < groups) ? g_lo + gpb : groups;
  const uint32_t d2 = threadIdx.x & (D2 - 1u), lanes_per_g = 256u / D2, sub = threadIdx.x / D2;  // D2 <= 256
  uint32_t s = 0;
  for (int g = g_lo + (int)sub; g < g_hi; g += (int)lanes_per_g) s += rows_true[(uint64_t)g * TB + (uint32_t)d1 * D2 + d2];
  (&part[0][0])[threadIdx.x] = s;
  __syncthreads();
  {
    uint32_t tot = 0;
    if (threadIdx.x < D2)
      for (uint32_t q = 0; q < lanes_per_g; ++q) tot += (&part[0][0])[q * D2 + threadIdx.x];
    hist2[(uint64_t)threadIdx.x * pieces + k] = tot;  // all kRadix rows are scanned
  }
  if (threadIdx.x == 0) {
    uint32_t start = 0;  // records with a smaller first digit
    for (int d = 0; d < d1; ++d) start += totals1[d];
    const uint32_t b = g_lo < groups ? start + offsets1[(uint64_t)d1 * groups + g_lo] : start + totals1[d1];
    const uint32_t e = g_hi < groups ? start + offsets1[(uint64_t)d1 * groups + g_hi] : start + totals1[d1];
    ranges[k] = make_uint2(b, e);
    // launch order: the pieces of the most popular first digits first (a piece's size follows its digit's total)
    const uint32_t mine = totals1[d1];
    uint32_t before = 0;
    for (int d = 0; d < (int)D1; ++d) {
      const uint32_t o = totals1[d];
      before += (o > mine || (o == mine && d < d1)) ? 1u : 0u;
    }
    order[before * (uint32_t)blocks + (uint32_t)blk] = (uint32_t)k;
  }
}

// (experiments, PCV_SORT_MSD) Most significant digit FIRST: the second pass then sorts every bucket of the first one by the lower
// digit INSIDE the bucket's own range of the output. hist2[d2][piece] (piece = (d1, blk)) turns into the absolute position of
// that (digit, piece) run: start of bucket d1 + records of the bucket with a smaller d2 + same d2, earlier blocks; the
// downsweep's digit prefix (totals) is zeroed. One workgroup per first digit.
__global__ __launch_bounds__(256) void msd_offsets_kernel(uint32_t* __restrict__ hist2, int pieces, int blocks, int nbits2,
                                                           const uint32_t* __restrict__ totals1, uint32_t* __restrict__ totals2) {
  __shared__ uint32_t wave_tot[4];
  const int d1 = blockIdx.x;
  const uint32_t D2 = 1u << nbits2, total = D2 * (uint32_t)blocks;
  if (d1 == 0) totals2[threadIdx.x] = 0;  // kRadix == 256 entries
  uint32_t start = 0;
  for (int d = 0; d < d1; ++d) start += totals1[d];
  const uint32_t per = (total + 255u) / 256u;
  uint32_t running = start;  // (uniform) everything before the chunk of 256 x per values in flight
  // value i of the bucket's sequence: digit i / blocks, block i % blocks
  auto at = [&](uint32_t i) -> uint32_t& { return hist2[(uint64_t)(i / (uint32_t)blocks) * pieces + (uint32_t)d1 * blocks + i % (uint32_t)blocks]; };
  const uint32_t begin = threadIdx.x * per;
  uint32_t sum = 0;
  for (uint32_t i = 0; i < per; ++i)
    if (begin + i < total) sum += at(begin + i);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t woff = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) woff += (w < wave) ? wave_tot[w] : 0u;
  uint32_t run = running + woff + inc - sum;
  for (uint32_t i = 0; i < per; ++i)
    if (begin + i < total) {
      uint32_t& v = at(begin + i);
      const uint32_t c = v;
      v = run;
      run += c;
    }
}

// Geometry of the 12-byte record downsweep. What moves this kernel is the length of the write runs (tile / digit
// values), not the occupancy (r03a / r03d A/B at 100 M records, both passes together, one box per line):
//   tiles of 4 096: 256 lanes x 16 at 8 waves per CU 1.36-1.40 ms, at 12 waves per CU 1.40, 512 x 8 at 16 waves per CU 1.36
//   tiles of 8 192: 1 024 x 8 1.20 ms (ships), 512 x 16 1.25; non-temporal stores +35 %
//   tiles of 16 384 by staging keys and payloads one after the other through the same LDS: 1.27-1.29 against 1.01-1.11
//   (two more barriers per tile, one workgroup per CU) — dropped
template <int R, int MAP, bool PL, bool WC = false, bool PK = false>
void launch_rec12(pcv_ctx* ctx, const PcvSortRec12Args& a) {
  const auto kernel = downsweep_rec12_kernel<1024, 8, R, 4, false, MAP, PL, WC, PK>;
  // dynamic LDS (the map, the staged colours): once per instantiation, the size from the tables the plan's limits come from
  if constexpr (MAP == 1 || PK) {
    static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)(PK ? pcv_sort_rec12_dyn_attr(R) : pcv_sort_map_lds(PL, R).attr_bytes)) == hipSuccess;
    (void)ok;
  }
  hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(1024), a.dyn_lds + a.color_lds, ctx->stream, a.src, a.dst, a.n, a.chunk, a.grid, a.shift,
                     a.nbits, a.hist, a.totals, (const uint2*)a.vec_in, (uint2*)a.vec_out, a.map, a.map_entries, (const uint2*)a.ranges, a.order,
                     a.plane_in, a.plane_out, a.color_in, a.color_stride);
}
template <bool PL, int BLOCK, int R>
void launch_settle(pcv_ctx* ctx, const PcvSortRec12Args& a) {
  hipLaunchKernelGGL((downsweep_settle_kernel<PL, BLOCK, R>), dim3(a.grid), dim3(BLOCK), 0, ctx->stream, a.src, a.dst, a.n, a.chunk, a.grid,
                     a.shift, a.nbits, a.hist, a.totals, (const uint2*)a.vec_in, (uint2*)a.vec_out, (const uint2*)a.ranges, a.order,
                     a.plane_in, a.plane_out, *a.fuse);
}

PcvSortRec12Args rec12_args(const PcvSortPlan& plan, const PcvSortPass& p, const PcvSortSides& s, const uint32_t* hist,
                            const uint32_t* totals) {
  PcvSortRec12Args r;
  r.R = p.R, r.MAP = p.MAP, r.PL = p.PL, r.dyn_lds = p.dyn_lds;
  r.PK = p.packed, r.color_lds = p.color_lds;
  r.grid = p.down == PCV_DOWN_REC12_PIECES ? plan.pieces : plan.geom.groups;
  r.src = (const uint32_t*)s.src, r.dst = (uint32_t*)s.dst, r.n = plan.geom.n, r.chunk = plan.geom.chunk;
  r.shift = p.shift, r.nbits = p.nbits, r.hist = hist, r.totals = totals;
  r.vec_in = s.vec_in, r.vec_out = s.vec_out, r.plane_in = s.plane_in, r.plane_out = s.plane_out;
  return r;
}

// The second pass of the two-pass rows form: its layout — pieces of whole first-pass runs, digit counts and ranges from rows_true
// and the first pass's scanned histogram, two small kernels that need the histograms and not the first pass — on the side stream
// BESIDE the first pass where the pass is held back; then the pass itself, or what pcv_radix_sort_records_second needs for it.
void rows_second_pass(pcv_ctx* ctx, const PcvSortPlan& plan, uint32_t* a, uint32_t* b, const PcvSortPayload* payload, void* scratch,
                      const PcvSortScratch& lay, bool side_layout, PcvSortSecond* second) {
  const PcvSortPass &p1 = plan.pass[0], &p2 = plan.pass[1];
  uint32_t* hist2 = pcv_sort_scratch_at<uint32_t>(scratch, lay.hist2);
  uint32_t* totals2 = pcv_sort_scratch_at<uint32_t>(scratch, lay.totals2);
  uint2* ranges = pcv_sort_scratch_at<uint2>(scratch, lay.ranges);
  uint32_t* order = pcv_sort_scratch_at<uint32_t>(scratch, lay.order);
  const uint32_t* totals = pcv_sort_scratch_at<uint32_t>(scratch, lay.totals);
  if (side_layout) std::swap(ctx->stream, ctx->side);
  {
    PcvProf prof(ctx, PCV_K_SORT_HIST_ROWS);
    hipLaunchKernelGGL(pass2_layout_kernel, dim3(plan.pieces), dim3(256), 0, ctx->stream, pcv_sort_scratch_at<uint32_t>(scratch, lay.rows_true),
                       p1.nbits, p2.nbits, plan.geom.groups, plan.blocks, plan.gpb, pcv_sort_scratch_at<uint32_t>(scratch, lay.hist), totals,
                       plan.pieces, hist2, ranges, order);
  }
  if (plan.msd) {  // absolute positions of every (digit, piece) run inside its bucket; no digit prefix
    PcvProf prof(ctx, PCV_K_SORT_SCAN);
    hipLaunchKernelGGL(msd_offsets_kernel, dim3(1 << p1.nbits), dim3(256), 0, ctx->stream, hist2, plan.pieces, plan.blocks, p2.nbits, totals,
                       totals2);
  } else {
    pcv_sort_launch_scan(ctx, hist2, plan.pieces, totals2);
  }
  if (side_layout) std::swap(ctx->stream, ctx->side);
  PcvSortRec12Args r = rec12_args(plan, p2, pcv_sort_sides(a, b, payload, 1), hist2, totals2);
  r.ranges = ranges, r.order = order;
  if (plan.held_back) {  // the caller queues the pass itself (pcv_radix_sort_records_second)
    second->pending = true;
    second->join_side = side_layout;
    second->src = r.src, second->dst = r.dst, second->vec_src = r.vec_in, second->vec_dst = r.vec_out;
    second->plane_src = r.plane_in, second->plane_dst = r.plane_out;
    second->n = r.n, second->chunk = r.chunk;
    second->pieces = plan.pieces, second->shift = p2.shift, second->nbits = p2.nbits;
    second->low_bits = p1.nbits, second->blocks = plan.blocks;
    second->hist = hist2, second->totals = totals2, second->order = order, second->ranges = ranges;
    return;
  }
#ifdef PCV_EXPERIMENTS
  r.WC = (pcv_switches().rec_wc & 2) && !plan.with_plane && p2.nbits <= 7;
#endif
  pcv_sort_launch_rec12(ctx, r);
}

// The rows form: the first pass's histogram from the rank counts (both passes' in the two-pass form) -> scan -> first pass, the
// rank map applied as the records are loaded -> the second pass, if the sort has exactly two (rows_second_pass).
void rows_form(pcv_ctx* ctx, const PcvSortPlan& plan, uint32_t* a, uint32_t* b, const PcvSortPayload* payload, void* scratch,
               const uint32_t* map, uint32_t map_entries, const uint32_t* rows, PcvSortSecond* second) {
  const PcvSortPass& p1 = plan.pass[0];
  const PcvSortGeom& g = plan.geom;
  const PcvSortScratch lay = pcv_sort_scratch(g.n, pcv_switches().rows_true_bins);
  uint32_t* hist = pcv_sort_scratch_at<uint32_t>(scratch, lay.hist);
  uint32_t* totals = pcv_sort_scratch_at<uint32_t>(scratch, lay.totals);
  {
    PcvProf prof(ctx, PCV_K_SORT_HIST_ROWS);
    if (plan.two_pass) {  // (msd: the first pass takes the rank's upper digit, the second the lower one)
      static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(&hist12_from_rows_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, 131072) == hipSuccess;
      (void)ok;
      const int p2_bits = plan.pass[1].nbits;
      hipLaunchKernelGGL(hist12_from_rows_kernel, dim3(g.groups), dim3(256), std::min<size_t>((size_t)4 << (p1.nbits + p2_bits), 131072),
                         ctx->stream, rows, map_entries, map, p1.nbits, p2_bits, g.groups, hist,
                         pcv_sort_scratch_at<uint32_t>(scratch, lay.rows_true), plan.msd ? 1 : 0);
    } else {  // (the rank's lowest digit)
      hipLaunchKernelGGL(hist_from_rows_kernel, dim3(g.groups), dim3(256), 0, ctx->stream, rows, map_entries, map, 0, (1u << p1.nbits) - 1u,
                         g.groups, hist);
    }
  }
  pcv_sort_launch_scan(ctx, hist, g.groups, totals);
  // held-back second pass: its layout runs on the side stream; pcv_radix_sort_records_second joins the streams in front of the pass
  const bool side_layout = plan.held_back && ctx->side && ctx->side_begin() == PCV_OK;
  PcvSortRec12Args r = rec12_args(plan, p1, pcv_sort_sides(a, b, payload, 0), hist, totals);
  r.map = map, r.map_entries = map_entries;
  r.color_in = payload->color_in, r.color_stride = payload->color_stride;
#ifdef PCV_EXPERIMENTS
  // rec_wc (bit 0: first pass, bit 1: second pass): the write-combining form of the downsweep measured slower than the kernel
  // that ships (profiles/r05_sort_same_box.json): not instantiated in libpcv_hip.so
  r.WC = (pcv_switches().rec_wc & 1) && !plan.with_plane && p1.nbits <= 7 && !payload->color_in;
  if (r.WC) r.MAP = 2, r.dyn_lds = 0, r.color_lds = 0;  // (that form gathers the map from global memory)
#endif
  pcv_sort_launch_rec12(ctx, r);
  if (plan.two_pass) rows_second_pass(ctx, plan, a, b, payload, scratch, lay, side_layout, second);
}

}  // namespace

// One launcher for every form of the 12-byte record downsweep: exactly the instantiations below exist.
void pcv_sort_launch_rec12(pcv_ctx* ctx, const PcvSortRec12Args& a) {
  if (a.fuse) {
    PcvProf prof(ctx, PCV_K_SORT_SETTLE);
    switch (pcv_sort_settle_form(a.nbits, a.plane_in != nullptr)) {
      case PCV_SETTLE_512: return launch_settle<false, 512, 128>(ctx, a);
      case PCV_SETTLE_1024_PLANE: return launch_settle<true, 1024, 128>(ctx, a);
      case PCV_SETTLE_1024_R256: return launch_settle<false, 1024, 256>(ctx, a);
    }
    return;
  }
  PcvProf prof(ctx, PCV_K_SORT_DOWNSWEEP_REC);
#ifdef PCV_EXPERIMENTS
  if (a.WC) return a.MAP ? launch_rec12<128, 2, false, true>(ctx, a) : launch_rec12<128, 0, false, true>(ctx, a);
#endif
  if (a.PK) {  // the chain pass's packed records (planned for the rows form without a plane only)
    if (a.MAP == 1) return a.R == 256 ? launch_rec12<256, 1, false, false, true>(ctx, a) : launch_rec12<128, 1, false, false, true>(ctx, a);
    return a.R == 256 ? launch_rec12<256, 2, false, false, true>(ctx, a) : launch_rec12<128, 2, false, false, true>(ctx, a);
  }
  switch ((a.MAP << 2) | (a.R == 256 ? 2 : 0) | (a.PL ? 1 : 0)) {
    case 0: return launch_rec12<128, 0, false>(ctx, a);
    case 1: return launch_rec12<128, 0, true>(ctx, a);
    case 2: return launch_rec12<256, 0, false>(ctx, a);
    case 3: return launch_rec12<256, 0, true>(ctx, a);
    case 4: return launch_rec12<128, 1, false>(ctx, a);
    case 5: return launch_rec12<128, 1, true>(ctx, a);
    case 6: return launch_rec12<256, 1, false>(ctx, a);
    case 7: return launch_rec12<256, 1, true>(ctx, a);
    case 8: return launch_rec12<128, 2, false>(ctx, a);
    case 9: return launch_rec12<128, 2, true>(ctx, a);
    case 10: return launch_rec12<256, 2, false>(ctx, a);
    case 11: return launch_rec12<256, 2, true>(ctx, a);
  }
}

// Record sort whose first pass also translates the ranks through `map` (single-chain build); 12-byte records
// (payload->vec_bytes == 8): the rank sits in bits 8.. of the key
int pcv_radix_sort_records_mapped(pcv_ctx* ctx, uint32_t* keys_a, uint32_t* keys_b, uint64_t n, int key_bits,
                                  PcvSortPayload* payload, void* scratch, const uint32_t* map, uint32_t map_entries,
                                  bool* result_in_a, const uint32_t* rows, PcvSortSecond* second) {
  *result_in_a = true;
  if (second) second->pending = false;
  const int base = payload && payload->vec_bytes == 8 ? 8 : 0;
  PcvSortFacts f = pcv_sort_facts(n, 4, base, base + key_bits, payload);
  f.map = map != nullptr, f.map_entries = map_entries, f.rows = rows != nullptr, f.second = second != nullptr;
  PcvSortPlan plan;
  if (const char* why = pcv_sort_plan(f, &plan)) return ctx->fail(PCV_E_INVALID, why);
  if (plan.npasses == 0) return PCV_OK;
  int first = 0;
  if (plan.pass[0].hist == PCV_HIST_ROWS || plan.pass[0].hist == PCV_HIST_ROWS_TRUE) {
    rows_form(ctx, plan, keys_a, keys_b, payload, scratch, map, map_entries, rows, second);
    first = plan.two_pass ? 2 : 1;
  }
  pcv_sort_generic_passes_u32(ctx, plan, first, keys_a, keys_b, payload, scratch, map, map_entries);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  *result_in_a = plan.result_in_a;
  return PCV_OK;
}

int pcv_radix_sort_records_second(pcv_ctx* ctx, PcvSortSecond* sd, const PcvSortFuse* fuse) {
  if (!sd || !sd->pending) return PCV_OK;
  sd->pending = false;
  if (sd->join_side && ctx->side_end() != PCV_OK) return ctx->fail(PCV_E_HIP, "record sort: side stream");
  const bool plane = sd->plane_src != nullptr;
  PcvSortRec12Args r;
  r.R = sd->nbits <= 7 ? 128 : 256, r.PL = plane, r.grid = sd->pieces;
  r.src = sd->src, r.dst = sd->dst, r.n = sd->n, r.chunk = sd->chunk, r.shift = sd->shift, r.nbits = sd->nbits;
  r.hist = sd->hist, r.totals = sd->totals, r.vec_in = sd->vec_src, r.vec_out = sd->vec_dst;
  r.plane_in = sd->plane_src, r.plane_out = sd->plane_dst, r.ranges = sd->ranges, r.order = sd->order;
  PcvSortFuse fz;
  if (fuse && pcv_sort_second_settles(sd->nbits, plane, fuse->inten_blob != nullptr)) {
    fz = *fuse;
    fz.low_bits = (uint32_t)sd->low_bits, fz.blocks = (uint32_t)sd->blocks;
    r.fuse = &fz;
  } else if (fuse) {
    // (the caller decides with the same predicate whether to pass `fuse`, pcv_build_finish `fuse_sort`; a caller that bypasses it
    // must not degrade silently into leaves nobody settles: one message per cause)
    if (plane && sd->nbits > 7)
      return ctx->fail(PCV_E_INVALID, "record sort: the settling pass with an intensity plane needs a second digit of <= 7 bits");
    return ctx->fail(PCV_E_INVALID, "record sort: the settling pass with an intensity plane needs the octree's intensity blob");
  }
  pcv_sort_launch_rec12(ctx, r);
  return hipGetLastError() == hipSuccess ? PCV_OK : ctx->fail(PCV_E_HIP, "record sort: second pass");
}

void pcv_sort_rec12_geometry(uint64_t n, int* groups, uint64_t* chunk) {
  const PcvSortGeom g = pcv_sort_geom(n, kPcvSortRec12Tile);
  *groups = g.groups;
  *chunk = g.chunk;
}
