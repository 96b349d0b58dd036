// pcv_rows_dev.h — the tile scheme of the result writers, device side: what the row kernels of pcv_ply_rows.hip and
// pcv_las_write.hip share, and the store that pcv_tiles3d.hip shares with them. One workgroup of 256 packs one TILE of
// consecutive rows: it finds the chunk that holds the tile's first row by bisection over the scanned chunk offsets, its 4 waves
// walk the chunks from there (ranks by ballot over the keep bytes for the octree batch, as query_compact_kernel counts them; the
// per-candidate offsets for an S2 query), every lane lays its point's row into an LDS image of the tile whose byte 0 stands at
// the alignment (mod 16) the tile has in the output, and after a barrier the image leaves as aligned 16-byte vectors with a
// bytewise head and tail. The walks take the format's part as a callable; all byte offsets into the output are u64.
#pragma once
#include "pcv_query_dev.h"
#include "pcv_s2_query_dev.h"

// `bytes` bytes whose byte 0 stands at img[phase], phase = (address of dst) % 16 and img 16-byte aligned, to dst: the interior
// as aligned 16-byte vectors, its unaligned head and tail bytewise.
__device__ __forceinline__ void pcv_store_image(const uint8_t* img, uint8_t* __restrict__ dst, uint32_t phase, uint32_t bytes) {
  const uint32_t head = min(bytes, (16u - phase) & 15u);
  for (uint32_t j = threadIdx.x; j < head; j += 256u) dst[j] = img[phase + j];
  const uint32_t nvec = (bytes - head) >> 4;
  uint4* __restrict__ gv = reinterpret_cast<uint4*>(dst + head);
  const uint4* lv = reinterpret_cast<const uint4*>(img + phase + head);  // phase + head is 0 or 16
  for (uint32_t v = threadIdx.x; v < nvec; v += 256u) gv[v] = lv[v];
  const uint32_t done = head + (nvec << 4);
  for (uint32_t j = done + threadIdx.x; j < bytes; j += 256u) dst[j] = img[phase + j];
}

// the last chunk c of [c0, c1) whose first row start(c) is <= g; start(c0) <= g by the caller's choice of c0
template <typename Start>
__device__ __forceinline__ uint64_t pcv_chunk_of_row(uint64_t c0, uint64_t c1, uint64_t g, Start start) {
  uint64_t lo = c0, hi = c1;  // start(lo) <= g, start(hi) > g (or hi == c1)
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (start(mid) <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The tile of workgroup blockIdx.x: rows [g0, g1) of the result, `rows` of them, to dst = out + (g0 - row0) * stride, whose
// address mod 16 is `phase`. `nrows` rows from row0 on are packed by the launch.
struct PcvRowsTile {
  uint32_t rows, phase;
  uint64_t g0, g1;
  uint8_t* dst;
};
__device__ __forceinline__ PcvRowsTile pcv_rows_tile(uint64_t row0, uint64_t nrows, uint32_t tile_rows, uint32_t stride, uint8_t* out) {
  const uint64_t t0 = (uint64_t)blockIdx.x * tile_rows;
  const uint32_t rows = (uint32_t)min((uint64_t)tile_rows, nrows - t0);
  const uint64_t g0 = row0 + t0;
  uint8_t* dst = out + t0 * stride;
  return PcvRowsTile{rows, (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u), g0, g0 + rows, dst};
}

// Rows [g0, g1) of the octree batch among the chunks [c0, c1) of the caller's segment range; chunk_off their scanned kept counts
// (the row of a chunk's first kept point). f(mine, view, q, attr_index, row_in_tile) is called by every lane of every 64-point
// step (a callable may hold ballots): `mine` says that point q of the chunk behind `view` is kept and its row lies in the tile,
// at row_in_tile < g1 - g0 (any value where !mine); attr_index is its index in the rgb / intensity blobs.
template <typename F>
__device__ __forceinline__ void pcv_walk_octree_rows(const ChunkDesc* __restrict__ desc, uint64_t c0, uint64_t c1, const uint8_t* __restrict__ xyz_blob,
                                                     const uint8_t* __restrict__ keep, const uint64_t* __restrict__ chunk_off, uint64_t g0, uint64_t g1,
                                                     F f) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t first = pcv_chunk_of_row(c0, c1, g0, [&](uint64_t c) { return chunk_off[c]; });
  for (uint64_t ci = first + wave; ci < c1; ci += 4) {
    uint64_t pos0 = chunk_off[ci];
    if (pos0 >= g1) break;                  // (uniform) offsets only grow
    if (chunk_off[ci + 1] <= g0) continue;  // nothing of this chunk in the tile (an empty chunk among them)
    const ChunkDesc& d = desc[ci];
    const PointsView v = points_view_of(d, xyz_blob);  // the decode of query_compact_kernel: the same bits as pcv_query_batch_points
    const uint8_t* kp = keep + d.keep_off;
    for (uint32_t q0 = 0; q0 < d.cnt && pos0 < g1; q0 += 64) {
      const uint32_t q = q0 + lane;
      const unsigned long long b = __ballot(q < d.cnt && kp[q]);
      const uint64_t pos = pos0 + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
      f(((b >> lane) & 1ull) && pos >= g0 && pos < g1, v, q, d.attr_index + q, (uint32_t)(pos - g0));
      pos0 += (uint64_t)__popcll(b);
    }
  }
}

// The same over an S2 query: u32 flags and a scanned offset per candidate. f(mine, i, row_in_tile), by every lane of every
// 64-candidate step (uniform trip count); i is the point's index in the cloud's columns.
template <typename F>
__device__ __forceinline__ void pcv_walk_s2_rows(const PcvS2Chunk* __restrict__ chunks, uint64_t c0, uint64_t c1, const uint32_t* __restrict__ flags,
                                                 const uint64_t* __restrict__ offsets, uint64_t g0, uint64_t g1, F f) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t first = pcv_chunk_of_row(c0, c1, g0, [&](uint64_t c) { return offsets[chunks[c].first]; });
  for (uint64_t ci = first + wave; ci < c1; ci += 4) {
    const PcvS2Chunk c = chunks[ci];
    if (offsets[c.first] >= g1) break;
    if (offsets[c.first + c.count] <= g0) continue;
    for (uint32_t q0 = 0; q0 < c.count; q0 += 64) {
      const uint32_t q = q0 + lane;
      bool mine = q < c.count && flags[c.first + q] != 0;
      uint64_t pos = 0;
      if (mine) {
        pos = offsets[c.first + q];
        mine = pos >= g0 && pos < g1;
      }
      f(mine, c.src + q, (uint32_t)(pos - g0));
    }
  }
}
