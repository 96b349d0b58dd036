// pcv_las_dev.h — device side of the LAS decode (pcv_las.hip): the layout of the statistics block, the staging of a tile of
// records into LDS by aligned 16-byte loads, and the per-wave aggregation in front of the hot histogram bins.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kLasTile = 256;  // records per workgroup, one per lane
// A tile is staged in LDS while 256 records and the alignment slack fit 56 KiB; longer records (extra bytes) are picked from
// global memory directly.
constexpr uint32_t kLasStagedMaxStride = 224;
// The statistics of a load, u64 each, in device memory: counters first, then the two maxima, then the running output base.
constexpr int kLasStatClass = 0, kLasStatReturn = 256, kLasStatFlags = 272, kLasStatKept = 276, kLasStatDropClass = 277,
              kLasStatDropWithheld = 278, kLasStatMaxColor = 279, kLasStatMaxIntensity = 280, kLasStatBase = 281, kLasStatWords = 288;

// Bytes [from, from + bytes) into lds[0 ..]: `from` is 16-byte aligned and may lie up to 15 bytes before `lo`; only bytes inside
// [lo, hi) are read, whole 16-byte words by one load, the words that straddle an end byte by byte.
__device__ __forceinline__ void las_stage_tile(uint4* lds, const uint8_t* from, uint32_t bytes, const uint8_t* lo, const uint8_t* hi) {
  const uint32_t words = (bytes + 15) / 16;
  for (uint32_t w = threadIdx.x; w < words; w += kLasTile) {
    const uint8_t* p = from + 16 * (size_t)w;
    if (p >= lo && p + 16 <= hi) {
      lds[w] = *reinterpret_cast<const uint4*>(p);
    } else {
      uint8_t* d = reinterpret_cast<uint8_t*>(lds + w);
      for (int k = 0; k < 16; ++k)
        if (p + k >= lo && p + k < hi) d[k] = p[k];
    }
  }
}

// hist[bin] += 1 for every active lane, one LDS atomic per distinct bin of the wave: a file whose every record has one class
// costs one add per wave, not 64 on one address. Called by all lanes of a converged wave.
__device__ __forceinline__ void las_wave_hist_add(uint32_t* hist, uint32_t bin, bool active) {
  const uint32_t lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(active);
  while (todo) {  // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t b = (uint32_t)__shfl((int)bin, leader);
    const unsigned long long same = __ballot(active && bin == b);  // holds the leader's bit: the loop ends
    if (lane == (uint32_t)leader) atomicAdd(&hist[b], (uint32_t)__popcll(same));
    todo &= ~same;
  }
}
__device__ __forceinline__ uint32_t las_wave_max(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, off);
    v = o > v ? o : v;
  }
  return v;
}
