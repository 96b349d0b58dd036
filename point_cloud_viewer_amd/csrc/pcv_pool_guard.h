// pcv_pool_guard.h — the layout arithmetic of the device pool's guard mode (pcv_ctx_set_pool_guard, pcv_ctx.hip) and the scan
// of a fence that came back to the host. Pure host code without a HIP type: tests/pool_guard_driver.cpp runs it under the host
// sanitizers.
//
// A guarded block, from its base address (what hipMalloc returned and what the pool's maps hold):
//   [0, 256)                        front fence
//   [256, 256 + requested)          the caller's bytes, `fill` when handed out; the user pointer is base + 256
//   [256 + requested, block_bytes)  back fence: the slack of the 256-byte rounding, 256 bytes more, and whatever the cache's
//                                   loose match made the block larger than the request
// Both fences hold the canary byte. The back fence begins at the requested byte count, not at the rounded one.
#pragma once
#include <stddef.h>
#include <stdint.h>

constexpr size_t kPcvGuardFront = 256;  // keeps the user pointer as aligned as the block
constexpr size_t kPcvGuardBackMin = 256;

struct PcvGuardLayout {
  size_t block_bytes = 0;  // the whole block
  size_t user_off = 0;     // user pointer - base
  size_t back_off = 0;     // back fence - base
  size_t back_bytes = 0;   // to the end of the block
};

// What a request of `requested` bytes asks the pool for under mode 2 (the pool rounds it no further: a multiple of 256).
inline size_t pcv_guard_block_request(size_t requested) {
  return kPcvGuardFront + ((requested + 255) & ~(size_t)255) + kPcvGuardBackMin;
}

// The layout of `requested` bytes in a block of `block_bytes` (>= pcv_guard_block_request(requested): a cached block may be
// larger). false: the block is too small.
inline bool pcv_guard_layout(size_t requested, size_t block_bytes, PcvGuardLayout* out) {
  if (block_bytes < pcv_guard_block_request(requested)) return false;
  out->block_bytes = block_bytes;
  out->user_off = kPcvGuardFront;
  out->back_off = kPcvGuardFront + requested;
  out->back_bytes = block_bytes - out->back_off;
  return true;
}

// A canary that differs from the fill.
inline uint8_t pcv_guard_canary(uint8_t fill) { return fill == 0xC5 ? 0x5C : 0xC5; }

// Index of the first byte of `fence` that is not `canary`, -1 if none.
inline int64_t pcv_guard_scan(const uint8_t* fence, size_t len, uint8_t canary) {
  for (size_t i = 0; i < len; ++i)
    if (fence[i] != canary) return (int64_t)i;
  return -1;
}

// The two fences of one block as copied back: false if both are whole, otherwise *offset is the first damaged byte relative
// to the user pointer (negative in the front fence, >= requested in the back fence; the front fence is looked at first).
inline bool pcv_guard_first_damage(const uint8_t* front, const uint8_t* back, const PcvGuardLayout& lay, uint8_t canary,
                                   int64_t* offset) {
  int64_t at = pcv_guard_scan(front, lay.user_off, canary);
  if (at >= 0) {
    *offset = at - (int64_t)lay.user_off;
    return true;
  }
  at = pcv_guard_scan(back, lay.back_bytes, canary);
  if (at >= 0) {
    *offset = at + (int64_t)(lay.back_off - lay.user_off);
    return true;
  }
  return false;
}

// Every byte of `bytes` equals `fill`? (the selftest's read-back) -1, or the first index that differs.
inline int64_t pcv_guard_first_unfilled(const uint8_t* bytes, size_t len, uint8_t fill) { return pcv_guard_scan(bytes, len, fill); }
