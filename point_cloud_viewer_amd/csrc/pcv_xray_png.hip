// pcv_xray_png.hip — compressed xray tiles on the device: the run-length deflate stream of pcv_xray_png_dev.h, one wave
// per (tile, band), no match search, no Huffman tables, no bit-level concatenation across work items.
//
//   xray_png_band_kernel    a wave filters its band straight from the RGBA tile (the row above comes from global memory),
//                           64 scanline bytes per step. A byte that differs from the one before it closes the run before
//                           it: a ballot marks those bytes, the lane of each finds the run's start from the ballot (or
//                           from the step before), counts the run's bits, a wave scan turns the counts into bit offsets,
//                           and the lane ORs the run's tokens into a zeroed LDS bit buffer. The lane one past the band's
//                           last byte closes the last run and adds end-of-block. The empty stored block follows, the
//                           buffer goes out in words to the band's slot (sized by the bound), and the band's byte count and
//                           Adler-32 partial sums go to the band tables.
//   xray_png_layout_kernel  one workgroup: per tile the exclusive scan of its band sizes and the Adler-32 combined from the
//                           partial sums, then the exclusive scan of the tile sizes over the chunk (count + 1 offsets).
//   xray_png_gather_kernel  a workgroup per (tile, band) copies the slot to its place in the tile's stream; the first band
//                           adds 78 01, the last the Adler-32.
//
// Only the compacted streams and the offsets are copied to the host (pcv_xray.hip).
#include "pcv_xray_png.h"

#include <algorithm>

namespace {

constexpr uint32_t kAdler = 65521u;

struct PngBandArgs {
  const uint8_t* a;
  const uint8_t* b;
  uint64_t na, tiles;
  uint32_t W, rows, bands, slot_words;
  uint8_t* slots;
  uint32_t* band_bytes;
  uint32_t* band_adler;
};

__global__ __launch_bounds__(64) void xray_png_band_kernel(PngBandArgs g) {
  extern __shared__ uint32_t bitbuf[];  // slot_words words
  const uint32_t lane = threadIdx.x;
  const uint32_t S = 1 + 4 * g.W;
  const uint64_t tile_bytes = 4ull * g.W * g.W, items = g.tiles * g.bands;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t t = item / g.bands;
    const uint32_t band = (uint32_t)(item % g.bands);
    const uint8_t* tile = t < g.na ? g.a + t * tile_bytes : g.b + (t - g.na) * tile_bytes;
    const uint32_t row0 = band * g.rows, n = min(g.rows, g.W - row0) * S;
    for (uint32_t i = lane; i < g.slot_words; i += 64) bitbuf[i] = i == 0 ? 2u : 0u;  // BFINAL 0, BTYPE 01
    __syncthreads();
    uint32_t bitpos = 3, open = 0, prev = 0;  // `open`: where the run that is still open starts
    uint32_t sum_a = 0;
    uint64_t sum_b = 0;
    for (uint32_t base = 0; base <= n; base += 64) {  // position n closes the last run
      const uint32_t j = base + lane;
      uint32_t v = 0;
      if (j < n) {
        v = pcv_png_filtered(tile, g.W, row0 + j / S, j % S);
        sum_a += v;
        sum_b += (uint64_t)(n - j) * v;
      }
      uint32_t before = __shfl_up(v, 1);
      if (lane == 0) before = prev;
      const bool closes = j >= 1 && j <= n && (j == n || v != before);
      const uint64_t marks = __ballot(closes);
      const uint64_t below = marks & ((1ull << lane) - 1ull);
      const uint32_t start = below ? base + 63u - (uint32_t)__clzll((long long)below) : open;
      const uint32_t len = j - start;
      uint32_t bits = 0;
      if (closes) bits = pcv_png_run_bits(len, before) + (j == n ? 7u : 0u);
      uint32_t upto = bits;  // inclusive wave scan
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(upto, d);
        if (lane >= d) upto += o;
      }
      if (closes) {
        uint32_t at = bitpos + upto - bits;
        pcv_png_run_emit(len, before, [&](uint32_t tok, uint32_t ntok) {
          const uint64_t x = (uint64_t)tok << (at & 31u);
          atomicOr(&bitbuf[at >> 5], (uint32_t)x);
          if (x >> 32) atomicOr(&bitbuf[(at >> 5) + 1], (uint32_t)(x >> 32));
          at += ntok;
        });  // end-of-block is seven zero bits: counted, nothing to OR
      }
      bitpos += __shfl(upto, 63);
      if (marks) open = base + 63u - (uint32_t)__clzll((long long)marks);
      prev = __shfl(v, 63);
    }
    __syncthreads();
    // the empty stored block: BFINAL (1 after the last band), BTYPE 00, pad, LEN 0, NLEN ffff
    const uint32_t tail = (bitpos + 3 + 7) / 8, total = tail + 4;
    if (lane == 0) {
      if (band + 1 == g.bands) atomicOr(&bitbuf[bitpos >> 5], 1u << (bitpos & 31u));
      reinterpret_cast<uint8_t*>(bitbuf)[tail + 2] = 0xff;
      reinterpret_cast<uint8_t*>(bitbuf)[tail + 3] = 0xff;
    }
    __syncthreads();
    uint32_t* slot = reinterpret_cast<uint32_t*>(g.slots) + item * g.slot_words;
    for (uint32_t i = lane; i < (total + 3) / 4; i += 64) slot[i] = bitbuf[i];
    sum_a %= kAdler;
    uint32_t sb = (uint32_t)(sum_b % kAdler);
    for (uint32_t d = 32; d; d >>= 1) {  // 64 values below 2^16 each
      sum_a += __shfl_xor(sum_a, d);
      sb += __shfl_xor(sb, d);
    }
    if (lane == 0) {
      g.band_bytes[item] = total;
      g.band_adler[2 * item] = sum_a % kAdler;
      g.band_adler[2 * item + 1] = sb % kAdler;
    }
    __syncthreads();  // the next band clears the buffer
  }
}

struct PngLayoutArgs {
  uint64_t tiles;
  uint32_t W, rows, bands;
  const uint32_t* band_bytes;
  const uint32_t* band_adler;
  uint32_t* band_off;
  uint32_t* tile_adler;
  uint64_t* offsets;
};

__global__ __launch_bounds__(256) void xray_png_layout_kernel(PngLayoutArgs g) {
  __shared__ uint64_t part[256];
  const uint32_t tid = threadIdx.x;
  const uint32_t S = 1 + 4 * g.W;
  // a thread takes a contiguous share of the tiles: their band offsets and checksums, and the share's bytes
  const uint64_t share = (g.tiles + 255) / 256, lo = min(g.tiles, tid * share), hi = min(g.tiles, lo + share);
  uint64_t mine = 0;
  for (uint64_t t = lo; t < hi; ++t) {
    uint32_t off = 0, s1 = 1, s2 = 0;
    for (uint32_t b = 0; b < g.bands; ++b) {
      const uint64_t item = t * g.bands + b;
      const uint32_t n = min(g.rows, g.W - b * g.rows) * S;
      g.band_off[item] = off;
      off += g.band_bytes[item];
      // n more bytes: s2 grows by n times the s1 before them, plus the sum of (n - j) * byte j
      s2 = (uint32_t)((s2 + (uint64_t)s1 * (n % kAdler) + g.band_adler[2 * item + 1]) % kAdler);
      s1 = (s1 + g.band_adler[2 * item]) % kAdler;
    }
    g.tile_adler[t] = s2 << 16 | s1;
    mine += 2ull + off + 4ull;
  }
  part[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    uint64_t run = 0;
    for (uint32_t i = 0; i < 256; ++i) {
      const uint64_t p = part[i];
      part[i] = run;
      run += p;
    }
    g.offsets[g.tiles] = run;
  }
  __syncthreads();
  uint64_t at = part[tid];
  for (uint64_t t = lo; t < hi; ++t) {
    g.offsets[t] = at;
    const uint64_t last = t * g.bands + g.bands - 1;
    at += 2ull + g.band_off[last] + g.band_bytes[last] + 4ull;
  }
}

struct PngGatherArgs {
  uint64_t tiles;
  uint32_t bands;
  uint64_t slot_bytes;
  const uint8_t* slots;
  const uint32_t* band_bytes;
  const uint32_t* band_off;
  const uint32_t* tile_adler;
  const uint64_t* offsets;
  uint8_t* out;
};

__global__ __launch_bounds__(256) void xray_png_gather_kernel(PngGatherArgs g) {
  const uint64_t items = g.tiles * g.bands;
  for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const uint64_t t = item / g.bands;
    const uint32_t band = (uint32_t)(item % g.bands);
    const uint8_t* src = g.slots + item * g.slot_bytes;
    const uint32_t n = g.band_bytes[item];
    uint8_t* stream = g.out + g.offsets[t];
    uint8_t* dst = stream + 2 + g.band_off[item];
    for (uint32_t i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
    if (threadIdx.x == 0) {
      if (band == 0) {
        stream[0] = 0x78;
        stream[1] = 0x01;
      }
      if (band + 1 == g.bands) {
        const uint32_t ad = g.tile_adler[t];
        dst[n] = (uint8_t)(ad >> 24);
        dst[n + 1] = (uint8_t)(ad >> 16);
        dst[n + 2] = (uint8_t)(ad >> 8);
        dst[n + 3] = (uint8_t)ad;
      }
    }
  }
}

}  // namespace

int pcv_xray_png_work_alloc(pcv_ctx* ctx, uint32_t W, uint64_t tiles, PcvPngWork* wk) {
  if (W == 0 || W > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return ctx->fail(PCV_E_INVALID, "xray: compressed tiles are at most " + std::to_string(PCV_XRAY_PNG_DEFLATE_MAX_EDGE) + " pixels wide");
  *wk = PcvPngWork();
  wk->W = W;
  wk->rows = PCV_XRAY_PNG_BAND_ROWS(W);
  wk->bands = (W + wk->rows - 1) / wk->rows;
  wk->tiles = tiles;
  wk->slot_bytes = (pcv_png_band_bound((uint64_t)std::min(wk->rows, W) * (1 + 4ull * W)) + 3) / 4 * 4;
  wk->tile_bound = pcv_png_stream_bound(W, W);
  const uint64_t items = tiles * wk->bands;
  int rc;
  if ((rc = ctx->dev_alloc((void**)&wk->slots, items * wk->slot_bytes)) || (rc = ctx->dev_alloc((void**)&wk->band_bytes, 4 * items)) ||
      (rc = ctx->dev_alloc((void**)&wk->band_off, 4 * items)) || (rc = ctx->dev_alloc((void**)&wk->band_adler, 8 * items)) ||
      (rc = ctx->dev_alloc((void**)&wk->tile_adler, 4 * tiles)) || (rc = ctx->dev_alloc((void**)&wk->offsets, 8 * (tiles + 1))) ||
      (rc = ctx->dev_alloc((void**)&wk->out, tiles * wk->tile_bound))) {
    pcv_xray_png_work_free(ctx, wk);
    return ctx->fail(PCV_E_OOM, "xray: no device memory to compress " + std::to_string(tiles) + " tiles (" + ctx->last_error + ")");
  }
  return PCV_OK;
}

void pcv_xray_png_work_free(pcv_ctx* ctx, PcvPngWork* wk) {
  void* blocks[] = {wk->slots, wk->band_bytes, wk->band_off, wk->band_adler, wk->tile_adler, wk->offsets, wk->out};
  for (void* p : blocks)
    if (p) ctx->dev_free(p);
  *wk = PcvPngWork();
}

int pcv_xray_png_launch(pcv_ctx* ctx, const PcvPngWork& wk, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t count) {
  if (count == 0 || count > wk.tiles) return ctx->fail(PCV_E_INVALID, "xray: bad chunk for the tile compressor");
  const uint64_t items = count * wk.bands;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(items, 1u << 16);
  PngBandArgs ba{a, b, na, count, wk.W, wk.rows, wk.bands, (uint32_t)(wk.slot_bytes / 4), wk.slots, wk.band_bytes, wk.band_adler};
  {
    PcvProf prof(ctx, PCV_K_XRAY_PNG_BAND);
    hipLaunchKernelGGL(xray_png_band_kernel, dim3(grid), dim3(64), wk.slot_bytes, ctx->stream, ba);
  }
  PngLayoutArgs la{count, wk.W, wk.rows, wk.bands, wk.band_bytes, wk.band_adler, wk.band_off, wk.tile_adler, wk.offsets};
  {
    PcvProf prof(ctx, PCV_K_XRAY_PNG_LAYOUT);
    hipLaunchKernelGGL(xray_png_layout_kernel, dim3(1), dim3(256), 0, ctx->stream, la);
  }
  PngGatherArgs ga{count, wk.bands, wk.slot_bytes, wk.slots, wk.band_bytes, wk.band_off, wk.tile_adler, wk.offsets, wk.out};
  {
    PcvProf prof(ctx, PCV_K_XRAY_PNG_GATHER);
    hipLaunchKernelGGL(xray_png_gather_kernel, dim3(grid), dim3(256), 0, ctx->stream, ga);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return ctx->fail(PCV_E_HIP, std::string("xray png kernels: ") + hipGetErrorString(e));
  return PCV_OK;
}
