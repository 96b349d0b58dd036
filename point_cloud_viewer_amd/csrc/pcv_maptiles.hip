// pcv_maptiles.hip — map tiles on the device (include/pcv_hip.h "map tiles"): z/x/y PNG pyramids of ECEF clouds.
// A keyed scatter-reduce whose key comes out of the web-mercator chain, the image resolve, the parent levels and the
// slippy-map directory.
//   per piece  maptiles_project_kernel: the chain of pcv_wmr_dev.h and the pixel rule of pcv_maptiles_dev.h, one thread per
//              point, leaves an 8-byte (gx, gy) key per point (all ones: dropped) and counts the dropped. It is the only
//              kernel that carries the chain's registers.
//              maptiles_mark_kernel: reads keys; every tile a key touches for the first time enters a hash table keyed by
//              (x, y) (open addressing, one 64-bit CAS per new tile) and takes a slot. The host grows the pool of
//              accumulators to the slots handed out, as the terrain does.
//              maptiles_accum_kernel: reads keys and colours; per drawn point two 64-bit atomicAdds onto the packed
//              [r | g << 32] and [n | b << 32] of its pixel: exact while a pixel holds at most 2^24 points.
//   queries    a result's rows in pieces cut at any row: the PLY output's packer fills a bounded buffer of 27-byte rows,
//              maptiles_unpack_kernel spreads them into staging planes, then as above
//   finish     the touched tiles sorted by (x, y) on the host, maptiles_resolve_kernel (accumulators -> RGBA8 by xray's
//              `colored` and the background rule, the count plane, the 2^24 check), accumulators released
//   parents    xray_build_levels (pcv_xray_pyramid.hip) over the quadtree indices of the tiles: no second resize
//   files      the xray quadtree's writer (xray_tile_files of pcv_xray_files.hip: stored and deflate encoders, chunked
//              downloads, host threads) under <dir>/<z>/<x>/<y>.png names, then tiles.json
// Every byte is an exact function of the multiset of points: integer sums only.
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <new>

#include "pcv_internal.h"
#include "pcv_maptiles_dev.h"
#include "pcv_query_dev.h"
#include "pcv_result_rows.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_query_dev.h"
#include "pcv_terrain_files.h"
#include "pcv_xray_obj.h"

namespace {

constexpr uint64_t kEmpty = ~0ull;                // a free table entry; no tile key has bit 63 set
constexpr uint64_t kMaxTiles = 1ull << 22;
constexpr uint64_t kTilePixels = (uint64_t)kMapTilePx * kMapTilePx;
constexpr uint64_t kTileBytes = kTilePixels * 16;  // two u64 per pixel
constexpr uint64_t kImageBytes = kTilePixels * 4;
constexpr uint64_t kChunkBytes = 64ull << 20;     // the pool grows by doubling up to chunks of this size
constexpr uint32_t kRows = 32768;                 // tiles per launch of the resolve (gridDim.y)

enum { kCtrDropped = 0, kCtrSlots = 1, kCtrNoStorage = 2, kCtrOverLimit = 3, kCtrTableFull = 4, kCtrs = 5 };

// what the kernels take by value
struct MapDev {
  uint32_t zoom, cap_mask;  // table capacity - 1 (a power of two)
  uint32_t shift;           // 64 - log2(capacity)
  uint32_t max_tiles, nslots_alloc, background;
  uint64_t* keys;       // capacity tile keys (x << 32 | y), kEmpty where free
  uint32_t* vals;       // slot + 1 of the key beside it; 0 between the CAS and the slot
  uint64_t* slot_key;   // slot -> tile key
  uint64_t* slot_base;  // slot -> its accumulators: per pixel [r | g << 32], [n | b << 32]
  uint64_t* ctr;        // kCtr*
};

__device__ inline uint64_t tile_of(uint64_t key) { return (((key & 0xffffffffull) >> 8) << 32) | (key >> 40); }
__device__ inline uint32_t pixel_of(uint64_t key) { return (uint32_t)(((key >> 32) & 255u) << 8) | (uint32_t)(key & 255u); }
__device__ inline uint32_t home(const MapDev& d, uint64_t tile) { return (uint32_t)((tile * 0x9E3779B97F4A7C15ull) >> d.shift) & d.cap_mask; }

__global__ __launch_bounds__(256) void maptiles_project_kernel(uint32_t zoom, uint64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                              const double* __restrict__ z, uint64_t* __restrict__ keys, uint64_t* __restrict__ ctr) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false;
  if (k < n) {
    uint32_t gx, gy;
    dropped = !pcv_maptiles_pixel(zoom, x[k], y[k], z[k], &gx, &gy);
    keys[k] = dropped ? kMapTileNoKey : pcv_maptiles_key(gx, gy);
  }
  const unsigned long long drops = __ballot(dropped);
  if ((threadIdx.x & 63) == 0 && drops) atomicAdd((unsigned long long*)&ctr[kCtrDropped], (unsigned long long)__popcll(drops));
}

__global__ __launch_bounds__(256) void maptiles_mark_kernel(MapDev d, uint64_t n, const uint64_t* __restrict__ keys) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t key = k < n ? keys[k] : kMapTileNoKey;
  const uint64_t tile = key == kMapTileNoKey ? kEmpty : tile_of(key);
  // neighbours in a stream mostly share a tile: a lane whose left neighbour asks for the same tile leaves it to that lane
  const uint64_t left = (uint64_t)__shfl_up((unsigned long long)tile, 1);
  if (tile == kEmpty || ((threadIdx.x & 63) != 0 && left == tile)) return;
  uint32_t h = home(d, tile);
  for (uint32_t step = 0; step <= d.cap_mask; ++step, h = (h + 1) & d.cap_mask) {
    uint64_t cur = __atomic_load_n(&d.keys[h], __ATOMIC_RELAXED);
    if (cur == kEmpty) {
      if (__atomic_load_n(&d.ctr[kCtrSlots], __ATOMIC_RELAXED) >= d.max_tiles) {
        // every slot is handed out, each after its key's CAS: a key that is not here now never gets one. One tile too many:
        // the host ends the layer; the table takes no more keys, so it cannot fill
        cur = __atomic_load_n(&d.keys[h], __ATOMIC_RELAXED);
        if (cur == kEmpty) break;
      } else {
        cur = atomicCAS((unsigned long long*)&d.keys[h], (unsigned long long)kEmpty, (unsigned long long)tile);
        if (cur == kEmpty) {
          const uint64_t slot = atomicAdd((unsigned long long*)&d.ctr[kCtrSlots], 1ull);
          if (slot >= d.max_tiles) break;
          d.slot_key[slot] = tile;
          atomicExch(&d.vals[h], (uint32_t)slot + 1);
          return;
        }
      }
    }
    if (cur == tile) return;
  }
  d.ctr[kCtrTableFull] = 1;
}

__global__ __launch_bounds__(256) void maptiles_accum_kernel(MapDev d, uint64_t n, const uint64_t* __restrict__ keys, const uint8_t* __restrict__ rgb) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const uint64_t key = keys[k];
  if (key == kMapTileNoKey) return;
  const uint64_t tile = tile_of(key);
  uint32_t h = home(d, tile), slot = 0;
  for (uint32_t step = 0; step <= d.cap_mask; ++step, h = (h + 1) & d.cap_mask) {
    const uint64_t cur = d.keys[h];
    if (cur == tile) {
      slot = d.vals[h];
      break;
    }
    if (cur == kEmpty) break;
  }
  if (slot == 0 || slot - 1 >= d.nslots_alloc) {
    d.ctr[kCtrNoStorage] = 1;  // the mark pass and the host's growth cover every tile: a point without storage is a bug, not data
    return;
  }
  const uint64_t r = rgb[3 * k], g = rgb[3 * k + 1], b = rgb[3 * k + 2];
  uint64_t* w = (uint64_t*)d.slot_base[slot - 1] + 2ull * pixel_of(key);
  atomicAdd((unsigned long long*)&w[0], (unsigned long long)(r | (g << 32)));
  atomicAdd((unsigned long long*)&w[1], (unsigned long long)(1ull | (b << 32)));
}

// n packed rows (x y z as doubles at any alignment, then r g b; kPcvXyzRgbRowBytes each) into planes
__global__ __launch_bounds__(256) void maptiles_unpack_kernel(uint64_t n, const uint8_t* __restrict__ rows, double* __restrict__ x, double* __restrict__ y,
                                                             double* __restrict__ z, uint8_t* __restrict__ rgb) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const uint8_t* r = rows + k * kPcvXyzRgbRowBytes;
  double p[3];
  for (int a = 0; a < 3; ++a) {
    uint64_t bits = 0;
    for (int b = 0; b < 8; ++b) bits |= (uint64_t)r[8 * a + b] << (8 * b);
    memcpy(&p[a], &bits, 8);
  }
  x[k] = p[0], y[k] = p[1], z[k] = p[2];
  rgb[3 * k] = r[24], rgb[3 * k + 1] = r[25], rgb[3 * k + 2] = r[26];
}

// accumulators -> image and count plane: grid = (256 blocks per tile, tiles)
__global__ __launch_bounds__(256) void maptiles_resolve_kernel(MapDev d, uint32_t tile0, const uint32_t* __restrict__ out_slot, uint32_t* __restrict__ images,
                                                              uint32_t* __restrict__ counts) {
  const uint32_t px = blockIdx.x * 256 + threadIdx.x;  // < 65536: the grid is exact
  const uint32_t tile = tile0 + blockIdx.y;
  const uint64_t* w = (const uint64_t*)d.slot_base[out_slot[tile]] + 2ull * px;
  const uint64_t rg = w[0], nb = w[1];
  const uint32_t n = (uint32_t)nb;
  const bool over = n > kMapTilePixelLimit;
  const uint64_t o = (uint64_t)tile * kTilePixels + px;
  images[o] = over ? d.background : pcv_maptiles_rgba(rg & 0xffffffffull, rg >> 32, nb >> 32, n, d.background);
  counts[o] = n;
  const unsigned long long m = __ballot(over);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd((unsigned long long*)&d.ctr[kCtrOverLimit], (unsigned long long)__popcll(m));
}

struct Level {  // one built zoom below the maximum: its tiles ascending by (x, y)
  std::vector<uint32_t> xy;       // 2 per tile
  std::vector<uint64_t> image;    // per tile: its position among all parent images (d_parents)
};

}  // namespace

struct pcv_maptiles {
  pcv_ctx* ctx = nullptr;
  pcv_maptiles_params params{};
  MapDev dev{};
  uint64_t capacity = 0;       // entries of the table
  uint64_t cap_bytes = 0, pool_bytes = 0;
  std::vector<void*> chunks;   // the pool
  std::vector<uint64_t> slot_base;  // host copy, [nslots_alloc]
  uint32_t nslots = 0;         // slots handed out by the device
  uint64_t points_added = 0, dropped = 0;
  // staging of host input and of query results, and the keys of a piece
  double *sx = nullptr, *sy = nullptr, *sz = nullptr;
  uint8_t* srgb = nullptr;
  uint8_t* srows = nullptr;
  uint64_t staging_cap = 0;
  uint64_t* d_keys = nullptr;
  uint64_t keys_cap = 0;
  bool finished = false, dead = false;
  // after finish
  std::vector<uint32_t> xy;    // 2 per tile of the maximum zoom
  uint32_t* d_images = nullptr;
  uint32_t* d_counts = nullptr;
  // after build_parents
  bool parents_built = false;
  uint32_t min_zoom = 0;
  std::vector<Level> levels;   // levels[k]: zoom - 1 - k
  uint32_t* d_parents = nullptr;

  void free_pool() {
    for (void* p : chunks) ctx->dev_free(p);
    chunks.clear();
    slot_base.clear();
    pool_bytes = 0;
    dev.nslots_alloc = 0;
  }
  void free_staging() {
    for (void* p : {(void*)sx, (void*)sy, (void*)sz, (void*)srgb, (void*)srows, (void*)d_keys})
      if (p) ctx->dev_free(p);
    sx = sy = sz = nullptr, srgb = srows = nullptr, d_keys = nullptr, staging_cap = keys_cap = 0;
  }
  void free_table() {
    for (void* p : {(void*)dev.keys, (void*)dev.vals, (void*)dev.slot_key, (void*)dev.slot_base, (void*)dev.ctr})
      if (p) ctx->dev_free(p);
    dev.keys = dev.slot_key = dev.slot_base = dev.ctr = nullptr, dev.vals = nullptr;
  }
  // everything on the device, after the stream has drained
  void release_all() {
    (void)hipStreamSynchronize(ctx->stream);
    free_pool();
    free_staging();
    free_table();
    for (void* p : {(void*)d_images, (void*)d_counts, (void*)d_parents})
      if (p) ctx->dev_free(p);
    d_images = d_counts = d_parents = nullptr;
  }
  int die(int code, const std::string& msg) {
    release_all();
    dead = true;
    return ctx->fail(code, msg);
  }
  // the tiles of a built zoom: their (x, y) list, null where the zoom is not built
  const std::vector<uint32_t>* tiles_of(uint32_t zoom) const {
    if (zoom == params.zoom) return &xy;
    if (zoom > params.zoom || zoom < min_zoom) return nullptr;
    return &levels[params.zoom - 1 - zoom].xy;
  }
};

namespace {

int check_params(const pcv_maptiles_params* p, uint32_t min_zoom, std::string* why) {
  auto bad = [&](const std::string& m) {
    *why = m;
    return PCV_E_INVALID;
  };
  if (!p) return bad("null pcv_maptiles_params");
  if (p->zoom > kMapTileMaxZoom) return bad("map tiles: zoom must be in 0 ..= 23, got " + std::to_string(p->zoom));
  if (p->max_tiles == 0 || p->max_tiles > kMaxTiles) return bad("map tiles: max_tiles must be in 1 ..= 2^22, got " + std::to_string(p->max_tiles));
  if (min_zoom > p->zoom) return bad("map tiles: min_zoom " + std::to_string(min_zoom) + " is above zoom " + std::to_string(p->zoom));
  return PCV_OK;
}

int usable(const pcv_maptiles* m, bool want_finished) {
  if (m->dead) return m->ctx->fail(PCV_E_INVALID, "the map-tile layer failed earlier and can only be freed");
  if (m->finished != want_finished)
    return m->ctx->fail(PCV_E_INVALID, want_finished ? "the map-tile layer is not finished" : "the map-tile layer is finished: no more points");
  return PCV_OK;
}

template <typename T>
int alloc(pcv_maptiles* m, T** p, uint64_t count) {
  void* q = nullptr;
  if (int rc = m->ctx->dev_alloc(&q, std::max<uint64_t>(count, 1) * sizeof(T))) return rc;
  *p = (T*)q;
  return PCV_OK;
}

// reads the counters; the stream is idle afterwards
int read_counters(pcv_maptiles* m, uint64_t out[kCtrs]) {
  pcv_ctx* ctx = m->ctx;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, m->dev.ctr, kCtrs * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < kCtrs; ++k) out[k] = ctx->mailbox[k];
  return PCV_OK;
}

// storage for the slots [nslots_alloc, want): chunks that double up to kChunkBytes, zeroed on the stream
int grow_pool(pcv_maptiles* m, uint32_t want) {
  pcv_ctx* ctx = m->ctx;
  const uint32_t have = m->dev.nslots_alloc;
  if (want <= have) return PCV_OK;
  const uint64_t need = (uint64_t)(want - have);
  const uint64_t room = (m->cap_bytes - std::min(m->cap_bytes, m->pool_bytes)) / kTileBytes;
  if (need > room)
    return m->die(PCV_E_OOM, "map tiles: " + std::to_string(want) + " touched tiles of " + std::to_string(kTileBytes) + " bytes pass max_pool_bytes = " +
                                 std::to_string(m->cap_bytes));
  // what is asked for, or as much again as there is (up to a chunk): both fit, by the check above and want <= max_tiles
  const uint64_t by_size = kChunkBytes / kTileBytes;
  const uint64_t tiles = std::min({std::max<uint64_t>(need, std::min<uint64_t>(by_size, have)), room, m->params.max_tiles - (uint64_t)have});
  uint8_t* p = nullptr;
  if (int rc = alloc(m, &p, tiles * kTileBytes)) {
    const std::string why = ctx->last_error;
    return m->die(rc, why);
  }
  m->chunks.push_back(p);
  m->pool_bytes += tiles * kTileBytes;
  if (hipMemsetAsync(p, 0, tiles * kTileBytes, ctx->stream) != hipSuccess) return m->die(PCV_E_HIP, "hipMemsetAsync (map-tile pool)");
  for (uint64_t k = 0; k < tiles; ++k) m->slot_base.push_back((uint64_t)(uintptr_t)(p + k * kTileBytes));
  const uint32_t now = (uint32_t)m->slot_base.size();
  // the new entries only; pageable source, so the copy has left the vector when the call returns
  if (hipMemcpyAsync(m->dev.slot_base + have, m->slot_base.data() + have, (size_t)(now - have) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return m->die(PCV_E_HIP, "hipMemcpyAsync (map-tile slot table)");
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return m->die(PCV_E_HIP, "hipStreamSynchronize (map-tile slot table)");
  m->dev.nslots_alloc = now;
  return PCV_OK;
}

uint64_t piece_points(const pcv_maptiles* m) { return m->params.staging_points ? m->params.staging_points : (1ull << 22); }

int reserve_keys(pcv_maptiles* m, uint64_t points) {
  if (points <= m->keys_cap) return PCV_OK;
  (void)hipStreamSynchronize(m->ctx->stream);  // a kernel may still read the old buffer
  if (m->d_keys) m->ctx->dev_free(m->d_keys);
  m->d_keys = nullptr, m->keys_cap = 0;
  if (int rc = alloc(m, &m->d_keys, points)) return rc;
  m->keys_cap = points;
  return PCV_OK;
}

// n points in device memory, a piece at a time: project, mark, grow, accumulate
int add_device(pcv_maptiles* m, uint64_t n, const double* x, const double* y, const double* z, const uint8_t* rgb) {
  pcv_ctx* ctx = m->ctx;
  const uint64_t piece = std::min(n, piece_points(m));
  if (int rc = reserve_keys(m, piece)) return rc;
  for (uint64_t at = 0; at < n; at += piece) {
    const uint64_t c = std::min(piece, n - at);
    const dim3 grid((uint32_t)((c + 255) / 256)), block(256);
    {
      PcvProf prof(ctx, PCV_K_MAPTILES_PROJECT);
      hipLaunchKernelGGL(maptiles_project_kernel, grid, block, 0, ctx->stream, m->dev.zoom, c, x + at, y + at, z + at, m->d_keys, m->dev.ctr);
    }
    {
      PcvProf prof(ctx, PCV_K_MAPTILES_MARK);
      hipLaunchKernelGGL(maptiles_mark_kernel, grid, block, 0, ctx->stream, m->dev, c, (const uint64_t*)m->d_keys);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    uint64_t ctr[kCtrs];
    if (int rc = read_counters(m, ctr)) return rc;
    if (ctr[kCtrTableFull] || ctr[kCtrSlots] > m->params.max_tiles)
      return m->die(PCV_E_OOM, "map tiles: the points touch more than max_tiles = " + std::to_string(m->params.max_tiles) + " tiles at zoom " +
                                   std::to_string(m->params.zoom));
    m->nslots = (uint32_t)ctr[kCtrSlots];
    if (int rc = grow_pool(m, m->nslots)) return rc;
    {
      PcvProf prof(ctx, PCV_K_MAPTILES_ACCUM);
      hipLaunchKernelGGL(maptiles_accum_kernel, grid, block, 0, ctx->stream, m->dev, c, (const uint64_t*)m->d_keys, rgb + 3 * at);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  m->points_added += n;
  return PCV_OK;
}

int reserve_staging(pcv_maptiles* m, uint64_t points) {
  if (points <= m->staging_cap) return PCV_OK;
  (void)hipStreamSynchronize(m->ctx->stream);  // a kernel may still read the old buffers
  m->free_staging();
  int rc;
  if ((rc = alloc(m, &m->sx, points)) || (rc = alloc(m, &m->sy, points)) || (rc = alloc(m, &m->sz, points)) || (rc = alloc(m, &m->srgb, 3 * points))) {
    m->free_staging();
    return rc;
  }
  m->staging_cap = points;
  return PCV_OK;
}

int check_total(pcv_maptiles* m, uint64_t n) {
  if (n > 0xffffffffull - m->points_added) return m->ctx->fail(PCV_E_INVALID, "map tiles: more than 2^32 - 1 points in total");
  return PCV_OK;
}

// segments [first, first + num) of a query result in pieces of at most staging_points rows, cut at any row: pack(row0, rows,
// out) packs a row range as x y z r g b rows (the PLY output's packer), maptiles_unpack_kernel spreads them into the planes
template <typename Pack>
int add_segments(pcv_maptiles* m, const uint64_t* seg_off, uint64_t nseg, uint64_t first, uint64_t num, Pack pack) {
  pcv_ctx* ctx = m->ctx;
  if (first > nseg || num > nseg - first) return ctx->fail(PCV_E_INVALID, "segment range past the end");
  const uint64_t p0 = seg_off[first], np = seg_off[first + num] - p0;
  if (int rc = check_total(m, np)) return rc;
  if (np == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint64_t piece = std::min(np, piece_points(m));
  int rc;
  if ((rc = reserve_staging(m, piece))) return rc;
  if (!m->srows && (rc = alloc(m, &m->srows, m->staging_cap * kPcvXyzRgbRowBytes))) return rc;
  for (uint64_t at = 0; at < np; at += piece) {
    const uint64_t c = std::min(piece, np - at);
    if ((rc = pack(p0 + at, c, m->srows))) return rc;
    {
      PcvProf prof(ctx, PCV_K_MAPTILES_UNPACK);
      hipLaunchKernelGGL(maptiles_unpack_kernel, dim3((uint32_t)((c + 255) / 256)), dim3(256), 0, ctx->stream, c, (const uint8_t*)m->srows, m->sx, m->sy, m->sz,
                         m->srgb);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = add_device(m, c, m->sx, m->sy, m->sz, m->srgb))) return rc;
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the staging is refilled next
  }
  ctx->prof_resolve();
  return PCV_OK;
}

int check_range(const pcv_maptiles* m, uint32_t zoom, uint64_t first, uint64_t count, const std::vector<uint32_t>** tiles) {
  *tiles = m->tiles_of(zoom);
  if (!*tiles) return m->ctx->fail(PCV_E_INVALID, "map tiles: zoom " + std::to_string(zoom) + " is not built (" + std::to_string(m->min_zoom) + " ..= " +
                                                      std::to_string(m->params.zoom) + " are)");
  const uint64_t have = (*tiles)->size() / 2;
  if (first > have || count > have - first) return m->ctx->fail(PCV_E_INVALID, "tile range past the end");
  return PCV_OK;
}

// the images of tiles [first, first + count) of a built zoom into dst, runs of neighbours in one copy; no synchronisation
int queue_images(pcv_maptiles* m, uint32_t zoom, uint64_t first, uint64_t count, uint8_t* dst, hipMemcpyKind kind) {
  pcv_ctx* ctx = m->ctx;
  if (count == 0) return PCV_OK;
  if (zoom == m->params.zoom) {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst, reinterpret_cast<const uint8_t*>(m->d_images) + first * kImageBytes, count * kImageBytes, kind, ctx->stream));
    return PCV_OK;
  }
  const std::vector<uint64_t>& image = m->levels[m->params.zoom - 1 - zoom].image;
  for (uint64_t k = 0; k < count;) {
    uint64_t run = 1;
    while (k + run < count && image[first + k + run] == image[first + k] + run) ++run;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst + k * kImageBytes, reinterpret_cast<const uint8_t*>(m->d_parents) + image[first + k] * kImageBytes, run * kImageBytes,
                                      kind, ctx->stream));
    k += run;
  }
  return PCV_OK;
}

// The PNG files of tiles [first, first + count) of a built zoom through the xray quadtree's writer (xray_tile_files), in the
// tile list's order on the calling thread: the maximum zoom's images lie in that order; a parent zoom's requested tiles are
// gathered side by side first
int ordered_tile_files(pcv_maptiles* m, uint32_t zoom, uint64_t first, uint64_t count, int mode, const XrayFileSink& sink) {
  pcv_ctx* ctx = m->ctx;
  if (count == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  const uint8_t* tiles = reinterpret_cast<const uint8_t*>(m->d_images) + first * kImageBytes;
  if (zoom != m->params.zoom) {
    uint8_t* d_stage = nullptr;
    int rc;
    if ((rc = sc.get(&d_stage, count * kImageBytes)) || (rc = queue_images(m, zoom, first, count, d_stage, hipMemcpyDeviceToDevice))) return rc;
    tiles = d_stage;
  }
  return xray_tile_files(
      ctx, kMapTilePx, count, mode, false,
      [&](uint64_t f, uint64_t, const uint8_t** a, uint64_t* na, const uint8_t** b) { *a = nullptr, *na = 0, *b = tiles + f * kImageBytes; }, sink);
}

// Every tile of a built zoom to sink(tile, file, len), `tile` its place in the zoom's list, from the writer's host threads and
// in the order the images lie on the device: a parent zoom's images lie side by side in quadtree order
int all_tile_files(pcv_maptiles* m, uint32_t zoom, int mode, const XrayFileSink& sink) {
  pcv_ctx* ctx = m->ctx;
  const uint64_t count = m->tiles_of(zoom)->size() / 2;
  if (count == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint8_t* tiles = reinterpret_cast<const uint8_t*>(m->d_images);
  std::vector<uint64_t> tile_of_image;  // empty: the identity
  if (zoom != m->params.zoom) {
    const std::vector<uint64_t>& image = m->levels[m->params.zoom - 1 - zoom].image;
    const uint64_t base = *std::min_element(image.begin(), image.end());  // a level's images are one range of d_parents
    tile_of_image.resize(count);
    for (uint64_t t = 0; t < count; ++t) tile_of_image[image[t] - base] = t;
    tiles = reinterpret_cast<const uint8_t*>(m->d_parents) + base * kImageBytes;
  }
  return xray_tile_files(
      ctx, kMapTilePx, count, mode, true,
      [&](uint64_t f, uint64_t, const uint8_t** a, uint64_t* na, const uint8_t** b) { *a = nullptr, *na = 0, *b = tiles + f * kImageBytes; },
      [&](uint64_t i, const uint8_t* file, uint64_t len) { return sink(tile_of_image.empty() ? i : tile_of_image[i], file, len); });
}

int check_png_mode(pcv_maptiles* m, int mode) {
  if (mode != PCV_XRAY_PNG_STORED && mode != PCV_XRAY_PNG_DEFLATE) return m->ctx->fail(PCV_E_INVALID, "map tiles: unknown PNG mode");
  return PCV_OK;
}

std::string tiles_json(uint32_t min_zoom, uint32_t max_zoom, const uint64_t* counts, const uint32_t* xy) {
  auto f = pcv_terrain_f64_json;
  const uint32_t nz = max_zoom - min_zoom + 1;
  uint64_t before = 0;
  for (uint32_t k = 0; k + 1 < nz; ++k) before += counts[k];
  // the hull of the corners of the tiles of max_zoom: to_lat_lng is monotone in u and in v, so the hull's corners do
  double bounds[4] = {0.0, 0.0, 0.0, 0.0};
  if (counts[nz - 1]) {
    uint32_t lo[2] = {0xffffffffu, 0xffffffffu}, hi[2] = {0, 0};
    for (uint64_t k = 0; k < counts[nz - 1]; ++k)
      for (int a = 0; a < 2; ++a) {
        const uint32_t v = xy[2 * (before + k) + a];
        lo[a] = std::min(lo[a], v), hi[a] = std::max(hi[a], v);
      }
    const double scale = (double)(1u << max_zoom), deg = 180.0 / wmr::kPi;
    const double u[2] = {(double)lo[0] / scale, ((double)hi[0] + 1.0) / scale}, v[2] = {(double)lo[1] / scale, ((double)hi[1] + 1.0) / scale};
    double lat[2], lng[2];
    pcv_wmr_to_lat_lng(2, u, v, lat, lng);
    bounds[0] = lng[0] * deg, bounds[1] = lat[1] * deg, bounds[2] = lng[1] * deg, bounds[3] = lat[0] * deg;  // west south east north
  }
  std::string s = "{\"scheme\":\"xyz\",\"format\":\"png\",\"tile_size\":" + std::to_string(kMapTilePx);
  s += ",\"minzoom\":" + std::to_string(min_zoom) + ",\"maxzoom\":" + std::to_string(max_zoom);
  s += ",\"bounds\":[" + f(bounds[0]) + "," + f(bounds[1]) + "," + f(bounds[2]) + "," + f(bounds[3]) + "]";
  s += ",\"tiles\":{";
  uint64_t at = 0;
  for (uint32_t k = 0; k < nz; ++k) {
    if (k) s += ",";
    s += "\"" + std::to_string(min_zoom + k) + "\":[";
    for (uint64_t i = 0; i < counts[k]; ++i, ++at) {
      if (i) s += ",";
      s += "[" + std::to_string(xy[2 * at]) + "," + std::to_string(xy[2 * at + 1]) + "]";
    }
    s += "]";
  }
  s += "}}";
  return s;
}

bool make_dir(const std::string& path) { return mkdir(path.c_str(), 0755) == 0 || errno == EEXIST; }

}  // namespace

extern "C" int pcv_maptiles_begin(pcv_ctx* ctx, const pcv_maptiles_params* params, pcv_maptiles** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  std::string why;
  if (check_params(params, params ? params->zoom : 0, &why)) return ctx->fail(PCV_E_INVALID, why);
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  pcv_maptiles* m = new (std::nothrow) pcv_maptiles;
  if (!m) return ctx->fail(PCV_E_OOM, "out of host memory");
  m->ctx = ctx, m->params = *params, m->min_zoom = params->zoom;
  uint32_t bits = 1;
  while ((1ull << bits) < 2 * params->max_tiles) ++bits;  // <= 23
  m->capacity = 1ull << bits;
  MapDev& d = m->dev;
  d.zoom = params->zoom, d.cap_mask = (uint32_t)(m->capacity - 1), d.shift = 64 - bits;
  d.max_tiles = (uint32_t)params->max_tiles, d.nslots_alloc = 0, d.background = params->background;
  m->cap_bytes = params->max_pool_bytes ? params->max_pool_bytes : (2ull << 30);
  int rc;
  if ((rc = alloc(m, &d.keys, m->capacity)) || (rc = alloc(m, &d.vals, m->capacity)) || (rc = alloc(m, &d.slot_key, params->max_tiles)) ||
      (rc = alloc(m, &d.slot_base, params->max_tiles)) || (rc = alloc(m, &d.ctr, kCtrs))) {
    m->release_all();
    delete m;
    return rc;
  }
  if (hipMemsetAsync(d.keys, 0xff, m->capacity * sizeof(uint64_t), ctx->stream) != hipSuccess ||
      hipMemsetAsync(d.vals, 0, m->capacity * sizeof(uint32_t), ctx->stream) != hipSuccess ||
      hipMemsetAsync(d.ctr, 0, kCtrs * sizeof(uint64_t), ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
    m->release_all();
    delete m;
    return ctx->fail(PCV_E_HIP, "map tiles: clearing the tile table failed");
  }
  *out = m;
  return PCV_OK;
}

extern "C" int pcv_maptiles_add_points(pcv_maptiles* m, uint64_t n, const double* x, const double* y, const double* z, const uint8_t* rgb, int mem) {
  if (!m) return PCV_E_INVALID;
  pcv_ctx* ctx = m->ctx;
  if (int rc = usable(m, false)) return rc;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (n && (!x || !y || !z || !rgb)) return ctx->fail(PCV_E_INVALID, "null point arrays");
  if (int rc = check_total(m, n)) return rc;
  if (n == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (mem == PCV_MEM_DEVICE) {
    if (int rc = add_device(m, n, x, y, z, rgb)) return rc;
  } else {
    const uint64_t piece = std::min(n, piece_points(m));
    if (int rc = reserve_staging(m, piece)) return rc;
    for (uint64_t at = 0; at < n; at += piece) {
      const uint64_t c = std::min(piece, n - at);
      int rc;
      if ((rc = ctx->h2d(m->sx, x + at, c * 8)) || (rc = ctx->h2d(m->sy, y + at, c * 8)) || (rc = ctx->h2d(m->sz, z + at, c * 8)) ||
          (rc = ctx->h2d(m->srgb, rgb + 3 * at, c * 3)) || (rc = add_device(m, c, m->sx, m->sy, m->sz, m->srgb)))
        return rc;
      PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the staging is refilled next
    }
  }
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_maptiles_add_query_batch(pcv_maptiles* m, pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments) {
  if (!m) return PCV_E_INVALID;
  if (int rc = usable(m, false)) return rc;
  if (!b || b->ctx != m->ctx) return m->ctx->fail(PCV_E_INVALID, "map tiles: the query batch is null or of another context");
  return add_segments(m, b->seg_off.data(), b->nseg, first_segment, num_segments, [&](uint64_t row0, uint64_t rows, uint8_t* out) {
    return pcv_ply_pack_xyz_rgb(source_of(b), first_segment, num_segments, row0, rows, out);
  });
}

extern "C" int pcv_maptiles_add_s2_query(pcv_maptiles* m, pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments) {
  if (!m) return PCV_E_INVALID;
  if (int rc = usable(m, false)) return rc;
  if (!q || !q->cloud || q->cloud->ctx != m->ctx) return m->ctx->fail(PCV_E_INVALID, "map tiles: the S2 query is null or of another context");
  return add_segments(m, q->seg_offset.data(), q->nseg, first_segment, num_segments, [&](uint64_t row0, uint64_t rows, uint8_t* out) {
    return pcv_ply_pack_xyz_rgb(source_of(q), first_segment, num_segments, row0, rows, out);
  });
}

namespace {

// pcv_maptiles_finish behind its checks; a failure leaves buffers half made, which the caller releases
int finish(pcv_maptiles* m) {
  pcv_ctx* ctx = m->ctx;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  MapDev& d = m->dev;
  uint64_t ctr[kCtrs];
  if (int rc = read_counters(m, ctr)) return rc;
  if (ctr[kCtrNoStorage]) return m->die(PCV_E_HIP, "map tiles: a point found no storage for its tile");
  m->dropped = ctr[kCtrDropped];
  m->free_staging();
  const uint32_t nslots = m->nslots;
  if (nslots > d.nslots_alloc) return m->die(PCV_E_HIP, "map tiles: more slots than storage");
  std::vector<uint64_t> slot_key(nslots);
  if (nslots) {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(slot_key.data(), d.slot_key, nslots * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  // every touched tile holds a drawn point; ascending by (x, y) is ascending by key
  std::vector<std::pair<uint64_t, uint32_t>> order(nslots);
  for (uint32_t s = 0; s < nslots; ++s) order[s] = {slot_key[s], s};
  std::sort(order.begin(), order.end());
  std::vector<uint32_t> out_slot(nslots);
  m->xy.resize(2ull * nslots);
  for (uint32_t k = 0; k < nslots; ++k) {
    m->xy[2 * k] = (uint32_t)(order[k].first >> 32), m->xy[2 * k + 1] = (uint32_t)order[k].first;
    out_slot[k] = order[k].second;
  }
  if (nslots) {
    int rc;
    if ((rc = alloc(m, &m->d_images, nslots * kTilePixels)) || (rc = alloc(m, &m->d_counts, nslots * kTilePixels))) {
      const std::string why = ctx->last_error;
      return m->die(rc, why);
    }
    PcvScratch sc(ctx);
    uint32_t* d_out_slot = nullptr;
    if ((rc = sc.get(&d_out_slot, nslots))) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_out_slot, out_slot.data(), nslots * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    for (uint32_t k0 = 0; k0 < nslots; k0 += kRows) {
      PcvProf prof(ctx, PCV_K_MAPTILES_RESOLVE);
      hipLaunchKernelGGL(maptiles_resolve_kernel, dim3((uint32_t)(kTilePixels / 256), std::min(kRows, nslots - k0)), dim3(256), 0, ctx->stream, d, k0,
                         (const uint32_t*)d_out_slot, m->d_images, m->d_counts);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = read_counters(m, ctr))) return rc;
    if (ctr[kCtrOverLimit])
      return m->die(PCV_E_INVALID, "map tiles: " + std::to_string(ctr[kCtrOverLimit]) + " pixels hold more than 2^24 points at zoom " +
                                       std::to_string(m->params.zoom) + ": choose a larger zoom");
  }
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  m->free_pool();  // the accumulators have been read for the last time
  m->free_table();
  m->finished = true;
  ctx->prof_resolve();
  return PCV_OK;
}

int build_parents(pcv_maptiles* m, uint32_t min_zoom) {
  pcv_ctx* ctx = m->ctx;
  const uint32_t zoom = m->params.zoom;
  const uint64_t nt = m->xy.size() / 2;
  std::vector<uint64_t> base(nt);
  for (uint64_t k = 0; k < nt; ++k) base[k] = pcv_maptiles_quad_index(zoom, m->xy[2 * k], m->xy[2 * k + 1]);
  XrayLevels lv;
  if (int rc = xray_build_levels(ctx, kMapTilePx, m->params.background, base, zoom, min_zoom, m->d_images, PCV_K_MAPTILES_PARENT, nullptr, &lv)) return rc;
  m->d_parents = lv.d_parents;
  m->levels.assign(zoom - min_zoom, Level{});
  for (uint32_t k = 0; k + 1 < lv.first.size() && k < zoom - min_zoom; ++k) {
    Level& level = m->levels[k];
    const uint32_t z = zoom - 1 - k;
    std::vector<std::pair<uint64_t, uint64_t>> tiles;  // (x << 32 | y, image)
    for (uint64_t p = lv.first[k]; p < lv.first[k + 1]; ++p) {
      uint32_t x, y;
      pcv_maptiles_quad_tile(z, lv.pindex[p], &x, &y);
      tiles.emplace_back(((uint64_t)x << 32) | y, p);
    }
    std::sort(tiles.begin(), tiles.end());
    for (const auto& t : tiles) {
      level.xy.push_back((uint32_t)(t.first >> 32));
      level.xy.push_back((uint32_t)t.first);
      level.image.push_back(t.second);
    }
  }
  m->min_zoom = min_zoom;
  m->parents_built = true;
  ctx->prof_resolve();
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_maptiles_finish(pcv_maptiles* m) {
  if (!m) return PCV_E_INVALID;
  if (int rc = usable(m, false)) return rc;
  const int rc = finish(m);
  if (rc != PCV_OK && !m->dead) {  // neither finished nor able to take points: everything goes, the handle can only be freed
    const std::string why = m->ctx->last_error;
    return m->die(rc, why);
  }
  return rc;
}

extern "C" int pcv_maptiles_build_parents(pcv_maptiles* m, uint32_t min_zoom) {
  if (!m) return PCV_E_INVALID;
  if (int rc = usable(m, true)) return rc;
  std::string why;
  if (check_params(&m->params, min_zoom, &why)) return m->ctx->fail(PCV_E_INVALID, why);
  if (m->parents_built)
    return min_zoom == m->min_zoom ? PCV_OK
                                   : m->ctx->fail(PCV_E_INVALID, "map tiles: the parents are built down to zoom " + std::to_string(m->min_zoom) + " already");
  return build_parents(m, min_zoom);
}

extern "C" int pcv_maptiles_info_get(const pcv_maptiles* m, pcv_maptiles_info* out) {
  if (!m || !out) return PCV_E_INVALID;
  std::memset(out, 0, sizeof *out);
  out->points_added = m->points_added, out->dropped = m->dropped;
  out->drawn = m->finished ? m->points_added - m->dropped : 0;
  out->pool_bytes = m->pool_bytes;
  out->zoom = m->params.zoom, out->min_zoom = m->min_zoom;
  out->finished = m->finished ? 1 : 0;
  out->tiles[m->params.zoom] = m->finished ? m->xy.size() / 2 : m->nslots;
  for (size_t k = 0; k < m->levels.size(); ++k) out->tiles[m->params.zoom - 1 - k] = m->levels[k].xy.size() / 2;
  return PCV_OK;
}

extern "C" int pcv_maptiles_tiles(const pcv_maptiles* m, uint32_t zoom, uint64_t capacity, uint32_t* xy, uint64_t* num_tiles) {
  if (!m) return PCV_E_INVALID;
  if (int rc = usable(m, true)) return rc;
  const std::vector<uint32_t>* tiles;
  if (int rc = check_range(m, zoom, 0, 0, &tiles)) return rc;
  const uint64_t n = tiles->size() / 2;
  if (num_tiles) *num_tiles = n;
  if (xy && std::min(n, capacity)) std::memcpy(xy, tiles->data(), std::min(n, capacity) * 2 * sizeof(uint32_t));
  return PCV_OK;
}

extern "C" int pcv_maptiles_images(pcv_maptiles* m, uint32_t zoom, uint64_t first, uint64_t count, int mem, uint8_t* rgba) {
  if (!m) return PCV_E_INVALID;
  pcv_ctx* ctx = m->ctx;
  const std::vector<uint32_t>* tiles;
  int rc;
  if ((rc = usable(m, true)) || (rc = check_range(m, zoom, first, count, &tiles))) return rc;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (count == 0) return PCV_OK;
  if (!rgba) return ctx->fail(PCV_E_INVALID, "null output");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  rc = queue_images(m, zoom, first, count, rgba, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return rc;
}

extern "C" int pcv_maptiles_counts(pcv_maptiles* m, uint64_t first, uint64_t count, int mem, uint32_t* out) {
  if (!m) return PCV_E_INVALID;
  pcv_ctx* ctx = m->ctx;
  const std::vector<uint32_t>* tiles;
  int rc;
  if ((rc = usable(m, true)) || (rc = check_range(m, m->params.zoom, first, count, &tiles))) return rc;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (count == 0) return PCV_OK;
  if (!out) return ctx->fail(PCV_E_INVALID, "null output");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, m->d_counts + first * kTilePixels, count * kTilePixels * sizeof(uint32_t),
                                    mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_maptiles_tile_pngs(pcv_maptiles* m, uint32_t zoom, uint64_t first, uint64_t count, int mode, uint64_t capacity, uint8_t* out,
                                      uint64_t* offsets) {
  if (!m) return PCV_E_INVALID;
  pcv_ctx* ctx = m->ctx;
  const std::vector<uint32_t>* tiles;
  int rc;
  if ((rc = usable(m, true)) || (rc = check_range(m, zoom, first, count, &tiles)) || (rc = check_png_mode(m, mode))) return rc;
  if (!offsets) return ctx->fail(PCV_E_INVALID, "null offsets");
  offsets[0] = 0;
  uint64_t at = 0, index = 0;
  bool fits = true;
  rc = ordered_tile_files(m, zoom, first, count, mode, [&](uint64_t, const uint8_t* file, uint64_t len) {
    if (out && len <= capacity - std::min(capacity, at)) std::memcpy(out + at, file, len);
    else if (out) fits = false;
    at += len;
    offsets[++index] = at;
    return true;
  });
  if (rc) return rc;
  if (!fits) return ctx->fail(PCV_E_INVALID, "map tiles: capacity below the " + std::to_string(at) + " bytes of these files");
  return PCV_OK;
}

extern "C" int pcv_maptiles_write_dir(pcv_maptiles* m, const char* directory, int png_mode) {
  if (!m) return PCV_E_INVALID;
  pcv_ctx* ctx = m->ctx;
  int rc;
  if ((rc = usable(m, true)) || (rc = check_png_mode(m, png_mode))) return rc;
  if (!directory) return ctx->fail(PCV_E_INVALID, "null directory");
  const std::string dir = directory;
  if (!make_dir(dir)) return ctx->fail(PCV_E_IO, "cannot create directory " + dir + ": " + strerror(errno));
  std::vector<uint64_t> counts;
  std::vector<uint32_t> all;
  for (uint32_t z = m->min_zoom; z <= m->params.zoom; ++z) {
    const std::vector<uint32_t>& xy = *m->tiles_of(z);
    const uint64_t n = xy.size() / 2;
    counts.push_back(n);
    all.insert(all.end(), xy.begin(), xy.end());
    if (n == 0) continue;
    const std::string zdir = dir + "/" + std::to_string(z);
    if (!make_dir(zdir)) return ctx->fail(PCV_E_IO, "cannot create directory " + zdir + ": " + strerror(errno));
    for (uint64_t k = 0; k < n; ++k)  // ascending by x: a new column is a new directory
      if (k == 0 || xy[2 * k] != xy[2 * k - 2]) {
        const std::string xdir = zdir + "/" + std::to_string(xy[2 * k]);
        if (!make_dir(xdir)) return ctx->fail(PCV_E_IO, "cannot create directory " + xdir + ": " + strerror(errno));
      }
    std::vector<std::string> why(n);
    rc = all_tile_files(m, z, png_mode, [&](uint64_t k, const uint8_t* file, uint64_t len) {
      return pcv_terrain_write_file(zdir + "/" + std::to_string(xy[2 * k]) + "/" + std::to_string(xy[2 * k + 1]) + ".png", file, (size_t)len, &why[k]) == PCV_OK;
    });
    if (rc == PCV_E_IO)
      for (const std::string& w : why)
        if (!w.empty()) return ctx->fail(PCV_E_IO, w);
    if (rc) return rc;
  }
  const std::string json = tiles_json(m->min_zoom, m->params.zoom, counts.data(), all.data());
  std::string why;
  if (int r = pcv_terrain_write_file(dir + "/tiles.json", json.data(), json.size(), &why)) return ctx->fail(r, why);
  return PCV_OK;
}

extern "C" void pcv_maptiles_free(pcv_maptiles* m) {
  if (!m) return;
  if (!m->dead) m->release_all();
  delete m;
}

// ---- host only, no context ------------------------------------------------------------------------------------------------
extern "C" int pcv_maptiles_check_params_host(const pcv_maptiles_params* params, uint32_t min_zoom) {
  std::string why;
  if (int rc = check_params(params, min_zoom, &why)) return pcv_host_fail(rc, why);
  return PCV_OK;
}

extern "C" int pcv_maptiles_pixels_host(uint32_t zoom, uint64_t n, const double* x, const double* y, const double* z, uint32_t* gx, uint32_t* gy,
                                        uint8_t* ok) {
  if (zoom > kMapTileMaxZoom) return pcv_host_fail(PCV_E_INVALID, "map tiles: zoom must be in 0 ..= 23, got " + std::to_string(zoom));
  if (n && (!x || !y || !z)) return pcv_host_fail(PCV_E_INVALID, "null point arrays");
  for (uint64_t k = 0; k < n; ++k) {
    uint32_t px, py;
    const bool good = pcv_maptiles_pixel(zoom, x[k], y[k], z[k], &px, &py);
    if (gx) gx[k] = px;
    if (gy) gy[k] = py;
    if (ok) ok[k] = good ? 1 : 0;
  }
  return PCV_OK;
}

extern "C" int pcv_maptiles_quad_index_host(uint32_t zoom, uint32_t x, uint32_t y, uint64_t* index) {
  if (!index) return pcv_host_fail(PCV_E_INVALID, "null output");
  if (zoom > kMapTileMaxZoom || (x >> zoom) || (y >> zoom))
    return pcv_host_fail(PCV_E_INVALID, "map tiles: tile (" + std::to_string(x) + ", " + std::to_string(y) + ") does not exist at zoom " + std::to_string(zoom));
  *index = pcv_maptiles_quad_index(zoom, x, y);
  return PCV_OK;
}

extern "C" int pcv_maptiles_quad_tile_host(uint32_t zoom, uint64_t index, uint32_t* x, uint32_t* y) {
  if (!x || !y) return pcv_host_fail(PCV_E_INVALID, "null output");
  if (zoom > kMapTileMaxZoom || (index >> (2 * zoom)))
    return pcv_host_fail(PCV_E_INVALID, "map tiles: index " + std::to_string(index) + " does not exist at zoom " + std::to_string(zoom));
  pcv_maptiles_quad_tile(zoom, index, x, y);
  return PCV_OK;
}

extern "C" int pcv_maptiles_json_host(uint32_t min_zoom, uint32_t max_zoom, const uint64_t* counts, const uint32_t* xy, char* buf, uint64_t cap,
                                      uint64_t* len) {
  if (max_zoom > kMapTileMaxZoom || min_zoom > max_zoom) return pcv_host_fail(PCV_E_INVALID, "map tiles: zooms must satisfy min_zoom <= max_zoom <= 23");
  if (!counts) return pcv_host_fail(PCV_E_INVALID, "null tile counts");
  uint64_t total = 0;
  for (uint32_t k = 0; k <= max_zoom - min_zoom; ++k) total += counts[k];
  if (total && !xy) return pcv_host_fail(PCV_E_INVALID, "null tile positions");
  const std::string s = tiles_json(min_zoom, max_zoom, counts, xy);
  if (len) *len = s.size();
  if (buf && cap) std::memcpy(buf, s.data(), (size_t)std::min<uint64_t>(cap, s.size()));
  return PCV_OK;
}
