// pcv_terrain.hip — terrain layers on the device (include/pcv_hip.h "terrain layers"): a keyed scatter-reduce of a
// point stream into a sparse grid of tiles, then a neighbourhood pass that crosses tile seams.
//   begin     the world box -> a vertex range and a dense u32 tile-slot table over the range's tiles
//   add       terrain_mark_kernel gives every tile a point touches a slot (one CAS per new tile); the host grows the pool of
//             per-vertex accumulators to the slots handed out; terrain_accum_kernel: one thread per point, the chain of
//             pcv_terrain_dev.h, then MAX / MIN: one no-return 64-bit atomicMax on ord(h) << 32 | rgb and one atomicAdd on
//             the count — MEAN: four 64-bit atomicAdds (hq, r, g, b: exact integers) and the count
//   queries   a result's rows in pieces cut at any row: the PLY output's packer (pcv_ply_pack_xyz_rgb) fills a bounded buffer of
//             27-byte rows, terrain_unpack_kernel spreads them into staging planes, then as add
//   finish    terrain_count_kernel (set vertices per slot), the tiles with a set vertex sorted by (x, y) on the host,
//             terrain_resolve_kernel (accumulators -> height, colour, count in the output layout), terrain_mask_kernel (the
//             set flags of a vertex's 3 x 3 neighbourhood through the tile table -> the quad mask), accumulators released
//   from_tiles / open_dir   a finished terrain from tiles made elsewhere (a directory written earlier): the tiles sorted by
//             (x, y) and copied to the device; no accumulators, no counts. pcv_terrain_layer_view hands the renderer
//             (pcv_render.hip) the tiles and a sorted key per tile, made on first use
// Every result is an exact function of the multiset of points: integer sums and a total-order maximum.
#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <new>

#include "pcv_internal.h"
#include "pcv_query_dev.h"
#include "pcv_result_rows.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_query_dev.h"
#include "pcv_terrain_dev.h"
#include "pcv_terrain_files.h"
#include "pcv_terrain_obj.h"

namespace {

constexpr uint32_t kNoTile = 0xffffffffu;
constexpr uint32_t kClaimed = 0xffffffffu;        // a table entry between its CAS and its slot
constexpr uint64_t kMaxTiles = 1ull << 22;
constexpr uint64_t kChunkBytes = 64ull << 20;     // the pool grows by doubling up to chunks of this size
constexpr uint64_t kLaunchPoints = 1ull << 30;    // points per launch of the two per-point kernels
constexpr double kMeanLimit = 2097152.0;          // 2^21
constexpr uint32_t kRows = 32768;                 // tiles per launch of the per-tile kernels (gridDim.y)

// what the kernels take by value
struct TerrainDev {
  PcvTerrainGrid grid;
  int64_t imin, imax, jmin, jmax;  // the declared vertex range
  int64_t tx0, ty0;                // first tile of the table
  uint32_t ntx, nty;
  uint32_t T, statistic;
  uint32_t min_points, nslots_alloc;  // slots that have storage
  uint64_t cells;                  // T * T
  uint32_t* table;                 // ntx * nty: 0 = untouched, else slot + 1
  uint32_t* slot_tile;             // slot -> index into the table
  uint64_t* slot_base;             // slot -> its accumulators: K * cells u64, then cells u32 counts
  uint64_t* ctr;                   // [0] outside, [1] slots handed out, [2] a point found no storage (never), [3] rendered quads
};

__device__ inline uint32_t words_per_vertex(uint32_t statistic) { return statistic == PCV_TERRAIN_MEAN ? 4u : 1u; }

// the vertex of point k and where it lands: false = dropped
__device__ inline bool locate(const TerrainDev& d, double px, double py, double pz, PcvTerrainVertex* v, uint64_t* tile, uint64_t* cell) {
  if (!pcv_terrain_vertex(d.grid, px, py, pz, v)) return false;
  if (v->i < d.imin || v->i > d.imax || v->j < d.jmin || v->j > d.jmax) return false;
  if (d.statistic == PCV_TERRAIN_MEAN && !(fabs(v->dz) < kMeanLimit)) return false;
  const int64_t T = (int64_t)d.T;
  const int64_t tx = pcv_terrain_floor_div(v->i, T) - d.tx0, ty = pcv_terrain_floor_div(v->j, T) - d.ty0;
  if (tx < 0 || ty < 0 || tx >= (int64_t)d.ntx || ty >= (int64_t)d.nty) return false;  // the range lies inside the table
  *tile = (uint64_t)ty * d.ntx + (uint64_t)tx;
  *cell = (uint64_t)pcv_terrain_floor_mod(v->j, T) * d.T + (uint64_t)pcv_terrain_floor_mod(v->i, T);
  return true;
}

__global__ __launch_bounds__(256) void terrain_mark_kernel(TerrainDev d, uint64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                          const double* __restrict__ z) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  PcvTerrainVertex v;
  uint64_t tile, cell;
  if (!locate(d, x[k], y[k], z[k], &v, &tile, &cell)) return;
  if (d.table[tile] != 0) return;
  if (atomicCAS(&d.table[tile], 0u, kClaimed) != 0u) return;
  const uint32_t slot = (uint32_t)atomicAdd((unsigned long long*)&d.ctr[1], 1ull);  // < ntx * nty: one slot per tile at most
  d.slot_tile[slot] = (uint32_t)tile;
  atomicExch(&d.table[tile], slot + 1);
}

__global__ __launch_bounds__(256) void terrain_accum_kernel(TerrainDev d, uint64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                           const double* __restrict__ z, const uint8_t* __restrict__ rgb) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool dropped = false;
  if (k < n) {
    PcvTerrainVertex v;
    uint64_t tile, cell;
    dropped = !locate(d, x[k], y[k], z[k], &v, &tile, &cell);
    if (!dropped) {
      const uint32_t slot = d.table[tile];
      if (slot == 0 || slot == kClaimed || slot - 1 >= d.nslots_alloc) {
        d.ctr[2] = 1;  // the mark pass and the host's growth cover every tile: a point without storage is a bug, not data
      } else {
        const uint32_t r = rgb[3 * k], g = rgb[3 * k + 1], b = rgb[3 * k + 2];
        uint64_t* w = (uint64_t*)d.slot_base[slot - 1];
        uint32_t* cnt = (uint32_t*)(w + (uint64_t)words_per_vertex(d.statistic) * d.cells);
        if (d.statistic == PCV_TERRAIN_MEAN) {
          atomicAdd((unsigned long long*)&w[cell], (unsigned long long)pcv_terrain_hq(v.dz));  // two's complement: a signed sum
          atomicAdd((unsigned long long*)&w[d.cells + cell], (unsigned long long)r);
          atomicAdd((unsigned long long*)&w[2 * d.cells + cell], (unsigned long long)g);
          atomicAdd((unsigned long long*)&w[3 * d.cells + cell], (unsigned long long)b);
        } else {
          atomicMax((unsigned long long*)&w[cell], (unsigned long long)pcv_terrain_key(v.h, r, g, b, d.statistic == PCV_TERRAIN_MIN));
        }
        atomicAdd(&cnt[cell], 1u);
      }
    }
  }
  const unsigned long long drops = __ballot(dropped);
  if ((threadIdx.x & 63) == 0 && drops) atomicAdd((unsigned long long*)&d.ctr[0], (unsigned long long)__popcll(drops));
}

// n packed rows (x y z as doubles at any alignment, then r g b; kPcvXyzRgbRowBytes each) into planes
__global__ __launch_bounds__(256) void terrain_unpack_kernel(uint64_t n, const uint8_t* __restrict__ rows, double* __restrict__ x, double* __restrict__ y,
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

// set vertices per slot: grid = (blocks per tile, slots)
__global__ __launch_bounds__(256) void terrain_count_kernel(TerrainDev d, uint32_t slot0, uint32_t* __restrict__ nset) {
  const uint32_t slot = slot0 + blockIdx.y;
  const uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  bool set = false;
  if (cell < d.cells) {
    const uint64_t* w = (const uint64_t*)d.slot_base[slot];
    const uint32_t* cnt = (const uint32_t*)(w + (uint64_t)words_per_vertex(d.statistic) * d.cells);
    set = cnt[cell] >= d.min_points;
  }
  const unsigned long long m = __ballot(set);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&nset[slot], (uint32_t)__popcll(m));
}

// accumulators -> the output layout: grid = (blocks per tile, kept tiles)
__global__ __launch_bounds__(256) void terrain_resolve_kernel(TerrainDev d, uint32_t tile0, const uint32_t* __restrict__ out_slot,
                                                             float* __restrict__ heights, uint8_t* __restrict__ colors, uint32_t* __restrict__ counts) {
  const uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (cell >= d.cells) return;
  const uint32_t tile = tile0 + blockIdx.y;
  const uint64_t o = (uint64_t)tile * d.cells + cell;
  const uint64_t* w = (const uint64_t*)d.slot_base[out_slot[tile]];
  const uint32_t* cnt = (const uint32_t*)(w + (uint64_t)words_per_vertex(d.statistic) * d.cells);
  const uint32_t c = cnt[cell];
  float h = 0.0f;
  uint32_t r = 0, g = 0, b = 0, a = 0;
  if (c >= d.min_points) {
    a = 255;
    if (d.statistic == PCV_TERRAIN_MEAN) {
      h = pcv_terrain_mean_height((int64_t)w[cell], c);
      r = pcv_terrain_mean_channel(w[d.cells + cell], c);
      g = pcv_terrain_mean_channel(w[2 * d.cells + cell], c);
      b = pcv_terrain_mean_channel(w[3 * d.cells + cell], c);
    } else {
      const uint64_t key = w[cell];
      h = pcv_terrain_key_height(key, d.statistic == PCV_TERRAIN_MIN);
      r = (uint32_t)(key >> 16) & 255u, g = (uint32_t)(key >> 8) & 255u, b = (uint32_t)key & 255u;
    }
  }
  heights[2 * o] = h;
  heights[2 * o + 1] = 0.0f;
  reinterpret_cast<uint32_t*>(colors)[o] = r | (g << 8) | (b << 16) | (a << 24);
  counts[o] = c;
}

// is vertex (i, j) set? through the tile table: the vertex may belong to any tile, kept or not, or to none
__device__ inline bool vertex_set(const TerrainDev& d, const uint32_t* __restrict__ slot_out, const uint32_t* __restrict__ counts, int64_t i,
                                  int64_t j) {
  const int64_t T = (int64_t)d.T;
  const int64_t tx = pcv_terrain_floor_div(i, T) - d.tx0, ty = pcv_terrain_floor_div(j, T) - d.ty0;
  if (tx < 0 || ty < 0 || tx >= (int64_t)d.ntx || ty >= (int64_t)d.nty) return false;
  const uint32_t slot = d.table[(uint64_t)ty * d.ntx + (uint64_t)tx];
  if (slot == 0 || slot - 1 >= d.nslots_alloc) return false;
  const uint32_t o = slot_out[slot - 1];
  if (o == kNoTile) return false;
  const uint64_t cell = (uint64_t)pcv_terrain_floor_mod(j, T) * d.T + (uint64_t)pcv_terrain_floor_mod(i, T);
  return counts[(uint64_t)o * d.cells + cell] >= d.min_points;
}

// the quad masks: grid = (blocks per tile, kept tiles); tile_pos: 2 x i32 per kept tile
__global__ __launch_bounds__(256) void terrain_mask_kernel(TerrainDev d, uint32_t tile0, const int32_t* __restrict__ tile_pos,
                                                          const uint32_t* __restrict__ slot_out, const uint32_t* __restrict__ counts,
                                                          float* __restrict__ heights) {
  const uint64_t cell = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t tile = tile0 + blockIdx.y;
  bool quad_here = false;
  if (cell < d.cells) {
    const uint64_t o = (uint64_t)tile * d.cells + cell;
    if (counts[o] >= d.min_points) {
      const int64_t i = (int64_t)tile_pos[2 * tile] * d.T + (int64_t)(cell % d.T);
      const int64_t j = (int64_t)tile_pos[2 * tile + 1] * d.T + (int64_t)(cell / d.T);
      bool s[3][3];  // s[dy + 1][dx + 1]
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) s[dy + 1][dx + 1] = (dx == 0 && dy == 0) || vertex_set(d, slot_out, counts, i + dx, j + dy);
      uint32_t m = 0;
      for (int qy = -1; qy <= 0; ++qy)
        for (int qx = -1; qx <= 0; ++qx)
          if (s[qy + 1][qx + 1] && s[qy + 1][qx + 2] && s[qy + 2][qx + 1] && s[qy + 2][qx + 2]) m |= pcv_terrain_quad_bit(i + qx, j + qy);
      quad_here = s[1][2] && s[2][1] && s[2][2];  // the quad whose lower corner is this vertex: each rendered quad counted once
      heights[2 * o + 1] = (float)m;
    }
  }
  const unsigned long long q = __ballot(quad_here);
  if ((threadIdx.x & 63) == 0 && q) atomicAdd((unsigned long long*)&d.ctr[3], (unsigned long long)__popcll(q));
}

}  // namespace

struct pcv_terrain {
  pcv_ctx* ctx = nullptr;
  pcv_terrain_params params{};
  TerrainDev dev{};
  uint32_t words = 1;          // u64 accumulators per vertex
  uint64_t tile_bytes = 0;     // accumulators of one tile
  uint64_t cap_bytes = 0, pool_bytes = 0;
  uint64_t ntiles = 0;         // entries of the table
  std::vector<void*> chunks;   // the pool
  std::vector<uint64_t> slot_base;  // host copy, [nslots_alloc]
  uint32_t nslots = 0;         // slots handed out by the device
  uint64_t points_added = 0, outside = 0, set_vertices = 0, rendered_quads = 0;
  // staging of host input and of query results
  double *sx = nullptr, *sy = nullptr, *sz = nullptr;
  uint8_t* srgb = nullptr;
  uint8_t* srows = nullptr;  // the query adders' packed rows, staging_cap of them
  uint64_t staging_cap = 0;
  bool finished = false, dead = false;
  // after finish
  std::vector<int32_t> positions;  // 2 per kept tile
  float* d_heights = nullptr;
  uint8_t* d_colors = nullptr;
  uint32_t* d_counts = nullptr;    // null for a terrain made from tiles
  int64_t* d_tile_keys = nullptr;  // the renderer's tile table (pcv_terrain_layer_view), made on first use
  bool from_tiles = false;

  void free_pool() {
    for (void* p : chunks) ctx->dev_free(p);
    chunks.clear();
    slot_base.clear();
    pool_bytes = 0;
    dev.nslots_alloc = 0;
  }
  void free_staging() {
    for (void* p : {(void*)sx, (void*)sy, (void*)sz, (void*)srgb, (void*)srows})
      if (p) ctx->dev_free(p);
    sx = sy = sz = nullptr, srgb = srows = nullptr, staging_cap = 0;
  }
  // everything on the device, after the stream has drained
  void release_all() {
    (void)hipStreamSynchronize(ctx->stream);
    free_pool();
    free_staging();
    for (void* p : {(void*)dev.table, (void*)dev.slot_tile, (void*)dev.slot_base, (void*)dev.ctr, (void*)d_heights, (void*)d_colors, (void*)d_counts,
                    (void*)d_tile_keys})
      if (p) ctx->dev_free(p);
    dev.table = dev.slot_tile = nullptr, dev.slot_base = dev.ctr = nullptr;
    d_heights = nullptr, d_colors = nullptr, d_counts = nullptr, d_tile_keys = nullptr;
  }
  int die(int code, const std::string& msg) {
    release_all();
    dead = true;
    return ctx->fail(code, msg);
  }
};

namespace {

int usable(pcv_terrain* t, bool want_finished) {
  if (t->dead) return t->ctx->fail(PCV_E_INVALID, "the terrain failed earlier and can only be freed");
  if (t->finished != want_finished)
    return t->ctx->fail(PCV_E_INVALID, want_finished       ? "the terrain is not finished"
                                       : t->from_tiles ? "the terrain was made from tiles: it takes no points"
                                                       : "the terrain is finished: no more points");
  return PCV_OK;
}

template <typename T>
int alloc(pcv_terrain* t, T** p, uint64_t count) {
  void* q = nullptr;
  if (int rc = t->ctx->dev_alloc(&q, std::max<uint64_t>(count, 1) * sizeof(T))) return rc;
  *p = (T*)q;
  return PCV_OK;
}

// reads the counters; the stream is idle afterwards
int read_counters(pcv_terrain* t, uint64_t out[4]) {
  pcv_ctx* ctx = t->ctx;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, t->dev.ctr, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 4; ++k) out[k] = ctx->mailbox[k];
  return PCV_OK;
}

// storage for the slots [nslots_alloc, want): chunks that double up to kChunkBytes, zeroed on the stream
int grow_pool(pcv_terrain* t, uint32_t want) {
  pcv_ctx* ctx = t->ctx;
  const uint32_t have = t->dev.nslots_alloc;
  if (want <= have) return PCV_OK;
  const uint64_t need = (uint64_t)(want - have);
  if (need > (t->cap_bytes - std::min(t->cap_bytes, t->pool_bytes)) / t->tile_bytes)
    return t->die(PCV_E_OOM, "terrain: " + std::to_string(want) + " touched tiles of " + std::to_string(t->tile_bytes) + " bytes pass max_pool_bytes = " +
                                 std::to_string(t->cap_bytes));
  {
    // what is asked for, or as much again as there is (up to a chunk): both fit, by the check above and want <= ntiles
    const uint64_t room = (t->cap_bytes - t->pool_bytes) / t->tile_bytes;
    const uint64_t by_size = std::max<uint64_t>(1, kChunkBytes / t->tile_bytes);
    const uint64_t tiles = std::min({std::max<uint64_t>(need, std::min<uint64_t>(by_size, have)), room, t->ntiles - (uint64_t)have});
    uint8_t* p = nullptr;
    if (int rc = alloc(t, &p, tiles * t->tile_bytes)) {
      const std::string why = ctx->last_error;
      return t->die(rc, why);
    }
    t->chunks.push_back(p);
    t->pool_bytes += tiles * t->tile_bytes;
    if (hipMemsetAsync(p, 0, tiles * t->tile_bytes, ctx->stream) != hipSuccess) return t->die(PCV_E_HIP, "hipMemsetAsync (terrain pool)");
    for (uint64_t k = 0; k < tiles; ++k) t->slot_base.push_back((uint64_t)(uintptr_t)(p + k * t->tile_bytes));
  }
  const uint32_t now = (uint32_t)t->slot_base.size();
  // the new entries only; pageable source, so the copy has left the vector when the call returns
  if (hipMemcpyAsync(t->dev.slot_base + have, t->slot_base.data() + have, (size_t)(now - have) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
    return t->die(PCV_E_HIP, "hipMemcpyAsync (terrain slot table)");
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return t->die(PCV_E_HIP, "hipStreamSynchronize (terrain slot table)");
  t->dev.nslots_alloc = now;
  return PCV_OK;
}

// n points in device memory
int add_device(pcv_terrain* t, uint64_t n, const double* x, const double* y, const double* z, const uint8_t* rgb) {
  pcv_ctx* ctx = t->ctx;
  for (uint64_t at = 0; at < n; at += kLaunchPoints) {
    const uint64_t m = std::min(kLaunchPoints, n - at);
    const dim3 grid((uint32_t)((m + 255) / 256)), block(256);
    {
      PcvProf prof(ctx, PCV_K_TERRAIN_MARK);
      hipLaunchKernelGGL(terrain_mark_kernel, grid, block, 0, ctx->stream, t->dev, m, x + at, y + at, z + at);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    uint64_t c[4];
    if (int rc = read_counters(t, c)) return rc;
    if (c[1] > t->ntiles) return t->die(PCV_E_HIP, "terrain: more slots than tiles");
    t->nslots = (uint32_t)c[1];
    if (int rc = grow_pool(t, t->nslots)) return rc;
    {
      PcvProf prof(ctx, PCV_K_TERRAIN_ACCUM);
      hipLaunchKernelGGL(terrain_accum_kernel, grid, block, 0, ctx->stream, t->dev, m, x + at, y + at, z + at, rgb + 3 * at);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  t->points_added += n;
  return PCV_OK;
}

int reserve_staging(pcv_terrain* t, uint64_t points) {
  if (points <= t->staging_cap) return PCV_OK;
  (void)hipStreamSynchronize(t->ctx->stream);  // a kernel may still read the old buffers
  t->free_staging();
  int rc;
  if ((rc = alloc(t, &t->sx, points)) || (rc = alloc(t, &t->sy, points)) || (rc = alloc(t, &t->sz, points)) || (rc = alloc(t, &t->srgb, 3 * points))) {
    t->free_staging();
    return rc;
  }
  t->staging_cap = points;
  return PCV_OK;
}

uint64_t piece_points(const pcv_terrain* t) { return t->params.staging_points ? t->params.staging_points : (1ull << 22); }

int check_total(pcv_terrain* t, uint64_t n) {
  if (n > 0xffffffffull - t->points_added) return t->ctx->fail(PCV_E_INVALID, "terrain: more than 2^32 - 1 points in total");
  return PCV_OK;
}

// segments [first, first + num) of a query result in pieces of at most staging_points rows, cut at any row: pack(row0, rows,
// out) packs a row range as x y z r g b rows (the PLY output's packer), terrain_unpack_kernel spreads them into the planes
template <typename Pack>
int add_segments(pcv_terrain* t, const uint64_t* seg_off, uint64_t nseg, uint64_t first, uint64_t num, Pack pack) {
  pcv_ctx* ctx = t->ctx;
  if (first > nseg || num > nseg - first) return ctx->fail(PCV_E_INVALID, "segment range past the end");
  const uint64_t p0 = seg_off[first], np = seg_off[first + num] - p0;
  if (int rc = check_total(t, np)) return rc;
  if (np == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint64_t piece = std::min(np, piece_points(t));
  int rc;
  if ((rc = reserve_staging(t, piece))) return rc;
  if (!t->srows && (rc = alloc(t, &t->srows, t->staging_cap * kPcvXyzRgbRowBytes))) return rc;
  for (uint64_t at = 0; at < np; at += piece) {
    const uint64_t m = std::min(piece, np - at);
    if ((rc = pack(p0 + at, m, t->srows))) return rc;
    {
      PcvProf prof(ctx, PCV_K_TERRAIN_UNPACK);
      hipLaunchKernelGGL(terrain_unpack_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, ctx->stream, m, (const uint8_t*)t->srows, t->sx, t->sy, t->sz,
                         t->srgb);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = add_device(t, m, t->sx, t->sy, t->sz, t->srgb))) return rc;
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the staging is refilled next
  }
  ctx->prof_resolve();
  return PCV_OK;
}

int check_range_output(const pcv_terrain* t, uint64_t first_tile, uint64_t num_tiles, int mem, const void* out) {
  const uint64_t have = t->positions.size() / 2;
  if (first_tile > have || num_tiles > have - first_tile) return t->ctx->fail(PCV_E_INVALID, "tile range past the end");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return t->ctx->fail(PCV_E_INVALID, "bad mem");
  if (num_tiles && !out) return t->ctx->fail(PCV_E_INVALID, "null output");
  return PCV_OK;
}

int copy_out(pcv_terrain* t, const void* src, uint64_t bytes, int mem, void* out) {
  pcv_ctx* ctx = t->ctx;
  if (bytes == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, src, bytes, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_terrain_begin(pcv_ctx* ctx, const pcv_terrain_params* params, const double bbox_min[3], const double bbox_max[3], pcv_terrain** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  std::string why;
  if (pcv_terrain_check_params(params, &why)) return ctx->fail(PCV_E_INVALID, why);
  if (!bbox_min || !bbox_max) return ctx->fail(PCV_E_INVALID, "null bounding box");
  const PcvTerrainGrid g = pcv_terrain_grid(*params);
  int64_t lo[2] = {INT64_MAX, INT64_MAX}, hi[2] = {INT64_MIN, INT64_MIN};
  for (int c = 0; c < 8; ++c) {
    PcvTerrainVertex v;
    const double px = (c & 1) ? bbox_max[0] : bbox_min[0], py = (c & 2) ? bbox_max[1] : bbox_min[1], pz = (c & 4) ? bbox_max[2] : bbox_min[2];
    // only u and v make the range: the corner goes through the chain with its height taken out
    PcvTerrainGrid flat = g;
    flat.m[6] = flat.m[7] = flat.m[8] = 0.0, flat.o[2] = 0.0;
    if (!std::isfinite(px) || !std::isfinite(py) || !std::isfinite(pz) || !pcv_terrain_vertex(flat, px, py, pz, &v))
      return ctx->fail(PCV_E_INVALID, "terrain: a corner of the bounding box has no grid vertex (not finite, or out of reach)");
    lo[0] = std::min(lo[0], v.i), hi[0] = std::max(hi[0], v.i), lo[1] = std::min(lo[1], v.j), hi[1] = std::max(hi[1], v.j);
  }
  const int64_t T = (int64_t)params->tile_size;
  int64_t t0[2], t1[2];
  for (int a = 0; a < 2; ++a) {
    lo[a] -= 1, hi[a] += 1;  // |i| < 2^62: no overflow
    t0[a] = pcv_terrain_floor_div(lo[a], T), t1[a] = pcv_terrain_floor_div(hi[a], T);
    if (t0[a] < INT32_MIN || t1[a] > INT32_MAX) return ctx->fail(PCV_E_INVALID, "terrain: tile positions outside i32");
  }
  const uint64_t ntx = (uint64_t)(t1[0] - t0[0] + 1), nty = (uint64_t)(t1[1] - t0[1] + 1);
  if (ntx > kMaxTiles || nty > kMaxTiles || ntx * nty > kMaxTiles)
    return ctx->fail(PCV_E_INVALID, "terrain: the bounding box covers " + std::to_string(ntx) + " x " + std::to_string(nty) + " tiles, more than 2^22");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  pcv_terrain* t = new (std::nothrow) pcv_terrain;
  if (!t) return ctx->fail(PCV_E_OOM, "out of host memory");
  t->ctx = ctx, t->params = *params;
  TerrainDev& d = t->dev;
  d.grid = g;
  d.imin = lo[0], d.imax = hi[0], d.jmin = lo[1], d.jmax = hi[1];
  d.tx0 = t0[0], d.ty0 = t0[1], d.ntx = (uint32_t)ntx, d.nty = (uint32_t)nty;
  d.T = params->tile_size, d.statistic = params->statistic, d.min_points = params->min_points, d.nslots_alloc = 0;
  d.cells = (uint64_t)d.T * d.T;
  t->words = params->statistic == PCV_TERRAIN_MEAN ? 4 : 1;
  t->tile_bytes = ((d.cells * (8ull * t->words + 4) + 7) / 8) * 8;
  t->cap_bytes = params->max_pool_bytes ? params->max_pool_bytes : (2ull << 30);
  t->ntiles = ntx * nty;
  int rc;
  if ((rc = alloc(t, &d.table, t->ntiles)) || (rc = alloc(t, &d.slot_tile, t->ntiles)) || (rc = alloc(t, &d.slot_base, t->ntiles)) || (rc = alloc(t, &d.ctr, 4))) {
    t->release_all();
    delete t;
    return rc;
  }
  if (hipMemsetAsync(d.table, 0, t->ntiles * sizeof(uint32_t), ctx->stream) != hipSuccess || hipMemsetAsync(d.ctr, 0, 4 * sizeof(uint64_t), ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) {
    t->release_all();
    delete t;
    return ctx->fail(PCV_E_HIP, "terrain: clearing the tile table failed");
  }
  *out = t;
  return PCV_OK;
}

extern "C" int pcv_terrain_add_points(pcv_terrain* t, uint64_t n, const double* x, const double* y, const double* z, const uint8_t* rgb, int mem) {
  if (!t) return PCV_E_INVALID;
  pcv_ctx* ctx = t->ctx;
  if (int rc = usable(t, false)) return rc;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (n && (!x || !y || !z || !rgb)) return ctx->fail(PCV_E_INVALID, "null point arrays");
  if (int rc = check_total(t, n)) return rc;
  if (n == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (mem == PCV_MEM_DEVICE) {
    if (int rc = add_device(t, n, x, y, z, rgb)) return rc;
  } else {
    const uint64_t piece = std::min(n, piece_points(t));
    if (int rc = reserve_staging(t, piece)) return rc;
    for (uint64_t at = 0; at < n; at += piece) {
      const uint64_t m = std::min(piece, n - at);
      int rc;
      if ((rc = ctx->h2d(t->sx, x + at, m * 8)) || (rc = ctx->h2d(t->sy, y + at, m * 8)) || (rc = ctx->h2d(t->sz, z + at, m * 8)) ||
          (rc = ctx->h2d(t->srgb, rgb + 3 * at, m * 3)) || (rc = add_device(t, m, t->sx, t->sy, t->sz, t->srgb)))
        return rc;
      PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the staging is refilled next
    }
  }
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_terrain_add_query_batch(pcv_terrain* t, pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments) {
  if (!t) return PCV_E_INVALID;
  if (int rc = usable(t, false)) return rc;
  if (!b || b->ctx != t->ctx) return t->ctx->fail(PCV_E_INVALID, "terrain: the query batch is null or of another context");
  return add_segments(t, b->seg_off.data(), b->nseg, first_segment, num_segments, [&](uint64_t row0, uint64_t rows, uint8_t* out) {
    return pcv_ply_pack_xyz_rgb(source_of(b), first_segment, num_segments, row0, rows, out);
  });
}

extern "C" int pcv_terrain_add_s2_query(pcv_terrain* t, pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments) {
  if (!t) return PCV_E_INVALID;
  if (int rc = usable(t, false)) return rc;
  if (!q || !q->cloud || q->cloud->ctx != t->ctx) return t->ctx->fail(PCV_E_INVALID, "terrain: the S2 query is null or of another context");
  return add_segments(t, q->seg_offset.data(), q->nseg, first_segment, num_segments, [&](uint64_t row0, uint64_t rows, uint8_t* out) {
    return pcv_ply_pack_xyz_rgb(source_of(q), first_segment, num_segments, row0, rows, out);
  });
}

namespace {

// pcv_terrain_finish behind its checks; a failure leaves buffers half made, which the caller releases
int finish(pcv_terrain* t) {
  pcv_ctx* ctx = t->ctx;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  TerrainDev& d = t->dev;
  uint64_t c[4];
  if (int rc = read_counters(t, c)) return rc;
  if (c[2]) return t->die(PCV_E_HIP, "terrain: a point found no storage for its tile");
  t->outside = c[0];
  t->free_staging();
  const uint32_t nslots = t->nslots;
  const uint32_t blocks = (uint32_t)((d.cells + 255) / 256);
  std::vector<uint32_t> slot_tile(nslots), nset(nslots), slot_out(nslots, kNoTile), out_slot;
  PcvScratch sc(ctx);
  uint32_t *d_nset = nullptr, *d_slot_out = nullptr, *d_out_slot = nullptr;
  int32_t* d_pos = nullptr;
  int rc;
  if (nslots) {
    if ((rc = sc.get(&d_nset, nslots)) || (rc = sc.get(&d_slot_out, nslots))) return rc;
    PCV_HIP_CHECK(ctx, hipMemsetAsync(d_nset, 0, nslots * sizeof(uint32_t), ctx->stream));
    for (uint32_t s0 = 0; s0 < nslots; s0 += kRows) {
      PcvProf prof(ctx, PCV_K_TERRAIN_COUNT);
      hipLaunchKernelGGL(terrain_count_kernel, dim3(blocks, std::min(kRows, nslots - s0)), dim3(256), 0, ctx->stream, d, s0, d_nset);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(nset.data(), d_nset, nslots * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(slot_tile.data(), d.slot_tile, nslots * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  // the tiles with a set vertex, ascending by (x, y)
  struct Kept {
    int32_t x, y;
    uint32_t slot;
  };
  std::vector<Kept> kept;
  t->set_vertices = 0;
  for (uint32_t s = 0; s < nslots; ++s) {
    if (slot_tile[s] >= t->ntiles) return t->die(PCV_E_HIP, "terrain: a slot names no tile");
    if (nset[s] == 0) continue;
    t->set_vertices += nset[s];
    kept.push_back(Kept{(int32_t)(d.tx0 + (int64_t)(slot_tile[s] % d.ntx)), (int32_t)(d.ty0 + (int64_t)(slot_tile[s] / d.ntx)), s});
  }
  std::sort(kept.begin(), kept.end(), [](const Kept& a, const Kept& b) { return a.x != b.x ? a.x < b.x : a.y < b.y; });
  const uint64_t nk = kept.size();
  t->positions.resize(2 * nk);
  out_slot.resize(nk);
  for (uint64_t k = 0; k < nk; ++k) {
    t->positions[2 * k] = kept[k].x, t->positions[2 * k + 1] = kept[k].y;
    out_slot[k] = kept[k].slot, slot_out[kept[k].slot] = (uint32_t)k;
  }
  t->rendered_quads = 0;
  if (nk) {
    if ((rc = alloc(t, &t->d_heights, nk * d.cells * 2)) || (rc = alloc(t, &t->d_colors, nk * d.cells * 4)) || (rc = alloc(t, &t->d_counts, nk * d.cells))) {
      const std::string why = ctx->last_error;
      return t->die(rc, why);
    }
    if ((rc = sc.get(&d_out_slot, nk)) || (rc = sc.get(&d_pos, 2 * nk))) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_out_slot, out_slot.data(), nk * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_slot_out, slot_out.data(), nslots * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_pos, t->positions.data(), 2 * nk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    for (uint64_t k0 = 0; k0 < nk; k0 += kRows) {
      PcvProf prof(ctx, PCV_K_TERRAIN_RESOLVE);
      hipLaunchKernelGGL(terrain_resolve_kernel, dim3(blocks, (uint32_t)std::min<uint64_t>(kRows, nk - k0)), dim3(256), 0, ctx->stream, d, (uint32_t)k0,
                         d_out_slot, t->d_heights, t->d_colors, t->d_counts);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    for (uint64_t k0 = 0; k0 < nk; k0 += kRows) {  // after every tile is resolved: a neighbour may be any kept tile
      PcvProf prof(ctx, PCV_K_TERRAIN_MASK);
      hipLaunchKernelGGL(terrain_mask_kernel, dim3(blocks, (uint32_t)std::min<uint64_t>(kRows, nk - k0)), dim3(256), 0, ctx->stream, d, (uint32_t)k0, d_pos,
                         d_slot_out, t->d_counts, t->d_heights);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    if ((rc = read_counters(t, c))) return rc;
    t->rendered_quads = c[3];
  }
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  t->free_pool();  // the accumulators have been read for the last time
  t->finished = true;
  ctx->prof_resolve();
  return PCV_OK;
}

}  // namespace

extern "C" int pcv_terrain_finish(pcv_terrain* t) {
  if (!t) return PCV_E_INVALID;
  if (int rc = usable(t, false)) return rc;
  const int rc = finish(t);
  if (rc != PCV_OK && !t->dead) {  // neither finished nor able to take points: everything goes, the handle can only be freed
    const std::string why = t->ctx->last_error;
    return t->die(rc, why);
  }
  return rc;
}

extern "C" int pcv_terrain_info_get(const pcv_terrain* t, pcv_terrain_info* out) {
  if (!t || !out) return PCV_E_INVALID;
  auto sat = [](int64_t v) { return (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v)); };
  std::memset(out, 0, sizeof *out);
  out->points_added = t->points_added, out->outside = t->outside;
  out->set_vertices = t->set_vertices, out->rendered_quads = t->rendered_quads;
  out->tiles = t->finished ? t->positions.size() / 2 : t->nslots;
  out->pool_bytes = t->pool_bytes;
  out->vertex_min[0] = sat(t->dev.imin), out->vertex_min[1] = sat(t->dev.jmin);
  out->vertex_max[0] = sat(t->dev.imax), out->vertex_max[1] = sat(t->dev.jmax);
  out->finished = t->finished ? 1 : 0;
  return PCV_OK;
}

extern "C" int pcv_terrain_tiles(const pcv_terrain* t, uint64_t capacity, int32_t* positions, uint64_t* num_tiles) {
  if (!t) return PCV_E_INVALID;
  if (int rc = usable(const_cast<pcv_terrain*>(t), true)) return rc;
  const uint64_t n = t->positions.size() / 2;
  if (num_tiles) *num_tiles = n;
  if (positions && std::min(n, capacity)) std::memcpy(positions, t->positions.data(), std::min(n, capacity) * 2 * sizeof(int32_t));
  return PCV_OK;
}

extern "C" int pcv_terrain_heights(pcv_terrain* t, uint64_t first_tile, uint64_t num_tiles, int mem, float* out) {
  if (!t) return PCV_E_INVALID;
  int rc;
  if ((rc = usable(t, true)) || (rc = check_range_output(t, first_tile, num_tiles, mem, out))) return rc;
  const uint64_t per = t->dev.cells * 2;
  return copy_out(t, t->d_heights + first_tile * per, num_tiles * per * sizeof(float), mem, out);
}

extern "C" int pcv_terrain_colors(pcv_terrain* t, uint64_t first_tile, uint64_t num_tiles, int mem, uint8_t* out) {
  if (!t) return PCV_E_INVALID;
  int rc;
  if ((rc = usable(t, true)) || (rc = check_range_output(t, first_tile, num_tiles, mem, out))) return rc;
  const uint64_t per = t->dev.cells * 4;
  return copy_out(t, t->d_colors + first_tile * per, num_tiles * per, mem, out);
}

extern "C" int pcv_terrain_counts(pcv_terrain* t, uint64_t first_tile, uint64_t num_tiles, int mem, uint32_t* out) {
  if (!t) return PCV_E_INVALID;
  int rc;
  if ((rc = usable(t, true))) return rc;
  if (t->from_tiles) return t->ctx->fail(PCV_E_INVALID, "the terrain was made from tiles: it has no point counts");
  if ((rc = check_range_output(t, first_tile, num_tiles, mem, out))) return rc;
  const uint64_t per = t->dev.cells;
  return copy_out(t, t->d_counts + first_tile * per, num_tiles * per * sizeof(uint32_t), mem, out);
}

extern "C" int pcv_terrain_write_dir(pcv_terrain* t, const char* directory) {
  if (!t) return PCV_E_INVALID;
  pcv_ctx* ctx = t->ctx;
  if (int rc = usable(t, true)) return rc;
  if (!directory) return ctx->fail(PCV_E_INVALID, "null directory");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const std::string dir = directory;
  if (mkdir(dir.c_str(), 0755) != 0 && errno != EEXIST) return ctx->fail(PCV_E_IO, "cannot create directory " + dir + ": " + strerror(errno));
  if (int rc = ctx->ring_ensure()) return rc;  // starts the host threads
  const uint64_t nk = t->positions.size() / 2, hbytes = t->dev.cells * 8, cbytes = t->dev.cells * 4;
  const uint64_t per_piece = std::max<uint64_t>(1, (64ull << 20) / (hbytes + cbytes));
  void* host = nullptr;
  if (nk)
    if (int rc = ctx->host_alloc(&host, std::min(nk, per_piece) * (hbytes + cbytes))) return rc;
  int rc = PCV_OK;
  for (uint64_t k0 = 0; k0 < nk && rc == PCV_OK; k0 += per_piece) {
    const uint64_t m = std::min(per_piece, nk - k0);
    uint8_t* hh = (uint8_t*)host;
    uint8_t* hc = hh + m * hbytes;
    if (hipMemcpyAsync(hh, t->d_heights + k0 * t->dev.cells * 2, m * hbytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(hc, t->d_colors + k0 * cbytes, m * cbytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
      rc = ctx->fail(PCV_E_HIP, "terrain: copying tiles to the host failed");
      break;
    }
    std::vector<int> frc(2 * m, PCV_OK);
    std::vector<std::string> fwhy(2 * m);
    ctx->host_pool.run((size_t)(2 * m), [&](size_t f) {
      const uint64_t k = f / 2;
      const std::string name = dir + "/" + pcv_terrain_tile_name(t->positions[2 * (k0 + k)], t->positions[2 * (k0 + k) + 1]);
      frc[f] = (f & 1) ? pcv_terrain_write_file(name + ".color", hc + k * cbytes, cbytes, &fwhy[f])
                       : pcv_terrain_write_file(name + ".height", hh + k * hbytes, hbytes, &fwhy[f]);
    });
    for (size_t f = 0; f < frc.size() && rc == PCV_OK; ++f)
      if (frc[f]) rc = ctx->fail(frc[f], fwhy[f]);
  }
  if (host) ctx->host_release(host);
  if (rc) return rc;
  const std::string json = pcv_terrain_meta_json(t->params, nk, t->positions.data());
  std::string why;
  if (int r = pcv_terrain_write_file(dir + "/meta.json", json.data(), json.size(), &why)) return ctx->fail(r, why);
  return PCV_OK;
}

extern "C" int pcv_terrain_from_tiles(pcv_ctx* ctx, const pcv_terrain_params* params, uint64_t num_tiles, const int32_t* positions, const float* heights,
                                      const uint8_t* colors, int mem, pcv_terrain** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  std::string why;
  if (pcv_terrain_check_params(params, &why)) return ctx->fail(PCV_E_INVALID, why);
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (num_tiles > kMaxTiles) return ctx->fail(PCV_E_INVALID, "terrain: more than 2^22 tiles");
  if (num_tiles && (!positions || !heights || !colors)) return ctx->fail(PCV_E_INVALID, "null tile arrays");
  // ascending by (x, y), as finish leaves them
  std::vector<uint64_t> order(num_tiles);
  for (uint64_t k = 0; k < num_tiles; ++k) order[k] = k;
  auto key = [&](uint64_t k) { return pcv_terrain_tile_key(positions[2 * k], positions[2 * k + 1]); };
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return key(a) < key(b); });
  for (uint64_t k = 1; k < num_tiles; ++k)
    if (key(order[k]) == key(order[k - 1]))
      return ctx->fail(PCV_E_INVALID, "terrain: tile (" + std::to_string(positions[2 * order[k]]) + ", " + std::to_string(positions[2 * order[k] + 1]) +
                                          ") is given twice");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  pcv_terrain* t = new (std::nothrow) pcv_terrain;
  if (!t) return ctx->fail(PCV_E_OOM, "out of host memory");
  t->ctx = ctx, t->params = *params;
  t->dev.grid = pcv_terrain_grid(*params);
  t->dev.T = params->tile_size, t->dev.statistic = params->statistic, t->dev.min_points = params->min_points;
  t->dev.cells = (uint64_t)t->dev.T * t->dev.T;
  t->from_tiles = true, t->finished = true;
  t->positions.resize(2 * num_tiles);
  for (uint64_t k = 0; k < num_tiles; ++k) t->positions[2 * k] = positions[2 * order[k]], t->positions[2 * k + 1] = positions[2 * order[k] + 1];
  int rc = PCV_OK;
  if (num_tiles) {
    const uint64_t hper = t->dev.cells * 2, cper = t->dev.cells * 4;
    if ((rc = alloc(t, &t->d_heights, num_tiles * hper)) || (rc = alloc(t, &t->d_colors, num_tiles * cper))) {
      t->release_all();
      delete t;
      return rc;
    }
    const hipMemcpyKind kind = mem == PCV_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    // runs of tiles that are already in order go in one copy each
    for (uint64_t k = 0; k < num_tiles && rc == PCV_OK;) {
      uint64_t n = 1;
      while (k + n < num_tiles && order[k + n] == order[k] + n) ++n;
      if (hipMemcpyAsync(t->d_heights + k * hper, heights + order[k] * hper, n * hper * sizeof(float), kind, ctx->stream) != hipSuccess ||
          hipMemcpyAsync(t->d_colors + k * cper, colors + order[k] * cper, n * cper, kind, ctx->stream) != hipSuccess)
        rc = ctx->fail(PCV_E_HIP, "terrain: copying tiles to the device failed");
      k += n;
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == PCV_OK) rc = ctx->fail(PCV_E_HIP, "terrain: copying tiles to the device failed");
    if (rc) {
      t->release_all();
      delete t;
      return rc;
    }
  }
  *out = t;
  return PCV_OK;
}

extern "C" int pcv_terrain_open_dir(pcv_ctx* ctx, const char* directory, pcv_terrain** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!directory || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  const std::string dir = directory;
  std::string text, why;
  if (int rc = pcv_terrain_read_text(dir + "/meta.json", &text, &why)) return ctx->fail(rc, why);
  pcv_terrain_params params;
  std::vector<int32_t> positions;
  if (int rc = pcv_terrain_meta_read(text.data(), text.size(), &params, &positions, &why)) return ctx->fail(rc, dir + "/" + why);
  const uint64_t n = positions.size() / 2, cells = (uint64_t)params.tile_size * params.tile_size;
  if (n > kMaxTiles) return ctx->fail(PCV_E_INVALID, "terrain: more than 2^22 tiles");
  std::vector<float> heights;
  std::vector<uint8_t> colors;
  try {
    heights.resize(n * cells * 2);
    colors.resize(n * cells * 4);
  } catch (const std::bad_alloc&) {
    return ctx->fail(PCV_E_OOM, "out of host memory");
  }
  if (int rc = ctx->ring_ensure()) return rc;  // starts the host threads
  std::vector<int> frc(2 * n, PCV_OK);
  std::vector<std::string> fwhy(2 * n);
  ctx->host_pool.run((size_t)(2 * n), [&](size_t f) {
    const uint64_t k = f / 2;
    const std::string name = dir + "/" + pcv_terrain_tile_name(positions[2 * k], positions[2 * k + 1]);
    frc[f] = (f & 1) ? pcv_terrain_read_file(name + ".color", colors.data() + k * cells * 4, cells * 4, &fwhy[f])
                     : pcv_terrain_read_file(name + ".height", heights.data() + k * cells * 2, cells * 8, &fwhy[f]);
  });
  for (size_t f = 0; f < frc.size(); ++f)
    if (frc[f]) return ctx->fail(frc[f], fwhy[f]);
  return pcv_terrain_from_tiles(ctx, &params, n, positions.data(), heights.data(), colors.data(), PCV_MEM_HOST, out);
}

int pcv_terrain_layer_view(pcv_terrain* t, pcv_ctx* ctx, PcvTerrainLayerView* out) {
  if (!t || t->ctx != ctx) return ctx->fail(PCV_E_INVALID, "render: a terrain layer is null or of another context");
  if (int rc = usable(t, true)) return rc;
  const uint64_t n = t->positions.size() / 2;
  if (n && !t->d_tile_keys) {
    std::vector<int64_t> keys(n);
    for (uint64_t k = 0; k < n; ++k) keys[k] = pcv_terrain_tile_key(t->positions[2 * k], t->positions[2 * k + 1]);
    if (int rc = alloc(t, &t->d_tile_keys, n)) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->d_tile_keys, keys.data(), n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the vector goes away
  }
  out->grid = t->dev.grid, out->T = t->dev.T, out->ntiles = n;
  out->d_tile_keys = t->d_tile_keys, out->d_heights = t->d_heights, out->d_colors = t->d_colors;
  return PCV_OK;
}

extern "C" void pcv_terrain_free(pcv_terrain* t) {
  if (!t) return;
  if (!t->dead) t->release_all();
  delete t;
}

// ---- host only, no context (pcv_terrain_files.cpp, pcv_terrain_dev.h) -------------------------------------------------------
extern "C" int pcv_terrain_check_params_host(const pcv_terrain_params* params) {
  std::string why;
  if (int rc = pcv_terrain_check_params(params, &why)) return pcv_host_fail(rc, why);
  return PCV_OK;
}

extern "C" int pcv_terrain_frame_host(const pcv_terrain_params* params, double frame[12]) {
  if (int rc = pcv_terrain_check_params_host(params)) return rc;
  if (!frame) return pcv_host_fail(PCV_E_INVALID, "null output");
  const PcvTerrainGrid g = pcv_terrain_grid(*params);
  for (int k = 0; k < 9; ++k) frame[k] = g.m[k];
  for (int k = 0; k < 3; ++k) frame[9 + k] = g.t[k];
  return PCV_OK;
}

extern "C" int pcv_terrain_vertex_host(const pcv_terrain_params* params, uint64_t n, const double* x, const double* y, const double* z, int64_t* i,
                                       int64_t* j, float* h, uint8_t* ok) {
  if (int rc = pcv_terrain_check_params_host(params)) return rc;
  if (n && (!x || !y || !z)) return pcv_host_fail(PCV_E_INVALID, "null point arrays");
  const PcvTerrainGrid g = pcv_terrain_grid(*params);
  for (uint64_t k = 0; k < n; ++k) {
    PcvTerrainVertex v;
    const bool good = pcv_terrain_vertex(g, x[k], y[k], z[k], &v);
    if (i) i[k] = v.i;
    if (j) j[k] = v.j;
    if (h) h[k] = v.h;
    if (ok) ok[k] = good ? 1 : 0;
  }
  return PCV_OK;
}

extern "C" int pcv_terrain_quad_masks_host(int64_t i0, int64_t j0, uint32_t w, uint32_t h, const uint8_t* set, uint32_t* masks) {
  if ((uint64_t)w * h && (!set || !masks)) return pcv_host_fail(PCV_E_INVALID, "null bitmap");
  if (w > (1u << 20) || h > (1u << 20)) return pcv_host_fail(PCV_E_INVALID, "window too large");
  pcv_terrain_quad_masks(i0, j0, w, h, set, masks);
  return PCV_OK;
}

extern "C" int pcv_terrain_tile_name_host(int32_t x, int32_t y, char* buf, uint64_t cap) {
  const std::string s = pcv_terrain_tile_name(x, y);
  if (!buf || cap < s.size() + 1) return pcv_host_fail(PCV_E_INVALID, "buffer too small for a tile name");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return PCV_OK;
}

extern "C" int pcv_terrain_meta_read_host(const char* json, uint64_t len, pcv_terrain_params* params, uint64_t capacity, int32_t* positions,
                                          uint64_t* num_tiles) {
  if (!json || !params) return pcv_host_fail(PCV_E_INVALID, "null argument");
  std::vector<int32_t> pos;
  std::string why;
  if (int rc = pcv_terrain_meta_read(json, (size_t)len, params, &pos, &why)) return pcv_host_fail(rc, why);
  const uint64_t n = pos.size() / 2;
  if (num_tiles) *num_tiles = n;
  if (positions && std::min(n, capacity)) std::memcpy(positions, pos.data(), std::min(n, capacity) * 2 * sizeof(int32_t));
  return PCV_OK;
}

extern "C" int pcv_render_terrain_window_host(const pcv_terrain_params* params, const double camera_position[3], uint32_t window, int64_t pos[2]) {
  if (int rc = pcv_terrain_check_params_host(params)) return rc;
  if (!camera_position || !pos) return pcv_host_fail(PCV_E_INVALID, "null argument");
  if (window < 2 || window > 1024 || (window & 1)) return pcv_host_fail(PCV_E_INVALID, "render: the terrain window must be even and in 2 ..= 1024");
  if (!pcv_terrain_window_pos(pcv_terrain_grid(*params), camera_position, window, pos)) return pcv_host_fail(PCV_E_INVALID, "Terrain location not representable.");
  return PCV_OK;
}

extern "C" int pcv_terrain_meta_json_host(const pcv_terrain_params* params, uint64_t num_tiles, const int32_t* positions, char* buf, uint64_t cap,
                                          uint64_t* len) {
  if (int rc = pcv_terrain_check_params_host(params)) return rc;
  if (num_tiles && !positions) return pcv_host_fail(PCV_E_INVALID, "null tile positions");
  const std::string s = pcv_terrain_meta_json(*params, num_tiles, positions);
  if (len) *len = s.size();
  if (buf && cap) std::memcpy(buf, s.data(), (size_t)std::min<uint64_t>(cap, s.size()));
  return PCV_OK;
}
