// pcv_ctx.hip — the context behind every entry point of the C ABI (include/pcv_hip.h): the caching device pool and its guard
// mode (pcv_ctx_set_pool_guard, a test hook), the pinned blocks, the host-thread pool and the host-to-device staging ring, the
// per-launch profile and its name table, and pcv_ctx_create / destroy / synchronize / wait_stream / signal_stream / trim.
// Host code only.
#include <algorithm>
#include <atomic>
#include <cstring>

#include "pcv_internal.h"

// ------------------------------------------------------------------------------------------------
// context, pool
// ------------------------------------------------------------------------------------------------
void* PcvPool::alloc(size_t bytes, hipError_t* err) {
  *err = hipSuccess;
  if (bytes == 0) bytes = 256;
  bytes = (bytes + 255) & ~(size_t)255;
  // Reuse a cached block only if it is about the requested size: a loose match lets a small request grab a big block
  // and the big request that follows pays a multi-millisecond hipMalloc in the middle of a build.
  auto it = free_blocks.lower_bound(bytes);
  if (it != free_blocks.end() && it->first <= bytes + bytes / 8 + (64u << 10)) {
    void* p = it->second;
    live[p] = it->first;
    live_bytes += it->first;
    peak_bytes = std::max(peak_bytes, live_bytes);
    free_blocks.erase(it);
    return p;
  }
  void* p = nullptr;
  *err = hipMalloc(&p, bytes);
  if (*err != hipSuccess) {
    // drop the cache and retry once
    trim();
    *err = hipMalloc(&p, bytes);
    if (*err != hipSuccess) return nullptr;
  }
  live[p] = bytes;
  live_bytes += bytes;
  peak_bytes = std::max(peak_bytes, live_bytes);
  return p;
}
void PcvPool::release(void* p) {
  if (!p) return;
  auto it = live.find(p);
  if (it == live.end()) return;
  free_blocks.insert({it->second, p});
  live_bytes -= it->second;
  live.erase(it);
}
void PcvPool::trim() {
  for (auto& kv : free_blocks) (void)hipFree(kv.second);
  free_blocks.clear();
}

int pcv_ctx::dev_alloc(void** p, size_t bytes) {
  if (guard.mode) return guard_alloc(p, bytes);
  hipError_t e;
  *p = pool.alloc(bytes, &e);
  if (!*p) return fail(e == hipErrorOutOfMemory ? PCV_E_OOM : PCV_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  return PCV_OK;
}
void pcv_ctx::dev_free(void* p) {
  if (guard.mode == 2) {
    auto it = guard.blocks.find(p);
    if (it == guard.blocks.end()) return;
    guard_sync();  // whatever still writes the block, on either stream, has to land before its fences are read
    guard_check(p, it->second);
    p = it->second.base;
    guard.blocks.erase(it);
  }
  pool.release(p);
}

// ---- guard mode (pcv_ctx_set_pool_guard): a test hook, DESIGN "The pool's contract" ----
// The block is painted on the context's stream and the call waits for it: a block may be used first on the side stream, and a
// poison that lands late would overwrite real data.
int pcv_ctx::guard_alloc(void** p, size_t bytes) {
  hipError_t e;
  *p = nullptr;
  uint8_t* base = (uint8_t*)pool.alloc(guard.mode == 2 ? pcv_guard_block_request(bytes) : bytes, &e);
  if (!base) return fail(e == hipErrorOutOfMemory ? PCV_E_OOM : PCV_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  ++guard.serial;
  uint8_t* user = base;
  hipError_t m = hipSuccess;
  if (guard.mode == 2) {
    PcvGuardLayout lay;
    if (!pcv_guard_layout(bytes, pool.live[base], &lay)) {
      pool.release(base);
      return fail(PCV_E_INVALID, "pool guard: the block is smaller than its layout");
    }
    user = base + lay.user_off;
    m = hipMemsetAsync(base, guard.canary, lay.user_off, stream);
    if (m == hipSuccess) m = hipMemsetAsync(base + lay.back_off, guard.canary, lay.back_bytes, stream);
    guard.blocks[user] = {base, bytes, guard.serial};
  }
  if (m == hipSuccess && bytes) m = hipMemsetAsync(user, guard.fill, bytes, stream);
  if (m == hipSuccess) m = hipStreamSynchronize(stream);
  if (m != hipSuccess) {
    guard.blocks.erase(user);
    pool.release(base);
    return fail(PCV_E_HIP, std::string("pool guard, painting a block: ") + hipGetErrorString(m));
  }
  *p = user;
  return PCV_OK;
}
void pcv_ctx::guard_sync() {
  (void)hipStreamSynchronize(stream);
  if (side) (void)hipStreamSynchronize(side);
}
// A damaged fence is counted, never an error of the call that found it.
void pcv_ctx::guard_check(void* user, const PcvPoolGuard::Block& b) {
  auto it = pool.live.find(b.base);
  PcvGuardLayout lay;
  if (it == pool.live.end() || !pcv_guard_layout(b.requested, it->second, &lay)) return;
  guard.host.resize(lay.user_off + lay.back_bytes);
  if (hipMemcpy(guard.host.data(), b.base, lay.user_off, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(guard.host.data() + lay.user_off, (const uint8_t*)b.base + lay.back_off, lay.back_bytes, hipMemcpyDeviceToHost) != hipSuccess)
    return;
  ++guard.checked;
  int64_t off = 0;
  if (!pcv_guard_first_damage(guard.host.data(), guard.host.data() + lay.user_off, lay, guard.canary, &off)) return;
  if (guard.damaged++ == 0) {
    guard.first_bytes = b.requested;
    guard.first_serial = b.serial;
    guard.first_offset = off;
  }
}

extern "C" int pcv_ctx_set_pool_guard(pcv_ctx* ctx, int mode, int fill) {
  if (!ctx) return PCV_E_INVALID;
  if (mode < 0 || mode > 2 || fill < 0 || fill > 255) return ctx->fail(PCV_E_INVALID, "pool guard: mode is 0, 1 or 2 and fill a byte");
  if (!ctx->pool.live.empty())
    return ctx->fail(PCV_E_INVALID, "pool guard: " + std::to_string(ctx->pool.live.size()) +
                                        " block(s) of the pool are live; set the guard before anything is built on the context");
  (void)hipSetDevice(ctx->device);
  ctx->guard_sync();
  ctx->pool.trim();  // no unfenced block survives into guard mode, no fenced one out of it
  ctx->guard = PcvPoolGuard();
  ctx->guard.mode = mode;
  ctx->guard.fill = (uint8_t)fill;
  ctx->guard.canary = pcv_guard_canary((uint8_t)fill);
  return PCV_OK;
}

extern "C" int pcv_ctx_pool_guard_check(pcv_ctx* ctx) {
  if (!ctx) return PCV_E_INVALID;
  if (ctx->guard.mode != 2) return ctx->fail(PCV_E_INVALID, "pool guard: no fences to check (mode 2 is not set)");
  (void)hipSetDevice(ctx->device);
  ctx->guard_sync();
  for (auto& kv : ctx->guard.blocks) ctx->guard_check(kv.first, kv.second);
  return PCV_OK;
}

extern "C" int pcv_ctx_pool_guard_report(pcv_ctx* ctx, uint64_t* checked, uint64_t* damaged, uint64_t* first_bytes,
                                         uint64_t* first_serial, int64_t* first_offset) {
  if (!ctx) return PCV_E_INVALID;
  if (checked) *checked = ctx->guard.checked;
  if (damaged) *damaged = ctx->guard.damaged;
  if (first_bytes) *first_bytes = ctx->guard.first_bytes;
  if (first_serial) *first_serial = ctx->guard.first_serial;
  if (first_offset) *first_offset = ctx->guard.first_offset;
  return PCV_OK;
}

// Host code and hipMemset / hipMemcpy only: the guard shown to work on a block of the caller's size, and one byte planted
// at user + offset for the report to find. The steps are those of the header's comment.
extern "C" int pcv_ctx_pool_guard_selftest(pcv_ctx* ctx, uint64_t bytes, int64_t offset) {
  if (!ctx) return PCV_E_INVALID;
  if (ctx->guard.mode != 2) return ctx->fail(PCV_E_INVALID, "pool guard selftest: mode 2 is not set");
  (void)hipSetDevice(ctx->device);
  std::vector<uint8_t> back(bytes);
  void *first = nullptr, *p = nullptr;
  void* first_base = nullptr;
  for (int round = 0; round < 2; ++round) {
    if (int rc = ctx->dev_alloc(&p, bytes)) return rc;
    const PcvPoolGuard::Block blk = ctx->guard.blocks[p];
    if (round == 0) {
      first = p;
      first_base = blk.base;
    } else if (p != first || blk.base != first_base) {
      ctx->dev_free(p);
      return ctx->fail(PCV_E_INVALID, "pool guard selftest: the second request was not served from the cache");
    }
    if (bytes && hipMemcpy(back.data(), p, bytes, hipMemcpyDeviceToHost) != hipSuccess) {
      ctx->dev_free(p);
      return ctx->fail(PCV_E_HIP, "pool guard selftest: copying the block back failed");
    }
    const int64_t bad = pcv_guard_first_unfilled(back.data(), bytes, ctx->guard.fill);
    if (bad >= 0) {
      ctx->dev_free(p);
      return ctx->fail(PCV_E_INVALID, std::string("pool guard selftest: byte ") + std::to_string(bad) + " of a " +
                                          (round ? "recycled" : "fresh") + " block is not the fill");
    }
    if (round == 0) {  // a pattern that is neither fill nor canary, for the second round to find if the fill is missing
      const uint8_t inverse = (uint8_t)~ctx->guard.fill, pattern = inverse == ctx->guard.canary ? (uint8_t)0x33 : inverse;
      hipError_t e = bytes ? hipMemsetAsync(p, pattern, bytes, ctx->stream) : hipSuccess;
      ctx->dev_free(p);  // (waits for the stream)
      if (e != hipSuccess) return ctx->fail(PCV_E_HIP, "pool guard selftest: hipMemset");
      continue;
    }
    // the planted byte must lie in memory the block owns
    const size_t block_bytes = ctx->pool.live[blk.base];
    const int64_t lo = -(int64_t)kPcvGuardFront, hi = (int64_t)(block_bytes - kPcvGuardFront);
    if (offset < lo || offset >= hi) {
      ctx->dev_free(p);
      return ctx->fail(PCV_E_INVALID, "pool guard selftest: offset " + std::to_string(offset) + " is outside the block [" +
                                          std::to_string(lo) + ", " + std::to_string(hi) + ")");
    }
    hipError_t e = hipMemsetAsync((uint8_t*)p + offset, (uint8_t)(ctx->guard.canary ^ 0x80), 1, ctx->stream);
    ctx->dev_free(p);  // (waits for the stream, then reads the fences)
    if (e != hipSuccess) return ctx->fail(PCV_E_HIP, "pool guard selftest: hipMemset");
  }
  return PCV_OK;
}

int pcv_ctx::host_alloc(void** p, size_t bytes) {
  const size_t asked = bytes;
  if (bytes == 0) bytes = 256;
  auto it = host_free.lower_bound(bytes);
  if (it != host_free.end() && it->first <= bytes * 2 + (1u << 20)) {
    *p = it->second;
    host_live[*p] = it->first;
    host_free.erase(it);
    if (guard.mode) std::memset(*p, guard.fill, asked);
    return PCV_OK;
  }
  hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
  if (e != hipSuccess) return fail(PCV_E_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  host_live[*p] = bytes;
  if (guard.mode) std::memset(*p, guard.fill, asked);
  return PCV_OK;
}
void pcv_ctx::host_release(void* p) {
  if (!p) return;
  auto it = host_live.find(p);
  if (it == host_live.end()) return;
  host_free.insert({it->second, p});
  host_live.erase(it);
}
int pcv_ctx::pinned_reserve(size_t bytes) {
  if (bytes <= pinned_bytes) return PCV_OK;
  if (pinned) (void)hipHostFree(pinned);
  pinned = nullptr;
  pinned_bytes = 0;
  hipError_t e = hipHostMalloc(&pinned, bytes, hipHostMallocDefault);
  if (e != hipSuccess) return fail(PCV_E_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  pinned_bytes = bytes;
  return PCV_OK;
}

int pcv_ctx::table_dev_reserve(size_t bytes) {
  // guard mode: the block has one user, the node tables of pcv_build.hip, and every reserve there starts a new set of tables
  // that the build writes before it reads them, so the block is filled like a pool block. No fence: it is no pool block.
  if (guard.mode && bytes <= table_dev_bytes) {
    guard_sync();
    if (hipMemsetAsync(table_dev, guard.fill, table_dev_bytes, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
      return fail(PCV_E_HIP, "pool guard, painting the node tables");
  }
  if (bytes <= table_dev_bytes) return PCV_OK;
  // the old block may still be read by work in flight: drain both streams before it goes away
  if (table_dev) {
    (void)hipStreamSynchronize(stream);
    (void)hipStreamSynchronize(side);
    (void)hipFree(table_dev);
    table_dev = nullptr;
    table_dev_bytes = 0;
  }
  const size_t want = (bytes + (bytes >> 1) + 4095) & ~(size_t)4095;
  if (hipMalloc(&table_dev, want) != hipSuccess) return fail(PCV_E_OOM, "out of device memory (node tables)");
  table_dev_bytes = want;
  if (guard.mode) {
    guard_sync();
    if (hipMemsetAsync(table_dev, guard.fill, table_dev_bytes, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess)
      return fail(PCV_E_HIP, "pool guard, painting the node tables");
  }
  return PCV_OK;
}

int pcv_ctx::pinned_spec_reserve(size_t bytes) {
  if (bytes <= pinned_spec_bytes) return PCV_OK;
  bytes += bytes / 2;  // the size follows the node count of the input: leave room so that similar builds do not regrow it
  if (pinned_spec) (void)hipHostFree(pinned_spec);  // waits for copies in flight
  pinned_spec = nullptr;
  pinned_spec_bytes = 0;
  hipError_t e = hipHostMalloc(&pinned_spec, bytes, hipHostMallocDefault);
  if (e != hipSuccess) return fail(PCV_E_OOM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  pinned_spec_bytes = bytes;
  return PCV_OK;
}

void PcvHostPool::start(unsigned n) {
  if (!threads.empty()) return;
  for (unsigned k = 0; k < n; ++k)
    threads.emplace_back([this] {
      uint64_t seen = 0;
      for (;;) {
        std::unique_lock<std::mutex> lk(mu);
        wake.wait(lk, [&] { return stop || (generation != seen && next < count); });
        if (stop) return;
        while (next < count) {
          const size_t i = next++;
          lk.unlock();
          job(i);
          lk.lock();
          if (++finished == count) done.notify_all();
        }
        seen = generation;
      }
    });
}
void PcvHostPool::run(size_t n, const std::function<void(size_t)>& fn) {
  if (n == 0) return;
  if (threads.empty() || n == 1) {
    for (size_t i = 0; i < n; ++i) fn(i);
    return;
  }
  std::unique_lock<std::mutex> lk(mu);
  job = fn;
  next = 0;
  count = n;
  finished = 0;
  ++generation;
  wake.notify_all();
  while (next < count) {  // the caller works too
    const size_t i = next++;
    lk.unlock();
    fn(i);
    lk.lock();
    ++finished;
  }
  done.wait(lk, [&] { return finished == count; });
  count = 0;
}
PcvHostPool::~PcvHostPool() {
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  wake.notify_all();
  for (auto& th : threads) th.join();
}

// Pageable caller memory -> device: the runtime's own staging of a pageable hipMemcpy runs on one thread (~45 GB/s
// here); several host threads filling a ring of pinned chunks keep the link busy instead (every chunk is one DMA).
int pcv_ctx::h2d(void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return PCV_OK;
  if (bytes < (4u << 20)) {  // small arrays: not worth the ring
    PCV_HIP_CHECK(this, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
    return PCV_OK;
  }
  const uint8_t* from = (const uint8_t*)src;
  return h2d_fill(dst, bytes, [from](uint8_t* to, size_t off, size_t len) {
    std::memcpy(to, from + off, len);
    return true;
  });
}

// The ring of pinned chunks and the host threads that fill them, created on first use (h2d_fill, pcv_ingest_begin).
int pcv_ctx::ring_ensure() {
  if (ring[0]) return PCV_OK;
  for (int k = 0; k < kRingSlots; ++k) {
    if (hipHostMalloc(&ring[k], kRingChunk, hipHostMallocDefault) != hipSuccess) return fail(PCV_E_OOM, "hipHostMalloc (staging ring)");
    if (hipEventCreateWithFlags(&ring_ev[k], hipEventDisableTiming) != hipSuccess) return fail(PCV_E_HIP, "hipEventCreate");
  }
  unsigned hw = std::thread::hardware_concurrency();
  // copies into pinned memory saturate the link with 7 threads; preads from a file (pcv_build_octree_from_ply) want more
  unsigned workers = hw >= 64 ? 15 : (hw >= 16 ? 7 : (hw > 2 ? hw / 2 - 1 : 0));
  host_pool.start(workers);
  return PCV_OK;
}

// Host -> device through the ring of pinned chunks: `fill(to, off, len)` produces bytes [off, off + len) of the source
// into pinned memory (a memcpy from pageable memory, a pread from a file) and is called from the context's host threads,
// 2 MiB per call, several calls in parallel; one DMA per 32 MiB chunk follows. false from `fill` -> PCV_E_IO.
int pcv_ctx::h2d_fill(void* dst, size_t bytes, const std::function<bool(uint8_t*, size_t, size_t)>& fill) {
  if (bytes == 0) return PCV_OK;
  if (int rc = ring_ensure()) return rc;
  // one part per worker (the caller works too) and chunk, not less than 256 KiB
  const size_t nworkers = host_pool.threads.size() + 1;
  const size_t kPart = std::max<size_t>(256u << 10, ((kRingChunk + nworkers - 1) / nworkers + 4095) & ~(size_t)4095);
  std::atomic<int> bad{0};
  for (size_t off = 0; off < bytes; off += kRingChunk) {
    const size_t len = bytes - off < kRingChunk ? bytes - off : kRingChunk;
    const int slot = ring_take();
    if (ring_busy[slot]) PCV_HIP_CHECK(this, hipEventSynchronize(ring_ev[slot]));  // its previous DMA has left the chunk
    uint8_t* chunk = (uint8_t*)ring[slot];
    host_pool.run((len + kPart - 1) / kPart, [&](size_t p) {
      const size_t b = p * kPart, e = b + kPart < len ? b + kPart : len;
      if (!fill(chunk + b, off + b, e - b)) bad.store(1);
    });
    if (bad.load()) return fail(PCV_E_IO, "reading the source of a host-to-device copy failed");
    PCV_HIP_CHECK(this, hipMemcpyAsync((uint8_t*)dst + off, chunk, len, hipMemcpyHostToDevice, stream));
    PCV_HIP_CHECK(this, hipEventRecord(ring_ev[slot], stream));
    ring_busy[slot] = true;
  }
  return PCV_OK;
}

hipEvent_t pcv_ctx::prof_event() {
  if (!prof_free.empty()) {
    hipEvent_t e = prof_free.back();
    prof_free.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
// Call only after the stream has been synchronised.
void pcv_ctx::prof_resolve() {
  for (auto& p : prof_pending) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      prof_ms[p.id] += ms;
      prof_launches[p.id] += 1;
    }
    prof_free.push_back(p.a);
    prof_free.push_back(p.b);
  }
  prof_pending.clear();
}

static const char* kKernelNames[PCV_K_COUNT] = {
    "aabb_partial_kernel", "chain_keys_kernel",  "upsweep_kernel<u64>",   "scan_kernel",
    "downsweep_kernel<u64>", "split_search_kernel", "split_assign_kernel", "leaf_encode_kernel",
    "upsweep_kernel<u32>", "downsweep_kernel<u32>", "promote_settle_kernel", "downsweep_rec_kernel", "cull_nodes_kernel",
    "visible_nodes_kernel", "nodes_in_location_kernel", "cull_points_kernel", "transform_points_kernel",
    "query_compact_kernel", "route_bucket_kernel", "partition_count_kernel", "partition_scatter_kernel",
    "promote_climb_kernel", "spec_encode_kernel", "rank_hist_kernel", "spec_continue_kernel", "spec_replay_kernel", "upsweep_map_kernel",
    "hist_from_rows_kernel", "cull_nodes_sparse_kernel", "downsweep_settle_kernel", "ingest_batch_kernel",
    "batch_nodes_kernel", "batch_chunks_kernel", "batch_flags_kernel", "batch_scan_kernel", "batch_compact_kernel",
    "xray_bin_kernel", "xray_scatter_kernel", "xray_accum_kernel", "xray_parent_kernel",
    "xray_sorted_kernel", "render_chunks_kernel", "render_splat_kernel", "render_resolve_kernel",
    "xray_merge_stage_copy", "xray_merge_parent_kernel", "xray_png_band_kernel", "xray_png_layout_kernel",
    "xray_png_gather_kernel", "render_outline_kernel", "xray_inpaint_stitch_kernel", "xray_inpaint_row_kernel",
    "xray_inpaint_col_kernel", "xray_inpaint_list_kernel", "xray_inpaint_fill_kernel", "xray_inpaint_blend_kernel",
    "s2_ids_kernel", "s2_unique_kernel", "s2_rank_kernel", "s2_gather_kernel", "s2_union_kernel",
    "s2_cell_table_kernel", "s2_location_kernel", "s2_pair_kernel", "s2_flags_kernel", "s2_gather_points_kernel",
    "union_node_rects_kernel", "s2_merge_kernel", "s2_attr_gather_kernel", "s2_attr_merge_kernel", "s2_attr_filter_kernel",
    "s2_attr_gather_points_kernel", "ply_rows_kernel", "terrain_mark_kernel", "terrain_accum_kernel", "terrain_unpack_kernel", "terrain_count_kernel",
    "terrain_resolve_kernel", "terrain_mask_kernel", "render_terrain_gather_kernel", "render_terrain_edges_kernel",
    "maptiles_project_kernel", "maptiles_mark_kernel", "maptiles_accum_kernel", "maptiles_unpack_kernel", "maptiles_resolve_kernel",
    "maptiles_parent_kernel", "las_tile_count_kernel", "las_tile_scan_kernel", "las_decode_kernel", "las_color_kernel", "tiles3d_pack_kernel",
    "las_records_kernel", "las_min_kernel"};
static_assert(sizeof(kKernelNames) / sizeof(kKernelNames[0]) == PCV_K_COUNT, "kernel name table out of sync");

extern "C" int pcv_ctx_set_profiling(pcv_ctx* ctx, int enabled) {
  if (!ctx) return PCV_E_INVALID;
  ctx->profiling = enabled == 2 ? 2 : (enabled != 0 ? 1 : 0);
  return PCV_OK;
}
extern "C" int pcv_ctx_reset_kernel_stats(pcv_ctx* ctx) {
  if (!ctx) return PCV_E_INVALID;
  for (int i = 0; i < PCV_K_COUNT; ++i) {
    ctx->prof_launches[i] = 0;
    ctx->prof_ms[i] = 0;
  }
  return PCV_OK;
}
extern "C" int pcv_ctx_kernel_stats(pcv_ctx* ctx, int kernel_id, const char** name, uint64_t* launches,
                                    double* total_ms) {
  if (!ctx) return PCV_E_INVALID;
  if (kernel_id < 0 || kernel_id >= PCV_K_COUNT) return PCV_K_COUNT;
  if (!ctx->prof_pending.empty()) {  // launches of the stage-level entry points are resolved on first read
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->prof_resolve();
  }
  if (name) *name = kKernelNames[kernel_id];
  if (launches) *launches = ctx->prof_launches[kernel_id];
  if (total_ms) *total_ms = ctx->prof_ms[kernel_id];
  return PCV_K_COUNT;
}

extern "C" int pcv_ctx_pool_stats(pcv_ctx* ctx, uint64_t* live_bytes, uint64_t* peak_bytes, int reset_peak) {
  if (!ctx) return PCV_E_INVALID;
  if (live_bytes) *live_bytes = ctx->pool.live_bytes;
  if (peak_bytes) *peak_bytes = ctx->pool.peak_bytes;
  if (reset_peak) ctx->pool.peak_bytes = ctx->pool.live_bytes;
  return PCV_OK;
}

extern "C" int pcv_abi_version(void) { return PCV_ABI_VERSION; }

extern "C" int pcv_ctx_create(int device, void* stream, pcv_ctx** out) {
  if (!out) return PCV_E_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return PCV_E_HIP;
  if (hipSetDevice(device) != hipSuccess) return PCV_E_HIP;
  pcv_ctx* c = new pcv_ctx();
  c->device = device;
  if (hipHostMalloc((void**)&c->mailbox, kPcvMailboxSlots * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
    delete c;
    return PCV_E_OOM;
  }
  if (hipHostGetDevicePointer((void**)&c->mailbox_dev, c->mailbox, 0) != hipSuccess) c->mailbox_dev = c->mailbox;
  if (stream) {
    c->stream = (hipStream_t)stream;
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return PCV_E_HIP;
    }
    c->own_stream = true;
  }
  for (auto& e : c->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      delete c;
      return PCV_E_HIP;
    }
  for (int k = 0; k < PCV_NUM_STAGES; ++k)
    if (hipEventCreate(&c->stage_b[k]) != hipSuccess || hipEventCreate(&c->stage_e[k]) != hipSuccess) {
      delete c;
      return PCV_E_HIP;
    }
  if (hipEventCreateWithFlags(&c->spec_ev, hipEventDisableTiming) != hipSuccess) {
    delete c;
    return PCV_E_HIP;
  }
  if (hipEventCreateWithFlags(&c->xev, hipEventDisableTiming) != hipSuccess) {
    delete c;
    return PCV_E_HIP;
  }
  if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&c->side_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->side_join, hipEventDisableTiming) != hipSuccess) {
    delete c;
    return PCV_E_HIP;
  }
  *out = c;
  return PCV_OK;
}

extern "C" void pcv_ctx_destroy(pcv_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->pool.trim();
  if (ctx->guard.mode == 2) {  // blocks still live: their fences are read like those of a freed block
    ctx->guard_sync();
    for (auto& kv : ctx->guard.blocks) ctx->guard_check(kv.first, kv.second);
  }
  {
    for (auto& kv : ctx->pool.live) (void)hipFree(kv.first);  // (base addresses, with the guard on as well)
  }
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->pinned_spec) (void)hipHostFree(ctx->pinned_spec);
  for (int k = 0; k < pcv_ctx::kRingSlots; ++k) {
    if (ctx->ring[k]) (void)hipHostFree(ctx->ring[k]);
    if (ctx->ring_ev[k]) (void)hipEventDestroy(ctx->ring_ev[k]);
  }
  if (ctx->mailbox) (void)hipHostFree(ctx->mailbox);
  for (auto& kv : ctx->host_free) (void)hipHostFree(kv.second);
  for (auto& kv : ctx->host_live) (void)hipHostFree(kv.first);
  for (auto& e : ctx->ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->xev) (void)hipEventDestroy(ctx->xev);
  if (ctx->spec_ev) (void)hipEventDestroy(ctx->spec_ev);
  if (ctx->side) {
    (void)hipStreamSynchronize(ctx->side);
    (void)hipStreamDestroy(ctx->side);
  }
  if (ctx->side_fork) (void)hipEventDestroy(ctx->side_fork);
  if (ctx->side_join) (void)hipEventDestroy(ctx->side_join);
  if (ctx->table_dev) (void)hipFree(ctx->table_dev);
  for (int k = 0; k < PCV_NUM_STAGES; ++k) {
    if (ctx->stage_b[k]) (void)hipEventDestroy(ctx->stage_b[k]);
    if (ctx->stage_e[k]) (void)hipEventDestroy(ctx->stage_e[k]);
  }
  for (auto& p : ctx->prof_pending) {
    (void)hipEventDestroy(p.a);
    (void)hipEventDestroy(p.b);
  }
  for (auto& e : ctx->prof_free) (void)hipEventDestroy(e);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

extern "C" const char* pcv_last_error(const pcv_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

extern "C" int pcv_ctx_synchronize(pcv_ctx* ctx) {
  if (!ctx) return PCV_E_INVALID;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

// Stream hand-off with the caller's runtime (torch, RCCL): order the context's stream after / before another stream
// of the same device without blocking the host. `stream` may be NULL: the legacy default stream (torch's default).
extern "C" int pcv_ctx_wait_stream(pcv_ctx* ctx, void* stream) {
  if (!ctx) return PCV_E_INVALID;
  if ((hipStream_t)stream == ctx->stream) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipEventRecord(ctx->xev, (hipStream_t)stream));
  PCV_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ctx->xev, 0));
  return PCV_OK;
}
extern "C" int pcv_ctx_signal_stream(pcv_ctx* ctx, void* stream) {
  if (!ctx) return PCV_E_INVALID;
  if ((hipStream_t)stream == ctx->stream) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipEventRecord(ctx->xev, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamWaitEvent((hipStream_t)stream, ctx->xev, 0));
  return PCV_OK;
}

extern "C" int pcv_ctx_trim(pcv_ctx* ctx) {
  if (!ctx) return PCV_E_INVALID;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  ctx->pool.trim();
  for (auto& kv : ctx->host_free) (void)hipHostFree(kv.second);
  ctx->host_free.clear();
  return PCV_OK;
}
