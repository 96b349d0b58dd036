// pcv_las.hip — LAS files onto the device. The host parses the header (pcv_las.cpp) and moves record bytes: piece
// after piece, pread by the context's host threads into the pinned ring and copied up on the side stream while the piece before
// is decoded on the context's stream. Per piece:
//   las_tile_count_kernel  (only with a filter) kept records per tile of 256, from the class and flag bytes alone
//   las_tile_scan_kernel   (only with a filter) tile offsets of the piece on top of the running base, which stays on the device
//   las_decode_kernel      the tile's bytes into LDS by aligned 16-byte loads at the alignment the tile has in the piece, one
//                          record per lane picked out of LDS through pcv_las.h's field table; the maxima, both histograms and
//                          the flag counts over ALL records, aggregated per wave and in LDS before one atomic per touched bin and
//                          workgroup; a stable compaction (ballot and rank in the wave, wave sums in the tile, the tile's
//                          offset); coalesced plane stores
// and once per load, where the colour rule waits for the file's maxima (AUTO, INTENSITY): las_color_kernel narrows the parked
// 16-bit values. The device holds PCV_LAS_RAW_PIECES raw pieces, never the file.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>

#include "pcv_internal.h"
#include "pcv_las.h"
#include "pcv_las_dev.h"

namespace {

struct LasOut {  // device columns
  double *x, *y, *z;
  uint8_t* rgb;
  float* inten;
  uint16_t* park;  // AUTO on a format with colour: r g b per kept point; INTENSITY: the intensity
  void* extra[PCV_LAS_MAX_EXTRAS];
};
enum : uint32_t { kLasColorDirect = 0, kLasColorParkRgb = 1, kLasColorParkIntensity = 2 };

__global__ __launch_bounds__(kLasTile) void las_tile_count_kernel(PcvLasPlan pl, const uint8_t* __restrict__ raw, uint32_t n,
                                                                   uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t s_wave[kLasTile / 64];
  const uint32_t i = blockIdx.x * kLasTile + threadIdx.x;
  bool keep = false;
  if (i < n) {
    uint32_t c;
    bool withheld;
    pcv_las_pick_filter(pl.f, raw + (uint64_t)i * pl.stride, &c, &withheld);
    keep = pcv_las_verdict(pl, c, withheld) == 0;
  }
  const unsigned long long b = __ballot(keep);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// one workgroup: off[t] = base + kept records of the piece's tiles before t; base (stats[kLasStatBase]) moves on by the piece
__global__ __launch_bounds__(256) void las_tile_scan_kernel(const uint32_t* __restrict__ cnt, uint32_t tiles, uint32_t* __restrict__ off,
                                                             unsigned long long* __restrict__ stats) {
  __shared__ uint32_t s_sum[256];
  const uint32_t per = (tiles + 255) / 256, b = threadIdx.x * per, e = b + per < tiles ? b + per : tiles;
  uint32_t sum = 0;
  for (uint32_t k = b; k < e; ++k) sum += cnt[k];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = (uint32_t)stats[kLasStatBase];
    for (int k = 0; k < 256; ++k) {
      const uint32_t t = s_sum[k];
      s_sum[k] = run;
      run += t;
    }
    stats[kLasStatBase] = run;
  }
  __syncthreads();
  uint32_t run = s_sum[threadIdx.x];
  for (uint32_t k = b; k < e; ++k) {
    off[k] = run;
    run += cnt[k];
  }
}

// raw: the piece's first record; n: its records; tile_off: null without a filter (the tile's records then go to out_first + their
// index in the piece)
template <bool STAGED>
__global__ __launch_bounds__(kLasTile) void las_decode_kernel(PcvLasPlan pl, LasOut o, uint32_t color_path, const uint8_t* __restrict__ raw,
                                                               uint32_t n, const uint32_t* __restrict__ tile_off, uint32_t out_first,
                                                               unsigned long long* __restrict__ stats) {
  extern __shared__ uint4 las_tile_lds[];
  __shared__ uint32_t s_stat[kLasStatBase];
  __shared__ uint32_t s_wave[kLasTile / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t k = tid; k < (uint32_t)kLasStatBase; k += kLasTile) s_stat[k] = 0;
  const uint32_t t0 = blockIdx.x * kLasTile, cnt = n - t0 < (uint32_t)kLasTile ? n - t0 : (uint32_t)kLasTile;
  const uint8_t* g0 = raw + (uint64_t)t0 * pl.stride;
  uint32_t skew = 0;
  if (STAGED) {
    skew = (uint32_t)(reinterpret_cast<uintptr_t>(g0) & 15);
    las_stage_tile(las_tile_lds, g0 - skew, skew + cnt * pl.stride, raw, raw + (uint64_t)n * pl.stride);
  }
  __syncthreads();
  const bool live = tid < cnt;
  PcvLasRecord r = {};
  uint32_t verdict = 3;
  if (live) {
    const uint8_t* p = STAGED ? reinterpret_cast<const uint8_t*>(las_tile_lds) + skew + tid * pl.stride : g0 + (uint64_t)tid * pl.stride;
    pcv_las_pick(pl.f, p, &r);
    verdict = pcv_las_verdict(pl, r.classification, (r.class_flags >> 2) & 1);
  }
  // statistics over all records of the tile, dropped ones too
  const uint32_t c3 = r.r > r.g ? (r.r > r.b ? r.r : r.b) : (r.g > r.b ? r.g : r.b);
  const uint32_t mc = las_wave_max(c3), mi = las_wave_max(r.intensity);
  las_wave_hist_add(s_stat + kLasStatClass, r.classification, live);
  las_wave_hist_add(s_stat + kLasStatReturn, r.return_number, live);
  const unsigned long long keep_b = __ballot(verdict == 0), class_b = __ballot(verdict == 1), withheld_b = __ballot(verdict == 2);
  unsigned long long flag_b[4];
  for (int b = 0; b < 4; ++b) flag_b[b] = __ballot(live && ((r.class_flags >> b) & 1));
  if (lane == 0) {
    if (mc) atomicMax(&s_stat[kLasStatMaxColor], mc);
    if (mi) atomicMax(&s_stat[kLasStatMaxIntensity], mi);
    for (int b = 0; b < 4; ++b)
      if (flag_b[b]) atomicAdd(&s_stat[kLasStatFlags + b], (uint32_t)__popcll(flag_b[b]));
    if (keep_b) atomicAdd(&s_stat[kLasStatKept], (uint32_t)__popcll(keep_b));
    if (class_b) atomicAdd(&s_stat[kLasStatDropClass], (uint32_t)__popcll(class_b));
    if (withheld_b) atomicAdd(&s_stat[kLasStatDropWithheld], (uint32_t)__popcll(withheld_b));
    s_wave[wave] = (uint32_t)__popcll(keep_b);
  }
  __syncthreads();
  if (verdict == 0) {
    uint32_t base = tile_off ? tile_off[blockIdx.x] : out_first + t0;
    for (uint32_t w = 0; w < wave; ++w) base += s_wave[w];
    const uint64_t slot = base + (uint32_t)__popcll(keep_b & ((1ull << lane) - 1));
    double x, y, z;
    pcv_las_position(pl, r, &x, &y, &z);
    o.x[slot] = x, o.y[slot] = y, o.z[slot] = z;
    if (color_path == kLasColorDirect) {
      uint8_t c[3];
      pcv_las_color(pl.color_mode, pl.constant_color, 0, r.r, r.g, r.b, r.intensity, c);
      o.rgb[3 * slot] = c[0], o.rgb[3 * slot + 1] = c[1], o.rgb[3 * slot + 2] = c[2];
    } else if (color_path == kLasColorParkRgb) {
      o.park[3 * slot] = r.r, o.park[3 * slot + 1] = r.g, o.park[3 * slot + 2] = r.b;
    } else {
      o.park[slot] = r.intensity;
    }
    if (o.inten) o.inten[slot] = (float)r.intensity;
    for (uint32_t k = 0; k < pl.num_extras; ++k) pcv_las_store_extra(pl.extra_id[k], r, o.extra[k], slot);  // kernel-uniform
  }
  // one atomic per touched counter and workgroup
  for (uint32_t k = tid; k < (uint32_t)kLasStatBase; k += kLasTile) {
    const uint32_t v = s_stat[k];
    if (v == 0) continue;
    if (k >= (uint32_t)kLasStatMaxColor) atomicMax(&stats[k], (unsigned long long)v);
    else atomicAdd(&stats[k], (unsigned long long)v);
  }
}

// the parked 16-bit values of the kept points under the rule that the file's maxima decided
__global__ __launch_bounds__(256) void las_color_kernel(uint32_t rule, uint32_t color_path, uint32_t max_intensity, uint32_t n,
                                                         const uint16_t* __restrict__ park, uint8_t* __restrict__ rgb) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint8_t none[3] = {0, 0, 0};
  uint8_t c[3];
  if (color_path == kLasColorParkRgb) pcv_las_color(rule, none, max_intensity, park[3 * (uint64_t)i], park[3 * (uint64_t)i + 1], park[3 * (uint64_t)i + 2], 0, c);
  else pcv_las_color(rule, none, max_intensity, 0, 0, 0, park[i], c);
  rgb[3 * (uint64_t)i] = c[0], rgb[3 * (uint64_t)i + 1] = c[1], rgb[3 * (uint64_t)i + 2] = c[2];
}

// ---- the engine: records from a file, from host memory or from device memory through the kernels ----------------------------
struct LasSource {
  const uint8_t* host = nullptr;
  const uint8_t* dev = nullptr;
  int fd = -1;
  uint64_t file_at = 0;  // offset to point data
};
struct LasEvents {
  hipEvent_t copied[PCV_LAS_RAW_PIECES] = {}, decoded[PCV_LAS_RAW_PIECES] = {};
  int create() {
    for (int k = 0; k < PCV_LAS_RAW_PIECES; ++k)
      if (hipEventCreateWithFlags(&copied[k], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&decoded[k], hipEventDisableTiming) != hipSuccess)
        return PCV_E_HIP;
    return PCV_OK;
  }
  ~LasEvents() {
    for (int k = 0; k < PCV_LAS_RAW_PIECES; ++k) {
      if (copied[k]) (void)hipEventDestroy(copied[k]);
      if (decoded[k]) (void)hipEventDestroy(decoded[k]);
    }
  }
};
// both streams drained on every way out: what the caller releases next is no longer in flight
struct LasDrain {
  pcv_ctx* ctx;
  ~LasDrain() {
    (void)hipStreamSynchronize(ctx->side);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->prof_resolve();
  }
};

uint32_t las_color_path(const PcvLasPlan& pl) {
  if (pl.color_mode == PCV_LAS_COLOR_INTENSITY || (pl.color_mode == PCV_LAS_COLOR_AUTO && !pl.f.rgb_at)) return kLasColorParkIntensity;
  return pl.color_mode == PCV_LAS_COLOR_AUTO ? kLasColorParkRgb : kLasColorDirect;
}
uint32_t las_piece_points(const PcvLasPlan& pl, uint32_t asked) {
  const uint32_t most = (uint32_t)(pcv_ctx::kRingChunk / pl.stride);  // >= 512: a record is below 2^16 bytes
  return asked == 0 || asked > most ? most / kLasTile * kLasTile : asked;
}

int las_alloc_columns(PcvScratch& sc, const PcvLasPlan& pl, uint64_t n, LasOut* o) {
  *o = LasOut{};
  if (n == 0) return PCV_OK;
  int rc;
  if ((rc = sc.get(&o->x, n)) || (rc = sc.get(&o->y, n)) || (rc = sc.get(&o->z, n)) || (rc = sc.get(&o->rgb, 3 * n)) ||
      (pl.keep_intensity && (rc = sc.get(&o->inten, n))))
    return rc;
  for (uint32_t k = 0; k < pl.num_extras; ++k) {
    uint8_t* col;
    if ((rc = sc.get(&col, n * pcv_las_extra_bytes(pl.extra_id[k])))) return rc;
    o->extra[k] = col;
  }
  return PCV_OK;
}

// n records -> the columns of `o` (device memory for n points each) and info; returns with both streams idle
int las_run(pcv_ctx* ctx, const PcvLasPlan& pl, const LasSource& src, uint64_t n, uint32_t asked_piece_points, LasOut o, pcv_las_info* info) {
  pcv_las_info in{};
  in.num_records = n;
  if (n == 0) {
    in.color_rule = pcv_las_resolve_rule(pl, 0);
    *info = in;
    return PCV_OK;
  }
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint32_t pp = las_piece_points(pl, asked_piece_points), stride = pl.stride;
  const uint64_t pieces = (n + pp - 1) / pp;
  const uint32_t piece_tiles = (uint32_t)((std::min<uint64_t>(pp, n) + kLasTile - 1) / kLasTile);
  const bool filter = pl.filter_classes || pl.drop_withheld, staged = stride <= kLasStagedMaxStride;
  const uint32_t color_path = las_color_path(pl);
  PcvScratch sc(ctx);
  LasEvents ev;
  unsigned long long* stats;
  uint32_t *tile_cnt = nullptr, *tile_off = nullptr;
  uint8_t* rawbuf[PCV_LAS_RAW_PIECES] = {};
  int rc;
  if ((rc = sc.get(&stats, (size_t)kLasStatWords))) return rc;
  if (filter && ((rc = sc.get(&tile_cnt, piece_tiles)) || (rc = sc.get(&tile_off, piece_tiles)))) return rc;
  if (color_path != kLasColorDirect && (rc = sc.get(&o.park, (color_path == kLasColorParkRgb ? 3 : 1) * n))) return rc;
  if (!src.dev) {
    const size_t piece_bytes = (size_t)std::min<uint64_t>(pp, n) * stride;
    for (int b = 0; b < PCV_LAS_RAW_PIECES && (uint64_t)b < pieces; ++b)
      if ((rc = sc.get(&rawbuf[b], piece_bytes))) return rc;
    if ((rc = ctx->ring_ensure())) return rc;
    if (ev.create() != PCV_OK) return ctx->fail(PCV_E_HIP, "hipEventCreate");
  }
  if ((rc = ctx->pinned_reserve(kLasStatWords * sizeof(unsigned long long)))) return rc;
  LasDrain drain{ctx};
  PCV_HIP_CHECK(ctx, hipMemsetAsync(stats, 0, kLasStatWords * sizeof(unsigned long long), ctx->stream));
  if (!src.dev && (rc = ctx->side_begin())) return ctx->fail(rc, "hipEventRecord (side stream)");
  const size_t nworkers = ctx->host_pool.threads.size() + 1;
  for (uint64_t k = 0; k < pieces; ++k) {
    const uint64_t first = k * pp;
    const uint32_t cnt = (uint32_t)std::min<uint64_t>(pp, n - first);
    const size_t bytes = (size_t)cnt * stride;
    const int b = (int)(k % PCV_LAS_RAW_PIECES);
    const uint8_t* d_piece;
    if (src.dev) {
      d_piece = src.dev + first * stride;
    } else {
      // the buffer's last reader (the decode of piece k - PCV_LAS_RAW_PIECES) must have finished before the copy overwrites it
      if (k >= PCV_LAS_RAW_PIECES) PCV_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->side, ev.decoded[b], 0));
      const int slot = ctx->ring_take();
      if (ctx->ring_busy[slot]) PCV_HIP_CHECK(ctx, hipEventSynchronize(ctx->ring_ev[slot]));
      uint8_t* chunk = (uint8_t*)ctx->ring[slot];
      const size_t part = std::max<size_t>(256u << 10, ((bytes + nworkers - 1) / nworkers + 4095) & ~(size_t)4095);
      std::atomic<int> bad{0};
      const uint64_t at = first * stride;
      ctx->host_pool.run((bytes + part - 1) / part, [&](size_t p) {
        const size_t b0 = p * part, e0 = b0 + part < bytes ? b0 + part : bytes;
        if (src.host) {
          std::memcpy(chunk + b0, src.host + at + b0, e0 - b0);
          return;
        }
        size_t got = b0;
        while (got < e0) {  // pread is thread-safe: the host threads fill different parts of the chunk
          const ssize_t rd = pread(src.fd, chunk + got, e0 - got, (off_t)(src.file_at + at + got));
          if (rd <= 0) {
            bad.store(1);
            return;
          }
          got += (size_t)rd;
        }
      });
      if (bad.load()) return ctx->fail(PCV_E_IO, "LAS: unexpected end of file in the point records");
      PCV_HIP_CHECK(ctx, hipMemcpyAsync(rawbuf[b], chunk, bytes, hipMemcpyHostToDevice, ctx->side));
      PCV_HIP_CHECK(ctx, hipEventRecord(ctx->ring_ev[slot], ctx->side));
      ctx->ring_busy[slot] = true;
      PCV_HIP_CHECK(ctx, hipEventRecord(ev.copied[b], ctx->side));
      PCV_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ev.copied[b], 0));
      d_piece = rawbuf[b];
    }
    const uint32_t tiles = (cnt + kLasTile - 1) / kLasTile;
    if (filter) {
      {
        PcvProf prof(ctx, PCV_K_LAS_COUNT);
        hipLaunchKernelGGL(las_tile_count_kernel, dim3(tiles), dim3(kLasTile), 0, ctx->stream, pl, d_piece, cnt, tile_cnt);
      }
      {
        PcvProf prof(ctx, PCV_K_LAS_SCAN);
        hipLaunchKernelGGL(las_tile_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, tile_cnt, tiles, tile_off, stats);
      }
    }
    {
      PcvProf prof(ctx, PCV_K_LAS_DECODE);
      if (staged)
        hipLaunchKernelGGL(las_decode_kernel<true>, dim3(tiles), dim3(kLasTile), (size_t)kLasTile * stride + 32, ctx->stream, pl, o, color_path, d_piece,
                           cnt, filter ? tile_off : nullptr, (uint32_t)first, stats);
      else
        hipLaunchKernelGGL(las_decode_kernel<false>, dim3(tiles), dim3(kLasTile), 0, ctx->stream, pl, o, color_path, d_piece, cnt,
                           filter ? tile_off : nullptr, (uint32_t)first, stats);
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    if (!src.dev) PCV_HIP_CHECK(ctx, hipEventRecord(ev.decoded[b], ctx->stream));
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->pinned, stats, kLasStatWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t* st = (const uint64_t*)ctx->pinned;
  for (int c = 0; c < 256; ++c) in.class_hist[c] = st[kLasStatClass + c];
  for (int c = 0; c < 16; ++c) in.return_hist[c] = st[kLasStatReturn + c];
  for (int c = 0; c < 4; ++c) in.flag_counts[c] = st[kLasStatFlags + c];
  in.num_kept = st[kLasStatKept], in.dropped_class = st[kLasStatDropClass], in.dropped_withheld = st[kLasStatDropWithheld];
  in.max_color = (uint32_t)st[kLasStatMaxColor], in.max_intensity = (uint32_t)st[kLasStatMaxIntensity];
  in.color_rule = pcv_las_resolve_rule(pl, in.max_color);
  in.num_pieces = (uint32_t)pieces;
  if (in.num_kept > n || (filter && st[kLasStatBase] != in.num_kept)) return ctx->fail(PCV_E_HIP, "LAS: the kept counts of the count pass and the decode differ");
  if (color_path != kLasColorDirect && in.num_kept > 0) {
    PcvProf prof(ctx, PCV_K_LAS_COLOR);
    hipLaunchKernelGGL(las_color_kernel, dim3((unsigned)((in.num_kept + 255) / 256)), dim3(256), 0, ctx->stream, in.color_rule, color_path, in.max_intensity,
                       (uint32_t)in.num_kept, o.park, o.rgb);
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  *info = in;
  return PCV_OK;  // LasDrain waits for the colour pass
}

int las_plan(pcv_ctx* ctx, const pcv_las_header* h, const pcv_las_params* params, PcvLasPlan* pl) {
  std::string why;
  const int rc = pcv_las_make_plan(h, params, pl, &why);
  return rc ? ctx->fail(rc, why) : PCV_OK;
}

}  // namespace

struct pcv_las_cloud {
  pcv_ctx* ctx = nullptr;
  PcvLasPlan plan{};
  pcv_las_info info{};
  LasOut o{};
};

extern "C" void pcv_las_cloud_free(pcv_las_cloud* c) {
  if (!c) return;
  void* all[5] = {c->o.x, c->o.y, c->o.z, c->o.rgb, c->o.inten};
  for (void* p : all) c->ctx->dev_free(p);
  for (void* p : c->o.extra) c->ctx->dev_free(p);
  delete c;
}

extern "C" int pcv_las_load(pcv_ctx* ctx, const char* path, const pcv_las_params* params, pcv_las_cloud** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  if (!path || !params) return ctx->fail(PCV_E_INVALID, "null argument");
  pcv_las_header h;
  std::string why;
  if (int rc = pcv_las_read_header(path, &h, &why)) return ctx->fail(rc, why);
  PcvLasPlan pl;
  if (int rc = las_plan(ctx, &h, params, &pl)) return rc;
  LasSource src;
  src.fd = open(path, O_RDONLY | O_CLOEXEC);
  if (src.fd < 0) return ctx->fail(PCV_E_IO, std::string("LAS: could not open ") + path);
  src.file_at = h.offset_to_points;
  pcv_las_cloud* c = new pcv_las_cloud;
  c->ctx = ctx, c->plan = pl;
  int rc;
  {
    PcvScratch sc(ctx);
    if ((rc = las_alloc_columns(sc, pl, h.num_points, &c->o)) == PCV_OK &&
        (rc = las_run(ctx, pl, src, h.num_points, params->piece_points, c->o, &c->info)) == PCV_OK)
      sc.ptrs.clear();  // the cloud owns the columns now
    else
      c->o = LasOut{};
  }
  close(src.fd);
  if (rc != PCV_OK) {
    delete c;
    return rc;
  }
  c->o.park = nullptr;
  *out = c;
  return PCV_OK;
}

extern "C" int pcv_las_cloud_info(const pcv_las_cloud* c, pcv_las_info* out) {
  if (!c || !out) return PCV_E_INVALID;
  *out = c->info;
  return PCV_OK;
}
extern "C" int pcv_las_cloud_points(const pcv_las_cloud* c, pcv_points* out) {
  if (!c || !out) return PCV_E_INVALID;
  *out = pcv_points{};
  out->n = c->info.num_kept;
  out->x = c->o.x, out->y = c->o.y, out->z = c->o.z;
  out->color = c->o.rgb, out->color_stride = 3;
  out->intensity = c->o.inten;
  out->mem = PCV_MEM_DEVICE;
  return PCV_OK;
}
extern "C" int pcv_las_cloud_attributes(const pcv_las_cloud* c, uint32_t* count, pcv_attribute* out) {
  if (!c || !count) return PCV_E_INVALID;
  *count = c->plan.num_extras;
  for (uint32_t k = 0; out && k < c->plan.num_extras; ++k)
    out[k] = pcv_attribute{pcv_las_extra_name(c->plan.extra_id[k]), pcv_las_extra_type(c->plan.extra_id[k]), 0, c->o.extra[k]};
  return PCV_OK;
}
extern "C" int pcv_las_cloud_read(const pcv_las_cloud* c, const char* name, void* out, uint64_t capacity_bytes) {
  if (!c) return PCV_E_INVALID;
  pcv_ctx* ctx = c->ctx;
  if (!name || (!out && capacity_bytes)) return ctx->fail(PCV_E_INVALID, "null argument");
  const uint64_t n = c->info.num_kept;
  const void* from = nullptr;
  uint64_t bytes = 0;
  const std::string s(name);
  if (s == "x") from = c->o.x, bytes = 8 * n;
  else if (s == "y") from = c->o.y, bytes = 8 * n;
  else if (s == "z") from = c->o.z, bytes = 8 * n;
  else if (s == "color") from = c->o.rgb, bytes = 3 * n;
  else if (s == "intensity" && c->plan.keep_intensity) from = c->o.inten, bytes = 4 * n;
  else {
    uint32_t k = 0;
    while (k < c->plan.num_extras && s != pcv_las_extra_name(c->plan.extra_id[k])) ++k;
    if (k == c->plan.num_extras) return ctx->fail(PCV_E_INVALID, "LAS: the cloud has no column '" + s + "'");
    from = c->o.extra[k], bytes = n * pcv_las_extra_bytes(c->plan.extra_id[k]);
  }
  if (capacity_bytes < bytes) return ctx->fail(PCV_E_INVALID, "LAS: column '" + s + "' takes " + std::to_string(bytes) + " bytes");
  if (bytes == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, from, bytes, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_las_decode(pcv_ctx* ctx, const pcv_las_header* header, const pcv_las_params* params, const void* raw, uint64_t n, int mem,
                              pcv_las_columns* out, pcv_las_info* info) {
  if (!ctx) return PCV_E_INVALID;
  if (!header || !params || !out || !info || (!raw && n)) return ctx->fail(PCV_E_INVALID, "null argument");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "mem is neither PCV_MEM_HOST nor PCV_MEM_DEVICE");
  if (n >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "LAS: 2^32 - 1 or more records");
  PcvLasPlan pl;
  if (int rc = las_plan(ctx, header, params, &pl)) return rc;
  if (n && (!out->x || !out->y || !out->z || !out->color || (pl.keep_intensity && !out->intensity))) return ctx->fail(PCV_E_INVALID, "null output column");
  for (uint32_t k = 0; n && k < pl.num_extras; ++k)
    if (!out->extras[k]) return ctx->fail(PCV_E_INVALID, "null output column");
  LasSource src;
  (mem == PCV_MEM_DEVICE ? src.dev : src.host) = (const uint8_t*)raw;
  PcvScratch sc(ctx);
  LasOut o{};
  int rc;
  if (mem == PCV_MEM_DEVICE) {
    o.x = out->x, o.y = out->y, o.z = out->z, o.rgb = out->color, o.inten = pl.keep_intensity ? out->intensity : nullptr;
    for (uint32_t k = 0; k < pl.num_extras; ++k) o.extra[k] = out->extras[k];
  } else if ((rc = las_alloc_columns(sc, pl, n, &o))) {
    return rc;
  }
  if ((rc = las_run(ctx, pl, src, n, params->piece_points, o, info))) return rc;
  if (mem == PCV_MEM_HOST && info->num_kept) {
    const uint64_t m = info->num_kept;
    PCV_HIP_CHECK(ctx, hipMemcpy(out->x, o.x, 8 * m, hipMemcpyDeviceToHost));
    PCV_HIP_CHECK(ctx, hipMemcpy(out->y, o.y, 8 * m, hipMemcpyDeviceToHost));
    PCV_HIP_CHECK(ctx, hipMemcpy(out->z, o.z, 8 * m, hipMemcpyDeviceToHost));
    PCV_HIP_CHECK(ctx, hipMemcpy(out->color, o.rgb, 3 * m, hipMemcpyDeviceToHost));
    if (pl.keep_intensity) PCV_HIP_CHECK(ctx, hipMemcpy(out->intensity, o.inten, 4 * m, hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < pl.num_extras; ++k)
      PCV_HIP_CHECK(ctx, hipMemcpy(out->extras[k], o.extra[k], m * pcv_las_extra_bytes(pl.extra_id[k]), hipMemcpyDeviceToHost));
  }
  return PCV_OK;
}

extern "C" int pcv_build_octree_from_las(pcv_ctx* ctx, const pcv_build_params* params, const char* path, const pcv_las_params* las_params,
                                         pcv_octree** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  if (!params || !path || !las_params) return ctx->fail(PCV_E_INVALID, "null argument");
  pcv_las_cloud* c = nullptr;
  if (int rc = pcv_las_load(ctx, path, las_params, &c)) return rc;
  pcv_points pts;
  pcv_las_cloud_points(c, &pts);
  pcv_build_params p = *params;
  p.flags |= PCV_BUILD_COMPUTE_BBOX;
  const int rc = pcv_build_octree(ctx, &p, &pts, out);  // synchronous: the cloud outlives every kernel that reads it
  pcv_las_cloud_free(c);
  return rc;
}

// ---- the host entries of pcv_las.cpp behind the C ABI (messages: pcv_host_last_error) ------------------------------------------
extern "C" int pcv_las_header_host(const char* path, pcv_las_header* out) {
  std::string why;
  const int rc = pcv_las_read_header(path, out, &why);
  return rc ? pcv_host_fail(rc, why) : PCV_OK;
}
extern "C" int pcv_las_check_params_host(const pcv_las_header* header, const pcv_las_params* params) {
  std::string why;
  PcvLasPlan pl;
  const int rc = pcv_las_make_plan(header, params, &pl, &why);
  return rc ? pcv_host_fail(rc, why) : PCV_OK;
}
extern "C" int pcv_las_extras_host(uint32_t point_format, const char** names, int32_t* types, uint32_t* count) {
  if (point_format > 10 || !count) return pcv_host_fail(PCV_E_INVALID, "LAS: point data record format above 10, or count is null");
  const PcvLasFormat f = pcv_las_format(point_format);
  uint32_t m = 0;
  for (uint32_t id = 0; id < kLasNumExtras; ++id) {
    if (!pcv_las_format_has(f, id)) continue;
    if (names) names[m] = pcv_las_extra_name(id);
    if (types) types[m] = pcv_las_extra_type(id);
    ++m;
  }
  *count = m;
  return PCV_OK;
}
extern "C" int pcv_las_decode_host(const pcv_las_header* header, const pcv_las_params* params, const void* raw, uint64_t n, pcv_las_columns* out,
                                   pcv_las_info* info) {
  std::string why;
  PcvLasPlan pl;
  if (int rc = pcv_las_make_plan(header, params, &pl, &why)) return pcv_host_fail(rc, why);
  if ((!raw && n) || !out || !info) return pcv_host_fail(PCV_E_INVALID, "LAS: null argument");
  pcv_las_decode_records(pl, (const uint8_t*)raw, n, out, info);
  info->num_pieces = 1;
  return PCV_OK;
}
extern "C" int pcv_las_read(const char* path, const pcv_las_params* params, pcv_las** out) {
  std::string why;
  const int rc = pcv_las_read_file(path, params, out, &why);
  return rc ? pcv_host_fail(rc, why) : PCV_OK;
}
extern "C" uint64_t pcv_las_num_points(const pcv_las* las) { return las ? las->n : 0; }
extern "C" int pcv_las_points(const pcv_las* las, pcv_points* out) {
  if (!las || !out) return PCV_E_INVALID;
  *out = pcv_points{};
  out->n = las->n;
  out->x = las->x.data(), out->y = las->y.data(), out->z = las->z.data();
  out->color = las->color.data(), out->color_stride = 3;
  out->intensity = las->plan.keep_intensity ? las->intensity.data() : nullptr;
  out->mem = PCV_MEM_HOST;
  return PCV_OK;
}
extern "C" int pcv_las_attributes(const pcv_las* las, uint32_t* count, pcv_attribute* out) {
  if (!las || !count) return PCV_E_INVALID;
  *count = las->plan.num_extras;
  for (uint32_t k = 0; out && k < las->plan.num_extras; ++k)
    out[k] = pcv_attribute{pcv_las_extra_name(las->plan.extra_id[k]), pcv_las_extra_type(las->plan.extra_id[k]), 0, las->extras[k].data()};
  return PCV_OK;
}
extern "C" int pcv_las_info_get(const pcv_las* las, pcv_las_info* out) {
  if (!las || !out) return PCV_E_INVALID;
  *out = las->info;
  return PCV_OK;
}
extern "C" void pcv_las_free(pcv_las* las) { delete las; }
