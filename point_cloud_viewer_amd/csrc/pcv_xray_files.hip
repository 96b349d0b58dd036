// pcv_xray_files.hip — node images and node files of any kind of xray quadtree: built on the device (pcv_xray.hip,
// pcv_xray_pyramid.hip), opened from a directory (pcv_xray_open_dir) or merged from such parts.
//
//   images   pcv_xray_node_images: device to host or device copies, opened nodes decoded from their files (pcv_png.cpp)
//   files    xray_node_files: every node's PNG to a sink. Opened nodes are passed on as their files are. Device tiles come
//            down in chunks of pcv_ctx_set_xray_chunk_bytes through two pinned buffers, as images (stored mode, encoded by
//            pcv_png.cpp on the host) or as zlib streams compressed where they live (deflate mode, pcv_xray_png.hip);
//            while chunk k + 1 is on its way a pool of host threads wraps and hands out chunk k
//   sinks    a caller's buffer (pcv_xray_node_pngs) or a directory (pcv_xray_write_dir_ex), which also gets the meta file
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pcv_xray_obj.h"
#include "pcv_xray_png.h"

namespace {

bool write_at(int dirfd, const std::string& name, const uint8_t* data, uint64_t len) {
  const int fd = openat(dirfd, name.c_str(), O_CREAT | O_WRONLY | O_TRUNC | O_CLOEXEC, 0666);
  if (fd < 0) return false;
  bool ok = true;
  while (len) {
    const ssize_t w = ::write(fd, data, (size_t)len);
    if (w <= 0) {
      ok = false;
      break;
    }
    data += w;
    len -= (uint64_t)w;
  }
  return ::close(fd) == 0 && ok;
}

bool read_file(const std::string& path, std::vector<uint8_t>& data) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  data.clear();
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) data.insert(data.end(), buf, buf + k);
  const bool ok = !std::ferror(f);
  std::fclose(f);
  return ok;
}

std::string node_file_name(const pcv_xray* x, uint64_t node) {
  const XrayNodeId id = xray_node_id(x, node);
  return quad_name(id.level, id.index) + ".png";
}

}  // namespace

// ---- node images --------------------------------------------------------------------------------------------------------
int queue_node_images(pcv_xray* x, uint64_t first, uint64_t count, uint8_t* dst, hipMemcpyKind kind) {
  pcv_ctx* ctx = x->ctx;
  const uint64_t nc = x->created.size(), tile_bytes = 4ull * x->W * x->W;
  const uint64_t nl = first < nc ? std::min(count, nc - first) : 0;
  if (nl)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst, reinterpret_cast<const uint8_t*>(x->d_images) + first * tile_bytes, nl * tile_bytes, kind, ctx->stream));
  if (count > nl)
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst + nl * tile_bytes, reinterpret_cast<const uint8_t*>(x->d_parents) + (first + nl - nc) * tile_bytes,
                                      (count - nl) * tile_bytes, kind, ctx->stream));
  return PCV_OK;
}

int opened_node_to_host(const pcv_xray* x, uint64_t node, uint8_t* dst) {
  const std::string path = x->dir + "/" + node_file_name(x, node);
  std::vector<uint8_t> file;
  if (!read_file(path, file)) return xray_fail(x, PCV_E_IO, "xray: cannot read " + path);
  uint32_t w = 0, h = 0;
  int rc = pcv_png_decode(file.data(), file.size(), &w, &h, nullptr, 0);
  if (rc) return xray_fail(x, rc == PCV_E_INVALID ? PCV_E_IO : rc, path + ": " + pcv_host_last_error());
  if (w != x->W || h != x->W)
    return xray_fail(x, PCV_E_INVALID, path + " is " + std::to_string(w) + " x " + std::to_string(h) + ", the meta's tile_size is " + std::to_string(x->W));
  rc = pcv_png_decode(file.data(), file.size(), &w, &h, dst, 4ull * x->W * x->W);
  if (rc) return xray_fail(x, PCV_E_IO, path + ": " + pcv_host_last_error());
  return PCV_OK;
}

int xray_node_images(pcv_xray* x, uint64_t first, uint64_t count, int mem, uint8_t* rgba) {
  pcv_ctx* ctx = x->ctx;
  const uint64_t tile_bytes = 4ull * x->W * x->W;
  if (mem == PCV_MEM_DEVICE && !ctx) return xray_fail(x, PCV_E_INVALID, "xray: a quadtree opened without a context has host images only");
  if (ctx) PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  if (xray_owns_tiles(x)) {
    const int rc = queue_node_images(x, first, count, rgba, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    if (rc) return rc;
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return PCV_OK;
  }
  if (x->kind == kXrayOpened) {
    if (mem == PCV_MEM_HOST) {
      for (uint64_t i = 0; i < count; ++i)
        if (int rc = opened_node_to_host(x, first + i, rgba + i * tile_bytes)) return rc;
      return PCV_OK;
    }
    uint8_t* host = nullptr;  // decoded into pinned memory, one upload
    int rc = ctx->host_alloc((void**)&host, count * tile_bytes);
    if (rc) return rc;
    for (uint64_t i = 0; !rc && i < count; ++i) rc = opened_node_to_host(x, first + i, host + i * tile_bytes);
    if (!rc) {
      hipError_t e = hipMemcpyAsync(rgba, host, count * tile_bytes, hipMemcpyHostToDevice, ctx->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (e != hipSuccess) rc = ctx->fail(PCV_E_HIP, std::string("xray: image upload: ") + hipGetErrorString(e));
    }
    ctx->host_release(host);
    return rc;
  }
  // merged: runs of nodes that belong to one part go to that part; the new levels are this object's own
  for (const XrayPartRef& r : x->parts)
    if (!xray_part_alive(r)) return ctx->fail(PCV_E_INVALID, "xray: a part of this merged quadtree was freed before it");
  const uint64_t own_first = x->node_index.size() - x->parent_index.size();
  uint64_t at = first;
  const uint64_t end = first + count;
  for (const XrayPartRef& r : x->parts) {
    if (at >= end) break;
    if (at >= r.first + r.count || r.count == 0) continue;
    const uint64_t k = std::min(end, r.first + r.count) - at;
    const int rc = xray_node_images(r.part, at - r.first, k, mem, rgba + (at - first) * tile_bytes);
    if (rc) return r.part->ctx ? rc : ctx->fail(rc, pcv_host_last_error());
    at += k;
  }
  if (at < end) {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(rgba + (at - first) * tile_bytes, reinterpret_cast<const uint8_t*>(x->d_parents) + (at - own_first) * tile_bytes,
                                      (end - at) * tile_bytes, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                      ctx->stream));
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return PCV_OK;
}

extern "C" int pcv_xray_node_images(pcv_xray* x, uint64_t first, uint64_t count, uint64_t capacity, int mem, uint8_t* rgba) {
  if (!x) return PCV_E_INVALID;
  const uint64_t n = xray_num_nodes(x);
  if (first > n || count > n - first) return xray_fail(x, PCV_E_INVALID, "xray: node range past the end");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return xray_fail(x, PCV_E_INVALID, "bad mem");
  const uint64_t tile_bytes = 4ull * x->W * x->W;
  if (count * tile_bytes > capacity) return xray_fail(x, PCV_E_INVALID, "xray: capacity below count x W x W x 4 bytes");
  if (count == 0) return PCV_OK;
  if (!rgba) return xray_fail(x, PCV_E_INVALID, "null output");
  return xray_node_images(x, first, count, mem, rgba);
}

// ---- opening a directory: one handle per meta*.pb -----------------------------------------------------------------------
extern "C" int pcv_xray_open_dir(pcv_ctx* ctx, const char* directory, uint32_t capacity, pcv_xray** parts, uint32_t* num_parts) {
  auto fail = [&](int code, const std::string& m) { return ctx ? ctx->fail(code, m) : pcv_host_fail(code, m); };
  if (!directory || !num_parts) return fail(PCV_E_INVALID, "null argument");
  const std::string dir(directory);
  DIR* d = opendir(dir.c_str());
  if (!d) return fail(PCV_E_IO, "cannot open directory " + dir);
  std::vector<std::string> names;  // "meta*.pb" (META_PREFIX, META_EXTENSION)
  while (struct dirent* e = readdir(d)) {
    const std::string name(e->d_name);
    if (name.size() >= 7 && name.compare(0, 4, "meta") == 0 && name.compare(name.size() - 3, 3, ".pb") == 0) names.push_back(name);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  *num_parts = (uint32_t)names.size();
  if (capacity < names.size() || names.empty()) return PCV_OK;
  if (!parts) return fail(PCV_E_INVALID, "null argument");
  std::vector<pcv_xray*> made;
  auto undo = [&](int code, const std::string& m) {
    for (pcv_xray* x : made) pcv_xray_free(x);
    return fail(code, m);
  };
  for (const std::string& name : names) {
    const std::string path = dir + "/" + name;
    std::vector<uint8_t> data;
    if (!read_file(path, data)) return undo(PCV_E_IO, "cannot read " + path);
    XrayMeta m;
    if (!parse_meta(data, &m)) return undo(PCV_E_INVALID, "Could not parse " + path);
    const std::string why = xray_meta_check(m);
    if (!why.empty()) return undo(PCV_E_INVALID, path + why);
    pcv_xray* x = new pcv_xray();
    made.push_back(x);
    x->ctx = ctx;
    x->kind = kXrayOpened;
    x->W = m.tile_size;
    x->dir = dir;
    x->geo.deepest_level = m.deepest_level;
    // Meta::from_proto: Rect.min where present, else the deprecated f32 fields widened (version 2 files)
    x->geo.rect[0] = m.has_min ? m.min[0] : (double)m.dmin[0];
    x->geo.rect[1] = m.has_min ? m.min[1] : (double)m.dmin[1];
    x->geo.rect[2] = m.has_min ? m.edge : (double)m.dedge;
    // the node set in a stated order: descending level, then ascending index (duplicates of a file fold, as in a set)
    std::sort(m.nodes.begin(), m.nodes.end(), [](const std::pair<uint32_t, uint64_t>& a, const std::pair<uint32_t, uint64_t>& b) {
      return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    m.nodes.erase(std::unique(m.nodes.begin(), m.nodes.end()), m.nodes.end());
    for (const auto& nd : m.nodes) {
      x->node_level.push_back(nd.first);
      x->node_index.push_back(nd.second);
      if (nd.first == m.deepest_level) {
        x->created.push_back(x->geo.index.size());
        x->geo.index.push_back(nd.second);
      }
    }
  }
  for (size_t i = 0; i < made.size(); ++i) parts[i] = made[i];
  return PCV_OK;
}

// ---- device tiles to files: one chunked download per mode, one pool of host threads ------------------------------------
namespace {

// fn(i, buf) for every i < n, on up to 8 host threads when `parallel` (one directory: more writers queue on its lock,
// pcv_io.cpp); buf is the calling thread's own, kept between items. fn makes no HIP call.
template <typename Fn>
void xray_parallel_for(uint64_t n, bool parallel, Fn&& fn) {
  unsigned nt = 1;
  if (parallel) {
    nt = std::thread::hardware_concurrency();
    if (nt == 0) nt = 4;
    if (nt > 8) nt = 8;
  }
  nt = (unsigned)std::min<uint64_t>(nt, n);
  std::atomic<uint64_t> next{0};
  auto worker = [&]() {
    std::vector<uint8_t> buf;
    for (uint64_t i; (i = next.fetch_add(1)) < n;) fn(i, buf);
  };
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < nt; ++t) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
}

// the device tiles of nodes [f, f + c): a built quadtree's leaves then parents, a merged quadtree's own levels. Tile i is
// a + i * 4 W W for i < na and b + (i - na) * 4 W W after that
void xray_device_tiles(const pcv_xray* x, uint64_t f, uint64_t c, const uint8_t** a, uint64_t* na, const uint8_t** b) {
  const uint64_t tile_bytes = 4ull * x->W * x->W;
  if (x->kind == kXrayMerged) {
    *na = 0;
    *b = reinterpret_cast<const uint8_t*>(x->d_parents) + (f - (x->node_index.size() - x->parent_index.size())) * tile_bytes;
    return;
  }
  const uint64_t nc = x->created.size();
  *na = f < nc ? std::min(c, nc - f) : 0;
  *a = reinterpret_cast<const uint8_t*>(x->d_images) + f * tile_bytes;
  *b = reinterpret_cast<const uint8_t*>(x->d_parents) + (f + *na - nc) * tile_bytes;
}

// The images of `count` device tiles, per_chunk at a time through two pinned buffers: src(f, c, &a, &na, &b) names tiles
// [f, f + c); use(f, c, images) runs on the host while the next chunk is copied.
template <typename Src, typename Use>
int xray_stored_chunks(pcv_ctx* ctx, uint32_t W, uint64_t count, uint64_t per_chunk, Src&& src, Use&& use) {
  if (count == 0) return PCV_OK;
  const uint64_t tile_bytes = 4ull * W * W;
  per_chunk = std::max<uint64_t>(1, std::min(per_chunk, count));
  const uint64_t chunks = (count + per_chunk - 1) / per_chunk;
  uint8_t* host[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  int rc = PCV_OK;
  if (hipSetDevice(ctx->device) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "hipSetDevice");
  for (int k = 0; !rc && k < 2 && (uint64_t)k < chunks; ++k) {
    rc = ctx->host_alloc((void**)&host[k], per_chunk * tile_bytes);
    if (!rc && hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "hipEventCreate");
  }
  auto copy = [&](uint8_t* dst, const uint8_t* from, uint64_t tiles) -> int {
    if (tiles) PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst, from, tiles * tile_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return PCV_OK;
  };
  auto queue = [&](uint64_t k) -> int {
    const uint64_t f = k * per_chunk, c = std::min(per_chunk, count - f);
    const uint8_t *a = nullptr, *b = nullptr;
    uint64_t na = 0;
    src(f, c, &a, &na, &b);
    int r = copy(host[k & 1], a, na);
    if (!r) r = copy(host[k & 1] + na * tile_bytes, b, c - na);
    if (!r && hipEventRecord(ev[k & 1], ctx->stream) != hipSuccess) r = ctx->fail(PCV_E_HIP, "hipEventRecord");
    return r;
  };
  if (!rc) rc = queue(0);
  for (uint64_t k = 0; !rc && k < chunks; ++k) {
    if (k + 1 < chunks && (rc = queue(k + 1))) break;  // its buffer's users (chunk k - 1) have finished
    if (hipEventSynchronize(ev[k & 1]) != hipSuccess) {
      rc = ctx->fail(PCV_E_HIP, "xray: image download failed");
      break;
    }
    rc = use(k * per_chunk, std::min(per_chunk, count - k * per_chunk), host[k & 1]);
  }
  (void)hipStreamSynchronize(ctx->stream);
  for (int k = 0; k < 2; ++k) {
    if (ev[k]) (void)hipEventDestroy(ev[k]);
    if (host[k]) ctx->host_release(host[k]);
  }
  return rc;
}

// One chunk in flight on the device and one on the host: the scratch of pcv_xray_png_launch and two pinned buffers, each
// for the compacted streams of a chunk and their offsets. Only offsets and compressed bytes are copied down.
struct XrayPngPipe {
  pcv_ctx* ctx = nullptr;
  PcvPngWork wk;
  uint8_t* host[2] = {nullptr, nullptr};
  uint64_t* tab[2] = {nullptr, nullptr};
  hipEvent_t ev_tab[2] = {nullptr, nullptr}, ev_bytes[2] = {nullptr, nullptr};
  int open(pcv_ctx* c, uint32_t W, uint64_t tiles, int buffers) {
    ctx = c;
    int rc = pcv_xray_png_work_alloc(ctx, W, tiles, &wk);
    for (int k = 0; !rc && k < buffers; ++k) {
      if ((rc = ctx->host_alloc((void**)&host[k], tiles * wk.tile_bound)) || (rc = ctx->host_alloc((void**)&tab[k], 8 * (tiles + 1)))) break;
      if (hipEventCreateWithFlags(&ev_tab[k], hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&ev_bytes[k], hipEventDisableTiming) != hipSuccess)
        rc = ctx->fail(PCV_E_HIP, "hipEventCreate");
    }
    return rc;
  }
  // kernels of a chunk, then its offsets on their way down
  int launch(int s, const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t count) {
    if (int rc = pcv_xray_png_launch(ctx, wk, a, na, b, count)) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(tab[s], wk.offsets, 8 * (count + 1), hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipEventRecord(ev_tab[s], ctx->stream));
    return PCV_OK;
  }
  // once the offsets are here: exactly the compressed bytes on their way down
  int fetch(int s, uint64_t count) {
    PCV_HIP_CHECK(ctx, hipEventSynchronize(ev_tab[s]));
    const uint64_t total = tab[s][count];
    if (total > count * wk.tile_bound) return ctx->fail(PCV_E_HIP, "xray: compressed chunk larger than its bound");
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(host[s], wk.out, total, hipMemcpyDeviceToHost, ctx->stream));
    PCV_HIP_CHECK(ctx, hipEventRecord(ev_bytes[s], ctx->stream));
    return PCV_OK;
  }
  int wait(int s) {
    PCV_HIP_CHECK(ctx, hipEventSynchronize(ev_bytes[s]));
    return PCV_OK;
  }
  void close() {
    if (!ctx) return;
    (void)hipStreamSynchronize(ctx->stream);
    for (int k = 0; k < 2; ++k) {
      if (ev_tab[k]) (void)hipEventDestroy(ev_tab[k]);
      if (ev_bytes[k]) (void)hipEventDestroy(ev_bytes[k]);
      if (host[k]) ctx->host_release(host[k]);
      if (tab[k]) ctx->host_release(tab[k]);
    }
    pcv_xray_png_work_free(ctx, &wk);
  }
};

// The zlib streams of `count` device tiles, per_chunk at a time: src as above; use(f, c, streams, offsets) runs on the
// host while the next chunk is compressed and copied.
template <typename Src, typename Use>
int xray_deflate_chunks(pcv_ctx* ctx, uint32_t W, uint64_t count, uint64_t per_chunk, Src&& src, Use&& use) {
  if (count == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  per_chunk = std::max<uint64_t>(1, std::min(per_chunk, count));
  const uint64_t chunks = (count + per_chunk - 1) / per_chunk;
  XrayPngPipe pipe;
  int rc = pipe.open(ctx, W, per_chunk, chunks > 1 ? 2 : 1);
  auto start = [&](uint64_t k) -> int {
    const uint64_t f = k * per_chunk, c = std::min(per_chunk, count - f);
    const uint8_t *a = nullptr, *b = nullptr;
    uint64_t na = 0;
    src(f, c, &a, &na, &b);
    if (int r = pipe.launch((int)(k & 1), a, na, b, c)) return r;
    return pipe.fetch((int)(k & 1), c);
  };
  if (!rc) rc = start(0);
  for (uint64_t k = 0; !rc && k < chunks; ++k) {
    if (k + 1 < chunks && (rc = start(k + 1))) break;  // its buffer's users (chunk k - 1) have finished
    if ((rc = pipe.wait((int)(k & 1)))) break;
    const uint64_t f = k * per_chunk, c = std::min(per_chunk, count - f);
    rc = use(f, c, pipe.host[k & 1], pipe.tab[k & 1]);
  }
  pipe.close();
  return rc;
}

}  // namespace

int xray_tile_files(pcv_ctx* ctx, uint32_t W, uint64_t count, int mode, bool parallel, const XrayTileSrc& src, const XrayFileSink& sink) {
  const uint64_t tile_bytes = 4ull * W * W;
  const uint64_t per_chunk = ctx->xray_chunk_bytes / tile_bytes;
  std::atomic<int> failed{0};
  if (mode == PCV_XRAY_PNG_DEFLATE)
    return xray_deflate_chunks(ctx, W, count, per_chunk, src, [&](uint64_t f, uint64_t c, const uint8_t* streams, const uint64_t* offs) {
      xray_parallel_for(c, parallel, [&](uint64_t i, std::vector<uint8_t>& png) {
        if (failed.load()) return;
        png.resize(kPcvPngWrap + offs[i + 1] - offs[i]);
        pcv_png_wrap(W, W, streams + offs[i], offs[i + 1] - offs[i], png.data());
        if (!sink(f + i, png.data(), png.size())) failed.store(1);
      });
      return failed.load() ? PCV_E_IO : PCV_OK;
    });
  return xray_stored_chunks(ctx, W, count, per_chunk, src, [&](uint64_t f, uint64_t c, const uint8_t* images) {
    xray_parallel_for(c, parallel, [&](uint64_t i, std::vector<uint8_t>& png) {
      if (failed.load()) return;
      png.resize(pcv_png_stored_size(W, W));
      pcv_png_stored_encode(images + i * tile_bytes, W, W, png.data());
      if (!sink(f + i, png.data(), png.size())) failed.store(1);
    });
    return failed.load() ? PCV_E_IO : PCV_OK;
  });
}

namespace {

// nodes [first, first + count) whose images are on x's device, encoded in `mode`, each file to the sink
int xray_device_node_files(pcv_xray* x, uint64_t first, uint64_t count, int mode, bool parallel, const XrayFileSink& sink) {
  return xray_tile_files(
      x->ctx, x->W, count, mode, parallel,
      [&](uint64_t f, uint64_t c, const uint8_t** a, uint64_t* na, const uint8_t** b) { xray_device_tiles(x, first + f, c, a, na, b); },
      [&](uint64_t i, const uint8_t* file, uint64_t len) { return sink(first + i, file, len); });
}

// the files of nodes [first, first + count) of any kind of quadtree: opened nodes as their files are, the others encoded
int xray_node_files(pcv_xray* x, uint64_t first, uint64_t count, int mode, bool parallel, const XrayFileSink& sink) {
  if (count == 0) return PCV_OK;
  if (xray_owns_tiles(x)) return xray_device_node_files(x, first, count, mode, parallel, sink);
  if (x->kind == kXrayOpened) {
    std::vector<uint8_t> file;
    for (uint64_t i = first; i < first + count; ++i) {
      const std::string path = x->dir + "/" + node_file_name(x, i);
      if (!read_file(path, file)) return xray_fail(x, PCV_E_IO, "xray: cannot read " + path);
      if (!sink(i, file.data(), file.size())) return PCV_E_IO;
    }
    return PCV_OK;
  }
  pcv_ctx* ctx = x->ctx;
  for (const XrayPartRef& r : x->parts)
    if (!xray_part_alive(r)) return ctx->fail(PCV_E_INVALID, "xray: a part of this merged quadtree was freed before it");
  uint64_t at = first;
  const uint64_t end = first + count;
  for (const XrayPartRef& r : x->parts) {
    if (at >= end) break;
    if (at >= r.first + r.count || r.count == 0) continue;
    const uint64_t k = std::min(end, r.first + r.count) - at;
    const uint64_t shift = r.first;
    const int rc = xray_node_files(r.part, at - r.first, k, mode, parallel,
                                   [&](uint64_t node, const uint8_t* file, uint64_t len) { return sink(node + shift, file, len); });
    if (rc) return r.part->ctx == ctx || rc == PCV_E_IO ? rc : ctx->fail(rc, r.part->ctx ? r.part->ctx->last_error : pcv_host_last_error());
    at += k;
  }
  return at < end ? xray_device_node_files(x, at, end - at, mode, parallel, sink) : PCV_OK;
}

// files appended to a caller's buffer with their offsets; out == nullptr: the offsets alone
struct XrayPngAppend {
  uint8_t* out;
  uint64_t capacity, at = 0, index = 0;
  uint64_t* offsets;
  bool fits = true;
  bool take(const uint8_t* file, uint64_t len) {
    offsets[index++] = at;
    if (out && len <= capacity - std::min(capacity, at)) std::memcpy(out + at, file, len);
    else if (out) fits = false;
    at += len;
    offsets[index] = at;
    return true;
  }
};

// A directory that takes files from several threads: the first "cannot write" is kept and handed to the context once
struct XrayDirSink {
  pcv_ctx* ctx = nullptr;
  std::string dir;
  int dirfd = -1;
  std::mutex mu;
  std::string first_error;
  ~XrayDirSink() {
    if (dirfd >= 0) ::close(dirfd);
  }
  int open(pcv_ctx* c, const char* directory) {
    ctx = c;
    dir = directory;
    ::mkdir(dir.c_str(), 0777);  // build_xray_quadtree :565 ignores errors: the directory may be there
    struct stat st;
    if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return ctx->fail(PCV_E_IO, "cannot create directory " + dir);
    dirfd = ::open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
    return dirfd < 0 ? ctx->fail(PCV_E_IO, "cannot open directory " + dir) : PCV_OK;
  }
  bool write(const std::string& name, const uint8_t* data, uint64_t len) {
    if (write_at(dirfd, name, data, len)) return true;
    std::lock_guard<std::mutex> g(mu);
    if (first_error.empty()) first_error = "cannot write " + dir + "/" + name;
    return false;
  }
  // the code of a step that wrote here: a write that failed becomes the context's message
  int status(int rc) {
    if (rc != PCV_E_IO || first_error.empty()) return rc;
    std::string m;
    m.swap(first_error);
    return ctx->fail(rc, m);
  }
};

bool same_directory(const std::string& a, const std::string& b) {  // copy_images :29: canonicalize() of both
  char* ra = realpath(a.c_str(), nullptr);
  char* rb = realpath(b.c_str(), nullptr);
  const bool same = ra && rb && std::strcmp(ra, rb) == 0;
  std::free(ra);
  std::free(rb);
  return same;
}

}  // namespace

extern "C" int pcv_xray_node_pngs(pcv_xray* x, uint64_t first, uint64_t count, int mode, uint64_t capacity, uint8_t* out, uint64_t* offsets) {
  if (!x) return PCV_E_INVALID;
  const uint64_t n = xray_num_nodes(x);
  if (first > n || count > n - first) return xray_fail(x, PCV_E_INVALID, "xray: node range past the end");
  if (mode != PCV_XRAY_PNG_STORED && mode != PCV_XRAY_PNG_DEFLATE) return xray_fail(x, PCV_E_INVALID, "xray: unknown PNG mode");
  if (!offsets) return xray_fail(x, PCV_E_INVALID, "null offsets");
  if (mode == PCV_XRAY_PNG_DEFLATE && x->kind != kXrayOpened && x->W > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return xray_fail(x, PCV_E_INVALID, "xray: compressed tiles are at most " + std::to_string(PCV_XRAY_PNG_DEFLATE_MAX_EDGE) + " pixels wide");
  offsets[0] = 0;
  XrayPngAppend app{out, capacity};
  app.offsets = offsets;
  const int rc = xray_node_files(x, first, count, mode, false, [&](uint64_t, const uint8_t* file, uint64_t len) { return app.take(file, len); });
  if (rc) return rc;
  if (!app.fits) return xray_fail(x, PCV_E_INVALID, "xray: capacity below the " + std::to_string(app.at) + " bytes of these files");
  return PCV_OK;
}

extern "C" int pcv_xray_write_dir(pcv_xray* x, const char* directory) { return pcv_xray_write_dir_ex(x, directory, PCV_XRAY_PNG_STORED); }

extern "C" int pcv_xray_write_dir_ex(pcv_xray* x, const char* directory, int mode) {
  if (!x) return PCV_E_INVALID;
  if (!directory) return xray_fail(x, PCV_E_INVALID, "null directory");
  if (mode != PCV_XRAY_PNG_STORED && mode != PCV_XRAY_PNG_DEFLATE) return xray_fail(x, PCV_E_INVALID, "xray: unknown PNG mode");
  if (x->kind == kXrayOpened)
    return xray_fail(x, PCV_E_INVALID, "xray: an opened quadtree is written through pcv_xray_merge (its files are already a directory)");
  if (mode == PCV_XRAY_PNG_DEFLATE && x->W > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return xray_fail(x, PCV_E_INVALID, "xray: compressed tiles are at most " + std::to_string(PCV_XRAY_PNG_DEFLATE_MAX_EDGE) + " pixels wide");
  pcv_ctx* ctx = x->ctx;
  const bool merged = x->kind == kXrayMerged;
  for (const XrayPartRef& r : x->parts)
    if (!xray_part_alive(r)) return ctx->fail(PCV_E_INVALID, "xray: a part of this merged quadtree was freed before it");
  if (!merged && !x->parents_built && !x->created.empty() && x->root_level < x->geo.deepest_level)
    return ctx->fail(PCV_E_INVALID, "xray: parent levels are not built (pcv_xray_build_parents)");
  XrayDirSink out;
  int rc = out.open(ctx, directory);
  if (rc) return rc;
  // copy_images: the files of opened parts byte for byte (none where the part is this directory); every other node is
  // encoded, in runs of consecutive nodes
  const uint64_t n = xray_num_nodes(x);
  std::vector<std::pair<uint64_t, uint64_t>> runs;  // first, count
  auto encode = [&](uint64_t first, uint64_t count) {
    if (count && !runs.empty() && runs.back().first + runs.back().second == first) runs.back().second += count;
    else if (count) runs.emplace_back(first, count);
  };
  uint64_t at = 0;
  std::vector<uint8_t> file;
  for (const XrayPartRef& r : x->parts) {
    at = r.first + r.count;
    if (r.part->kind != kXrayOpened) {
      encode(r.first, r.count);
      continue;
    }
    if (same_directory(r.part->dir, out.dir)) continue;
    for (uint64_t i = r.first; !rc && i < at; ++i) {
      const std::string name = node_file_name(x, i);
      if (!read_file(r.part->dir + "/" + name, file)) rc = ctx->fail(PCV_E_IO, "cannot read " + r.part->dir + "/" + name);
      else if (!out.write(name, file.data(), file.size())) rc = out.status(PCV_E_IO);
    }
  }
  encode(at, n - at);  // a merged quadtree's own levels; a built quadtree whole
  const XrayFileSink to_dir = [&](uint64_t node, const uint8_t* png, uint64_t len) { return out.write(node_file_name(x, node), png, len); };
  for (size_t i = 0; !rc && i < runs.size(); ++i) rc = out.status(xray_node_files(x, runs[i].first, runs[i].second, mode, true, to_dir));
  if (rc) return rc;
  XrayMeta m;
  double rect[3];
  if (merged || x->kind == kXrayInpainted) std::memcpy(rect, x->geo.rect, sizeof(rect));  // kept as the root's rect
  else built_root_rect(x, rect);
  m.min[0] = rect[0];
  m.min[1] = rect[1];
  m.edge = rect[2];
  m.deepest_level = x->geo.deepest_level;
  m.tile_size = x->W;
  for (uint64_t i = 0; i < n; ++i) {
    const XrayNodeId id = xray_node_id(x, i);
    m.nodes.emplace_back(id.level, id.index);
  }
  const std::vector<uint8_t> bytes = xray_meta_encode(m);
  const std::string name = merged ? xray_meta_name(0, 0) : xray_meta_name(x->root_level, x->root_index);
  return out.write(name, bytes.data(), bytes.size()) ? PCV_OK : out.status(PCV_E_IO);
}

extern "C" int pcv_xray_png_encode_tiles(pcv_ctx* ctx, const uint8_t* rgba, int mem, uint32_t w, uint64_t count, uint64_t chunk_tiles,
                                         uint64_t capacity, uint8_t* out, uint64_t* offsets) {
  if (!ctx) return PCV_E_INVALID;
  if (!offsets || (count && !rgba) || w == 0) return ctx->fail(PCV_E_INVALID, "xray: bad arguments to pcv_xray_png_encode_tiles");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (w > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return ctx->fail(PCV_E_INVALID, "xray: compressed tiles are at most " + std::to_string(PCV_XRAY_PNG_DEFLATE_MAX_EDGE) + " pixels wide");
  offsets[0] = 0;
  if (count == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint64_t tile_bytes = 4ull * w * w;
  PcvScratch sc(ctx);
  const uint8_t* tiles = rgba;
  if (mem == PCV_MEM_HOST) {
    uint8_t* d = nullptr;
    if (int rc = sc.get(&d, count * tile_bytes)) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d, rgba, count * tile_bytes, hipMemcpyHostToDevice, ctx->stream));
    tiles = d;
  }
  XrayPngAppend app{out, capacity};
  app.offsets = offsets;
  const uint64_t per_chunk = chunk_tiles ? chunk_tiles : std::max<uint64_t>(1, ctx->xray_chunk_bytes / tile_bytes);
  const int rc = xray_deflate_chunks(
      ctx, w, count, per_chunk,
      [&](uint64_t f, uint64_t, const uint8_t** a, uint64_t* na, const uint8_t** b) {
        *na = 0;
        *a = nullptr;
        *b = tiles + f * tile_bytes;
      },
      [&](uint64_t, uint64_t c, const uint8_t* streams, const uint64_t* offs) {
        std::vector<uint8_t> png;
        for (uint64_t i = 0; i < c; ++i) {
          png.resize(kPcvPngWrap + offs[i + 1] - offs[i]);
          pcv_png_wrap(w, w, streams + offs[i], offs[i + 1] - offs[i], png.data());
          app.take(png.data(), png.size());
        }
        return PCV_OK;
      });
  if (rc) return rc;
  if (!app.fits) return ctx->fail(PCV_E_INVALID, "xray: capacity below the " + std::to_string(app.at) + " bytes of these files");
  return PCV_OK;
}

extern "C" int pcv_ctx_set_xray_chunk_bytes(pcv_ctx* ctx, uint64_t bytes) {
  if (!ctx) return PCV_E_INVALID;
  ctx->xray_chunk_bytes = bytes ? bytes : 64ull << 20;
  return PCV_OK;
}
