// pcv_tiles3d.hip — an octree as an OGC 3D Tiles 1.0 tileset (the contract is stated in include/pcv_hip.h): one
// .pnts file per node that holds points, packed on the device from the node blobs the tree already holds there, returned as
// they are (pcv_tiles3d_tile_files) or streamed into a directory through two device buffers and two pinned blocks
// (pcv_tiles3d_write_dir). The container — header, JSON, which nodes are tiles, the tileset — is host code in
// pcv_tiles3d_files.cpp; its host-only entry points are at the end of this file.
//
// A piece is a run of whole files, back to back. The host uploads one block per piece: a 128-byte record per file (where its
// node's bytes are, count, encoding, cube, centre, where the file and its sections go, where its header and JSON bytes sit in
// the arena), a work list of (file, first point) items of kT3dChunkPoints points, and the arena. ONE launch packs the piece,
// one workgroup per item: the item's source bytes — a node's .xyz starts at any byte — are read as aligned 16-byte vectors into
// LDS, every lane converts its points by the chain of pcv_tiles3d_dev.h into an LDS image of the output whose byte 0 stands at
// the alignment (mod 16) the destination has, and the image leaves as aligned 16-byte vectors with a bytewise head and tail.
// Colour and intensity are the same re-alignment without arithmetic. The workgroup of a file's first item also places the
// header and JSON bytes and writes every padding byte: nothing of a file is left unwritten. All blob offsets are u64.
// The store of an image is pcv_rows_dev.h's, the piece pipeline pcv_result_rows.h's; the staging, the conversion
// and what a piece of whole files needs — an upload table per buffer, one host job per file — are this file's.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pcv_internal.h"
#include "pcv_result_rows.h"
#include "pcv_rows_dev.h"
#include "pcv_tiles3d_dev.h"
#include "pcv_tiles3d_files.h"

namespace {

constexpr uint32_t kT3dChunkPoints = 1024;
// LDS, carved from one 16-byte aligned dynamic block (no static LDS in this file): [0, kT3dSrcBytes) the staged source — 24
// bytes a point at the most, up to 15 bytes of phase in front and the rest of the last vector behind —, then the image of the
// output, 12 bytes a point at the most and 15 bytes of phase. 36.9 KiB: four workgroups a CU.
constexpr uint32_t kT3dSrcBytes = kT3dChunkPoints * 24 + 32;
constexpr uint32_t kT3dImgBytes = kT3dChunkPoints * 12 + 16;
constexpr uint32_t kT3dLdsBytes = kT3dSrcBytes + kT3dImgBytes;
static_assert(kT3dSrcBytes % 16 == 0 && kT3dImgBytes % 16 == 0, "carve offsets are multiples of 16");

struct alignas(16) T3dFile {
  uint64_t src_xyz;  // byte offset of the node's .xyz content in the xyz blob
  uint64_t src_pt;   // index of the node's first point in the rgb / intensity blobs
  uint64_t dst;      // the file's first byte in the piece
  double mn[3], edge, rc[3];
  uint32_t n, enc, mode, intensity;
  uint32_t head_at, head_len;    // header and feature JSON with its padding, in the arena; they go to byte 0 of the file
  uint32_t bjson_at, bjson_len;  // batch JSON with its padding, in the arena
  uint32_t fbin_off, bjson_off, bbin_off, file_bytes;  // section offsets from the file's start
};
static_assert(sizeof(T3dFile) == 128, "file record");

struct T3dBlobs {
  const uint8_t *xyz, *rgb, *inten;
  uint64_t xyz_bytes, rgb_bytes, int_bytes;
};

extern __shared__ __attribute__((aligned(16))) uint8_t t3d_lds[];  // the only LDS of this kernel: its base stays 16-byte aligned

// Bytes [off, off + bytes) of a blob into the source region, byte j at t3d_lds[phase + j] with phase = (its address) % 16, which
// is returned: whole aligned vectors where they lie inside the blob, bytewise where one would cross its first or last byte.
__device__ __forceinline__ uint32_t stage(const uint8_t* __restrict__ blob, uint64_t blob_bytes, uint64_t off, uint32_t bytes) {
  const uint8_t* src = blob + off;
  const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u);
  const uint8_t* base = src - phase;
  const uint8_t* end = blob + blob_bytes;
  const uint32_t nvec = (phase + bytes + 15u) >> 4;
  uint4* lv = reinterpret_cast<uint4*>(t3d_lds);
  for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
    const uint8_t* p = base + 16u * v;
    if (p >= blob && p + 16 <= end) {
      lv[v] = *reinterpret_cast<const uint4*>(p);
    } else {
      for (uint32_t k = 0; k < 16u; ++k)
        if (p + k >= src && p + k < src + bytes) t3d_lds[16u * v + k] = p[k];
    }
  }
  return phase;
}

// `bytes` bytes of a blob to dst as they are: staged, moved to the destination's phase, stored. Ends with a barrier.
__device__ __forceinline__ void realign(const uint8_t* __restrict__ blob, uint64_t blob_bytes, uint64_t off, uint32_t bytes, uint8_t* __restrict__ dst) {
  const uint32_t sphase = stage(blob, blob_bytes, off, bytes);
  const uint32_t dphase = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  __syncthreads();
  if (sphase == dphase) {  // (uniform) the staged bytes are the image
    pcv_store_image(t3d_lds, dst, dphase, bytes);
  } else {
    const uint8_t* s = t3d_lds + sphase;
    uint8_t* img = t3d_lds + kT3dSrcBytes;
    for (uint32_t j = threadIdx.x; j < bytes; j += 256u) img[dphase + j] = s[j];
    __syncthreads();
    pcv_store_image(img, dst, dphase, bytes);
  }
  __syncthreads();
}

template <typename T>
__device__ __forceinline__ T lds_get(const uint8_t* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const T*>(p);
  T v;
  uint8_t b[sizeof(T)];
#pragma unroll
  for (uint32_t k = 0; k < sizeof(T); ++k) b[k] = p[k];
  memcpy(&v, b, sizeof(T));
  return v;
}

// the staged coordinate at p as the chain takes it; `aligned`: p is a multiple of the coordinate's size (uniform)
template <uint32_t ENC>
__device__ __forceinline__ PcvTiles3dCoord coord_at(const uint8_t* p, bool aligned) {
  PcvTiles3dCoord c{0u, 0.0};
  if (ENC == PCV_ENC_UINT8) c.code = p[0];
  else if (ENC == PCV_ENC_UINT16) c.code = lds_get<uint16_t>(p, aligned);
  else if (ENC == PCV_ENC_FLOAT32) c.t = (double)lds_get<float>(p, aligned);
  else c.t = lds_get<double>(p, aligned);
  return c;
}

// points [0, m) of the staged source (at t3d_lds + sphase) into the image (byte 0 at img[dphase])
template <uint32_t ENC>
__device__ __forceinline__ void convert(const T3dFile& f, uint32_t sphase, uint32_t dphase, uint32_t m) {
  constexpr uint32_t CB = ENC == PCV_ENC_UINT8 ? 1u : ENC == PCV_ENC_UINT16 ? 2u : ENC == PCV_ENC_FLOAT32 ? 4u : 8u;
  const uint8_t* s = t3d_lds + sphase;
  uint8_t* img = t3d_lds + kT3dSrcBytes + dphase;
  const bool src_aligned = (sphase & (CB - 1u)) == 0;  // a point is 3 CB bytes: every coordinate is as aligned as the first
  if (f.mode == PCV_TILES3D_POS_QUANTIZED) {
    const bool dst_aligned = (dphase & 1u) == 0;
    for (uint32_t i = threadIdx.x; i < m; i += 256u) {
#pragma unroll
      for (uint32_t a = 0; a < 3u; ++a) {
        const uint16_t q = pcv_tiles3d_quantized(ENC, coord_at<ENC>(s + i * 3u * CB + a * CB, src_aligned));
        uint8_t* o = img + i * 6u + 2u * a;
        if (dst_aligned) *reinterpret_cast<uint16_t*>(o) = q;
        else o[0] = (uint8_t)q, o[1] = (uint8_t)(q >> 8);
      }
    }
  } else {
    const bool dst_aligned = (dphase & 3u) == 0;
    for (uint32_t i = threadIdx.x; i < m; i += 256u) {
#pragma unroll
      for (uint32_t a = 0; a < 3u; ++a) {
        const float v = pcv_tiles3d_float(ENC, coord_at<ENC>(s + i * 3u * CB + a * CB, src_aligned), f.mn[a], f.edge, f.rc[a]);
        const uint32_t b = __float_as_uint(v);
        uint8_t* o = img + i * 12u + 4u * a;
        if (dst_aligned) *reinterpret_cast<uint32_t*>(o) = b;
        else o[0] = (uint8_t)b, o[1] = (uint8_t)(b >> 8), o[2] = (uint8_t)(b >> 16), o[3] = (uint8_t)(b >> 24);
      }
    }
  }
}

// One workgroup per item: points [p0, p0 + m) of file items[blockIdx.x].x.
__global__ __launch_bounds__(256) void tiles3d_pack_kernel(const T3dFile* __restrict__ files, const uint2* __restrict__ items,
                                                            const uint8_t* __restrict__ arena, T3dBlobs blobs, uint8_t* __restrict__ out) {
  const uint2 item = items[blockIdx.x];
  const T3dFile f = files[item.x];  // (uniform: scalar loads)
  const uint32_t p0 = item.y, m = min(kT3dChunkPoints, f.n - p0);
  uint8_t* file = out + f.dst;
  const uint32_t cb = pcv_tiles3d_src_bytes(f.enc), sstride = 3u * cb, dstride = f.mode == PCV_TILES3D_POS_QUANTIZED ? 6u : 12u;
  if (p0 == 0) {  // the file's first item: header, JSON, every padding byte
    for (uint32_t j = threadIdx.x; j < f.head_len; j += 256u) file[j] = arena[f.head_at + j];
    for (uint32_t j = f.fbin_off + f.n * (dstride + 3u) + threadIdx.x; j < f.bjson_off; j += 256u) file[j] = 0;
    for (uint32_t j = threadIdx.x; j < f.bjson_len; j += 256u) file[f.bjson_off + j] = arena[f.bjson_at + j];
    if (f.intensity)
      for (uint32_t j = f.bbin_off + 4u * f.n + threadIdx.x; j < f.file_bytes; j += 256u) file[j] = 0;
  }
  // positions
  uint8_t* pos = file + f.fbin_off + (uint64_t)p0 * dstride;
  const uint32_t dphase = (uint32_t)(reinterpret_cast<uintptr_t>(pos) & 15u);
  const uint32_t sphase = stage(blobs.xyz, blobs.xyz_bytes, f.src_xyz + (uint64_t)p0 * sstride, m * sstride);
  __syncthreads();
  switch (f.enc) {  // (uniform)
    case PCV_ENC_UINT8: convert<PCV_ENC_UINT8>(f, sphase, dphase, m); break;
    case PCV_ENC_UINT16: convert<PCV_ENC_UINT16>(f, sphase, dphase, m); break;
    case PCV_ENC_FLOAT32: convert<PCV_ENC_FLOAT32>(f, sphase, dphase, m); break;
    default: convert<PCV_ENC_FLOAT64>(f, sphase, dphase, m); break;
  }
  __syncthreads();
  pcv_store_image(t3d_lds + kT3dSrcBytes, pos, dphase, m * dstride);
  __syncthreads();
  // colours, after the file's last position without a gap; intensity
  realign(blobs.rgb, blobs.rgb_bytes, (f.src_pt + p0) * 3u, m * 3u, file + f.fbin_off + (uint64_t)f.n * dstride + (uint64_t)p0 * 3u);
  if (f.intensity) realign(blobs.inten, blobs.int_bytes, (f.src_pt + p0) * 4u, m * 4u, file + f.bbin_off + (uint64_t)p0 * 4u);
}

}  // namespace

struct pcv_tiles3d {
  pcv_ctx* ctx = nullptr;
  pcv_octree* tree = nullptr;
  pcv_tiles3d_params params{};
  pcv_tiles3d_info info{};
  std::vector<PcvTiles3dFilePlan> files;  // the content tiles, in node-table order
  std::vector<uint64_t> node_of;          // their nodes
  std::vector<uint64_t> file_bytes;
  std::string json;
};

namespace {

// The upload block of files [first, first + count) laid out back to back from byte 0 of a piece: records, items, arena.
struct T3dUpload {
  std::vector<uint8_t> bytes;
  size_t items_at = 0, arena_at = 0;
  uint64_t num_items = 0, piece_bytes = 0;
};
size_t upload_bytes(const pcv_tiles3d* t, uint64_t first, uint64_t count, uint64_t* num_items) {
  uint64_t items = 0, arena = 0;
  for (uint64_t k = first; k < first + count; ++k) {
    items += (t->files[k].n + kT3dChunkPoints - 1) / kT3dChunkPoints;
    arena += t->files[k].head.size() + t->files[k].batch_json.size();
  }
  if (num_items) *num_items = items;
  return (size_t)(count * sizeof(T3dFile) + ((items * sizeof(uint2) + 15) & ~15ull) + ((arena + 15) & ~15ull));
}
int make_upload(const pcv_tiles3d* t, uint64_t first, uint64_t count, T3dUpload* up) {
  pcv_ctx* ctx = t->ctx;
  up->bytes.assign(upload_bytes(t, first, count, &up->num_items), 0);
  up->items_at = (size_t)count * sizeof(T3dFile);
  up->arena_at = up->items_at + (size_t)((up->num_items * sizeof(uint2) + 15) & ~15ull);
  if (up->bytes.size() - up->arena_at > 0xffffffffull || count > 0xffffffffull) return ctx->fail(PCV_E_INVALID, "too many files for one piece");
  T3dFile* rec = reinterpret_cast<T3dFile*>(up->bytes.data());
  uint2* item = reinterpret_cast<uint2*>(up->bytes.data() + up->items_at);
  uint8_t* arena = up->bytes.data() + up->arena_at;
  uint64_t dst = 0, at = 0, it = 0;
  for (uint64_t k = 0; k < count; ++k) {
    const PcvTiles3dFilePlan& f = t->files[first + k];
    const pcv_node_info& nd = t->tree->nodes[t->node_of[first + k]];
    T3dFile& r = rec[k];
    r.src_xyz = nd.xyz_offset, r.src_pt = nd.point_offset, r.dst = dst;
    for (int a = 0; a < 3; ++a) r.mn[a] = nd.cube_min[a], r.rc[a] = f.rc[a];
    r.edge = nd.cube_edge;
    r.n = (uint32_t)f.n, r.enc = f.encoding, r.mode = f.mode, r.intensity = f.intensity ? 1u : 0u;
    r.head_at = (uint32_t)at, r.head_len = (uint32_t)f.head.size();
    std::memcpy(arena + at, f.head.data(), f.head.size());
    at += f.head.size();
    r.bjson_at = (uint32_t)at, r.bjson_len = (uint32_t)f.batch_json.size();
    std::memcpy(arena + at, f.batch_json.data(), f.batch_json.size());
    at += f.batch_json.size();
    r.fbin_off = (uint32_t)f.feature_binary_offset, r.bjson_off = (uint32_t)f.batch_json_offset;
    r.bbin_off = (uint32_t)f.batch_binary_offset, r.file_bytes = (uint32_t)f.file_bytes;
    for (uint64_t p0 = 0; p0 < f.n; p0 += kT3dChunkPoints) item[it++] = make_uint2((uint32_t)k, (uint32_t)p0);
    dst += f.file_bytes;
  }
  up->piece_bytes = dst;
  return PCV_OK;
}

// files [first, first + count) into d_out on the context's stream: the upload (into d_up, which holds up->bytes.size() bytes;
// `up` stays alive until the stream has passed the copy) and ONE launch. Nothing is waited for.
int launch_piece(pcv_tiles3d* t, const T3dUpload& up, uint8_t* d_up, uint8_t* d_out) {
  pcv_ctx* ctx = t->ctx;
  const pcv_octree* tree = t->tree;
  if (up.num_items == 0) return PCV_OK;
  if (up.num_items > 0x7fffffffull) return ctx->fail(PCV_E_INVALID, "too many points for one launch: pack the tiles in pieces");
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_up, up.bytes.data(), up.bytes.size(), hipMemcpyHostToDevice, ctx->stream));
  const T3dBlobs blobs{tree->d_xyz, tree->d_rgb, tree->d_int, tree->xyz_bytes, tree->rgb_bytes, tree->int_bytes};
  {
    PcvProf prof(ctx, PCV_K_TILES3D_PACK);
    hipLaunchKernelGGL(tiles3d_pack_kernel, dim3((uint32_t)up.num_items), dim3(256), kT3dLdsBytes, ctx->stream, (const T3dFile*)d_up,
                       (const uint2*)(d_up + up.items_at), (const uint8_t*)(d_up + up.arena_at), blobs, d_out);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

int check_live(const pcv_tiles3d* t) {
  if (!t->tree->d_xyz || !t->tree->d_rgb || (t->params.flags & PCV_TILES3D_INTENSITY && !t->tree->d_int))
    return t->ctx->fail(PCV_E_INVALID, "the octree's node bytes are not on the device");
  return PCV_OK;
}

bool write_file_at(int dirfd, const std::string& name, const uint8_t* data, uint64_t len) {
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

struct T3dDir {  // the output directory, open while its files are written
  int fd = -1;
  ~T3dDir() {
    if (fd >= 0) ::close(fd);
  }
};

}  // namespace

extern "C" int pcv_tiles3d_plan(pcv_octree* tree, const pcv_tiles3d_params* params, pcv_tiles3d** out) {
  if (out) *out = nullptr;
  if (!tree || !tree->ctx) return PCV_E_INVALID;
  pcv_ctx* ctx = tree->ctx;
  if (!params || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  std::string why;
  if (int rc = pcv_tiles3d_check_params(params, &why)) return ctx->fail(rc, why);
  if (tree->pending) return ctx->fail(PCV_E_INVALID, "the octree's build is not finished");
  if ((params->flags & PCV_TILES3D_INTENSITY) && !tree->has_intensity) return ctx->fail(PCV_E_INVALID, "PCV_TILES3D_INTENSITY: the octree carries no intensity");
  std::unique_ptr<pcv_tiles3d> t(new pcv_tiles3d);
  t->ctx = ctx, t->tree = tree, t->params = *params;
  std::vector<uint8_t> kinds;
  if (int rc = pcv_tiles3d_tileset(tree->nodes.data(), tree->nodes.size(), *params, &t->json, &kinds, &why)) return ctx->fail(rc, why);
  const uint64_t chunk = params->chunk_bytes ? params->chunk_bytes : PCV_TILES3D_DEFAULT_CHUNK_BYTES;
  for (size_t i = 0; i < kinds.size(); ++i) {
    if (kinds[i]) ++t->info.tiles;
    if (kinds[i] != 2) continue;
    PcvTiles3dFilePlan f;
    if (int rc = pcv_tiles3d_file_plan(tree->nodes[i], *params, tree->has_intensity, &f, &why)) return ctx->fail(rc, why);
    if (f.file_bytes > chunk)
      return ctx->fail(PCV_E_INVALID, "the file of node " + pcv_tiles3d_node_name(tree->nodes[i]) + " holds " + std::to_string(f.file_bytes) +
                                          " bytes, chunk_bytes is " + std::to_string(chunk));
    t->info.points += f.n;
    t->info.total_file_bytes += f.file_bytes;
    t->file_bytes.push_back(f.file_bytes);
    t->node_of.push_back(i);
    t->files.push_back(std::move(f));
  }
  t->info.content_tiles = t->files.size();
  t->info.chunk_points = kT3dChunkPoints;
  if (!tree->directory.empty())
    if (int rc = pcv_octree_load_device(tree)) return rc;
  if (int rc = check_live(t.get())) return rc;
  *out = t.release();
  return PCV_OK;
}

extern "C" int pcv_tiles3d_info_get(const pcv_tiles3d* t, pcv_tiles3d_info* out) {
  if (!t || !out) return PCV_E_INVALID;
  *out = t->info;
  return PCV_OK;
}

extern "C" int pcv_tiles3d_tiles(const pcv_tiles3d* t, uint64_t capacity, pcv_tiles3d_tile* out, uint64_t* num_tiles) {
  if (!t) return PCV_E_INVALID;
  if (num_tiles) *num_tiles = t->files.size();
  if (capacity && !out) return t->ctx->fail(PCV_E_INVALID, "null output");
  for (uint64_t k = 0; k < std::min<uint64_t>(capacity, t->files.size()); ++k) pcv_tiles3d_fill_tile(t->files[k], t->node_of[k], out + k);
  return PCV_OK;
}

extern "C" int pcv_tiles3d_tile_files(pcv_tiles3d* t, uint64_t first, uint64_t count, int mem, uint64_t capacity, uint8_t* out, uint64_t* offsets) {
  if (!t) return PCV_E_INVALID;
  pcv_ctx* ctx = t->ctx;
  if (first > t->files.size() || count > t->files.size() - first) return ctx->fail(PCV_E_INVALID, "tile range past the end");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  uint64_t total = 0;
  for (uint64_t k = 0; k < count; ++k) {
    if (offsets) offsets[k] = total;
    total += t->file_bytes[first + k];
  }
  if (offsets) offsets[count] = total;
  if (!out || count == 0) return PCV_OK;
  if (capacity < total) return ctx->fail(PCV_E_INVALID, "the tiles hold " + std::to_string(total) + " bytes, capacity is " + std::to_string(capacity) + " bytes");
  int rc;
  if ((rc = check_live(t))) return rc;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  T3dUpload up;
  if ((rc = make_upload(t, first, count, &up))) return rc;
  PcvScratch sc(ctx);
  uint8_t *d_up, *d_out = out;
  if ((rc = sc.get(&d_up, up.bytes.size())) || (mem == PCV_MEM_HOST && (rc = sc.get(&d_out, total)))) return rc;
  rc = launch_piece(t, up, d_up, d_out);
  if (!rc && mem == PCV_MEM_HOST && hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
    rc = ctx->fail(PCV_E_HIP, "copying the tile files to the host failed");
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && !rc) rc = ctx->fail(PCV_E_HIP, "packing the tile files failed");  // `up` lives until here
  if (rc) return rc;
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_tiles3d_tileset_json(const pcv_tiles3d* t, char* buf, uint64_t cap, uint64_t* len) {
  if (!t) return PCV_E_INVALID;
  if (len) *len = t->json.size();
  if (buf && cap) std::memcpy(buf, t->json.data(), (size_t)std::min<uint64_t>(cap, t->json.size()));
  return PCV_OK;
}

// pcv_tiles3d_write_dir: whole files through the piece pipeline, one host job per file. Device and pinned memory: two buffers
// of the largest piece, two upload blocks of the largest table.
extern "C" int pcv_tiles3d_write_dir(pcv_tiles3d* t, const char* directory) {
  if (!t) return PCV_E_INVALID;
  pcv_ctx* ctx = t->ctx;
  if (!directory) return ctx->fail(PCV_E_INVALID, "null argument");
  int rc;
  if ((rc = check_live(t))) return rc;
  const std::string dir(directory);
  ::mkdir(dir.c_str(), 0777);  // it may be there already
  struct stat st;
  if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) return ctx->fail(PCV_E_IO, "cannot create directory " + dir);
  T3dDir d;
  d.fd = open(dir.c_str(), O_RDONLY | O_DIRECTORY | O_CLOEXEC);
  if (d.fd < 0) return ctx->fail(PCV_E_IO, "cannot open directory " + dir);
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint64_t chunk = t->params.chunk_bytes ? t->params.chunk_bytes : PCV_TILES3D_DEFAULT_CHUNK_BYTES;
  const std::vector<uint64_t> first = pcv_tiles3d_pieces(t->file_bytes, chunk);
  const uint64_t npieces = first.size() - 1;
  uint64_t most = 0;
  size_t most_up = 0;
  for (uint64_t k = 0; k < npieces; ++k) {
    uint64_t b = 0;
    for (uint64_t i = first[k]; i < first[k + 1]; ++i) b += t->file_bytes[i];
    most = std::max(most, b);
    most_up = std::max(most_up, upload_bytes(t, first[k], first[k + 1] - first[k], nullptr));
  }
  const uint64_t buf_bytes = (most + 255) & ~255ull;
  PcvScratch sc(ctx);
  uint8_t *d_buf[2], *d_up[2];
  PcvPiecePipe pipe;
  if ((rc = sc.get(&d_buf[0], buf_bytes)) || (rc = sc.get(&d_buf[1], buf_bytes)) || (rc = sc.get(&d_up[0], most_up)) || (rc = sc.get(&d_up[1], most_up)) ||
      (rc = ctx->pinned_reserve(2 * buf_bytes)) || (rc = pipe.make(ctx)) || (rc = ctx->ring_ensure()))  // the ring's host threads write the files
    return rc;
  uint8_t* h_buf[2] = {(uint8_t*)ctx->pinned, (uint8_t*)ctx->pinned + buf_bytes};
  T3dUpload up[2];  // with d_up: one per buffer, free again when the buffer is
  rc = pcv_run_pieces(
      ctx, pipe, npieces,
      [&](uint64_t k, int b) -> int {
        if (int r = make_upload(t, first[k], first[k + 1] - first[k], &up[b])) return r;
        return launch_piece(t, up[b], d_up[b], d_buf[b]);
      },
      [&](uint64_t k) { return up[k & 1].piece_bytes; }, d_buf, h_buf,
      [&](uint64_t k, int b) -> int {
        if (hipEventSynchronize(pipe.copied[b]) != hipSuccess) return ctx->fail(PCV_E_HIP, "copying tile files to the host failed");
        const uint64_t f0 = first[k], nf = first[k + 1] - f0;
        std::vector<uint64_t> at(nf + 1, 0);
        for (uint64_t i = 0; i < nf; ++i) at[i + 1] = at[i] + t->file_bytes[f0 + i];
        std::vector<uint8_t> bad(nf, 0);
        ctx->host_pool.run((size_t)nf, [&](size_t i) {
          const std::string name = pcv_tiles3d_node_name(t->tree->nodes[t->node_of[f0 + i]]) + ".pnts";
          if (!write_file_at(d.fd, name, h_buf[b] + at[i], t->file_bytes[f0 + i])) bad[i] = 1;
        });
        for (uint64_t i = 0; i < nf; ++i)
          if (bad[i]) return ctx->fail(PCV_E_IO, "cannot write " + dir + "/" + pcv_tiles3d_node_name(t->tree->nodes[t->node_of[f0 + i]]) + ".pnts");
        return PCV_OK;
      });
  if (rc) return rc;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->side) != hipSuccess) return ctx->fail(PCV_E_HIP, "packing the tile files failed");
  ctx->prof_resolve();
  // tileset.json last: a directory that has it is complete
  if (!write_file_at(d.fd, "tileset.json", (const uint8_t*)t->json.data(), t->json.size())) return ctx->fail(PCV_E_IO, "cannot write " + dir + "/tileset.json");
  return PCV_OK;
}

extern "C" void pcv_tiles3d_free(pcv_tiles3d* t) { delete t; }

// ---- the host-only entry points (pcv_tiles3d_files.cpp) -----------------------------------------------------------------------
extern "C" int pcv_tiles3d_check_params_host(const pcv_tiles3d_params* params) {
  std::string why;
  if (int rc = pcv_tiles3d_check_params(params, &why)) return pcv_host_fail(rc, why);
  return PCV_OK;
}

extern "C" int pcv_tiles3d_rtc_host(const pcv_node_info* node, double rc[3]) {
  if (!node || !rc) return pcv_host_fail(PCV_E_INVALID, "null argument");
  for (int a = 0; a < 3; ++a) rc[a] = pcv_tiles3d_rtc(node->cube_min[a], node->cube_edge);
  return PCV_OK;
}

extern "C" int pcv_tiles3d_tile_host(const pcv_node_info* node, const pcv_tiles3d_params* params, const uint8_t* xyz, const uint8_t* rgb,
                                     const float* intensity, uint8_t* out, uint64_t capacity, uint64_t* len, pcv_tiles3d_tile* tile) {
  std::string why;
  if (int rc = pcv_tiles3d_tile_into(node, params, xyz, rgb, intensity, out, capacity, len, tile, &why)) return pcv_host_fail(rc, why);
  return PCV_OK;
}

extern "C" int pcv_tiles3d_tileset_json_host(const pcv_node_info* nodes, uint64_t count, const pcv_tiles3d_params* params, char* buf, uint64_t cap,
                                             uint64_t* len) {
  std::string why;
  if (int rc = pcv_tiles3d_tileset_into(nodes, count, params, buf, cap, len, &why)) return pcv_host_fail(rc, why);
  return PCV_OK;
}
