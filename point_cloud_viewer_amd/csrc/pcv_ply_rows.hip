// pcv_ply_rows.hip — the result of a batched point query as the rows of a binary PLY: packed on the device from
// the query's own tables, returned as they are (pcv_query_batch_ply_rows, pcv_s2_query_ply_rows) or streamed into a file
// through two device buffers and two pinned blocks (pcv_query_batch_write_ply, pcv_s2_query_write_ply). The format itself —
// columns, header, append — is host code in pcv_ply_write.cpp; its three host-only entry points are at the end of this file.
//
// A row is the transpose of what the device holds: position as three doubles, then the attribute columns ascending by name,
// packed without padding, so a stride is 24 + anything and a workgroup's byte range starts at any alignment. One workgroup
// packs one TILE of `tile_rows` consecutive rows: it finds the chunk that holds the tile's first row by bisection over the
// scanned chunk offsets, its waves walk the chunks from there (ranks by ballot over the keep bytes for the octree batch, as
// query_compact_kernel counts them; the per-candidate offsets for an S2 query), every lane writes its point's row into an LDS
// image of the tile whose byte 0 stands at the alignment (mod 16) the tile has in the output, and the image leaves as aligned
// 16-byte vectors with a bytewise head and tail. All byte offsets into the output are u64.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pcv_internal.h"
#include "pcv_ply_write.h"
#include "pcv_query_dev.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_query_dev.h"

namespace {

constexpr int kPlyMaxCols = 2 + PCV_S2_MAX_EXTRAS;  // color, intensity, the extras
struct PlyCol {
  const uint8_t* base;  // the column on the device, element i at base + i * elem
  uint32_t elem, off;   // bytes per point; byte offset inside the row
};
struct PlyCols {
  uint32_t n, stride;
  PlyCol c[kPlyMaxCols];
};
// Two workgroups of the largest tile fit a CU's 160 KiB of LDS with room to spare; smaller tiles keep more waves per CU for
// the gathers. The image is tile_rows * stride + 15 bytes (the phase).
constexpr uint32_t kPlyTileBytes = 32u << 10;
inline uint32_t ply_tile_rows(uint32_t stride) { return std::max(1u, kPlyTileBytes / stride); }
constexpr uint64_t kPlyDefaultChunkPoints = 1ull << 20;

extern __shared__ __attribute__((aligned(16))) uint8_t ply_image[];  // the only LDS of these kernels: its base stays 16-byte aligned

// WORDS: every row of the image starts on a dword (stride % 4 == 0 and an output on a dword: every tile's phase is then a
// multiple of 4 as well)
template <bool WORDS>
__device__ __forceinline__ void put32(uint8_t* dst, uint32_t off, uint32_t v) {
  if (WORDS && (off & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(dst + off) = v;
  } else {
    dst[off] = (uint8_t)v, dst[off + 1] = (uint8_t)(v >> 8), dst[off + 2] = (uint8_t)(v >> 16), dst[off + 3] = (uint8_t)(v >> 24);
  }
}
template <bool WORDS>
__device__ __forceinline__ void put64(uint8_t* dst, uint32_t off, uint64_t v) {
  put32<WORDS>(dst, off, (uint32_t)v);
  put32<WORDS>(dst, off + 4, (uint32_t)(v >> 32));
}

// the attribute columns of point `i` into its row; the element size is uniform over the wave
template <bool WORDS>
__device__ __forceinline__ void put_columns(uint8_t* row, const PlyCols& cols, uint64_t i) {
  for (uint32_t k = 0; k < cols.n; ++k) {
    const PlyCol c = cols.c[k];
    switch (c.elem) {
      case 1: row[c.off] = c.base[i]; break;
      case 2: {
        const uint16_t v = reinterpret_cast<const uint16_t*>(c.base)[i];
        row[c.off] = (uint8_t)v, row[c.off + 1] = (uint8_t)(v >> 8);
        break;
      }
      case 3: {
        const uint8_t* s = c.base + 3 * i;
        row[c.off] = s[0], row[c.off + 1] = s[1], row[c.off + 2] = s[2];
        break;
      }
      case 4: put32<WORDS>(row, c.off, reinterpret_cast<const uint32_t*>(c.base)[i]); break;
      case 8: put64<WORDS>(row, c.off, reinterpret_cast<const uint64_t*>(c.base)[i]); break;
      default: {  // 24: F64Vec3
        const uint64_t* s = reinterpret_cast<const uint64_t*>(c.base) + 3 * i;
        put64<WORDS>(row, c.off, s[0]);
        put64<WORDS>(row, c.off + 8, s[1]);
        put64<WORDS>(row, c.off + 16, s[2]);
      }
    }
  }
}

// The image of `bytes` bytes, whose byte 0 stands at ply_image[phase] with phase = (address of dst) % 16, to dst: the interior
// as aligned 16-byte vectors, its unaligned head and tail bytewise.
__device__ __forceinline__ void store_image(uint8_t* __restrict__ dst, uint32_t phase, uint32_t bytes) {
  const uint32_t head = min(bytes, (16u - phase) & 15u);
  for (uint32_t j = threadIdx.x; j < head; j += 256u) dst[j] = ply_image[phase + j];
  const uint32_t nvec = (bytes - head) >> 4;
  uint4* __restrict__ gv = reinterpret_cast<uint4*>(dst + head);
  const uint4* lv = reinterpret_cast<const uint4*>(ply_image + phase + head);  // phase + head is 0 or 16
  for (uint32_t v = threadIdx.x; v < nvec; v += 256u) gv[v] = lv[v];
  const uint32_t done = head + (nvec << 4);
  for (uint32_t j = done + threadIdx.x; j < bytes; j += 256u) dst[j] = ply_image[phase + j];
}

// the last chunk c of [c0, c1) whose first row start(c) is <= g; start(c0) <= g by the caller's choice of c0
template <typename Start>
__device__ __forceinline__ uint64_t chunk_of_row(uint64_t c0, uint64_t c1, uint64_t g, Start start) {
  uint64_t lo = c0, hi = c1;  // start(lo) <= g, start(hi) > g (or hi == c1)
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (start(mid) <= g) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Rows [row0 + blockIdx.x * tile_rows, ...) of the octree batch, `nrows` from row0 on, to out + (row - row0) * stride. The chunks
// [c0, c1) are those of the caller's segment range; chunk_off their scanned kept counts (the row of a chunk's first kept point).
template <bool WORDS>
__global__ __launch_bounds__(256) void ply_rows_octree_kernel(const ChunkDesc* __restrict__ desc, uint64_t c0, uint64_t c1,
                                                               const uint8_t* __restrict__ xyz_blob, const uint8_t* __restrict__ keep,
                                                               const uint64_t* __restrict__ chunk_off, PlyCols cols, uint64_t row0,
                                                               uint64_t nrows, uint32_t tile_rows, uint8_t* __restrict__ out) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t t0 = (uint64_t)blockIdx.x * tile_rows;
  const uint32_t rows = (uint32_t)min((uint64_t)tile_rows, nrows - t0);
  const uint64_t g0 = row0 + t0, g1 = g0 + rows;
  uint8_t* dst = out + t0 * cols.stride;
  const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const uint64_t first = chunk_of_row(c0, c1, g0, [&](uint64_t c) { return chunk_off[c]; });
  for (uint64_t ci = first + wave; ci < c1; ci += 4) {
    uint64_t pos0 = chunk_off[ci];
    if (pos0 >= g1) break;                   // (uniform) offsets only grow
    if (chunk_off[ci + 1] <= g0) continue;   // nothing of this chunk in the tile (an empty chunk among them)
    const ChunkDesc& d = desc[ci];
    PointsView v{};
    v.encoded = xyz_blob + d.src;
    v.enc = d.enc & 15u;
    v.cube_min[0] = d.cube_min[0];
    v.cube_min[1] = d.cube_min[1];
    v.cube_min[2] = d.cube_min[2];
    v.cube_edge = d.cube_edge;
    const uint8_t* kp = keep + d.keep_off;
    for (uint32_t q0 = 0; q0 < d.cnt && pos0 < g1; q0 += 64) {
      const uint32_t q = q0 + lane;
      const unsigned long long b = __ballot(q < d.cnt && kp[q]);
      const uint64_t pos = pos0 + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
      if (((b >> lane) & 1ull) && pos >= g0 && pos < g1) {
        const V3d p = load_point(v, q);  // the decode of query_compact_kernel: the same bits as pcv_query_batch_points
        uint8_t* row = ply_image + phase + (uint32_t)(pos - g0) * cols.stride;
        put64<WORDS>(row, 0, (uint64_t)__double_as_longlong(p.x));
        put64<WORDS>(row, 8, (uint64_t)__double_as_longlong(p.y));
        put64<WORDS>(row, 16, (uint64_t)__double_as_longlong(p.z));
        put_columns<WORDS>(row, cols, d.attr_index + q);
      }
      pos0 += (uint64_t)__popcll(b);
    }
  }
  __syncthreads();
  store_image(dst, phase, rows * cols.stride);
}

// The same over an S2 query: u32 flags and a scanned offset per candidate, positions copied as the 24 bytes they are.
template <bool WORDS>
__global__ __launch_bounds__(256) void ply_rows_s2_kernel(const PcvS2Chunk* __restrict__ chunks, uint64_t c0, uint64_t c1,
                                                           const uint8_t* __restrict__ xyz, const uint32_t* __restrict__ flags,
                                                           const uint64_t* __restrict__ offsets, PlyCols cols, uint64_t row0, uint64_t nrows,
                                                           uint32_t tile_rows, uint8_t* __restrict__ out) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t t0 = (uint64_t)blockIdx.x * tile_rows;
  const uint32_t rows = (uint32_t)min((uint64_t)tile_rows, nrows - t0);
  const uint64_t g0 = row0 + t0, g1 = g0 + rows;
  uint8_t* dst = out + t0 * cols.stride;
  const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
  const uint64_t first = chunk_of_row(c0, c1, g0, [&](uint64_t c) { return offsets[chunks[c].first]; });
  for (uint64_t ci = first + wave; ci < c1; ci += 4) {
    const PcvS2Chunk c = chunks[ci];
    if (offsets[c.first] >= g1) break;
    if (offsets[c.first + c.count] <= g0) continue;
    for (uint32_t q = lane; q < c.count; q += 64) {
      if (!flags[c.first + q]) continue;
      const uint64_t pos = offsets[c.first + q];
      if (pos < g0 || pos >= g1) continue;
      const uint64_t i = c.src + q;
      const uint64_t* p = reinterpret_cast<const uint64_t*>(xyz) + 3 * i;
      uint8_t* row = ply_image + phase + (uint32_t)(pos - g0) * cols.stride;
      put64<WORDS>(row, 0, p[0]);
      put64<WORDS>(row, 8, p[1]);
      put64<WORDS>(row, 16, p[2]);
      put_columns<WORDS>(row, cols, i);
    }
  }
  __syncthreads();
  store_image(dst, phase, rows * cols.stride);
}

// ---- what the two kinds of result share on the host -------------------------------------------------------------------------
// A result as the packer sees it: the columns it can name, its segment tables, and the launch of its kernel.
struct PlySource {
  pcv_ctx* ctx = nullptr;
  pcv_query_batch* octree = nullptr;
  pcv_s2_query* s2 = nullptr;
  uint64_t nseg = 0;
  const uint64_t *seg_off = nullptr, *seg_chunk = nullptr;  // nseg + 1 each
};

PlySource source_of(pcv_query_batch* b) {
  PlySource s;
  s.ctx = b->ctx, s.octree = b, s.nseg = b->nseg, s.seg_off = b->seg_off.data(), s.seg_chunk = b->seg_chunk.data();
  return s;
}
PlySource source_of(pcv_s2_query* q) {
  PlySource s;
  s.ctx = q->cloud->ctx, s.s2 = q, s.nseg = q->nseg, s.seg_off = q->seg_offset.data(), s.seg_chunk = q->seg_first_chunk.data();
  return s;
}

// `attributes` (NULL: every attribute the cloud has) as the sorted columns of a row and their device sources. Loads the named
// extras of a cloud opened from a directory, and only those.
int resolve_columns(const PlySource& s, const char* const* attributes, uint32_t num_attributes, std::vector<PcvPlyColumn>* cols, uint32_t* stride,
                    PlyCols* dev) {
  pcv_ctx* ctx = s.ctx;
  std::vector<std::string> have_names;
  std::vector<int32_t> have_types;
  have_names.push_back("color"), have_types.push_back(PCV_ATTR_U8VEC3);
  const bool has_intensity = s.octree ? s.octree->has_intensity : s.s2->cloud->has_intensity;
  if (has_intensity) have_names.push_back("intensity"), have_types.push_back(PCV_ATTR_F32);
  if (s.s2)
    for (const PcvS2Extra& e : s.s2->cloud->extras) have_names.push_back(e.name), have_types.push_back(e.data_type);
  std::vector<const char*> names;
  std::vector<int32_t> types;
  if (!attributes) {
    for (size_t k = 0; k < have_names.size(); ++k) names.push_back(have_names[k].c_str()), types.push_back(have_types[k]);
  } else {
    for (uint32_t k = 0; k < num_attributes; ++k) {
      if (!attributes[k]) return ctx->fail(PCV_E_INVALID, "attribute " + std::to_string(k) + " is null");
      const auto it = std::find(have_names.begin(), have_names.end(), std::string(attributes[k]));
      names.push_back(attributes[k]);
      types.push_back(it == have_names.end() ? 0 : have_types[(size_t)(it - have_names.begin())]);  // 0: "... not found."
    }
  }
  std::string why;
  if (pcv_ply_columns(names.data(), types.data(), (uint32_t)names.size(), cols, stride, &why)) return ctx->fail(PCV_E_INVALID, why);
  if (cols->size() > (size_t)kPlyMaxCols) return ctx->fail(PCV_E_INVALID, "too many attributes");
  dev->n = (uint32_t)cols->size(), dev->stride = *stride;
  for (size_t k = 0; k < cols->size(); ++k) {
    const PcvPlyColumn& c = (*cols)[k];
    const uint8_t* base = nullptr;
    if (c.name == "color") base = s.octree ? s.octree->tree->d_rgb : s.s2->cloud->d_rgb;
    else if (c.name == "intensity") base = s.octree ? s.octree->tree->d_int : s.s2->cloud->d_int;
    else {
      const int e = s.s2->cloud->find_extra(c.name.c_str());
      if (int rc = pcv_s2_extra_resident(s.s2->cloud, (size_t)e)) return rc;
      base = s.s2->cloud->extras[(size_t)e].d;
    }
    dev->c[k] = PlyCol{base, c.elem, c.offset};
  }
  return PCV_OK;
}

// rows [row0, row0 + nrows) of the result, found among the chunks [c0, c1), into d_out (device) on ctx->stream
int launch_rows(const PlySource& s, const PlyCols& cols, uint64_t c0, uint64_t c1, uint64_t row0, uint64_t nrows, uint8_t* d_out) {
  pcv_ctx* ctx = s.ctx;
  const uint32_t tile = ply_tile_rows(cols.stride);
  const uint64_t blocks = (nrows + tile - 1) / tile;
  if (blocks > 0x7fffffffull) return ctx->fail(PCV_E_INVALID, "too many rows for one launch: pack the result in pieces");
  const size_t lds = (size_t)tile * cols.stride + 16;
  const bool words = cols.stride % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % 4 == 0;  // then every row of every tile's image starts on a dword
  const dim3 grid((uint32_t)blocks), block(256);
  if (s.octree) {
    const pcv_query_batch* b = s.octree;
    PcvProf prof(ctx, PCV_K_PLY_ROWS);
    auto kernel = words ? ply_rows_octree_kernel<true> : ply_rows_octree_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, (const ChunkDesc*)b->d_desc, c0, c1, (const uint8_t*)b->tree->d_xyz,
                       (const uint8_t*)b->d_keep, (const uint64_t*)b->d_chunk_off, cols, row0, nrows, tile, d_out);
  } else {
    const pcv_s2_query* q = s.s2;
    PcvProf prof(ctx, PCV_K_PLY_ROWS);
    auto kernel = words ? ply_rows_s2_kernel<true> : ply_rows_s2_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, block, lds, ctx->stream, (const PcvS2Chunk*)q->d_chunks, c0, c1, (const uint8_t*)q->cloud->d_xyz,
                       (const uint32_t*)q->d_flags, (const uint64_t*)q->d_offsets, cols, row0, nrows, tile, d_out);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

int check_range(const PlySource& s, uint64_t first_segment, uint64_t num_segments) {
  if (first_segment > s.nseg || num_segments > s.nseg - first_segment) return s.ctx->fail(PCV_E_INVALID, "segment range past the end");
  return PCV_OK;
}

int ply_rows(const PlySource& s, uint64_t first_segment, uint64_t num_segments, const char* const* attributes, uint32_t num_attributes,
             uint64_t capacity_bytes, int mem, void* out, uint32_t* stride_out, uint64_t* num_rows) {
  pcv_ctx* ctx = s.ctx;
  if (stride_out) *stride_out = 0;
  if (num_rows) *num_rows = 0;
  int rc;
  if ((rc = check_range(s, first_segment, num_segments))) return rc;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<PcvPlyColumn> cols;
  uint32_t stride = 0;
  PlyCols dev{};
  if ((rc = resolve_columns(s, attributes, num_attributes, &cols, &stride, &dev))) return rc;
  const uint64_t p0 = s.seg_off[first_segment], np = s.seg_off[first_segment + num_segments] - p0;
  if (stride_out) *stride_out = stride;
  if (num_rows) *num_rows = np;
  if (np > capacity_bytes / stride)
    return ctx->fail(PCV_E_INVALID, "the segments hold " + std::to_string(np) + " rows of " + std::to_string(stride) + " bytes, capacity is " +
                                        std::to_string(capacity_bytes) + " bytes");
  if (np == 0) return PCV_OK;
  if (!out) return ctx->fail(PCV_E_INVALID, "null output");
  const uint64_t c0 = s.seg_chunk[first_segment], c1 = s.seg_chunk[first_segment + num_segments];
  PcvScratch sc(ctx);
  uint8_t* d_out = (uint8_t*)out;
  if (mem == PCV_MEM_HOST && (rc = sc.get(&d_out, np * stride))) return rc;
  if ((rc = launch_rows(s, dev, c0, c1, p0, np, d_out))) return rc;
  if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, np * stride, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

// The pipeline of pcv_*_write_ply: the rows in pieces of at most `chunk_points`, cut at any row (the packer finds a piece's
// first chunk itself, so neither a segment of millions of points nor a chunk sets a piece's size); piece k + 1 is packed on
// the context's stream while piece k crosses to its pinned block on the side stream and piece k - 1 is written by the host
// threads. Device and pinned memory: two buffers of chunk_points * stride bytes each, whatever the result's size.
struct PlyPipe {
  pcv_ctx* ctx;
  hipEvent_t packed[2] = {}, copied[2] = {};
  bool made = false;
  explicit PlyPipe(pcv_ctx* c) : ctx(c) {}
  int make() {
    for (int k = 0; k < 2; ++k) {
      PCV_HIP_CHECK(ctx, hipEventCreateWithFlags(&packed[k], hipEventDisableTiming));
      PCV_HIP_CHECK(ctx, hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
    }
    made = true;
    return PCV_OK;
  }
  ~PlyPipe() {
    for (int k = 0; k < 2; ++k) {
      if (packed[k]) (void)hipEventDestroy(packed[k]);
      if (copied[k]) (void)hipEventDestroy(copied[k]);
    }
  }
};

int write_ply(const PlySource& s, uint64_t first_segment, uint64_t num_segments, const char* path, const pcv_ply_write_params* params,
              uint64_t* written) {
  pcv_ctx* ctx = s.ctx;
  if (written) *written = 0;
  if (!path || !params) return ctx->fail(PCV_E_INVALID, "null argument");
  if (params->struct_size < sizeof(pcv_ply_write_params)) return ctx->fail(PCV_E_INVALID, "pcv_ply_write_params.struct_size is too small");
  if (params->open_mode != PCV_PLY_TRUNCATE && params->open_mode != PCV_PLY_APPEND) return ctx->fail(PCV_E_INVALID, "bad open_mode");
  int rc;
  if ((rc = check_range(s, first_segment, num_segments))) return rc;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<PcvPlyColumn> cols;
  uint32_t stride = 0;
  PlyCols dev{};
  if ((rc = resolve_columns(s, params->attributes, params->num_attributes, &cols, &stride, &dev))) return rc;
  const uint64_t p0 = s.seg_off[first_segment], np = s.seg_off[first_segment + num_segments] - p0;
  PcvPlyFile file;
  std::string why;
  if ((rc = file.begin(path, params->open_mode == PCV_PLY_APPEND, cols, &why))) return ctx->fail(rc, why);
  if (np == 0) return PCV_OK;  // nothing written, no file (node_writer.rs:78-84); an appended file stays as it is
  const uint64_t c0 = s.seg_chunk[first_segment], c1 = s.seg_chunk[first_segment + num_segments];
  const uint64_t piece = std::min<uint64_t>(np, params->chunk_points ? params->chunk_points : kPlyDefaultChunkPoints);
  const uint64_t piece_bytes = ((piece * stride + 255) / 256) * 256;
  PcvScratch sc(ctx);
  uint8_t* d_buf[2];
  PlyPipe pipe(ctx);
  if ((rc = sc.get(&d_buf[0], piece_bytes)) || (rc = sc.get(&d_buf[1], piece_bytes)) || (rc = ctx->pinned_reserve(2 * piece_bytes)) || (rc = pipe.make()))
    return rc;
  uint8_t* h_buf[2] = {(uint8_t*)ctx->pinned, (uint8_t*)ctx->pinned + piece_bytes};
  if ((rc = file.open_for_rows(&why))) return ctx->fail(rc, why);
  const uint64_t npieces = (np + piece - 1) / piece;
  auto rows_of = [&](uint64_t k) { return std::min(piece, np - k * piece); };
  // the host's part for piece k: wait for its copy, then pwrite it in slices, one per host thread
  auto write_piece = [&](uint64_t k) -> int {
    const int b = (int)(k & 1);
    if (hipEventSynchronize(pipe.copied[b]) != hipSuccess) return ctx->fail(PCV_E_HIP, "copying PLY rows to the host failed");
    const uint64_t bytes = rows_of(k) * stride, at = k * piece * stride;
    const size_t workers = ctx->host_pool.threads.size() + 1;
    const uint64_t slice = std::max<uint64_t>(4u << 20, (bytes + workers - 1) / workers);
    const size_t parts = (size_t)((bytes + slice - 1) / slice);
    std::vector<int> part_rc(parts, PCV_OK);
    std::vector<std::string> part_why(parts);
    auto one = [&](size_t p) {
      const uint64_t lo = p * slice, len = std::min(slice, bytes - lo);
      part_rc[p] = file.write_at(at + lo, h_buf[b] + lo, len, &part_why[p]);
    };
    if (parts == 1) one(0);
    else ctx->host_pool.run(parts, one);
    for (size_t p = 0; p < parts; ++p)
      if (part_rc[p]) return ctx->fail(part_rc[p], part_why[p]);
    return PCV_OK;
  };
  auto run = [&]() -> int {
    for (uint64_t k = 0; k < npieces; ++k) {
      const int b = (int)(k & 1);
      // d_buf[b] was last read by the copy of piece k - 2, which write_piece(k - 2) has waited for; h_buf[b] likewise
      if (int r = launch_rows(s, dev, c0, c1, p0 + k * piece, rows_of(k), d_buf[b])) return r;
      PCV_HIP_CHECK(ctx, hipEventRecord(pipe.packed[b], ctx->stream));
      PCV_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->side, pipe.packed[b], 0));
      PCV_HIP_CHECK(ctx, hipMemcpyAsync(h_buf[b], d_buf[b], rows_of(k) * stride, hipMemcpyDeviceToHost, ctx->side));
      PCV_HIP_CHECK(ctx, hipEventRecord(pipe.copied[b], ctx->side));
      if (k > 0)
        if (int r = write_piece(k - 1)) return r;
    }
    return write_piece(npieces - 1);
  };
  rc = run();
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing queued may still write into what is freed here
    (void)hipStreamSynchronize(ctx->side);
    (void)hipGetLastError();
    file.abandon();
    return rc;
  }
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  if ((rc = file.commit(np, stride, &why))) return ctx->fail(rc, why);
  ctx->prof_resolve();
  if (written) *written = np;
  return PCV_OK;
}

}  // namespace

// pcv_internal.h: rows [row0, row0 + nrows) of the result's segments [first_segment, first_segment + num_segments) as 27-byte rows
// (x y z as doubles, then r g b) into d_out on the context's stream, nothing waited for — any row range, for callers that
// stream a result through a bounded buffer (pcv_terrain.hip). Exactly one of b / q is set.
int pcv_ply_pack_xyz_rgb(pcv_query_batch* b, pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, uint64_t row0, uint64_t nrows,
                         uint8_t* d_out) {
  const PlySource s = b ? source_of(b) : source_of(q);
  int rc;
  if ((rc = check_range(s, first_segment, num_segments))) return rc;
  const uint64_t p0 = s.seg_off[first_segment], p1 = s.seg_off[first_segment + num_segments];
  if (row0 < p0 || row0 > p1 || nrows > p1 - row0) return s.ctx->fail(PCV_E_INVALID, "row range outside the segments");
  if (nrows == 0) return PCV_OK;
  static const char* const kColor[] = {"color"};
  std::vector<PcvPlyColumn> cols;
  uint32_t stride = 0;
  PlyCols dev{};
  if ((rc = resolve_columns(s, kColor, 1, &cols, &stride, &dev))) return rc;
  if (stride != kPcvXyzRgbRowBytes) return s.ctx->fail(PCV_E_INVALID, "unexpected row layout");
  return launch_rows(s, dev, s.seg_chunk[first_segment], s.seg_chunk[first_segment + num_segments], row0, nrows, d_out);
}

extern "C" int pcv_query_batch_ply_rows(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const char* const* attributes,
                                        uint32_t num_attributes, uint64_t capacity_bytes, int mem, void* out, uint32_t* stride,
                                        uint64_t* num_rows) {
  if (!b) return PCV_E_INVALID;
  return ply_rows(source_of(b), first_segment, num_segments, attributes, num_attributes, capacity_bytes, mem, out, stride, num_rows);
}

extern "C" int pcv_s2_query_ply_rows(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const char* const* attributes,
                                     uint32_t num_attributes, uint64_t capacity_bytes, int mem, void* out, uint32_t* stride, uint64_t* num_rows) {
  if (!q) return PCV_E_INVALID;
  return ply_rows(source_of(q), first_segment, num_segments, attributes, num_attributes, capacity_bytes, mem, out, stride, num_rows);
}

extern "C" int pcv_query_batch_write_ply(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const char* path,
                                         const pcv_ply_write_params* params, uint64_t* written) {
  if (!b) return PCV_E_INVALID;
  return write_ply(source_of(b), first_segment, num_segments, path, params, written);
}

extern "C" int pcv_s2_query_write_ply(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const char* path,
                                      const pcv_ply_write_params* params, uint64_t* written) {
  if (!q) return PCV_E_INVALID;
  return write_ply(source_of(q), first_segment, num_segments, path, params, written);
}

// ---- the format's host-only entry points (pcv_ply_write.cpp) -----------------------------------------------------------------
extern "C" int pcv_ply_layout_host(const char* const* names, const int32_t* data_types, uint32_t n, uint32_t* offsets, uint32_t* stride) {
  std::vector<PcvPlyColumn> cols;
  std::string why;
  uint32_t s = 0;
  if (pcv_ply_columns(names, data_types, n, &cols, &s, &why)) return pcv_host_fail(PCV_E_INVALID, why);
  for (const PcvPlyColumn& c : cols)
    if (offsets) offsets[c.given] = c.offset;
  if (stride) *stride = s;
  return PCV_OK;
}

extern "C" int pcv_ply_header_host(const char* const* names, const int32_t* data_types, uint32_t n, uint64_t count, char* buf, uint64_t cap,
                                   uint64_t* len) {
  std::vector<PcvPlyColumn> cols;
  std::string why;
  if (pcv_ply_columns(names, data_types, n, &cols, nullptr, &why)) return pcv_host_fail(PCV_E_INVALID, why);
  const std::string h = pcv_ply_header(cols, count);
  if (len) *len = h.size();
  if (buf && cap) std::memcpy(buf, h.data(), (size_t)std::min<uint64_t>(cap, h.size()));
  return PCV_OK;
}

extern "C" int pcv_ply_append_check_host(const char* path, const char* const* names, const int32_t* data_types, uint32_t n, uint64_t* old_count) {
  if (old_count) *old_count = 0;
  std::vector<PcvPlyColumn> cols;
  std::string why;
  if (pcv_ply_columns(names, data_types, n, &cols, nullptr, &why)) return pcv_host_fail(PCV_E_INVALID, why);
  uint64_t count = 0, size = 0;
  if (int rc = pcv_ply_append_check(path, cols, &count, &size, &why)) return pcv_host_fail(rc, why);
  if (old_count) *old_count = count;
  return PCV_OK;
}
