// pcv_ply_rows.hip — the result of a batched point query as the rows of a binary PLY: packed on the device from
// the query's own tables, returned as they are (pcv_query_batch_ply_rows, pcv_s2_query_ply_rows) or streamed into a file
// through two device buffers and two pinned blocks (pcv_query_batch_write_ply, pcv_s2_query_write_ply). The format itself —
// columns, header, append — is host code in pcv_ply_write.cpp; its three host-only entry points are at the end of this file.
//
// A row is the transpose of what the device holds: position as three doubles, then the attribute columns ascending by name,
// packed without padding, so a stride is 24 + anything and a workgroup's byte range starts at any alignment. Tiles, walks and
// the store are those of pcv_rows_dev.h, the source, the piece pipeline and the slice writer those of pcv_result_rows.h; what is
// this file's is the row itself (put64, put_columns), which columns a result has, and the PLY file around the rows.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "pcv_internal.h"
#include "pcv_ply_write.h"
#include "pcv_result_rows.h"
#include "pcv_rows_dev.h"

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

// Rows [row0 + blockIdx.x * tile_rows, ...) of the octree batch, `nrows` from row0 on, to out + (row - row0) * stride. The chunks
// [c0, c1) are those of the caller's segment range; chunk_off their scanned kept counts (the row of a chunk's first kept point).
template <bool WORDS>
__global__ __launch_bounds__(256) void ply_rows_octree_kernel(const ChunkDesc* __restrict__ desc, uint64_t c0, uint64_t c1,
                                                               const uint8_t* __restrict__ xyz_blob, const uint8_t* __restrict__ keep,
                                                               const uint64_t* __restrict__ chunk_off, PlyCols cols, uint64_t row0,
                                                               uint64_t nrows, uint32_t tile_rows, uint8_t* __restrict__ out) {
  const PcvRowsTile t = pcv_rows_tile(row0, nrows, tile_rows, cols.stride, out);
  pcv_walk_octree_rows(desc, c0, c1, xyz_blob, keep, chunk_off, t.g0, t.g1,
                       [&](bool mine, const PointsView& v, uint32_t q, uint64_t attr_index, uint32_t row_in_tile) {
                         if (!mine) return;
                         const V3d p = load_point(v, q);
                         uint8_t* row = ply_image + t.phase + row_in_tile * cols.stride;
                         put64<WORDS>(row, 0, (uint64_t)__double_as_longlong(p.x));
                         put64<WORDS>(row, 8, (uint64_t)__double_as_longlong(p.y));
                         put64<WORDS>(row, 16, (uint64_t)__double_as_longlong(p.z));
                         put_columns<WORDS>(row, cols, attr_index);
                       });
  __syncthreads();
  pcv_store_image(ply_image, t.dst, t.phase, t.rows * cols.stride);
}

// The same over an S2 query: u32 flags and a scanned offset per candidate, positions copied as the 24 bytes they are. The walk
// is this kernel's own lane-strided loop, not pcv_walk_s2_rows: nothing here needs every lane in every step, and in that form
// the kernel measured 0.4 % slower over rows with three extras (profiles/result_rows_refactor.md).
template <bool WORDS>
__global__ __launch_bounds__(256) void ply_rows_s2_kernel(const PcvS2Chunk* __restrict__ chunks, uint64_t c0, uint64_t c1,
                                                           const uint8_t* __restrict__ xyz, const uint32_t* __restrict__ flags,
                                                           const uint64_t* __restrict__ offsets, PlyCols cols, uint64_t row0, uint64_t nrows,
                                                           uint32_t tile_rows, uint8_t* __restrict__ out) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const PcvRowsTile t = pcv_rows_tile(row0, nrows, tile_rows, cols.stride, out);
  const uint64_t first = pcv_chunk_of_row(c0, c1, t.g0, [&](uint64_t c) { return offsets[chunks[c].first]; });
  for (uint64_t ci = first + wave; ci < c1; ci += 4) {
    const PcvS2Chunk c = chunks[ci];
    if (offsets[c.first] >= t.g1) break;
    if (offsets[c.first + c.count] <= t.g0) continue;
    for (uint32_t q = lane; q < c.count; q += 64) {
      if (!flags[c.first + q]) continue;
      const uint64_t pos = offsets[c.first + q];
      if (pos < t.g0 || pos >= t.g1) continue;
      const uint64_t i = c.src + q;
      const uint64_t* p = reinterpret_cast<const uint64_t*>(xyz) + 3 * i;
      uint8_t* row = ply_image + t.phase + (uint32_t)(pos - t.g0) * cols.stride;
      put64<WORDS>(row, 0, p[0]);
      put64<WORDS>(row, 8, p[1]);
      put64<WORDS>(row, 16, p[2]);
      put_columns<WORDS>(row, cols, i);
    }
  }
  __syncthreads();
  pcv_store_image(ply_image, t.dst, t.phase, t.rows * cols.stride);
}

// ---- what the two kinds of result share on the host -------------------------------------------------------------------------
// `attributes` (NULL: every attribute the cloud has) as the sorted columns of a row and their device sources. Loads the named
// extras of a cloud opened from a directory, and only those.
int resolve_columns(const PcvResultSource& s, const char* const* attributes, uint32_t num_attributes, std::vector<PcvPlyColumn>* cols, uint32_t* stride,
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
int launch_rows(const PcvResultSource& s, const PlyCols& cols, uint64_t c0, uint64_t c1, uint64_t row0, uint64_t nrows, uint8_t* d_out) {
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

int ply_rows(const PcvResultSource& s, uint64_t first_segment, uint64_t num_segments, const char* const* attributes, uint32_t num_attributes,
             uint64_t capacity_bytes, int mem, void* out, uint32_t* stride_out, uint64_t* num_rows) {
  pcv_ctx* ctx = s.ctx;
  if (stride_out) *stride_out = 0;
  if (num_rows) *num_rows = 0;
  int rc;
  if ((rc = s.check_range(first_segment, num_segments))) return rc;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<PcvPlyColumn> cols;
  uint32_t stride = 0;
  PlyCols dev{};
  if ((rc = resolve_columns(s, attributes, num_attributes, &cols, &stride, &dev))) return rc;
  const auto [p0, np, c0, c1] = s.rows_of_segments(first_segment, num_segments);
  if (stride_out) *stride_out = stride;
  if (num_rows) *num_rows = np;
  if (np > capacity_bytes / stride)
    return ctx->fail(PCV_E_INVALID, "the segments hold " + std::to_string(np) + " rows of " + std::to_string(stride) + " bytes, capacity is " +
                                        std::to_string(capacity_bytes) + " bytes");
  if (np == 0) return PCV_OK;
  if (!out) return ctx->fail(PCV_E_INVALID, "null output");
  PcvScratch sc(ctx);
  uint8_t* d_out = (uint8_t*)out;
  if (mem == PCV_MEM_HOST && (rc = sc.get(&d_out, np * stride))) return rc;
  if ((rc = launch_rows(s, dev, c0, c1, p0, np, d_out))) return rc;
  if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, np * stride, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

// pcv_*_write_ply: the rows through the piece pipeline in pieces of at most `chunk_points`, cut at any row (the packer finds a
// piece's first chunk itself, so neither a segment of millions of points nor a chunk sets a piece's size).
int write_ply(const PcvResultSource& s, uint64_t first_segment, uint64_t num_segments, const char* path, const pcv_ply_write_params* params,
              uint64_t* written) {
  pcv_ctx* ctx = s.ctx;
  if (written) *written = 0;
  if (!path || !params) return ctx->fail(PCV_E_INVALID, "null argument");
  if (params->struct_size < sizeof(pcv_ply_write_params)) return ctx->fail(PCV_E_INVALID, "pcv_ply_write_params.struct_size is too small");
  if (params->open_mode != PCV_PLY_TRUNCATE && params->open_mode != PCV_PLY_APPEND) return ctx->fail(PCV_E_INVALID, "bad open_mode");
  int rc;
  if ((rc = s.check_range(first_segment, num_segments))) return rc;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  std::vector<PcvPlyColumn> cols;
  uint32_t stride = 0;
  PlyCols dev{};
  if ((rc = resolve_columns(s, params->attributes, params->num_attributes, &cols, &stride, &dev))) return rc;
  const PcvResultSource::Rows r = s.rows_of_segments(first_segment, num_segments);
  const uint64_t np = r.np;
  PcvPlyFile file;
  std::string why;
  if ((rc = file.begin(path, params->open_mode == PCV_PLY_APPEND, cols, &why))) return ctx->fail(rc, why);
  if (np == 0) return PCV_OK;  // nothing written, no file (node_writer.rs:78-84); an appended file stays as it is
  const uint64_t piece = std::min<uint64_t>(np, params->chunk_points ? params->chunk_points : kPlyDefaultChunkPoints);
  const uint64_t piece_bytes = ((piece * stride + 255) / 256) * 256;
  PcvScratch sc(ctx);
  uint8_t* d_buf[2];
  PcvPiecePipe pipe;
  if ((rc = sc.get(&d_buf[0], piece_bytes)) || (rc = sc.get(&d_buf[1], piece_bytes)) || (rc = ctx->pinned_reserve(2 * piece_bytes)) ||
      (rc = pipe.make(ctx)))
    return rc;
  uint8_t* h_buf[2] = {(uint8_t*)ctx->pinned, (uint8_t*)ctx->pinned + piece_bytes};
  if ((rc = file.open_for_rows(&why))) return ctx->fail(rc, why);
  auto rows_of = [&](uint64_t k) { return std::min(piece, np - k * piece); };
  rc = pcv_run_pieces(
      ctx, pipe, (np + piece - 1) / piece, [&](uint64_t k, int b) { return launch_rows(s, dev, r.c0, r.c1, r.p0 + k * piece, rows_of(k), d_buf[b]); },
      [&](uint64_t k) { return rows_of(k) * stride; }, d_buf, h_buf,
      [&](uint64_t k, int b) -> int {
        if (hipEventSynchronize(pipe.copied[b]) != hipSuccess) return ctx->fail(PCV_E_HIP, "copying PLY rows to the host failed");
        const uint64_t at = k * piece * stride;
        return pcv_write_slices(ctx, rows_of(k) * stride,
                                [&](uint64_t lo, uint64_t len, std::string* w) { return file.write_at(at + lo, h_buf[b] + lo, len, w); });
      });
  if (rc != PCV_OK) {
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

// pcv_result_rows.h
int pcv_ply_pack_xyz_rgb(const PcvResultSource& s, uint64_t first_segment, uint64_t num_segments, uint64_t row0, uint64_t nrows, uint8_t* d_out) {
  int rc;
  if ((rc = s.check_range(first_segment, num_segments))) return rc;
  const auto [p0, np, c0, c1] = s.rows_of_segments(first_segment, num_segments);
  if (row0 < p0 || row0 > p0 + np || nrows > p0 + np - row0) return s.ctx->fail(PCV_E_INVALID, "row range outside the segments");
  if (nrows == 0) return PCV_OK;
  static const char* const kColor[] = {"color"};
  std::vector<PcvPlyColumn> cols;
  uint32_t stride = 0;
  PlyCols dev{};
  if ((rc = resolve_columns(s, kColor, 1, &cols, &stride, &dev))) return rc;
  if (stride != kPcvXyzRgbRowBytes) return s.ctx->fail(PCV_E_INVALID, "unexpected row layout");
  return launch_rows(s, dev, c0, c1, row0, nrows, d_out);
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
