// pcv_s2.hip — S2 cell clouds: what S2Splitter::write (reference src/read_write/s2.rs:60-115) leaves on disk, built on the
// device from one batch of ECEF points, and CellUnion::contains per point. The chain is pcv_s2_dev.h.
//
//   ids      s2_ids_kernel: one thread per point — validity, cell id at the split level; the first invalid index by atomicMin
//   regroup  radix sort of a copy of the ids (pcv_sort.hip, the bits that vary only) -> distinct cells and their first slots
//            (count / scan / write over tiles of 2 048 keys) -> every point's dense cell rank by binary search -> the stable
//            pair sort of (rank, input index) over ceil(log2(cells)) bits: the permutation "by cell, input order inside"
//   gather   s2_gather_kernel: xyz as 24-byte AoS f64, rgb, intensity into cell-contiguous blobs that stay on the device
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "pcv_internal.h"
#include "pcv_s2_dev.h"
#include "pcv_s2_obj.h"

int pcv_s2_cloud::fail(int code, const std::string& msg) const { return ctx ? ctx->fail(code, msg) : pcv_host_fail(code, msg); }

namespace {

constexpr uint32_t kNoInvalid = 0xffffffffu;
constexpr int kTileKeys = 2048;  // keys per workgroup of the unique kernels: 256 lanes x 8 consecutive keys
constexpr uint32_t kMaxGrid = 1u << 16;

inline uint32_t grid_for(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + 255) / 256, kMaxGrid); }

// ---- ids ----------------------------------------------------------------------------------------------------------------
template <bool kValidate>
__global__ __launch_bounds__(256) void s2_ids_kernel(uint64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                      const double* __restrict__ z, uint32_t level, uint64_t* __restrict__ ids,
                                                      uint32_t* __restrict__ first_invalid) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const double px = x[i], py = y[i], pz = z[i];
    if (kValidate && !s2::valid_ecef(px, py, pz)) atomicMin(first_invalid, (uint32_t)i);
    ids[i] = s2::parent(s2::leaf_from_point(px, py, pz), level);
  }
}

__global__ __launch_bounds__(256) void s2_union_kernel(uint64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                        const double* __restrict__ z, const uint64_t* __restrict__ cells,
                                                        uint32_t num_cells, uint8_t* __restrict__ keep) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride)
    keep[i] = s2::union_contains(cells, num_cells, s2::leaf_from_point(x[i], y[i], z[i])) ? 1 : 0;
}

// ---- distinct cells from the sorted ids ---------------------------------------------------------------------------------
// exclusive scan of one value per lane over a workgroup of NT lanes; *total = the workgroup's sum
template <int NT>
__device__ inline uint32_t block_scan_exclusive(uint32_t v, uint32_t* wave_sums /* NT / 64 words of LDS */, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_sums[wave] = inc;
  __syncthreads();
  uint32_t base = 0, sum = 0;
  for (int w = 0; w < NT / 64; ++w) {
    const uint32_t s = wave_sums[w];
    if (w < wave) base += s;
    sum += s;
  }
  __syncthreads();  // the caller may use wave_sums again
  *total = sum;
  return base + inc - v;
}

// heads among the 8 keys of this lane: bit k set = key (first + k) starts a run
__device__ inline uint32_t lane_heads(const uint64_t* __restrict__ sorted, uint64_t n, uint64_t first, uint64_t* keys) {
  uint32_t heads = 0;
  uint64_t prev = first > 0 && first <= n ? sorted[first - 1] : 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint64_t i = first + (uint64_t)k;
    if (i < n) {
      const uint64_t key = sorted[i];
      keys[k] = key;
      if (i == 0 || key != prev) heads |= 1u << k;
      prev = key;
    }
  }
  return heads;
}

__global__ __launch_bounds__(256) void s2_unique_count_kernel(const uint64_t* __restrict__ sorted, uint64_t n,
                                                               uint32_t* __restrict__ tile_counts) {
  __shared__ uint32_t wave_sums[4];
  uint64_t keys[8];
  const uint64_t first = (uint64_t)blockIdx.x * kTileKeys + (uint64_t)threadIdx.x * 8u;
  const uint32_t heads = lane_heads(sorted, n, first, keys);
  uint32_t total;
  (void)block_scan_exclusive<256>((uint32_t)__popc(heads), wave_sums, &total);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// one workgroup: exclusive scan of the tile counts in place, the sum into *total
__global__ __launch_bounds__(1024) void s2_unique_scan_kernel(uint32_t* __restrict__ tile_counts, uint32_t tiles,
                                                               uint32_t* __restrict__ total) {
  __shared__ uint32_t wave_sums[16];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < tiles; base += 1024u) {
    const uint32_t at = base + threadIdx.x;
    const uint32_t v = at < tiles ? tile_counts[at] : 0u;
    uint32_t sum;
    const uint32_t ex = block_scan_exclusive<1024>(v, wave_sums, &sum);
    if (at < tiles) tile_counts[at] = carry + ex;
    carry += sum;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void s2_unique_kernel(const uint64_t* __restrict__ sorted, uint64_t n,
                                                         const uint32_t* __restrict__ tile_offsets, uint32_t num_cells,
                                                         uint64_t* __restrict__ cell_ids, uint32_t* __restrict__ cell_first) {
  __shared__ uint32_t wave_sums[4];
  uint64_t keys[8];
  const uint64_t first = (uint64_t)blockIdx.x * kTileKeys + (uint64_t)threadIdx.x * 8u;
  const uint32_t heads = lane_heads(sorted, n, first, keys);
  uint32_t total;
  uint32_t at = tile_offsets[blockIdx.x] + block_scan_exclusive<256>((uint32_t)__popc(heads), wave_sums, &total);
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((heads >> k) & 1u) {
      if (at < num_cells) {  // (always: the counts come from the same keys)
        cell_ids[at] = keys[k];
        cell_first[at] = (uint32_t)(first + (uint64_t)k);
      }
      ++at;
    }
}

__global__ __launch_bounds__(256) void s2_rank_kernel(uint64_t n, const uint64_t* __restrict__ ids, const uint64_t* __restrict__ cell_ids,
                                                       uint32_t num_cells, uint32_t* __restrict__ rank, uint32_t* __restrict__ index) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    const uint32_t r = s2::lower_bound(cell_ids, num_cells, ids[i]);
    rank[i] = r < num_cells ? r : num_cells - 1u;  // (every id is in the list)
    index[i] = (uint32_t)i;
  }
}

// ---- gather -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void s2_gather_kernel(uint64_t n, const uint32_t* __restrict__ order, const double* __restrict__ x,
                                                         const double* __restrict__ y, const double* __restrict__ z,
                                                         const uint8_t* __restrict__ color, uint32_t color_stride,
                                                         const float* __restrict__ intensity, uint32_t* __restrict__ order_out,
                                                         double* __restrict__ xyz, uint8_t* __restrict__ rgb, float* __restrict__ inten) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < n; s += stride) {
    const uint32_t src = order[s];
    if (order_out) order_out[s] = src;  // (null: a part of a directory stream, which keeps no input order)
    xyz[3 * s + 0] = x[src];
    xyz[3 * s + 1] = y[src];
    xyz[3 * s + 2] = z[src];
    const uint8_t* c = color + (uint64_t)src * color_stride;
    rgb[3 * s + 0] = c[0];
    rgb[3 * s + 1] = c[1];
    rgb[3 * s + 2] = c[2];
    if (intensity) inten[s] = intensity[src];
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
struct DevCloud {
  uint64_t n = 0;
  const double *x = nullptr, *y = nullptr, *z = nullptr;
  const uint8_t* color = nullptr;
  uint32_t color_stride = 3;
  const float* intensity = nullptr;
};

int check_points(pcv_ctx* ctx, const pcv_points* p, bool need_color) {
  if (!p) return ctx->fail(PCV_E_INVALID, "points is null");
  if (p->mem != PCV_MEM_HOST && p->mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "points.mem must be PCV_MEM_HOST or PCV_MEM_DEVICE");
  if (p->n >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "an S2 call takes fewer than 2^32 - 1 points; split the input");
  if (p->n > 0 && (!p->x || !p->y || !p->z)) return ctx->fail(PCV_E_INVALID, "x/y/z must be non-null");
  if (need_color) {
    if (p->n > 0 && !p->color) return ctx->fail(PCV_E_INVALID, "color is required");
    if (p->color_stride != 3 && p->color_stride != 4) return ctx->fail(PCV_E_INVALID, "color_stride must be 3 or 4");
  }
  return PCV_OK;
}

int stage(pcv_ctx* ctx, PcvScratch& sc, const pcv_points* p, bool with_attrs, DevCloud* d) {
  d->n = p->n;
  d->color_stride = p->color_stride;
  if (p->mem == PCV_MEM_DEVICE || p->n == 0) {
    d->x = p->x, d->y = p->y, d->z = p->z;
    d->color = p->color;
    d->intensity = p->intensity;
    return PCV_OK;
  }
  double *x, *y, *z;
  int rc;
  if ((rc = sc.get(&x, p->n)) || (rc = sc.get(&y, p->n)) || (rc = sc.get(&z, p->n))) return rc;
  if ((rc = ctx->h2d(x, p->x, p->n * 8)) || (rc = ctx->h2d(y, p->y, p->n * 8)) || (rc = ctx->h2d(z, p->z, p->n * 8))) return rc;
  d->x = x, d->y = y, d->z = z;
  if (with_attrs) {
    uint8_t* c;
    if ((rc = sc.get(&c, p->n * p->color_stride)) || (rc = ctx->h2d(c, p->color, p->n * p->color_stride))) return rc;
    d->color = c;
    if (p->intensity) {
      float* f;
      if ((rc = sc.get(&f, p->n)) || (rc = ctx->h2d(f, p->intensity, p->n * 4))) return rc;
      d->intensity = f;
    }
  }
  return PCV_OK;
}

// the exact min / max of the points into out6 (device), by pcv_aabb_reduce's kernel (its vector loads want 16-byte bases)
int launch_bbox(pcv_ctx* ctx, PcvScratch& sc, const DevCloud& d, double* out6) {
  double* partial;
  int rc = sc.get(&partial, (size_t)2048 * 6 + 6);
  if (rc) return rc;
  const double *x = d.x, *y = d.y, *z = d.z;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)z) & 15) {
    double *cx, *cy, *cz;
    if ((rc = sc.get(&cx, d.n)) || (rc = sc.get(&cy, d.n)) || (rc = sc.get(&cz, d.n))) return rc;
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(cx, x, d.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(cy, y, d.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(cz, z, d.n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    x = cx, y = cy, z = cz;
  }
  pcv_launch_aabb(ctx, d.n, x, y, z, partial, out6);
  PCV_HIP_CHECK(ctx, hipGetLastError());
  return PCV_OK;
}

void release_cloud(pcv_s2_cloud* c) {
  if (!c) return;
  if (c->ctx) {
    (void)hipSetDevice(c->ctx->device);
    if (c->d_order) c->ctx->dev_free(c->d_order);
    if (c->d_xyz) c->ctx->dev_free(c->d_xyz);
    if (c->d_rgb) c->ctx->dev_free(c->d_rgb);
    if (c->d_int) c->ctx->dev_free(c->d_int);
    if (c->d_ids) c->ctx->dev_free(c->d_ids);
    if (c->d_table) c->ctx->dev_free(c->d_table);
    pcv_s2_extras_release(c);
  }
  delete c;
}

// an opened cloud's cell files, read and uploaded on first use (as an opened octree's node files are)
int ensure_resident(pcv_s2_cloud* c) {
  if (c->resident) return PCV_OK;
  pcv_ctx* ctx = c->ctx;
  if (c->n) {
    PcvS2Dir meta;
    meta.ids = c->ids, meta.counts = c->counts, meta.has_intensity = c->has_intensity;
    std::vector<uint8_t> xyz, rgb, inten;
    try {
      xyz.resize(c->n * 24);
      rgb.resize(c->n * 3);
      if (c->has_intensity) inten.resize(c->n * 4);
    } catch (...) {
      return c->fail(PCV_E_OOM, "no host memory for the cell files of " + c->directory);
    }
    std::string error;
    int rc = pcv_s2_read_cells(c->directory.c_str(), meta, xyz.data(), rgb.data(), c->has_intensity ? inten.data() : nullptr, &error);
    if (rc != PCV_OK) return c->fail(rc, error);
    if (!ctx) {  // host only: the blobs stay where they are
      c->h_xyz.swap(xyz), c->h_rgb.swap(rgb), c->h_int.swap(inten);
      c->resident = true;
      return PCV_OK;
    }
    PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint8_t *d_xyz = nullptr, *d_rgb = nullptr, *d_int = nullptr;
    if ((rc = ctx->dev_alloc((void**)&d_xyz, c->n * 24)) == PCV_OK && (rc = ctx->dev_alloc((void**)&d_rgb, c->n * 3)) == PCV_OK && c->has_intensity)
      rc = ctx->dev_alloc((void**)&d_int, c->n * 4);
    if (rc == PCV_OK && (rc = ctx->h2d(d_xyz, xyz.data(), c->n * 24)) == PCV_OK && (rc = ctx->h2d(d_rgb, rgb.data(), c->n * 3)) == PCV_OK && d_int)
      rc = ctx->h2d(d_int, inten.data(), c->n * 4);
    if (rc == PCV_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "uploading the cell files failed");
    if (rc != PCV_OK) {
      (void)hipStreamSynchronize(ctx->stream);
      if (d_xyz) ctx->dev_free(d_xyz);
      if (d_rgb) ctx->dev_free(d_rgb);
      if (d_int) ctx->dev_free(d_int);
      return rc;
    }
    c->d_xyz = d_xyz, c->d_rgb = d_rgb, c->d_int = d_int;
  }
  c->resident = true;
  return PCV_OK;
}

int split_impl(pcv_ctx* ctx, const pcv_points* points, uint32_t level, pcv_s2_cloud* c, bool with_order = true,
               std::vector<PcvS2Extra>* extras = nullptr) {
  const uint64_t n = points->n;
  c->ctx = ctx;
  c->n = n;
  c->level = level;
  c->has_intensity = points->intensity != nullptr;
  if (extras) c->extras.swap(*extras);  // names and types hold for a cloud without points too
  if (n == 0) return PCV_OK;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  PcvScratch sc(ctx);
  DevCloud d;
  int rc;
  if ((rc = stage(ctx, sc, points, true, &d))) return rc;

  // ---- ids, validity, bounding box ----
  uint64_t* ids;
  uint32_t* d_words;  // [0] first invalid index, [1] number of cells
  double* d_box;
  if ((rc = sc.get(&ids, n)) || (rc = sc.get(&d_words, 4)) || (rc = sc.get(&d_box, 6))) return rc;
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_words, 0xff, 16, st));
  {
    PcvProf prof(ctx, PCV_K_S2_IDS);
    hipLaunchKernelGGL(s2_ids_kernel<true>, dim3(grid_for(n)), dim3(256), 0, st, n, d.x, d.y, d.z, level, ids, d_words);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if ((rc = launch_bbox(ctx, sc, d, d_box))) return rc;
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox, d_box, 48, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox + 6, d_words, 8, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const uint32_t first_invalid = (uint32_t)(ctx->mailbox[6] & 0xffffffffull);
  if (first_invalid != kNoInvalid) {  // s2.rs:64-71, the first one in input order
    double p[3];
    if (points->mem == PCV_MEM_HOST) {
      p[0] = points->x[first_invalid], p[1] = points->y[first_invalid], p[2] = points->z[first_invalid];
    } else {
      PCV_HIP_CHECK(ctx, hipMemcpy(&p[0], d.x + first_invalid, 8, hipMemcpyDeviceToHost));
      PCV_HIP_CHECK(ctx, hipMemcpy(&p[1], d.y + first_invalid, 8, hipMemcpyDeviceToHost));
      PCV_HIP_CHECK(ctx, hipMemcpy(&p[2], d.z + first_invalid, 8, hipMemcpyDeviceToHost));
    }
    char msg[256];
    snprintf(msg, sizeof(msg), "Point (%.17g, %.17g, %.17g) at index %u is not a valid ECEF point", p[0], p[1], p[2], first_invalid);
    return ctx->fail(PCV_E_INVALID, msg);
  }
  std::memcpy(c->bbox_min, ctx->mailbox, 24);
  std::memcpy(c->bbox_max, ctx->mailbox + 3, 24);

  // ---- regroup: sorted copy of the ids -> distinct cells ----
  uint64_t *keys_a, *keys_b;
  void* sort_scratch;
  uint32_t* tile_counts;
  const uint32_t tiles = (uint32_t)((n + kTileKeys - 1) / kTileKeys);
  if ((rc = sc.get(&keys_a, n)) || (rc = sc.get(&keys_b, n)) || (rc = sc.get(&tile_counts, tiles))) return rc;
  if ((rc = ctx->dev_alloc(&sort_scratch, pcv_sort_scratch_bytes(n)))) return rc;
  sc.ptrs.push_back(sort_scratch);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(keys_a, ids, n * 8, hipMemcpyDeviceToDevice, st));
  PcvSortPayload none;
  bool in_a = true;
  // a cell id of level L: the face and 2 L bits of position above the marker bit 2 (30 - L); nothing below varies
  if ((rc = pcv_radix_sort_u64(ctx, keys_a, keys_b, n, 2 * (s2::kMaxLevel - (int)level) + 1, 64, &none, sort_scratch, &in_a))) return rc;
  const uint64_t* sorted = in_a ? keys_a : keys_b;
  {
    PcvProf prof(ctx, PCV_K_S2_UNIQUE);
    hipLaunchKernelGGL(s2_unique_count_kernel, dim3(tiles), dim3(256), 0, st, sorted, n, tile_counts);
    hipLaunchKernelGGL(s2_unique_scan_kernel, dim3(1), dim3(1024), 0, st, tile_counts, tiles, d_words + 1);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(ctx->mailbox + 6, d_words, 8, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  const uint32_t cells = (uint32_t)(ctx->mailbox[6] >> 32);
  if (cells == 0 || (uint64_t)cells > n) return ctx->fail(PCV_E_HIP, "the cell count of the sorted ids is out of range");
  uint64_t* d_cell_ids;
  uint32_t* d_cell_first;
  if ((rc = sc.get(&d_cell_ids, cells)) || (rc = sc.get(&d_cell_first, cells))) return rc;
  {
    PcvProf prof(ctx, PCV_K_S2_UNIQUE);
    hipLaunchKernelGGL(s2_unique_kernel, dim3(tiles), dim3(256), 0, st, sorted, n, tile_counts, cells, d_cell_ids, d_cell_first);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  c->ids.resize(cells);
  std::vector<uint32_t> first(cells);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(c->ids.data(), d_cell_ids, (size_t)cells * 8, hipMemcpyDeviceToHost, st));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(first.data(), d_cell_first, (size_t)cells * 4, hipMemcpyDeviceToHost, st));

  // ---- regroup: dense ranks, the stable pair sort (the sorted keys are done with: their buffers hold the pairs) ----
  uint32_t *rank_a = (uint32_t*)keys_a, *index_a = rank_a + n, *rank_b = (uint32_t*)keys_b, *index_b = rank_b + n;
  {
    PcvProf prof(ctx, PCV_K_S2_RANK);
    hipLaunchKernelGGL(s2_rank_kernel, dim3(grid_for(n)), dim3(256), 0, st, n, ids, d_cell_ids, cells, rank_a, index_a);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  int bits = 0;
  while (bits < 32 && (1ull << bits) < (uint64_t)cells) ++bits;
  PcvSortPayload pairs;
  pairs.nwords = 1;
  pairs.in[0] = index_a;
  pairs.out[0] = index_b;
  if ((rc = pcv_radix_sort_u32(ctx, rank_a, rank_b, n, 0, bits, &pairs, sort_scratch, &in_a))) return rc;
  const uint32_t* order = in_a ? index_a : index_b;

  // ---- gather ----
  if ((with_order && (rc = ctx->dev_alloc((void**)&c->d_order, n * 4))) || (rc = ctx->dev_alloc((void**)&c->d_xyz, n * 24)) ||
      (rc = ctx->dev_alloc((void**)&c->d_rgb, n * 3)) || (c->has_intensity && (rc = ctx->dev_alloc((void**)&c->d_int, n * 4))))
    return rc;
  {
    PcvProf prof(ctx, PCV_K_S2_GATHER);
    hipLaunchKernelGGL(s2_gather_kernel, dim3(grid_for(n)), dim3(256), 0, st, n, order, d.x, d.y, d.z, d.color, d.color_stride, d.intensity,
                       c->d_order, (double*)c->d_xyz, c->d_rgb, (float*)c->d_int);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  // the extras: one launch each over the same permutation, in pcv_s2_attr.hip
  if (!c->extras.empty() && (rc = pcv_s2_attr_gather(ctx, sc, order, n, points->mem, c))) return rc;
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(st));
  ctx->prof_resolve();
  c->offsets.resize(cells);
  c->counts.resize(cells);
  for (uint32_t k = 0; k < cells; ++k) {
    c->offsets[k] = first[k];
    c->counts[k] = (k + 1 < cells ? (uint64_t)first[k + 1] : n) - (uint64_t)first[k];
  }
  return PCV_OK;
}

}  // namespace

int pcv_s2_check_union(const uint64_t* cells, uint32_t num_cells, std::string* why) {
  if (num_cells && !cells) {
    *why = "cells is null";
    return PCV_E_INVALID;
  }
  for (uint32_t k = 0; k < num_cells; ++k) {
    if (cells[k] == 0) {
      *why = "cell " + std::to_string(k) + " of the union is 0, which is no cell id";
      return PCV_E_INVALID;
    }
    if (k > 0 && cells[k] < cells[k - 1]) {
      *why = "the cells of a union must ascend by id: cell " + std::to_string(k) + " is below its predecessor";
      return PCV_E_INVALID;
    }
  }
  return PCV_OK;
}

int pcv_s2_make_resident(pcv_s2_cloud* c) { return ensure_resident(c); }

// pcv_s2_split as a stream takes it (pcv_s2_stream.hip): the same checks, the same split, the slot -> input index plane on request
int pcv_s2_split_part(pcv_ctx* ctx, const pcv_points* points, uint32_t level, bool with_order, pcv_s2_cloud** out,
                      std::vector<PcvS2Extra>* extras) {
  *out = nullptr;
  int rc = check_points(ctx, points, true);
  if (rc) return rc;
  pcv_s2_cloud* c = new pcv_s2_cloud();
  rc = split_impl(ctx, points, level, c, with_order, extras);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing queued still reads what is released now
    release_cloud(c);
    return rc;
  }
  *out = c;
  return PCV_OK;
}
void pcv_s2_release(pcv_s2_cloud* c) { release_cloud(c); }

// ---- host twins (no context) --------------------------------------------------------------------------------------------
extern "C" int pcv_s2_cell_ids_host(uint64_t n, const double* x, const double* y, const double* z, uint32_t level, uint64_t* ids) {
  if (level > (uint32_t)s2::kMaxLevel) return pcv_host_fail(PCV_E_INVALID, "an S2 level is 0 ..= 30");
  if (n && (!x || !y || !z || !ids)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n; ++i) ids[i] = s2::parent(s2::leaf_from_point(x[i], y[i], z[i]), level);
  return PCV_OK;
}

extern "C" int pcv_s2_cell_token(uint64_t id, char out[17]) {
  if (!out) return PCV_E_INVALID;
  const std::string t = pcv_s2_token(id);
  std::memcpy(out, t.c_str(), t.size() + 1);
  return PCV_OK;
}

extern "C" int pcv_s2_union_contains_host(const uint64_t* cells, uint32_t num_cells, uint64_t n, const double* x, const double* y,
                                          const double* z, uint8_t* keep) {
  std::string why;
  if (pcv_s2_check_union(cells, num_cells, &why)) return pcv_host_fail(PCV_E_INVALID, why);
  if (n && (!x || !y || !z || !keep)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  for (uint64_t i = 0; i < n; ++i) keep[i] = s2::union_contains(cells, num_cells, s2::leaf_from_point(x[i], y[i], z[i])) ? 1 : 0;
  return PCV_OK;
}

// ---- device entry points ------------------------------------------------------------------------------------------------
extern "C" int pcv_s2_cell_ids(pcv_ctx* ctx, const pcv_points* points, uint32_t level, uint64_t* ids, int mem) {
  if (!ctx) return PCV_E_INVALID;
  int rc = check_points(ctx, points, false);
  if (rc) return rc;
  if (level > (uint32_t)s2::kMaxLevel) return ctx->fail(PCV_E_INVALID, "an S2 level is 0 ..= 30");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  const uint64_t n = points->n;
  if (n == 0) return PCV_OK;
  if (!ids) return ctx->fail(PCV_E_INVALID, "ids is null");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  DevCloud d;
  if ((rc = stage(ctx, sc, points, false, &d))) return rc;
  uint64_t* d_ids = ids;
  if (mem == PCV_MEM_HOST && (rc = sc.get(&d_ids, n))) return rc;
  {
    PcvProf prof(ctx, PCV_K_S2_IDS);
    hipLaunchKernelGGL(s2_ids_kernel<false>, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, d.x, d.y, d.z, level, d_ids, (uint32_t*)nullptr);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipMemcpyAsync(ids, d_ids, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_s2_union_contains(pcv_ctx* ctx, const uint64_t* cells, uint32_t num_cells, const pcv_points* points, uint8_t* keep,
                                     int mem) {
  if (!ctx) return PCV_E_INVALID;
  int rc = check_points(ctx, points, false);
  if (rc) return rc;
  std::string why;
  if (pcv_s2_check_union(cells, num_cells, &why)) return ctx->fail(PCV_E_INVALID, why);
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  const uint64_t n = points->n;
  if (n == 0) return PCV_OK;
  if (!keep) return ctx->fail(PCV_E_INVALID, "keep is null");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  DevCloud d;
  if ((rc = stage(ctx, sc, points, false, &d))) return rc;
  uint64_t* d_cells;
  if ((rc = sc.get(&d_cells, (size_t)num_cells + 1))) return rc;
  if (num_cells) PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_cells, cells, (size_t)num_cells * 8, hipMemcpyHostToDevice, ctx->stream));
  uint8_t* d_keep = keep;
  if (mem == PCV_MEM_HOST && (rc = sc.get(&d_keep, n))) return rc;
  {
    PcvProf prof(ctx, PCV_K_S2_UNION);
    hipLaunchKernelGGL(s2_union_kernel, dim3(grid_for(n)), dim3(256), 0, ctx->stream, n, d.x, d.y, d.z, d_cells, num_cells, d_keep);
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipMemcpyAsync(keep, d_keep, n, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (also: `cells` may be the caller's pageable memory)
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_s2_split(pcv_ctx* ctx, const pcv_points* points, uint32_t split_level, pcv_s2_cloud** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  int rc = check_points(ctx, points, true);
  if (rc) return rc;
  if (split_level > (uint32_t)s2::kMaxLevel) return ctx->fail(PCV_E_INVALID, "an S2 split level is 0 ..= 30");
  pcv_s2_cloud* c = new pcv_s2_cloud();
  rc = split_impl(ctx, points, split_level, c);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing queued still reads what is released now
    release_cloud(c);
    return rc;
  }
  *out = c;
  return PCV_OK;
}

// S2Cells::from_data_provider (src/s2_cells/mod.rs:199-212) over a directory
extern "C" int pcv_s2_open_dir(pcv_ctx* ctx, const char* directory, pcv_s2_cloud** out) {
  auto fail = [&](int code, const std::string& m) { return ctx ? ctx->fail(code, m) : pcv_host_fail(code, m); };
  if (!directory || !out) return fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  PcvS2Dir meta;
  std::string error;
  const int rc = pcv_s2_read_meta(directory, &meta, &error);
  if (rc != PCV_OK) return fail(rc, error);
  pcv_s2_cloud* c = new pcv_s2_cloud();
  c->ctx = ctx;
  c->directory = directory;
  c->opened = true;
  c->has_intensity = meta.has_intensity;
  for (const auto& a : meta.extras) {  // their files are read when a call first names them (pcv_s2_extra_resident)
    PcvS2Extra e;
    e.name = a.first, e.data_type = a.second, e.elem = pcv_s2_attr_size(a.second), e.resident = false;
    c->extras.push_back(std::move(e));
  }
  std::memcpy(c->bbox_min, meta.bbox_min, 24);
  std::memcpy(c->bbox_max, meta.bbox_max, 24);
  c->ids = meta.ids;
  c->counts = meta.counts;
  c->offsets.resize(c->ids.size());
  c->level = 0xffffffffu;  // the common level of the ids; 0xffffffff when they differ (legal for the reader) or there are none
  for (size_t k = 0; k < c->ids.size(); ++k) {
    c->offsets[k] = c->n;
    c->n += c->counts[k];
    const uint64_t id = c->ids[k];
    const uint32_t tz = id ? (uint32_t)__builtin_ctzll(id) : 1u;
    const uint32_t level = (tz & 1u) || tz > 60u ? 0xffffffffu : (uint32_t)s2::kMaxLevel - (tz >> 1);
    if (k == 0) c->level = level;
    else if (c->level != level) c->level = 0xffffffffu;
  }
  c->resident = c->n == 0;
  for (PcvS2Extra& e : c->extras) e.resident = c->n == 0;
  *out = c;
  return PCV_OK;
}

extern "C" int pcv_s2_info(const pcv_s2_cloud* c, uint64_t* num_cells, uint64_t* num_points, double bbox_min[3], double bbox_max[3],
                           int* has_intensity, uint32_t* level) {
  if (!c) return PCV_E_INVALID;
  if (num_cells) *num_cells = c->ids.size();
  if (num_points) *num_points = c->n;
  for (int a = 0; a < 3; ++a) {
    if (bbox_min) bbox_min[a] = c->bbox_min[a];
    if (bbox_max) bbox_max[a] = c->bbox_max[a];
  }
  if (has_intensity) *has_intensity = c->has_intensity ? 1 : 0;
  if (level) *level = c->level;
  return PCV_OK;
}

extern "C" int pcv_s2_cells(const pcv_s2_cloud* c, uint64_t* ids, uint64_t* counts, uint64_t* offsets) {
  if (!c) return PCV_E_INVALID;
  const size_t bytes = c->ids.size() * 8;
  if (bytes) {
    if (ids) std::memcpy(ids, c->ids.data(), bytes);
    if (counts) std::memcpy(counts, c->counts.data(), bytes);
    if (offsets) std::memcpy(offsets, c->offsets.data(), bytes);
  }
  return PCV_OK;
}

extern "C" int pcv_s2_order(pcv_s2_cloud* c, uint32_t* input_index, int mem) {
  if (!c) return PCV_E_INVALID;
  if (c->opened) return c->fail(PCV_E_INVALID, "an S2 cell cloud opened from a directory has no input order");
  pcv_ctx* ctx = c->ctx;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (c->n == 0) return PCV_OK;
  if (!input_index) return ctx->fail(PCV_E_INVALID, "input_index is null");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(input_index, c->d_order, c->n * 4, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                    ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_s2_cell_points(pcv_s2_cloud* c, uint64_t first_cell, uint64_t num_cells, uint64_t capacity, int mem, double* xyz,
                                  uint8_t* rgb, float* intensity) {
  if (!c) return PCV_E_INVALID;
  pcv_ctx* ctx = c->ctx;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return c->fail(PCV_E_INVALID, "bad mem");
  if (!ctx && mem != PCV_MEM_HOST) return c->fail(PCV_E_INVALID, "a cloud opened without a context serves host memory only");
  const uint64_t cells = c->ids.size();
  if (first_cell > cells || num_cells > cells - first_cell) return c->fail(PCV_E_INVALID, "cell range past the end");
  if (num_cells == 0) return PCV_OK;
  const uint64_t begin = c->offsets[first_cell];
  const uint64_t end = first_cell + num_cells < cells ? c->offsets[first_cell + num_cells] : c->n;
  const uint64_t count = end - begin;
  if (count > capacity) return c->fail(PCV_E_INVALID, "the cells hold " + std::to_string(count) + " points, capacity is " + std::to_string(capacity));
  if (intensity && !c->has_intensity) return c->fail(PCV_E_INVALID, "this S2 cell cloud has no intensity attribute");
  if (int rc = ensure_resident(c)) return rc;
  if (!ctx) {
    if (xyz && count) std::memcpy(xyz, c->h_xyz.data() + begin * 24, count * 24);
    if (rgb && count) std::memcpy(rgb, c->h_rgb.data() + begin * 3, count * 3);
    if (intensity && count) std::memcpy(intensity, c->h_int.data() + begin * 4, count * 4);
    return PCV_OK;
  }
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const hipMemcpyKind kind = mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (xyz) PCV_HIP_CHECK(ctx, hipMemcpyAsync(xyz, c->d_xyz + begin * 24, count * 24, kind, ctx->stream));
  if (rgb) PCV_HIP_CHECK(ctx, hipMemcpyAsync(rgb, c->d_rgb + begin * 3, count * 3, kind, ctx->stream));
  if (intensity) PCV_HIP_CHECK(ctx, hipMemcpyAsync(intensity, c->d_int + begin * 4, count * 4, kind, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_s2_write_dir(pcv_s2_cloud* c, const char* directory) {
  if (!c) return PCV_E_INVALID;
  pcv_ctx* ctx = c->ctx;
  if (!directory) return c->fail(PCV_E_INVALID, "directory is null");
  uint8_t *h_xyz = nullptr, *h_rgb = nullptr, *h_int = nullptr;
  int rc = ensure_resident(c);
  if (rc != PCV_OK) return rc;
  // the extras' files first, meta.pb — which lists them — last, as before
  std::vector<std::pair<std::string, int32_t>> extras;
  if (!c->extras.empty() && (rc = pcv_s2_attr_write(c, directory, nullptr, &extras)) != PCV_OK) return rc;
  if (!ctx) {
    std::string error;
    rc = pcv_s2_write_files(directory, c->bbox_min, c->bbox_max, c->ids.size(), c->ids.data(), c->counts.data(), c->offsets.data(),
                            c->h_xyz.data(), c->h_rgb.data(), c->has_intensity ? (c->n ? c->h_int.data() : (const uint8_t*)"") : nullptr, &error,
                            &extras);
    return rc == PCV_OK ? rc : c->fail(rc, error);
  }
  if (c->n) {
    PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((rc = ctx->host_alloc((void**)&h_xyz, c->n * 24)) == PCV_OK && (rc = ctx->host_alloc((void**)&h_rgb, c->n * 3)) == PCV_OK &&
        c->has_intensity)
      rc = ctx->host_alloc((void**)&h_int, c->n * 4);
    if (rc == PCV_OK && (hipMemcpyAsync(h_xyz, c->d_xyz, c->n * 24, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         hipMemcpyAsync(h_rgb, c->d_rgb, c->n * 3, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         (h_int && hipMemcpyAsync(h_int, c->d_int, c->n * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
                         hipStreamSynchronize(ctx->stream) != hipSuccess))
      rc = ctx->fail(PCV_E_HIP, "downloading the cell blobs failed");
  }
  if (rc == PCV_OK) {
    std::string error;
    rc = pcv_s2_write_files(directory, c->bbox_min, c->bbox_max, c->ids.size(), c->ids.data(), c->counts.data(), c->offsets.data(), h_xyz,
                            h_rgb, c->has_intensity ? (h_int ? h_int : (const uint8_t*)"") : nullptr, &error, &extras);
    if (rc != PCV_OK) ctx->fail(rc, error);
  }
  if (h_xyz) ctx->host_release(h_xyz);
  if (h_rgb) ctx->host_release(h_rgb);
  if (h_int) ctx->host_release(h_int);
  return rc;
}

extern "C" void pcv_s2_free(pcv_s2_cloud* c) {
  if (c && c->ctx) (void)hipStreamSynchronize(c->ctx->stream);
  release_cloud(c);
}
