// pcv_s2_attr.hip — the typed extra attributes of an S2 cell cloud (DESIGN §9c the write side, §9d the read side): S2Splitter::write regroups every attribute
// of a batch (reference src/read_write/s2.rs:85-107), get_meta lists them (s2.rs:139-173), a PointQuery filters on any scalar
// one (src/iterator.rs:66-119). `color` and `intensity` stay in the kernels of pcv_s2.hip / pcv_s2_stream.hip /
// pcv_s2_points.hip, which this file leaves as they are: an extra runs in launches of its own, one column at a time.
//
//   gather   s2_attr_gather_kernel<W, C>: out[s] = in[order[s]], one lane per output word, grid-stride
//   merge    s2_attr_merge_kernel<W, C>: one workgroup per output chunk of the merge plan; (part, slot) per point as
//            s2_merge_kernel derives them, then the chunk's words, consecutive lanes on consecutive words
//   filter   s2_attr_filter_kernel<T>: flags[candidate] &= keep(col[point], lo, hi) over the chunks whose location filters
//   points   s2_attr_gather_points_kernel<W, C>: the kept elements of a segment range to offsets[candidate] - base
// Element-granular gathers read scattered and write in order; no rate is promised for them.
#include <algorithm>
#include <cstring>

#include "pcv_internal.h"
#include "pcv_s2_attr_dev.h"
#include "pcv_s2_merge_plan.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_query_dev.h"

namespace {

constexpr uint32_t kMaxGrid = 1u << 16;
constexpr uint32_t kMergeLdsSegments = 1024;  // as s2_merge_kernel stages them

struct FilterIval {  // per location: the interval of the extra being filtered (unused rows are never read)
  double lo, hi;
};

// ---- kernels ------------------------------------------------------------------------------------------------------------
template <typename W, int C>
__global__ __launch_bounds__(256) void s2_attr_gather_kernel(uint64_t n, const uint32_t* __restrict__ order, const W* __restrict__ in,
                                                              W* __restrict__ out) {
  const uint64_t words = n * (uint64_t)C, stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t e = (uint64_t)blockIdx.x * 256u + threadIdx.x; e < words; e += stride) {
    const uint64_t s = e / (uint64_t)C;
    const uint32_t c = (uint32_t)(e - s * (uint64_t)C);
    out[e] = in[(uint64_t)order[s] * (uint64_t)C + c];
  }
}

// One workgroup per output chunk, as s2_merge_kernel: every output word has one writer, decided by the plan.
template <typename W, int C>
__global__ __launch_bounds__(256) void s2_attr_merge_kernel(uint64_t n, uint64_t num_segments, uint64_t num_chunks,
                                                             const uint64_t* __restrict__ seg_dst, const pcv_s2_merge_segment* __restrict__ segs,
                                                             const uint64_t* __restrict__ chunk_first, const W* const* __restrict__ cols,
                                                             W* __restrict__ out) {
  __shared__ uint64_t s_dst[kMergeLdsSegments];
  __shared__ uint32_t s_part[kMergeChunkPoints];
  __shared__ uint32_t s_src[kMergeChunkPoints];
  const uint64_t chunk = blockIdx.x;
  const uint64_t begin = chunk * kMergeChunkPoints;
  if (chunk >= num_chunks || begin >= n) return;
  const uint32_t m = (uint32_t)(n - begin < (uint64_t)kMergeChunkPoints ? n - begin : (uint64_t)kMergeChunkPoints);
  const uint64_t lo = chunk_first[chunk];
  const uint64_t hi = chunk + 1 < num_chunks ? chunk_first[chunk + 1] : num_segments - 1;
  const uint64_t span = hi - lo + 1;
  const bool staged = span <= (uint64_t)kMergeLdsSegments;
  if (staged)
    for (uint32_t i = threadIdx.x; i < (uint32_t)span; i += 256u) s_dst[i] = seg_dst[lo + i];
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < m; j += 256u) {
    const uint64_t dst = begin + j;
    uint64_t a = 0, b = span - 1;  // the last segment of the range that starts at or before dst
    while (a < b) {
      const uint64_t mid = (a + b + 1) >> 1;
      const uint64_t at = staged ? s_dst[mid] : seg_dst[lo + mid];
      if (at <= dst) a = mid;
      else b = mid - 1;
    }
    const pcv_s2_merge_segment sg = segs[lo + a];
    s_part[j] = sg.part;
    s_src[j] = (uint32_t)(sg.src_offset + (dst - sg.dst_offset));
  }
  __syncthreads();
  W* o = out + begin * (uint64_t)C;
  for (uint32_t e = threadIdx.x; e < (uint32_t)C * m; e += 256u) {
    const uint32_t p = e / (uint32_t)C, c = e - (uint32_t)C * p;
    o[e] = cols[s_part[p]][(uint64_t)s_src[p] * (uint64_t)C + c];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void s2_attr_filter_kernel(const PcvS2Chunk* __restrict__ chunks, const uint32_t* __restrict__ which,
                                                              const FilterIval* __restrict__ ivals, const T* __restrict__ col,
                                                              uint32_t* __restrict__ flags) {
  const PcvS2Chunk c = chunks[which[blockIdx.x]];
  const FilterIval iv = ivals[c.location];
  for (uint32_t q = threadIdx.x; q < c.count; q += 256u) {
    const bool k = s2attr::keep<T>(col[c.src + q], iv.lo, iv.hi);
    flags[c.first + q] &= k ? 1u : 0u;
  }
}

template <typename W, int C>
__global__ __launch_bounds__(256) void s2_attr_gather_points_kernel(const PcvS2Chunk* __restrict__ chunks, uint64_t first_chunk,
                                                                     const uint32_t* __restrict__ flags, const uint64_t* __restrict__ offsets,
                                                                     uint64_t base, const W* __restrict__ col, W* __restrict__ out) {
  const PcvS2Chunk c = chunks[first_chunk + blockIdx.x];
  for (uint32_t q = threadIdx.x; q < c.count; q += 256u) {
    if (!flags[c.first + q]) continue;
    const uint64_t i = c.src + q, o = offsets[c.first + q] - base;
#pragma unroll
    for (int k = 0; k < C; ++k) out[o * (uint64_t)C + k] = col[i * (uint64_t)C + k];
  }
}

// f(W{}, integral_constant<int, C>) for the (word, components) form of a data type
template <typename F>
void dispatch_form(int32_t t, F&& f) {
  if (t == s2attr::U8Vec3) return f(uint8_t{}, std::integral_constant<int, 3>{});
  if (t == s2attr::F64Vec3) return f(uint64_t{}, std::integral_constant<int, 3>{});
  switch (s2attr::element_size(t)) {
    case 1: return f(uint8_t{}, std::integral_constant<int, 1>{});
    case 2: return f(uint16_t{}, std::integral_constant<int, 1>{});
    case 4: return f(uint32_t{}, std::integral_constant<int, 1>{});
    default: return f(uint64_t{}, std::integral_constant<int, 1>{});
  }
}

inline uint32_t grid_for(uint64_t work) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((work + 255) / 256, 1), kMaxGrid); }

bool aligned_for(int32_t t, const void* p) { return ((uintptr_t)p & (uintptr_t)(s2attr::word_size(t) - 1u)) == 0; }

std::string not_found(const char* name) { return std::string("Data type for attribute '") + (name ? name : "") + "' not found."; }  // lib.rs:94

}  // namespace

// ---- vocabulary ---------------------------------------------------------------------------------------------------------
uint32_t pcv_s2_attr_size(int32_t data_type) { return s2attr::element_size(data_type); }

bool pcv_s2_attr_name_ok(const std::string& name, std::string* why) {
  static const char* const kReserved[] = {"color", "intensity", "position", "xyz", "rgb", "meta"};
  if (name.empty()) {
    *why = "an attribute's name may not be empty";
    return false;
  }
  if (name.size() > PCV_S2_MAX_ATTR_NAME) {
    *why = "attribute '" + name.substr(0, PCV_S2_MAX_ATTR_NAME) + "...': a name is " + std::to_string(PCV_S2_MAX_ATTR_NAME) + " bytes at most";
    return false;
  }
  for (const char* r : kReserved)
    if (name == r) {
      *why = "attribute '" + name + "': the name is reserved";
      return false;
    }
  for (char ch : name)
    if (ch == '/' || ch == '.' || ch == '\0') {
      *why = "attribute '" + name + "': a name may not contain '/', '.' or NUL (it is the extension of the cells' files)";
      return false;
    }
  return true;
}

int pcv_s2_attr_check(const pcv_attribute* attrs, uint32_t num_attrs, uint64_t n, std::vector<PcvS2Extra>* out, std::string* why) {
  out->clear();
  if (num_attrs == 0) return PCV_OK;
  if (!attrs) {
    *why = "attrs is null";
    return PCV_E_INVALID;
  }
  if (num_attrs > PCV_S2_MAX_EXTRAS) {
    *why = "a cloud holds " + std::to_string(PCV_S2_MAX_EXTRAS) + " extra attributes at most, got " + std::to_string(num_attrs);
    return PCV_E_INVALID;
  }
  for (uint32_t k = 0; k < num_attrs; ++k) {
    const pcv_attribute& a = attrs[k];
    if (!a.name) {
      *why = "attribute " + std::to_string(k) + " has no name";
      return PCV_E_INVALID;
    }
    const std::string name(a.name);
    if (!pcv_s2_attr_name_ok(name, why)) return PCV_E_INVALID;
    PcvS2Extra e;
    e.name = name;
    e.data_type = a.data_type;
    e.elem = s2attr::element_size(a.data_type);
    if (e.elem == 0) {
      *why = "Attribute data type invalid (attribute '" + name + "', data type " + std::to_string(a.data_type) + ")";
      return PCV_E_INVALID;
    }
    if (n > 0 && !a.data) {
      *why = "attribute '" + name + "': data is null";
      return PCV_E_INVALID;
    }
    e.src = a.data;
    for (const PcvS2Extra& o : *out)
      if (o.name == name) {
        *why = "attribute '" + name + "' is given twice";
        return PCV_E_INVALID;
      }
    out->push_back(std::move(e));
  }
  std::sort(out->begin(), out->end(), [](const PcvS2Extra& a, const PcvS2Extra& b) { return a.name < b.name; });
  return PCV_OK;
}

// ---- split --------------------------------------------------------------------------------------------------------------
int pcv_s2_attr_gather(pcv_ctx* ctx, PcvScratch& sc, const uint32_t* order, uint64_t n, int mem, pcv_s2_cloud* c) {
  for (PcvS2Extra& e : c->extras) {
    int rc;
    const uint8_t* in = (const uint8_t*)e.src;
    if (mem == PCV_MEM_HOST) {  // staged through scratch, as colour is
      uint8_t* staged;
      if ((rc = sc.get(&staged, n * e.elem)) || (rc = ctx->h2d(staged, e.src, n * e.elem))) return rc;
      in = staged;
    } else if (!aligned_for(e.data_type, in)) {
      return ctx->fail(PCV_E_INVALID, "attribute '" + e.name + "': device data must be aligned to its element's words");
    }
    if ((rc = ctx->dev_alloc((void**)&e.d, n * e.elem))) return rc;
    {
      PcvProf prof(ctx, PCV_K_S2_ATTR_GATHER);
      dispatch_form(e.data_type, [&](auto w, auto comps) {
        using W = decltype(w);
        constexpr int C = decltype(comps)::value;
        hipLaunchKernelGGL((s2_attr_gather_kernel<W, C>), dim3(grid_for(n * C)), dim3(256), 0, ctx->stream, n, order, (const W*)in, (W*)e.d);
      });
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    e.src = nullptr;
  }
  return PCV_OK;
}

// ---- merge --------------------------------------------------------------------------------------------------------------
int pcv_s2_attr_merge(pcv_ctx* ctx, PcvScratch& sc, uint64_t n, uint64_t num_segments, uint64_t num_chunks, const uint64_t* d_seg_dst,
                      const pcv_s2_merge_segment* d_segs, const uint64_t* d_chunk_first, const std::vector<pcv_s2_cloud*>& parts,
                      pcv_s2_cloud* out) {
  if (parts.empty()) return PCV_OK;
  const size_t num_extras = parts[0]->extras.size();
  out->extras.clear();
  for (size_t k = 0; k < num_extras; ++k) {
    const PcvS2Extra& e0 = parts[0]->extras[k];
    PcvS2Extra e;
    e.name = e0.name, e.data_type = e0.data_type, e.elem = e0.elem;
    out->extras.push_back(std::move(e));
  }
  if (n == 0 || num_extras == 0) return PCV_OK;
  std::vector<const uint8_t*> table(parts.size() * num_extras);
  for (size_t k = 0; k < num_extras; ++k)
    for (size_t p = 0; p < parts.size(); ++p) {
      const pcv_s2_cloud* part = parts[p];
      if (part->extras.size() != num_extras || part->extras[k].name != out->extras[k].name || part->extras[k].data_type != out->extras[k].data_type)
        return ctx->fail(PCV_E_HIP, "the parts of the stream disagree on attribute " + out->extras[k].name);
      table[k * parts.size() + p] = part->extras[k].d;
    }
  const uint8_t** d_table;
  int rc;
  if ((rc = sc.get(&d_table, table.size())) || (rc = ctx->h2d(d_table, table.data(), table.size() * sizeof(void*)))) return rc;
  for (size_t k = 0; k < num_extras; ++k) {
    PcvS2Extra& e = out->extras[k];
    if ((rc = ctx->dev_alloc((void**)&e.d, n * e.elem))) return rc;
    {
      PcvProf prof(ctx, PCV_K_S2_ATTR_MERGE);
      dispatch_form(e.data_type, [&](auto w, auto comps) {
        using W = decltype(w);
        constexpr int C = decltype(comps)::value;
        hipLaunchKernelGGL((s2_attr_merge_kernel<W, C>), dim3((uint32_t)num_chunks), dim3(256), 0, ctx->stream, n, num_segments, num_chunks,
                           d_seg_dst, d_segs, d_chunk_first, (const W* const*)(d_table + k * parts.size()), (W*)e.d);
      });
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  // `table` is a host vector of this scope: the upload has to be over before it goes
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

// ---- residency of an opened cloud's extras ------------------------------------------------------------------------------
int pcv_s2_extra_resident(pcv_s2_cloud* c, size_t k, bool* absent) {
  PcvS2Extra& e = c->extras[k];
  if (absent) *absent = false;
  if (e.resident) return PCV_OK;
  pcv_ctx* ctx = c->ctx;
  if (c->n) {
    std::vector<uint8_t> col;
    try {
      col.resize(c->n * e.elem);
    } catch (...) {
      return c->fail(PCV_E_OOM, "no host memory for the ." + e.name + " files of " + c->directory);
    }
    std::string error;
    int rc = pcv_s2_read_extra(c->directory.c_str(), c->ids, c->counts, e.name, e.elem, col.data(), &error, absent);
    if (rc != PCV_OK) return c->fail(rc, error);
    if (!ctx) {
      e.h.swap(col);
    } else {
      PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
      uint8_t* d = nullptr;
      if ((rc = ctx->dev_alloc((void**)&d, c->n * e.elem)) == PCV_OK) rc = ctx->h2d(d, col.data(), c->n * e.elem);
      if (rc == PCV_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = ctx->fail(PCV_E_HIP, "uploading the ." + e.name + " files failed");
      if (rc != PCV_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        if (d) ctx->dev_free(d);
        return rc;
      }
      e.d = d;
    }
  }
  e.resident = true;
  return PCV_OK;
}

void pcv_s2_extras_release(pcv_s2_cloud* c) {
  for (PcvS2Extra& e : c->extras)
    if (e.d && c->ctx) c->ctx->dev_free(e.d), e.d = nullptr;
}

std::vector<std::pair<std::string, int32_t>> pcv_s2_extra_list(const pcv_s2_cloud* c) {
  std::vector<std::pair<std::string, int32_t>> list;
  for (const PcvS2Extra& e : c->extras) list.emplace_back(e.name, e.data_type);
  return list;
}

// every extra's runs onto the cells' `<token>.<name>` files (pcv_s2_write_dir, a stream's flush)
int pcv_s2_attr_write(pcv_s2_cloud* c, const char* directory, const uint8_t* truncate, std::vector<std::pair<std::string, int32_t>>* written) {
  pcv_ctx* ctx = c->ctx;
  for (size_t k = 0; k < c->extras.size(); ++k) {
    bool absent;
    int rc = pcv_s2_extra_resident(c, k, &absent);
    if (rc != PCV_OK && absent) continue;  // meta.pb names an attribute the directory has no file of: nothing to carry over
    if (rc != PCV_OK) return rc;
    PcvS2Extra& e = c->extras[k];
    if (written) written->emplace_back(e.name, e.data_type);
    std::string error;
    if (!ctx || c->n == 0) {
      rc = pcv_s2_write_extra(directory, c->ids.size(), c->ids.data(), c->counts.data(), c->offsets.data(), truncate, e.name, e.elem,
                              c->n ? e.h.data() : nullptr, &error);
      if (rc != PCV_OK) return c->fail(rc, error);
      continue;
    }
    PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint8_t* h = nullptr;
    if ((rc = ctx->host_alloc((void**)&h, c->n * e.elem)) != PCV_OK) return rc;
    if (hipMemcpyAsync(h, e.d, c->n * e.elem, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      rc = ctx->fail(PCV_E_HIP, "downloading attribute " + e.name + " failed");
    if (rc == PCV_OK) {
      rc = pcv_s2_write_extra(directory, c->ids.size(), c->ids.data(), c->counts.data(), c->offsets.data(), truncate, e.name, e.elem, h, &error);
      if (rc != PCV_OK) ctx->fail(rc, error);
    }
    ctx->host_release(h);
    if (rc != PCV_OK) return rc;
  }
  return PCV_OK;
}

// ---- query: filter launches between the flags and the scan (pcv_s2_points.hip) ------------------------------------------
int pcv_s2_attr_filter(pcv_ctx* ctx, PcvScratch& sc, pcv_s2_cloud* c, const PcvS2Chunk* d_chunks, const std::vector<PcvS2Chunk>& chunks,
                       uint64_t locations, const std::vector<PcvS2ExtraFilter>& filters, uint32_t* d_flags) {
  std::vector<int> distinct;
  for (const PcvS2ExtraFilter& f : filters)
    if (std::find(distinct.begin(), distinct.end(), f.extra) == distinct.end()) distinct.push_back(f.extra);
  std::sort(distinct.begin(), distinct.end());
  for (int extra : distinct) {
    int rc = pcv_s2_extra_resident(c, (size_t)extra);
    if (rc != PCV_OK) return rc;
    const PcvS2Extra& e = c->extras[(size_t)extra];
    std::vector<FilterIval> ivals(locations, FilterIval{0.0, 0.0});
    std::vector<uint8_t> used(locations, 0);
    for (const PcvS2ExtraFilter& f : filters) {
      if (f.extra != extra) continue;
      if (f.location == kPcvS2EveryLocation) {  // the table filled uniformly: every chunk of the call takes the launch
        std::fill(ivals.begin(), ivals.end(), FilterIval{f.lo, f.hi});
        std::fill(used.begin(), used.end(), (uint8_t)1);
      } else {
        ivals[f.location] = FilterIval{f.lo, f.hi}, used[f.location] = 1;
      }
    }
    std::vector<uint32_t> which;
    for (size_t k = 0; k < chunks.size(); ++k)
      if (used[chunks[k].location]) which.push_back((uint32_t)k);
    if (which.empty()) continue;
    FilterIval* d_ivals;
    uint32_t* d_which;
    if ((rc = sc.get(&d_ivals, locations)) || (rc = sc.get(&d_which, which.size())) || (rc = ctx->h2d(d_ivals, ivals.data(), locations * sizeof(FilterIval))) ||
        (rc = ctx->h2d(d_which, which.data(), which.size() * 4)))
      return rc;
    {
      PcvProf prof(ctx, PCV_K_S2_ATTR_FILTER);
      s2attr::dispatch_scalar(e.data_type, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(s2_attr_filter_kernel<T>, dim3((uint32_t)which.size()), dim3(256), 0, ctx->stream, d_chunks, d_which, d_ivals,
                           (const T*)e.d, d_flags);
      });
    }
    PCV_HIP_CHECK(ctx, hipGetLastError());
    PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (ivals / which are host vectors of this iteration)
  }
  return PCV_OK;
}

// ---- entry points -------------------------------------------------------------------------------------------------------
extern "C" int pcv_s2_split_ex(pcv_ctx* ctx, const pcv_points* points, const pcv_attribute* attrs, uint32_t num_attrs, uint32_t split_level,
                               pcv_s2_cloud** out) {
  if (num_attrs == 0) return pcv_s2_split(ctx, points, split_level, out);
  if (!ctx) return PCV_E_INVALID;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  *out = nullptr;
  if (!points) return ctx->fail(PCV_E_INVALID, "points is null");
  if (split_level > 30u) return ctx->fail(PCV_E_INVALID, "an S2 split level is 0 ..= 30");
  std::vector<PcvS2Extra> extras;
  std::string why;
  if (pcv_s2_attr_check(attrs, num_attrs, points->n, &extras, &why)) return ctx->fail(PCV_E_INVALID, why);
  return pcv_s2_split_part(ctx, points, split_level, true, out, &extras);
}

extern "C" int pcv_s2_attributes_check_host(const pcv_attribute* attrs, uint32_t num_attrs) {
  std::vector<PcvS2Extra> extras;
  std::string why;
  if (pcv_s2_attr_check(attrs, num_attrs, 0, &extras, &why)) return pcv_host_fail(PCV_E_INVALID, why);
  return PCV_OK;
}

extern "C" int pcv_s2_attributes(const pcv_s2_cloud* c, uint32_t* count, const char** names, int32_t* data_types) {
  if (!c) return PCV_E_INVALID;
  if (count) *count = (uint32_t)c->extras.size();
  for (size_t k = 0; k < c->extras.size(); ++k) {
    if (names) names[k] = c->extras[k].name.c_str();
    if (data_types) data_types[k] = c->extras[k].data_type;
  }
  return PCV_OK;
}

extern "C" int pcv_s2_cell_attribute(pcv_s2_cloud* c, const char* name, uint64_t first_cell, uint64_t num_cells, uint64_t capacity, int mem,
                                     void* out) {
  if (!c) return PCV_E_INVALID;
  pcv_ctx* ctx = c->ctx;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return c->fail(PCV_E_INVALID, "bad mem");
  if (!ctx && mem != PCV_MEM_HOST) return c->fail(PCV_E_INVALID, "a cloud opened without a context serves host memory only");
  const int k = c->find_extra(name);
  if (k < 0) return c->fail(PCV_E_INVALID, not_found(name));
  const uint64_t cells = c->ids.size();
  if (first_cell > cells || num_cells > cells - first_cell) return c->fail(PCV_E_INVALID, "cell range past the end");
  if (num_cells == 0) return PCV_OK;
  const uint64_t begin = c->offsets[first_cell];
  const uint64_t end = first_cell + num_cells < cells ? c->offsets[first_cell + num_cells] : c->n;
  const uint64_t count = end - begin;
  if (count > capacity) return c->fail(PCV_E_INVALID, "the cells hold " + std::to_string(count) + " points, capacity is " + std::to_string(capacity));
  if (int rc = pcv_s2_extra_resident(c, (size_t)k)) return rc;
  if (count == 0) return PCV_OK;
  if (!out) return c->fail(PCV_E_INVALID, "out is null");
  const PcvS2Extra& e = c->extras[(size_t)k];
  if (!ctx) {
    std::memcpy(out, e.h.data() + begin * e.elem, count * e.elem);
    return PCV_OK;
  }
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, e.d + begin * e.elem, count * e.elem, mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                    ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_s2_query_attribute(pcv_s2_query* b, const char* name, uint64_t first_segment, uint64_t num_segments, uint64_t capacity,
                                      int mem, void* out) {
  if (!b) return PCV_E_INVALID;
  pcv_s2_cloud* c = b->cloud;
  pcv_ctx* ctx = c->ctx;
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  const int k = c->find_extra(name);
  if (k < 0) return ctx->fail(PCV_E_INVALID, not_found(name));
  if (first_segment > b->nseg || num_segments > b->nseg - first_segment) return ctx->fail(PCV_E_INVALID, "segment range past the end");
  const uint64_t base = b->seg_offset[first_segment], count = b->seg_offset[first_segment + num_segments] - base;
  if (count > capacity) return ctx->fail(PCV_E_INVALID, "the segments hold " + std::to_string(count) + " points, capacity is " + std::to_string(capacity));
  const uint64_t chunk0 = b->seg_first_chunk[first_segment], nchunks = b->seg_first_chunk[first_segment + num_segments] - chunk0;
  if (count == 0 || nchunks == 0) return PCV_OK;
  if (!out) return ctx->fail(PCV_E_INVALID, "out is null");
  int rc = pcv_s2_extra_resident(c, (size_t)k);
  if (rc != PCV_OK) return rc;
  const PcvS2Extra& e = c->extras[(size_t)k];
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PcvScratch sc(ctx);
  uint8_t* d_out = (uint8_t*)out;
  if (mem == PCV_MEM_HOST) {
    if ((rc = sc.get(&d_out, count * e.elem))) return rc;
  } else if (!aligned_for(e.data_type, out)) {
    return ctx->fail(PCV_E_INVALID, "attribute '" + e.name + "': device output must be aligned to its element's words");
  }
  {
    PcvProf prof(ctx, PCV_K_S2_ATTR_GATHER_POINTS);
    dispatch_form(e.data_type, [&](auto w, auto comps) {
      using W = decltype(w);
      constexpr int C = decltype(comps)::value;
      hipLaunchKernelGGL((s2_attr_gather_points_kernel<W, C>), dim3((uint32_t)nchunks), dim3(256), 0, ctx->stream, b->d_chunks, chunk0, b->d_flags,
                         b->d_offsets, base, (const W*)e.d, (W*)d_out);
    });
  }
  PCV_HIP_CHECK(ctx, hipGetLastError());
  if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipMemcpyAsync(out, d_out, count * e.elem, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->prof_resolve();
  return PCV_OK;
}

extern "C" int pcv_s2_filter_keep_host(int32_t data_type, uint64_t n, const void* data, double lo, double hi, uint8_t* keep) {
  if (s2attr::element_size(data_type) == 0) return pcv_host_fail(PCV_E_INVALID, "Attribute data type invalid");
  if (!s2attr::is_scalar(data_type)) return pcv_host_fail(PCV_E_INVALID, "a filter takes a scalar attribute; a vector attribute has no interval test");
  if (n && (!data || !keep)) return pcv_host_fail(PCV_E_INVALID, "null argument");
  s2attr::dispatch_scalar(data_type, [&](auto t) {
    using T = decltype(t);
    const uint8_t* p = (const uint8_t*)data;
    for (uint64_t i = 0; i < n; ++i) {
      T v;
      std::memcpy(&v, p + i * sizeof(T), sizeof(T));  // (the caller's buffer may stand at any byte)
      keep[i] = (uint8_t)(keep[i] && s2attr::keep<T>(v, lo, hi) ? 1 : 0);
    }
  });
  return PCV_OK;
}
