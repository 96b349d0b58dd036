// pcv_octree_obj.hip — the finished octree as an object: release, accessors, the device blobs and their host copies, node
// bytes and node copies. Host code only.
#include <cstring>

#include "pcv_build_state.h"
#include "pcv_internal.h"

extern "C" void pcv_octree_free(pcv_octree* t) {
  if (!t) return;
  delete t->pending;
  if (t->ctx) {
    pcv_octree_release_query(t);
    t->ctx->host_release(t->h_xyz.p);
    t->ctx->host_release(t->h_rgb.p);
    t->ctx->host_release(t->h_int.p);
    t->ctx->dev_free(t->d_xyz);
    t->ctx->dev_free(t->d_rgb);
    t->ctx->dev_free(t->d_int);
  }
  delete t;
}
extern "C" uint64_t pcv_octree_num_nodes(const pcv_octree* t) { return t ? t->nodes.size() : 0; }
extern "C" uint64_t pcv_octree_num_points(const pcv_octree* t) { return t ? t->num_points : 0; }
extern "C" int pcv_octree_has_intensity(const pcv_octree* t) { return t && t->has_intensity; }
extern "C" int pcv_octree_node(const pcv_octree* t, uint64_t i, pcv_node_info* out) {
  if (!t || !out || i >= t->nodes.size()) return PCV_E_INVALID;
  *out = t->nodes[i];
  return PCV_OK;
}
extern "C" void pcv_octree_meta(const pcv_octree* t, double* resolution, double bbox_min[3], double bbox_max[3],
                                int* version) {
  if (!t) return;
  if (resolution) *resolution = t->resolution;
  for (int a = 0; a < 3; ++a) {
    if (bbox_min) bbox_min[a] = t->bbox_min[a];
    if (bbox_max) bbox_max[a] = t->bbox_max[a];
  }
  if (version) *version = 13;  // CURRENT_VERSION, reference src/lib.rs:48
}
extern "C" int pcv_octree_stage_ms(const pcv_octree* t, float* ms, int cap) {
  if (!t || !ms) return 0;
  int n = cap < PCV_NUM_STAGES ? cap : PCV_NUM_STAGES;
  for (int i = 0; i < n; ++i) ms[i] = t->stage_ms[i];
  return n;
}
extern "C" void pcv_octree_build_info(const pcv_octree* t, int* key_levels, int* attempts) {
  if (!t) return;
  if (key_levels) *key_levels = t->key_levels;
  if (attempts) *attempts = t->key_attempts;
}
extern "C" void pcv_octree_spec_stats(const pcv_octree* t, uint64_t stats[4]) {
  if (!t || !stats) return;
  for (int k = 0; k < 4; ++k) stats[k] = t->spec_stats[k];
}
extern "C" int pcv_octree_record_bytes(const pcv_octree* t) { return t ? t->record_bytes : 0; }
extern "C" int pcv_octree_packed_handover(const pcv_octree* t) { return t ? t->packed_handover : 0; }
extern "C" uint64_t pcv_octree_spec_continued(const pcv_octree* t) { return t ? t->spec_continued : 0; }
extern "C" uint64_t pcv_octree_wide_pool_entries(const pcv_octree* t) { return t ? t->wide_pool_entries : 0; }
extern "C" uint64_t pcv_octree_settled_in_sort(const pcv_octree* t) { return t ? t->settled_in_sort : 0; }
extern "C" int pcv_octree_device_blob(const pcv_octree* t, int which, const void** dptr, uint64_t* len) {
  if (!t || !dptr || !len || which < 0 || which > 2) return PCV_E_INVALID;
  *dptr = which == 0 ? t->d_xyz : (which == 1 ? t->d_rgb : t->d_int);
  *len = which == 0 ? t->xyz_bytes : (which == 1 ? t->rgb_bytes : t->int_bytes);
  return PCV_OK;
}

int pcv_octree_fetch_host(pcv_octree* t) {
  if (t->host_valid) return PCV_OK;
  pcv_ctx* ctx = t->ctx;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  int hrc;
  if (t->xyz_bytes && (hrc = ctx->host_alloc((void**)&t->h_xyz.p, t->xyz_bytes))) return hrc;
  if (t->rgb_bytes && (hrc = ctx->host_alloc((void**)&t->h_rgb.p, t->rgb_bytes))) return hrc;
  if (t->int_bytes && (hrc = ctx->host_alloc((void**)&t->h_int.p, t->int_bytes))) return hrc;
  if (t->xyz_bytes) PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->h_xyz.data(), t->d_xyz, t->xyz_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (t->rgb_bytes) PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->h_rgb.data(), t->d_rgb, t->rgb_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (t->int_bytes) PCV_HIP_CHECK(ctx, hipMemcpyAsync(t->h_int.data(), t->d_int, t->int_bytes, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  t->host_valid = true;
  return PCV_OK;
}

extern "C" int pcv_octree_node_data(pcv_octree* t, uint64_t i, int which, const uint8_t** data, uint64_t* len) {
  if (!t || !data || !len || i >= t->nodes.size() || which < 0 || which > 2) return PCV_E_INVALID;
  if (!t->directory.empty()) return pcv_octree_read_node_file(t, i, which, data, len);
  int rc = pcv_octree_fetch_host(t);
  if (rc) return rc;
  const pcv_node_info& nd = t->nodes[i];
  uint64_t np = (uint64_t)nd.num_points;
  if (which == 0) {
    *data = t->h_xyz.data() + nd.xyz_offset;
    *len = np * 3 * (uint64_t)pcv_bytes_per_coordinate(nd.encoding);
  } else if (which == 1) {
    *data = t->h_rgb.data() + nd.point_offset * 3;
    *len = np * 3;
  } else {
    if (!t->has_intensity) {
      *data = nullptr;
      *len = 0;
    } else {
      *data = t->h_int.data() + nd.point_offset * 4;
      *len = np * 4;
    }
  }
  return PCV_OK;
}

extern "C" int pcv_octree_copy_node(const pcv_octree* t, uint64_t i, int which, void* dst, uint64_t capacity, int mem) {
  if (!t || i >= t->nodes.size() || which < 0 || which > 2 || (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE)) return PCV_E_INVALID;
  pcv_ctx* ctx = t->ctx;
  if (!t->directory.empty()) return ctx->fail(PCV_E_INVALID, "pcv_octree_copy_node works on built octrees (device blobs)");
  const pcv_node_info& nd = t->nodes[i];
  const uint64_t np = (uint64_t)nd.num_points;
  const uint8_t* src = nullptr;
  uint64_t len = 0;
  if (which == 0) {
    src = t->d_xyz + nd.xyz_offset;
    len = np * 3 * (uint64_t)pcv_bytes_per_coordinate(nd.encoding);
  } else if (which == 1) {
    src = t->d_rgb + nd.point_offset * 3;
    len = np * 3;
  } else if (t->has_intensity) {
    src = t->d_int + nd.point_offset * 4;
    len = np * 4;
  }
  if (len > capacity) return ctx->fail(PCV_E_INVALID, "destination too small for the node's bytes");
  if (len == 0) return PCV_OK;
  if (!dst) return ctx->fail(PCV_E_INVALID, "dst is null");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, len, mem == PCV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  // device destinations stay asynchronous on the context's stream (pcv_ctx_synchronize, or stream order, completes them)
  if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

// Batch form of pcv_octree_copy_node for the multi-GPU top merge: every rank copies its (sparsely filled, global-size)
// root / level-1 nodes into one buffer that is then all-reduced — one call instead of one per node and file kind.
extern "C" int pcv_octree_copy_nodes(const pcv_octree* t, const pcv_node_copy* copies, uint64_t count, void* dst, uint64_t capacity,
                                     int mem) {
  if (!t || (count && !copies) || (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE)) return PCV_E_INVALID;
  pcv_ctx* ctx = t->ctx;
  if (!t->directory.empty()) return ctx->fail(PCV_E_INVALID, "pcv_octree_copy_nodes works on built octrees (device blobs)");
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const hipMemcpyKind kind = mem == PCV_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  for (uint64_t k = 0; k < count; ++k) {
    const pcv_node_copy& c = copies[k];
    if (c.node >= t->nodes.size()) return ctx->fail(PCV_E_INVALID, "pcv_octree_copy_nodes: node index out of range");
    const pcv_node_info& nd = t->nodes[c.node];
    const uint64_t np = (uint64_t)nd.num_points;
    const uint8_t* src[3] = {t->d_xyz + nd.xyz_offset, t->d_rgb + nd.point_offset * 3, t->has_intensity ? t->d_int + nd.point_offset * 4 : nullptr};
    const uint64_t len[3] = {np * 3 * (uint64_t)pcv_bytes_per_coordinate(nd.encoding), np * 3, t->has_intensity ? np * 4 : 0};
    for (int w = 0; w < 3; ++w) {
      if (c.dst_offset[w] == UINT64_MAX || len[w] == 0) continue;
      if (c.dst_offset[w] > capacity || len[w] > capacity - c.dst_offset[w])
        return ctx->fail(PCV_E_INVALID, "pcv_octree_copy_nodes: destination too small for a node's bytes");
      if (!dst) return ctx->fail(PCV_E_INVALID, "dst is null");
      PCV_HIP_CHECK(ctx, hipMemcpyAsync((uint8_t*)dst + c.dst_offset[w], src[w], len[w], kind, ctx->stream));
    }
  }
  if (mem == PCV_MEM_HOST) PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}
