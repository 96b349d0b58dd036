// pcv_render.hip — the viewer's frame on the device: V cameras over one octree in one call.
//
// The reference's sdl_viewer draws a frame with OpenGL (sdl_viewer/src/lib.rs:158-209, node_drawer.rs:124-160,
// shaders/points.vs / points.fs): get_visible_nodes(world_to_gl), every visible node as GL_POINTS under a depth test, a
// point size and a gamma, over a black clear. gfx950 has no graphics pipeline; this file restates that frame as two kernels:
//
//   K_rc  render_chunks   one ChunkDesc per chunk of every (view, drawn node) — the descriptor form of the query batch; a
//                         chunk's `keep_off` is the draw rank of its first point inside its view, `enc >> 8` the view
//   K_rs  render_splat    a wave per chunk: the shader's decode (f32 attribute, f64 cube transform), clip_from_query in f64,
//                         one rounding to f32, clip test, window transform, and one atomicMin of (bits(zw) << 32 | rank)
//                         per covered pixel of the view's u64 key plane
//   K_rr  render_resolve  a thread per pixel: key -> rank -> (node, index) by binary search in the view's u64 prefix of
//                         point counts -> colour bytes -> gamma table -> RGBA8, zw to the depth plane, covered pixels
//
// An integer minimum does not depend on the order the atomics arrive in, so a frame's bytes do not depend on scheduling.
// Every f32 step is a single correctly rounded operation (-ffp-contract=off, correctly rounded f32 division, denormals
// kept); no libm call is made on the device: the gamma table comes from the host.
// Bounds: K_rs reads 3 / 6 / 12 / 24 node bytes per submitted point (HBM stream) and issues 8 atomic bytes per covered
// pixel (L2 atomics); which of the two binds depends on how much of the view's points the frustum keeps.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pcv_query_dev.h"

namespace {

constexpr uint64_t kDefaultWorkspace = 2ull << 30;
constexpr uint32_t kMaxExtent = 16384;
constexpr unsigned long long kEmptyKey = ~0ull;

// points per chunk: what fills 6 KiB at the node's encoding (256 f64, 512 f32, 1 024 u16, 2 048 u8 points), as the query
// batch's chunks at shift 0
__host__ __device__ inline uint32_t enc_stride(uint32_t enc) {
  return enc == PCV_ENC_UINT8 ? 3u : enc == PCV_ENC_UINT16 ? 6u : enc == PCV_ENC_FLOAT32 ? 12u : 24u;
}
__host__ __device__ inline uint32_t chunk_points(uint32_t enc) { return 256u * (24u / enc_stride(enc)); }

// K_rc: the segment of chunk c is the last one whose first chunk is <= c (no segment is empty: zero-point nodes are not
// in a visible list)
__global__ __launch_bounds__(256) void render_chunks_kernel(const uint32_t* __restrict__ seg_node, const uint32_t* __restrict__ seg_view,
                                                             const uint64_t* __restrict__ seg_chunk, const uint64_t* __restrict__ seg_pts,
                                                             const uint64_t* __restrict__ view_seg, uint64_t nseg,
                                                             const BatchNode* __restrict__ nodes, uint64_t nchunks,
                                                             ChunkDesc* __restrict__ desc) {
  for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += (uint64_t)gridDim.x * 256) {
    uint64_t lo = 0, hi = nseg;
    while (hi - lo > 1) {
      const uint64_t mid = (lo + hi) >> 1;
      if (seg_chunk[mid] <= c) lo = mid;
      else hi = mid;
    }
    const BatchNode nd = nodes[seg_node[lo]];
    const uint32_t view = seg_view[lo];
    const uint32_t stride = enc_stride(nd.enc), per = chunk_points(nd.enc);
    const uint64_t kk = (c - seg_chunk[lo]) * per;
    ChunkDesc d;
    d.src = nd.xyz_off + kk * stride;
    d.attr_index = nd.point_off + kk;
    d.cube_min[0] = nd.cube_min[0];
    d.cube_min[1] = nd.cube_min[1];
    d.cube_min[2] = nd.cube_min[2];
    d.cube_edge = nd.cube_edge;
    d.keep_off = (seg_pts[lo] - seg_pts[view_seg[view]]) + kk;  // draw rank of the chunk's first point inside its view
    d.enc = nd.enc | ((uint32_t)PCV_SHAPE_FRUSTUM << 4) | (view << 8);
    d.cnt = (uint32_t)(nd.n - kk < per ? nd.n - kk : per);
    desc[c] = d;
  }
}

// points.vs: the vertex attribute as GL hands it to the shader — normalised integers become f32 (c / max), Float32 stays,
// Float64 arrives as a dvec3 — then position * edge_length + min in f64
__device__ __forceinline__ double shader_attribute(uint32_t enc, const uint8_t* at, uint32_t axis) {
  switch (enc) {  // wave-uniform
    case PCV_ENC_UINT8: return (double)((float)at[axis] / 255.0f);
    case PCV_ENC_UINT16: return (double)((float)reinterpret_cast<const uint16_t*>(at)[axis] / 65535.0f);
    case PCV_ENC_FLOAT32: return (double)reinterpret_cast<const float*>(at)[axis];
    default: return reinterpret_cast<const double*>(at)[axis];
  }
}

// GL pixels i of [0, n) with lo <= i + 0.5 < hi, all in f32: [first, last], empty as first > last. (float)i + 0.5f is exact
// for i < 2^23 and grows with i, so the covered pixels are one run; its ends are found by testing the predicate itself.
__device__ __forceinline__ void covered_run(float centre, float half, uint32_t n, int32_t* first, int32_t* last) {
  const float lo = centre - half, hi = centre + half;
  *first = 0;
  *last = -1;
  if (!(lo < hi)) return;  // NaN
  // lo >= -32.5 and hi <= 16 416.5 for a point that passed the clip test: both conversions are in range
  int32_t a = (int32_t)lo - 1, b = (int32_t)hi + 1;
  if (a < 0) a = 0;
  if (b > (int32_t)n - 1) b = (int32_t)n - 1;
  while (a <= b && !(lo <= (float)a + 0.5f)) ++a;
  while (b >= a && !((float)b + 0.5f < hi)) --b;
  *first = a;
  *last = b;
}

struct RenderSplatArgs {
  const ChunkDesc* desc;
  uint64_t c0, c1;              // the group's chunks
  const PcvShapeDev* shapes;    // the frusta: clip_from_query of view v at shapes[v]
  const uint8_t* xyz;
  unsigned long long* keys;     // the group's key planes, H x W each, rows top to bottom
  unsigned long long* drawn;    // per view of the call: points that passed the clip test
  uint32_t view0;               // the group's first view
  uint32_t W, H;
  float half_w, half_h;         // 0.5f * (float)W, 0.5f * (float)H
  float half_size;              // 0.5f * point_size
};

// K_rs: persistent waves, wave w takes chunks w, w + waves, ...
__global__ __launch_bounds__(256) void render_splat_kernel(RenderSplatArgs a) {
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const uint64_t plane = (uint64_t)a.W * a.H;
  for (uint64_t c = a.c0 + (uint64_t)blockIdx.x * 4 + wave; c < a.c1; c += (uint64_t)gridDim.x * 4) {
    const ChunkDesc d = a.desc[c];
    const uint32_t view = d.enc >> 8, enc = d.enc & 15u, stride = enc_stride(enc);
    const double* m = a.shapes[view].clip_from_query;  // column-major, as nalgebra stores world_to_gl
    double mm[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) mm[i] = m[i];
    unsigned long long* keys = a.keys + (uint64_t)(view - a.view0) * plane;
    const uint8_t* src = a.xyz + d.src;
    uint32_t ndrawn = 0;
    for (uint32_t q0 = 0; q0 < d.cnt; q0 += 64) {
      const uint32_t q = q0 + lane;
      bool draw = false;
      float xw = 0.0f, yw = 0.0f, zw = 0.0f;
      if (q < d.cnt) {
        const uint8_t* at = src + (uint64_t)q * stride;
        const double px = shader_attribute(enc, at, 0) * d.cube_edge + d.cube_min[0];
        const double py = shader_attribute(enc, at, 1) * d.cube_edge + d.cube_min[1];
        const double pz = shader_attribute(enc, at, 2) * d.cube_edge + d.cube_min[2];
        // gl_Position = vec4(world_to_gl * dvec4(p, 1)): f64, left to right, one rounding to f32 per component
        const float x = (float)(((mm[0] * px + mm[4] * py) + mm[8] * pz) + mm[12]);
        const float y = (float)(((mm[1] * px + mm[5] * py) + mm[9] * pz) + mm[13]);
        const float z = (float)(((mm[2] * px + mm[6] * py) + mm[10] * pz) + mm[14]);
        const float w = (float)(((mm[3] * px + mm[7] * py) + mm[11] * pz) + mm[15]);
        // the clip volume; a NaN fails every comparison, and a w that rounded to +inf is refused (inf / inf has no depth)
        draw = w > 0.0f && w <= 3.40282347e+38f && -w <= x && x <= w && -w <= y && y <= w && -w <= z && z <= w;
        if (draw) {
          const float xd = x / w, yd = y / w, zd = z / w;
          xw = (xd + 1.0f) * a.half_w;
          yw = (yd + 1.0f) * a.half_h;
          zw = zd * 0.5f + 0.5f;
        }
      }
      ndrawn += (uint32_t)__popcll(__ballot(draw));
      if (draw) {
        int32_t i0, i1, j0, j1;
        covered_run(xw, a.half_size, a.W, &i0, &i1);
        covered_run(yw, a.half_size, a.H, &j0, &j1);
        // GL_LESS with the points submitted in draw order: smallest depth, then smallest rank
        const unsigned long long key = ((unsigned long long)__float_as_uint(zw) << 32) | (unsigned long long)((uint32_t)d.keep_off + q);
        for (int32_t j = j0; j <= j1; ++j) {
          unsigned long long* row = keys + (uint64_t)(a.H - 1u - (uint32_t)j) * a.W;  // image row 0 is the top
          for (int32_t i = i0; i <= i1; ++i) atomicMin(row + i, key);
        }
      }
    }
    if (lane == 0 && ndrawn) atomicAdd(a.drawn + view, (unsigned long long)ndrawn);
  }
}

struct RenderResolveArgs {
  const unsigned long long* keys;  // the group's key planes
  uint64_t npix, plane;            // pixels of the group, of one view
  uint32_t view0;
  const uint64_t* view_seg;        // V + 1: first segment of each view
  const uint64_t* seg_pts;         // nseg + 1: points before each segment (over all views)
  const uint32_t* seg_node;
  const BatchNode* nodes;
  const uint8_t* rgb;
  const uint8_t* lut;              // 256 entries (pcv_render_gamma_lut)
  uint32_t* image;                 // all views of the call
  float* depth;                    // all views of the call
  unsigned long long* covered;     // per view of the call
};

// K_rr: a thread per pixel of the group
__global__ __launch_bounds__(256) void render_resolve_kernel(RenderResolveArgs a) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < a.npix; p += (uint64_t)gridDim.x * 256) {
    const uint32_t view = a.view0 + (uint32_t)(p / a.plane);
    const unsigned long long key = a.keys[p];
    const bool cov = key != kEmptyKey;
    uint32_t px = 0xff000000u;  // (0, 0, 0, 255)
    float zw = 1.0f;
    if (cov) {
      const uint64_t s0 = a.view_seg[view], s1 = a.view_seg[view + 1];
      const uint64_t g = a.seg_pts[s0] + (uint32_t)key;  // the point's place among the points of all views
      uint64_t lo = s0, hi = s1;
      while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a.seg_pts[mid] <= g) lo = mid;
        else hi = mid;
      }
      const uint8_t* c = a.rgb + 3 * (a.nodes[a.seg_node[lo]].point_off + (g - a.seg_pts[lo]));
      px = (uint32_t)a.lut[c[0]] | (uint32_t)a.lut[c[1]] << 8 | (uint32_t)a.lut[c[2]] << 16 | 0xff000000u;
      zw = __uint_as_float((uint32_t)(key >> 32));
    }
    const uint64_t at = (uint64_t)a.view0 * a.plane + p;
    a.image[at] = px;
    a.depth[at] = zw;
    // covered pixels per view: one add per wave where the wave's pixels are of one view
    const unsigned long long act = __ballot(true), cv = __ballot(cov);
    const uint32_t v0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)view);
    if (__ballot(view == v0) == act) {
      if (cv && lane == (uint32_t)(__ffsll(act) - 1)) atomicAdd(a.covered + v0, (unsigned long long)__popcll(cv));
    } else if (cov) {
      atomicAdd(a.covered + view, 1ull);
    }
  }
}

struct ViewInfo {
  int32_t status = 0;
  uint32_t nodes_visible = 0, nodes_drawn = 0;
  uint64_t points_submitted = 0, points_drawn = 0, pixels_covered = 0;
};

int resident_grid(pcv_ctx* ctx, const void* kernel, int* grid) {
  int cus = 0, per_cu = 0;
  PCV_HIP_CHECK(ctx, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device));
  PCV_HIP_CHECK(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0));
  *grid = std::max(cus, 1) * std::max(per_cu, 1);
  return PCV_OK;
}

}  // namespace

struct pcv_render {
  pcv_ctx* ctx = nullptr;
  uint32_t V = 0, W = 0, H = 0;
  uint32_t* d_images = nullptr;
  float* d_depth = nullptr;
  std::vector<ViewInfo> info;
};

extern "C" int pcv_render_check_params(const pcv_render_params* p) {
  if (!p) return PCV_E_INVALID;
  if (p->width < 1 || p->width > kMaxExtent || p->height < 1 || p->height > kMaxExtent) return PCV_E_INVALID;
  if (!(p->point_size >= 1.0f && p->point_size <= (float)PCV_RENDER_MAX_POINT_SIZE)) return PCV_E_INVALID;  // (a NaN fails both)
  if (!(p->gamma > 0.0f) || !std::isfinite(p->gamma)) return PCV_E_INVALID;
  return PCV_OK;
}

extern "C" int pcv_render_gamma_lut(float gamma, uint8_t lut[256]) {
  if (!lut || !(gamma > 0.0f) || !std::isfinite(gamma)) return PCV_E_INVALID;
  // points.fs: pow(color, vec3(1.0 / gamma)) on the normalised colour, then the framebuffer's 8-bit conversion
  for (int c = 0; c < 256; ++c) lut[c] = (uint8_t)roundf(255.0f * powf((float)c / 255.0f, 1.0f / gamma));
  return PCV_OK;
}

extern "C" void pcv_render_free(pcv_render* r) {
  if (!r) return;
  r->ctx->dev_free(r->d_images);
  r->ctx->dev_free(r->d_depth);
  delete r;
}

static int render_views(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* p, pcv_render* r) {
  const uint32_t V = frusta->count, W = p->width, H = p->height;
  const uint64_t plane = (uint64_t)W * H;
  r->V = V;
  r->W = W;
  r->H = H;
  r->info.assign(V, ViewInfo());
  if (V == 0) return PCV_OK;
  // the key planes of one group of views are the workspace; a single view over the limit is refused before anything is
  // allocated
  const uint64_t workspace = p->max_workspace_bytes ? p->max_workspace_bytes : kDefaultWorkspace;
  const uint64_t group_views = std::min<uint64_t>(V, workspace / (8 * plane));
  if (group_views == 0) return ctx->fail(PCV_E_OOM, "render: the key plane of one view exceeds max_workspace_bytes");
  if (!tree->d_xyz && !tree->nodes.empty()) {  // an octree opened from a directory: node files are uploaded on first use
    int lrc = pcv_octree_load_device(tree);
    if (lrc) return lrc;
  }
  int rc = pcv_octree_prepare_query(tree);
  if (rc) return rc;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  const uint32_t m = (uint32_t)tree->nodes.size();
  // 1. the visible lists, heap pop order, cut to max_nodes (take(max_nodes_to_display), lib.rs:172-176)
  const uint32_t cap = m == 0 ? 0u : (p->max_nodes ? std::min(p->max_nodes, m) : m);
  std::vector<uint32_t> counts(V, 0), lists((size_t)V * std::max(cap, 1u));
  std::vector<int32_t> status(V, 0);
  if ((rc = pcv_visible_nodes(ctx, frusta, tree, cap, counts.data(), lists.data(), status.data()))) return rc;
  // 2. one segment per (view, drawn node); u64 prefixes of chunks and of points
  std::vector<uint32_t> seg_node, seg_view;
  std::vector<uint64_t> seg_chunk(1, 0), seg_pts(1, 0), view_seg(V + 1, 0), view_chunk(V + 1, 0);
  for (uint32_t v = 0; v < V; ++v) {
    ViewInfo& vi = r->info[v];
    vi.status = status[v];
    vi.nodes_visible = counts[v];
    if (status[v] == 0) {  // 1 / 2: the reference panics; the view is a cleared image
      vi.nodes_drawn = std::min(counts[v], cap);
      for (uint32_t k = 0; k < vi.nodes_drawn; ++k) {
        const uint32_t node = lists[(size_t)v * cap + k];
        const pcv_node_info& nd = tree->nodes[node];
        const uint64_t n = (uint64_t)std::max<int64_t>(nd.num_points, 0);
        if (n == 0) continue;  // (never: zero-point nodes are not listed)
        const uint32_t per = chunk_points(nd.encoding);
        seg_node.push_back(node);
        seg_view.push_back(v);
        seg_chunk.push_back(seg_chunk.back() + (n + per - 1) / per);
        seg_pts.push_back(seg_pts.back() + n);
        vi.points_submitted += n;
      }
      if (vi.points_submitted >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "render: a view draws 2^32 - 1 points or more");
    }
    view_seg[v + 1] = seg_node.size();
    view_chunk[v + 1] = seg_chunk.back();
  }
  const uint64_t nseg = seg_node.size(), nchunks = seg_chunk.back();
  // 3. the images of all views, and the scratch
  if ((rc = ctx->dev_alloc((void**)&r->d_images, 4 * plane * V)) || (rc = ctx->dev_alloc((void**)&r->d_depth, 4 * plane * V))) return rc;
  PcvScratch sc(ctx);
  unsigned long long *d_keys, *d_counters;
  uint8_t* d_lut;
  uint32_t *d_seg_node, *d_seg_view;
  uint64_t *d_seg_chunk, *d_seg_pts, *d_view_seg;
  ChunkDesc* d_desc;
  if ((rc = sc.get(&d_keys, group_views * plane)) || (rc = sc.get(&d_counters, 2 * (size_t)V)) || (rc = sc.get(&d_lut, 256)) ||
      (rc = sc.get(&d_seg_node, std::max<uint64_t>(nseg, 1))) || (rc = sc.get(&d_seg_view, std::max<uint64_t>(nseg, 1))) ||
      (rc = sc.get(&d_seg_chunk, nseg + 1)) || (rc = sc.get(&d_seg_pts, nseg + 1)) || (rc = sc.get(&d_view_seg, (size_t)V + 1)) ||
      (rc = sc.get(&d_desc, std::max<uint64_t>(nchunks, 1))))
    return rc;
  uint8_t lut[256];
  if ((rc = pcv_render_gamma_lut(p->gamma, lut))) return ctx->fail(rc, "render: gamma");
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_lut, lut, 256, hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_counters, 0, 16 * (size_t)V, ctx->stream));
  if (nseg) {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_node, seg_node.data(), 4 * nseg, hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_view, seg_view.data(), 4 * nseg, hipMemcpyHostToDevice, ctx->stream));
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_chunk, seg_chunk.data(), 8 * (nseg + 1), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_pts, seg_pts.data(), 8 * (nseg + 1), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_view_seg, view_seg.data(), 8 * ((size_t)V + 1), hipMemcpyHostToDevice, ctx->stream));
  const BatchNode* d_nodes = pcv_octree_query_nodes(tree);
  // grids of resident size that stride over chunks / pixels: no dispatch grows with V or with the node count
  int splat_grid = 1, resolve_grid = 1, chunks_grid = 1;
  if ((rc = resident_grid(ctx, (const void*)render_splat_kernel, &splat_grid)) ||
      (rc = resident_grid(ctx, (const void*)render_resolve_kernel, &resolve_grid)) ||
      (rc = resident_grid(ctx, (const void*)render_chunks_kernel, &chunks_grid)))
    return rc;
  if (nchunks) {
    PcvProf prof(ctx, PCV_K_RENDER_CHUNKS);
    hipLaunchKernelGGL(render_chunks_kernel, dim3((uint32_t)std::min<uint64_t>((nchunks + 255) / 256, (uint64_t)chunks_grid)), dim3(256), 0,
                       ctx->stream, d_seg_node, d_seg_view, d_seg_chunk, d_seg_pts, d_view_seg, nseg, d_nodes, nchunks, d_desc);
    PCV_HIP_CHECK(ctx, hipGetLastError());
  }
  RenderSplatArgs sa{};
  sa.desc = d_desc;
  sa.shapes = frusta->dev;
  sa.xyz = tree->d_xyz;
  sa.keys = d_keys;
  sa.drawn = d_counters;
  sa.W = W;
  sa.H = H;
  sa.half_w = 0.5f * (float)W;
  sa.half_h = 0.5f * (float)H;
  sa.half_size = 0.5f * p->point_size;
  RenderResolveArgs ra{};
  ra.keys = d_keys;
  ra.plane = plane;
  ra.view_seg = d_view_seg;
  ra.seg_pts = d_seg_pts;
  ra.seg_node = d_seg_node;
  ra.nodes = d_nodes;
  ra.rgb = tree->d_rgb;
  ra.lut = d_lut;
  ra.image = r->d_images;
  ra.depth = r->d_depth;
  ra.covered = d_counters + V;
  for (uint32_t v0 = 0; v0 < V; v0 += (uint32_t)group_views) {
    const uint32_t nv = (uint32_t)std::min<uint64_t>(group_views, V - v0);
    PCV_HIP_CHECK(ctx, hipMemsetAsync(d_keys, 0xff, 8 * plane * nv, ctx->stream));
    sa.c0 = view_chunk[v0];
    sa.c1 = view_chunk[v0 + nv];
    sa.view0 = v0;
    if (sa.c1 > sa.c0) {
      PcvProf prof(ctx, PCV_K_RENDER_SPLAT);
      hipLaunchKernelGGL(render_splat_kernel, dim3((uint32_t)std::min<uint64_t>((sa.c1 - sa.c0 + 3) / 4, (uint64_t)splat_grid)), dim3(256), 0,
                         ctx->stream, sa);
      PCV_HIP_CHECK(ctx, hipGetLastError());
    }
    ra.npix = plane * nv;
    ra.view0 = v0;
    {
      PcvProf prof(ctx, PCV_K_RENDER_RESOLVE);
      hipLaunchKernelGGL(render_resolve_kernel, dim3((uint32_t)std::min<uint64_t>((ra.npix + 255) / 256, (uint64_t)resolve_grid)), dim3(256), 0,
                         ctx->stream, ra);
      PCV_HIP_CHECK(ctx, hipGetLastError());
    }
  }
  std::vector<unsigned long long> h_counters(2 * (size_t)V);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(h_counters.data(), d_counters, 16 * (size_t)V, hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the scratch is released on return
  for (uint32_t v = 0; v < V; ++v) {
    r->info[v].points_drawn = h_counters[v];
    r->info[v].pixels_covered = h_counters[(size_t)V + v];
  }
  return PCV_OK;
}

extern "C" int pcv_render_views(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* params, pcv_render** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!frusta || !tree || !params || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (pcv_render_check_params(params) != PCV_OK)
    return ctx->fail(PCV_E_INVALID, "render: width and height in 1 ..= 16384, point_size in 1 ..= 64, gamma finite and > 0");
  if (frusta->ctx != ctx || tree->ctx != ctx) return ctx->fail(PCV_E_INVALID, "render: shapes and octree must belong to the context");
  if (frusta->count >= (1u << kBatchShapeBits)) return ctx->fail(PCV_E_INVALID, "render: at most 2^24 - 1 views");
  for (int32_t kind : frusta->kinds)
    if (kind != PCV_SHAPE_FRUSTUM && kind != PCV_SHAPE_FRUSTUM_WITH_INVERSE) return ctx->fail(PCV_E_INVALID, "render: every shape must be a frustum");
  pcv_render* r = new pcv_render();
  r->ctx = ctx;
  const int rc = render_views(ctx, frusta, tree, params, r);
  if (rc != PCV_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing queued may still write into what is freed here
    (void)hipGetLastError();
    pcv_render_free(r);
    return rc;
  }
  ctx->prof_resolve();
  *out = r;
  return PCV_OK;
}

extern "C" int pcv_render_info(pcv_render* r, uint32_t view, int32_t* status, uint32_t* nodes_visible, uint32_t* nodes_drawn,
                               uint64_t* points_submitted, uint64_t* points_drawn, uint64_t* pixels_covered) {
  if (!r) return PCV_E_INVALID;
  if (view >= r->V) return r->ctx->fail(PCV_E_INVALID, "render: view past the end");
  const ViewInfo& vi = r->info[view];
  if (status) *status = vi.status;
  if (nodes_visible) *nodes_visible = vi.nodes_visible;
  if (nodes_drawn) *nodes_drawn = vi.nodes_drawn;
  if (points_submitted) *points_submitted = vi.points_submitted;
  if (points_drawn) *points_drawn = vi.points_drawn;
  if (pixels_covered) *pixels_covered = vi.pixels_covered;
  return PCV_OK;
}

static int render_copy(pcv_render* r, const void* src, uint32_t first, uint32_t count, void* dst, int mem) {
  if (!r) return PCV_E_INVALID;
  pcv_ctx* ctx = r->ctx;
  if (first > r->V || count > r->V - first) return ctx->fail(PCV_E_INVALID, "render: view range past the end");
  if (mem != PCV_MEM_HOST && mem != PCV_MEM_DEVICE) return ctx->fail(PCV_E_INVALID, "bad mem");
  if (count == 0) return PCV_OK;
  if (!dst) return ctx->fail(PCV_E_INVALID, "null output");
  const uint64_t view_bytes = 4 * (uint64_t)r->W * r->H;
  PCV_HIP_CHECK(ctx, hipSetDevice(ctx->device));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(dst, (const uint8_t*)src + view_bytes * first, view_bytes * count,
                                    mem == PCV_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return PCV_OK;
}

extern "C" int pcv_render_images(pcv_render* r, uint32_t first, uint32_t count, void* rgba, int mem) {
  return render_copy(r, r ? r->d_images : nullptr, first, count, rgba, mem);
}

extern "C" int pcv_render_depth(pcv_render* r, uint32_t first, uint32_t count, void* zw_f32, int mem) {
  return render_copy(r, r ? r->d_depth : nullptr, first, count, zw_f32, mem);
}
