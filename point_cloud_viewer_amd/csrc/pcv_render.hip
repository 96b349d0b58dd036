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
// With show_octree_nodes (pcv_render_views_ex, PCV_RENDER_OUTLINE_NODES; lib.rs:202-208, box_drawer.rs) one more runs between
// the two, and the prefix counts n + 1 ranks per node: the last rank of a node is its outline's:
//
//   K_ro  render_outline  a lane per (view, drawn node, edge): the cube's two corners to clip space as a point's position,
//                         Liang-Barsky against the seven half-spaces in f32, window transform, width-1 raster along the
//                         major axis, one atomicMin of (bits(zw) << 32 | outline rank) per fragment
//
// With terrain layers (pcv_render_views_terrain; sdl_viewer --terrain, lib.rs:602-606, terrain_drawer/, shaders/terrain.*) two
// more run after the group's points and outlines, and the resolve runs as render_resolve_terrain:
//
//   K_tg  render_terrain_gather  a thread per window vertex of every (view, layer): the vertex's tile through the layer's sorted
//                                tile keys, the f64 chain of terrain.vs once per vertex, the f32 clip point, mask and colour
//                                stored (24 bytes): the window loader
//   K_te  render_terrain_edges   a workgroup per patch of 14 x 14 edge origins, its 16 x 16 vertices staged in LDS: the mask
//                                test of terrain.gs per triangle, every edge of a rendered triangle once, clipped and rasterised
//                                by the outline's own segment walk (draw_segment), one atomicMin per fragment with the edge's rank
//
// An integer minimum does not depend on the order the atomics arrive in, so a frame's bytes do not depend on scheduling.
// Every f32 step is a single correctly rounded operation (-ffp-contract=off, correctly rounded f32 division, denormals
// kept); no libm call is made on the device: the gamma table comes from the host.
// Bounds: K_rs reads 3 / 6 / 12 / 24 node bytes per submitted point (HBM stream) and issues 8 atomic bytes per covered
// pixel (L2 atomics); which of the two binds depends on how much of the view's points the frustum keeps.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pcv_query_dev.h"
#include "pcv_terrain_files.h"
#include "pcv_terrain_obj.h"

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

// box_drawer.rs:63-98, a nibble per entry: the corners as picks (bit 0 x, bit 1 y, bit 2 z: set takes min + edge, the
// table's +1), and the two corners of each of the 12 edges in index order
constexpr uint32_t kCornerPick = 0x23106754u;
constexpr uint64_t kEdgeFrom = 0x346176543210ull, kEdgeTo = 0x702547650321ull;
constexpr float kF32Max = 3.40282347e+38f;

struct RenderOutlineArgs {
  const uint32_t* seg_node;
  const uint32_t* seg_view;
  const uint64_t* seg_rank;      // nseg + 1: ranks before each segment (n + 1 per segment), over all views
  const uint64_t* view_seg;      // V + 1
  uint64_t s0, s1;               // the group's segments
  const BatchNode* nodes;
  const PcvShapeDev* shapes;
  unsigned long long* keys;      // the group's key planes
  unsigned long long* seg_drawn; // per view of the call: segments that survived the clip
  uint32_t view0;
  uint32_t W, H;
  float half_w, half_h;
};

// a corner of the node's cube in clip space: steps 2-3 of a point with the attribute at 0 or 1
__device__ __forceinline__ void outline_corner(const BatchNode& nd, const double* mm, uint32_t pick, float c[4]) {
  const double px = (pick & 1u) ? nd.cube_min[0] + nd.cube_edge : nd.cube_min[0];
  const double py = (pick & 2u) ? nd.cube_min[1] + nd.cube_edge : nd.cube_min[1];
  const double pz = (pick & 4u) ? nd.cube_min[2] + nd.cube_edge : nd.cube_min[2];
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] = (float)(((mm[r] * px + mm[4 + r] * py) + mm[8 + r] * pz) + mm[12 + r]);
}

__device__ __forceinline__ bool f32_finite(float v) { return __builtin_fabsf(v) <= kF32Max; }  // (a NaN fails)

// one half-space of Liang-Barsky: d0, d1 the endpoints' distances, `strict` for w > 0. Returns false when both are outside.
__device__ __forceinline__ bool clip_plane(float d0, float d1, bool strict, float& t_in, float& t_out) {
  const bool in0 = strict ? d0 > 0.0f : d0 >= 0.0f, in1 = strict ? d1 > 0.0f : d1 >= 0.0f;
  const float t = d0 / (d0 - d1);  // read only where one end is outside (a NaN fails both comparisons)
  if (in0 && !in1 && t < t_out) t_out = t;
  if (!in0 && in1 && t > t_in) t_in = t;
  return in0 || in1;
}

// Steps 10 and 11 of a segment between two f32 clip points, the one text for the node outlines and the terrain edges, and
// for the terrain's resolve, which walks the same steps again for one pixel (SINGLE: only the fragment of major-axis pixel
// single_x / single_y). survived() is called once for a segment that passes the clip, begin() once before its first
// fragment (what it returns goes to every emit), emit(state, gx, gy, zw, t, t_in, t_out) per fragment inside the image: gx, gy
// count from the lower left, t is the raster parameter between the clipped ends, t_in and t_out those ends on the segment.
template <bool SINGLE, typename Survived, typename Begin, typename Emit>
__device__ __forceinline__ void draw_segment(const float (&p)[4], const float (&q)[4], float half_w, float half_h, uint32_t W, uint32_t H,
                                             int32_t single_x, int32_t single_y, Survived survived, Begin begin, Emit emit) {
  bool alive = true;
#pragma unroll
  for (int r = 0; r < 4; ++r) alive = alive && f32_finite(p[r]) && f32_finite(q[r]);
  if (!alive) return;
  // w > 0, then w + x, w - x, w + y, w - y, w + z, w - z >= 0: every distance one f32 operation on the unclipped endpoints
  float t_in = 0.0f, t_out = 1.0f;
  alive = clip_plane(p[3], q[3], true, t_in, t_out);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    alive = clip_plane(p[3] + p[r], q[3] + q[r], false, t_in, t_out) && alive;
    alive = clip_plane(p[3] - p[r], q[3] - q[r], false, t_in, t_out) && alive;
  }
  if (!alive || t_in > t_out) return;
  float c0[4], c1[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float d = q[r] - p[r];
    c0[r] = t_in > 0.0f ? p[r] + t_in * d : p[r];
    c1[r] = t_out < 1.0f ? p[r] + t_out * d : q[r];
  }
  if (!(c0[3] > 0.0f && c0[3] <= kF32Max && c1[3] > 0.0f && c1[3] <= kF32Max)) return;
  const float x0 = (c0[0] / c0[3] + 1.0f) * half_w, y0 = (c0[1] / c0[3] + 1.0f) * half_h, z0 = (c0[2] / c0[3]) * 0.5f + 0.5f;
  const float x1 = (c1[0] / c1[3] + 1.0f) * half_w, y1 = (c1[1] / c1[3] + 1.0f) * half_h, z1 = (c1[2] / c1[3]) * 0.5f + 0.5f;
  if (!(f32_finite(x0) && f32_finite(y0) && f32_finite(z0) && f32_finite(x1) && f32_finite(y1) && f32_finite(z1))) return;
  survived();
  // width 1: the pixel centres of the major axis inside [min, max), one fragment each
  const bool x_major = __builtin_fabsf(x1 - x0) >= __builtin_fabsf(y1 - y0);
  const float m0 = x_major ? x0 : y0, m1 = x_major ? x1 : y1, n0 = x_major ? y0 : x0, n1 = x_major ? y1 : x1;
  const uint32_t size_m = x_major ? W : H, size_n = x_major ? H : W;
  const float lo = m0 < m1 ? m0 : m1, hi = m0 < m1 ? m1 : m0;
  if (!(lo < hi)) return;
  // both ends are brought into [-1, size + 1] before the conversion, then found by testing the predicate itself
  const float top = (float)size_m + 1.0f;
  int32_t i0 = (int32_t)(lo < -1.0f ? -1.0f : lo > top ? top : lo) - 1, i1 = (int32_t)(hi < -1.0f ? -1.0f : hi > top ? top : hi) + 1;
  if (i0 < 0) i0 = 0;
  if (i1 > (int32_t)size_m - 1) i1 = (int32_t)size_m - 1;
  if constexpr (SINGLE) {  // the predicate on the one pixel
    const int32_t i = x_major ? single_x : single_y;
    if (i < i0 || i > i1 || !(lo <= (float)i + 0.5f) || !((float)i + 0.5f < hi)) return;
    i0 = i1 = i;
  } else {
    while (i0 <= i1 && !(lo <= (float)i0 + 0.5f)) ++i0;
    while (i1 >= i0 && !((float)i1 + 0.5f < hi)) --i1;
  }
  auto state = begin();
  const float dm = m1 - m0, dn = n1 - n0, dz = z1 - z0, limit = (float)size_n;
  for (int32_t i = i0; i <= i1; ++i) {
    const float t = (((float)i + 0.5f) - m0) / dm;
    const float n = n0 + t * dn;
    if (!(n >= 0.0f && n < limit)) continue;  // outside the image (or NaN); inside, the conversion below is floorf
    const uint32_t j = (uint32_t)(int32_t)n;
    float zw = z0 + t * dz;
    if (!(zw > 0.0f)) zw = 0.0f;  // (a NaN and -0.0f too: the key orders by the bit pattern)
    if (zw > 1.0f) zw = 1.0f;
    const uint32_t gx = x_major ? (uint32_t)i : j, gy = x_major ? j : (uint32_t)i;
    emit(state, gx, gy, zw, t, t_in, t_out);
  }
}

// K_ro: item = segment * 12 + edge over the group's segments; the grid strides over the items
__global__ __launch_bounds__(256) void render_outline_kernel(RenderOutlineArgs a) {
  const uint64_t items = (a.s1 - a.s0) * 12, plane = (uint64_t)a.W * a.H;
  for (uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (uint64_t)gridDim.x * 256) {
    const uint64_t s = a.s0 + it / 12;
    const uint32_t e = (uint32_t)(it % 12), view = a.seg_view[s];
    const BatchNode nd = a.nodes[a.seg_node[s]];
    const double* mm = a.shapes[view].clip_from_query;
    float p[4], q[4];
    outline_corner(nd, mm, (kCornerPick >> (4u * (uint32_t)((kEdgeFrom >> (4u * e)) & 15u))) & 7u, p);
    outline_corner(nd, mm, (kCornerPick >> (4u * (uint32_t)((kEdgeTo >> (4u * e)) & 15u))) & 7u, q);
    unsigned long long* keys = nullptr;
    draw_segment<false>(
        p, q, a.half_w, a.half_h, a.W, a.H, 0, 0, [&]() { atomicAdd(a.seg_drawn + view, 1ull); },
        [&]() {
          keys = a.keys + (uint64_t)(view - a.view0) * plane;
          // the outline's rank is the last of its node's n + 1
          return (unsigned long long)(uint32_t)(a.seg_rank[s + 1] - 1 - a.seg_rank[a.view_seg[view]]);
        },
        [&](unsigned long long rank, uint32_t gx, uint32_t gy, float zw, float, float, float) {
          atomicMin(keys + (uint64_t)(a.H - 1u - gy) * a.W + gx, ((unsigned long long)__float_as_uint(zw) << 32) | rank);
        });
  }
}

// ---- terrain layers -------------------------------------------------------------------------------
// one layer as the kernels read it
struct TerrainLayerDev {
  PcvTerrainGrid grid;
  uint64_t ntiles;
  const int64_t* tile_keys;  // ascending (pcv_terrain_tile_key)
  const float* heights;      // ntiles x T x T x (height, mask)
  const uint8_t* colors;     // ntiles x T x T x 4
  uint32_t T, pad;
};

struct RenderTerrainArgs {
  const TerrainLayerDev* layers;
  const int64_t* pos;              // per (view of the call, layer): the window position
  const uint32_t* view_status;     // per view of the call: 0 draws
  const PcvShapeDev* shapes;
  const uint64_t* view_seg;        // V + 1
  const uint64_t* seg_rank;        // nseg + 1: the ranks of the nodes (and outlines); a view's terrain ranks follow them
  float4* clip;                    // the group's windows, (view - view0) * L + layer, Wn x Wn each: f32 clip points,
  uint32_t* mask;                  //   masks,
  uint32_t* color;                 //   colours as stored (r | g << 8 | b << 16 | a << 24)
  unsigned long long* keys;        // the group's key planes
  unsigned long long* counters;    // per (view of the call, layer): edges submitted, edges drawn, pixels won
  uint32_t L, Wn;
  uint32_t view0, nv;
  uint32_t W, H;
  float half_w, half_h;
};

// K_tg: a thread per window vertex of every (view, layer) of the group, the grid strides over them: the tile of the vertex by
// binary search in the layer's sorted tile keys, then step 14. This is the window loader: 24 bytes out per vertex.
__global__ __launch_bounds__(256) void render_terrain_gather_kernel(RenderTerrainArgs a) {
  const uint64_t per = (uint64_t)a.Wn * a.Wn, items = per * a.L * a.nv;
  for (uint64_t it = (uint64_t)blockIdx.x * 256 + threadIdx.x; it < items; it += (uint64_t)gridDim.x * 256) {
    const uint32_t vl = (uint32_t)(it / per), cell = (uint32_t)(it % per);
    const uint32_t view = a.view0 + vl / a.L, layer = vl % a.L;
    if (a.view_status[view] != 0) continue;  // a cleared view: its windows are never read
    const uint32_t ax = cell % a.Wn, ay = cell / a.Wn;
    const TerrainLayerDev& ly = a.layers[layer];
    const int64_t px = a.pos[2 * ((uint64_t)view * a.L + layer)], py = a.pos[2 * ((uint64_t)view * a.L + layer) + 1];
    const int64_t gi = px + (int64_t)ax, gj = py + (int64_t)ay;  // |pos| < 2^53 + 512
    const int64_t T = (int64_t)ly.T;
    const int64_t tx = pcv_terrain_floor_div(gi, T), ty = pcv_terrain_floor_div(gj, T);
    float height = 0.0f, maskf = 0.0f;
    uint32_t color = 0;
    if (tx >= INT32_MIN && tx <= INT32_MAX && ty >= INT32_MIN && ty <= INT32_MAX && ly.ntiles) {
      const int64_t key = pcv_terrain_tile_key((int32_t)tx, (int32_t)ty);
      uint64_t lo = 0, hi = ly.ntiles;  // the last tile whose key is <= key
      while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ly.tile_keys[mid] <= key) lo = mid;
        else hi = mid;
      }
      if (ly.tile_keys[lo] == key) {
        const uint64_t o = lo * (uint64_t)(T * T) + (uint64_t)pcv_terrain_floor_mod(gj, T) * ly.T + (uint64_t)pcv_terrain_floor_mod(gi, T);
        height = ly.heights[2 * o];
        maskf = ly.heights[2 * o + 1];
        color = reinterpret_cast<const uint32_t*>(ly.colors)[o];
      }
    }
    const PcvTerrainGrid& g = ly.grid;
    const double lx = g.o[0] + g.res * ((double)ax + (double)px);
    const double lyy = g.o[1] + g.res * ((double)ay + (double)py);
    const double lz = g.o[2] + (double)height;
    // world = M^T loc + t: column r of M against loc
    const double wx = ((g.m[0] * lx + g.m[3] * lyy) + g.m[6] * lz) + g.t[0];
    const double wy = ((g.m[1] * lx + g.m[4] * lyy) + g.m[7] * lz) + g.t[1];
    const double wz = ((g.m[2] * lx + g.m[5] * lyy) + g.m[8] * lz) + g.t[2];
    const double* mm = a.shapes[view].clip_from_query;
    float4 c;
    c.x = (float)(((mm[0] * wx + mm[4] * wy) + mm[8] * wz) + mm[12]);
    c.y = (float)(((mm[1] * wx + mm[5] * wy) + mm[9] * wz) + mm[13]);
    c.z = (float)(((mm[2] * wx + mm[6] * wy) + mm[10] * wz) + mm[14]);
    c.w = (float)(((mm[3] * wx + mm[7] * wy) + mm[11] * wz) + mm[15]);
    a.clip[it] = c;
    a.mask[it] = (maskf >= 0.0f && maskf < 4294967296.0f) ? (uint32_t)maskf : 0u;  // (a NaN fails both)
    a.color[it] = color;
  }
}

// the ranks a view's nodes (and outlines) take: its first terrain rank
__device__ __forceinline__ uint64_t terrain_rank0(const uint64_t* view_seg, const uint64_t* seg_rank, uint32_t view) {
  return seg_rank[view_seg[view + 1]] - seg_rank[view_seg[view]];
}

constexpr uint32_t kTerrainPatch = 14;  // edge origins per patch side: 16 x 16 vertices in LDS, a rim of one vertex around them

// K_te: a workgroup per patch of 14 x 14 edge origins of one (view, layer), the grid strides over the patches. The patch's
// 16 x 16 vertices (one beyond it on every side; outside the window: mask 0) are staged in LDS, so the three edges of an
// origin and the four triangle tests that own them read LDS only. Then steps 15-16 and one atomicMin per fragment.
__global__ __launch_bounds__(256) void render_terrain_edges_kernel(RenderTerrainArgs a) {
  __shared__ float4 s_clip[256];
  __shared__ uint32_t s_mask[256];
  __shared__ uint32_t s_count[2];
  const uint32_t tid = threadIdx.x, lx = tid & 15u, lyy = tid >> 4;
  const uint32_t side = (a.Wn + kTerrainPatch - 1) / kTerrainPatch;
  const uint64_t per_vl = (uint64_t)side * side, patches = per_vl * a.L * a.nv, per = (uint64_t)a.Wn * a.Wn, plane = (uint64_t)a.W * a.H;
  for (uint64_t patch = blockIdx.x; patch < patches; patch += gridDim.x) {
    const uint32_t vl = (uint32_t)(patch / per_vl), pr = (uint32_t)(patch % per_vl);
    const uint32_t view = a.view0 + vl / a.L, layer = vl % a.L;
    if (a.view_status[view] != 0) continue;  // (the whole workgroup)
    const int32_t ax = (int32_t)((pr % side) * kTerrainPatch + lx) - 1, ay = (int32_t)((pr / side) * kTerrainPatch + lyy) - 1;
    const bool inside = ax >= 0 && ay >= 0 && ax < (int32_t)a.Wn && ay < (int32_t)a.Wn;
    const uint64_t at = (uint64_t)vl * per + (uint64_t)(inside ? ay : 0) * a.Wn + (uint64_t)(inside ? ax : 0);
    s_clip[tid] = inside ? a.clip[at] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s_mask[tid] = inside ? a.mask[at] : 0u;
    if (tid < 2) s_count[tid] = 0;
    __syncthreads();
    uint32_t submitted = 0, drawn = 0;
    if (inside && lx >= 1 && lx <= kTerrainPatch && lyy >= 1 && lyy <= kTerrainPatch) {
      const uint32_t m00 = s_mask[tid], m10 = s_mask[tid + 1], m01 = s_mask[tid + 16], m11 = s_mask[tid + 17];
      const bool t1 = (m00 & m10 & m01) != 0, t2 = (m10 & m01 & m11) != 0;
      const bool t2_below = (s_mask[tid - 15] & m00 & m10) != 0;  // T2 of quad (ax, ay - 1): (ax + 1, ay - 1) (ax, ay) (ax + 1, ay)
      const bool t2_left = (m00 & s_mask[tid + 15] & m01) != 0;   // T2 of quad (ax - 1, ay): (ax, ay) (ax - 1, ay + 1) (ax, ay + 1)
      const uint64_t first = terrain_rank0(a.view_seg, a.seg_rank, view) + (uint64_t)layer * 3 * per + 3 * ((uint64_t)ay * a.Wn + (uint64_t)ax);
      unsigned long long* keys = a.keys + (uint64_t)(view - a.view0) * plane;
      for (uint32_t kind = 0; kind < 3; ++kind) {  // H, V, D
        if (!(kind == 0 ? (t1 || t2_below) : kind == 1 ? (t1 || t2_left) : (t1 || t2))) continue;
        ++submitted;
        const float4 cp = s_clip[kind == 2 ? tid + 1 : tid], cq = s_clip[kind == 0 ? tid + 1 : tid + 16];
        const float p[4] = {cp.x, cp.y, cp.z, cp.w}, q[4] = {cq.x, cq.y, cq.z, cq.w};
        draw_segment<false>(
            p, q, a.half_w, a.half_h, a.W, a.H, 0, 0, [&]() { ++drawn; }, [&]() { return (unsigned long long)(uint32_t)(first + kind); },
            [&](unsigned long long rank, uint32_t gx, uint32_t gy, float zw, float, float, float) {
              atomicMin(keys + (uint64_t)(a.H - 1u - gy) * a.W + gx, ((unsigned long long)__float_as_uint(zw) << 32) | rank);
            });
      }
    }
    if (submitted) atomicAdd(&s_count[0], submitted);
    if (drawn) atomicAdd(&s_count[1], drawn);
    __syncthreads();  // (and the patch's vertices have been read for the last time)
    if (tid < 2 && s_count[tid]) atomicAdd(a.counters + 3 * ((uint64_t)view * a.L + layer) + tid, (unsigned long long)s_count[tid]);
    __syncthreads();  // the counts are read before the next patch clears them
  }
}

// Steps 16-17 again for the pixel (gx, gy from the lower left) that edge `e` of a window won: the colour of its fragment.
__device__ __forceinline__ uint32_t terrain_fragment_color(const RenderTerrainArgs& a, uint64_t window, uint32_t e, uint32_t gx, uint32_t gy) {
  const uint32_t kind = e % 3u, cell = e / 3u;
  const uint64_t v00 = window * ((uint64_t)a.Wn * a.Wn) + cell;
  const uint64_t from = kind == 2 ? v00 + 1 : v00, to = kind == 0 ? v00 + 1 : v00 + a.Wn;
  const float4 cp = a.clip[from], cq = a.clip[to];
  const float p[4] = {cp.x, cp.y, cp.z, cp.w}, q[4] = {cq.x, cq.y, cq.z, cq.w};
  const uint32_t c0 = a.color[from], c1 = a.color[to];
  uint32_t px = 0xff000000u;  // (kept only if the edge left no fragment here: never)
  draw_segment<true>(
      p, q, a.half_w, a.half_h, a.W, a.H, (int32_t)gx, (int32_t)gy, []() {}, []() { return 0; },
      [&](int, uint32_t, uint32_t, float, float t, float t_in, float t_out) {
        const float s = t_in + t * (t_out - t_in);
#pragma unroll
        for (uint32_t ch = 0; ch < 3; ++ch) {
          const float f0 = (float)((c0 >> (8u * ch)) & 255u), f1 = (float)((c1 >> (8u * ch)) & 255u);
          float v = f0 + s * (f1 - f0);
          if (!(v > 0.0f)) v = 0.0f;  // (a NaN too)
          if (v > 255.0f) v = 255.0f;
          px |= (uint32_t)(v + 0.5f) << (8u * ch);  // v + 0.5 >= 0: the conversion is floorf
        }
      });
  return px;
}

struct RenderResolveArgs {
  const unsigned long long* keys;  // the group's key planes
  uint64_t npix, plane;            // pixels of the group, of one view
  uint32_t view0;
  const uint64_t* view_seg;        // V + 1: first segment of each view
  const uint64_t* seg_pts;         // nseg + 1: points before each segment (over all views); with outlines: ranks, n + 1 per segment
  const uint32_t* seg_node;
  const BatchNode* nodes;
  const uint8_t* rgb;
  const uint8_t* lut;              // 256 entries (pcv_render_gamma_lut)
  uint32_t* image;                 // all views of the call
  float* depth;                    // all views of the call
  unsigned long long* covered;     // per view of the call
  unsigned long long* outlined;    // OUTLINE: per view of the call, the pixels an outline won
  uint32_t outline_px;             // OUTLINE: outline_rgba as the image stores it
};

// K_rr: a thread per pixel of the group. OUTLINE: the rank after a node's points is its outline's, in outline_px as given.
// TERRAIN: the ranks after the view's nodes are its layers' edges, 3 Wn^2 per layer; the colour is the fragment's, found by
// walking the edge again from the stored window vertices (no side buffer that fragments would race for)
template <bool OUTLINE, bool TERRAIN>
__device__ __forceinline__ void render_resolve_pixels(const RenderResolveArgs& a, const RenderTerrainArgs& terrain) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < a.npix; p += (uint64_t)gridDim.x * 256) {
    const uint32_t view = a.view0 + (uint32_t)(p / a.plane);
    const unsigned long long key = a.keys[p];
    const bool cov = key != kEmptyKey;
    bool box = false, ground = false;
    uint32_t px = 0xff000000u;  // (0, 0, 0, 255)
    uint32_t layer = 0;         // TERRAIN: of a pixel a layer won
    float zw = 1.0f;
    if (cov) {
      const uint64_t s0 = a.view_seg[view], s1 = a.view_seg[view + 1];
      if constexpr (TERRAIN) ground = (uint64_t)(uint32_t)key >= a.seg_pts[s1] - a.seg_pts[s0];
      if (ground) {
        const uint64_t per = 3ull * terrain.Wn * terrain.Wn, r = (uint64_t)(uint32_t)key - (a.seg_pts[s1] - a.seg_pts[s0]);
        const uint32_t q = (uint32_t)((p % a.plane) / terrain.W);
        layer = (uint32_t)(r / per);
        px = terrain_fragment_color(terrain, (uint64_t)(view - a.view0) * terrain.L + layer, (uint32_t)(r % per), (uint32_t)((p % a.plane) % terrain.W),
                                    terrain.H - 1u - q);
      } else {
        const uint64_t g = a.seg_pts[s0] + (uint32_t)key;  // the point's place among the points of all views
        uint64_t lo = s0, hi = s1;
        while (hi - lo > 1) {
          const uint64_t mid = (lo + hi) >> 1;
          if (a.seg_pts[mid] <= g) lo = mid;
          else hi = mid;
        }
        const BatchNode* nd = a.nodes + a.seg_node[lo];
        if constexpr (OUTLINE) box = g - a.seg_pts[lo] == nd->n;
        if (box) {
          px = a.outline_px;
        } else {
          const uint8_t* c = a.rgb + 3 * (nd->point_off + (g - a.seg_pts[lo]));
          px = (uint32_t)a.lut[c[0]] | (uint32_t)a.lut[c[1]] << 8 | (uint32_t)a.lut[c[2]] << 16 | 0xff000000u;
        }
      }
      zw = __uint_as_float((uint32_t)(key >> 32));
    }
    const uint64_t at = (uint64_t)a.view0 * a.plane + p;
    a.image[at] = px;
    a.depth[at] = zw;
    // covered pixels per view: one add per wave where the wave's pixels are of one view
    const unsigned long long act = __ballot(true), cv = __ballot(cov);
    const uint32_t v0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)view);
    const bool one_view = __ballot(view == v0) == act;
    if (one_view) {
      if (cv && lane == (uint32_t)(__ffsll(act) - 1)) atomicAdd(a.covered + v0, (unsigned long long)__popcll(cv));
    } else if (cov) {
      atomicAdd(a.covered + view, 1ull);
    }
    if constexpr (TERRAIN) {  // the pixels each layer won: one add per wave for the layer of the wave's first such pixel
      const unsigned long long gm = __ballot(ground);
      if (gm) {
        const uint32_t slot = view * terrain.L + layer, first = (uint32_t)(__ffsll(gm) - 1);
        const uint32_t slot0 = (uint32_t)__shfl((int)slot, (int)first);
        const unsigned long long same = __ballot(ground && slot == slot0);
        if (ground && slot != slot0) atomicAdd(terrain.counters + 3 * (uint64_t)slot + 2, 1ull);
        else if (lane == first) atomicAdd(terrain.counters + 3 * (uint64_t)slot0 + 2, (unsigned long long)__popcll(same));
      }
    }
    if constexpr (OUTLINE) {  // the pixels an outline won, counted the same way
      const unsigned long long bx = __ballot(box);
      if (one_view) {
        if (bx && lane == (uint32_t)(__ffsll(act) - 1)) atomicAdd(a.outlined + v0, (unsigned long long)__popcll(bx));
      } else if (box) {
        atomicAdd(a.outlined + view, 1ull);
      }
    }
  }
}

template <bool OUTLINE>
__global__ __launch_bounds__(256) void render_resolve_kernel(RenderResolveArgs a) {
  render_resolve_pixels<OUTLINE, false>(a, RenderTerrainArgs{});
}

// K_rr over a frame with terrain layers: `t` holds the group's windows and the per-layer counters
template <bool OUTLINE>
__global__ __launch_bounds__(256) void render_resolve_terrain_kernel(RenderResolveArgs a, RenderTerrainArgs t) {
  render_resolve_pixels<OUTLINE, true>(a, t);
}

struct ViewInfo {
  int32_t status = 0;
  uint32_t nodes_visible = 0, nodes_drawn = 0;
  uint64_t points_submitted = 0, points_drawn = 0, pixels_covered = 0;
  uint64_t segments_submitted = 0, segments_drawn = 0, outline_pixels = 0;  // show_octree_nodes
};

struct TerrainViewInfo {  // per (view, layer)
  int64_t pos[2] = {0, 0};
  uint64_t edges_submitted = 0, edges_drawn = 0, pixels_won = 0;
};

constexpr uint64_t kTerrainVertexBytes = 24;  // a window vertex: f32 clip point, mask, colour

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
  uint32_t L = 0;  // terrain layers
  std::vector<TerrainViewInfo> terrain_info;  // V x L
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

static int render_views(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* p,
                        const pcv_render_overlay* overlay, const pcv_render_terrain_layers* terrain, pcv_render* r) {
  const bool outline = overlay && (overlay->flags & PCV_RENDER_OUTLINE_NODES);
  const uint32_t V = frusta->count, W = p->width, H = p->height;
  const uint32_t L = terrain ? terrain->num_layers : 0, Wn = L ? terrain->window : 0;
  const uint64_t plane = (uint64_t)W * H, window_vertices = (uint64_t)Wn * Wn;
  r->V = V;
  r->W = W;
  r->H = H;
  r->L = L;
  r->info.assign(V, ViewInfo());
  r->terrain_info.assign((size_t)V * L, TerrainViewInfo());
  if (V == 0) return PCV_OK;
  // the key planes of one group of views, and with terrain the group's window vertices, are the workspace; a single view
  // over the limit is refused before anything is allocated
  const uint64_t workspace = p->max_workspace_bytes ? p->max_workspace_bytes : kDefaultWorkspace;
  const uint64_t view_bytes = 8 * plane + (uint64_t)L * window_vertices * kTerrainVertexBytes;  // < 2^32 L
  const uint64_t group_views = std::min<uint64_t>(V, workspace / view_bytes);
  if (group_views == 0)
    return ctx->fail(PCV_E_OOM, L ? "render: the key plane and the terrain windows of one view exceed max_workspace_bytes"
                                  : "render: the key plane of one view exceeds max_workspace_bytes");
  if (3 * window_vertices * L >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "render: a view's terrain edges take 2^32 - 1 draw ranks or more");
  // step 13: every view's window over every layer
  std::vector<PcvTerrainLayerView> layer_view(L);
  std::vector<int64_t> window_pos((size_t)V * L * 2, 0);
  for (uint32_t k = 0; k < L; ++k) {
    if (int lrc = pcv_terrain_layer_view(terrain->layers[k], ctx, &layer_view[k])) return lrc;
    for (uint32_t v = 0; v < V; ++v) {
      int64_t* pos = &window_pos[2 * ((size_t)v * L + k)];
      if (!pcv_terrain_window_pos(layer_view[k].grid, terrain->camera_positions + 3 * (size_t)v, Wn, pos))
        return ctx->fail(PCV_E_INVALID, "Terrain location not representable.");
      r->terrain_info[(size_t)v * L + k].pos[0] = pos[0], r->terrain_info[(size_t)v * L + k].pos[1] = pos[1];
    }
  }
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
  // with outlines a node owns n + 1 ranks (its points, then its outline): seg_pts then counts ranks, not points
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
        seg_pts.push_back(seg_pts.back() + n + (outline ? 1 : 0));
        vi.points_submitted += n;
        if (outline) vi.segments_submitted += 12;
      }
      if (vi.points_submitted >= 0xffffffffull) return ctx->fail(PCV_E_INVALID, "render: a view draws 2^32 - 1 points or more");
      if (vi.points_submitted + vi.segments_submitted / 12 >= 0xffffffffull)
        return ctx->fail(PCV_E_INVALID, "render: a view's points and node outlines take 2^32 - 1 draw ranks or more");
      if (vi.points_submitted + vi.segments_submitted / 12 + 3 * window_vertices * L >= 0xffffffffull)
        return ctx->fail(PCV_E_INVALID, "render: a view's points, node outlines and terrain edges take 2^32 - 1 draw ranks or more");
    }
    view_seg[v + 1] = seg_node.size();
    view_chunk[v + 1] = seg_chunk.back();
  }
  const uint64_t nseg = seg_node.size(), nchunks = seg_chunk.back();
  // 3. the images of all views, and the scratch
  if ((rc = ctx->dev_alloc((void**)&r->d_images, 4 * plane * V)) || (rc = ctx->dev_alloc((void**)&r->d_depth, 4 * plane * V))) return rc;
  PcvScratch sc(ctx);
  const size_t ncounters = outline ? 4 : 2;  // per view: points drawn, pixels covered; segments drawn, outline pixels
  unsigned long long *d_keys, *d_counters;
  uint8_t* d_lut;
  uint32_t *d_seg_node, *d_seg_view;
  uint64_t *d_seg_chunk, *d_seg_pts, *d_view_seg;
  ChunkDesc* d_desc;
  if ((rc = sc.get(&d_keys, group_views * plane)) || (rc = sc.get(&d_counters, ncounters * (size_t)V)) || (rc = sc.get(&d_lut, 256)) ||
      (rc = sc.get(&d_seg_node, std::max<uint64_t>(nseg, 1))) || (rc = sc.get(&d_seg_view, std::max<uint64_t>(nseg, 1))) ||
      (rc = sc.get(&d_seg_chunk, nseg + 1)) || (rc = sc.get(&d_seg_pts, nseg + 1)) || (rc = sc.get(&d_view_seg, (size_t)V + 1)) ||
      (rc = sc.get(&d_desc, std::max<uint64_t>(nchunks, 1))))
    return rc;
  RenderTerrainArgs ta{};
  if (L) {
    TerrainLayerDev* d_layers;
    int64_t* d_pos;
    uint32_t* d_status;
    float4* d_clip;
    uint32_t *d_mask, *d_color;
    unsigned long long* d_tcounters;
    const uint64_t nvert = group_views * L * window_vertices;
    if ((rc = sc.get(&d_layers, L)) || (rc = sc.get(&d_pos, window_pos.size())) || (rc = sc.get(&d_status, V)) || (rc = sc.get(&d_clip, nvert)) ||
        (rc = sc.get(&d_mask, nvert)) || (rc = sc.get(&d_color, nvert)) || (rc = sc.get(&d_tcounters, 3 * (size_t)V * L)))
      return rc;
    std::vector<TerrainLayerDev> layers(L);
    for (uint32_t k = 0; k < L; ++k) {
      layers[k].grid = layer_view[k].grid;
      layers[k].ntiles = layer_view[k].ntiles;
      layers[k].tile_keys = layer_view[k].d_tile_keys;
      layers[k].heights = layer_view[k].d_heights;
      layers[k].colors = layer_view[k].d_colors;
      layers[k].T = layer_view[k].T;
      layers[k].pad = 0;
    }
    std::vector<uint32_t> view_status(V);
    for (uint32_t v = 0; v < V; ++v) view_status[v] = (uint32_t)status[v];
    // pageable sources: the copies have left the vectors when the calls return
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_layers, layers.data(), sizeof(TerrainLayerDev) * L, hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_pos, window_pos.data(), 8 * window_pos.size(), hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_status, view_status.data(), 4 * (size_t)V, hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemsetAsync(d_tcounters, 0, 8 * 3 * (size_t)V * L, ctx->stream));
    ta.layers = d_layers;
    ta.pos = d_pos;
    ta.view_status = d_status;
    ta.shapes = frusta->dev;
    ta.view_seg = d_view_seg;
    ta.seg_rank = d_seg_pts;
    ta.clip = d_clip;
    ta.mask = d_mask;
    ta.color = d_color;
    ta.keys = d_keys;
    ta.counters = d_tcounters;
    ta.L = L;
    ta.Wn = Wn;
    ta.W = W;
    ta.H = H;
    ta.half_w = 0.5f * (float)W;
    ta.half_h = 0.5f * (float)H;
  }
  uint8_t lut[256];
  if ((rc = pcv_render_gamma_lut(p->gamma, lut))) return ctx->fail(rc, "render: gamma");
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_lut, lut, 256, hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemsetAsync(d_counters, 0, 8 * ncounters * (size_t)V, ctx->stream));
  if (nseg) {
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_node, seg_node.data(), 4 * nseg, hipMemcpyHostToDevice, ctx->stream));
    PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_view, seg_view.data(), 4 * nseg, hipMemcpyHostToDevice, ctx->stream));
  }
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_chunk, seg_chunk.data(), 8 * (nseg + 1), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_seg_pts, seg_pts.data(), 8 * (nseg + 1), hipMemcpyHostToDevice, ctx->stream));
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(d_view_seg, view_seg.data(), 8 * ((size_t)V + 1), hipMemcpyHostToDevice, ctx->stream));
  const BatchNode* d_nodes = pcv_octree_query_nodes(tree);
  // grids of resident size that stride over chunks / pixels: no dispatch grows with V or with the node count
  int splat_grid = 1, resolve_grid = 1, chunks_grid = 1, outline_grid = 1, gather_grid = 1, edges_grid = 1;
  const void* resolve = L ? (outline ? (const void*)render_resolve_terrain_kernel<true> : (const void*)render_resolve_terrain_kernel<false>)
                          : (outline ? (const void*)render_resolve_kernel<true> : (const void*)render_resolve_kernel<false>);
  if ((rc = resident_grid(ctx, (const void*)render_splat_kernel, &splat_grid)) || (rc = resident_grid(ctx, resolve, &resolve_grid)) ||
      (rc = resident_grid(ctx, (const void*)render_chunks_kernel, &chunks_grid)) ||
      (outline && (rc = resident_grid(ctx, (const void*)render_outline_kernel, &outline_grid))) ||
      (L && ((rc = resident_grid(ctx, (const void*)render_terrain_gather_kernel, &gather_grid)) ||
             (rc = resident_grid(ctx, (const void*)render_terrain_edges_kernel, &edges_grid)))))
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
  RenderOutlineArgs oa{};
  if (outline) {
    const uint8_t* c = overlay->outline_rgba;
    ra.outline_px = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;  // as given: no gamma
    ra.outlined = d_counters + 3 * (size_t)V;
    oa.seg_node = d_seg_node;
    oa.seg_view = d_seg_view;
    oa.seg_rank = d_seg_pts;
    oa.view_seg = d_view_seg;
    oa.nodes = d_nodes;
    oa.shapes = frusta->dev;
    oa.keys = d_keys;
    oa.seg_drawn = d_counters + 2 * (size_t)V;
    oa.W = W;
    oa.H = H;
    oa.half_w = sa.half_w;
    oa.half_h = sa.half_h;
  }
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
    oa.s0 = view_seg[v0];
    oa.s1 = view_seg[v0 + nv];
    oa.view0 = v0;
    if (outline && oa.s1 > oa.s0) {  // after the group's points, before its pixels are resolved
      PcvProf prof(ctx, PCV_K_RENDER_OUTLINE);
      hipLaunchKernelGGL(render_outline_kernel, dim3((uint32_t)std::min<uint64_t>(((oa.s1 - oa.s0) * 12 + 255) / 256, (uint64_t)outline_grid)),
                         dim3(256), 0, ctx->stream, oa);
      PCV_HIP_CHECK(ctx, hipGetLastError());
    }
    if (L) {  // after the group's points and outlines: the windows, then their edges
      ta.view0 = v0;
      ta.nv = nv;
      const uint64_t side = (Wn + kTerrainPatch - 1) / kTerrainPatch;
      {
        PcvProf prof(ctx, PCV_K_RENDER_TERRAIN_GATHER);
        hipLaunchKernelGGL(render_terrain_gather_kernel, dim3((uint32_t)std::min<uint64_t>((window_vertices * L * nv + 255) / 256, (uint64_t)gather_grid)),
                           dim3(256), 0, ctx->stream, ta);
        PCV_HIP_CHECK(ctx, hipGetLastError());
      }
      {
        PcvProf prof(ctx, PCV_K_RENDER_TERRAIN_EDGES);
        hipLaunchKernelGGL(render_terrain_edges_kernel, dim3((uint32_t)std::min<uint64_t>(side * side * L * nv, (uint64_t)edges_grid)), dim3(256), 0,
                           ctx->stream, ta);
        PCV_HIP_CHECK(ctx, hipGetLastError());
      }
    }
    ra.npix = plane * nv;
    ra.view0 = v0;
    {
      PcvProf prof(ctx, PCV_K_RENDER_RESOLVE);
      const dim3 grid((uint32_t)std::min<uint64_t>((ra.npix + 255) / 256, (uint64_t)resolve_grid));
      if (L && outline) hipLaunchKernelGGL(render_resolve_terrain_kernel<true>, grid, dim3(256), 0, ctx->stream, ra, ta);
      else if (L) hipLaunchKernelGGL(render_resolve_terrain_kernel<false>, grid, dim3(256), 0, ctx->stream, ra, ta);
      else if (outline) hipLaunchKernelGGL(render_resolve_kernel<true>, grid, dim3(256), 0, ctx->stream, ra);
      else hipLaunchKernelGGL(render_resolve_kernel<false>, grid, dim3(256), 0, ctx->stream, ra);
      PCV_HIP_CHECK(ctx, hipGetLastError());
    }
  }
  std::vector<unsigned long long> h_counters(ncounters * (size_t)V);
  PCV_HIP_CHECK(ctx, hipMemcpyAsync(h_counters.data(), d_counters, 8 * ncounters * (size_t)V, hipMemcpyDeviceToHost, ctx->stream));
  std::vector<unsigned long long> h_tcounters(3 * (size_t)V * L);
  if (L) PCV_HIP_CHECK(ctx, hipMemcpyAsync(h_tcounters.data(), ta.counters, 8 * h_tcounters.size(), hipMemcpyDeviceToHost, ctx->stream));
  PCV_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // the scratch is released on return
  for (size_t k = 0; k < (size_t)V * L; ++k) {
    r->terrain_info[k].edges_submitted = h_tcounters[3 * k];
    r->terrain_info[k].edges_drawn = h_tcounters[3 * k + 1];
    r->terrain_info[k].pixels_won = h_tcounters[3 * k + 2];
  }
  for (uint32_t v = 0; v < V; ++v) {
    r->info[v].points_drawn = h_counters[v];
    r->info[v].pixels_covered = h_counters[(size_t)V + v];
    if (outline) {
      r->info[v].segments_drawn = h_counters[2 * (size_t)V + v];
      r->info[v].outline_pixels = h_counters[3 * (size_t)V + v];
    }
  }
  return PCV_OK;
}

static const char* overlay_error(const pcv_render_overlay* o) {
  if (o && (o->flags & ~(uint32_t)PCV_RENDER_OUTLINE_NODES)) return "render: unknown overlay flag bits (only PCV_RENDER_OUTLINE_NODES is defined)";
  return nullptr;
}

extern "C" int pcv_render_check_overlay(const pcv_render_overlay* overlay, char* message, uint64_t capacity) {
  const char* why = overlay_error(overlay);
  if (message && capacity) snprintf(message, (size_t)capacity, "%s", why ? why : "");
  return why ? PCV_E_INVALID : PCV_OK;
}

extern "C" int pcv_render_views(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* params, pcv_render** out) {
  return pcv_render_views_ex(ctx, frusta, tree, params, nullptr, out);
}

extern "C" int pcv_render_views_ex(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* params,
                                   const pcv_render_overlay* overlay, pcv_render** out) {
  return pcv_render_views_terrain(ctx, frusta, tree, params, overlay, nullptr, out);
}

static const char* terrain_error(const pcv_render_terrain_layers* t) {
  if (!t || t->num_layers == 0) return nullptr;
  if (t->window < 2 || t->window > PCV_RENDER_TERRAIN_WINDOW || (t->window & 1u)) return "render: the terrain window must be even and in 2 ..= 1024";
  if (!t->layers) return "render: null terrain layer array";
  for (uint32_t k = 0; k < t->num_layers; ++k)
    if (!t->layers[k]) return "render: a terrain layer is null";
  if (!t->camera_positions) return "render: terrain layers need the camera positions of the views";
  return nullptr;
}

extern "C" int pcv_render_check_terrain_host(const pcv_render_terrain_layers* terrain, char* message, uint64_t capacity) {
  const char* why = terrain_error(terrain);
  if (message && capacity) snprintf(message, (size_t)capacity, "%s", why ? why : "");
  return why ? PCV_E_INVALID : PCV_OK;
}

extern "C" int pcv_render_views_terrain(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* params,
                                        const pcv_render_overlay* overlay, const pcv_render_terrain_layers* terrain, pcv_render** out) {
  if (!ctx) return PCV_E_INVALID;
  if (!frusta || !tree || !params || !out) return ctx->fail(PCV_E_INVALID, "null argument");
  *out = nullptr;
  if (const char* why = overlay_error(overlay)) return ctx->fail(PCV_E_INVALID, why);
  if (const char* why = terrain_error(terrain)) return ctx->fail(PCV_E_INVALID, why);
  if (pcv_render_check_params(params) != PCV_OK)
    return ctx->fail(PCV_E_INVALID, "render: width and height in 1 ..= 16384, point_size in 1 ..= 64, gamma finite and > 0");
  if (frusta->ctx != ctx || tree->ctx != ctx) return ctx->fail(PCV_E_INVALID, "render: shapes and octree must belong to the context");
  if (frusta->count >= (1u << kBatchShapeBits)) return ctx->fail(PCV_E_INVALID, "render: at most 2^24 - 1 views");
  for (int32_t kind : frusta->kinds)
    if (kind != PCV_SHAPE_FRUSTUM && kind != PCV_SHAPE_FRUSTUM_WITH_INVERSE) return ctx->fail(PCV_E_INVALID, "render: every shape must be a frustum");
  pcv_render* r = new pcv_render();
  r->ctx = ctx;
  const int rc = render_views(ctx, frusta, tree, params, overlay, terrain && terrain->num_layers ? terrain : nullptr, r);
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

extern "C" int pcv_render_outline_info(pcv_render* r, uint32_t view, uint64_t* segments_submitted, uint64_t* segments_drawn,
                                       uint64_t* outline_pixels) {
  if (!r) return PCV_E_INVALID;
  if (view >= r->V) return r->ctx->fail(PCV_E_INVALID, "render: view past the end");
  const ViewInfo& vi = r->info[view];
  if (segments_submitted) *segments_submitted = vi.segments_submitted;
  if (segments_drawn) *segments_drawn = vi.segments_drawn;
  if (outline_pixels) *outline_pixels = vi.outline_pixels;
  return PCV_OK;
}

extern "C" int pcv_render_terrain_info(pcv_render* r, uint32_t view, uint32_t layer, int64_t pos[2], uint64_t* edges_submitted,
                                       uint64_t* edges_drawn, uint64_t* pixels_won) {
  if (!r) return PCV_E_INVALID;
  if (view >= r->V || layer >= r->L) return r->ctx->fail(PCV_E_INVALID, "render: view or terrain layer past the end");
  const TerrainViewInfo& ti = r->terrain_info[(size_t)view * r->L + layer];
  if (pos) pos[0] = ti.pos[0], pos[1] = ti.pos[1];
  if (edges_submitted) *edges_submitted = ti.edges_submitted;
  if (edges_drawn) *edges_drawn = ti.edges_drawn;
  if (pixels_won) *pixels_won = ti.pixels_won;
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
