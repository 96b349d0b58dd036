// pcv_xray_obj.h — the xray quadtree handle as its sources share it: pcv_xray.hip (leaf level, the handle's life),
// pcv_xray_pyramid.hip (parent levels, merge), pcv_xray_inpaint.hip (hole filling) and pcv_xray_files.hip (node images and
// files of any kind of quadtree).
#pragma once
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "pcv_internal.h"
#include "pcv_xray_meta.h"

constexpr uint32_t kBlk = 32;  // pixel block edge: one accumulation / resize workgroup per (tile, 32 x 32 pixels)

struct PCV_XRAY_LOCAL LeafGeometry {
  double rect[3];  // bounding rect: min x, min y, edge
  uint32_t deepest_level;
  double bbox_min[3], bbox_max[3];  // get_bounding_box
  std::vector<uint64_t> index;      // leaf node indices at deepest_level, get_nodes_at_level order
  std::vector<double> rect_min;     // 2 per leaf
  double leaf_edge;
};

// kXrayInpainted (pcv_xray_inpaint): owns leaf and parent images like a built quadtree (d_images, d_parents, created =
// 0 .. n - 1) and carries its node list and its root's rect like an opened one
enum XrayKind : uint32_t { kXrayBuilt = 0, kXrayOpened = 1, kXrayMerged = 2, kXrayInpainted = 3 };

struct XrayPartRef {  // one part of a merged quadtree: its nodes are [first, first + count) of the merged node list
  pcv_xray* part;
  uint64_t serial, first, count;
};

struct pcv_xray {
  pcv_xray();   // enters the registry of live objects (pcv_xray.hip) under a serial number of its own
  ~pcv_xray();  // leaves it
  uint64_t serial = 0;
  XrayKind kind = kXrayBuilt;
  // opened (pcv_xray_open_dir) and merged (pcv_xray_merge) quadtrees: the node list itself; of `geo` only deepest_level
  // and rect are set (the meta's bounding rect), geo.index / created list the nodes at deepest_level
  std::vector<uint32_t> node_level;
  std::vector<uint64_t> node_index;
  uint64_t root_count = 0;   // nodes at the minimum level (a merge needs exactly one, or no node at all)
  std::string dir;           // opened: the directory the PNGs are read from
  std::vector<XrayPartRef> parts;  // merged; the new levels follow the parts' nodes and live in d_parents
  pcv_ctx* ctx = nullptr;    // null: opened without a context (host only)
  uint32_t W = 0;
  LeafGeometry geo;
  uint32_t root_level = 0;
  uint64_t root_index = 0;
  uint32_t bg = 0;                // tile_background_color.to_u8(), packed RGBA8
  std::vector<uint64_t> created;  // positions in the leaf list
  std::vector<uint64_t> kept, drawn;
  std::vector<uint64_t> negative;  // colored_with_intensity: kept points with intensity < 0 per created tile
  uint32_t* d_images = nullptr;
  // parent levels (pcv_xray_build_parents): the node list after the created leaves, deepest - 1 up to root_level, each
  // level in ascending index; level_first[k] is the first parent of level deepest - 1 - k in that list
  bool parents_built = false;
  std::vector<uint32_t> parent_level;
  std::vector<uint64_t> parent_index;
  std::vector<uint64_t> level_first;
  uint32_t* d_parents = nullptr;
  // inpainted (pcv_xray_inpaint_info): per leaf, within the final tile
  std::vector<uint64_t> inpaint_target, inpaint_filled, inpaint_blended;
};

// Every live pcv_xray is known by address with its serial number: a merged quadtree refers to its parts, and asks here
// whether a part is still the object it was given before it touches it
PCV_XRAY_LOCAL bool xray_is_live(const pcv_xray* x);
PCV_XRAY_LOCAL bool xray_part_alive(const XrayPartRef& r);

// a failure on a handle that may have no context (opened host only): the message goes where the caller can read it
PCV_XRAY_LOCAL inline int xray_fail(const pcv_xray* x, int code, const std::string& msg) { return x->ctx ? x->ctx->fail(code, msg) : pcv_host_fail(code, msg); }
PCV_XRAY_LOCAL inline int xray_not_built(const pcv_xray* x, const char* what) {
  return xray_fail(x, PCV_E_INVALID, std::string("xray: ") + what + " needs a quadtree built by pcv_xray_run, not an opened, merged or inpainted one");
}
// the node images live on the device in d_images (leaves) and d_parents: built and inpainted quadtrees
PCV_XRAY_LOCAL inline bool xray_owns_tiles(const pcv_xray* x) { return x->kind == kXrayBuilt || x->kind == kXrayInpainted; }

// The node list of any kind of quadtree: a built one's created leaves then its parents, an opened or merged one's own list
struct XrayNodeId {
  uint32_t level;
  uint64_t index;
};
PCV_XRAY_LOCAL inline uint64_t xray_num_nodes(const pcv_xray* x) {
  return x->kind == kXrayBuilt ? x->created.size() + x->parent_index.size() : x->node_index.size();
}
PCV_XRAY_LOCAL inline XrayNodeId xray_node_id(const pcv_xray* x, uint64_t i) {
  if (x->kind != kXrayBuilt) return {x->node_level[i], x->node_index[i]};
  const uint64_t nc = x->created.size();
  return i < nc ? XrayNodeId{x->geo.deepest_level, x->geo.index[x->created[i]]} : XrayNodeId{x->parent_level[i - nc], x->parent_index[i - nc]};
}

// root_node.bounding_rect of a built quadtree: Node::from_node_id_and_root_bounding_rect(root_node_id, rect), what its
// meta file holds
PCV_XRAY_LOCAL inline void built_root_rect(const pcv_xray* x, double rect[3]) {
  std::memcpy(rect, x->geo.rect, sizeof(x->geo.rect));
  for (int l = (int)x->root_level - 1; l >= 0; --l) {
    const uint32_t ci = (uint32_t)(x->root_index >> (2 * l)) & 3u;
    const double half = rect[2] / 2.0;
    if (ci & 1u) rect[1] += half;
    if (ci & 2u) rect[0] += half;
    rect[2] = half;
  }
}

// pcv_xray_pyramid.hip. The levels above a set of nodes: the node list after them (plevel, pindex; first[k] = the first
// parent of level from - 1 - k in it) and their images on the device
struct XrayLevels {
  std::vector<uint32_t> plevel;
  std::vector<uint64_t> pindex, first;
  uint32_t* d_parents = nullptr;
};
// the number of nodes create_non_leaf_nodes(base, from, to) makes
PCV_XRAY_LOCAL uint64_t xray_count_levels(const std::vector<uint64_t>& base, uint32_t from, uint32_t to);
// create_non_leaf_nodes(base, from, to) for the nodes `base` of level `from` (node positions 0 .. base.size() - 1, their
// images at d_base), one xray_parent_kernel launch per level under the kernel-stat id `prof_id`. images: null (the parent
// images are allocated here, before any launch, and freed on failure) or the caller's block of xray_count_levels tiles
PCV_XRAY_LOCAL int xray_build_levels(pcv_ctx* ctx, uint32_t W, uint32_t bg, const std::vector<uint64_t>& base, uint32_t from, uint32_t to,
                                     const uint32_t* d_base, int prof_id, uint32_t* images, XrayLevels* out);

// pcv_xray_files.hip, for the merge's staging of root tiles (pcv_xray_pyramid.hip)
// node images [first, first + count) of a built quadtree's node list into dst (host or device), no synchronisation
PCV_XRAY_LOCAL int queue_node_images(pcv_xray* x, uint64_t first, uint64_t count, uint8_t* dst, hipMemcpyKind kind);
// node `node` of an opened quadtree, decoded from its file into W x W x 4 host bytes
PCV_XRAY_LOCAL int opened_node_to_host(const pcv_xray* x, uint64_t node, uint8_t* dst);
// node images of any kind of quadtree into checked arguments; returns after the copies have completed
PCV_XRAY_LOCAL int xray_node_images(pcv_xray* x, uint64_t first, uint64_t count, int mem, uint8_t* rgba);

// pcv_xray_files.hip, the writer of device tiles as the map tiles use it too (pcv_maptiles.hip)
// takes the finished file of tile i; false: it could not be kept (PCV_E_IO). May be called from several threads at once where
// xray_tile_files is asked to work in parallel
using XrayFileSink = std::function<bool(uint64_t i, const uint8_t* file, uint64_t len)>;
// names the device tiles [f, f + c): tile i of them is a + i * 4 W W for i < na and b + (i - na) * 4 W W after that
using XrayTileSrc = std::function<void(uint64_t f, uint64_t c, const uint8_t** a, uint64_t* na, const uint8_t** b)>;
// `count` W x W device tiles encoded in `mode` (PCV_XRAY_PNG_STORED / _DEFLATE), a chunk of pcv_ctx_set_xray_chunk_bytes at a
// time through two pinned buffers; while chunk k + 1 is on its way, up to 8 host threads (`parallel`; else the caller, in
// order) wrap chunk k and hand each file to the sink
PCV_XRAY_LOCAL int xray_tile_files(pcv_ctx* ctx, uint32_t W, uint64_t count, int mode, bool parallel, const XrayTileSrc& src, const XrayFileSink& sink);
