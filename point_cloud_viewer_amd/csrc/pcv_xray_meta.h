// pcv_xray_meta.h — the meta*.pb of an xray quadtree directory (xray_proto Meta) and the node file names, written and read.
// Standard C++ only: the directory writers and pcv_xray_open_dir (pcv_xray_files.hip) use it, and a stand-alone driver
// runs it under the sanitizers (tests/xray_meta_driver.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

// shared between the xray sources, not part of the library's interface
#define PCV_XRAY_LOCAL __attribute__((visibility("hidden")))

constexpr uint32_t kMaxTilePx = 1u << 15;  // tile edge of a run and of a meta file

struct XrayMeta {
  int32_t version = 0;
  bool has_min = false;
  double min[2] = {0, 0}, edge = 0;   // Rect.min, Rect.edge_length
  float dmin[2] = {0, 0}, dedge = 0;  // the deprecated f32 fields (version 2 files)
  uint32_t deepest_level = 0, tile_size = 0;
  std::vector<std::pair<uint32_t, uint64_t>> nodes;  // (level, index)
};

// NodeId Display (quadtree/src/lib.rs:218-234): "r" and one digit per level
PCV_XRAY_LOCAL std::string quad_name(uint32_t level, uint64_t index);
// get_meta_pb_path: the root id with "r" -> "meta", + ".pb"
PCV_XRAY_LOCAL std::string xray_meta_name(uint32_t root_level, uint64_t root_index);
// the bytes of a Meta of CURRENT_VERSION 3: m's min, edge, deepest_level, tile_size and nodes in their order
PCV_XRAY_LOCAL std::vector<uint8_t> xray_meta_encode(const XrayMeta& m);
// Meta::from_proto's wire format; false: not a Meta message
PCV_XRAY_LOCAL bool parse_meta(const std::vector<uint8_t>& data, XrayMeta* m);
// what a parsed Meta must hold before a handle is made of it: empty, or the message that follows the file's path
PCV_XRAY_LOCAL std::string xray_meta_check(const XrayMeta& m);
