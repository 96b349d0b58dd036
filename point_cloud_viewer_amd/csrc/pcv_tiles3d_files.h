// pcv_tiles3d_files.h — the 3D Tiles export, the part that needs no device: the parameter rules, the plan of a
// .pnts file (sizes, section offsets, its header and JSON bytes), the file made on the host, and the tileset walk over a node
// table. Plain C++ without a HIP type: tests/tiles3d_host_driver.cpp runs it under the host sanitizers.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pcv_hip.h"

constexpr uint64_t kPcvTiles3dHeaderBytes = 28;

// One .pnts file as far as it does not depend on the points' bytes.
struct PcvTiles3dFilePlan {
  uint32_t mode = 0;        // PCV_TILES3D_POS_QUANTIZED or _FLOAT
  uint32_t encoding = 0;    // the node's PCV_ENC_*
  uint32_t src_stride = 0;  // bytes of a point in the node's .xyz
  uint32_t dst_stride = 0;  // bytes of a point's position in the feature binary: 6 or 12
  bool intensity = false;
  uint64_t n = 0;
  double rc[3] = {0, 0, 0};
  std::string head;         // the 28-byte header and the feature JSON with its padding: bytes [0, feature_binary_offset)
  std::string batch_json;   // with its padding; empty without intensity
  uint64_t feature_binary_offset = 0, feature_binary_bytes = 0;  // the length with padding; positions, then colours, then zeros
  uint64_t batch_json_offset = 0;
  uint64_t batch_binary_offset = 0, batch_binary_bytes = 0;
  uint64_t file_bytes = 0;
};

// "r" and one octal digit per level (NodeId Display, src/octree/node.rs:73-86)
std::string pcv_tiles3d_node_name(const pcv_node_info& n);
int pcv_tiles3d_check_params(const pcv_tiles3d_params* p, std::string* why);
// has_intensity: the source carries intensity (PCV_TILES3D_INTENSITY without it is refused). PCV_E_INVALID with *why else.
int pcv_tiles3d_file_plan(const pcv_node_info& node, const pcv_tiles3d_params& p, bool has_intensity, PcvTiles3dFilePlan* out, std::string* why);
void pcv_tiles3d_fill_tile(const PcvTiles3dFilePlan& f, uint64_t node, pcv_tiles3d_tile* out);
// The whole file from the node's host bytes (intensity: null unless the plan has it): the device's twin.
void pcv_tiles3d_build_file(const pcv_node_info& node, const PcvTiles3dFilePlan& f, const uint8_t* xyz, const uint8_t* rgb, const float* intensity,
                            std::vector<uint8_t>* out);
// tileset.json of `count` nodes in (level, index) order. kinds (nullable): per node 0 = left out, 1 = a tile without content,
// 2 = a tile with content. PCV_E_INVALID with *why: an unordered table, a node without its parent, no point at all.
int pcv_tiles3d_tileset(const pcv_node_info* nodes, uint64_t count, const pcv_tiles3d_params& p, std::string* json, std::vector<uint8_t>* kinds,
                        std::string* why);

// What pcv_tiles3d_tile_host and pcv_tiles3d_tileset_json_host do once their message has a place to go: *len the whole length,
// out / buf (nullable) takes min(capacity, *len) bytes.
int pcv_tiles3d_tile_into(const pcv_node_info* node, const pcv_tiles3d_params* params, const uint8_t* xyz, const uint8_t* rgb, const float* intensity,
                          uint8_t* out, uint64_t capacity, uint64_t* len, pcv_tiles3d_tile* tile, std::string* why);
int pcv_tiles3d_tileset_into(const pcv_node_info* nodes, uint64_t count, const pcv_tiles3d_params* params, char* buf, uint64_t cap, uint64_t* len,
                             std::string* why);

// Whole files grouped into pieces of at most chunk_bytes, in order: piece k holds files [first[k], first[k + 1]).
std::vector<uint64_t> pcv_tiles3d_pieces(const std::vector<uint64_t>& file_bytes, uint64_t chunk_bytes);
