// pcv_tiles3d_files.cpp — the 3D Tiles export without the device (the contract is stated in include/pcv_hip.h):
// parameter rules, the plan and the host build of one .pnts file, the tileset walk over the (level, index)-ordered node table,
// and the grouping of files into pieces. The positions go through pcv_tiles3d_dev.h, the text the kernel compiles too.
#include "pcv_tiles3d_files.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pcv_terrain_files.h"
#include "pcv_tiles3d_dev.h"

namespace {

typedef unsigned __int128 u128;

u128 node_index(const pcv_node_info& n) { return ((u128)(n.id_high & 0x00ffffffffffffffull) << 64) | n.id_low; }

void put_u32(std::string& s, uint32_t v) {
  for (int k = 0; k < 4; ++k) s.push_back((char)(uint8_t)(v >> (8 * k)));
}

std::string vec3_json(double a, double b, double c) {
  auto f = pcv_terrain_f64_json;
  return "[" + f(a) + "," + f(b) + "," + f(c) + "]";
}

uint64_t pad8(uint64_t v) { return (v + 7) & ~7ull; }

}  // namespace

std::string pcv_tiles3d_node_name(const pcv_node_info& n) {
  std::string s = "r";
  const u128 index = node_index(n);
  for (int j = (int)n.level - 1; j >= 0; --j) s.push_back(j >= 42 ? '0' : (char)('0' + (int)((index >> (3 * j)) & 7)));
  return s;
}

int pcv_tiles3d_check_params(const pcv_tiles3d_params* p, std::string* why) {
  auto bad = [&](const std::string& m) {
    *why = m;
    return PCV_E_INVALID;
  };
  if (!p) return bad("null pcv_tiles3d_params");
  if (!std::isfinite(p->error_factor) || p->error_factor < 0) return bad("error_factor must be finite and not negative");
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(p->transform[k])) return bad("transform must be finite");
  if (p->flags & ~PCV_TILES3D_INTENSITY) return bad("unknown flags: " + std::to_string(p->flags & ~PCV_TILES3D_INTENSITY));
  if (p->position_mode > PCV_TILES3D_POS_FLOAT) return bad("unknown position_mode " + std::to_string(p->position_mode));
  if (p->chunk_bytes != 0 && p->chunk_bytes < PCV_TILES3D_MIN_CHUNK_BYTES)
    return bad("chunk_bytes must be 0 or at least " + std::to_string(PCV_TILES3D_MIN_CHUNK_BYTES) + ", got " + std::to_string(p->chunk_bytes));
  return PCV_OK;
}

int pcv_tiles3d_file_plan(const pcv_node_info& node, const pcv_tiles3d_params& p, bool has_intensity, PcvTiles3dFilePlan* out, std::string* why) {
  auto bad = [&](const std::string& m) {
    *why = m;
    return PCV_E_INVALID;
  };
  if (node.encoding < PCV_ENC_UINT8 || node.encoding > PCV_ENC_FLOAT64) return bad("node " + pcv_tiles3d_node_name(node) + ": unknown encoding");
  if (node.num_points <= 0) return bad("node " + pcv_tiles3d_node_name(node) + " holds no point: it has no file");
  if ((p.flags & PCV_TILES3D_INTENSITY) && !has_intensity) return bad("PCV_TILES3D_INTENSITY: the octree carries no intensity");
  PcvTiles3dFilePlan f;
  f.mode = pcv_tiles3d_mode_of(p.position_mode, node.encoding);
  f.encoding = node.encoding;
  f.src_stride = 3 * pcv_tiles3d_src_bytes(node.encoding);
  f.dst_stride = f.mode == PCV_TILES3D_POS_QUANTIZED ? 6 : 12;
  f.intensity = (p.flags & PCV_TILES3D_INTENSITY) != 0;
  f.n = (uint64_t)node.num_points;
  // byteLength is a u32: 19 bytes a point at the most, and well under a KiB of header and JSON
  if (f.n > (0xffffffffull - 4096) / 19) return bad("node " + pcv_tiles3d_node_name(node) + ": a .pnts file cannot hold 4 GiB");
  for (int a = 0; a < 3; ++a) f.rc[a] = pcv_tiles3d_rtc(node.cube_min[a], node.cube_edge);
  auto f64 = pcv_terrain_f64_json;
  const std::string n = std::to_string(f.n);
  std::string js = "{\"POINTS_LENGTH\":" + n + ",\"RTC_CENTER\":" + vec3_json(f.rc[0], f.rc[1], f.rc[2]);
  if (f.mode == PCV_TILES3D_POS_QUANTIZED) {
    js += ",\"QUANTIZED_VOLUME_OFFSET\":" + vec3_json(node.cube_min[0] - f.rc[0], node.cube_min[1] - f.rc[1], node.cube_min[2] - f.rc[2]);
    js += ",\"QUANTIZED_VOLUME_SCALE\":[" + f64(node.cube_edge) + "," + f64(node.cube_edge) + "," + f64(node.cube_edge) + "]";
    js += ",\"POSITION_QUANTIZED\":{\"byteOffset\":0}";
  } else {
    js += ",\"POSITION\":{\"byteOffset\":0}";
  }
  js += ",\"RGB\":{\"byteOffset\":" + std::to_string(f.n * f.dst_stride) + "}}";
  while ((kPcvTiles3dHeaderBytes + js.size()) % 8) js.push_back(' ');
  if (f.intensity) {
    f.batch_json = "{\"INTENSITY\":{\"byteOffset\":0,\"componentType\":\"FLOAT\",\"type\":\"SCALAR\"}}";
    while (f.batch_json.size() % 8) f.batch_json.push_back(' ');
  }
  f.feature_binary_offset = kPcvTiles3dHeaderBytes + js.size();
  f.feature_binary_bytes = pad8(f.n * (f.dst_stride + 3));
  f.batch_json_offset = f.feature_binary_offset + f.feature_binary_bytes;
  f.batch_binary_offset = f.batch_json_offset + f.batch_json.size();
  f.batch_binary_bytes = f.intensity ? pad8(f.n * 4) : 0;
  f.file_bytes = f.batch_binary_offset + f.batch_binary_bytes;
  f.head = "pnts";
  put_u32(f.head, 1);
  put_u32(f.head, (uint32_t)f.file_bytes);
  put_u32(f.head, (uint32_t)js.size());
  put_u32(f.head, (uint32_t)f.feature_binary_bytes);
  put_u32(f.head, (uint32_t)f.batch_json.size());
  put_u32(f.head, (uint32_t)f.batch_binary_bytes);
  f.head += js;
  *out = std::move(f);
  return PCV_OK;
}

void pcv_tiles3d_fill_tile(const PcvTiles3dFilePlan& f, uint64_t node, pcv_tiles3d_tile* out) {
  out->node = node;
  out->num_points = f.n;
  out->mode = f.mode;
  out->reserved = 0;
  out->file_bytes = f.file_bytes;
  out->feature_json_offset = kPcvTiles3dHeaderBytes;
  out->feature_binary_offset = f.feature_binary_offset;
  out->batch_json_offset = f.batch_json_offset;
  out->batch_binary_offset = f.batch_binary_offset;
}

void pcv_tiles3d_build_file(const pcv_node_info& node, const PcvTiles3dFilePlan& f, const uint8_t* xyz, const uint8_t* rgb, const float* intensity,
                            std::vector<uint8_t>* out) {
  out->assign((size_t)f.file_bytes, 0);  // the binaries' padding is 0x00
  uint8_t* w = out->data();
  std::memcpy(w, f.head.data(), f.head.size());
  uint8_t* pos = w + f.feature_binary_offset;
  const uint32_t cb = f.src_stride / 3;
  for (uint64_t i = 0; i < f.n; ++i)
    for (int a = 0; a < 3; ++a) {
      const PcvTiles3dCoord c = pcv_tiles3d_load(f.encoding, xyz + i * f.src_stride + (uint64_t)a * cb);
      if (f.mode == PCV_TILES3D_POS_QUANTIZED) {
        const uint16_t q = pcv_tiles3d_quantized(f.encoding, c);
        pos[i * 6 + 2 * a] = (uint8_t)q, pos[i * 6 + 2 * a + 1] = (uint8_t)(q >> 8);
      } else {
        const float v = pcv_tiles3d_float(f.encoding, c, node.cube_min[a], node.cube_edge, f.rc[a]);
        std::memcpy(pos + i * 12 + 4 * a, &v, 4);
      }
    }
  std::memcpy(pos + f.n * f.dst_stride, rgb, (size_t)(f.n * 3));
  if (f.intensity) {
    std::memcpy(w + f.batch_json_offset, f.batch_json.data(), f.batch_json.size());
    std::memcpy(w + f.batch_binary_offset, intensity, (size_t)(f.n * 4));
  }
}

namespace {

struct Key {
  uint32_t level;
  u128 index;
  bool operator<(const Key& o) const { return level != o.level ? level < o.level : index < o.index; }
};

struct Walk {
  const pcv_node_info* nodes;
  const std::vector<Key>& keys;
  const std::vector<uint64_t>& subtree;
  const pcv_tiles3d_params& p;
  std::string* js;

  // the nodes [lo, hi) that are children of node i
  void children(size_t i, size_t* lo, size_t* hi) const {
    const Key first{keys[i].level + 1, keys[i].index << 3}, last{keys[i].level + 1, (keys[i].index << 3) | 7};
    *lo = (size_t)(std::lower_bound(keys.begin(), keys.end(), first) - keys.begin());
    *hi = (size_t)(std::upper_bound(keys.begin(), keys.end(), last) - keys.begin());
  }
  void tile(size_t i, bool root) {
    auto f = pcv_terrain_f64_json;
    const pcv_node_info& n = nodes[i];
    const double h = n.cube_edge / 2.0;
    const std::string hs = f(h);
    size_t lo, hi;
    children(i, &lo, &hi);
    bool any = false;
    for (size_t c = lo; c < hi; ++c) any = any || subtree[c] > 0;
    *js += "{\"boundingVolume\":{\"box\":[" + f(n.cube_min[0] + h) + "," + f(n.cube_min[1] + h) + "," + f(n.cube_min[2] + h) + "," + hs +
           ",0.0,0.0,0.0," + hs + ",0.0,0.0,0.0," + hs + "]},\"geometricError\":" + f(any ? n.cube_edge * p.error_factor : 0.0);
    if (root) {
      *js += ",\"refine\":\"ADD\"";
      bool has = false;
      for (int k = 0; k < 16; ++k) has = has || p.transform[k] != 0.0;
      if (has) {
        *js += ",\"transform\":[";
        for (int k = 0; k < 16; ++k) *js += (k ? "," : "") + f(p.transform[k]);
        *js += "]";
      }
    }
    if (n.num_points > 0) *js += ",\"content\":{\"uri\":\"" + pcv_tiles3d_node_name(n) + ".pnts\"}";
    if (any) {
      *js += ",\"children\":[";
      bool first = true;
      for (size_t c = lo; c < hi; ++c) {
        if (subtree[c] == 0) continue;
        if (!first) *js += ",";
        first = false;
        tile(c, false);
      }
      *js += "]";
    }
    *js += "}";
  }
};

}  // namespace

int pcv_tiles3d_tileset(const pcv_node_info* nodes, uint64_t count, const pcv_tiles3d_params& p, std::string* json, std::vector<uint8_t>* kinds,
                        std::string* why) {
  auto bad = [&](const std::string& m) {
    *why = m;
    return PCV_E_INVALID;
  };
  if (count == 0 || !nodes) return bad("the node table is empty");
  if (nodes[0].level != 0) return bad("the node table does not begin with the root");
  std::vector<Key> keys((size_t)count);
  for (size_t i = 0; i < count; ++i) {
    if (nodes[i].level > 40) return bad("node " + std::to_string(i) + ": level above 40");
    if (nodes[i].num_points < 0) return bad("node " + std::to_string(i) + ": negative num_points");
    keys[i] = Key{nodes[i].level, node_index(nodes[i])};
    if (i > 0 && !(keys[i - 1] < keys[i])) return bad("the node table is not ascending by (level, index) at node " + std::to_string(i));
  }
  std::vector<uint64_t> subtree((size_t)count);
  for (size_t i = 0; i < count; ++i) subtree[i] = (uint64_t)nodes[i].num_points;
  for (size_t i = (size_t)count; i-- > 1;) {  // parents come before their children: a child is complete when it is added
    const Key parent{keys[i].level - 1, keys[i].index >> 3};
    const auto it = std::lower_bound(keys.begin(), keys.begin() + (long)i, parent);
    if (it == keys.begin() + (long)i || parent < *it) return bad("node " + pcv_tiles3d_node_name(nodes[i]) + " has no parent in the table");
    subtree[(size_t)(it - keys.begin())] += subtree[i];
  }
  if (subtree[0] == 0) return bad("the octree holds no point");
  if (kinds) {
    kinds->resize((size_t)count);
    for (size_t i = 0; i < count; ++i) (*kinds)[i] = nodes[i].num_points > 0 ? 2 : subtree[i] > 0 ? 1 : 0;
  }
  if (json) {
    *json = "{\"asset\":{\"version\":\"1.0\"},\"geometricError\":" + pcv_terrain_f64_json(nodes[0].cube_edge) + ",\"root\":";
    Walk w{nodes, keys, subtree, p, json};
    w.tile(0, true);
    *json += "}";
  }
  return PCV_OK;
}

int pcv_tiles3d_tile_into(const pcv_node_info* node, const pcv_tiles3d_params* params, const uint8_t* xyz, const uint8_t* rgb, const float* intensity,
                          uint8_t* out, uint64_t capacity, uint64_t* len, pcv_tiles3d_tile* tile, std::string* why) {
  if (len) *len = 0;
  if (!node || !xyz || !rgb) {
    *why = "null argument";
    return PCV_E_INVALID;
  }
  if (int rc = pcv_tiles3d_check_params(params, why)) return rc;
  PcvTiles3dFilePlan f;
  if (int rc = pcv_tiles3d_file_plan(*node, *params, intensity != nullptr, &f, why)) return rc;
  if (len) *len = f.file_bytes;
  if (tile) pcv_tiles3d_fill_tile(f, 0, tile);
  if (out && capacity) {
    std::vector<uint8_t> file;
    pcv_tiles3d_build_file(*node, f, xyz, rgb, intensity, &file);
    std::memcpy(out, file.data(), (size_t)std::min<uint64_t>(capacity, file.size()));
  }
  return PCV_OK;
}

int pcv_tiles3d_tileset_into(const pcv_node_info* nodes, uint64_t count, const pcv_tiles3d_params* params, char* buf, uint64_t cap, uint64_t* len,
                             std::string* why) {
  if (len) *len = 0;
  std::string json;
  if (int rc = pcv_tiles3d_check_params(params, why)) return rc;
  if (int rc = pcv_tiles3d_tileset(nodes, count, *params, &json, nullptr, why)) return rc;
  if (len) *len = json.size();
  if (buf && cap) std::memcpy(buf, json.data(), (size_t)std::min<uint64_t>(cap, json.size()));
  return PCV_OK;
}

std::vector<uint64_t> pcv_tiles3d_pieces(const std::vector<uint64_t>& file_bytes, uint64_t chunk_bytes) {
  std::vector<uint64_t> first{0};
  uint64_t held = 0;
  for (size_t k = 0; k < file_bytes.size(); ++k) {
    if (held > 0 && held + file_bytes[k] > chunk_bytes) first.push_back(k), held = 0;
    held += file_bytes[k];
  }
  first.push_back(file_bytes.size());
  return first;
}
