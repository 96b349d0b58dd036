// pcv_xray_meta.cpp — xray_proto Meta on the wire, both ways, and the names of a quadtree directory's files.
#include "pcv_xray_meta.h"

#include <cstring>

namespace {

// ---- written: rust-protobuf 2.x, proto3: fields in number order, zero scalars omitted, set message fields always written
void pb_varint(std::vector<uint8_t>& o, uint64_t v) {
  while (v >= 0x80) {
    o.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  o.push_back((uint8_t)v);
}
void pb_double(std::vector<uint8_t>& o, uint32_t field, double v) {
  if (v == 0.0) return;
  pb_varint(o, field << 3 | 1);
  uint8_t b[8];
  std::memcpy(b, &v, 8);
  o.insert(o.end(), b, b + 8);
}
void pb_uint(std::vector<uint8_t>& o, uint32_t field, uint64_t v) {
  if (v == 0) return;
  pb_varint(o, field << 3);
  pb_varint(o, v);
}
void pb_bytes(std::vector<uint8_t>& o, uint32_t field, const std::vector<uint8_t>& m) {
  pb_varint(o, field << 3 | 2);
  pb_varint(o, m.size());
  o.insert(o.end(), m.begin(), m.end());
}

// ---- read (Meta::from_proto, xray/src/lib.rs:81-116) -------------------------------------------------------------------
// proto3 wire format of xray_proto_rust/src/proto.proto: Meta { int32 version = 1; Rect bounding_rect = 2; uint32
// deepest_level = 3; uint32 tile_size = 4; repeated NodeId nodes = 5 }, Rect { Vector2f deprecated_min = 1; float
// deprecated_edge_length = 2; Vector2d min = 3; double edge_length = 4 }, NodeId { uint32 level = 1; uint64 index = 2 }.
// Fields may come in any order, a repeated scalar field keeps its last value, unknown fields are skipped.
struct PbReader {
  const uint8_t* p;
  size_t n, pos = 0;
  bool bad = false;
  bool more() const { return !bad && pos < n; }
  uint64_t varint() {
    uint64_t v = 0;
    for (int shift = 0; shift < 64; shift += 7) {
      if (pos >= n) break;
      const uint8_t c = p[pos++];
      v |= (uint64_t)(c & 0x7f) << shift;
      if (c < 0x80) return v;
    }
    bad = true;
    return 0;
  }
  // one field: its number, wire type and value (varint / fixed bits in `v`, a length-delimited body in `sub`)
  bool field(uint32_t* num, uint32_t* wt, uint64_t* v, PbReader* sub) {
    const uint64_t key = varint();
    if (bad || (key >> 3) == 0 || (key >> 3) > 0x1fffffffu) return !(bad = true);
    *num = (uint32_t)(key >> 3);
    *wt = (uint32_t)(key & 7);
    *v = 0;
    if (*wt == 0) {
      *v = varint();
    } else if (*wt == 1 || *wt == 5) {
      const size_t k = *wt == 1 ? 8 : 4;
      if (n - pos < k) return !(bad = true);
      std::memcpy(v, p + pos, k);  // little endian, as the wire
      pos += k;
    } else if (*wt == 2) {
      const uint64_t k = varint();
      if (bad || k > n - pos) return !(bad = true);
      *sub = PbReader{p + pos, (size_t)k};
      pos += (size_t)k;
    } else {
      return !(bad = true);  // groups: not in this schema
    }
    return !bad;
  }
};

double pb_f64(uint64_t v) {
  double d;
  std::memcpy(&d, &v, 8);
  return d;
}
float pb_f32(uint64_t v) {
  const uint32_t u = (uint32_t)v;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

}  // namespace

std::string quad_name(uint32_t level, uint64_t index) {
  std::string s = "r";
  for (int l = (int)level - 1; l >= 0; --l) s.push_back((char)('0' + ((index >> (2 * l)) & 3u)));
  return s;
}

std::string xray_meta_name(uint32_t root_level, uint64_t root_index) { return "meta" + quad_name(root_level, root_index).substr(1) + ".pb"; }

std::vector<uint8_t> xray_meta_encode(const XrayMeta& m) {
  std::vector<uint8_t> meta, r, mn;
  pb_uint(meta, 1, 3);
  pb_double(mn, 1, m.min[0]);
  pb_double(mn, 2, m.min[1]);
  pb_bytes(r, 3, mn);
  pb_double(r, 4, m.edge);
  pb_bytes(meta, 2, r);
  pb_uint(meta, 3, m.deepest_level);
  pb_uint(meta, 4, m.tile_size);
  for (const auto& nd : m.nodes) {
    std::vector<uint8_t> id;
    pb_uint(id, 1, nd.first);
    pb_uint(id, 2, nd.second);
    pb_bytes(meta, 5, id);
  }
  return meta;
}

bool parse_meta(const std::vector<uint8_t>& data, XrayMeta* m) {
  PbReader top{data.data(), data.size()};
  uint32_t f, wt;
  uint64_t v;
  PbReader sub{nullptr, 0};
  while (top.more()) {
    if (!top.field(&f, &wt, &v, &sub)) return false;
    if (f == 1 && wt == 0) m->version = (int32_t)v;
    if (f == 3 && wt == 0) m->deepest_level = (uint32_t)v;
    if (f == 4 && wt == 0) m->tile_size = (uint32_t)v;
    if ((f == 1 || f == 3 || f == 4) && wt != 0) return false;
    if ((f == 2 || f == 5) && wt != 2) return false;
    if (f == 2) {
      PbReader rect = sub, vec{nullptr, 0};
      while (rect.more()) {
        uint32_t g, gw;
        if (!rect.field(&g, &gw, &v, &vec)) return false;
        if ((g == 1 || g == 3) && gw != 2) return false;
        if ((g == 2 && gw != 5) || (g == 4 && gw != 1)) return false;
        if (g == 2) m->dedge = pb_f32(v);
        if (g == 4) m->edge = pb_f64(v);
        if (g == 1 || g == 3) {
          if (g == 3) m->has_min = true;
          PbReader none{nullptr, 0};
          while (vec.more()) {
            uint32_t c, cw;
            if (!vec.field(&c, &cw, &v, &none)) return false;
            if ((c == 1 || c == 2) && cw != (g == 3 ? 1u : 5u)) return false;
            if (c == 1 || c == 2) {
              if (g == 3) m->min[c - 1] = pb_f64(v);
              else m->dmin[c - 1] = pb_f32(v);
            }
          }
          if (vec.bad) return false;
        }
      }
      if (rect.bad) return false;
    }
    if (f == 5) {
      PbReader id = sub, none{nullptr, 0};
      uint32_t level = 0;
      uint64_t index = 0;
      while (id.more()) {
        uint32_t g, gw;
        if (!id.field(&g, &gw, &v, &none)) return false;
        if ((g == 1 || g == 2) && gw != 0) return false;
        if (g == 1) level = (uint32_t)v;
        if (g == 2) index = v;
      }
      if (id.bad) return false;
      m->nodes.emplace_back(level, index);
    }
  }
  return !top.bad;
}

std::string xray_meta_check(const XrayMeta& m) {
  if (m.version != 2 && m.version != 3) return ": Invalid version. We only support 3, but found " + std::to_string(m.version) + ".";
  if (m.tile_size == 0 || m.tile_size > kMaxTilePx) return ": tile_size outside 1 ..= 32768";
  if (m.deepest_level > 31) return ": deepest_level above 31 (a u64 index holds 32 levels)";
  for (const auto& nd : m.nodes)
    if (nd.first > m.deepest_level || (nd.first < 32 && (nd.second >> (2 * nd.first)) != 0)) return ": a node outside the quadtree";
  return std::string();
}
