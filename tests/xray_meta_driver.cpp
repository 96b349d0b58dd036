// Stand-alone driver for a sanitizer build of the xray Meta code (csrc/pcv_xray_meta.cpp): xray_meta_driver <v3.pb> <v2.pb>.
// The first file holds kMeta below as the protobuf runtime writes it (tests/meta_proto.py), the second a version-2 Meta
// with the deprecated f32 fields. Encodes kMeta, compares and parses it back; then every truncation and every single-byte
// change of both files goes through parse_meta and xray_meta_check from a buffer of exactly its size. Prints the number
// of parses and of those accepted; exit status 1 on any mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../point_cloud_viewer_amd/csrc/pcv_xray_meta.h"

static std::vector<uint8_t> read_all(const char* path) {
  std::vector<uint8_t> d;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  uint8_t buf[4096];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + k);
  std::fclose(f);
  return d;
}

#define REQUIRE(cond)                                                      \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

// what pcv_xray_open_dir relies on after the checks, restated
static bool in_range(const XrayMeta& m) {
  if (m.version != 2 && m.version != 3) return false;
  if (m.tile_size < 1 || m.tile_size > 32768 || m.deepest_level > 31) return false;
  for (const auto& nd : m.nodes) {
    if (nd.first > m.deepest_level) return false;
    if (nd.second >= (uint64_t)1 << (2 * nd.first)) return false;  // level <= 31: the shift is below 64
  }
  return true;
}

static unsigned long g_parses = 0, g_accepted = 0;
static void one(const std::vector<uint8_t>& data) {
  XrayMeta m;
  ++g_parses;
  if (!parse_meta(data, &m) || !xray_meta_check(m).empty()) return;
  REQUIRE(in_range(m));
  ++g_accepted;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  XrayMeta want;
  want.version = 3;
  want.has_min = true;
  want.min[0] = 0.1;
  want.min[1] = -333333.25;
  want.edge = 0.3;
  want.deepest_level = 5;
  want.tile_size = 256;
  for (uint64_t i = 0; i < 20; ++i) {  // every level several times, the root (an empty NodeId) among them
    const uint32_t level = (uint32_t)(i % 6);
    want.nodes.emplace_back(level, (i * 2654435761ull) % ((uint64_t)1 << (2 * level)));
  }
  const std::vector<uint8_t> v3 = read_all(argv[1]), v2 = read_all(argv[2]);
  REQUIRE(xray_meta_encode(want) == v3);
  REQUIRE(xray_meta_name(0, 0) == "meta.pb" && xray_meta_name(3, 27) == "meta123.pb" && quad_name(2, 1) == "r01");
  XrayMeta got;
  REQUIRE(parse_meta(v3, &got) && xray_meta_check(got).empty());
  REQUIRE(got.version == 3 && got.has_min && got.min[0] == want.min[0] && got.min[1] == want.min[1] && got.edge == want.edge);
  REQUIRE(got.deepest_level == want.deepest_level && got.tile_size == want.tile_size && got.nodes == want.nodes);
  XrayMeta old;
  REQUIRE(parse_meta(v2, &old) && xray_meta_check(old).empty());
  REQUIRE(old.version == 2 && !old.has_min && old.dmin[0] == 0.5f && old.dmin[1] == -1024.25f && old.dedge == 2048.0f);
  REQUIRE(old.nodes == want.nodes);
  for (const std::vector<uint8_t>* file : {&v3, &v2}) {
    for (size_t cut = 0; cut <= file->size(); ++cut) one(std::vector<uint8_t>(file->begin(), file->begin() + (long)cut));
    std::vector<uint8_t> d(*file);
    for (size_t at = 0; at < d.size(); ++at) {
      const uint8_t was = d[at];
      for (unsigned v = 0; v < 256; ++v) {
        if (v == was) continue;
        d[at] = (uint8_t)v;
        one(d);
      }
      d[at] = was;
    }
  }
  std::printf("%lu %lu\n", g_parses, g_accepted);
  return 0;
}
