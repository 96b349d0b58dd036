// Stand-alone driver of csrc/pcv_tiles3d_files.cpp (no HIP, no library; tests/test_tiles3d_cpu.py builds it with
// -fsanitize=address,undefined). argv[1] is a binary file of cases, argv[2] the file the results go to. Little endian.
//   u32 number of cases, then per case a u32 kind:
//   kind 1, a file: u32 encoding, position_mode, flags, n; f64 cube_min[3], cube_edge; the node's .xyz, .rgb (3 n) and
//           .intensity (4 n) bytes. Result: i32 rc, u64 len, len bytes. The file is also asked for at the capacities 0, 1, 27,
//           28, len - 1, len and len + 64 into heap blocks of exactly that size, each of which must hold a prefix of the file
//           (a write past one is a sanitizer report), and without an output.
//   kind 2, a tileset: u32 count; f64 error_factor, transform[16]; per node u64 id_high, id_low, i64 num_points, u32 level,
//           encoding, f64 cube_min[3], cube_edge. Result: i32 rc, u64 len, len bytes; the same capacities.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "pcv_tiles3d_files.h"

namespace {

struct Reader {
  const std::vector<uint8_t>& b;
  size_t at = 0;
  bool ok = true;
  template <typename T>
  T get() {
    T v{};
    if (at + sizeof(T) > b.size()) {
      ok = false;
      return v;
    }
    std::memcpy(&v, b.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  std::vector<uint8_t> bytes(size_t n) {
    if (at + n > b.size()) {
      ok = false;
      return {};
    }
    std::vector<uint8_t> v(b.begin() + (long)at, b.begin() + (long)(at + n));
    at += n;
    return v;
  }
};

template <typename T>
void put(std::vector<uint8_t>& o, T v) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
  o.insert(o.end(), p, p + sizeof(T));
}

std::vector<uint64_t> capacities(uint64_t len) {
  std::vector<uint64_t> c{0, 1, 27, 28, len, len + 64};
  if (len) c.push_back(len - 1);
  return c;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<uint8_t> input((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  Reader r{input};
  std::vector<uint8_t> result;
  const uint32_t cases = r.get<uint32_t>();
  for (uint32_t c = 0; c < cases && r.ok; ++c) {
    const uint32_t kind = r.get<uint32_t>();
    std::string why;
    if (kind == 1) {
      pcv_node_info nd{};
      pcv_tiles3d_params p{};
      nd.encoding = r.get<uint32_t>();
      p.position_mode = r.get<uint32_t>();
      p.flags = r.get<uint32_t>();
      const uint32_t n = r.get<uint32_t>();
      nd.num_points = n;
      for (int a = 0; a < 3; ++a) nd.cube_min[a] = r.get<double>();
      nd.cube_edge = r.get<double>();
      p.error_factor = PCV_TILES3D_DEFAULT_ERROR_FACTOR;
      const uint32_t cb = nd.encoding == PCV_ENC_UINT8 ? 1 : nd.encoding == PCV_ENC_UINT16 ? 2 : nd.encoding == PCV_ENC_FLOAT32 ? 4 : 8;
      const std::vector<uint8_t> xyz = r.bytes((size_t)n * 3 * cb), rgb = r.bytes((size_t)n * 3), ib = r.bytes((size_t)n * 4);
      if (!r.ok) break;
      std::vector<float> inten(n);
      if (n) std::memcpy(inten.data(), ib.data(), ib.size());
      const float* ip = (p.flags & PCV_TILES3D_INTENSITY) ? inten.data() : nullptr;
      uint64_t len = 0;
      pcv_tiles3d_tile tile{};
      int rc = pcv_tiles3d_tile_into(&nd, &p, xyz.data(), rgb.data(), ip, nullptr, 0, &len, &tile, &why);
      std::vector<uint8_t> file((size_t)len);
      if (rc == PCV_OK) rc = pcv_tiles3d_tile_into(&nd, &p, xyz.data(), rgb.data(), ip, file.data(), len, &len, nullptr, &why);
      if (rc == PCV_OK) {
        if (tile.file_bytes != len || tile.feature_json_offset != 28) return std::fprintf(stderr, "case %u: plan\n", c), 1;
        for (uint64_t cap : capacities(len)) {
          std::vector<uint8_t> part((size_t)cap);
          uint64_t l2 = 0;
          if (pcv_tiles3d_tile_into(&nd, &p, xyz.data(), rgb.data(), ip, part.data(), cap, &l2, nullptr, &why) != PCV_OK || l2 != len ||
              (cap && std::memcmp(part.data(), file.data(), (size_t)(cap < len ? cap : len)) != 0))
            return std::fprintf(stderr, "case %u: capacity %llu\n", c, (unsigned long long)cap), 1;
          for (uint64_t k = len; k < cap; ++k)
            if (part[(size_t)k] != 0) return std::fprintf(stderr, "case %u: a byte past the file was written\n", c), 1;
        }
      } else if (why.empty()) {
        return std::fprintf(stderr, "case %u: a refusal without a reason\n", c), 1;
      }
      put<int32_t>(result, rc);
      put<uint64_t>(result, rc == PCV_OK ? len : 0);
      if (rc == PCV_OK) result.insert(result.end(), file.begin(), file.end());
    } else if (kind == 2) {
      const uint32_t count = r.get<uint32_t>();
      pcv_tiles3d_params p{};
      p.error_factor = r.get<double>();
      for (int k = 0; k < 16; ++k) p.transform[k] = r.get<double>();
      std::vector<pcv_node_info> nodes(count);
      for (pcv_node_info& nd : nodes) {
        nd = pcv_node_info{};
        nd.id_high = r.get<uint64_t>(), nd.id_low = r.get<uint64_t>(), nd.num_points = r.get<int64_t>();
        nd.level = r.get<uint32_t>(), nd.encoding = r.get<uint32_t>();
        for (int a = 0; a < 3; ++a) nd.cube_min[a] = r.get<double>();
        nd.cube_edge = r.get<double>();
      }
      if (!r.ok) break;
      uint64_t len = 0;
      int rc = pcv_tiles3d_tileset_into(nodes.data(), count, &p, nullptr, 0, &len, &why);
      std::vector<char> text((size_t)len);
      if (rc == PCV_OK) rc = pcv_tiles3d_tileset_into(nodes.data(), count, &p, text.data(), len, &len, &why);
      if (rc == PCV_OK) {
        for (uint64_t cap : capacities(len)) {
          std::vector<char> part((size_t)cap);
          uint64_t l2 = 0;
          if (pcv_tiles3d_tileset_into(nodes.data(), count, &p, part.data(), cap, &l2, &why) != PCV_OK || l2 != len ||
              (cap && std::memcmp(part.data(), text.data(), (size_t)(cap < len ? cap : len)) != 0))
            return std::fprintf(stderr, "case %u: capacity %llu\n", c, (unsigned long long)cap), 1;
        }
      } else if (why.empty()) {
        return std::fprintf(stderr, "case %u: a refusal without a reason\n", c), 1;
      }
      put<int32_t>(result, rc);
      put<uint64_t>(result, rc == PCV_OK ? len : 0);
      if (rc == PCV_OK) result.insert(result.end(), text.begin(), text.end());
    } else {
      return std::fprintf(stderr, "case %u: unknown kind %u\n", c, kind), 1;
    }
  }
  if (!r.ok) return std::fprintf(stderr, "the case file is cut off\n"), 1;
  // the grouping into pieces: every file in exactly one piece, in order, no piece above the limit unless it is one file
  const std::vector<uint64_t> sizes{5, 5, 5, 20, 1, 1, 30, 2};
  for (uint64_t chunk : {1ull, 10ull, 11ull, 30ull, 1000ull}) {
    const std::vector<uint64_t> first = pcv_tiles3d_pieces(sizes, chunk);
    if (first.front() != 0 || first.back() != sizes.size()) return std::fprintf(stderr, "pieces: ends\n"), 1;
    for (size_t k = 0; k + 1 < first.size(); ++k) {
      uint64_t sum = 0;
      for (uint64_t i = first[k]; i < first[k + 1]; ++i) sum += sizes[(size_t)i];
      if (first[k] >= first[k + 1] || (sum > chunk && first[k + 1] - first[k] != 1)) return std::fprintf(stderr, "pieces: chunk %llu\n", (unsigned long long)chunk), 1;
    }
  }
  std::ofstream out(argv[2], std::ios::binary);
  out.write(reinterpret_cast<const char*>(result.data()), (std::streamsize)result.size());
  return out.good() ? 0 : 1;
}
