// Stand-alone driver of csrc/pcv_ply_write.cpp and csrc/pcv_ply.cpp (no HIP, no library; tests/test_ply_write_cpu.py builds
// it with -fsanitize=address,undefined). argv[1] is a file of commands, one per line, fields separated by blanks; an attribute
// is written name:data_type (the PCV_ATTR_* number):
//   layout <attr>...                      -> "layout <rc> <stride> <offset of every given attribute>..." or "layout <rc>" + reason
//   header <count> <attr>...              -> "header <rc> <hex of the header>"
//   check <path> <attr>...                -> "check <rc> <old count> <old size>", then the reason ("-" if none)
//   file <path> <t|a> <rows> <commit|abandon> <attr>...
//                                         -> the PcvPlyFile of one write call: `rows` rows whose byte j of row r is (r * 31 + j +
//                                            old rows * 7) & 255, written as two pieces in swapped order; "file <rc> <old count>"
//   read <path> <flags>                   -> "read <rc> <n> <has color> <has intensity> <extras>", then hex lines "x", "y", "z",
//                                            "rgb", "intensity" and per extra "<name> <data type> <hex>"; a refusal: the reason
// The last line is "commands <n>".
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../include/pcv_hip.h"
#include "../point_cloud_viewer_amd/csrc/pcv_ply_write.h"

namespace {

struct Attrs {
  std::vector<std::string> names;
  std::vector<const char*> ptrs;
  std::vector<int32_t> types;
};
Attrs parse_attrs(std::istringstream& in) {
  Attrs a;
  std::string tok;
  while (in >> tok) {
    const size_t colon = tok.rfind(':');
    a.names.push_back(tok.substr(0, colon));
    a.types.push_back(std::stoi(tok.substr(colon + 1)));
  }
  for (const std::string& n : a.names) a.ptrs.push_back(n.c_str());
  return a;
}
std::string hex(const void* data, size_t bytes) {
  static const char* digits = "0123456789abcdef";
  std::string out = bytes ? "" : "-";
  const uint8_t* p = (const uint8_t*)data;
  for (size_t k = 0; k < bytes; ++k) out.push_back(digits[p[k] >> 4]), out.push_back(digits[p[k] & 15]);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream script(argv[1]);
  std::string line;
  int commands = 0;
  while (std::getline(script, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    ++commands;
    std::vector<PcvPlyColumn> cols;
    std::string why;
    uint32_t stride = 0;
    if (cmd == "layout") {
      Attrs a = parse_attrs(in);
      const int rc = pcv_ply_columns(a.ptrs.data(), a.types.data(), (uint32_t)a.names.size(), &cols, &stride, &why);
      std::cout << "layout " << rc;
      if (rc != PCV_OK) {
        std::cout << "\n" << why << "\n";
        continue;
      }
      std::vector<uint32_t> offsets(a.names.size());
      for (const PcvPlyColumn& c : cols) offsets[c.given] = c.offset;
      std::cout << " " << stride;
      for (uint32_t o : offsets) std::cout << " " << o;
      std::cout << "\n";
    } else if (cmd == "header") {
      unsigned long long count;
      in >> count;
      Attrs a = parse_attrs(in);
      const int rc = pcv_ply_columns(a.ptrs.data(), a.types.data(), (uint32_t)a.names.size(), &cols, &stride, &why);
      const std::string h = rc == PCV_OK ? pcv_ply_header(cols, count) : why;
      std::cout << "header " << rc << " " << hex(h.data(), h.size()) << "\n";
    } else if (cmd == "check") {
      std::string path;
      in >> path;
      Attrs a = parse_attrs(in);
      if (pcv_ply_columns(a.ptrs.data(), a.types.data(), (uint32_t)a.names.size(), &cols, &stride, &why)) return 3;
      uint64_t old_count = 99, old_size = 99;
      const int rc = pcv_ply_append_check(path.c_str(), cols, &old_count, &old_size, &why);
      std::cout << "check " << rc << " " << old_count << " " << old_size << "\n" << (why.empty() ? "-" : why) << "\n";
    } else if (cmd == "file") {
      std::string path, mode, end;
      uint64_t rows;
      in >> path >> mode >> rows >> end;
      Attrs a = parse_attrs(in);
      if (pcv_ply_columns(a.ptrs.data(), a.types.data(), (uint32_t)a.names.size(), &cols, &stride, &why)) return 3;
      PcvPlyFile f;
      int rc = f.begin(path.c_str(), mode == "a", cols, &why);
      if (rc == PCV_OK && rows) {
        std::vector<uint8_t> body(rows * stride);
        for (uint64_t r = 0; r < rows; ++r)
          for (uint32_t j = 0; j < stride; ++j) body[r * stride + j] = (uint8_t)(r * 31 + j + f.old_count * 7);
        const uint64_t cut = (rows / 2) * stride;
        rc = f.open_for_rows(&why);
        if (rc == PCV_OK) rc = f.write_at(cut, body.data() + cut, body.size() - cut, &why);
        if (rc == PCV_OK) rc = f.write_at(0, body.data(), cut, &why);
        if (rc != PCV_OK || end == "abandon") f.abandon();
        else rc = f.commit(rows, stride, &why);
      }
      std::cout << "file " << rc << " " << f.old_count << "\n" << (why.empty() ? "-" : why) << "\n";
    } else if (cmd == "read") {
      std::string path;
      uint32_t flags;
      in >> path >> flags;
      pcv_ply* ply = nullptr;
      char err[256] = "";
      const int rc = pcv_ply_read_ex(path.c_str(), flags, &ply, err, sizeof(err));
      if (rc != PCV_OK) {
        std::cout << "read " << rc << "\n" << err << "\n";
        continue;
      }
      pcv_points p;
      pcv_ply_points(ply, &p);
      uint32_t count = 0;
      pcv_attribute extras[PCV_S2_MAX_EXTRAS];
      pcv_ply_attributes(ply, &count, extras);
      std::cout << "read " << rc << " " << p.n << " " << (p.color ? 1 : 0) << " " << (p.intensity ? 1 : 0) << " " << count << "\n";
      std::cout << "x " << hex(p.x, p.n * 8) << "\ny " << hex(p.y, p.n * 8) << "\nz " << hex(p.z, p.n * 8) << "\n";
      std::cout << "rgb " << hex(p.color, p.color ? p.n * 3 : 0) << "\nintensity " << hex(p.intensity, p.intensity ? p.n * 4 : 0) << "\n";
      for (uint32_t k = 0; k < count; ++k)
        std::cout << extras[k].name << " " << extras[k].data_type << " " << hex(extras[k].data, p.n * pcv_ply_elem_size(extras[k].data_type)) << "\n";
      pcv_ply_free(ply);
    } else {
      return 4;
    }
  }
  std::cout << "commands " << commands << "\n";
  return 0;
}
