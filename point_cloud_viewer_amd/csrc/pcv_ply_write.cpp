// pcv_ply_write.cpp — the write half of the PLY format (host side, standard C++, no HIP).
//
// Restates PlyNodeWriter with Encoding::Plain (reference src/read_write/ply.rs:559-732): position as three doubles, then
// the attributes of the batch in BTreeMap order (ascending by name, bytewise), each written little endian as it is
// (write_le_pos, :604-606); a header whose vertex count is a fixed 20-digit field (:32-34) patched when the writer is
// dropped (:641-660), after a single trailing newline (:646); OpenMode::Append (:663-689) reads the old count from that field
// and writes over the trailing newline.
// Departures: an append first compares the header these columns give with the file's, byte for byte, and
// refuses a file of other columns (the reference appends whatever it is given); a file that exists but is shorter than the
// fixed prefix is written anew. The ScaledToCube position encodings (:697-702) are node files, not an exchange format: out
// of scope.
#include "pcv_ply_write.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>

#include "../../include/pcv_hip.h"

namespace {

const char kStart[] = "ply\nformat binary_little_endian 1.0\nelement vertex ";  // ply.rs:32-33
static_assert(sizeof(kStart) - 1 == kPcvPlyCountAt, "the count field starts behind the fixed prefix");

const char* type_word(int32_t t) {  // ply.rs:582-593
  switch (t) {
    case PCV_ATTR_U8: case PCV_ATTR_U8VEC3: return "uchar";
    case PCV_ATTR_U16: return "ushort";
    case PCV_ATTR_U32: return "uint";
    case PCV_ATTR_U64: return "ulonglong";
    case PCV_ATTR_I8: return "char";
    case PCV_ATTR_I16: return "short";
    case PCV_ATTR_I32: return "int";
    case PCV_ATTR_I64: return "longlong";
    case PCV_ATTR_F32: return "float";
    default: return "double";  // F64, F64Vec3
  }
}
uint32_t dims(int32_t t) { return t == PCV_ATTR_U8VEC3 || t == PCV_ATTR_F64VEC3 ? 3u : 1u; }  // AttributeData::dim

std::string count_field(uint64_t count) {
  char buf[32];
  snprintf(buf, sizeof(buf), "%020llu", (unsigned long long)count);  // "{:0width$}" (ply.rs:652-657)
  return buf;
}

std::vector<std::string> lines_of(const std::string& s) {
  std::vector<std::string> out;
  size_t at = 0;
  while (at < s.size()) {
    const size_t nl = s.find('\n', at);
    out.push_back(s.substr(at, nl == std::string::npos ? std::string::npos : nl - at));
    if (nl == std::string::npos) break;
    at = nl + 1;
  }
  return out;
}

bool write_all(int fd, uint64_t at, const void* data, uint64_t bytes) {
  const uint8_t* p = (const uint8_t*)data;
  while (bytes) {
    const ssize_t w = pwrite(fd, p, (size_t)std::min<uint64_t>(bytes, 1u << 30), (off_t)at);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    p += w, at += (uint64_t)w, bytes -= (uint64_t)w;
  }
  return true;
}

}  // namespace

uint32_t pcv_ply_elem_size(int32_t t) {
  switch (t) {
    case PCV_ATTR_U8: case PCV_ATTR_I8: return 1;
    case PCV_ATTR_U16: case PCV_ATTR_I16: return 2;
    case PCV_ATTR_U32: case PCV_ATTR_I32: case PCV_ATTR_F32: return 4;
    case PCV_ATTR_U64: case PCV_ATTR_I64: case PCV_ATTR_F64: return 8;
    case PCV_ATTR_U8VEC3: return 3;
    case PCV_ATTR_F64VEC3: return 24;
    default: return 0;
  }
}

int pcv_ply_columns(const char* const* names, const int32_t* data_types, uint32_t n, std::vector<PcvPlyColumn>* cols, uint32_t* stride,
                    std::string* why) {
  cols->clear();
  if (n && (!names || !data_types)) return *why = "null argument", PCV_E_INVALID;
  for (uint32_t k = 0; k < n; ++k) {
    if (!names[k] || !names[k][0]) return *why = "attribute " + std::to_string(k) + " has no name", PCV_E_INVALID;
    PcvPlyColumn c;
    c.name = names[k], c.data_type = data_types[k], c.given = k;
    if (c.data_type == 0) return *why = "Data type for attribute '" + c.name + "' not found.", PCV_E_INVALID;  // lib.rs:94
    c.elem = pcv_ply_elem_size(c.data_type);
    if (c.elem == 0) return *why = "Attribute data type invalid (attribute '" + c.name + "')", PCV_E_INVALID;
    cols->push_back(c);
  }
  std::sort(cols->begin(), cols->end(), [](const PcvPlyColumn& a, const PcvPlyColumn& b) { return a.name < b.name; });  // bytewise
  uint32_t at = kPcvPlyPositionBytes;
  for (size_t k = 0; k < cols->size(); ++k) {
    if (k && (*cols)[k].name == (*cols)[k - 1].name) return *why = "attribute '" + (*cols)[k].name + "' is named twice", PCV_E_INVALID;
    (*cols)[k].offset = at;
    at += (*cols)[k].elem;
  }
  if (stride) *stride = at;
  return PCV_OK;
}

std::string pcv_ply_header(const std::vector<PcvPlyColumn>& cols, uint64_t count) {
  std::string h = kStart;
  h += count_field(count);
  h += "\n";
  for (const char* axis : {"x", "y", "z"}) h += std::string("property double ") + axis + "\n";
  for (const PcvPlyColumn& c : cols) {
    const std::string word = type_word(c.data_type);
    const uint32_t d = dims(c.data_type);
    if (c.name == "color" || c.name == "rgb" || c.name == "rgba") {  // ply.rs:710-716
      const char* colors[] = {"red", "green", "blue", "alpha"};
      for (uint32_t i = 0; i < d; ++i) h += "property " + word + " " + colors[i] + "\n";
    } else if (d > 1) {  // :717-723
      for (uint32_t i = 0; i < d; ++i) h += "property " + word + " " + c.name + std::to_string(i) + "\n";
    } else {
      h += "property " + word + " " + c.name + "\n";
    }
  }
  h += "end_header\n";
  return h;
}

int pcv_ply_append_check(const char* path, const std::vector<PcvPlyColumn>& cols, uint64_t* old_count, uint64_t* old_size, std::string* why) {
  *old_count = 0, *old_size = 0;
  if (!path) return *why = "null argument", PCV_E_INVALID;
  const std::string p(path);
  FILE* f = fopen(path, "rb");
  if (!f) {
    if (errno == ENOENT) return PCV_OK;  // File::open fails: nothing to append to (ply.rs:667)
    return *why = "cannot read " + p + ": " + strerror(errno), PCV_E_IO;
  }
  struct stat st;
  if (fstat(fileno(f), &st) != 0 || !S_ISREG(st.st_mode)) {
    fclose(f);
    return *why = "cannot read " + p + ": not a regular file", PCV_E_IO;
  }
  const uint64_t size = (uint64_t)st.st_size;
  if (size < kPcvPlyCountAt + kPcvPlyCountDigits) {  // ply.rs:668-670: the count stays 0
    fclose(f);
    return PCV_OK;
  }
  const std::string want0 = pcv_ply_header(cols, 0);
  std::string have(std::min<uint64_t>(size, want0.size() + 256), '\0');
  const size_t got = fread(&have[0], 1, have.size(), f);
  fclose(f);
  if (got != have.size()) return *why = "cannot read " + p, PCV_E_IO;
  if (have.compare(0, kPcvPlyCountAt, kStart) != 0)
    return *why = p + " does not start like a binary little-endian PLY of this library (line 'ply' / 'format' / 'element vertex')", PCV_E_INVALID;
  uint64_t count = 0;
  for (uint32_t k = 0; k < kPcvPlyCountDigits; ++k) {
    const char ch = have[kPcvPlyCountAt + k];
    if (ch < '0' || ch > '9') return *why = p + ": the vertex count is not a " + std::to_string(kPcvPlyCountDigits) + "-digit field", PCV_E_INVALID;
    count = count * 10 + (uint64_t)(ch - '0');  // 20 digits may pass 2^64: such a count fails the length check below
  }
  const std::string want = pcv_ply_header(cols, count);
  if (have.compare(0, want.size(), want) != 0) {
    const std::vector<std::string> a = lines_of(want), b = lines_of(have.substr(0, have.find("end_header\n") == std::string::npos
                                                                                     ? have.size()
                                                                                     : have.find("end_header\n") + 11));
    size_t k = 0;
    while (k < a.size() && k < b.size() && a[k] == b[k]) ++k;
    const std::string ours = k < a.size() ? a[k] : "(nothing)", theirs = k < b.size() ? b[k] : "(nothing)";
    return *why = p + " holds other columns: header line " + std::to_string(k + 1) + " is '" + theirs + "', the requested attributes give '" + ours + "'",
           PCV_E_INVALID;
  }
  uint32_t stride = kPcvPlyPositionBytes;
  for (const PcvPlyColumn& c : cols) stride += c.elem;
  const uint64_t body = size - want.size();
  const bool fits = count == 0 ? body == 0 : (body >= 1 && (body - 1) / stride == count && (body - 1) % stride == 0);
  if (!fits)
    return *why = p + ": " + std::to_string(body) + " bytes behind the header are not " + std::to_string(count) + " rows of " + std::to_string(stride) +
                  " bytes and a newline",
           PCV_E_INVALID;
  *old_count = count, *old_size = size;
  return PCV_OK;
}

int PcvPlyFile::begin(const char* p, bool app, const std::vector<PcvPlyColumn>& cols, std::string* why) {
  if (!p || !p[0]) return *why = "path is empty", PCV_E_INVALID;
  path = p, append = app, fd = -1, opened = false, old_count = 0, old_size = 0, rows = 0;
  if (append) {
    const int rc = pcv_ply_append_check(p, cols, &old_count, &old_size, why);
    if (rc != PCV_OK) return rc;
  }
  header = pcv_ply_header(cols, old_count);
  // a file with rows ends in a newline, which the new rows go over (ply.rs:680-683)
  body_at = old_count > 0 ? old_size - 1 : header.size();
  return PCV_OK;
}

int PcvPlyFile::open_for_rows(std::string* why) {
  const bool fresh = old_size == 0;  // truncate mode, or nothing usable to append to
  fd = open(path.c_str(), fresh ? (O_WRONLY | O_CREAT | O_TRUNC) : O_WRONLY, 0644);
  if (fd < 0) return *why = "cannot open " + path + " for writing: " + strerror(errno), PCV_E_IO;
  opened = true;
  if (fresh && !write_all(fd, 0, header.data(), header.size())) return *why = "cannot write " + path + ": " + strerror(errno), PCV_E_IO;
  return PCV_OK;
}

int PcvPlyFile::write_at(uint64_t offset, const void* data, uint64_t bytes, std::string* why) {
  if (!write_all(fd, body_at + offset, data, bytes)) return *why = "cannot write " + path + ": " + strerror(errno), PCV_E_IO;
  return PCV_OK;
}

int PcvPlyFile::commit(uint64_t n, uint32_t stride, std::string* why) {
  rows = n;
  const std::string field = count_field(old_count + n);
  const bool ok = write_all(fd, body_at + n * stride, "\n", 1) && write_all(fd, kPcvPlyCountAt, field.data(), field.size());
  const int e = errno;
  const bool closed = close(fd) == 0;
  fd = -1;
  if (!ok || !closed) {
    *why = "cannot write " + path + ": " + strerror(ok ? errno : e);
    abandon();
    return PCV_E_IO;
  }
  return PCV_OK;
}

void PcvPlyFile::abandon() {
  if (fd >= 0) close(fd);
  fd = -1;
  if (!opened) return;  // nothing of this call has reached the file
  opened = false;
  if (old_size == 0) {
    unlink(path.c_str());  // (a truncate-mode file, or one that held nothing usable)
    return;
  }
  const int f = open(path.c_str(), O_WRONLY);
  if (f < 0) return;
  const std::string field = count_field(old_count);
  (void)write_all(f, kPcvPlyCountAt, field.data(), field.size());
  if (old_count > 0) (void)write_all(f, old_size - 1, "\n", 1);
  (void)ftruncate(f, (off_t)old_size);
  close(f);
}
