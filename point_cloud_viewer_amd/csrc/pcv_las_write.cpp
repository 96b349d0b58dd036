// pcv_las_write.cpp — LAS output on the host: the checks and the plan, the host twin of the device packer, the
// header, the append check and the file. No HIP and no context: failures come back as a status and a message.
#include "pcv_las_write.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>

namespace {

int fail(int code, std::string* why, const std::string& msg) {
  if (why) *why = msg;
  return code;
}
void put64(uint8_t* p, uint64_t v) { pcv_las_put32(p, (uint32_t)v), pcv_las_put32(p + 4, (uint32_t)(v >> 32)); }
void put_f64(uint8_t* p, double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  put64(p, b);
}
uint64_t get64(const uint8_t* p) { return (uint64_t)pcv_las_u32(p) | ((uint64_t)pcv_las_u32(p + 4) << 32); }
double get_f64(const uint8_t* p) {
  const uint64_t b = get64(p);
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}
bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

// the header's fixed offsets beside those of pcv_las.h
constexpr uint32_t kAtFileSourceId = 4, kAtGlobalEncoding = 6, kAtSystemId = 26, kAtSoftware = 58, kAtDay = 90, kAtYear = 92, kAtNumVlrs = 100,
                   kAtLegacyByReturn = 111, kAtBounds = 179, kAtNumEvlrs = 243, kAtByReturn64 = 255;

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

int field_id(const std::string& name) {
  for (uint32_t id = 0; id < kLasNumExtras; ++id)
    if (name == pcv_las_extra_name(id)) return (int)id;
  return -1;
}

}  // namespace

int pcv_las_write_make_plan(const pcv_las_write_params* params, const PcvLasSource& src, PcvLasWritePlan* plan, std::vector<int>* field_of,
                            bool* use_color, bool* use_intensity, pcv_las_write_info* info, std::string* why) {
  if (!params || !plan || !field_of || !use_color || !use_intensity) return fail(PCV_E_INVALID, why, "LAS: null argument");
  if (params->struct_size < sizeof(pcv_las_write_params)) return fail(PCV_E_INVALID, why, "pcv_las_write_params.struct_size is too small");
  if (params->open_mode != PCV_LAS_TRUNCATE && params->open_mode != PCV_LAS_APPEND) return fail(PCV_E_INVALID, why, "LAS: bad open_mode");
  const size_t ne = src.extra_names.size();
  // which field each extra of the source can fill
  std::vector<int> id_of(ne, -1);
  int have[kLasNumExtras];
  for (int& h : have) h = -1;
  uint32_t skipped = 0;
  for (size_t k = 0; k < ne; ++k) {
    const int id = field_id(src.extra_names[k]);
    if (id < 0) {
      ++skipped;
      continue;
    }
    if (src.extra_types[k] != pcv_las_extra_type((uint32_t)id))
      return fail(PCV_E_INVALID, why, "LAS: attribute '" + src.extra_names[k] + "' has data type " + std::to_string(src.extra_types[k]) +
                                          ", the LAS field of that name takes " + std::to_string(pcv_las_extra_type((uint32_t)id)));
    id_of[k] = id, have[id] = (int)k;
  }
  uint32_t format = params->point_format;
  if (format == PCV_LAS_FORMAT_AUTO) format = have[kLasNir] >= 0 ? 8 : have[kLasScannerChannel] >= 0 ? 7 : have[kLasGpsTime] >= 0 ? 3 : 2;
  if (format > 8 || format == 4 || format == 5)
    return fail(PCV_E_INVALID, why, "LAS: point data record format " + std::to_string(format) + " is not written (0 - 3 and 6 - 8 are)");
  uint32_t minor = params->version_minor;
  if (minor == 0) minor = format <= 3 ? 2 : 4;
  if (minor != 2 && minor != 4) return fail(PCV_E_INVALID, why, "LAS: version 1." + std::to_string(minor) + " is not written (1.2 and 1.4 are)");
  if (minor == 2 && format > 3) return fail(PCV_E_INVALID, why, "LAS: point data record format " + std::to_string(format) + " needs version 1.4");
  if (params->color_rule > PCV_LAS_WRITE_COLOR_RGB8) return fail(PCV_E_INVALID, why, "LAS: unknown color rule " + std::to_string(params->color_rule));
  const float is = params->intensity_scale == 0.0f ? 1.0f : params->intensity_scale;
  if (!std::isfinite(is)) return fail(PCV_E_INVALID, why, "LAS: intensity_scale is not finite");
  PcvLasWritePlan p{};
  p.f = pcv_las_format(format), p.stride = p.f.min_len, p.version_minor = minor, p.color_rule = params->color_rule, p.intensity_scale = is;
  for (int a = 0; a < 3; ++a) p.scale[a] = params->scale[a], p.offset[a] = params->auto_offset ? 0.0 : params->offset[a];
  if (int rc = pcv_las_write_check_offset(p, why)) return rc;  // (the resolved offset of auto_offset is checked by the caller)
  field_of->assign(ne, -1);
  if (!params->fields) {
    *use_color = p.f.rgb_at != 0, *use_intensity = src.has_intensity;
    for (size_t k = 0; k < ne; ++k)
      if (id_of[k] >= 0 && pcv_las_format_has(p.f, (uint32_t)id_of[k])) (*field_of)[k] = id_of[k];
  } else {
    *use_color = *use_intensity = false;
    for (uint32_t j = 0; j < params->num_fields; ++j) {
      if (!params->fields[j]) return fail(PCV_E_INVALID, why, "LAS: field " + std::to_string(j) + " is null");
      const std::string name = params->fields[j];
      const std::string lacks = "LAS: point data record format " + std::to_string(format) + " has no field '" + name + "'";
      if (name == "color") {
        if (!p.f.rgb_at) return fail(PCV_E_INVALID, why, lacks);
        *use_color = true;
      } else if (name == "intensity") {
        if (!src.has_intensity) return fail(PCV_E_INVALID, why, "Data type for attribute '" + name + "' not found.");
        *use_intensity = true;
      } else {
        const int id = field_id(name);
        if (id < 0 || have[id] < 0) {
          // an extra of the source under another name is no LAS field; one it lacks is the PLY writer's answer
          const bool foreign = id < 0 && std::find(src.extra_names.begin(), src.extra_names.end(), name) != src.extra_names.end();
          if (foreign) return fail(PCV_E_INVALID, why, "LAS: attribute '" + name + "' is no LAS field");
          return fail(PCV_E_INVALID, why, "Data type for attribute '" + name + "' not found.");
        }
        if (!pcv_las_format_has(p.f, (uint32_t)id)) return fail(PCV_E_INVALID, why, lacks);
        (*field_of)[(size_t)have[id]] = id;
      }
    }
  }
  *plan = p;
  if (info) {
    *info = pcv_las_write_info{};
    info->point_format = format, info->version_minor = minor, info->record_length = p.stride, info->header_size = kLasHeaderSize[minor];
    info->skipped_extras = skipped;
    for (int a = 0; a < 3; ++a) info->scale[a] = p.scale[a], info->offset[a] = p.offset[a];
  }
  return PCV_OK;
}

int pcv_las_write_check_offset(const PcvLasWritePlan& plan, std::string* why) {
  for (int a = 0; a < 3; ++a) {
    if (!(std::isfinite(plan.scale[a]) && plan.scale[a] > 0.0))
      return fail(PCV_E_INVALID, why, std::string("LAS: ") + "xyz"[a] + " scale factor must be finite and above 0");
    if (!std::isfinite(plan.offset[a])) return fail(PCV_E_INVALID, why, std::string("LAS: ") + "xyz"[a] + " offset is not finite");
  }
  return PCV_OK;
}

double pcv_las_floor_min(const double* v, uint64_t n) {
  if (n == 0) return 0.0;
  uint64_t best = ~0ull;
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t b;
    std::memcpy(&b, v + i, 8);
    best = std::min(best, pcv_las_order_key(b));
  }
  const uint64_t b = pcv_las_order_bits(best);
  double d;
  std::memcpy(&d, &b, 8);
  return std::floor(d);
}

void pcv_las_encode_records(const PcvLasWritePlan& pl, const double* x, const double* y, const double* z, uint64_t n, uint8_t* out,
                            PcvLasWriteAcc* acc) {
  PcvLasRecord r;
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t oor, cl, mk;
    pcv_las_make_record(pl, i, x[i], y[i], z[i], &r, &oor, &cl, &mk);
    pcv_las_put(pl.f, r, out + i * pl.stride);
    acc->out_of_range += oor, acc->clamped_intensity += cl, acc->masked_values += mk;
    const uint32_t slot = pcv_las_return_slot(pl.f, r);
    if (slot < 15) acc->by_return[slot] += 1;
    const int32_t v[3] = {r.X, r.Y, r.Z};
    for (int a = 0; a < 3; ++a) acc->hi[a] = std::max(acc->hi[a], pcv_las_hi_key(v[a])), acc->lo[a] = std::max(acc->lo[a], pcv_las_lo_key(v[a]));
  }
}

void pcv_las_write_fill_info(const PcvLasWritePlan& pl, const PcvLasWriteAcc& acc, uint64_t n, pcv_las_write_info* info) {
  info->point_format = pl.f.format, info->version_minor = pl.version_minor, info->record_length = pl.stride;
  info->header_size = kLasHeaderSize[pl.version_minor];
  info->num_records = n;
  for (int k = 0; k < 15; ++k) info->by_return[k] = acc.by_return[k];
  info->out_of_range = acc.out_of_range, info->clamped_intensity = acc.clamped_intensity, info->masked_values = acc.masked_values;
  for (int a = 0; a < 3; ++a) {
    info->scale[a] = pl.scale[a], info->offset[a] = pl.offset[a];
    info->max_xyz[a] = n ? (int32_t)(acc.hi[a] ^ 0x80000000u) : 0;
    info->min_xyz[a] = n ? (int32_t)(~acc.lo[a] ^ 0x80000000u) : 0;
    // the reader's own formula over the integer extremes
    info->bounds[2 * a] = n ? (double)info->max_xyz[a] * pl.scale[a] + pl.offset[a] : 0.0;
    info->bounds[2 * a + 1] = n ? (double)info->min_xyz[a] * pl.scale[a] + pl.offset[a] : 0.0;
  }
}

PcvLasTotals pcv_las_totals_of(const pcv_las_write_info& info) {
  PcvLasTotals t;
  t.count = info.num_records;
  for (int k = 0; k < 15; ++k) t.by_return[k] = info.by_return[k];
  for (int k = 0; k < 6; ++k) t.bounds[k] = info.bounds[k];
  return t;
}

PcvLasTotals pcv_las_totals_merge(const PcvLasTotals& a, const PcvLasTotals& b) {
  if (a.count == 0) return b;
  if (b.count == 0) return a;
  PcvLasTotals t = a;
  t.count += b.count;
  for (int k = 0; k < 15; ++k) t.by_return[k] += b.by_return[k];
  for (int k = 0; k < 6; ++k) t.bounds[k] = (k & 1) ? std::min(a.bounds[k], b.bounds[k]) : std::max(a.bounds[k], b.bounds[k]);
  return t;
}

uint32_t pcv_las_build_header(const pcv_las_write_params* params, const PcvLasWritePlan& pl, const PcvLasTotals& t, uint8_t* h) {
  const uint32_t size = kLasHeaderSize[pl.version_minor];
  std::memset(h, 0, kLasMaxHeader);
  std::memcpy(h + kLasAtSignature, "LASF", 4);
  pcv_las_put16(h + kAtFileSourceId, params->file_source_id), pcv_las_put16(h + kAtGlobalEncoding, params->global_encoding);
  // the GUID (8 .. 24) stays zero
  h[kLasAtVersionMajor] = 1, h[kLasAtVersionMinor] = (uint8_t)pl.version_minor;
  auto name = [&](uint32_t at, const char* given, const char* otherwise) {
    bool empty = true;
    for (int k = 0; k < 32; ++k) empty = empty && given[k] == 0;
    if (empty) std::memcpy(h + at, otherwise, std::strlen(otherwise));
    else std::memcpy(h + at, given, strnlen(given, 32));  // NUL padded behind the first NUL
  };
  name(kAtSystemId, params->system_identifier, "OTHER");
  name(kAtSoftware, params->generating_software, "point_cloud_viewer_amd");
  pcv_las_put16(h + kAtDay, params->day), pcv_las_put16(h + kAtYear, params->year);
  pcv_las_put16(h + kLasAtHeaderSize, size), pcv_las_put32(h + kLasAtOffsetToPoints, size);
  pcv_las_put32(h + kAtNumVlrs, 0);
  h[kLasAtFormat] = pl.f.format;
  pcv_las_put16(h + kLasAtRecordLength, pl.stride);
  if (!pl.f.modern) {  // the legacy fields: 1.2, and 1.4 with formats <= 5
    pcv_las_put32(h + kLasAtLegacyCount, (uint32_t)t.count);
    for (int k = 0; k < 5; ++k) pcv_las_put32(h + kAtLegacyByReturn + 4 * k, (uint32_t)t.by_return[k]);
  }
  for (int a = 0; a < 3; ++a) put_f64(h + kLasAtScale + 8 * a, pl.scale[a]), put_f64(h + kLasAtOffset + 8 * a, pl.offset[a]);
  for (int k = 0; k < 6; ++k) put_f64(h + kAtBounds + 8 * k, t.count ? t.bounds[k] : 0.0);
  if (pl.version_minor == 4) {  // waveform start, first EVLR, number of EVLRs stay zero
    put64(h + kLasAtCount64, t.count);
    for (int k = 0; k < 15; ++k) put64(h + kAtByReturn64 + 8 * k, t.by_return[k]);
  }
  return size;
}

int pcv_las_append_check(const char* path, const PcvLasWritePlan& pl, bool check_transform, bool* exists, PcvLasTotals* totals, double* scale,
                         double* offset, std::vector<uint8_t>* old_header, uint64_t* old_size, std::string* why) {
  *exists = false, *totals = PcvLasTotals{}, *old_size = 0;
  old_header->clear();
  if (!path) return fail(PCV_E_INVALID, why, "LAS: null argument");
  const std::string p(path);
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    if (errno == ENOENT) return PCV_OK;  // nothing to append to: written anew
    return fail(PCV_E_IO, why, "cannot read " + p + ": " + strerror(errno));
  }
  struct stat st;
  uint8_t h[kLasMaxHeader] = {};
  uint64_t got = 0;
  bool bad = fstat(fd, &st) != 0 || !S_ISREG(st.st_mode);
  while (!bad && got < kLasMaxHeader) {
    const ssize_t r = pread(fd, h + got, kLasMaxHeader - got, (off_t)got);
    if (r < 0) bad = true;
    if (r <= 0) break;
    got += (uint64_t)r;
  }
  close(fd);
  if (bad) return fail(PCV_E_IO, why, "cannot read " + p);
  const uint32_t size = kLasHeaderSize[pl.version_minor];
  auto differs = [&](const std::string& field, const std::string& theirs, const std::string& ours) {
    return fail(PCV_E_INVALID, why, p + " is not a file this call can append to: " + field + " is " + theirs + ", these params give " + ours);
  };
  if (got < 4 || std::memcmp(h, "LASF", 4) != 0) return differs("the file signature", "not LASF", "LASF");
  if (got < size) return differs("the file's length", std::to_string((uint64_t)st.st_size) + " bytes", "a header of " + std::to_string(size) + " bytes");
  if (h[kLasAtVersionMajor] != 1 || h[kLasAtVersionMinor] != pl.version_minor)
    return differs("the version", std::to_string(h[kLasAtVersionMajor]) + "." + std::to_string(h[kLasAtVersionMinor]), "1." + std::to_string(pl.version_minor));
  auto num = [&](const char* field, uint64_t theirs, uint64_t ours) { return theirs == ours ? PCV_OK : differs(field, std::to_string(theirs), std::to_string(ours)); };
  int rc;
  if ((rc = num("the header size", pcv_las_u16(h + kLasAtHeaderSize), size))) return rc;
  if ((rc = num("the offset to point data", pcv_las_u32(h + kLasAtOffsetToPoints), size))) return rc;
  if ((rc = num("the number of variable length records", pcv_las_u32(h + kAtNumVlrs), 0))) return rc;
  if ((rc = num("the point data record format", h[kLasAtFormat], pl.f.format))) return rc;
  if ((rc = num("the point data record length", pcv_las_u16(h + kLasAtRecordLength), pl.stride))) return rc;
  if (pl.version_minor == 4 && (rc = num("the number of extended variable length records", pcv_las_u32(h + kAtNumEvlrs), 0))) return rc;
  for (int a = 0; a < 3; ++a) {
    scale[a] = get_f64(h + kLasAtScale + 8 * a), offset[a] = get_f64(h + kLasAtOffset + 8 * a);
    if (check_transform && !same_bits(scale[a], pl.scale[a]))
      return differs(std::string("the ") + "xyz"[a] + " scale factor", std::to_string(scale[a]), std::to_string(pl.scale[a]));
    if (check_transform && !same_bits(offset[a], pl.offset[a]))
      return differs(std::string("the ") + "xyz"[a] + " offset", std::to_string(offset[a]), std::to_string(pl.offset[a]));
  }
  PcvLasTotals t;
  const uint64_t legacy = pcv_las_u32(h + kLasAtLegacyCount);
  t.count = pl.version_minor == 4 ? get64(h + kLasAtCount64) : legacy;
  if (pl.version_minor == 4 && (rc = num("the legacy number of point records", legacy, pl.f.modern ? 0 : t.count))) return rc;
  if (t.count >= 0xffffffffull || (uint64_t)st.st_size != size + t.count * pl.stride)
    return differs("the file's length", std::to_string((uint64_t)st.st_size) + " bytes",
                   "a header of " + std::to_string(size) + " bytes and " + std::to_string(t.count) + " records of " + std::to_string(pl.stride));
  if (pl.version_minor == 4) {
    for (int k = 0; k < 15; ++k) t.by_return[k] = get64(h + kAtByReturn64 + 8 * k);
  } else {
    for (int k = 0; k < 5; ++k) t.by_return[k] = pcv_las_u32(h + kAtLegacyByReturn + 4 * k);
  }
  for (int k = 0; k < 6; ++k) t.bounds[k] = get_f64(h + kAtBounds + 8 * k);
  *exists = true, *totals = t, *old_size = (uint64_t)st.st_size;
  old_header->assign(h, h + size);
  return PCV_OK;
}

int PcvLasFile::begin(const char* p, uint32_t header_size, bool exists, const PcvLasTotals& totals, const std::vector<uint8_t>& header,
                      uint64_t size, std::string* why) {
  if (!p || !p[0]) return fail(PCV_E_INVALID, why, "path is empty");
  path = p, fd = -1, opened = false, fresh = !exists;
  old_totals = exists ? totals : PcvLasTotals{};
  old_header = exists ? header : std::vector<uint8_t>();
  old_size = exists ? size : 0;
  body_at = exists ? size : header_size;
  return PCV_OK;
}

int PcvLasFile::open_for_rows(std::string* why) {
  fd = open(path.c_str(), fresh ? (O_WRONLY | O_CREAT | O_TRUNC) : O_WRONLY, 0644);
  if (fd < 0) return fail(PCV_E_IO, why, "cannot open " + path + " for writing: " + strerror(errno));
  opened = true;
  return PCV_OK;
}

int PcvLasFile::write_at(uint64_t offset, const void* data, uint64_t bytes, std::string* why) {
  if (!write_all(fd, body_at + offset, data, bytes)) return fail(PCV_E_IO, why, "cannot write " + path + ": " + strerror(errno));
  return PCV_OK;
}

int PcvLasFile::commit(const uint8_t* header, uint32_t header_size, std::string* why) {
  const bool ok = write_all(fd, 0, header, header_size);
  const int e = errno;
  const bool closed = close(fd) == 0;
  fd = -1;
  if (!ok || !closed) {
    fail(PCV_E_IO, why, "cannot write " + path + ": " + strerror(ok ? errno : e));
    abandon();
    return PCV_E_IO;
  }
  return PCV_OK;
}

void PcvLasFile::abandon() {
  if (fd >= 0) close(fd);
  fd = -1;
  if (!opened) return;  // nothing of this call has reached the file
  opened = false;
  if (fresh) {
    unlink(path.c_str());
    return;
  }
  const int f = open(path.c_str(), O_WRONLY);
  if (f < 0) return;
  (void)write_all(f, 0, old_header.data(), old_header.size());
  (void)ftruncate(f, (off_t)old_size);
  close(f);
}
