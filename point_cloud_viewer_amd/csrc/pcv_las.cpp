// pcv_las.cpp — LAS 1.0 - 1.4 on the host: the header parser, the checks and the host twin of the device decode, all
// through the field table and the rules of pcv_las.h. No HIP and no context: failures come back as a status and a message.
#include "pcv_las.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <new>

namespace {

const char* const kExtraNames[kLasNumExtras] = {"classification", "classification_flags", "return_number", "number_of_returns",
                                                "scan_direction_flag", "edge_of_flight_line", "scanner_channel", "scan_angle",
                                                "user_data", "point_source_id", "gps_time", "nir"};

int fail(int code, std::string* why, const std::string& msg) {
  if (why) *why = msg;
  return code;
}
uint64_t u64_at(const uint8_t* p) { return (uint64_t)pcv_las_u32(p) | ((uint64_t)pcv_las_u32(p + 4) << 32); }
double f64_at(const uint8_t* p) {
  const uint64_t b = u64_at(p);
  double d;
  std::memcpy(&d, &b, 8);
  return d;
}

// everything but the signature, the version and the LAZ bits, which only the file shows
int check_fields(const pcv_las_header* h, std::string* why) {
  if (h->version_major != 1) return fail(PCV_E_INVALID, why, "LAS: version major " + std::to_string(h->version_major) + " is not 1");
  if (h->version_minor > 4) return fail(PCV_E_INVALID, why, "LAS: version minor " + std::to_string(h->version_minor) + " is above 4");
  if (h->header_size < kLasHeaderSize[h->version_minor])
    return fail(PCV_E_INVALID, why, "LAS: header size " + std::to_string(h->header_size) + " is below the " + std::to_string(kLasHeaderSize[h->version_minor]) +
                                        " bytes of version 1." + std::to_string(h->version_minor));
  if (h->offset_to_points < h->header_size)
    return fail(PCV_E_INVALID, why, "LAS: offset to point data " + std::to_string(h->offset_to_points) + " is below the header size " + std::to_string(h->header_size));
  if (h->point_format > 10) return fail(PCV_E_INVALID, why, "LAS: point data record format " + std::to_string(h->point_format) + " is above 10");
  if (h->record_length < kLasMinRecord[h->point_format])
    return fail(PCV_E_INVALID, why, "LAS: point data record length " + std::to_string(h->record_length) + " is below the " +
                                        std::to_string(kLasMinRecord[h->point_format]) + " bytes of format " + std::to_string(h->point_format));
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(h->scale[a])) return fail(PCV_E_INVALID, why, std::string("LAS: ") + "xyz"[a] + " scale factor is not finite");
    if (!std::isfinite(h->offset[a])) return fail(PCV_E_INVALID, why, std::string("LAS: ") + "xyz"[a] + " offset is not finite");
  }
  if (h->num_points >= 0xffffffffull) return fail(PCV_E_INVALID, why, "LAS: number of point records " + std::to_string(h->num_points) + " is 2^32 - 1 or more");
  return PCV_OK;
}

}  // namespace

const char* pcv_las_extra_name(uint32_t id) { return id < kLasNumExtras ? kExtraNames[id] : ""; }

int pcv_las_check_header(const pcv_las_header* h, std::string* why) {
  if (!h) return fail(PCV_E_INVALID, why, "LAS: null header");
  return check_fields(h, why);
}

int pcv_las_parse_header(const uint8_t* bytes, uint64_t len, uint64_t file_size, pcv_las_header* out, std::string* why) {
  if (!bytes || !out) return fail(PCV_E_INVALID, why, "LAS: null argument");
  *out = pcv_las_header{};
  if (len < 4) return fail(PCV_E_IO, why, "LAS: the file ends inside the public header block");
  if (std::memcmp(bytes + kLasAtSignature, "LASF", 4) != 0) return fail(PCV_E_INVALID, why, "LAS: file signature is not LASF");
  if (len < kLasAtVersionMinor + 1) return fail(PCV_E_IO, why, "LAS: the file ends inside the public header block");
  pcv_las_header h{};
  h.version_major = bytes[kLasAtVersionMajor], h.version_minor = bytes[kLasAtVersionMinor];
  if (h.version_major != 1 || h.version_minor > 4) return check_fields(&h, why);
  const uint32_t need = kLasHeaderSize[h.version_minor];
  if (len < need) return fail(PCV_E_IO, why, "LAS: the file ends inside the public header block");
  h.header_size = (uint16_t)pcv_las_u16(bytes + kLasAtHeaderSize);
  h.offset_to_points = pcv_las_u32(bytes + kLasAtOffsetToPoints);
  const uint32_t format_byte = bytes[kLasAtFormat];
  if (format_byte & 0xc0)
    return fail(PCV_E_INVALID, why, "LAS: point data record format byte " + std::to_string(format_byte) + " has a compression bit set: this is a LAZ file, which is not read");
  h.point_format = (uint8_t)format_byte;
  h.record_length = (uint16_t)pcv_las_u16(bytes + kLasAtRecordLength);
  const uint64_t legacy = pcv_las_u32(bytes + kLasAtLegacyCount);
  h.num_points = legacy;
  if (h.version_minor == 4) {
    h.num_points = u64_at(bytes + kLasAtCount64);
    if (legacy != 0 && legacy != h.num_points)
      return fail(PCV_E_INVALID, why, "LAS: legacy number of point records " + std::to_string(legacy) + " differs from the 64-bit number of point records " +
                                          std::to_string(h.num_points));
  }
  for (int a = 0; a < 3; ++a) h.scale[a] = f64_at(bytes + kLasAtScale + 8 * a), h.offset[a] = f64_at(bytes + kLasAtOffset + 8 * a);
  if (int rc = check_fields(&h, why)) return rc;
  // below 2^32 records of below 2^16 bytes: no overflow
  if (file_size < (uint64_t)h.offset_to_points + h.num_points * (uint64_t)h.record_length)
    return fail(PCV_E_IO, why, "LAS: the file is shorter than its header and " + std::to_string(h.num_points) + " point records of " +
                                   std::to_string(h.record_length) + " bytes");
  *out = h;
  return PCV_OK;
}

int pcv_las_read_header(const char* path, pcv_las_header* out, std::string* why) {
  if (!path || !out) return fail(PCV_E_INVALID, why, "LAS: null argument");
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return fail(PCV_E_IO, why, std::string("LAS: could not open ") + path);
  struct stat st;
  uint8_t head[kLasMaxHeader];
  uint64_t got = 0;
  bool bad = fstat(fd, &st) != 0;
  while (!bad && got < kLasMaxHeader) {
    const ssize_t r = pread(fd, head + got, kLasMaxHeader - got, (off_t)got);
    if (r < 0) bad = true;
    if (r <= 0) break;
    got += (uint64_t)r;
  }
  close(fd);
  if (bad) return fail(PCV_E_IO, why, std::string("LAS: could not read ") + path);
  return pcv_las_parse_header(head, got, (uint64_t)st.st_size, out, why);
}

int pcv_las_make_plan(const pcv_las_header* h, const pcv_las_params* params, PcvLasPlan* plan, std::string* why) {
  if (!h || !params || !plan) return fail(PCV_E_INVALID, why, "LAS: null argument");
  if (int rc = check_fields(h, why)) return rc;
  PcvLasPlan p{};
  p.f = pcv_las_format(h->point_format);
  p.stride = h->record_length;
  if (params->color_mode > PCV_LAS_COLOR_CONSTANT) return fail(PCV_E_INVALID, why, "LAS: unknown color mode " + std::to_string(params->color_mode));
  if ((params->color_mode == PCV_LAS_COLOR_RGB16 || params->color_mode == PCV_LAS_COLOR_RGB8) && !p.f.rgb_at)
    return fail(PCV_E_INVALID, why, std::string("LAS: color mode ") + (params->color_mode == PCV_LAS_COLOR_RGB16 ? "RGB16" : "RGB8") +
                                        " on point data record format " + std::to_string(h->point_format) + ", which has no colour");
  p.color_mode = params->color_mode;
  for (int k = 0; k < 3; ++k) p.constant_color[k] = params->constant_color[k];
  p.keep_intensity = params->keep_intensity != 0, p.use_transform = params->use_transform != 0, p.drop_withheld = params->drop_withheld != 0;
  for (int k = 0; k < 4; ++k) p.class_mask[k] = params->class_mask[k], p.filter_classes |= params->class_mask[k] != 0;
  for (int a = 0; a < 3; ++a) p.scale[a] = h->scale[a], p.offset[a] = h->offset[a];
  if (p.use_transform)
    for (int k = 0; k < 7; ++k) {
      if (!std::isfinite(params->global_from_local[k])) return fail(PCV_E_INVALID, why, "LAS: global_from_local is not finite");
      p.iso[k] = params->global_from_local[k];
    }
  if (params->num_extras > PCV_LAS_MAX_EXTRAS) return fail(PCV_E_INVALID, why, "LAS: more than " + std::to_string(PCV_LAS_MAX_EXTRAS) + " extras");
  uint32_t seen = 0;
  for (uint32_t k = 0; k < params->num_extras; ++k) {
    const char* name = params->extras[k];
    if (!name) return fail(PCV_E_INVALID, why, "LAS: null extra name");
    uint32_t id = 0;
    while (id < kLasNumExtras && std::strcmp(name, kExtraNames[id]) != 0) ++id;
    if (id == kLasNumExtras) return fail(PCV_E_INVALID, why, std::string("LAS: unknown attribute '") + name + "'");
    if (!pcv_las_format_has(p.f, id))
      return fail(PCV_E_INVALID, why, std::string("LAS: point data record format ") + std::to_string(h->point_format) + " has no attribute '" + name + "'");
    if (seen & (1u << id)) return fail(PCV_E_INVALID, why, std::string("LAS: attribute '") + name + "' is named twice");
    seen |= 1u << id;
    p.extra_id[k] = (uint8_t)id;
  }
  p.num_extras = params->num_extras;
  *plan = p;
  return PCV_OK;
}

// Two passes, as the device makes them: the maxima, histograms and counts over ALL records, then the kept records in file order
// under the colour rule the maxima decide.
void pcv_las_decode_records(const PcvLasPlan& pl, const uint8_t* raw, uint64_t n, const pcv_las_columns* out, pcv_las_info* info) {
  pcv_las_info in{};
  in.num_records = n;
  PcvLasRecord r;
  for (uint64_t i = 0; i < n; ++i) {
    pcv_las_pick(pl.f, raw + i * pl.stride, &r);
    const uint32_t c = r.r > r.g ? (r.r > r.b ? r.r : r.b) : (r.g > r.b ? r.g : r.b);
    if (c > in.max_color) in.max_color = c;
    if (r.intensity > in.max_intensity) in.max_intensity = r.intensity;
    in.class_hist[r.classification] += 1, in.return_hist[r.return_number] += 1;
    for (int b = 0; b < 4; ++b) in.flag_counts[b] += (r.class_flags >> b) & 1;
    const uint32_t v = pcv_las_verdict(pl, r.classification, (r.class_flags >> 2) & 1);
    in.dropped_class += v == 1, in.dropped_withheld += v == 2, in.num_kept += v == 0;
  }
  in.color_rule = pcv_las_resolve_rule(pl, in.max_color);
  if (out) {
    uint64_t slot = 0;
    for (uint64_t i = 0; i < n; ++i) {
      pcv_las_pick(pl.f, raw + i * pl.stride, &r);
      if (pcv_las_verdict(pl, r.classification, (r.class_flags >> 2) & 1) != 0) continue;
      pcv_las_position(pl, r, out->x + slot, out->y + slot, out->z + slot);
      pcv_las_color(in.color_rule, pl.constant_color, in.max_intensity, r.r, r.g, r.b, r.intensity, out->color + 3 * slot);
      if (pl.keep_intensity) out->intensity[slot] = (float)r.intensity;
      for (uint32_t k = 0; k < pl.num_extras; ++k) pcv_las_store_extra(pl.extra_id[k], r, out->extras[k], slot);
      ++slot;
    }
  }
  if (info) *info = in;
}

int pcv_las_read_file(const char* path, const pcv_las_params* params, pcv_las** out, std::string* why) {
  if (!out) return fail(PCV_E_INVALID, why, "LAS: out is null");
  *out = nullptr;
  if (!path || !params) return fail(PCV_E_INVALID, why, "LAS: null argument");
  pcv_las_header h;
  if (int rc = pcv_las_read_header(path, &h, why)) return rc;
  PcvLasPlan pl;
  if (int rc = pcv_las_make_plan(&h, params, &pl, why)) return rc;
  const uint64_t n = h.num_points, bytes = n * pl.stride;
  pcv_las* las = new (std::nothrow) pcv_las;
  if (!las) return fail(PCV_E_OOM, why, "LAS: no host memory");
  las->plan = pl;
  int rc = PCV_OK;
  try {
    std::vector<uint8_t> raw(bytes);
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) rc = fail(PCV_E_IO, why, std::string("LAS: could not open ") + path);
    uint64_t got = 0;
    while (rc == PCV_OK && got < bytes) {  // never past offset + count * length, which the header check found inside the file
      const ssize_t k = pread(fd, raw.data() + got, bytes - got, (off_t)(h.offset_to_points + got));
      if (k <= 0) rc = fail(PCV_E_IO, why, "LAS: unexpected end of file in the point records");
      else got += (uint64_t)k;
    }
    if (fd >= 0) close(fd);
    if (rc == PCV_OK) {
      // the kept count first, then columns of exactly that size
      pcv_las_decode_records(pl, raw.data(), n, nullptr, &las->info);
      const uint64_t m = las->info.num_kept;
      las->n = m;
      las->x.resize(m), las->y.resize(m), las->z.resize(m), las->color.resize(3 * m);
      if (pl.keep_intensity) las->intensity.resize(m);
      pcv_las_columns cols{};
      cols.x = las->x.data(), cols.y = las->y.data(), cols.z = las->z.data(), cols.color = las->color.data(), cols.intensity = las->intensity.data();
      for (uint32_t k = 0; k < pl.num_extras; ++k) {
        las->extras[k].resize(m * pcv_las_extra_bytes(pl.extra_id[k]));
        cols.extras[k] = las->extras[k].data();
      }
      pcv_las_decode_records(pl, raw.data(), n, &cols, &las->info);
      las->info.num_pieces = 1;
    }
  } catch (const std::bad_alloc&) {
    rc = fail(PCV_E_OOM, why, "LAS: no host memory for " + std::to_string(n) + " records");
  }
  if (rc != PCV_OK) {
    delete las;
    return rc;
  }
  *out = las;
  return PCV_OK;
}
