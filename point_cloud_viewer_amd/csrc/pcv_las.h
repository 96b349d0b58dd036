// pcv_las.h — ASPRS LAS 1.0 - 1.4 as plain host C++: the public header block, the field table of point data record
// formats 0 - 10, the decode of one record and the rules for position, colour, filter and extras. Stated once: the host reader
// (pcv_las.cpp) and the device kernels (pcv_las.hip) both read the functions below. No HIP in pcv_las.cpp; here only the
// host / device markers where a HIP compiler reads the file.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pcv_hip.h"

#ifdef __HIPCC__
#define PCV_LAS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PCV_LAS_HD inline
#endif

// ---- the public header block: fixed offsets -----------------------------------------------------------------------------
constexpr uint32_t kLasAtSignature = 0, kLasAtVersionMajor = 24, kLasAtVersionMinor = 25, kLasAtHeaderSize = 94, kLasAtOffsetToPoints = 96,
                   kLasAtFormat = 104, kLasAtRecordLength = 105, kLasAtLegacyCount = 107, kLasAtScale = 131, kLasAtOffset = 155,
                   kLasAtCount64 = 247;
constexpr uint32_t kLasHeaderSize[5] = {227, 227, 227, 235, 375};  // by minor version
constexpr uint32_t kLasMaxHeader = 375;
constexpr uint32_t kLasMinRecord[11] = {20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67};

// ---- the field table ------------------------------------------------------------------------------------------------------
// Formats 0 - 5 ("legacy"): X 0, Y 4, Z 8 (i32), intensity 12 (u16), byte 14 = return number (bits 0-2) | number of returns (3-5) |
// scan direction (6) | edge of flight line (7), byte 15 = class (bits 0-4) | synthetic (5) | key-point (6) | withheld (7), scan
// angle rank 16 (i8, degrees), user data 17, point source id 18 (u16); then gps time (f64), R G B (u16 each) and the wave packet
// (29 bytes, skipped) as the format has them.
// Formats 6 - 10: X Y Z intensity as above, byte 14 = return number (bits 0-3) | number of returns (4-7), byte 15 = class flags
// (bits 0-3: synthetic, key-point, withheld, overlap) | scanner channel (4-5) | scan direction (6) | edge of flight line (7),
// class 16, user data 17, scan angle 18 (i16, units of 0.006 degrees), point source id 20, gps time 22; then R G B, NIR (u16) and
// the wave packet as the format has them.
struct PcvLasFormat {
  uint8_t format;
  uint8_t modern;   // 1: formats 6 - 10
  uint8_t min_len;  // kLasMinRecord
  uint8_t gps_at;   // byte offsets inside a record; 0 = the format has no such field
  uint8_t rgb_at;
  uint8_t nir_at;
};
PCV_LAS_HD PcvLasFormat pcv_las_format(uint32_t format) {
  PcvLasFormat f = {(uint8_t)format, (uint8_t)(format >= 6), 0, 0, 0, 0};
  switch (format) {
    case 0: f.min_len = 20; break;
    case 1: f.min_len = 28, f.gps_at = 20; break;
    case 2: f.min_len = 26, f.rgb_at = 20; break;
    case 3: f.min_len = 34, f.gps_at = 20, f.rgb_at = 28; break;
    case 4: f.min_len = 57, f.gps_at = 20; break;
    case 5: f.min_len = 63, f.gps_at = 20, f.rgb_at = 28; break;
    case 6: f.min_len = 30, f.gps_at = 22; break;
    case 7: f.min_len = 36, f.gps_at = 22, f.rgb_at = 30; break;
    case 8: f.min_len = 38, f.gps_at = 22, f.rgb_at = 30, f.nir_at = 36; break;
    case 9: f.min_len = 59, f.gps_at = 22; break;
    default: f.min_len = 67, f.gps_at = 22, f.rgb_at = 30, f.nir_at = 36; break;
  }
  return f;
}

// The extras, in the order of the contract's table.
enum PcvLasExtra : uint8_t {
  kLasClassification = 0,
  kLasClassificationFlags,
  kLasReturnNumber,
  kLasNumberOfReturns,
  kLasScanDirectionFlag,
  kLasEdgeOfFlightLine,
  kLasScannerChannel,
  kLasScanAngle,
  kLasUserData,
  kLasPointSourceId,
  kLasGpsTime,
  kLasNir,
  kLasNumExtras
};
static_assert(kLasNumExtras == PCV_LAS_MAX_EXTRAS, "one slot per extra");
const char* pcv_las_extra_name(uint32_t id);
PCV_LAS_HD int32_t pcv_las_extra_type(uint32_t id) {
  return id == kLasScanAngle ? PCV_ATTR_F32 : id == kLasGpsTime ? PCV_ATTR_F64 : (id == kLasPointSourceId || id == kLasNir) ? PCV_ATTR_U16 : PCV_ATTR_U8;
}
PCV_LAS_HD uint32_t pcv_las_extra_bytes(uint32_t id) {
  return id == kLasScanAngle ? 4 : id == kLasGpsTime ? 8 : (id == kLasPointSourceId || id == kLasNir) ? 2 : 1;
}
PCV_LAS_HD bool pcv_las_format_has(const PcvLasFormat& f, uint32_t id) {
  return id == kLasScannerChannel ? f.modern != 0 : id == kLasGpsTime ? f.gps_at != 0 : id == kLasNir ? f.nir_at != 0 : id < kLasNumExtras;
}

// ---- one record -------------------------------------------------------------------------------------------------------------
struct PcvLasRecord {
  int32_t X, Y, Z;
  uint16_t intensity;
  uint8_t return_number, number_of_returns, scan_direction, edge, classification, class_flags, channel, user_data;
  uint16_t point_source_id;
  uint16_t r, g, b, nir;
  float scan_angle;
  uint64_t gps_bits;
};
PCV_LAS_HD uint32_t pcv_las_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
PCV_LAS_HD uint32_t pcv_las_u32(const uint8_t* p) { return pcv_las_u16(p) | (pcv_las_u16(p + 2) << 16); }
// p: the first byte of the record, at any alignment, in any memory
PCV_LAS_HD void pcv_las_pick(const PcvLasFormat& f, const uint8_t* p, PcvLasRecord* r) {
  r->X = (int32_t)pcv_las_u32(p), r->Y = (int32_t)pcv_las_u32(p + 4), r->Z = (int32_t)pcv_las_u32(p + 8);
  r->intensity = (uint16_t)pcv_las_u16(p + 12);
  const uint32_t b14 = p[14], b15 = p[15];
  if (f.modern) {
    r->return_number = (uint8_t)(b14 & 15), r->number_of_returns = (uint8_t)(b14 >> 4);
    r->class_flags = (uint8_t)(b15 & 15), r->channel = (uint8_t)((b15 >> 4) & 3);
    r->classification = p[16];
    r->scan_angle = (float)(int16_t)pcv_las_u16(p + 18) * 0.006f;
    r->point_source_id = (uint16_t)pcv_las_u16(p + 20);
  } else {
    r->return_number = (uint8_t)(b14 & 7), r->number_of_returns = (uint8_t)((b14 >> 3) & 7);
    r->classification = (uint8_t)(b15 & 31), r->class_flags = (uint8_t)(b15 >> 5), r->channel = 0;
    r->scan_angle = (float)(int8_t)p[16];
    r->point_source_id = (uint16_t)pcv_las_u16(p + 18);
  }
  const uint32_t sd = f.modern ? b15 : b14;  // scan direction (bit 6) and edge of flight line (bit 7) share a byte in both layouts
  r->scan_direction = (uint8_t)((sd >> 6) & 1), r->edge = (uint8_t)(sd >> 7);
  r->user_data = p[17];
  r->gps_bits = 0;
  if (f.gps_at) r->gps_bits = (uint64_t)pcv_las_u32(p + f.gps_at) | ((uint64_t)pcv_las_u32(p + f.gps_at + 4) << 32);
  r->r = r->g = r->b = r->nir = 0;
  if (f.rgb_at) r->r = (uint16_t)pcv_las_u16(p + f.rgb_at), r->g = (uint16_t)pcv_las_u16(p + f.rgb_at + 2), r->b = (uint16_t)pcv_las_u16(p + f.rgb_at + 4);
  if (f.nir_at) r->nir = (uint16_t)pcv_las_u16(p + f.nir_at);
}
// the class and the withheld flag alone (the filter's count pass)
PCV_LAS_HD void pcv_las_pick_filter(const PcvLasFormat& f, const uint8_t* p, uint32_t* classification, bool* withheld) {
  const uint32_t b15 = p[15];
  *classification = f.modern ? p[16] : (b15 & 31);
  *withheld = f.modern ? (b15 >> 2) & 1 : (b15 >> 7) & 1;
}

// ---- the rules --------------------------------------------------------------------------------------------------------------
struct PcvLasPlan {  // a header and params, checked and resolved; passed to the kernels by value
  PcvLasFormat f;
  uint32_t stride;
  uint32_t color_mode;  // as requested (AUTO stays AUTO until the maxima are known)
  uint32_t keep_intensity, use_transform, drop_withheld, filter_classes;
  uint32_t num_extras;
  uint8_t extra_id[PCV_LAS_MAX_EXTRAS];
  uint8_t constant_color[4];
  uint64_t class_mask[4];
  double scale[3], offset[3], iso[7];
};
// 0 kept, 1 dropped by class, 2 dropped as withheld
PCV_LAS_HD uint32_t pcv_las_verdict(const PcvLasPlan& pl, uint32_t classification, bool withheld) {
  if (pl.filter_classes && !((pl.class_mask[classification >> 6] >> (classification & 63)) & 1)) return 1;
  return pl.drop_withheld && withheld ? 2 : 0;
}
// x = (double)X * scale + offset: two IEEE roundings (the library is built without contraction); then, when asked for, the
// arithmetic of pcv_transform_points (quat_rotate and the translation, pcv_query_dev.h), operation for operation
PCV_LAS_HD void pcv_las_position(const PcvLasPlan& pl, const PcvLasRecord& r, double* x, double* y, double* z) {
  const double vx = (double)r.X * pl.scale[0] + pl.offset[0], vy = (double)r.Y * pl.scale[1] + pl.offset[1],
               vz = (double)r.Z * pl.scale[2] + pl.offset[2];
  if (!pl.use_transform) {
    *x = vx, *y = vy, *z = vz;
    return;
  }
  const double qx = pl.iso[3], qy = pl.iso[4], qz = pl.iso[5], qw = pl.iso[6];
  const double tx = (qy * vz - qz * vy) * 2.0, ty = (qz * vx - qx * vz) * 2.0, tz = (qx * vy - qy * vx) * 2.0;  // 2 (q x v)
  const double cx = qy * tz - qz * ty, cy = qz * tx - qx * tz, cz = qx * ty - qy * tx;                            // q x t
  *x = ((tx * qw + cx) + vx) + pl.iso[0];
  *y = ((ty * qw + cy) + vy) + pl.iso[1];
  *z = ((tz * qw + cz) + vz) + pl.iso[2];
}
// rule: RGB16, RGB8, INTENSITY or CONSTANT
PCV_LAS_HD void pcv_las_color(uint32_t rule, const uint8_t* constant, uint32_t max_intensity, uint32_t r, uint32_t g, uint32_t b, uint32_t intensity,
                              uint8_t* out) {
  if (rule == PCV_LAS_COLOR_RGB16) {
    out[0] = (uint8_t)(r >> 8), out[1] = (uint8_t)(g >> 8), out[2] = (uint8_t)(b >> 8);
  } else if (rule == PCV_LAS_COLOR_RGB8) {
    out[0] = (uint8_t)(r < 255 ? r : 255), out[1] = (uint8_t)(g < 255 ? g : 255), out[2] = (uint8_t)(b < 255 ? b : 255);
  } else if (rule == PCV_LAS_COLOR_INTENSITY) {
    out[0] = out[1] = out[2] = (uint8_t)(max_intensity == 0 ? 0 : intensity * 255u / max_intensity);
  } else {
    out[0] = constant[0], out[1] = constant[1], out[2] = constant[2];
  }
}
PCV_LAS_HD uint32_t pcv_las_resolve_rule(const PcvLasPlan& pl, uint32_t max_color) {
  if (pl.color_mode != PCV_LAS_COLOR_AUTO) return pl.color_mode;
  return !pl.f.rgb_at ? PCV_LAS_COLOR_INTENSITY : max_color > 255 ? PCV_LAS_COLOR_RGB16 : PCV_LAS_COLOR_RGB8;
}
// the value of extra `id` of a record into element `slot` of its column
PCV_LAS_HD void pcv_las_store_extra(uint32_t id, const PcvLasRecord& r, void* column, uint64_t slot) {
  switch (id) {
    case kLasClassification: ((uint8_t*)column)[slot] = r.classification; break;
    case kLasClassificationFlags: ((uint8_t*)column)[slot] = r.class_flags; break;
    case kLasReturnNumber: ((uint8_t*)column)[slot] = r.return_number; break;
    case kLasNumberOfReturns: ((uint8_t*)column)[slot] = r.number_of_returns; break;
    case kLasScanDirectionFlag: ((uint8_t*)column)[slot] = r.scan_direction; break;
    case kLasEdgeOfFlightLine: ((uint8_t*)column)[slot] = r.edge; break;
    case kLasScannerChannel: ((uint8_t*)column)[slot] = r.channel; break;
    case kLasScanAngle: ((float*)column)[slot] = r.scan_angle; break;
    case kLasUserData: ((uint8_t*)column)[slot] = r.user_data; break;
    case kLasPointSourceId: ((uint16_t*)column)[slot] = r.point_source_id; break;
    case kLasGpsTime: ((uint64_t*)column)[slot] = r.gps_bits; break;
    default: ((uint16_t*)column)[slot] = r.nir; break;
  }
}

// ---- host entries (pcv_las.cpp); *why receives the message of a failure -------------------------------------------------------
// The header block from the first `len` bytes of a file (kLasMaxHeader are enough) of `file_size` bytes in all. PCV_E_IO: the
// bytes end inside the header, or the file is shorter than header plus records.
int pcv_las_parse_header(const uint8_t* bytes, uint64_t len, uint64_t file_size, pcv_las_header* out, std::string* why);
int pcv_las_read_header(const char* path, pcv_las_header* out, std::string* why);
// checks a header that did not come from the parser as the parser would (the stage entries take one from the caller)
int pcv_las_check_header(const pcv_las_header* h, std::string* why);
int pcv_las_make_plan(const pcv_las_header* h, const pcv_las_params* params, PcvLasPlan* plan, std::string* why);
void pcv_las_decode_records(const PcvLasPlan& plan, const uint8_t* raw, uint64_t n, const pcv_las_columns* out, pcv_las_info* info);
struct pcv_las {
  uint64_t n = 0;  // kept points
  PcvLasPlan plan{};
  pcv_las_info info{};
  std::vector<double> x, y, z;
  std::vector<uint8_t> color;
  std::vector<float> intensity;
  std::vector<uint8_t> extras[PCV_LAS_MAX_EXTRAS];
};
int pcv_las_read_file(const char* path, const pcv_las_params* params, pcv_las** out, std::string* why);
