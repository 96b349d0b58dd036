// pcv_las_write.h — query results as ASPRS LAS, the write half beside pcv_las.h: the inverse of pcv_las_pick, the
// quantiser and the rules for intensity, colour and scan angle, stated once for the host twin (pcv_las_write.cpp) and the
// kernels (pcv_las_write.hip); then the plan, the header builder, the append check and the file. No HIP in pcv_las_write.cpp;
// here only the host / device markers of pcv_las.h.
#pragma once
#include <cmath>

#include "pcv_las.h"

// ---- one record -------------------------------------------------------------------------------------------------------------
PCV_LAS_HD void pcv_las_put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8); }
PCV_LAS_HD void pcv_las_put32(uint8_t* p, uint32_t v) { pcv_las_put16(p, v), pcv_las_put16(p + 2, v >> 16); }

// F32 degrees -> the code of the layout: legacy (int8)clamp(rintf(a), -128, 127), modern (int16)clamp(rintf(a / 0.006f), -32768,
// 32767); NaN -> 0. The division is the correctly rounded IEEE one on the host and on the device (the library is built without
// fast-math; hipcc's f32 division is correctly rounded unless asked otherwise).
PCV_LAS_HD int32_t pcv_las_angle_code(bool modern, float a) {
  if (a != a) return 0;
  const float r = rintf(modern ? a / 0.006f : a);
  const float lo = modern ? -32768.0f : -128.0f, hi = modern ? 32767.0f : 127.0f;
  return (int32_t)(r < lo ? lo : r > hi ? hi : r);
}

// The widths of the bit fields: return number / number of returns, class, flags, channel.
PCV_LAS_HD uint32_t pcv_las_return_mask(const PcvLasFormat& f) { return f.modern ? 15u : 7u; }
PCV_LAS_HD uint32_t pcv_las_class_mask(const PcvLasFormat& f) { return f.modern ? 255u : 31u; }
PCV_LAS_HD uint32_t pcv_las_flags_mask(const PcvLasFormat& f) { return f.modern ? 15u : 7u; }
PCV_LAS_HD uint32_t pcv_las_channel_mask(const PcvLasFormat& f) { return f.modern ? 3u : 0u; }
// how many values of r are wider than their field in format f (pcv_las_put masks them)
PCV_LAS_HD uint32_t pcv_las_masked_count(const PcvLasFormat& f, const PcvLasRecord& r) {
  return (uint32_t)(r.return_number > pcv_las_return_mask(f)) + (uint32_t)(r.number_of_returns > pcv_las_return_mask(f)) +
         (uint32_t)(r.classification > pcv_las_class_mask(f)) + (uint32_t)(r.class_flags > pcv_las_flags_mask(f)) +
         (uint32_t)(r.channel > pcv_las_channel_mask(f)) + (uint32_t)(r.scan_direction > 1) + (uint32_t)(r.edge > 1);
}
// The exact inverse of pcv_las_pick: the same offsets and bit fields, legacy and modern. p: the first byte of the record, at any
// alignment, in any memory; f.min_len bytes are written, every one of them.
PCV_LAS_HD void pcv_las_put(const PcvLasFormat& f, const PcvLasRecord& r, uint8_t* p) {
  pcv_las_put32(p, (uint32_t)r.X), pcv_las_put32(p + 4, (uint32_t)r.Y), pcv_las_put32(p + 8, (uint32_t)r.Z);
  pcv_las_put16(p + 12, r.intensity);
  const uint32_t rm = pcv_las_return_mask(f), sd = ((r.scan_direction & 1u) << 6) | ((r.edge & 1u) << 7);
  const int32_t code = pcv_las_angle_code(f.modern != 0, r.scan_angle);
  if (f.modern) {
    p[14] = (uint8_t)((r.return_number & rm) | ((r.number_of_returns & rm) << 4));
    p[15] = (uint8_t)((r.class_flags & 15u) | ((r.channel & 3u) << 4) | sd);
    p[16] = r.classification;
    p[17] = r.user_data;
    pcv_las_put16(p + 18, (uint32_t)code);
    pcv_las_put16(p + 20, r.point_source_id);
  } else {
    p[14] = (uint8_t)((r.return_number & rm) | ((r.number_of_returns & rm) << 3) | sd);
    p[15] = (uint8_t)((r.classification & 31u) | ((r.class_flags & 7u) << 5));
    p[16] = (uint8_t)code;
    p[17] = r.user_data;
    pcv_las_put16(p + 18, r.point_source_id);
  }
  if (f.gps_at) pcv_las_put32(p + f.gps_at, (uint32_t)r.gps_bits), pcv_las_put32(p + f.gps_at + 4, (uint32_t)(r.gps_bits >> 32));
  if (f.rgb_at) pcv_las_put16(p + f.rgb_at, r.r), pcv_las_put16(p + f.rgb_at + 2, r.g), pcv_las_put16(p + f.rgb_at + 4, r.b);
  if (f.nir_at) pcv_las_put16(p + f.nir_at, r.nir);
}

// ---- the rules --------------------------------------------------------------------------------------------------------------
// X = (int32)rint((x - offset) / scale): one subtraction, one correctly rounded division (IEEE on the host and on the device:
// no fast-math, no contraction), round to nearest, ties to even. false (and *X = 0): the quotient is not inside
// (-2147483648.5, 2147483647.5) — NaN and the infinities among them —, which are exactly the quotients that round to an int32
// without the tie rule deciding about the range.
PCV_LAS_HD bool pcv_las_quantize(double x, double offset, double scale, int32_t* X) {
  const double q = (x - offset) / scale;
  if (!(q > -2147483648.5 && q < 2147483647.5)) {
    *X = 0;
    return false;
  }
  *X = (int32_t)rint(q);
  return true;
}
// float -> u16: v = intensity * scale (f32, one rounding); NaN -> 0; otherwise clamped to [0, 65535], then rintf. *clamped: NaN,
// or a value outside the range.
PCV_LAS_HD uint32_t pcv_las_intensity_u16(float intensity, float scale, bool* clamped) {
  const float v = intensity * scale;
  if (v != v) {
    *clamped = true;
    return 0;
  }
  *clamped = v < 0.0f || v > 65535.0f;
  return (uint32_t)rintf(v < 0.0f ? 0.0f : v > 65535.0f ? 65535.0f : v);
}
PCV_LAS_HD uint32_t pcv_las_color_u16(uint32_t rule, uint32_t c) {
  return rule == PCV_LAS_WRITE_COLOR_X257 ? c * 257u : rule == PCV_LAS_WRITE_COLOR_SHIFT8 ? c << 8 : c;
}
// a double as a key whose unsigned order is the total order of IEEE 754 (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)
PCV_LAS_HD uint64_t pcv_las_order_key(uint64_t bits) { return (bits >> 63) ? ~bits : bits | 0x8000000000000000ull; }
PCV_LAS_HD uint64_t pcv_las_order_bits(uint64_t key) { return (key >> 63) ? key & 0x7fffffffffffffffull : ~key; }

// Which column of the source feeds which field; null: nobody supplies it. Element i of a column belongs to point i.
struct PcvLasWriteCols {
  const uint8_t* color;     // 3 bytes per point
  const float* intensity;
  const uint8_t* extra[kLasNumExtras];  // in the table's types
};
// Checked and resolved params; passed to the kernels by value.
struct PcvLasWritePlan {
  PcvLasFormat f;
  uint32_t stride;  // == f.min_len
  uint32_t version_minor;
  uint32_t color_rule;
  float intensity_scale;
  double scale[3], offset[3];
  PcvLasWriteCols cols;
};
// What the header needs of the records, accumulated over the pieces; zero is its neutral state: the extremes are kept as
// keys under max (hi: X ^ 2^31 as u32; lo: ~ of that), so a zeroed block needs no other initial value.
struct PcvLasWriteAcc {
  unsigned long long by_return[15];
  unsigned long long out_of_range, clamped_intensity, masked_values;
  uint32_t hi[3], lo[3];
};
PCV_LAS_HD uint32_t pcv_las_hi_key(int32_t X) { return (uint32_t)X ^ 0x80000000u; }
PCV_LAS_HD uint32_t pcv_las_lo_key(int32_t X) { return ~pcv_las_hi_key(X); }

// Point i of the source at (x, y, z) as a record; what it adds to the three counters.
PCV_LAS_HD void pcv_las_make_record(const PcvLasWritePlan& pl, uint64_t i, double x, double y, double z, PcvLasRecord* r, uint32_t* out_of_range,
                                    uint32_t* clamped, uint32_t* masked) {
  const PcvLasWriteCols& c = pl.cols;
  const bool in_x = pcv_las_quantize(x, pl.offset[0], pl.scale[0], &r->X), in_y = pcv_las_quantize(y, pl.offset[1], pl.scale[1], &r->Y),
             in_z = pcv_las_quantize(z, pl.offset[2], pl.scale[2], &r->Z);
  const bool in = in_x && in_y && in_z;
  if (!in) r->X = r->Y = r->Z = 0;
  *out_of_range = in ? 0u : 1u;
  bool cl = false;
  r->intensity = c.intensity ? (uint16_t)pcv_las_intensity_u16(c.intensity[i], pl.intensity_scale, &cl) : (uint16_t)0;
  *clamped = cl ? 1u : 0u;
  r->r = r->g = r->b = 0;
  if (c.color) {
    const uint8_t* s = c.color + 3 * i;
    r->r = (uint16_t)pcv_las_color_u16(pl.color_rule, s[0]), r->g = (uint16_t)pcv_las_color_u16(pl.color_rule, s[1]),
    r->b = (uint16_t)pcv_las_color_u16(pl.color_rule, s[2]);
  }
  auto u8 = [&](uint32_t id, uint8_t none) { return c.extra[id] ? c.extra[id][i] : none; };
  r->classification = u8(kLasClassification, 0), r->class_flags = u8(kLasClassificationFlags, 0);
  r->return_number = u8(kLasReturnNumber, 1), r->number_of_returns = u8(kLasNumberOfReturns, 1);
  r->scan_direction = u8(kLasScanDirectionFlag, 0), r->edge = u8(kLasEdgeOfFlightLine, 0);
  r->channel = u8(kLasScannerChannel, 0), r->user_data = u8(kLasUserData, 0);
  r->scan_angle = c.extra[kLasScanAngle] ? reinterpret_cast<const float*>(c.extra[kLasScanAngle])[i] : 0.0f;
  r->point_source_id = c.extra[kLasPointSourceId] ? reinterpret_cast<const uint16_t*>(c.extra[kLasPointSourceId])[i] : (uint16_t)0;
  r->nir = c.extra[kLasNir] ? reinterpret_cast<const uint16_t*>(c.extra[kLasNir])[i] : (uint16_t)0;
  r->gps_bits = c.extra[kLasGpsTime] ? reinterpret_cast<const uint64_t*>(c.extra[kLasGpsTime])[i] : 0ull;
  *masked = pcv_las_masked_count(pl.f, *r);
}
// the slot of the by-return counts that a (masked) return number counts in; 15: nowhere
PCV_LAS_HD uint32_t pcv_las_return_slot(const PcvLasFormat& f, const PcvLasRecord& r) {
  const uint32_t v = r.return_number & pcv_las_return_mask(f);
  return v == 0 ? 15u : v - 1;
}

// ---- host entries (pcv_las_write.cpp); *why receives the message of a failure ------------------------------------------------
// The source as the plan maker sees it: what it has beside positions and colour.
struct PcvLasSource {
  bool has_intensity = false;
  std::vector<std::string> extra_names;
  std::vector<int32_t> extra_types;
};
// Checks the params against the source, chooses format and version, and says which field each extra of the source feeds:
// field_of[k] = the PcvLasExtra that extra k fills, -1 when it is not written (skipped, or not among `fields`). use_color /
// use_intensity: whether those columns are written. plan->cols stays empty: the caller points it at its columns. scale, offset
// of the params go into the plan as they are (auto_offset is the caller's to resolve); info: format, version, lengths, skipped_extras.
int pcv_las_write_make_plan(const pcv_las_write_params* params, const PcvLasSource& src, PcvLasWritePlan* plan, std::vector<int>* field_of,
                            bool* use_color, bool* use_intensity, pcv_las_write_info* info, std::string* why);
int pcv_las_write_check_offset(const PcvLasWritePlan& plan, std::string* why);  // scale finite and > 0, offset finite
// floor(min) of n doubles by the total-order key (0 for n == 0): the host twin of the min pass
double pcv_las_floor_min(const double* v, uint64_t n);
// The host twin of the packer: n points through pcv_las_make_record and pcv_las_put into out; acc accumulates.
void pcv_las_encode_records(const PcvLasWritePlan& plan, const double* x, const double* y, const double* z, uint64_t n, uint8_t* out,
                            PcvLasWriteAcc* acc);
// info's extremes, bounds, counts from the accumulator of `n` records; format, version, scale, offset from the plan
void pcv_las_write_fill_info(const PcvLasWritePlan& plan, const PcvLasWriteAcc& acc, uint64_t n, pcv_las_write_info* info);
// The totals a header states, as a file's header holds them (bounds as doubles: (double)X * scale + offset is monotone in X, so
// merging bounds is merging extremes).
struct PcvLasTotals {
  uint64_t count = 0;
  uint64_t by_return[15] = {};
  double bounds[6] = {};  // max x, min x, max y, min y, max z, min z; meaningless while count == 0
};
PcvLasTotals pcv_las_totals_of(const pcv_las_write_info& info);
PcvLasTotals pcv_las_totals_merge(const PcvLasTotals& a, const PcvLasTotals& b);
// every byte of the header (227 or 375) into out (kLasMaxHeader bytes); returns its size
uint32_t pcv_las_build_header(const pcv_las_write_params* params, const PcvLasWritePlan& plan, const PcvLasTotals& t, uint8_t* out);
// PCV_LAS_APPEND's check: *exists false for a missing file; otherwise the file's totals, scale and offset, its header bytes and
// length. PCV_E_INVALID naming the first field that differs from what this writer writes for the plan's format and version
// (and, with check_transform, its scale and offset); PCV_E_IO when the file cannot be read.
int pcv_las_append_check(const char* path, const PcvLasWritePlan& plan, bool check_transform, bool* exists, PcvLasTotals* totals, double* scale,
                         double* offset, std::vector<uint8_t>* old_header, uint64_t* old_size, std::string* why);

// The file of one write call, modelled on PcvPlyFile: nothing exists on disk before the first records arrive; commit writes the
// header last; abandon removes a new file and gives an appended one its old header and length back.
struct PcvLasFile {
  std::string path;
  int fd = -1;
  bool opened = false, fresh = true;
  uint64_t old_size = 0, body_at = 0;
  std::vector<uint8_t> old_header;
  PcvLasTotals old_totals;
  // append: the file was checked by pcv_las_append_check (exists, totals, header, size as it returned them)
  int begin(const char* path, uint32_t header_size, bool exists, const PcvLasTotals& totals, const std::vector<uint8_t>& header, uint64_t size,
            std::string* why);
  int open_for_rows(std::string* why);
  int write_at(uint64_t offset, const void* data, uint64_t bytes, std::string* why);  // from several threads, disjoint ranges
  int commit(const uint8_t* header, uint32_t header_size, std::string* why);
  void abandon();
};
