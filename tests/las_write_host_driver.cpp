// Stand-alone driver of the LAS output's host code for a sanitizer build (tests/test_las_write_cpu.py compiles it with
// csrc/pcv_las_write.cpp, csrc/pcv_las.cpp and -fsanitize=address,undefined; no library involved): argv[1] is a scratch path.
// The host twin encodes 257 points with the corners of every field into buffers of exactly the records' size for each of the
// seven formats and decodes them again (pick after put); the header builder writes a small file; the append check runs over
// that file, every truncation of it and every single-byte flip of its header. The driver checks the statuses and that an
// accepted file is one with the writer's own geometry; the sanitizers check the rest.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pcv_las_write.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static bool write_file(const char* path, const std::vector<uint8_t>& f) {
  std::FILE* fp = std::fopen(path, "wb");
  if (!fp) return false;
  const bool ok = f.empty() || std::fwrite(f.data(), 1, f.size(), fp) == f.size();
  return std::fclose(fp) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const char* scratch = argv[1];
  const uint64_t n = 257;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> x(n), y(n), z(n);
  std::vector<uint8_t> color(3 * n), u8[9];
  std::vector<float> intensity(n), angle(n);
  std::vector<uint16_t> source(n), nir(n);
  std::vector<uint64_t> gps(n);
  for (auto& c : u8) c.resize(n);
  for (uint64_t i = 0; i < n; ++i) {
    x[i] = (double)(int32_t)rnd() * 0.001, y[i] = (double)rnd() * 1e-4 - 2e5, z[i] = (double)(rnd() % 100000) * 0.01;
    for (int k = 0; k < 3; ++k) color[3 * i + k] = (uint8_t)rnd();
    for (auto& c : u8) c[i] = (uint8_t)rnd();
    intensity[i] = (float)(rnd() % 70000) - 2000.0f, angle[i] = (float)(rnd() % 500) - 250.0f;
    source[i] = (uint16_t)rnd(), nir[i] = (uint16_t)rnd(), gps[i] = ((uint64_t)rnd() << 32) | rnd();
  }
  x[0] = inf, x[1] = -inf, x[2] = nan, x[3] = 2147483.6475, x[4] = -2147483.6485, y[5] = nan, z[6] = 1e300;
  intensity[0] = (float)nan, intensity[1] = (float)inf, angle[0] = (float)nan, angle[1] = (float)-inf;
  const uint32_t formats[7] = {0, 1, 2, 3, 6, 7, 8};
  std::vector<uint8_t> small;  // a format 3 file of version 1.2
  uint32_t small_header = 0;
  for (uint32_t fmt : formats) {
    pcv_las_write_params params{};
    params.struct_size = sizeof(params), params.point_format = fmt;
    for (int a = 0; a < 3; ++a) params.scale[a] = 0.001;
    PcvLasSource src;
    src.has_intensity = true;
    for (uint32_t id = 0; id < kLasNumExtras; ++id) src.extra_names.push_back(pcv_las_extra_name(id)), src.extra_types.push_back(pcv_las_extra_type(id));
    src.extra_names.push_back("foreign"), src.extra_types.push_back(PCV_ATTR_I32);
    PcvLasWritePlan plan;
    std::vector<int> field_of;
    bool uc, ui;
    pcv_las_write_info info;
    std::string why;
    if (pcv_las_write_make_plan(&params, src, &plan, &field_of, &uc, &ui, &info, &why) != PCV_OK || info.skipped_extras != 1) return 3;
    if (uc) plan.cols.color = color.data();
    if (ui) plan.cols.intensity = intensity.data();
    int used = 0;
    for (size_t k = 0; k < field_of.size(); ++k) {
      if (field_of[k] < 0) continue;
      const uint32_t id = (uint32_t)field_of[k];
      plan.cols.extra[id] = id == kLasScanAngle ? (const uint8_t*)angle.data()
                            : id == kLasPointSourceId ? (const uint8_t*)source.data()
                            : id == kLasNir ? (const uint8_t*)nir.data()
                            : id == kLasGpsTime ? (const uint8_t*)gps.data()
                                                : u8[used++ % 9].data();
    }
    plan.offset[0] = pcv_las_floor_min(x.data() + 3, n - 3), plan.offset[1] = pcv_las_floor_min(y.data() + 6, n - 6), plan.offset[2] = 0.0;
    if (pcv_las_write_check_offset(plan, &why) != PCV_OK) return 3;
    std::vector<uint8_t> out(n * plan.stride);  // exactly: a byte past a record is a sanitizer report
    PcvLasWriteAcc acc{};
    pcv_las_encode_records(plan, x.data(), y.data(), z.data(), n, out.data(), &acc);
    pcv_las_write_fill_info(plan, acc, n, &info);
    if (info.out_of_range < 5 ||info.clamped_intensity < 2 || info.num_records != n) return 4;
    const PcvLasFormat f = pcv_las_format(fmt);
    for (uint64_t i = 0; i < n; ++i) {  // pick after put: the masked fields, and the same bytes when put again
      PcvLasRecord r;
      pcv_las_pick(f, out.data() + i * plan.stride, &r);
      uint8_t again[40];
      pcv_las_put(f, r, again);
      if (std::memcmp(again, out.data() + i * plan.stride, plan.stride) != 0) return 5;
    }
    uint8_t header[kLasMaxHeader];
    const uint32_t hs = pcv_las_build_header(&params, plan, pcv_las_totals_of(info), header);
    if (hs != kLasHeaderSize[plan.version_minor]) return 6;
    pcv_las_header parsed;
    std::vector<uint8_t> file(header, header + hs);
    file.insert(file.end(), out.begin(), out.end());
    if (pcv_las_parse_header(file.data(), hs, file.size(), &parsed, &why) != PCV_OK || parsed.num_points != n || parsed.point_format != fmt) return 6;
    if (fmt == 3) small.assign(file.begin(), file.begin() + hs + 5 * plan.stride), small_header = hs;
    // the append check over the whole file
    if (!write_file(scratch, file)) return 2;
    bool exists;
    PcvLasTotals t;
    double s[3], o[3];
    std::vector<uint8_t> old;
    uint64_t size;
    if (pcv_las_append_check(scratch, plan, true, &exists, &t, s, o, &old, &size, &why) != PCV_OK || !exists || t.count != n || size != file.size()) return 7;
  }
  // the small file: its count says 257, so as it stands it is refused; with the count set to 5 it is accepted
  PcvLasWritePlan plan{};
  plan.f = pcv_las_format(3), plan.stride = 34, plan.version_minor = 2;
  for (int a = 0; a < 3; ++a) plan.scale[a] = 0.001;
  pcv_las_put32(small.data() + kLasAtLegacyCount, 5);
  int cases = 0, accepted = 0;
  auto run_case = [&](const std::vector<uint8_t>& f) -> bool {
    if (!write_file(scratch, f)) return false;
    ++cases;
    bool exists;
    PcvLasTotals t;
    double s[3], o[3];
    std::vector<uint8_t> old;
    uint64_t size;
    std::string why;
    const int rc = pcv_las_append_check(scratch, plan, false, &exists, &t, s, o, &old, &size, &why);
    if (rc != PCV_OK && rc != PCV_E_INVALID) return false;
    if (rc != PCV_OK) return !why.empty();
    ++accepted;
    return exists && size == f.size() && old.size() == small_header && size == small_header + t.count * plan.stride;
  };
  if (!run_case(small) || accepted != 1) return 8;
  for (size_t k = 0; k < small.size(); ++k)  // every truncation
    if (!run_case(std::vector<uint8_t>(small.begin(), small.begin() + (long)k))) return 9;
  if (accepted != 1) return 9;
  for (size_t i = 0; i < small_header; ++i) {  // one byte of the header flipped
    std::vector<uint8_t> f(small);
    f[i] ^= (uint8_t)(1u << (i % 8));
    if (!run_case(f)) return 10;
  }
  std::vector<uint8_t> longer(small);
  longer.push_back(0);
  const int before = accepted;
  if (!run_case(longer) || accepted != before) return 11;  // over-long
  std::remove(scratch);
  bool exists = true;
  PcvLasTotals t;
  double s[3], o[3];
  std::vector<uint8_t> old;
  uint64_t size;
  std::string why;
  if (pcv_las_append_check(scratch, plan, false, &exists, &t, s, o, &old, &size, &why) != PCV_OK || exists) return 12;  // a missing file
  std::printf("%d cases, %d accepted\n", cases, accepted);
  return 0;
}
