// pcv_terrain_files.cpp — terrain layers, the part that needs no device: the parameter rules, the frame, the reader's
// on-disk contract (sdl_viewer/src/terrain_drawer/read_write.rs: meta.json, x{:08}_y{:08}.height / .color) and the quad masks
// over a host bitmap. The JSON is made in pcv_terrain_meta_json and nowhere else: the array form of the isometry is how
// nalgebra 0.22 serialises Isometry3 as far as could be read.
#include "pcv_terrain_files.h"

#include <errno.h>
#include <fcntl.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

int pcv_terrain_check_params(const pcv_terrain_params* p, std::string* why) {
  auto bad = [&](const std::string& m) {
    *why = m;
    return PCV_E_INVALID;
  };
  if (!p) return bad("null pcv_terrain_params");
  if (p->tile_size == 0 || p->tile_size > 4096) return bad("tile_size must be in 1 ..= 4096, got " + std::to_string(p->tile_size));
  if (!(p->resolution_m > 0) || !std::isfinite(p->resolution_m)) return bad("resolution_m must be positive and finite");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(p->origin[a])) return bad("origin must be finite");
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(p->world_from_terrain[a])) return bad("world_from_terrain: the translation must be finite");
  const double* q = p->world_from_terrain + 3;
  const double s = ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3];
  if (!(std::fabs(s - 1.0) <= 1e-9)) return bad("world_from_terrain: the quaternion is not of unit length");
  if (p->min_points == 0) return bad("min_points must be at least 1");
  if (p->statistic > PCV_TERRAIN_MEAN) return bad("unknown statistic " + std::to_string(p->statistic));
  return PCV_OK;
}

PcvTerrainGrid pcv_terrain_grid(const pcv_terrain_params& p) {
  const double i = p.world_from_terrain[3], j = p.world_from_terrain[4], k = p.world_from_terrain[5], w = p.world_from_terrain[6];
  const double ii = i * i, jj = j * j, kk = k * k, ww = w * w;
  const double ij = i * j, ik = i * k, jk = j * k, wi = w * i, wj = w * j, wk = w * k;
  const double s = ((ii + jj) + kk) + ww;
  // R, the rotation of world_from_terrain, rows r0 r1 r2
  const double r[9] = {((ww + ii) - jj) - kk, 2.0 * (ij - wk),       2.0 * (ik + wj),
                       2.0 * (ij + wk),       ((ww - ii) + jj) - kk, 2.0 * (jk - wi),
                       2.0 * (ik - wj),       2.0 * (jk + wi),       ((ww - ii) - jj) + kk};
  PcvTerrainGrid g;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) g.m[3 * a + b] = r[3 * b + a] / s;  // M = R^T / |q|^2
  for (int a = 0; a < 3; ++a) g.t[a] = p.world_from_terrain[a], g.o[a] = p.origin[a];
  g.res = p.resolution_m;
  return g;
}

std::string pcv_terrain_tile_name(int32_t x, int32_t y) {
  char buf[40];
  snprintf(buf, sizeof buf, "x%08d_y%08d", (int)x, (int)y);  // the sign counts toward the width, as in Rust's {:08}
  return buf;
}

std::string pcv_terrain_f64_json(double v) {
  char buf[48];
  for (int digits = 15; digits <= 17; ++digits) {
    snprintf(buf, sizeof buf, "%.*g", digits, v);
    if (strtod(buf, nullptr) == v) break;
  }
  std::string s = buf;
  if (s.find_first_of(".en") == std::string::npos) s += ".0";  // integral, no exponent ('n': nan / inf never get here)
  return s;
}

std::string pcv_terrain_meta_json(const pcv_terrain_params& p, uint64_t num_tiles, const int32_t* positions) {
  auto f = pcv_terrain_f64_json;
  const double* w = p.world_from_terrain;
  std::string s = "{\"tile_size\":" + std::to_string(p.tile_size);
  s += ",\"world_from_terrain\":{\"rotation\":[" + f(w[3]) + "," + f(w[4]) + "," + f(w[5]) + "," + f(w[6]) + "]";
  s += ",\"translation\":[" + f(w[0]) + "," + f(w[1]) + "," + f(w[2]) + "]}";
  s += ",\"origin\":[" + f(p.origin[0]) + "," + f(p.origin[1]) + "," + f(p.origin[2]) + "]";
  s += ",\"resolution_m\":" + f(p.resolution_m);
  s += ",\"tile_positions\":[";
  for (uint64_t k = 0; k < num_tiles; ++k) {
    if (k) s += ",";
    s += "[" + std::to_string(positions[2 * k]) + "," + std::to_string(positions[2 * k + 1]) + "]";
  }
  s += "]}";
  return s;
}

namespace {

// a reader for meta.json's fixed schema: every failure names the key whose value was being read
struct MetaReader {
  const char* p;
  const char* end;
  std::string key = "the top-level object";
  std::string why;

  bool fail(const std::string& what) {
    if (why.empty()) why = "meta.json: " + what + " in \"" + key + "\"";
    return false;
  }
  void ws() {
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r')) ++p;
  }
  bool take(char c) {
    ws();
    if (p >= end) return fail(std::string("the text ends where '") + c + "' is expected");
    if (*p != c) return fail(std::string("'") + c + "' expected, found '" + *p + "'");
    ++p;
    return true;
  }
  bool peek(char c) {
    ws();
    return p < end && *p == c;
  }
  bool string(std::string* out) {
    if (!take('"')) return false;
    out->clear();
    while (p < end && *p != '"') {
      if (*p == '\\') {
        if (++p >= end) break;
      }
      out->push_back(*p++);
    }
    if (p >= end) return fail("the text ends inside a string");
    ++p;
    return true;
  }
  // the characters of one JSON number
  bool number_text(std::string* out) {
    ws();
    const char* q = p;
    while (q < end && *q && (std::strchr("+-.eE", *q) || (*q >= '0' && *q <= '9'))) ++q;
    if (q == p) return fail(p >= end ? "the text ends where a number is expected" : "a number expected");
    if (q == end) return fail("the text ends inside a number");  // a number is always followed by ',', ']' or '}'
    out->assign(p, q);
    p = q;
    return true;
  }
  bool f64(double* v) {
    std::string s;
    if (!number_text(&s)) return false;
    char* e = nullptr;
    *v = strtod(s.c_str(), &e);
    return (e && *e == 0) ? true : fail("not a number: " + s);
  }
  bool integer(int64_t lo, int64_t hi, int64_t* v) {
    std::string s;
    if (!number_text(&s)) return false;
    char* e = nullptr;
    errno = 0;
    const long long k = strtoll(s.c_str(), &e, 10);
    if (!e || *e != 0 || errno != 0 || k < lo || k > hi) return fail("not an integer in range: " + s);
    *v = k;
    return true;
  }
  bool f64_array(double* v, int n) {
    if (!take('[')) return false;
    for (int k = 0; k < n; ++k)
      if ((k && !take(',')) || !f64(&v[k])) return false;
    return take(']');
  }
  // any value, skipped (an unknown key: serde ignores it)
  bool skip(int depth = 0) {
    ws();
    if (p >= end) return fail("the text ends where a value is expected");
    if (depth > 64) return fail("nesting too deep");
    if (*p == '"') {
      std::string s;
      return string(&s);
    }
    if (*p == '[' || *p == '{') {
      const char close = *p == '[' ? ']' : '}';
      const bool object = *p == '{';
      ++p;
      if (peek(close)) return take(close);
      for (;;) {
        std::string s;
        if (object && (!string(&s) || !take(':'))) return false;
        if (!skip(depth + 1)) return false;
        if (peek(',')) {
          ++p;
          continue;
        }
        return take(close);
      }
    }
    const char* q = p;
    while (q < end && *q && !std::strchr(",]} \t\r\n", *q)) ++q;  // a number, true, false, null
    if (q == p) return fail("a value expected");
    p = q;
    return true;
  }
};

}  // namespace

int pcv_terrain_meta_read(const char* text, size_t len, pcv_terrain_params* out, std::vector<int32_t>* positions, std::string* why) {
  MetaReader r{text, text + len};
  pcv_terrain_params p{};
  p.statistic = PCV_TERRAIN_MAX, p.min_points = 1;
  positions->clear();
  bool have[5] = {false, false, false, false, false};
  static const char* const kKeys[5] = {"tile_size", "world_from_terrain", "origin", "resolution_m", "tile_positions"};
  auto bad = [&]() {
    *why = r.why;
    return PCV_E_INVALID;
  };
  if (!text) {
    *why = "meta.json: null text";
    return PCV_E_INVALID;
  }
  if (!r.take('{')) return bad();
  if (!r.peek('}')) {
    for (;;) {
      std::string key;
      if (!r.string(&key)) return bad();
      r.key = key;
      if (!r.take(':')) return bad();
      if (key == "tile_size") {
        int64_t v;
        if (!r.integer(0, 0xffffffffll, &v)) return bad();
        p.tile_size = (uint32_t)v, have[0] = true;
      } else if (key == "world_from_terrain") {
        bool rot = false, tra = false;
        if (!r.take('{')) return bad();
        if (!r.peek('}')) {
          for (;;) {
            std::string part;
            if (!r.string(&part) || !r.take(':')) return bad();
            if (part == "rotation") {
              if (!r.f64_array(p.world_from_terrain + 3, 4)) return bad();
              rot = true;
            } else if (part == "translation") {
              if (!r.f64_array(p.world_from_terrain, 3)) return bad();
              tra = true;
            } else if (!r.skip()) {
              return bad();
            }
            if (r.peek(',')) {
              ++r.p;
              continue;
            }
            break;
          }
        }
        if (!r.take('}')) return bad();
        if (!rot || !tra) {
          r.fail(rot ? "no \"translation\"" : "no \"rotation\"");
          return bad();
        }
        have[1] = true;
      } else if (key == "origin") {
        if (!r.f64_array(p.origin, 3)) return bad();
        have[2] = true;
      } else if (key == "resolution_m") {
        if (!r.f64(&p.resolution_m)) return bad();
        have[3] = true;
      } else if (key == "tile_positions") {
        if (!r.take('[')) return bad();
        positions->clear();
        if (!r.peek(']')) {
          for (;;) {
            int64_t x, y;
            if (!r.take('[') || !r.integer(INT32_MIN, INT32_MAX, &x) || !r.take(',') || !r.integer(INT32_MIN, INT32_MAX, &y) || !r.take(']')) return bad();
            positions->push_back((int32_t)x), positions->push_back((int32_t)y);
            if (r.peek(',')) {
              ++r.p;
              continue;
            }
            break;
          }
        }
        if (!r.take(']')) return bad();
        have[4] = true;
      } else if (!r.skip()) {
        return bad();
      }
      if (r.peek(',')) {
        ++r.p;
        continue;
      }
      break;
    }
  }
  if (!r.take('}')) return bad();
  for (int k = 0; k < 5; ++k)
    if (!have[k]) {
      *why = std::string("meta.json: missing key \"") + kKeys[k] + "\"";
      return PCV_E_INVALID;
    }
  if (int rc = pcv_terrain_check_params(&p, why)) {
    *why = "meta.json: " + *why;
    return rc;
  }
  *out = p;
  return PCV_OK;
}

int pcv_terrain_read_file(const std::string& path, void* data, size_t bytes, std::string* why) {
  const int fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    *why = "cannot open " + path + ": " + strerror(errno);
    return PCV_E_IO;
  }
  uint8_t* p = (uint8_t*)data;
  size_t done = 0;
  uint8_t extra;
  for (;;) {  // one byte past the end is asked for: a longer file is told from a whole one
    const ssize_t k = done < bytes ? read(fd, p + done, bytes - done) : read(fd, &extra, 1);
    if (k < 0 && errno == EINTR) continue;
    if (k < 0) {
      *why = "reading " + path + " failed: " + strerror(errno);
      close(fd);
      return PCV_E_IO;
    }
    if (k == 0) break;
    if (done >= bytes) {
      done += 1;
      break;
    }
    done += (size_t)k;
  }
  close(fd);
  if (done != bytes) {
    *why = path + ": " + std::to_string(bytes) + " bytes expected, the file has " + (done > bytes ? "more" : std::to_string(done));
    return PCV_E_INVALID;
  }
  return PCV_OK;
}

int pcv_terrain_read_text(const std::string& path, std::string* text, std::string* why) {
  const int fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) {
    *why = "cannot open " + path + ": " + strerror(errno);
    return PCV_E_IO;
  }
  text->clear();
  char buf[4096];
  for (;;) {
    const ssize_t k = read(fd, buf, sizeof buf);
    if (k < 0 && errno == EINTR) continue;
    if (k < 0) {
      *why = "reading " + path + " failed: " + strerror(errno);
      close(fd);
      return PCV_E_IO;
    }
    if (k == 0) break;
    text->append(buf, (size_t)k);
  }
  close(fd);
  return PCV_OK;
}

bool pcv_terrain_window_pos(const PcvTerrainGrid& g, const double c[3], uint32_t window, int64_t pos[2]) {
  const double dx = c[0] - g.t[0], dy = c[1] - g.t[1], dz = c[2] - g.t[2];
  const double lx = (g.m[0] * dx + g.m[1] * dy) + g.m[2] * dz;
  const double ly = (g.m[3] * dx + g.m[4] * dy) + g.m[5] * dz;
  const double gx = floor((lx - g.o[0]) / g.res), gy = floor((ly - g.o[1]) / g.res);
  const double lim = 9007199254740992.0;  // 2^53
  pos[0] = pos[1] = 0;
  if (!(fabs(gx) < lim) || !(fabs(gy) < lim)) return false;  // (a NaN fails)
  pos[0] = (int64_t)gx - (int64_t)(window / 2), pos[1] = (int64_t)gy - (int64_t)(window / 2);
  return true;
}

void pcv_terrain_quad_masks(int64_t i0, int64_t j0, uint32_t w, uint32_t h, const uint8_t* set, uint32_t* masks) {
  auto is_set = [&](int64_t c, int64_t r) { return c >= 0 && r >= 0 && c < (int64_t)w && r < (int64_t)h && set[(size_t)r * w + (size_t)c] != 0; };
  for (int64_t r = 0; r < (int64_t)h; ++r)
    for (int64_t c = 0; c < (int64_t)w; ++c) {
      uint32_t m = 0;
      for (int dy = -1; dy <= 0; ++dy)
        for (int dx = -1; dx <= 0; ++dx) {
          const int64_t qc = c + dx, qr = r + dy;  // the quad's lower corner, window coordinates
          if (is_set(qc, qr) && is_set(qc + 1, qr) && is_set(qc, qr + 1) && is_set(qc + 1, qr + 1)) m |= pcv_terrain_quad_bit(i0 + qc, j0 + qr);
        }
      masks[(size_t)r * w + (size_t)c] = m;
    }
}

int pcv_terrain_write_file(const std::string& path, const void* data, size_t bytes, std::string* why) {
  const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (fd < 0) {
    *why = "cannot create " + path + ": " + strerror(errno);
    return PCV_E_IO;
  }
  const uint8_t* p = (const uint8_t*)data;
  size_t done = 0;
  while (done < bytes) {
    const ssize_t k = write(fd, p + done, bytes - done);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) {
      *why = "writing " + path + " failed: " + strerror(errno);
      close(fd);
      return PCV_E_IO;
    }
    done += (size_t)k;
  }
  if (close(fd) != 0) {
    *why = "closing " + path + " failed: " + strerror(errno);
    return PCV_E_IO;
  }
  return PCV_OK;
}
