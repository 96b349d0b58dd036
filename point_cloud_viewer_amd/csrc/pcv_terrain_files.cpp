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
