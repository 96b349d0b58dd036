// pcv_wmr.hip — host side of PCV_SHAPE_WEB_MERCATOR_RECT: the constructor's checks, the polyhedron's corners and the
// per-point chain evaluated on the host (reference src/geometry/web_mercator_rect.rs, src/math/web_mercator.rs). None of
// these touches the device. The corners use libm (exp, asin, sin, cos) — they are computed once per shape, on the host, and
// handed to shape_setup_kernel; the per-point chain is pcv_wmr_dev.h, the same code the point kernels run.
#include <cmath>

#include "../../include/pcv_hip.h"
#include "pcv_wmr_dev.h"

namespace {

// WebMercatorCoord::from_zoomed_coordinate (web_mercator.rs:84-97)
bool from_zoomed_coordinate(const double c[2], uint32_t z, double out[2]) {
  if (z > 23 || !(std::fmin(c[0], c[1]) >= 0.0)) return false;
  const double zoom = (double)(256u << z);
  if (!(std::fmax(c[0], c[1]) < zoom)) return false;
  out[0] = c[0] / zoom;
  out[1] = c[1] / zoom;
  return true;
}

// WebMercatorCoord::to_lat_lng (web_mercator.rs:55-64)
void to_lat_lng(double u, double v, double* lat, double* lng) {
  const double cx = u - 0.5, cy = v - 0.5;
  const double sin_term = std::exp(-cy * (4.0 * wmr::kPi));
  const double one_over_sin_y = (sin_term + 1.0) * -0.5;
  double sin_y = (1.0 / one_over_sin_y) + 1.0;
  sin_y = wmr::clamp_f64(sin_y, -wmr::kLatBoundSin, wmr::kLatBoundSin);
  *lng = wmr::clamp_f64(cx * wmr::kTwoPi, -wmr::kPi, wmr::kPi);
  *lat = std::asin(sin_y);
}

// nav-types WGS84 -> ECEF: the prime-vertical radius form
void wgs84_to_ecef(double lat, double lng, double h, double* out) {
  const double sl = std::sin(lat), cl = std::cos(lat);
  const double n = wmr::kA / std::sqrt(1.0 - wmr::kE2 * sl * sl);
  out[0] = (n + h) * cl * std::cos(lng);
  out[1] = (n + h) * cl * std::sin(lng);
  out[2] = (n * (1.0 - wmr::kE2) + h) * sl;
}

}  // namespace

extern "C" int pcv_wmr_from_zoomed(const double min[2], const double max[2], uint32_t z, double params[4]) {
  if (!min || !max || !params) return PCV_E_INVALID;
  double nw[2], se[2];
  if (!from_zoomed_coordinate(min, z, nw) || !from_zoomed_coordinate(max, z, se)) return PCV_E_INVALID;
  const double scale = (double)(1u << z);
  const double dx = (max[0] - min[0]) / scale, dy = (max[1] - min[1]) / scale;
  double rx = std::fmod(dx, 256.0);  // f64::rem_euclid
  if (rx < 0.0) rx += 256.0;
  if (rx > 1.0 || dy > 1.0 || dy < 0.0) return PCV_E_INVALID;
  params[0] = nw[0];
  params[1] = nw[1];
  params[2] = se[0];
  params[3] = se[1];
  return PCV_OK;
}

extern "C" int pcv_wmr_corners(const double params[4], double corners[24]) {
  if (!params || !corners) return PCV_E_INVALID;
  double nlat, wlng, slat, elng;
  to_lat_lng(params[0], params[1], &nlat, &wlng);
  to_lat_lng(params[2], params[3], &slat, &elng);
  const double lo = -500.0, hi = 10000.0;  // MIN_ELEVATION_M, MAX_ELEVATION_M (web_mercator_rect.rs:12,26)
  wgs84_to_ecef(nlat, wlng, lo, corners + 0);   // NW down
  wgs84_to_ecef(nlat, elng, lo, corners + 3);   // NE down
  wgs84_to_ecef(slat, elng, lo, corners + 6);   // SE down
  wgs84_to_ecef(slat, wlng, lo, corners + 9);   // SW down
  wgs84_to_ecef(nlat, wlng, hi, corners + 12);  // NW up
  wgs84_to_ecef(nlat, elng, hi, corners + 15);  // NE up
  wgs84_to_ecef(slat, elng, hi, corners + 18);  // SE up
  wgs84_to_ecef(slat, wlng, hi, corners + 21);  // SW up
  return PCV_OK;
}

extern "C" int pcv_wmr_project(uint64_t n, const double* x, const double* y, const double* z, double* u, double* v) {
  if (n && (!x || !y || !z || !u || !v)) return PCV_E_INVALID;
  for (uint64_t i = 0; i < n; ++i) wmr::project(x[i], y[i], z[i], u + i, v + i);
  return PCV_OK;
}

extern "C" int pcv_wmr_contains(const double params[4], uint64_t n, const double* x, const double* y, const double* z, uint8_t* keep) {
  if (!params || (n && (!x || !y || !z || !keep))) return PCV_E_INVALID;
  for (uint64_t i = 0; i < n; ++i) keep[i] = wmr::contains(params, x[i], y[i], z[i]) ? 1 : 0;
  return PCV_OK;
}

extern "C" int pcv_wmr_from_lat_lng(uint64_t n, const double* lat, const double* lng, double* u, double* v) {
  if (n && (!lat || !lng || !u || !v)) return PCV_E_INVALID;
  for (uint64_t i = 0; i < n; ++i) wmr::from_lat_lng(lat[i], lng[i], u + i, v + i);
  return PCV_OK;
}

extern "C" int pcv_wmr_to_lat_lng(uint64_t n, const double* u, const double* v, double* lat, double* lng) {
  if (n && (!u || !v || !lat || !lng)) return PCV_E_INVALID;
  for (uint64_t i = 0; i < n; ++i) to_lat_lng(u[i], v[i], lat + i, lng + i);
  return PCV_OK;
}

extern "C" int pcv_wmr_math(int fn, uint64_t n, const double* a, const double* b, double* out, double* out2) {
  if (n && (!a || !out)) return PCV_E_INVALID;
  switch (fn) {
    case PCV_WMR_FN_ATAN2:
      if (n && !b) return PCV_E_INVALID;
      for (uint64_t i = 0; i < n; ++i) out[i] = wmr::atan2_f64(a[i], b[i]);
      return PCV_OK;
    case PCV_WMR_FN_SINCOS:
      if (n && !out2) return PCV_E_INVALID;
      for (uint64_t i = 0; i < n; ++i) wmr::sincos_f64(a[i], out + i, out2 + i);
      return PCV_OK;
    case PCV_WMR_FN_LN:
      for (uint64_t i = 0; i < n; ++i) out[i] = wmr::ln_f64(a[i]);
      return PCV_OK;
    default: return PCV_E_INVALID;
  }
}
