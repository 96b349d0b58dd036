// pcv_wmr_dev.h — the per-point chain of WebMercatorRect::contains (reference src/geometry/web_mercator_rect.rs:121-127,
// src/math/web_mercator.rs:38-50) shared by the host helpers (pcv_wmr.hip) and the point kernels (pcv_query.hip).
//
// One __host__ __device__ implementation per transcendental, in plain f64 arithmetic: + - * / and sqrt only (IEEE, correctly
// rounded on both sides), no libm, no contraction (-ffp-contract=off) — so neither glibc nor the device math library decides
// a keep flag: the device's flag IS pcv_wmr_contains, bit for bit. Errors against libm / mpmath: DESIGN §5.
//
// ECEF -> WGS84 is nav-types' conversion, which is not vendored: restated as Bowring's closed form (DESIGN §5, §8 "unpinned").
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace wmr {

constexpr double kA = 6378137.0;                // WGS84 semi-major axis
constexpr double kB = 6356752.314245179;        // a (1 - f), f = 1 / 298.257223563
constexpr double kE2 = 0.006694379990141317;    // f (2 - f)
constexpr double kEp2 = 0.006739496742276435;   // e^2 / (1 - e^2)
constexpr double kPi = 3.141592653589793;
constexpr double kPiO2 = 1.5707963267948966;
constexpr double kTwoPi = 6.283185307179586;            // web_mercator.rs:15
constexpr double kFrac14Pi = 0.07957747154594767;       // 0.25 * FRAC_1_PI (web_mercator.rs:17)
constexpr double kLatBoundRad = 1.4844222297453324;     // web_mercator.rs:10
constexpr double kLatBoundSin = 0.99627207622075;       // web_mercator.rs:13

__host__ __device__ inline double abs_f64(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  b &= 0x7fffffffffffffffull;
  memcpy(&x, &b, 8);
  return x;
}
__host__ __device__ inline bool sign_f64(double x) {
  uint64_t b;
  memcpy(&b, &x, 8);
  return (b >> 63) != 0;
}

// atan of t in [0, 1]: t = c + d with c = k / 8 the nearest eighth, atan t = atan c + atan((t - c) / (1 + t c)), the second
// argument within 1 / 16: the odd series to r^15 (next term 0.0625^17 / 17 < 2e-22).
__host__ __device__ inline double atan_unit(double t) {
  const double tab[9] = {0.0, 0.12435499454676144, 0.24497866312686414, 0.35877067027057225, 0.4636476090008061,
                         0.5585993153435624, 0.6435011087932844, 0.7188299996216245, 0.7853981633974483};
  const int k = (int)(t * 8.0 + 0.5);
  const double c = (double)k * 0.125;
  const double r = (t - c) / (1.0 + t * c), z = r * r;
  const double poly =
      z * (-1.0 / 3.0 + z * (1.0 / 5.0 + z * (-1.0 / 7.0 + z * (1.0 / 9.0 + z * (-1.0 / 11.0 + z * (1.0 / 13.0 + z * (-1.0 / 15.0)))))));
  return tab[k] + (r + r * poly);
}

// atan2(y, x), all quadrants; atan2(0, 0) = 0 with y's sign, NaN in -> NaN out
__host__ __device__ inline double atan2_f64(double y, double x) {
  if (x != x || y != y) return x + y;
  const double ay = abs_f64(y), ax = abs_f64(x);
  const bool swap = ay > ax;
  const double mx = swap ? ay : ax, mn = swap ? ax : ay;
  double r;
  if (mx == 0.0) {
    r = 0.0;
  } else if (mx > 1.7976931348623157e308) {  // an infinity: 0, pi / 4 or pi / 2 before the quadrant
    r = mn > 1.7976931348623157e308 ? 0.7853981633974483 : 0.0;
  } else {
    r = atan_unit(mn / mx);
  }
  if (swap) r = (kPiO2 - r) + 6.123233995736766e-17;
  if (sign_f64(x)) r = (kPi - r) + 1.2246467991473532e-16;
  return sign_f64(y) ? -r : r;
}

// sin and cos of x together: x = k pi / 2 + y with |y| <= pi / 4 (Cody-Waite in two pieces: exact for |k| < 2^20), then the
// fdlibm kernels (FreeBSD msun k_sin.c / k_cos.c coefficients) without their tail argument.
__host__ __device__ inline void sincos_f64(double x, double* s, double* c) {
  if (!(abs_f64(x) <= 1.0e6)) {  // outside what the chain can feed (|x| <= pi): NaN, never a wrong flag
    *s = *c = __builtin_nan("");
    return;
  }
  const double kf = x * 0.6366197723675814;
  const long long k = (long long)(kf + (sign_f64(kf) ? -0.5 : 0.5));
  const double fk = (double)k;
  const double y = (x - fk * 1.57079632673412561417e+00) - fk * 6.07710050650619224932e-11;
  const double z = y * y;
  const double rs = 8.33333333332248946124e-03 +
                    z * (-1.98412698298579493134e-04 + z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double sy = y + (z * y) * (-1.66666666666666324348e-01 + z * rs);
  const double rc = z * (4.16666666666666019037e-02 +
                         z * (-1.38888888888741095749e-03 +
                              z * (2.48015872894767294178e-05 + z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double hz = 0.5 * z, w = 1.0 - hz;
  const double cy = w + (((1.0 - w) - hz) + z * rc);
  switch ((int)(k & 3)) {
    case 0: *s = sy, *c = cy; break;
    case 1: *s = cy, *c = -sy; break;
    case 2: *s = -sy, *c = -cy; break;
    default: *s = -cy, *c = sy; break;
  }
}

// ln x for finite x > 0 (the chain feeds (1 + s) / (1 - s) with |s| <= 0.99627207622075: 1.9e-3 .. 535); fdlibm e_log.c:
// x = 2^k (1 + f), sqrt(1/2) <= 1 + f < sqrt(2), s = f / (2 + f), ln(1 + f) = f - (f^2 / 2 - s (f^2 / 2 + R(s^2)))
__host__ __device__ inline double ln_f64(double x) {
  if (x != x || x < 0.0) return __builtin_nan("");
  if (x == 0.0) return -__builtin_inf();
  if (x > 1.7976931348623157e308) return x;
  uint64_t bits;
  memcpy(&bits, &x, 8);
  int k = 0;
  if ((bits >> 52) == 0) {  // subnormal
    x = x * 18014398509481984.0;
    memcpy(&bits, &x, 8);
    k = -54;
  }
  k += (int)(bits >> 52) - 1023;
  bits = (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
  double m;
  memcpy(&m, &bits, 8);
  if (m > 1.4142135623730951) {
    m = m * 0.5;
    k = k + 1;
  }
  const double f = m - 1.0, s = f / (2.0 + f), z = s * s, w = z * z;
  const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
  const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
  const double R = t2 + t1, hfsq = 0.5 * f * f, dk = (double)k;
  return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

__host__ __device__ inline double clamp_f64(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }  // nalgebra::clamp

// WebMercatorCoord::from_lat_lng (web_mercator.rs:38-50)
__host__ __device__ inline void from_lat_lng(double lat, double lng, double* u, double* v) {
  double sy, cy;
  sincos_f64(clamp_f64(lat, -kLatBoundRad, kLatBoundRad), &sy, &cy);
  *u = 0.5 + lng / kTwoPi;
  *v = 0.5 - ln_f64((1.0 + sy) / (1.0 - sy)) * kFrac14Pi;
}

// ECEF -> WGS84 latitude / longitude (Bowring's closed form)
__host__ __device__ inline void ecef_to_lat_lng(double x, double y, double z, double* lat, double* lng) {
  const double p = sqrt(x * x + y * y);
  const double theta = atan2_f64(z * kA, p * kB);
  double st, ct;
  sincos_f64(theta, &st, &ct);
  *lat = atan2_f64(z + (kEp2 * kB) * ((st * st) * st), p - (kE2 * kA) * ((ct * ct) * ct));
  *lng = atan2_f64(y, x);
}

__host__ __device__ inline void project(double x, double y, double z, double* u, double* v) {
  double lat, lng;
  ecef_to_lat_lng(x, y, z, &lat, &lng);
  from_lat_lng(lat, lng, u, v);
}

// web_mercator_rect.rs:121-127: partial_le(north_west, wmc) && partial_lt(wmc, south_east), component-wise
__host__ __device__ inline bool contains(const double* r /* nw.x nw.y se.x se.y */, double x, double y, double z) {
  double u, v;
  project(x, y, z, &u, &v);
  return r[0] <= u && r[1] <= v && u < r[2] && v < r[3];
}

}  // namespace wmr
