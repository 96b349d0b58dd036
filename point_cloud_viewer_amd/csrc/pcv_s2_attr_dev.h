// pcv_s2_attr_dev.h — the typed extra attributes of an S2 cell cloud: the data types of the reference's
// AttributeDataType (src/attributes.rs:8-21, 64-73) and the one filter test, `value.to_f64()` in a ClosedInterval<f64>
// (src/iterator.rs:82-91, math/mod.rs:86-88), as the device kernel and pcv_s2_filter_keep_host both compile it.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace s2attr {

// proto enum values (proto.proto AttributeDataType)
enum : int32_t { U8 = 1, U16 = 2, U32 = 3, U64 = 4, I8 = 6, I16 = 7, I32 = 8, I64 = 9, F32 = 11, F64 = 12, U8Vec3 = 27, F64Vec3 = 38 };

// bytes per element; 0: not a data type
__host__ __device__ inline uint32_t element_size(int32_t t) {
  switch (t) {
    case U8: case I8: return 1;
    case U16: case I16: return 2;
    case U32: case I32: case F32: return 4;
    case U64: case I64: case F64: return 8;
    case U8Vec3: return 3;
    case F64Vec3: return 24;
    default: return 0;
  }
}
__host__ __device__ inline bool is_scalar(int32_t t) { return element_size(t) != 0 && t != U8Vec3 && t != F64Vec3; }
// the word a column is moved in (gathers, merge): 3-component types move as 3 words of their component
__host__ __device__ inline uint32_t word_size(int32_t t) { return t == U8Vec3 ? 1u : t == F64Vec3 ? 8u : element_size(t); }

// Rust's `v as f64`: exact for every type but U64 / I64, which round to nearest, ties to even — what a C++ conversion does
// under the default rounding mode on the host and what the compiler's expansion does on the device. NaN fails both compares.
template <typename T>
__host__ __device__ inline bool keep(T v, double lo, double hi) {
  const double a = (double)v;
  return lo <= a && a <= hi;
}

// Rust `f64 as i64`: truncation, saturating; NaN -> 0 (the bin of xray/src/generation.rs:150)
__host__ __device__ inline int64_t rust_i64(double v) {
  if (v != v) return 0;
  if (v >= 9223372036854775808.0) return INT64_MAX;
  if (v < -9223372036854775808.0) return INT64_MIN;
  return (int64_t)v;
}

// BinnedColoringStrategy::bins (xray/src/generation.rs:138-157) for every 1-d data type: `(e as f64 / size) as i64`. The
// conversion is keep's; the division is one correctly rounded f64 division (no contraction, no fast math), and `size` is not
// validated: 0 gives +-inf or NaN, which rust_i64 saturates or sends to 0. The xray raster (pcv_xray.hip) and
// pcv_xray_bins_host both compile this.
template <typename T>
__host__ __device__ inline int64_t bin(T v, double size) {
  return rust_i64((double)v / size);
}

// f(T{}) for the scalar type t; false: t is no scalar type
template <typename F>
inline bool dispatch_scalar(int32_t t, F&& f) {
  switch (t) {
    case U8: f(uint8_t{}); return true;
    case U16: f(uint16_t{}); return true;
    case U32: f(uint32_t{}); return true;
    case U64: f(uint64_t{}); return true;
    case I8: f(int8_t{}); return true;
    case I16: f(int16_t{}); return true;
    case I32: f(int32_t{}); return true;
    case I64: f(int64_t{}); return true;
    case F32: f(float{}); return true;
    case F64: f(double{}); return true;
    default: return false;
  }
}

}  // namespace s2attr
