// pcv_levels.cpp — the level table of a cube (edges, encodings and the shortcuts the chain pass may take per level) and the
// promotion arithmetic of a node table: host arithmetic in standard C++, no HIP.
#include "pcv_levels.h"

#include <cmath>
#include <cstring>

#include "pcv_switches.h"

// ------------------------------------------------------------------------------------------------
// level table (host): reference codec.rs:31-40, node.rs:161, aabb.rs:149-157
// ------------------------------------------------------------------------------------------------
static uint32_t rust_as_u32(double v) {  // Rust `f64 as u32`: NaN -> 0, saturating, truncating
  if (!(v > 0.0)) return 0;
  if (v >= 4294967295.0) return 4294967295u;
  return (uint32_t)v;
}
static int position_encoding(double edge, double resolution) {
  uint32_t min_bits = rust_as_u32(std::log2(edge / resolution)) + 1u;  // wraps like a release build
  if (min_bits <= 8) return PCV_ENC_UINT8;
  if (min_bits <= 16) return PCV_ENC_UINT16;
  if (min_bits <= 24) return PCV_ENC_FLOAT32;
  return PCV_ENC_FLOAT64;
}

int pcv_make_levels(const double bmin[3], const double bmax[3], double resolution, int cap, PcvLevels* lv,
                    int* max_level, std::vector<double>* edges, std::vector<int32_t>* encs) {
  // Cube::bounding: f64::max chain of the extents (aabb.rs:149-157)
  double edge = std::fmax(std::fmax(bmax[0] - bmin[0], bmax[1] - bmin[1]), bmax[2] - bmin[2]);
  std::vector<double> e;
  std::vector<int32_t> c;
  e.push_back(edge);
  c.push_back(position_encoding(edge, resolution));
  int k = 0;
  while (k < cap) {
    ++k;
    edge /= 2.;
    e.push_back(edge);
    c.push_back(position_encoding(edge, resolution));
    if (edge <= resolution) break;  // generation.rs:137: such a node is never split
  }
  if (max_level) *max_level = k;
  if (lv) {
    std::memset(lv, 0, sizeof(*lv));
    for (int a = 0; a < 3; ++a) lv->root_min[a] = bmin[a];
    int nl = k < PCV_MAX_KEY_LEVELS ? k : PCV_MAX_KEY_LEVELS;
    lv->nlevels = nl;
    const int filled = k < PCV_MAX_LEVELS ? k : PCV_MAX_LEVELS;  // the tables cover the deep levels as well
    bool tame = std::fabs(bmin[0]) <= 0x1p+500 && std::fabs(bmin[1]) <= 0x1p+500 && std::fabs(bmin[2]) <= 0x1p+500;
    // largest |coordinate| of any cube min / max in the tree (every cube lies inside the root cube)
    double amax = 0.0;
    for (int a = 0; a < 3; ++a) amax = std::fmax(amax, std::fmax(std::fabs(bmin[a]), std::fabs(bmin[a] + e[0])));
    for (int j = 0; j < PCV_MAX_LEVELS + 2; ++j) lv->digit_half[j] = -1.0;
    for (int j = 0; j <= filled && j < (int)e.size(); ++j) {
      lv->edge[j] = e[j];
      // IEEE division on the host: correctly rounded reciprocal; 0 = "use plain division" (pcv_div_const)
      lv->inv_edge[j] = (e[j] >= 0x1p-100 && e[j] <= 0x1p+100) ? 1.0 / e[j] : 0.0;
      // low word of the double-double reciprocal: (1 - e * yh) is exact in one FMA, divided by e and rounded
      lv->inv_edge_lo[j] = lv->inv_edge[j] != 0.0 ? std::fma(-e[j], lv->inv_edge[j], 1.0) / e[j] : 0.0;
      lv->enc[j] = (uint32_t)c[j];
      tame = tame && lv->inv_edge[j] != 0.0;
      // pcv_digit_from_codes: valid where 1.01 u (2.5 A / e + 3) < 1 / (2 M) (u = 2^-53); required here with a factor
      // of two in hand. Level 0 has no codes (the chain starts from the raw position).
      if (j >= 1 && (c[j] == PCV_ENC_UINT8 || c[j] == PCV_ENC_UINT16) && std::isfinite(amax) && e[j] > 0.0) {
        const double m = c[j] == PCV_ENC_UINT8 ? 255.0 : 65535.0;
        if ((2.5 * amax / e[j] + 3.0) * 4.04 * m < 0x1p+53) {
          lv->digit_half[j] = c[j] == PCV_ENC_UINT8 ? 127.0 : 32767.0;
          lv->digit_mode[j] = 1;
        }
      }
      // pcv_f32 codes (pcv_chain_dev.h, pcv_bits_from_codes / pcv_f32_code_tie): the same inequality with M = 2^24 — the
      // floats next to 1/2 are 2^-25 away; only the single chain pass looks at digit_mode
      if (j >= 1 && c[j] == PCV_ENC_FLOAT32 && std::isfinite(amax) && e[j] > 0.0 &&
          (2.5 * amax / e[j] + 3.0) * 4.04 * 0x1p+24 < 0x1p+53) {
        lv->digit_half[j] = 0.5;
        lv->digit_mode[j] = 2;
      }
    }
    lv->fast_ok = tame ? 1 : 0;
    // "codes from codes" (pcv_chain_dev.h, round 5): the step from the Float32 codes of level j to those of level j + 1.
    // With v the level-j code, b = [v > 1/2] and w = 2 v - b (a float, exactly), the reference's chain computes
    //   t = (RN(RN(fma(v, e_j, m_j)) - RN(m_j + b e_{j+1})) / e_{j+1}) = w + delta,
    //   |delta| <= D = 1.01 (H / e_{j+1} + 3 u),   H = one ulp of the binade of the largest |coordinate| of the root cube
    // (each of the two roundings at that magnitude is off by at most H / 2; the subtraction and the division add at most
    // 2.1 u), and (float)clamp(t) == w whenever thr <= w < 1 for a power of two thr with D < thr 2^-25: the floats next to
    // w are at least thr 2^-24 away. The table stores the high word of the smallest such thr with a factor of two in hand;
    // steps whose thr would exceed 2^-8 are not admitted (most waves would hold a code below it).
    {
      const int none = 1 << 20;  // "no such step"
      int cb = none, ce = none;
      if (pcv_switches().code_steps && tame && std::isfinite(amax) && amax > 0.0) {
        const double H = std::ldexp(1.0, std::ilogb(amax * (1.0 + 0x1p-40)) - 52);
        for (int j = 1; j + 1 <= filled && j + 1 < (int)e.size() && j <= PCV_MAX_KEY_LEVELS; ++j) {
          if (c[j] != PCV_ENC_FLOAT32 || c[j + 1] != PCV_ENC_FLOAT32 || lv->digit_mode[j] != 2 || !(e[j + 1] > 0.0)) continue;
          const double D = (H / e[j + 1] + 3.0 * 0x1p-53) * 1.01;
          int ex = 0;
          (void)std::frexp(2.0 * D * 0x1p+25, &ex);  // 2 D 2^25 = f 2^ex, 1/2 <= f < 1: thr = 2^ex is strictly above it
          if (ex > -8) continue;
          if (ex < -100) ex = -100;
          lv->code_thr_hi[j] = (uint32_t)(1023 + ex) << 20;
        }
        for (cb = 1; cb <= PCV_MAX_KEY_LEVELS && !lv->code_thr_hi[cb]; ++cb) {
        }
        for (ce = cb; ce <= PCV_MAX_KEY_LEVELS && lv->code_thr_hi[ce]; ++ce) {
        }
        if (cb > PCV_MAX_KEY_LEVELS) cb = ce = none;
        for (int j = ce < PCV_MAX_KEY_LEVELS + 2 ? ce : PCV_MAX_KEY_LEVELS + 2; j < PCV_MAX_KEY_LEVELS + 2; ++j) lv->code_thr_hi[j] = 0;  // one contiguous range
      }
      lv->code_begin = cb;
      lv->code_end = ce;
    }
    {
      const int never = 1 << 20;
      int f16 = never, f8 = never, f32 = never;
      bool monotone = true;
      const int last = filled < (int)e.size() - 1 ? filled : (int)e.size() - 1;
      for (int j = 1; j <= last; ++j) {
        if (c[j] <= PCV_ENC_FLOAT32 && f32 == never) f32 = j;
        if (c[j] <= PCV_ENC_UINT16 && f16 == never) f16 = j;
        if (c[j] == PCV_ENC_UINT8 && f8 == never) f8 = j;
        if (j > 1 && c[j] > c[j - 1]) monotone = false;
      }
      if (f8 != never && f16 == never) f16 = f8;
      lv->first_f32 = monotone ? f32 : never;
      lv->first_u16 = monotone ? f16 : never;
      lv->first_u8 = monotone ? f8 : never;
    }
  }
  if (edges) *edges = e;
  if (encs) *encs = c;
  return PCV_OK;
}

extern "C" int pcv_level_table(const double bbox_min[3], const double bbox_max[3], double resolution, int cap,
                               double* edge, int32_t* encoding) {
  std::vector<double> e;
  std::vector<int32_t> c;
  int ml = 0;
  pcv_make_levels(bbox_min, bbox_max, resolution, cap, nullptr, &ml, &e, &c);
  for (int k = 0; k <= ml; ++k) {
    if (edge) edge[k] = e[k];
    if (encoding) encoding[k] = c[k];
  }
  return ml;
}

extern "C" int pcv_level_shortcuts(const double bbox_min[3], const double bbox_max[3], double resolution, uint32_t* digit_mode,
                                   double* code_threshold) {
  PcvLevels lv;
  int ml = 0;
  pcv_make_levels(bbox_min, bbox_max, resolution, PCV_MAX_LEVELS, &lv, &ml, nullptr, nullptr);
  for (int k = 0; k < PCV_MAX_KEY_LEVELS + 2; ++k) {
    if (digit_mode) digit_mode[k] = lv.digit_mode[k];
    if (code_threshold) {
      double thr = 0.0;
      if (k >= lv.code_begin && k < lv.code_end && lv.code_thr_hi[k]) {
        const uint64_t bits = (uint64_t)lv.code_thr_hi[k] << 32;
        std::memcpy(&thr, &bits, 8);
      }
      code_threshold[k] = thr;
    }
  }
  return ml;
}

int pcv_bytes_per_coordinate(uint32_t enc) { return enc == PCV_ENC_UINT8 ? 1 : enc == PCV_ENC_UINT16 ? 2 : enc == PCV_ENC_FLOAT32 ? 4 : 8; }

// ------------------------------------------------------------------------------------------------
// promotion arithmetic of a node table
// ------------------------------------------------------------------------------------------------
static uint64_t ceil8(uint64_t v) { return (v + 7) / 8; }  // (pcv_tables.h has the same as pcv_ceil8; that header needs HIP)

extern "C" int pcv_promote_assign(const pcv_split_node* nodes, uint64_t num_nodes, pcv_promote_node* per_node, uint64_t n,
                                  uint32_t* node_of_slot, uint32_t* slot_in_node) {
  if ((num_nodes && (!nodes || !per_node)) || ((node_of_slot == nullptr) != (slot_in_node == nullptr))) return PCV_E_INVALID;
  if (num_nodes == 0) return PCV_OK;
  if (num_nodes > 0xfffffffeull) return PCV_E_INVALID;
  const uint32_t m = (uint32_t)num_nodes;
  for (uint32_t i = 0; i < m; ++i) {  // children must follow their parent (breadth-first table) and exist
    if (nodes[i].is_leaf) continue;
    const uint32_t nchild = (uint32_t)__builtin_popcount(nodes[i].child_mask & 0xffu);
    if (nchild == 0 || nodes[i].first_child <= i || (uint64_t)nodes[i].first_child + nchild > m) return PCV_E_INVALID;
  }
  // bottom-up stream lengths: |pre(inner)| = sum ceil(|pre(child)| / 8)
  for (uint32_t i = m; i-- > 0;) {
    if (nodes[i].is_leaf) {
      per_node[i].stream_len = nodes[i].count;
    } else {
      uint64_t acc = 0;
      const uint32_t nchild = (uint32_t)__builtin_popcount(nodes[i].child_mask & 0xffu);
      for (uint32_t c = 0; c < nchild; ++c) {
        per_node[nodes[i].first_child + c].child_offset = acc;
        acc += ceil8(per_node[nodes[i].first_child + c].stream_len);
      }
      per_node[i].stream_len = acc;
    }
  }
  per_node[0].child_offset = 0;
  for (uint32_t i = 0; i < m; ++i)
    per_node[i].num_points = i == 0 ? per_node[0].stream_len : per_node[i].stream_len - ceil8(per_node[i].stream_len);
  if (!node_of_slot) return PCV_OK;
  for (uint32_t i = 0; i < m; ++i) {
    if (!nodes[i].is_leaf) continue;
    if (nodes[i].first + nodes[i].count > n) return PCV_E_INVALID;
    for (uint64_t j0 = 0; j0 < nodes[i].count; ++j0) {
      uint32_t node = i;
      uint64_t j = j0;
      while (node != 0 && (j & 7u) == 0) {  // an every-8th element of its stream climbs (generation.rs:222-238)
        j = per_node[node].child_offset + (j >> 3);
        node = nodes[node].parent;
        if (node >= m) return PCV_E_INVALID;
      }
      node_of_slot[nodes[i].first + j0] = node;
      slot_in_node[nodes[i].first + j0] = (uint32_t)(node == 0 ? j : j - (j >> 3) - 1);
    }
  }
  return PCV_OK;
}
