// pcv_levels.h — the per-level constants of a cube (PcvLevels) and the host function that derives them. Standard C++: no HIP
// header, so that the table can be built and checked on a machine without a GPU (tests/test_levels_cpu.py).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/pcv_hip.h"

// Per-level constants handed to every kernel by value (lands in SGPRs; uniform across the grid).
// edge[k], enc[k] for k = 0..nlevels: see pcv_level_table / reference codec.rs:31-40, node.rs:161.
// A path key word holds PCV_MAX_KEY_LEVELS (21) levels. Trees that need more (heavy duplicates in a cube with
// edge / resolution > 2^21) take the "deep" path: a second key word for levels 22..PCV_MAX_LEVELS. 40 levels is what the
// reference's NodeId can name (u128: 8 bits of level + 120 bits of index, node.rs:101-111).
#define PCV_MAX_LEVELS 40
struct PcvLevels {
  double root_min[3];
  double edge[PCV_MAX_LEVELS + 2];
  double inv_edge[PCV_MAX_LEVELS + 2];     // yh = RN(1 / edge[k]) for the exact constant-divisor division
  double inv_edge_lo[PCV_MAX_LEVELS + 2];  // yl = RN(1 / edge[k] - yh): the reciprocal as a double-double
  uint32_t enc[PCV_MAX_LEVELS + 3];  // 32-bit entries: a wave-uniform lv.enc[L] is a scalar load (a byte would be a vector load)
  // Octant digit of level k + 1 straight from the integer codes of level k (pcv_chain_dev.h, pcv_digit_from_codes):
  // digit_half[k] = 127 / 32767 when level k is u8 / u16-coded and the rounding-error bound holds there, else -1
  double digit_half[PCV_MAX_LEVELS + 2];
  // how the single chain pass gets the digit of level k + 1 (pcv_chain_dev.h): 0 = comparison against the cube centre,
  // 1 = from the integer codes of level k (digit_half[k] = 127 / 32767), 2 = from the Float32 codes of level k
  // (digit_half[k] = 0.5; a code of exactly 0.5 falls back to the comparison) — an integer so that the test is scalar
  uint32_t digit_mode[PCV_MAX_LEVELS + 2];
  // Encodings narrow with depth (the edge halves per level): levels [first_u16, first_u8) are u16-coded, levels from
  // first_u8 on u8-coded; both are "never" (a huge level) when the table is not monotone. The single chain pass runs one
  // straight-line loop per range instead of a switch per level.
  int32_t first_u16, first_u8;
  int32_t first_f32;  // levels [first_f32, first_u16) are Float32-coded ("never" when the table is not monotone)
  // Float32 codes of level k + 1 straight from the Float32 codes of level k (round 5; pcv_chain_dev.h "codes from codes"):
  // for the level steps k in [code_begin, code_end) the chain pass computes w = 2 v - bit per coordinate and keeps it as the
  // level-(k + 1) code wherever code_thr_hi[k] <= hi32(w) < hi32(1.0) for all three coordinates (code_thr_hi[k] = the high
  // word of the power of two below which a code of level k + 1 is too close to the rounding noise of the f64 chain to be
  // predicted: the wave then runs the full step). code_begin == code_end: no step admitted.
  uint32_t code_thr_hi[PCV_MAX_KEY_LEVELS + 2];
  int32_t code_begin, code_end;
  int32_t nlevels;  // number of digit levels materialised in the keys (<= PCV_MAX_KEY_LEVELS; <= PCV_MAX_LEVELS deep)
  int32_t fast_ok;  // root min and all edges are tame: unguarded exact division is valid for tame points
};

// Levels 0..*max_level of the cube around [bmin, bmax] (at most `cap` below the root; the walk ends at the first level whose
// edge is <= resolution): edge and encoding per level into *edges / *encs, the kernels' constants into *lv. Every output may
// be null.
int pcv_make_levels(const double bmin[3], const double bmax[3], double resolution, int cap, PcvLevels* lv,
                    int* max_level, std::vector<double>* edges, std::vector<int32_t>* encs);
int pcv_bytes_per_coordinate(uint32_t enc);
