// pcv_tables.h — the node table between the topology and K6: where it lies in memory and the host arithmetic on it.
//
// pcv_build_begin stages the tree's node table in the context's pinned block; pcv_build_finish derives from it everything
// K5 / K6 need and sends that to the context's device block. This header is the ONE definition of both blocks:
//
//   pinned block   | download area | upload area | record block |           each area starts 256-byte aligned
//   device block   | walk words (K5) | record block | 256 spare bytes |     the record block is one contiguous upload
//
// and of the host rules that fill them — parity rules of the reference (node.rs:108-111 ids, node.rs:157-172 cubes, the
// |pre| stream lengths of SURVEY Appendix A). Host code that makes no HIP call and takes no pcv_ctx (the include below is for
// PcvNodeRec, PcvLevels and the ABI structs; it is compiled like pcv_spec.cpp): unit-tested on the CPU through
// pcv_tables_selftest (tests/test_tables_cpu.py) against the oracle.
#pragma once
#include "pcv_internal.h"

inline size_t pcv_align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }
inline uint64_t pcv_ceil8(uint64_t v) { return (v + 7) / 8; }

// ---- the staged node table (pinned block) -------------------------------------------------------------------------------
// BFS order, children contiguous in digit order, [lo, hi) = the node's range of key-sorted slots: what the node split leaves
// on the device and pcv_spec_resolve derives on the host (PcvTrueTree).
struct PcvStagedTable {
  uint32_t M = 0;
  // download area: copied from the device table / a PcvTrueTree
  uint64_t* prefix = nullptr;       // offset 0
  uint32_t* lo = nullptr;           // 8 M
  uint32_t* hi = nullptr;           // 12 M
  uint32_t* first_child = nullptr;  // 16 M
  uint8_t* level = nullptr;         // 20 M
  uint8_t* child_mask = nullptr;    // 21 M
  uint8_t* open = nullptr;          // 22 M (the area keeps room for 27 M + 64 bytes)
  uint64_t* prefix_lo = nullptr;    // deep trees only: align8(27 M + 64), second prefix word; null otherwise
  // upload area: filled on the host (walk words go to the device for K5; the rest feeds the node records)
  uint64_t* walk = nullptr;         // PcvWalkTables::walk
  uint64_t* xyz_off = nullptr;
  uint64_t* point_off = nullptr;
  double* node_min = nullptr;       // 3 per node
  uint32_t* parent = nullptr;       // 0xffffffff for the root
  uint32_t* child_off = nullptr;    // offset of the node's promoted block inside the parent's stream
  uint32_t* leaf_lo = nullptr;      // per leaf rank (<= M entries): first sorted slot
  uint32_t* leaf_node = nullptr;    // per leaf rank: node index
  uint8_t* node_level = nullptr;    // copy of `level`
  uint8_t* records = nullptr;       // the record block starts here
};
size_t pcv_staged_table_bytes(uint32_t M, bool deep);  // offset of the record block == bytes of the two areas
PcvStagedTable pcv_staged_table(void* base, uint32_t M, bool deep);

// ---- the record block ---------------------------------------------------------------------------------------------------
struct PcvRecordCounts {
  uint32_t M = 0, num_leaves = 0;
  uint32_t num_items = 0;       // settle items
  uint32_t num_citems = 0;      // climb items
  uint32_t num_cont = 0;        // leaves whose chain is continued (PcvTrueTree::cont_nodes)
  uint32_t num_cont_items = 0;  // one per <= kPcvSettleTile slots of such a leaf
  bool fused = false;           // the record sort's second pass settles leaves itself: one flag byte per leaf
};
// Sections in this order, each 16-byte aligned. Built once on the pinned block (to fill) and once on the device block (to
// pass to the sort and K6): same counts, same offsets.
struct PcvRecordBlock {
  PcvNodeRec* node_rec = nullptr;         // M
  PcvNodeRec* leaf_rec = nullptr;         // num_leaves, in leaf-rank order
  uint32_t* climb_base = nullptr;         // num_leaves
  PcvSettleItem* items = nullptr;         // num_items
  PcvSettleItem* citems = nullptr;        // num_citems
  uint8_t* cont_ranges = nullptr;         // num_cont x pcv_cont_range_bytes()
  PcvSettleItem* cont_items = nullptr;    // num_cont_items
  uint8_t* fused = nullptr;               // num_leaves bytes when counts.fused
  size_t bytes = 0;
};
PcvRecordBlock pcv_record_block(void* base, const PcvRecordCounts& c);
// device block: the walk words come first
inline size_t pcv_table_dev_walk_bytes(uint32_t M) { return pcv_align_up((size_t)M * 8, 256); }
// What pcv_build_begin reserves of pinned memory for a tree of M nodes over n points: the two areas and the largest record
// block any such tree can need.
size_t pcv_table_pinned_bytes(uint32_t M, uint64_t n, bool deep);

// ---- host arithmetic on the staged table --------------------------------------------------------------------------------
// Bottom-up stream lengths: |pre(leaf)| = hi - lo, |pre(inner)| = sum ceil(|pre(child)| / 8). Fills pre[M],
// parent and child_off.
void pcv_table_stream_lengths(const PcvStagedTable& tb, uint64_t* pre);
// Lengths of the level-1 / level-2 streams of this (local) tree, into an *out the caller has zeroed.
void pcv_table_top_streams(const PcvStagedTable& tb, const uint64_t* pre, pcv_top_streams* out);
// Multi-GPU build: the nodes of level <= 1 take their GLOBAL stream lengths and the level-1 / level-2 nodes their global
// offsets. Returns the number of nodes of level <= 1.
uint32_t pcv_table_apply_top_layout(const PcvStagedTable& tb, const pcv_top_layout& top, uint64_t* pre);
// Leaves in key order == order of their sorted ranges: depth-first, children in digit order. Fills leaf_lo / leaf_node and
// rank_of[M] (zeroed by the caller: entries of inner nodes stay 0); *wide: some leaf level is Float64-coded. Returns the
// number of leaves.
uint32_t pcv_table_leaf_order(const PcvStagedTable& tb, const PcvLevels& lv, uint32_t* rank_of, bool* wide);
// Per node: walk word, cube min, u128 id, point count, encoding and the 16-byte-aligned blob offsets — nodes[M] and the upload
// arrays. Returns the total through *num_points / *xyz_bytes.
void pcv_table_node_infos(const PcvStagedTable& tb, const PcvLevels& lv, const double root_min[3], const uint64_t* pre,
                          const uint32_t* rank_of, pcv_node_info* nodes, uint64_t* num_points, uint64_t* xyz_bytes);

// Sorted slots whose points replay the chain after the record sort (a true leaf without usable codes, pcv_spec.h).
struct PcvFixRange {
  uint32_t lo, count, level;
};
// The K6 work lists of one build: decided first (counts -> record block -> does it fit), written second.
struct PcvWorkLists {
  PcvRecordCounts counts;
  bool by_leaf = true;              // leaf-wise settle / climb kernels (pcv_switches().settle_by_leaf)
  std::vector<uint32_t> cnt;        // points per leaf rank
  std::vector<uint32_t> settle_cnt; // fused only: what `settle` is left with per leaf (0 for the leaves the sort settles)
  std::vector<uint8_t> climbs;      // the leaf's node is not the root
  std::vector<uint8_t> fused_leaf;  // fused only
  uint64_t settled_points = 0;      // points of the leaves the sort's second pass settles
  uint64_t num_climbers = 0;        // (known once the lists are written)
};
// fuse: the held-back second pass of the record sort settles every leaf it can — integer codes, not the root, no chain to
// continue, no replay; `settle` gets items for the others only.
void pcv_table_plan_work(const PcvStagedTable& tb, const PcvLevels& lv, uint32_t num_leaves, const uint32_t* rank_of, bool by_leaf,
                         bool fuse, const uint32_t* cont_nodes, uint32_t num_cont, const PcvFixRange* fix, size_t num_fix,
                         PcvWorkLists* w);
// Node and leaf records, climb_base, settle / climb items, continuation ranges and items (with the `pad` marks of the settle
// items whose leaf continues its chain) and the fused flags, into a block built from w->counts (the plan counted every list
// with the function that writes it here, so the lists end where the block says).
void pcv_table_fill_records(const PcvStagedTable& tb, const PcvLevels& lv, const uint32_t* rank_of, const uint32_t* cont_nodes,
                            const uint32_t* cont_from, const PcvRecordBlock& rb, PcvWorkLists* w);
