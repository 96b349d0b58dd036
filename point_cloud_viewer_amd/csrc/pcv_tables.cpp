// pcv_tables.cpp — layouts of the staged node table and the record block, and the host arithmetic on them (see
// pcv_tables.h). Host code that makes no HIP call (its types come from pcv_internal.h): unit-tested on the CPU through
// pcv_tables_selftest (tests/test_tables_cpu.py).
#include "pcv_tables.h"

#include <algorithm>
#include <cstring>

// ---- layouts --------------------------------------------------------------------------------------------------------------
// download area: prefix (8) lo hi first_child (4 each) level child_mask open (1 each) = 23 bytes per node; the area keeps the
// 27 M + 64 bytes it has always had (a fourth u32 column that is no longer downloaded), so every later offset stays put
static size_t prefix_lo_offset(uint32_t M) { return pcv_align_up((size_t)M * (8 + 4 * 4 + 3) + 64, 8); }
// upload area: walk xyz_off point_off (8 each) node_min (24) parent child_off leaf_lo leaf_node (4 each) level (1)
static size_t upload_bytes(uint32_t M) { return (size_t)M * (8 * 3 + 24 + 4 * 4 + 1); }
static size_t upload_offset(uint32_t M, bool deep) { return pcv_align_up(prefix_lo_offset(M) + (deep ? (size_t)M * 8 : 0), 256); }

size_t pcv_staged_table_bytes(uint32_t M, bool deep) { return upload_offset(M, deep) + pcv_align_up(upload_bytes(M), 256); }

PcvStagedTable pcv_staged_table(void* base, uint32_t M, bool deep) {
  uint8_t* hp = (uint8_t*)base;
  PcvStagedTable t;
  t.M = M;
  t.prefix = (uint64_t*)hp;
  t.lo = (uint32_t*)(t.prefix + M);
  t.hi = t.lo + M;
  t.first_child = t.hi + M;
  t.level = (uint8_t*)(t.first_child + M);
  t.child_mask = t.level + M;
  t.open = t.child_mask + M;
  t.prefix_lo = deep ? (uint64_t*)(hp + prefix_lo_offset(M)) : nullptr;
  t.walk = (uint64_t*)(hp + upload_offset(M, deep));
  t.xyz_off = t.walk + M;
  t.point_off = t.xyz_off + M;
  t.node_min = (double*)(t.point_off + M);
  t.parent = (uint32_t*)(t.node_min + 3 * (size_t)M);
  t.child_off = t.parent + M;
  t.leaf_lo = t.child_off + M;
  t.leaf_node = t.leaf_lo + M;
  t.node_level = (uint8_t*)(t.leaf_node + M);
  t.records = hp + pcv_staged_table_bytes(M, deep);
  return t;
}

PcvRecordBlock pcv_record_block(void* base, const PcvRecordCounts& c) {
  static_assert(sizeof(PcvNodeRec) % 16 == 0 && sizeof(PcvSettleItem) == 16, "record sections stay 16-byte aligned");
  // byte offsets first (base may be null when only the size is asked for), pointers from them
  const size_t leaf_rec = (size_t)c.M * sizeof(PcvNodeRec);
  const size_t climb_base = leaf_rec + (size_t)c.num_leaves * sizeof(PcvNodeRec);
  const size_t items = pcv_align_up(climb_base + (size_t)c.num_leaves * 4, 16);
  const size_t citems = items + (size_t)c.num_items * sizeof(PcvSettleItem);
  const size_t cont_ranges = citems + (size_t)c.num_citems * sizeof(PcvSettleItem);
  const size_t cont_items = cont_ranges + pcv_align_up((size_t)c.num_cont * pcv_cont_range_bytes(), 16);
  const size_t fused = cont_items + (size_t)c.num_cont_items * sizeof(PcvSettleItem);
  PcvRecordBlock b;
  b.bytes = fused + (c.fused ? pcv_align_up(c.num_leaves, 16) : 0);
  if (!base) return b;
  uint8_t* p = (uint8_t*)base;
  b.node_rec = (PcvNodeRec*)p;
  b.leaf_rec = (PcvNodeRec*)(p + leaf_rec);
  b.climb_base = (uint32_t*)(p + climb_base);
  b.items = (PcvSettleItem*)(p + items);
  b.citems = (PcvSettleItem*)(p + citems);
  b.cont_ranges = p + cont_ranges;
  b.cont_items = (PcvSettleItem*)(p + cont_items);
  b.fused = p + fused;
  return b;
}

size_t pcv_table_pinned_bytes(uint32_t M, uint64_t n, bool deep) {
  PcvRecordCounts most;
  most.M = M;
  most.num_leaves = M;  // every node a leaf: the leaf records, climb_base and the fused flags cannot be longer
  // a leaf of c slots gets ceil(c / tile) settle items, and the leaves' slots add up to n (pcv_spec.h, pcv_settle_items)
  most.num_items = (uint32_t)(n / kPcvSettleTile) + M;
  // a climbing leaf of c slots has ceil(c / 8) climbers — at most n / 8 + M in all — and one item per kPcvClimbTile of them
  most.num_citems = (uint32_t)((n / 8 + M) / kPcvClimbTile) + M;
  most.num_cont = M;  // continued leaves are leaves
  // the continued leaves' slots are a part of the n: the bound of the settle items holds for their items too
  most.num_cont_items = (uint32_t)(n / kPcvSettleTile) + M;
  most.fused = true;
  return pcv_staged_table_bytes(M, deep) + pcv_record_block(nullptr, most).bytes;
}

// ---- stream lengths -------------------------------------------------------------------------------------------------------
void pcv_table_stream_lengths(const PcvStagedTable& tb, uint64_t* pre) {
  for (uint32_t i = tb.M; i-- > 0;) {
    if (!tb.open[i]) {
      pre[i] = (uint64_t)tb.hi[i] - tb.lo[i];
    } else {
      uint64_t acc = 0;
      uint32_t c = tb.first_child[i];
      for (int dgt = 0; dgt < 8; ++dgt)
        if ((tb.child_mask[i] >> dgt) & 1) {
          tb.child_off[c] = (uint32_t)acc;
          tb.parent[c] = i;
          acc += pcv_ceil8(pre[c]);
          ++c;
        }
      pre[i] = acc;
    }
  }
  tb.parent[0] = 0xffffffffu;
  tb.child_off[0] = 0;
}

void pcv_table_top_streams(const PcvStagedTable& tb, const uint64_t* pre, pcv_top_streams* out) {
  uint32_t c1 = tb.first_child[0];
  for (int c = 0; c < 8; ++c) {
    if (!((tb.child_mask[0] >> c) & 1)) continue;
    const uint32_t i = c1++;
    out->l1[c] = pre[i];
    if (!tb.open[i]) continue;
    out->l1_split_mask |= 1u << c;
    uint32_t c2 = tb.first_child[i];
    for (int dg = 0; dg < 8; ++dg)
      if ((tb.child_mask[i] >> dg) & 1) out->l2[c * 8 + dg] = pre[c2++];
  }
}

uint32_t pcv_table_apply_top_layout(const PcvStagedTable& tb, const pcv_top_layout& top, uint64_t* pre) {
  pre[0] = top.root_points;
  uint32_t c1 = tb.first_child[0];
  uint32_t top_nodes = 1;
  for (int c = 0; c < 8; ++c) {
    if (!((tb.child_mask[0] >> c) & 1)) continue;
    const uint32_t i = c1++;
    ++top_nodes;
    pre[i] = top.l1_stream[c];
    tb.child_off[i] = top.l1_offset[c];
    if (!tb.open[i]) continue;
    uint32_t c2 = tb.first_child[i];
    for (int dg = 0; dg < 8; ++dg)
      if ((tb.child_mask[i] >> dg) & 1) tb.child_off[c2++] = top.l2_offset[c * 8 + dg];
  }
  return top_nodes;
}

// ---- leaves and nodes -----------------------------------------------------------------------------------------------------
uint32_t pcv_table_leaf_order(const PcvStagedTable& tb, const PcvLevels& lv, uint32_t* rank_of, bool* wide) {
  uint32_t stack[7 * PCV_MAX_LEVELS + 8];  // a popped node of level k leaves at most 7 siblings per level above it
  uint32_t sp = 0, r = 0;
  stack[sp++] = 0;
  *wide = false;
  while (sp) {
    const uint32_t i = stack[--sp];
    if (tb.open[i]) {
      const uint32_t nchild = (uint32_t)__builtin_popcount(tb.child_mask[i]);
      for (uint32_t c = nchild; c-- > 0;) stack[sp++] = tb.first_child[i] + c;  // reversed: digit 0 is popped first
      continue;
    }
    rank_of[i] = r;
    tb.leaf_lo[r] = tb.lo[i];
    tb.leaf_node[r] = i;
    if (lv.enc[tb.level[i]] == PCV_ENC_FLOAT64) *wide = true;
    ++r;
  }
  return r;
}

void pcv_table_node_infos(const PcvStagedTable& tb, const PcvLevels& lv, const double root_min[3], const uint64_t* pre,
                          const uint32_t* rank_of, pcv_node_info* nodes, uint64_t* num_points, uint64_t* xyz_bytes) {
  uint64_t xyz_off = 0, point_off = 0;
  for (uint32_t i = 0; i < tb.M; ++i) {
    const int level = tb.level[i];
    tb.node_level[i] = (uint8_t)level;
    tb.walk[i] = tb.open[i] ? ((uint64_t)tb.first_child[i] | ((uint64_t)tb.child_mask[i] << 32) | ((uint64_t)level << 48))
                            : ((uint64_t)rank_of[i] | (1ull << 40) | ((uint64_t)level << 48));
    double* mn = tb.node_min + 3 * (size_t)i;
    // NodeId::find_bounding_cube recurrence (node.rs:157-172): parents precede children in the table
    if (i == 0) {
      for (int a = 0; a < 3; ++a) mn[a] = root_min[a];
    } else {
      const double* pm = tb.node_min + 3 * (size_t)tb.parent[i];
      const unsigned dgt = level <= PCV_MAX_KEY_LEVELS
                               ? (unsigned)(tb.prefix[i] >> (3 * (PCV_MAX_KEY_LEVELS - level))) & 7u
                               : (unsigned)(tb.prefix_lo[i] >> (3 * (2 * PCV_MAX_KEY_LEVELS - level))) & 7u;
      const double e = lv.edge[level];
      mn[0] = pm[0] + (double)((dgt >> 2) & 1) * e;
      mn[1] = pm[1] + (double)((dgt >> 1) & 1) * e;
      mn[2] = pm[2] + (double)(dgt & 1) * e;
    }
    const uint64_t np = i == 0 ? pre[0] : pre[i] - pcv_ceil8(pre[i]);
    pcv_node_info& ni = nodes[i];
    // u128 NodeId = level << 120 | index (node.rs:108-111); the index is the octal path, 3 bits per level
    unsigned __int128 index = 0;
    if (level > PCV_MAX_KEY_LEVELS)
      index = ((unsigned __int128)tb.prefix[i] << (3 * (level - PCV_MAX_KEY_LEVELS))) |
              (tb.prefix_lo[i] >> (3 * (2 * PCV_MAX_KEY_LEVELS - level)));
    else if (level)
      index = tb.prefix[i] >> (3 * (PCV_MAX_KEY_LEVELS - level));
    ni.id_high = ((uint64_t)level << 56) | (uint64_t)(index >> 64);
    ni.id_low = (uint64_t)index;
    ni.num_points = (int64_t)np;
    ni.level = (uint32_t)level;
    ni.encoding = lv.enc[level];
    for (int a = 0; a < 3; ++a) ni.cube_min[a] = mn[a];
    ni.cube_edge = lv.edge[level];
    ni.xyz_offset = xyz_off;
    ni.point_offset = point_off;
    tb.xyz_off[i] = xyz_off;
    tb.point_off[i] = point_off;
    xyz_off += (np * 3 * (uint64_t)pcv_bytes_per_coordinate(ni.encoding) + 15) & ~15ull;
    point_off += np;
  }
  *num_points = point_off;
  *xyz_bytes = xyz_off;
}

// ---- K6 work lists --------------------------------------------------------------------------------------------------------
// One item per <= kPcvSettleTile sorted slots of every leaf whose chain is continued; rank = index of the leaf's range.
// out == null: counts only (as pcv_settle_items / pcv_climb_layout: the plan and the fill share one rule per list).
static uint32_t cont_items(const PcvStagedTable& tb, const uint32_t* cont_nodes, uint32_t num_cont, PcvSettleItem* out) {
  uint32_t n = 0;
  for (uint32_t k = 0; k < num_cont; ++k) {
    const uint64_t e = tb.hi[cont_nodes[k]];
    for (uint64_t b = tb.lo[cont_nodes[k]]; b < e; b += kPcvSettleTile, ++n)
      if (out) out[n] = PcvSettleItem{k, (uint32_t)b, (uint32_t)std::min<uint64_t>(b + kPcvSettleTile, e), 0u};
  }
  return n;
}

void pcv_table_plan_work(const PcvStagedTable& tb, const PcvLevels& lv, uint32_t num_leaves, const uint32_t* rank_of, bool by_leaf,
                         bool fuse, const uint32_t* cont_nodes, uint32_t num_cont, const PcvFixRange* fix, size_t num_fix,
                         PcvWorkLists* w) {
  w->by_leaf = by_leaf;
  w->cnt.resize(num_leaves);
  w->climbs.resize(num_leaves);
  for (uint32_t r = 0; r < num_leaves; ++r) {
    const uint32_t i = tb.leaf_node[r];
    w->cnt[r] = tb.hi[i] - tb.lo[i];
    w->climbs[r] = tb.parent[i] != 0xffffffffu;
  }
  w->settled_points = 0;
  if (fuse) {
    w->fused_leaf.assign(num_leaves, 0);
    std::vector<uint8_t> cont_leaf(num_leaves, 0);
    for (uint32_t k = 0; k < num_cont; ++k) cont_leaf[rank_of[cont_nodes[k]]] = 1;
    for (size_t f = 0; f < num_fix; ++f) {  // replayed leaves: their records get their codes after the sort
      uint32_t r = (uint32_t)(std::lower_bound(tb.leaf_lo, tb.leaf_lo + num_leaves, fix[f].lo) - tb.leaf_lo);
      for (; r < num_leaves && tb.leaf_lo[r] == fix[f].lo; ++r) cont_leaf[r] = 1;  // (empty leaves share their neighbour's first slot)
    }
    w->settle_cnt = w->cnt;
    for (uint32_t r = 0; r < num_leaves; ++r)
      if (w->climbs[r] && !cont_leaf[r] && lv.enc[tb.level[tb.leaf_node[r]]] <= PCV_ENC_UINT16) {
        w->fused_leaf[r] = 1;
        w->settle_cnt[r] = 0;
        w->settled_points += w->cnt[r];
      }
  }
  PcvRecordCounts& c = w->counts;
  c = PcvRecordCounts();
  c.M = tb.M;
  c.num_leaves = num_leaves;
  c.fused = fuse;
  if (by_leaf) c.num_items = pcv_settle_items(tb.leaf_lo, (fuse ? w->settle_cnt : w->cnt).data(), num_leaves, nullptr);
  pcv_climb_layout(w->cnt.data(), w->climbs.data(), num_leaves, nullptr, nullptr, &c.num_citems);
  c.num_cont = num_cont;
  c.num_cont_items = cont_items(tb, cont_nodes, num_cont, nullptr);
}

void pcv_table_fill_records(const PcvStagedTable& tb, const PcvLevels& lv, const uint32_t* rank_of, const uint32_t* cont_nodes,
                            const uint32_t* cont_from, const PcvRecordBlock& rb, PcvWorkLists* w) {
  const PcvRecordCounts& c = w->counts;
  for (uint32_t i = 0; i < tb.M; ++i) {
    PcvNodeRec& nr = rb.node_rec[i];
    const int level = tb.node_level[i];
    nr.lo = tb.lo[i];
    nr.parent = tb.parent[i];
    nr.child_off = tb.child_off[i];
    nr.enc = lv.enc[level];
    nr.edge = lv.edge[level];
    // 0 = "no unchecked exact division here": also when the root cube's min is not tame (PcvLevels::fast_ok)
    nr.inv_edge = lv.fast_ok ? lv.inv_edge[level] : 0.0;
    nr.inv_edge_lo = lv.fast_ok ? lv.inv_edge_lo[level] : 0.0;
    nr.xyz_off = tb.xyz_off[i];
    nr.point_off = tb.point_off[i];
    for (int a = 0; a < 3; ++a) nr.mn[a] = tb.node_min[3 * (size_t)i + a];
  }
  for (uint32_t r = 0; r < c.num_leaves; ++r) rb.leaf_rec[r] = rb.node_rec[tb.leaf_node[r]];
  // climbers of K6 (every 8th point of every leaf; the root is never a leaf that climbs): dense index = climb_base[leaf] + j / 8,
  // and the work lists of the leaf-wise settle / climb kernels (pcv_spec.h)
  if (w->by_leaf) pcv_settle_items(tb.leaf_lo, (c.fused ? w->settle_cnt : w->cnt).data(), c.num_leaves, rb.items);
  uint32_t num_citems = 0;
  w->num_climbers = pcv_climb_layout(w->cnt.data(), w->climbs.data(), c.num_leaves, rb.climb_base, rb.citems, &num_citems);
  // single-chain build: leaves below a split first candidate continue their chain from the candidate's codes
  // (spec_continue_kernel): one range per leaf (levels + the candidate's cube min) and one item per <= kPcvSettleTile of its slots
  std::vector<uint32_t> cont_of_rank;
  if (c.num_cont && w->by_leaf) cont_of_rank.assign(c.num_leaves, 0u);
  cont_items(tb, cont_nodes, c.num_cont, rb.cont_items);
  for (uint32_t k = 0; k < c.num_cont; ++k) {
    const uint32_t leaf = cont_nodes[k], from = cont_from[k];
    pcv_fill_cont_range(rb.cont_ranges + (size_t)k * pcv_cont_range_bytes(), tb.level[from], tb.level[leaf],
                        tb.node_min + 3 * (size_t)from);
    if (w->by_leaf) cont_of_rank[rank_of[leaf]] = k + 1;
  }
  if (c.num_cont && w->by_leaf)  // the leaf-wise settle kernel continues these leaves' chains itself (it ignores the mark when it
                                 // is launched without the ranges)
    for (uint32_t j = 0; j < c.num_items; ++j) rb.items[j].pad = cont_of_rank[rb.items[j].rank];
  if (c.fused) std::memcpy(rb.fused, w->fused_leaf.data(), c.num_leaves);
}

// ---- CPU self-test hook (tests/test_tables_cpu.py) ----------------------------------------------------------------------
// Runs the table arithmetic of a build on a given node table, in a block of pcv_table_pinned_bytes(M, n, deep) bytes as
// pcv_build_begin reserves it. edge / enc: the level table, entries 0 .. nlevels. top (nullable): a pcv_top_layout to apply.
// cont_nodes / cont_from (num_cont entries) and fuse: the single-chain build's inputs to the work lists. Out: the node infos,
// the local top streams, and `sections` = byte offsets from the block's start of
//   [0..7]   prefix lo hi first_child level child_mask open prefix_lo(0 = none)
//   [8..16]  walk xyz_off point_off node_min parent child_off leaf_lo leaf_node level
//   [17..25] node_rec leaf_rec climb_base items citems cont_ranges cont_items fused, end of the record block
//   [26]     the reservation
// and counts = num_leaves, num_items, num_citems, num_cont_items, num_climbers, settled_points. Returns 1 when the record
// block would not fit the reservation (nothing is written then).
extern "C" int pcv_tables_selftest(uint32_t M, const uint64_t* prefix, const uint64_t* prefix_lo, const uint32_t* lo,
                                   const uint32_t* hi,
                                   const uint32_t* first_child, const uint8_t* level, const uint8_t* child_mask, const uint8_t* open,
                                   int deep, const double* edge, const uint32_t* enc, int nlevels, const double* root_min, uint64_t n,
                                   const pcv_top_layout* top, const uint32_t* cont_nodes, const uint32_t* cont_from, uint32_t num_cont,
                                   int fuse, pcv_node_info* nodes, pcv_top_streams* streams, uint64_t* sections /* [27] */,
                                   uint64_t* counts /* [6] */) {
  PcvLevels lv;
  std::memset(&lv, 0, sizeof(lv));
  for (int k = 0; k <= nlevels; ++k) {
    lv.edge[k] = edge[k];
    lv.enc[k] = enc[k];
  }
  lv.nlevels = nlevels;
  const size_t reserved = pcv_table_pinned_bytes(M, n, deep != 0);
  std::vector<uint64_t> block(reserved / 8 + 1);
  uint8_t* base = (uint8_t*)block.data();
  const PcvStagedTable tb = pcv_staged_table(base, M, deep != 0);
  std::memcpy(tb.prefix, prefix, (size_t)M * 8);
  std::memcpy(tb.lo, lo, (size_t)M * 4);
  std::memcpy(tb.hi, hi, (size_t)M * 4);
  std::memcpy(tb.first_child, first_child, (size_t)M * 4);
  std::memcpy(tb.level, level, M);
  std::memcpy(tb.child_mask, child_mask, M);
  std::memcpy(tb.open, open, M);
  if (deep) std::memcpy(tb.prefix_lo, prefix_lo, (size_t)M * 8);
  std::vector<uint64_t> pre(M);
  pcv_table_stream_lengths(tb, pre.data());
  pcv_table_top_streams(tb, pre.data(), streams);
  if (top) pcv_table_apply_top_layout(tb, *top, pre.data());
  std::vector<uint32_t> rank_of(M);
  bool wide = false;
  const uint32_t num_leaves = pcv_table_leaf_order(tb, lv, rank_of.data(), &wide);
  uint64_t num_points = 0, xyz_bytes = 0;
  pcv_table_node_infos(tb, lv, root_min, pre.data(), rank_of.data(), nodes, &num_points, &xyz_bytes);
  PcvWorkLists w;
  pcv_table_plan_work(tb, lv, num_leaves, rank_of.data(), true, fuse != 0, cont_nodes, num_cont, nullptr, 0, &w);
  const PcvRecordBlock rb = pcv_record_block(tb.records, w.counts);
  const void* at[26] = {tb.prefix,      tb.lo,       tb.hi,         tb.first_child, tb.level,     tb.child_mask, tb.open,
                        tb.prefix_lo,   tb.walk,     tb.xyz_off,    tb.point_off,   tb.node_min,  tb.parent,     tb.child_off,
                        tb.leaf_lo,     tb.leaf_node, tb.node_level, rb.node_rec,   rb.leaf_rec,  rb.climb_base, rb.items,
                        rb.citems,      rb.cont_ranges, rb.cont_items, rb.fused,    (const uint8_t*)rb.node_rec + rb.bytes};
  for (int k = 0; k < 26; ++k) sections[k] = at[k] ? (uint64_t)((const uint8_t*)at[k] - base) : 0;
  sections[26] = reserved;
  counts[0] = num_leaves;
  counts[1] = w.counts.num_items;
  counts[2] = w.counts.num_citems;
  counts[3] = w.counts.num_cont_items;
  counts[4] = 0;
  counts[5] = w.settled_points;
  if (sections[25] > reserved) return 1;
  pcv_table_fill_records(tb, lv, rank_of.data(), cont_nodes, cont_from, rb, &w);
  counts[4] = w.num_climbers;
  return 0;
}
