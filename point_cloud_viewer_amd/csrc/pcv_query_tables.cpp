// pcv_query_tables.cpp — the host arithmetic of pcv_query_tables.h. No HIP call, no pcv_ctx: unit-tested on the CPU through
// pcv_query_tables_selftest (tests/test_query_tables_cpu.py).
#include "pcv_query_tables.h"

#include <cmath>
#include <cstring>

PcvQueryTables pcv_query_tables(const pcv_node_info* nodes, uint32_t m, const double bbox_min[3], const double bbox_max[3]) {
  PcvQueryTables t;
  t.m = m;
  t.cubes.assign(4 * (size_t)m, 0.0);
  t.fb_cubes.assign(4 * (size_t)m, 0.0);
  t.first_child.assign(m, 0);
  t.child_mask.assign(m, 0);
  t.empty.assign(m, 0);
  t.nodes.resize(m);
  typedef unsigned __int128 u128;
  auto idx_of = [](const pcv_node_info& n) { return ((u128)(n.id_high & 0x00ffffffffffffffull) << 64) | n.id_low; };
  std::vector<uint32_t> level_start(258, m);  // first node of each level; an absent level starts where the next one does
  for (uint32_t i = m; i-- > 0;) level_start[nodes[i].level] = i;
  for (int l = 255; l >= 0; --l)
    if (level_start[l] == m) level_start[l] = level_start[l + 1];
  // root cube: Cube::bounding (aabb.rs:149-157)
  const double root_edge = std::fmax(std::fmax(bbox_max[0] - bbox_min[0], bbox_max[1] - bbox_min[1]), bbox_max[2] - bbox_min[2]);
  std::vector<uint8_t> has_parent(m, 0);  // the node's get_child cube is known
  for (uint32_t i = 0; i < m; ++i) {
    const pcv_node_info& n = nodes[i];
    t.empty[i] = n.num_points == 0;
    t.nodes[i] = batch_node(n);
    for (int a = 0; a < 3; ++a) t.fb_cubes[4 * (size_t)i + a] = n.cube_min[a];
    t.fb_cubes[4 * (size_t)i + 3] = n.cube_edge;
    if (n.level == 0) {  // (the root is node 0)
      for (int a = 0; a < 3; ++a) t.cubes[a] = bbox_min[a];
      t.cubes[3] = root_edge;
      has_parent[i] = 1;
    }
    // children: binary search the next level for index * 8 .. index * 8 + 7
    const uint32_t lo = level_start[n.level + 1], hi = level_start[n.level + 2];
    const u128 want = idx_of(n) << 3;
    uint32_t a = lo, b = hi;
    while (a < b) {
      const uint32_t mid = a + (b - a) / 2;
      if (idx_of(nodes[mid]) < want) a = mid + 1;
      else b = mid;
    }
    t.first_child[i] = a;
    for (uint32_t c = a; c < hi && (idx_of(nodes[c]) >> 3) == idx_of(n) && nodes[c].level == n.level + 1; ++c) {
      const unsigned digit = (unsigned)(idx_of(nodes[c]) & 7);
      t.child_mask[i] |= (uint8_t)(1u << digit);
      if (!has_parent[i]) continue;
      // Node::get_child (node.rs:190-211): min += half only where the bit is set
      const double* pc = &t.cubes[4 * (size_t)i];
      double* cc = &t.cubes[4 * (size_t)c];
      const double half = pc[3] / 2.;
      cc[0] = pc[0];
      cc[1] = pc[1];
      cc[2] = pc[2];
      if (digit & 1) cc[2] += half;
      if (digit & 2) cc[1] += half;
      if (digit & 4) cc[0] += half;
      cc[3] = half;
      has_parent[c] = 1;
    }
  }
  return t;
}

void pcv_query_walk(const uint8_t* relation, const uint32_t* first_child, const uint8_t* child_mask, uint32_t m,
                    std::vector<uint32_t>* out) {
  out->clear();
  if (m == 0) return;
  out->reserve(m);
  std::vector<uint32_t> queue;
  queue.reserve(m);
  queue.push_back(0);
  for (size_t head = 0; head < queue.size(); ++head) {
    const uint32_t cur = queue[head];
    if (relation[cur] == 2) continue;
    uint32_t c = first_child[cur];
    for (int ci = 0; ci < 8; ++ci)
      if ((child_mask[cur] >> ci) & 1) queue.push_back(c++);
    out->push_back(cur);
  }
}

// ---- CPU self-test hook (tests/test_query_tables_cpu.py) ----------------------------------------------------------------
// The tables of a node table of m rows (m entries each, 4 m doubles per cube table, m rows of 56 bytes), `layout` = the byte
// offsets of cubes, fb_cubes, nodes, first_child, child_mask, empty in the device block and its size, and — relation set —
// the walk of that relation row over these tables into walk[m], its length in *walk_count.
extern "C" int pcv_query_tables_selftest(const pcv_node_info* nodes, uint32_t m, const double* bbox_min, const double* bbox_max,
                                         double* cubes, double* fb_cubes, uint32_t* first_child, uint8_t* child_mask, uint8_t* empty,
                                         void* batch_nodes, uint64_t* layout /* [7] */, const uint8_t* relation, uint32_t* walk,
                                         uint32_t* walk_count) {
  const PcvQueryTables t = pcv_query_tables(nodes, m, bbox_min, bbox_max);
  if (m) {
    std::memcpy(cubes, t.cubes.data(), 32 * (size_t)m);
    std::memcpy(fb_cubes, t.fb_cubes.data(), 32 * (size_t)m);
    std::memcpy(first_child, t.first_child.data(), 4 * (size_t)m);
    std::memcpy(child_mask, t.child_mask.data(), m);
    std::memcpy(empty, t.empty.data(), m);
    std::memcpy(batch_nodes, t.nodes.data(), sizeof(BatchNode) * (size_t)m);
  }
  const PcvQueryLayout l(m);
  const size_t at[7] = {l.cubes, l.fb_cubes, l.nodes, l.first_child, l.child_mask, l.empty, l.bytes};
  for (int k = 0; k < 7; ++k) layout[k] = at[k];
  if (relation) {
    std::vector<uint32_t> w;
    pcv_query_walk(relation, t.first_child.data(), t.child_mask.data(), m, &w);
    if (!w.empty()) std::memcpy(walk, w.data(), 4 * w.size());
    *walk_count = (uint32_t)w.size();
  }
  return 0;
}
