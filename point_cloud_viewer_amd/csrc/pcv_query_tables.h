// pcv_query_tables.h — the query view of a finished octree: what the node kernels and the point query read of the node
// table, where it lies in the tree's one device block, and the host walk over a relation row.
//
// pcv_octree_prepare_query (pcv_cull.hip) calls pcv_query_tables, allocates PcvQueryLayout(m).bytes and uploads section by
// section; query_points_impl (pcv_query.hip) walks one shape's relation row with pcv_query_walk. Host code that makes no HIP
// call and takes no pcv_ctx (compiled like pcv_tables.cpp): unit-tested on the CPU through pcv_query_tables_selftest
// (tests/test_query_tables_cpu.py) against the oracle and the Python statements of the two cube recurrences.
#pragma once
#include <algorithm>

#include "pcv_internal.h"

struct BatchNode {  // what the point query's chunk descriptors need of one node
  uint64_t xyz_off, point_off;
  double cube_min[3];
  double cube_edge;
  uint32_t n, enc;
};
inline BatchNode batch_node(const pcv_node_info& nd) {
  BatchNode o;
  o.xyz_off = nd.xyz_offset;
  o.point_off = nd.point_offset;
  for (int a = 0; a < 3; ++a) o.cube_min[a] = nd.cube_min[a];
  o.cube_edge = nd.cube_edge;
  o.n = (uint32_t)std::max<int64_t>(nd.num_points, 0);
  o.enc = nd.encoding;
  return o;
}

// Node order = (level, index): a node's children are contiguous on the next level, in digit order.
struct PcvQueryTables {
  uint32_t m = 0;
  std::vector<double> cubes;     // 4 per node: Node::get_child recurrence from Cube::bounding of the tree's box (node.rs:190-211);
                                 // zeros for a node whose parent is not in the table
  std::vector<double> fb_cubes;  // 4 per node: NodeId::find_bounding_cube, as the node table has it
  std::vector<uint32_t> first_child;
  std::vector<uint8_t> child_mask;
  std::vector<uint8_t> empty;    // num_points == 0
  std::vector<BatchNode> nodes;
};
PcvQueryTables pcv_query_tables(const pcv_node_info* nodes, uint32_t m, const double bbox_min[3], const double bbox_max[3]);

// The device block: sections in this order, each of m + 1 entries (the last one spare), byte offsets from the block's start.
struct PcvQueryLayout {
  size_t cubes, fb_cubes, nodes, first_child, child_mask, empty, bytes;
  explicit PcvQueryLayout(uint32_t m) {
    const size_t n = (size_t)m + 1;
    cubes = 0;
    fb_cubes = cubes + 32 * n;
    nodes = fb_cubes + 32 * n;
    first_child = nodes + sizeof(BatchNode) * n;
    child_mask = first_child + 4 * n;
    empty = child_mask + n;
    bytes = empty + n;
  }
};
// every section starts aligned for any m when the block does: the kernels read a cube as one double4
static_assert(32 % alignof(BatchNode) == 0 && sizeof(BatchNode) % alignof(uint32_t) == 0 && sizeof(BatchNode) == 56,
              "PcvQueryLayout: 32-byte cubes, then 8-byte node rows, then dwords, then bytes");

// NodeIdsIterator over one shape's relation row (octree_iterator.rs:30-43): breadth first from the root, a node's children are
// visited iff the node is not Out (2); the nodes that are not Out, in that order.
void pcv_query_walk(const uint8_t* relation, const uint32_t* first_child, const uint8_t* child_mask, uint32_t m,
                    std::vector<uint32_t>* out);
