// pcv_s2_merge_plan.h — what the merge of a stream's parts will do, worked out before anything is launched. A part
// is what pcv_s2_split makes of one batch: cells ascending by id, the points of a cell in input order. The cloud of all batches
// is the parts' merge by cell, the parts in batch order inside a cell (S2Splitter::write appends to a cell's files call after
// call, src/read_write/s2.rs:121-136). Standard C++: no HIP header and no global is read, so that the plan can be built and
// checked on a machine without a GPU (tests/test_s2_merge_plan_cpu.py). pcv_s2_stream.hip launches what the plan says.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/pcv_hip.h"

// points of the output that one workgroup of s2_merge_kernel writes: 256 lanes x 8 points
constexpr uint32_t kMergeChunkPoints = 2048;

struct PcvS2MergePart {
  const uint64_t* ids;     // ascending, no 0
  const uint64_t* counts;  // > 0 each
  uint64_t num_cells;
};

struct PcvS2MergePlan {
  uint64_t n = 0;                              // points of the merge
  std::vector<uint64_t> ids, counts, offsets;  // the merged cells, ascending by id; offsets in points
  // one segment per (cell, part that holds the cell), ordered by cell, then by part: `count` points from `src_offset` of the
  // part's blobs to `dst_offset` of the merged ones. The segments tile [0, n) in this order.
  std::vector<pcv_s2_merge_segment> segments;
  // per output chunk c of chunk_points points: the segment that holds point c * chunk_points
  std::vector<uint64_t> chunk_first_segment;
};

// PCV_E_INVALID with *why for a part whose ids do not ascend strictly, an id of 0, a cell of no points, a part of 2^32 - 1 points
// or more, chunk_points == 0. Deterministic: the same parts give the same plan.
int pcv_s2_merge_plan(const PcvS2MergePart* parts, uint32_t num_parts, uint32_t chunk_points, PcvS2MergePlan* plan, std::string* why);
