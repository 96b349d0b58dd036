// pcv_s2_query_dev.h — the result of the batched point query over an S2 cell cloud (pcv_s2_points.hip) as its consumer on
// the device reads it (pcv_xray.hip), as pcv_query_dev.h states the octree batch: the candidates of every (location, listed
// cell) back to back in chunks of at most 1 024 points of one cell, one u32 keep flag per candidate, positions and attributes
// read from the cloud's own blobs (24-byte AoS f64, 3-byte colour, f32 intensity) at the chunk's point index.
#pragma once
#include <cstdint>
#include <vector>

struct pcv_s2_cloud;

struct PcvS2Chunk {
  uint64_t src;    // first point in the cloud's blobs
  uint64_t first;  // first candidate: its flag is flags[first]
  uint32_t count, location;
};
static_assert(sizeof(PcvS2Chunk) == 24, "the chunk list is read by the device as it is laid out here");
constexpr uint32_t kS2ChunkPoints = 1024;

struct pcv_s2_query {
  pcv_s2_cloud* cloud = nullptr;
  uint64_t nseg = 0, kept = 0, candidates = 0;
  std::vector<uint64_t> location_first;  // [locations + 1]
  std::vector<uint32_t> seg_cell;        // [nseg]
  std::vector<uint64_t> seg_offset;      // [nseg + 1] kept points before the segment
  std::vector<uint64_t> seg_first_chunk; // [nseg + 1]
  PcvS2Chunk* d_chunks = nullptr;        // in candidate order
  uint32_t* d_flags = nullptr;           // one per candidate
  uint64_t* d_offsets = nullptr;         // [candidates + 1]
};
