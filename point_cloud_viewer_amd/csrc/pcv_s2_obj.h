// pcv_s2_obj.h — an S2 cell cloud as pcv_s2.hip builds it and pcv_s2_query.hip reads it.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

struct pcv_ctx;

struct pcv_s2_cloud {
  pcv_ctx* ctx = nullptr;
  uint64_t n = 0;
  uint32_t level = 0;
  bool has_intensity = false;
  double bbox_min[3] = {0, 0, 0}, bbox_max[3] = {0, 0, 0};
  std::vector<uint64_t> ids, counts, offsets;  // per cell, ascending by id; offsets in points
  uint32_t* d_order = nullptr;                 // slot -> input index
  uint8_t *d_xyz = nullptr, *d_rgb = nullptr, *d_int = nullptr;
  // the query side (pcv_s2_query.hip), built on first use: the ids on the device and the cell table, s2::kCellPlanes planes of
  // one double per cell (rect bound, centre, (u, v) bounds, vertices, their lat / lng); null while the cloud has not been asked
  uint64_t* d_ids = nullptr;
  double* d_table = nullptr;
  // a cloud opened from a directory (pcv_s2_open_dir): its cell files are read and uploaded on first use; it has no d_order
  // With a null context (pcv_s2_open_dir(NULL, ...)) the cloud is host only: the files stay in h_xyz / h_rgb / h_int.
  std::string directory;
  bool opened = false, resident = true;
  std::vector<uint8_t> h_xyz, h_rgb, h_int;
  int fail(int code, const std::string& msg) const;  // through the context, or pcv_host_fail without one
};

// pcv_io.cpp — meta.pb of an S2 directory (S2Meta::from_proto: cells in any order come out ascending by id) and the cell
// files into cell-contiguous host blobs; *error carries the reference's message or names the file
struct PcvS2Dir {
  double bbox_min[3], bbox_max[3];
  std::vector<uint64_t> ids, counts;
  bool has_intensity;
};
int pcv_s2_read_meta(const char* directory, PcvS2Dir* out, std::string* error);
int pcv_s2_read_cells(const char* directory, const PcvS2Dir& meta, uint8_t* xyz, uint8_t* rgb, uint8_t* intensity, std::string* error);

// a union's cells as the entry points take them: ascending by id, no 0 (pcv_s2.hip); *why says what is wrong
int pcv_s2_check_union(const uint64_t* cells, uint32_t num_cells, std::string* why);
// several unions as pcv_s2_cells_in_location takes them (pcv_s2_query.hip): union_first[0] == 0, no descent, each union as above,
// every cell an S2 cell id
int pcv_s2_check_unions(uint32_t num_unions, const uint32_t* union_first, const uint64_t* union_cells, std::string* why);
// the blobs of an opened cloud on the device (pcv_s2.hip: read and uploaded on first use); nothing to do for a split
int pcv_s2_make_resident(pcv_s2_cloud* c);
// pcv_s2_split's checks and split for one batch of a stream (pcv_s2_stream.hip); with_order false: no d_order is made.
// pcv_s2_release frees a cloud whose device work the caller has waited for.
int pcv_s2_split_part(pcv_ctx* ctx, const pcv_points* points, uint32_t level, bool with_order, pcv_s2_cloud** out);
void pcv_s2_release(pcv_s2_cloud* c);
