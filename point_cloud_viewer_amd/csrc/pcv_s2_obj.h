// pcv_s2_obj.h — an S2 cell cloud as pcv_s2.hip builds it and pcv_s2_query.hip reads it.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

struct pcv_ctx;
struct pcv_points;
struct pcv_attribute;

// one extra attribute of a cloud (pcv_s2_attr.hip): a cell-contiguous column of n elements of `elem` bytes
struct PcvS2Extra {
  std::string name;
  int32_t data_type = 0;
  uint32_t elem = 0;          // bytes per point
  uint8_t* d = nullptr;       // device column (null while an opened cloud's files have not been asked for, or n == 0)
  std::vector<uint8_t> h;     // host-only clouds: the column as read
  bool resident = true;       // false: an opened cloud's extra whose files have not been read yet
  const void* src = nullptr;  // the caller's column while a split runs
};

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
  std::vector<PcvS2Extra> extras;  // ascending by name
  int find_extra(const char* name) const {
    for (size_t k = 0; name && k < extras.size(); ++k)
      if (extras[k].name == name) return (int)k;
    return -1;
  }
  int fail(int code, const std::string& msg) const;  // through the context, or pcv_host_fail without one
};

// pcv_io.cpp — meta.pb of an S2 directory (S2Meta::from_proto: cells in any order come out ascending by id) and the cell
// files into cell-contiguous host blobs; *error carries the reference's message or names the file
struct PcvS2Dir {
  double bbox_min[3], bbox_max[3];
  std::vector<uint64_t> ids, counts;
  bool has_intensity;
  std::vector<std::pair<std::string, int32_t>> extras;  // the entries that pcv_s2_attr_name_ok and pcv_s2_attr_size accept, ascending
};
int pcv_s2_read_meta(const char* directory, PcvS2Dir* out, std::string* error);
int pcv_s2_read_cells(const char* directory, const PcvS2Dir& meta, uint8_t* xyz, uint8_t* rgb, uint8_t* intensity, std::string* error);

// one extra's files into a cell-contiguous host column of `elem` bytes per point (pcv_io.cpp)
int pcv_s2_read_extra(const char* directory, const std::vector<uint64_t>& ids, const std::vector<uint64_t>& counts, const std::string& name,
                      uint32_t elem, uint8_t* out, std::string* error, bool* absent = nullptr /* set: the directory holds no file of it */);
// the runs of one extra onto `<token>.<name>` (pcv_io.cpp), as pcv_s2_write_cells writes the built-in columns
int pcv_s2_write_extra(const char* directory, uint64_t num_cells, const uint64_t* ids, const uint64_t* counts, const uint64_t* offsets,
                       const uint8_t* truncate, const std::string& name, uint32_t elem, const uint8_t* data, std::string* error);

// ---- extras (pcv_s2_attr.hip) -----------------------------------------------------------------------------------------------
uint32_t pcv_s2_attr_size(int32_t data_type);                         // bytes per element; 0: no data type of attributes.rs:8-21
bool pcv_s2_attr_name_ok(const std::string& name, std::string* why);  // the naming rules of include/pcv_hip.h
// the caller's list checked and sorted by name into *out (src set, nothing allocated); *why names the attribute
int pcv_s2_attr_check(const pcv_attribute* attrs, uint32_t num_attrs, uint64_t n, std::vector<PcvS2Extra>* out, std::string* why);
// split: c->extras[k].d = the column regrouped by `order` (device, n slots), one launch per extra; host columns staged through `sc`
struct PcvScratch;
int pcv_s2_attr_gather(pcv_ctx* ctx, PcvScratch& sc, const uint32_t* order, uint64_t n, int mem, pcv_s2_cloud* c);
// merge: one launch per extra over the plan that s2_merge_kernel ran on (device tables of pcv_s2_stream.hip)
struct pcv_s2_merge_segment;
int pcv_s2_attr_merge(pcv_ctx* ctx, PcvScratch& sc, uint64_t n, uint64_t num_segments, uint64_t num_chunks, const uint64_t* d_seg_dst,
                      const pcv_s2_merge_segment* d_segs, const uint64_t* d_chunk_first, const std::vector<pcv_s2_cloud*>& parts,
                      pcv_s2_cloud* out);
// an opened cloud's extra k: its files read (and uploaded) on first use
int pcv_s2_extra_resident(pcv_s2_cloud* c, size_t k, bool* absent = nullptr);
void pcv_s2_extras_release(pcv_s2_cloud* c);
// (name, data type) of the extras, as pcv_s2_write_meta lists them; every extra's runs onto the cells' `<token>.<name>` files.
// *written: the extras that were written — an opened cloud's extra of which its directory holds no file at all is left out
std::vector<std::pair<std::string, int32_t>> pcv_s2_extra_list(const pcv_s2_cloud* c);
int pcv_s2_attr_write(pcv_s2_cloud* c, const char* directory, const uint8_t* truncate /* as pcv_s2_write_cells takes it */,
                      std::vector<std::pair<std::string, int32_t>>* written = nullptr);
// query: one filter launch per distinct filtered extra, between the flags launches and the scan (pcv_s2_points.hip)
struct PcvS2Chunk;
constexpr uint32_t kPcvS2EveryLocation = 0xffffffffu;  // PcvS2ExtraFilter::location: every location of the call (xray's tiles)
struct PcvS2ExtraFilter {
  uint32_t location;
  int extra;  // index into pcv_s2_cloud::extras
  double lo, hi;
};
int pcv_s2_attr_filter(pcv_ctx* ctx, PcvScratch& sc, pcv_s2_cloud* c, const PcvS2Chunk* d_chunks, const std::vector<PcvS2Chunk>& chunks,
                       uint64_t locations, const std::vector<PcvS2ExtraFilter>& filters, uint32_t* d_flags);

// pcv_s2_query_run_ex's "every location" form (pcv_s2_points.hip), for a caller that has checked its filters itself
// (pcv_xray_run_s2_ex): `intervals` as pcv_s2_query_run takes them (nullable, on intensity), and filters on extras whose
// location is kPcvS2EveryLocation — no list of locations x filters is built
struct pcv_shapes;
struct pcv_s2_query;
int pcv_s2_query_run_every(pcv_s2_cloud* c, const pcv_shapes* shapes, const double* intervals, const std::vector<PcvS2ExtraFilter>& filters,
                           pcv_s2_query** out);

// a union's cells as the entry points take them: ascending by id, no 0 (pcv_s2.hip); *why says what is wrong
int pcv_s2_check_union(const uint64_t* cells, uint32_t num_cells, std::string* why);
// several unions as pcv_s2_cells_in_location takes them (pcv_s2_query.hip): union_first[0] == 0, no descent, each union as above,
// every cell an S2 cell id
int pcv_s2_check_unions(uint32_t num_unions, const uint32_t* union_first, const uint64_t* union_cells, std::string* why);
// the blobs of an opened cloud on the device (pcv_s2.hip: read and uploaded on first use); nothing to do for a split
int pcv_s2_make_resident(pcv_s2_cloud* c);
// pcv_s2_split's checks and split for one batch of a stream (pcv_s2_stream.hip); with_order false: no d_order is made.
// pcv_s2_release frees a cloud whose device work the caller has waited for.
// extras: null or the checked list of pcv_s2_attr_check (consumed).
int pcv_s2_split_part(pcv_ctx* ctx, const pcv_points* points, uint32_t level, bool with_order, pcv_s2_cloud** out,
                      std::vector<PcvS2Extra>* extras = nullptr);
void pcv_s2_release(pcv_s2_cloud* c);
