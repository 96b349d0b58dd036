// pcv_ply_write.h — the binary PLY that PlyNodeWriter writes with Encoding::Plain (reference src/read_write/ply.rs:559-732),
// as plain host C++: the columns of a row, the header, the append check and the file itself. No HIP; the rows come from
// pcv_ply_rows.hip.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

// One attribute column of a row. Position (three doubles, 24 bytes) always comes first and is not listed.
struct PcvPlyColumn {
  std::string name;
  int32_t data_type = 0;  // PCV_ATTR_*
  uint32_t elem = 0;      // bytes per point
  uint32_t offset = 0;    // byte offset inside the row
  uint32_t given = 0;     // the caller's index of this name
};

constexpr uint32_t kPcvPlyPositionBytes = 24;
constexpr uint32_t kPcvPlyCountAt = 51;      // HEADER_START_TO_NUM_VERTICES.len() (ply.rs:32-33)
constexpr uint32_t kPcvPlyCountDigits = 20;  // HEADER_NUM_VERTICES.len() (ply.rs:34)

uint32_t pcv_ply_elem_size(int32_t data_type);  // attributes.rs:64-73; 0: no data type
// The caller's (name, data type) list as the columns of a row: ascending by name, bytewise (BTreeMap<String, AttributeData>
// iteration order), offsets from 24 on, *stride the row's bytes. PCV_E_INVALID with *why: a null or repeated name, a data type
// of 0 ("Data type for attribute 'NAME' not found."), any other unknown data type.
int pcv_ply_columns(const char* const* names, const int32_t* data_types, uint32_t n, std::vector<PcvPlyColumn>* cols, uint32_t* stride,
                    std::string* why);
// create_header (ply.rs:691-731) with `count` in the fixed 20-digit field
std::string pcv_ply_header(const std::vector<PcvPlyColumn>& cols, uint64_t count);
// OpenMode::Append (ply.rs:663-689) with the header check of DESIGN §9f: *old_count from the fixed field and *old_size the file's
// length; a missing file or one shorter than the fixed prefix counts as empty (0, 0). PCV_E_INVALID with *why naming the first
// property line that differs from the header these columns give; PCV_E_IO when the file cannot be read.
int pcv_ply_append_check(const char* path, const std::vector<PcvPlyColumn>& cols, uint64_t* old_count, uint64_t* old_size, std::string* why);

// The file of one write call. Nothing exists on disk before the first rows arrive (DataWriter's drop removes an empty file,
// node_writer.rs:78-84: here it is never created); commit writes the trailing newline and patches the count (ply.rs:646-658);
// abandon removes a truncated file, and cuts an appended one back to its old length and count.
struct PcvPlyFile {
  std::string path;
  bool append = false;
  int fd = -1;
  bool opened = false;  // this call has created or opened the file
  uint64_t old_count = 0, old_size = 0;
  uint64_t body_at = 0;  // file offset of the first row this call writes
  uint64_t rows = 0;
  std::string header;    // of a file this call creates
  // checks (append) and remembers; opens nothing
  int begin(const char* path, bool append, const std::vector<PcvPlyColumn>& cols, std::string* why);
  int open_for_rows(std::string* why);  // before the first write: creates / opens, writes the header of a new file
  // `bytes` at `offset` past body_at; may be called from several threads at once for disjoint ranges
  int write_at(uint64_t offset, const void* data, uint64_t bytes, std::string* why);
  int commit(uint64_t rows, uint32_t stride, std::string* why);
  void abandon();
};
