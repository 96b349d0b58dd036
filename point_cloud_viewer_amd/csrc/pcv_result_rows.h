// pcv_result_rows.h — the host side that the result writers share: a query result as a packer sees it, and the
// piece pipeline that streams packed bytes into files through two device buffers and two pinned blocks (pcv_ply_rows.hip,
// pcv_las_write.hip, pcv_tiles3d.hip).
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "pcv_internal.h"
#include "pcv_query_dev.h"
#include "pcv_s2_obj.h"
#include "pcv_s2_query_dev.h"

// A result as a packer sees it: one of the two kinds of query, and its segment tables.
struct PcvResultSource {
  pcv_ctx* ctx = nullptr;
  pcv_query_batch* octree = nullptr;
  pcv_s2_query* s2 = nullptr;
  uint64_t nseg = 0;
  const uint64_t *seg_off = nullptr, *seg_chunk = nullptr;  // nseg + 1 each
  int check_range(uint64_t first_segment, uint64_t num_segments) const {
    if (first_segment > nseg || num_segments > nseg - first_segment) return ctx->fail(PCV_E_INVALID, "segment range past the end");
    return PCV_OK;
  }
  // the rows [p0, p0 + np) of a checked segment range, and the chunks [c0, c1) that hold them
  struct Rows {
    uint64_t p0, np, c0, c1;
  };
  Rows rows_of_segments(uint64_t first_segment, uint64_t num_segments) const {
    const uint64_t p0 = seg_off[first_segment];
    return Rows{p0, seg_off[first_segment + num_segments] - p0, seg_chunk[first_segment], seg_chunk[first_segment + num_segments]};
  }
};
inline PcvResultSource source_of(pcv_query_batch* b) {
  PcvResultSource s;
  s.ctx = b->ctx, s.octree = b, s.nseg = b->nseg, s.seg_off = b->seg_off.data(), s.seg_chunk = b->seg_chunk.data();
  return s;
}
inline PcvResultSource source_of(pcv_s2_query* q) {
  PcvResultSource s;
  s.ctx = q->cloud->ctx, s.s2 = q, s.nseg = q->nseg, s.seg_off = q->seg_offset.data(), s.seg_chunk = q->seg_first_chunk.data();
  return s;
}

// pcv_ply_rows.hip — rows [row0, row0 + nrows) of the result's segments [first_segment, first_segment + num_segments) as 27-byte
// rows (x y z as doubles, then r g b) into d_out on the context's stream, nothing waited for — any row range, for callers that
// stream a result through a bounded buffer (pcv_terrain.hip, pcv_maptiles.hip).
constexpr uint32_t kPcvXyzRgbRowBytes = 27;
int pcv_ply_pack_xyz_rgb(const PcvResultSource& s, uint64_t first_segment, uint64_t num_segments, uint64_t row0, uint64_t nrows, uint8_t* d_out);

// The piece pipeline: the output in pieces; piece k + 1 is packed on the context's stream while piece k crosses to its pinned
// block on the side stream and piece k - 1 is written by the host threads. Device and pinned memory: two buffers of the largest
// piece each, whatever the output's size.
struct PcvPiecePipe {
  hipEvent_t packed[2] = {}, copied[2] = {};
  int make(pcv_ctx* ctx) {
    for (int k = 0; k < 2; ++k) {
      PCV_HIP_CHECK(ctx, hipEventCreateWithFlags(&packed[k], hipEventDisableTiming));
      PCV_HIP_CHECK(ctx, hipEventCreateWithFlags(&copied[k], hipEventDisableTiming));
    }
    return PCV_OK;
  }
  ~PcvPiecePipe() {
    for (int k = 0; k < 2; ++k) {
      if (packed[k]) (void)hipEventDestroy(packed[k]);
      if (copied[k]) (void)hipEventDestroy(copied[k]);
    }
  }
};

// after a failure: nothing queued may still use what the caller frees next
inline void pcv_drain_pieces(pcv_ctx* ctx) {
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->side);
  (void)hipGetLastError();
}

// The loop. pack(k, b) queues piece k into d_buf[b] on ctx->stream; its bytes_of(k) bytes cross to h_buf[b] on ctx->side;
// write(k, b) is the host's part: it waits for pipe.copied[b], then writes h_buf[b]. A failure drains both streams before it is
// returned, so the caller's scratch and pinned blocks are never freed under queued work.
template <typename Pack, typename BytesOf, typename Write>
int pcv_run_pieces(pcv_ctx* ctx, const PcvPiecePipe& pipe, uint64_t npieces, Pack pack, BytesOf bytes_of, uint8_t* const d_buf[2],
                   uint8_t* const h_buf[2], Write write) {
  auto run = [&]() -> int {
    for (uint64_t k = 0; k < npieces; ++k) {
      const int b = (int)(k & 1);
      // d_buf[b] (and whatever else pack keeps per buffer) was last used by piece k - 2, whose copy write(k - 2) has waited
      // for; h_buf[b] likewise
      if (int r = pack(k, b)) return r;
      PCV_HIP_CHECK(ctx, hipEventRecord(pipe.packed[b], ctx->stream));
      PCV_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->side, pipe.packed[b], 0));
      PCV_HIP_CHECK(ctx, hipMemcpyAsync(h_buf[b], d_buf[b], bytes_of(k), hipMemcpyDeviceToHost, ctx->side));
      PCV_HIP_CHECK(ctx, hipEventRecord(pipe.copied[b], ctx->side));
      if (k > 0)
        if (int r = write(k - 1, b ^ 1)) return r;
    }
    return write(npieces - 1, (int)((npieces - 1) & 1));
  };
  const int rc = run();
  if (rc != PCV_OK) pcv_drain_pieces(ctx);
  return rc;
}

// `bytes` bytes by write_at(lo, len, &why) in slices of at least 4 MiB, one per host thread; the first failed slice's code and
// message are the context's
template <typename WriteAt>
int pcv_write_slices(pcv_ctx* ctx, uint64_t bytes, WriteAt write_at) {
  const size_t workers = ctx->host_pool.threads.size() + 1;
  const uint64_t slice = std::max<uint64_t>(4u << 20, (bytes + workers - 1) / workers);
  const size_t parts = (size_t)((bytes + slice - 1) / slice);
  std::vector<int> part_rc(parts, PCV_OK);
  std::vector<std::string> part_why(parts);
  auto one = [&](size_t p) {
    const uint64_t lo = p * slice;
    part_rc[p] = write_at(lo, std::min(slice, bytes - lo), &part_why[p]);
  };
  if (parts == 1) one(0);
  else ctx->host_pool.run(parts, one);
  for (size_t p = 0; p < parts; ++p)
    if (part_rc[p]) return ctx->fail(part_rc[p], part_why[p]);
  return PCV_OK;
}
