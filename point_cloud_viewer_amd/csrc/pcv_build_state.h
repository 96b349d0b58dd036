// pcv_build_state.h — what the files of the octree build share: the staged input (DevPoints), the state of a build between
// pcv_build_begin and pcv_build_finish (PcvBuild), and the functions of pcv_build.hip / pcv_single_chain.hip that the other
// build files call.
#pragma once
#include "pcv_internal.h"
#include "pcv_spec.h"
#include "pcv_tables.h"

struct DevPoints {
  uint64_t n = 0;
  const double *x = nullptr, *y = nullptr, *z = nullptr;
  PcvRouted routed;  // multi-GPU build: level-1 chain state instead of raw coordinates
  const uint8_t* color = nullptr;
  uint32_t color_stride = 3;
  const float* intensity = nullptr;
};

// State of a build between pcv_build_begin (through the topology) and pcv_build_finish (encode + promotion).
struct PcvBuild {
  pcv_ctx* ctx;
  PcvScratch sc;
  DevPoints d;
  uint64_t n = 0;
  bool stage_times = false;  // PCV_BUILD_STAGE_TIMES of THIS build (a context may have begun another one before the finish)
  PcvLevels lv;
  uint64_t *keys_a = nullptr, *keys_b = nullptr;
  void* sort_scratch = nullptr;
  uint32_t M = 0;
  std::vector<uint64_t> pre;  // |pre(node)| stream lengths, bottom-up
  bool deep = false;          // more than PCV_MAX_KEY_LEVELS levels: second key word, prefix_lo in the node table
  int levels = 0;             // levels the level tables are valid for in K5/K6 (full depth, or the deep depth)
  uint64_t* d_prefix_lo = nullptr;
  // single-chain build: the records (true-leaf rank, leaf codes + rgb[, intensity]) already exist when the topology does
  bool spec = false;
  void* spec_payload = nullptr;  // uint4[n]; uint2[n] with 12-byte records
  void* spec_wide = nullptr;     // set: 12-byte records (pcv_internal.h); uint4[n], the codes of Float32-coded leaves
  const uint32_t* spec_rows = nullptr;  // rank counts per sort workgroup (pcv_launch_rank_hist_rows), or null
  PcvSortSecond sort_second;            // the record sort's second pass, held back until the node tables are up (pcv_build_finish)
  uint64_t wide_levels = 0;      // bit k: level k is Float32-coded
  std::vector<PcvFixRange> fix_ranges;  // sorted slots whose points replay the chain after the record sort
  const uint32_t* spec_map_dev = nullptr;  // set: the record sort's first upsweep applies the rank map
  uint32_t spec_map_entries = 0;
  // true leaves below a split first candidate (PcvTrueTree::cont_nodes / cont_from): their chain is continued after the sort
  std::vector<uint32_t> cont_nodes, cont_from;
  // the record sort (queue_record_sort): buffers and where the sorted records ended up
  bool sort_queued = false, rec_in_a = true;
  void *pay_a = nullptr, *pay_b = nullptr;
  // device resolve (spec_resolve_kernel drives the record sort) vs host resolve (pcv_spec_resolve builds the tables): what the
  // device reported — {true leaves, too shallow} — lands in mailbox[kPcvMailboxResolve] and pcv_build_finish compares it with
  // the host's tree before anything of the build is handed out; check_map: the whole rank map is compared too
  bool resolve_on_device = false, resolve_check_map = false;
  uint32_t resolve_host_leaves = 0;
  std::vector<uint32_t> resolve_host_map;
  std::vector<uint8_t> resolve_host_inner;  // T'' node is an inner node: its map entry is never read (the device leaves it unwritten)
  PcvSortPayload pl;
  bool color_late = false;  // single-chain build: the chain pass wrote its records without the colour
  // ... and as packed 8-byte records with the ranks as a plane of half words in keys_a (pcv_packed_handover: the pass was
  // launched in that form and the predicted tree is small enough)
  bool pack_tried = false, packed = false;
  explicit PcvBuild(pcv_ctx* c) : ctx(c), sc(c) {}
  // A build dropped between begin and finish (an error in finish before the held-back pass was queued, a tree freed without
  // finish): the pass's layout kernels on the side stream write into `sc`'s sort scratch; the main stream must be ordered behind
  // them before the members below hand that scratch back to the pool
  ~PcvBuild() {
    if (sort_second.pending && sort_second.join_side) (void)ctx->side_end();
  }
  // The single-chain attempt is given up after its chain pass (`payload`, and `wide` with 12-byte records, are that pass's
  // buffers): the exact pipeline redoes the build.
  void drop_single_chain(void* payload, void* wide) {  // nothing of this attempt is kept; queued work on the scratch buffers drains harmlessly
    // (the pool is stream-ordered: a freed block is only handed to work queued later on the same stream). The record sort
    // that was queued ahead of the verdict leaves its second payload buffer and the rank-count rows behind: without this
    // the fallback — which allocates its own record buffers — would be the build's memory peak
    if (sort_queued && pay_b && pay_b != payload) {
      sc.detach(pay_b);
      ctx->dev_free(pay_b);
    }
    if (spec_rows) {
      sc.detach((void*)spec_rows);
      ctx->dev_free((void*)spec_rows);
    }
    pay_a = pay_b = nullptr;
    spec = false;
    spec_payload = nullptr;
    spec_wide = nullptr;
    spec_map_dev = nullptr;
    spec_rows = nullptr;
    sort_queued = false;
    // a held-back second pass is simply never queued — but its layout kernels may still be running on the side stream, writing
    // into the sort scratch that goes back to the (main-stream-ordered) pool below: join them first
    if (sort_second.pending && sort_second.join_side) (void)ctx->side_end();
    sort_second = PcvSortSecond();
    resolve_on_device = false;
    sc.detach(payload);
    ctx->dev_free(payload);
    if (wide) {
      sc.detach(wide);
      ctx->dev_free(wide);
    }
  }
};

// ---- pcv_build.hip: input staging, K1, the node table's scratch, the build up to the topology ----
int pcv_validate_points(pcv_ctx* ctx, const pcv_points* p, bool need_color);
int pcv_stage_points(pcv_ctx* ctx, PcvScratch& sc, const pcv_points* p, bool with_attrs, DevPoints* d);
// K1 in two halves (launch, wait), and both at once
int pcv_device_aabb_launch(pcv_ctx* ctx, PcvScratch& sc, const DevPoints& d);
int pcv_device_aabb_wait(pcv_ctx* ctx, double bmin[3], double bmax[3]);
int pcv_device_aabb(pcv_ctx* ctx, PcvScratch& sc, const DevPoints& d, double bmin[3], double bmax[3]);
// Scratch for a device node table of n points: capacity for every level down to `deepest`; max_open: open nodes a level may
// have as far as the scratch of the two-levels-per-launch kernels goes (capped at 2^22)
int pcv_alloc_node_table(PcvScratch& sc, uint64_t n, uint32_t max_points, int deepest, uint64_t max_open, PcvNodeTableDev* out);
// given_tree (pcv_gather_encode): the topology is an input
int pcv_build_begin_impl(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, const pcv_routed_points* routed,
                         pcv_octree** out, const PcvTrueTree* given_tree = nullptr);

// ---- pcv_single_chain.hip ----
int pcv_queue_record_sort(pcv_ctx* ctx, PcvBuild* bs, pcv_octree* t, const PcvWalkTables* wt, uint32_t num_leaves, bool wide);
int pcv_queue_replay(pcv_ctx* ctx, PcvBuild* bs);
int pcv_single_chain_topology(pcv_ctx* ctx, PcvBuild* bs, pcv_octree* t, const pcv_build_params* params, uint32_t max_points,
                              int full_levels, PcvNodeTableDev& nt, PcvTrueTree* tt, bool* used);
