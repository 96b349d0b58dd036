/* pcv_hip.h — C ABI of the MI355X-native octree-build / cull hot path of point_cloud_viewer.
 *
 * The reference (Rust) has no FFI boundary for this path; the boundary is the crate's public
 * surface. Each entry point below names the reference item it replaces (paths relative to the
 * reference checkout). A Rust veneer (point_cloud_viewer_amd/rust_shim/) binds these
 * 1:1 and keeps `build_octree`, `Octree`, `NodeId`, `PointCulling` as the user-facing names.
 *
 * Rules of the ABI
 *  - plain pointers and sizes only; the caller owns every input buffer, the library never frees them;
 *  - every function returns an int status (PCV_OK or a negative PCV_E_*), never unwinds;
 *    pcv_last_error(ctx) holds a human-readable message for the last failure on that context;
 *  - a pcv_ctx is bound to one HIP device + one stream and is NOT thread-safe; use one per host
 *    thread/device (reference: the build uses the global rayon pool, src/bin/build_octree.rs:43-46);
 *  - buffers are tagged PCV_MEM_HOST or PCV_MEM_DEVICE; device buffers must live on the ctx's device.
 */
#ifndef PCV_HIP_H
#define PCV_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* additions that leave every existing entry as it was (pcv_png_decode, pcv_xray_open_dir, pcv_xray_merge, ...) do not
 * move the version.
 * 2 (round 6): pcv_ingest_*, PCV_ROUTE_OCTANTS_ONLY, PCV_STAGE_SORT_SECOND (PCV_STAGE_TOTAL moved from 8 to 9) */
#define PCV_ABI_VERSION 2

/* status codes (reference: error-chain kinds src/errors.rs:18-48; the builder itself panics) */
#define PCV_OK 0
#define PCV_E_INVALID (-1) /* bad argument (ErrorKind::InvalidInput) */
#define PCV_E_HIP (-2)     /* HIP runtime failure */
#define PCV_E_IO (-3)      /* file system failure (ErrorKind::Io) */
#define PCV_E_OOM (-4)     /* device or host allocation failed / node table capacity exceeded */
#define PCV_E_DEPTH (-5)   /* a node at level 40 would still have to be split (the reference's NodeId ends there too) */
#define PCV_E_NOT_FOUND (-6) /* ErrorKind::NodeNotFound */

#define PCV_MEM_HOST 0
#define PCV_MEM_DEVICE 1

/* position encodings == proto PositionEncoding values (point_viewer_proto_rust/src/proto.proto:82-88) */
#define PCV_ENC_UINT8 1
#define PCV_ENC_UINT16 2
#define PCV_ENC_FLOAT32 3
#define PCV_ENC_FLOAT64 4

/* path digits kept per point: 3 bits per level in a 64-bit key word; deeper trees (up to 40 levels, all the
 * reference's u128 NodeId can name) use a second word inside the library */
#define PCV_MAX_KEY_LEVELS 21
/* reference src/octree/generation.rs:37 */
#define PCV_DEFAULT_MAX_POINTS_PER_NODE 100000u

typedef struct pcv_ctx pcv_ctx;
typedef struct pcv_octree pcv_octree;

/* ---- context -------------------------------------------------------------------------------- */
/* `stream` is a hipStream_t (may be NULL = a stream owned by the context). The context also owns a small side stream
 * for copies that would otherwise sit between two kernels (the build's host mirror of the predicted tree, the upload
 * of the node tables); everything queued there is joined back into `stream` before a kernel that depends on it, so
 * the caller only ever orders itself against `stream` (pcv_ctx_wait_stream / pcv_ctx_signal_stream). */
int pcv_ctx_create(int device, void* stream, pcv_ctx** out);
void pcv_ctx_destroy(pcv_ctx* ctx);
const char* pcv_last_error(const pcv_ctx* ctx);
int pcv_abi_version(void);
/* Wait for everything queued on the context's stream (the few entry points documented as asynchronous). */
int pcv_ctx_synchronize(pcv_ctx* ctx);
/* Stream hand-off with the caller's runtime (torch, RCCL, another library) without blocking the host:
 * pcv_ctx_wait_stream   - everything queued on the context's stream AFTER this call runs after what is queued on
 *                         `stream` now (the caller produced the inputs there);
 * pcv_ctx_signal_stream - what is queued on `stream` after this call runs after the context's work queued so far
 *                         (the caller consumes device-resident outputs there).
 * `stream` is a hipStream_t of the context's device; NULL names the legacy default stream. Because NULL in
 * pcv_ctx_create means "own stream", a caller whose work sits on the default stream MUST order it with these two
 * calls (or synchronise the device) before handing buffers over. */
int pcv_ctx_wait_stream(pcv_ctx* ctx, void* stream);
int pcv_ctx_signal_stream(pcv_ctx* ctx, void* stream);
/* Release cached device/host scratch held by the context. */
int pcv_ctx_trim(pcv_ctx* ctx);

/* Optional per-launch profile: enabled = 1 brackets every kernel launch of this context with HIP events on the
 * context's stream, enabled = 2 only the kernels that pass over the whole cloud (an event pair costs the stream a few
 * microseconds; a build makes ~100 small launches); pcv_ctx_kernel_stats returns, per kernel id (0 .. return value - 1),
 * the kernel's name, the number of launches and their summed duration since the last reset. */
int pcv_ctx_set_profiling(pcv_ctx* ctx, int enabled);
int pcv_ctx_reset_kernel_stats(pcv_ctx* ctx);
int pcv_ctx_kernel_stats(pcv_ctx* ctx, int kernel_id, const char** name, uint64_t* launches, double* total_ms);

/* ---- inputs --------------------------------------------------------------------------------- */
/* One batch of points, SoA. Replaces `PointsBatch` (src/lib.rs:102-107): positions Vec<Point3<f64>>,
 * "color" U8Vec3 and optional "intensity" F32 (src/octree/mod.rs:62-74). */
typedef struct pcv_points {
  uint64_t n;
  const double* x;
  const double* y;
  const double* z;
  const uint8_t* color;   /* n * color_stride bytes, r,g,b first; required */
  uint32_t color_stride;  /* 3 (as in .rgb files) or 4 (rgba, alpha ignored) */
  const float* intensity; /* NULL = no "intensity" attribute */
  int32_t mem;            /* PCV_MEM_HOST or PCV_MEM_DEVICE (all pointers alike) */
} pcv_points;

/* Arguments of `build_octree` (src/octree/generation.rs:289-295). */
typedef struct pcv_build_params {
  double resolution;            /* meters; reference CLI default 0.001 (src/bin/build_octree.rs:33) */
  double bbox_min[3];           /* `bounding_box: Aabb`; may be loose */
  double bbox_max[3];
  uint32_t max_points_per_node; /* 0 = PCV_DEFAULT_MAX_POINTS_PER_NODE (the reference's constant) */
  uint32_t flags;               /* PCV_BUILD_* */
} pcv_build_params;

/* Compute the bounding box on the device first (== build_octree_from_file's find_bounding_box pass,
 * generation.rs:256-287); bbox_min/max are then outputs. */
#define PCV_BUILD_COMPUTE_BBOX 1u
/* Exact two-chain pipeline with full-depth path keys: disables the single-chain build and the sampled depth
 * speculation (same result, slower). */
#define PCV_BUILD_NO_SPECULATION 2u
/* Take the single-chain build (topology predicted from a strided sample, ONE chain pass, exact per-leaf counts decide
 * the tree; see csrc/pcv_spec.h) whatever the input size; by default it is used from 2^22 points on. Same result: if
 * the prediction does not cover the tree the exact pipeline redoes the build. */
#define PCV_BUILD_FORCE_SINGLE_CHAIN 4u
/* Never take the single-chain build (the exact pipeline with its depth speculation runs instead). */
#define PCV_BUILD_NO_SINGLE_CHAIN 8u
/* Single-chain build, diagnostics: the device's predicted-leaf -> true-leaf rank map (which drives the record sort) is
 * downloaded and compared entry by entry with the host's (which the node tables come from) before the octree is handed
 * out; PCV_E_HIP on a difference. Without the flag only the number of true leaves and the "too shallow" verdict of the two
 * resolves are compared (always, for free). */
#define PCV_BUILD_CHECK_RESOLVE 16u
/* Record the GPU time of every stage of the build (pcv_octree_stage_ms). Off by default: the 16 event records of a build
 * cost its stream ~0.1 ms (measured: 5.31 -> 5.21 ms per 100 M-point build), which a caller who does not read the stage
 * times should not pay; without the flag only PCV_STAGE_TOTAL is measured and the other stages read 0. */
#define PCV_BUILD_STAGE_TIMES 32u

/* Multi-GPU build: level-1 nodes whose bit is set are split even if this rank's share of their points
 * is below the capacity — the split decision of the GLOBAL tree, made from the all-reduced bucket counts. */
#define PCV_BUILD_FORCE_SPLIT_L1(mask8) (((uint32_t)(mask8) & 0xffu) << 8)

/* ---- the build ------------------------------------------------------------------------------ */
/* Replaces build_octree (generation.rs:289-403) up to, but not including, the file writes:
 * the result holds the finished node table and node-contiguous .xyz/.rgb/.intensity bytes. */
int pcv_build_octree(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, pcv_octree** out);

/* Limits of one call (stated here, not discovered at run time): positions are addressed with 32 bits, so a build takes at
 * most 2^32 - 2 points (PCV_E_INVALID above that); everything is device-resident, about 80 bytes of HBM per point at the
 * peak of a build (27-31 B of input + records, rank counts, the wide-code pool and the output blobs), so ONE 288 GB MI355X
 * ends at roughly 3 x 10^9 points. The reference streams any size through node files (generation.rs:58-126); larger clouds
 * go through the out-of-core build (pcv_ooc_*, below: one GPU, the points wait in host memory — about 17-21 B per point with a
 * Float32-coded level 1, 28-32 B otherwise — and are built in passes of at most max_points_per_pass points, each under this
 * limit; the total is counted in 64 bits) or the multi-GPU path (pcv_route_* + pcv_build_begin_routed), which shards by subtree. */
#define PCV_MAX_POINTS_PER_BUILD 0xfffffffeull

/* ---- streaming batch ingest: the reference's `impl Iterator<Item = PointsBatch>` (generation.rs:289-295) ------------
 * A PointsBatch (src/lib.rs:102-107) holds `position: Vec<Point3<f64>>` — AoS, 24 bytes per point — "color"
 * Vec<Vector3<u8>> (3 bytes per point) and optionally "intensity" Vec<f32> (src/octree/mod.rs:62-74), and arrives 500 000
 * points at a time (src/lib.rs:52). These calls take the batches AS THEY ARE, one at a time:
 *   pcv_ingest_begin   num_points_hint = NumberOfPoints::num_points() of the stream (0 = unknown: the device arrays grow);
 *                      has_intensity = the attribute list names "intensity" (then every batch must carry it).
 *   pcv_ingest_append  copies the batch's three arrays side by side into the chunk of the context's pinned ring it has in
 *                      hand; a chunk that cannot take the next batch goes up in ONE DMA (32 MiB: two batches of 500 000
 *                      points), followed by ONE kernel per batch that transposes the positions AoS -> SoA into place behind
 *                      the points already on the device, copies colour / intensity behind theirs and folds the batch into
 *                      the running bounding box (find_bounding_box, generation.rs:256-270). Returns when the batch is in
 *                      the chunk — the caller's arrays are free again and the next batch can be produced while earlier
 *                      ones go up. Batches of any size (split into pieces of 2^20 points inside); n == 0 is a no-op. Host
 *                      memory: the ring (3 x 32 MiB), whatever the size of the cloud.
 *   pcv_ingest_bbox    the bounding box of the points appended so far (waits for the queued batches); Aabb::zero() for none.
 *   pcv_ingest_finish  pcv_build_octree on the ingested cloud; with PCV_BUILD_COMPUTE_BBOX the box folded during the ingest
 *                      is used (no pass over the cloud), otherwise params->bbox_* as build_octree takes it from its caller.
 *                      ALWAYS consumes the ingest, whatever it returns.
 *   pcv_ingest_abort   drops an ingest without building.
 * Other calls on the context between begin and finish (another ingest, a build from host arrays) are allowed: the chunk in
 * hand is theirs to pass over, not to reuse. */
typedef struct pcv_ingest pcv_ingest;
int pcv_ingest_begin(pcv_ctx* ctx, uint64_t num_points_hint, int has_intensity, pcv_ingest** out);
int pcv_ingest_append(pcv_ingest* ingest, const double* xyz /* n x 3, x y z per point (host) */, const uint8_t* rgb /* n x 3 (host) */,
                      const float* intensity /* n (host), NULL without the attribute */, uint64_t n);
uint64_t pcv_ingest_num_points(const pcv_ingest* ingest);
int pcv_ingest_bbox(pcv_ingest* ingest, double bbox_min[3], double bbox_max[3]);
int pcv_ingest_finish(pcv_ingest* ingest, const pcv_build_params* params, pcv_octree** out);
void pcv_ingest_abort(pcv_ingest* ingest);

/* The same build in two steps, for the multi-GPU path: when the level-2 subtrees of one level-1 node live on
 * different ranks, the every-8th promotion (generation.rs:195-253) into the level-1 node and into the root runs over
 * streams that span ranks, so the stream offsets must be agreed between the topology and the encode phase.
 *   pcv_build_begin       K1..K4 + the bottom-up stream lengths |pre(node)| of the local tree
 *   pcv_build_top_streams lengths of the local level-1 / level-2 streams (0 = node absent on this rank)
 *   pcv_build_finish      K5, record sort, K6. With a layout, the root and the level-1 nodes are laid out at their
 *                         GLOBAL size and this rank fills only its own slots (the rest is zero): the element-wise sum
 *                         of all ranks' top-node bytes is the finished node. NULL layout == pcv_build_octree.
 * The caller's device buffers must stay valid and no other call may be made on the context in between; after a
 * failed pcv_build_finish the tree can only be freed. */
typedef struct pcv_top_streams {
  uint64_t l1[8];          /* |pre(r_c)|: points the level-1 node c holds before its own promotion */
  uint64_t l2[64];         /* |pre(r_cd)| at index c * 8 + d */
  uint32_t l1_split_mask;  /* bit c: level-1 node c is an inner node here */
  uint32_t reserved;
} pcv_top_streams;
typedef struct pcv_top_layout {
  uint64_t root_points;    /* global |pre(root)| == points the root keeps */
  uint64_t l1_stream[8];   /* global |pre(r_c)| */
  uint32_t l1_offset[8];   /* offset of r_c's promoted segment inside pre(root) */
  uint32_t l2_offset[64];  /* offset of r_cd's promoted segment inside pre(r_c) */
} pcv_top_layout;
int pcv_build_begin(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, pcv_octree** out);
/* pcv_build_begin for points that crossed the exchange as their level-1 chain state (pcv_route_buckets with a
 * pcv_route_state): the root octant digit and the Float32 level-1 codes — with the colour 16 B per point in four 4-byte
 * planes instead of 27 B. The chain continues at level 2 from decode(code) — the position the sending rank held after level 1,
 * so everything downstream is bit-identical. Device memory only; params carry the GLOBAL bounding box. */
typedef struct pcv_routed_points {
  uint64_t n;
  const uint32_t* cx;      /* Float32 bit patterns of the level-1 codes (codec.rs:102-121 with the level-1 child cube) */
  const uint32_t* cy;
  const uint32_t* cz;
  const uint32_t* oct_rgb; /* level-1 digit (0..7) in byte 0, r, g, b in bytes 1..3 */
  const float* intensity;  /* NULL = no "intensity" attribute */
} pcv_routed_points;
int pcv_build_begin_routed(pcv_ctx* ctx, const pcv_build_params* params, const pcv_routed_points* routed, pcv_octree** out);
int pcv_build_top_streams(const pcv_octree* tree, pcv_top_streams* out);
int pcv_build_finish(pcv_octree* tree, const pcv_top_layout* top /* nullable */);

/* ---- out-of-core build: clouds larger than the device through ONE GPU (build_octree, generation.rs:289-403) -------------
 * The reference streams any number of points through node files on disk. These calls take its batches one at a time, like
 * pcv_ingest_*, and write its directory; the points wait in host memory between two phases:
 *   pcv_ooc_begin   params: resolution, the GLOBAL bounding box (PCV_BUILD_COMPUTE_BBOX is rejected: the stream is read once),
 *                   max_points_per_node. max_points_per_pass bounds the points resident on the device at once (0 = derived
 *                   from the free device memory); each pass also stays under PCV_MAX_POINTS_PER_BUILD.
 *   pcv_ooc_append  the batch goes up through the context's pinned ring; one HIP pass writes it as 64 stable level-2 bucket runs
 *                   (the level-1 chain state, 16 B per point, where level 1 is Float32-coded, the raw 27 B otherwise; + 4 B of
 *                   intensity) that come back into per-bucket host spills, each in global input order. Host memory on the
 *                   input side is O(batch); the spill is O(cloud).
 *   pcv_ooc_finish  the 64 global counts give the level-1 split mask and partitions of whole units (single buckets under split
 *                   level-1 nodes, whole octants otherwise) of at most max_points_per_pass points — PCV_E_OOM naming the bucket
 *                   when one unit alone is larger; every partition is built twice (topology, then pcv_build_finish with the
 *                   global pcv_top_layout), its nodes of level >= 2 written as it finishes; the root / level-1 files and meta.pb
 *                   come last (a failed build leaves no meta.pb). The same directory as pcv_build_octree + pcv_octree_write_dir
 *                   of the whole cloud, byte for byte, whatever the partitioning; an empty stream writes meta.pb without
 *                   nodes and returns stats with points == 0, like the in-core build of it. ALWAYS consumes the handle.
 *   pcv_ooc_abort   drops the build; releases all device and host memory.
 * Counts on the host are 64-bit: the total may exceed 2^32. Other calls on the context between appends are allowed. */
typedef struct pcv_ooc pcv_ooc;
typedef struct pcv_ooc_stats {
  uint64_t points;          /* appended */
  uint64_t nodes;           /* in meta.pb */
  uint64_t partitions;
  uint64_t largest_bucket;  /* points */
  uint64_t spill_bytes;     /* host memory the points waited in between the phases */
  uint64_t h2d_bytes;       /* over the host link: batches up, partitions up (twice) */
  uint64_t d2h_bytes;       /* bucket runs down, the top nodes down */
  double h2d_ms, d2h_ms;    /* time of those copies */
  double stream_ms;         /* appends: copy into the ring + DMA + bucket runs + spill */
  double topology_ms;       /* first pass over the partitions (upload + topology) */
  double build_ms;          /* second pass (upload + build to the finished blobs) */
  double merge_ms;          /* top nodes folded into the accumulator */
  double write_ms;          /* node files and meta.pb */
  uint32_t split_mask;      /* bit c: the level-1 node c is split */
  uint32_t routed;          /* 1: the spill held the level-1 chain state; 0: raw planes */
} pcv_ooc_stats;
int pcv_ooc_begin(pcv_ctx* ctx, const pcv_build_params* params, int has_intensity, uint64_t max_points_per_pass, pcv_ooc** out);
int pcv_ooc_append(pcv_ooc* ooc, const double* xyz /* n x 3 (host) */, const uint8_t* rgb /* n x 3 (host) */,
                   const float* intensity /* n (host), NULL without the attribute */, uint64_t n);
int pcv_ooc_finish(pcv_ooc* ooc, const char* directory, pcv_ooc_stats* stats /* nullable */);
void pcv_ooc_abort(pcv_ooc* ooc);
/* The plan of pcv_ooc_finish from the 64 global bucket counts (host only, pure): split_mask by plan_buckets' rule (level-1 node c
 * is split iff level1_can_split and its octant holds more than max_points_per_node points); units in bucket order go next-fit into
 * partitions of at most max_points_per_pass points (0 = PCV_MAX_POINTS_PER_BUILD); partition_of_bucket[b] = UINT32_MAX for an
 * empty bucket. PCV_E_OOM (message in err) when one unit is larger than the budget. */
int pcv_ooc_plan(const uint64_t counts[64], uint32_t max_points_per_node, int level1_can_split, uint64_t max_points_per_pass,
                 uint32_t partition_of_bucket[64], uint32_t* num_partitions, uint32_t* split_mask, char* err, uint64_t errcap);
/* The global top layout from the summed stream lengths (l1[c] ignored where split_mask has bit c); host only. */
int pcv_ooc_top_layout(const uint64_t l1[8], const uint64_t l2[64], uint32_t split_mask, pcv_top_layout* out);
/* The pass of pcv_ooc_append on n device-resident points (xyz n x 3 AoS, rgb n x 3, intensity nullable): planes[0..4] receive
 * the 64 stable bucket runs (routed != 0: cx, cy, cz, oct_rgb as pcv_route_state, then intensity; routed == 0: x, y, z (f64),
 * rgb (3 B), intensity), octant_digits[n] the level-2 digit of every point in its root octant's range, in input order;
 * counts[64] (host) the run lengths. params->flags: PCV_ROUTE_OCTANTS_ONLY as for pcv_route_plan. */
int pcv_ooc_bucket_runs(pcv_ctx* ctx, const pcv_build_params* params, const double* xyz, const uint8_t* rgb, const float* intensity,
                        uint64_t n, int routed, void* const planes[5], uint8_t* octant_digits, uint64_t counts[64]);

/* One finished node == one `proto::OctreeNode` (proto.proto:90-94) + where its bytes are. */
typedef struct pcv_node_info {
  uint64_t id_high;     /* NodeId u128 halves (src/octree/node.rs:101-111): level<<56 | index>>64 */
  uint64_t id_low;
  int64_t num_points;   /* may be 0 (node exists in meta, no files; generation.rs:241-243) */
  uint32_t level;
  uint32_t encoding;    /* PCV_ENC_* */
  double cube_min[3];   /* NodeId::find_bounding_cube (node.rs:157-172) */
  double cube_edge;
  uint64_t xyz_offset;  /* byte offset of this node's .xyz content inside the xyz blob */
  uint64_t point_offset;/* index of this node's first point inside the rgb / intensity blobs */
} pcv_node_info;

uint64_t pcv_octree_num_nodes(const pcv_octree* t);
uint64_t pcv_octree_num_points(const pcv_octree* t);
int pcv_octree_has_intensity(const pcv_octree* t);
int pcv_octree_node(const pcv_octree* t, uint64_t i, pcv_node_info* out); /* i in (level, index) order */
void pcv_octree_meta(const pcv_octree* t, double* resolution, double bbox_min[3], double bbox_max[3], int* version);
/* File content of node i. which: 0 = .xyz, 1 = .rgb, 2 = .intensity. The host pointer stays valid
 * until pcv_octree_free. Replaces Octree::get_node_data's reads (src/octree/mod.rs:285-307). */
int pcv_octree_node_data(pcv_octree* t, uint64_t i, int which, const uint8_t** data, uint64_t* len);
/* Device-side blobs (no copy): which as above. */
int pcv_octree_device_blob(const pcv_octree* t, int which, const void** dptr, uint64_t* len);
/* Copy the bytes of node i (which: 0 .xyz, 1 .rgb, 2 .intensity) out of the device blob into `dst` (host or device
 * memory, `capacity` bytes) without staging the whole octree on the host. A copy to device memory is only queued on
 * the context's stream (follow with pcv_ctx_synchronize or stream-ordered work); a copy to host memory is complete on
 * return. */
int pcv_octree_copy_node(const pcv_octree* tree, uint64_t i, int which, void* dst, uint64_t capacity, int mem);
/* The same for a list of nodes into ONE destination buffer: copies[k].dst_offset[which] is where node copies[k].node's
 * .xyz / .rgb / .intensity bytes go (UINT64_MAX: skip that file kind). The multi-GPU build uses it to lay its share of
 * the root / level-1 nodes out for the top all-reduce in one call. Same completion rules as pcv_octree_copy_node. */
typedef struct pcv_node_copy {
  uint64_t node;
  uint64_t dst_offset[3];
} pcv_node_copy;
int pcv_octree_copy_nodes(const pcv_octree* tree, const pcv_node_copy* copies, uint64_t count, void* dst, uint64_t capacity, int mem);
/* Write `<NodeId>.xyz/.rgb/.intensity` + meta.pb (version 13) exactly as the reference lays them out
 * (src/read_write/raw.rs:374-449, node_writer.rs:78-89, generation.rs:390-402). */
int pcv_octree_write_dir(pcv_octree* t, const char* directory);
/* Multi-GPU output: every rank writes the node files of its own subtrees (level >= min_level, no meta.pb) ... */
int pcv_octree_write_nodes(pcv_octree* t, const char* directory, uint32_t min_level);
/* ... and one rank writes meta.pb for the gathered node table (id_high, id_low, num_points, encoding are used).
 * Host only; returns PCV_E_IO when the file cannot be written. Layout: proto.proto:58-149, octree/mod.rs:87-99. */
int pcv_write_meta(const char* directory, double resolution, const double bbox_min[3], const double bbox_max[3],
                   const pcv_node_info* nodes, uint64_t count);
void pcv_octree_free(pcv_octree* t);

/* Milliseconds spent per stage of the last pcv_build_octree on this tree (HIP events on the ctx
 * stream). Index with PCV_STAGE_*; returns the number of stages filled. */
#define PCV_STAGE_AABB 0
#define PCV_STAGE_CHAIN_KEYS 1
#define PCV_STAGE_SORT_KEYS 2
#define PCV_STAGE_NODE_SPLIT 3
#define PCV_STAGE_TABLE 4      /* node-table D2H + host finalize + H2D */
#define PCV_STAGE_LEAF_ENCODE 5
#define PCV_STAGE_SORT_RECORDS 6 /* the record sort's FIRST pass (+ histograms); a sort that runs to its end on its own: all passes */
#define PCV_STAGE_PROMOTE_ENCODE 7 /* from the node tables to the finished blobs; CONTAINS PCV_STAGE_SORT_SECOND */
/* The record sort's second pass when it is held back until the node tables are up (it then settles the leaves' points itself,
 * pcv_octree_settled_in_sort): queued inside PCV_STAGE_PROMOTE_ENCODE, measured on its own here — sort time =
 * SORT_RECORDS + SORT_SECOND, promotion proper = PROMOTE_ENCODE - SORT_SECOND. 0 when no pass was held back. */
#define PCV_STAGE_SORT_SECOND 8
#define PCV_STAGE_TOTAL 9
#define PCV_NUM_STAGES 10
int pcv_octree_stage_ms(const pcv_octree* t, float* ms, int cap);
/* How the last build went: attempts == 0: single-chain build (key_levels = levels the sample keys covered);
 * attempts == 1: exact pipeline, the sampled depth estimate held (key_levels = digit levels sorted);
 * attempts >= 2: something was redone (single-chain prediction too shallow and/or depth estimate too shallow). */
void pcv_octree_build_info(const pcv_octree* t, int* key_levels, int* attempts);
/* Single-chain build statistics of the last build (zeros otherwise): nodes and leaves of the predicted tree, points
 * whose leaf is an unsplit candidate node (the codes they kept there are their leaf codes), points that replayed the
 * chain from their coordinates. pcv_octree_spec_continued: points whose chain was continued from the codes kept at a
 * candidate node that turned out to be split. */
void pcv_octree_spec_stats(const pcv_octree* t, uint64_t stats[4]);
uint64_t pcv_octree_spec_continued(const pcv_octree* t);
/* Single-chain build with 12-byte records: number of points whose record left the chain pass with the codes of a
 * Float32-coded level (they wait in a dense side pool, the record names the entry); 0 otherwise. */
uint64_t pcv_octree_wide_pool_entries(const pcv_octree* t);
/* Single-chain build: points of the leaves whose final bytes the record sort's second pass produced itself (integer-coded
 * leaves whose records hold their leaf codes; generation.rs:222-238 — the reference rewrites every point that stays in a
 * node once); the other leaves' records are finished by the settle kernel. 0 when the sort ran to its end on its own. */
uint64_t pcv_octree_settled_in_sort(const pcv_octree* t);
/* Bytes of one record of the last build's record sort (rank + leaf codes + colour): 20, or 12 when the single-chain
 * build packed the record (16-bit codes; the points of Float32-coded levels travel as the index of their pool entry). */
int pcv_octree_record_bytes(const pcv_octree* t);
/* How the chain pass handed its records to the record sort: 0 = records with their colour; 1 = packed 8-byte records and a
 * plane of 16-bit ranks, loaded as they are by the sort's first pass, which joins the colour; 2 = packed, but unpacked in place
 * in front of a sort that cannot take them. */
int pcv_octree_packed_handover(const pcv_octree* t);

/* ---- stage-level entry points (unit parity against the oracle) ------------------------------ */
/* K1: find_bounding_box (generation.rs:256-270; Aabb::grow aabb.rs:41-44). n == 0 -> Aabb::zero(). */
int pcv_aabb_reduce(pcv_ctx* ctx, const pcv_points* points, double bbox_min[3], double bbox_max[3]);

/* Per-level table: edge[k] = root_edge / 2^k (node.rs:161), encoding[k] = PositionEncoding::new
 * (src/read_write/codec.rs:31-40). Returns max_level = first k >= 1 with edge[k] <= resolution
 * (no node below it can be split, generation.rs:137), capped at `cap`. */
int pcv_level_table(const double bbox_min[3], const double bbox_max[3], double resolution, int cap, double* edge,
                    int32_t* encoding);
/* The per-level shortcuts the single chain pass takes for this cube (host tables, for the tests that replay them in
 * exact arithmetic): digit_mode[k] = how the octant digit of level k + 1 (node.rs:34-42) is read off the level-k codes
 * (0 = comparison against the centre, 1 = from integer codes, 2 = from Float32 codes); code_threshold[k] = the power of
 * two from which on a Float32 code of level k + 1 (codec.rs:115-121) is taken as 2 v - bit from the level-k code v
 * instead of through the divide / cast chain (0.0 = the step always runs in full). Arrays of PCV_MAX_KEY_LEVELS + 2
 * entries. Returns max_level as pcv_level_table. */
int pcv_level_shortcuts(const double bbox_min[3], const double bbox_max[3], double resolution, uint32_t* digit_mode,
                        double* code_threshold);

/* K2: per-point path digits through the quantise->decode chain (ChildIndex::from_bounding_cube
 * node.rs:34-42, encode codec.rs:102-121, decode codec.rs:124-139, cube recurrence node.rs:157-172).
 * keys[i] has the digit of level k in bits [3*(21-k), 3*(21-k)+3), k = 1..nlevels. */
int pcv_chain_keys(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, int nlevels,
                   uint64_t* keys /* same memory space as points */);

/* Multi-GPU routing (skew remedy): bucket[i] = 8 * d1 + d2, the level-1 and level-2 octant digits of
 * point i along the same quantise->decode chain K2 follows (ChildIndex::from_bounding_cube node.rs:34-42 against the
 * GLOBAL root cube, then against the level-1 cube after one encode/decode step); counts[b] = points in bucket b.
 * The ranks all-reduce the 64 counts, decide which level-1 nodes the global tree splits, and bin-pack the buckets
 * (whole octants where the level-1 node stays a leaf) onto ranks. Device-resident points only; bucket is a device
 * buffer of n u32, counts a host array of 64 entries. */
typedef struct pcv_route_state {  /* optional outputs of pcv_route_buckets: the level-1 chain state of every point */
  uint32_t* cx;                  /* device, n x u32: Float32 bit patterns of the level-1 codes */
  uint32_t* cy;
  uint32_t* cz;
  uint32_t* oct_rgb;             /* device, n x u32: level-1 digit | r << 8 | g << 16 | b << 24 (needs points->color) */
} pcv_route_state;
int pcv_route_buckets(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, uint32_t* bucket,
                      uint64_t counts[64], const pcv_route_state* state /* nullable; needs a Float32-encoded level 1 */);

/* The same routing in two passes that never write the level-1 state in input order (69 instead of 87 bytes of traffic per
 * point; a Float32-encoded level 1 is required, as for pcv_route_state):
 *   pcv_route_plan     bucket BYTE of every point (device, n bytes), the bucket histogram of every tile of 4 096 points
 *                      (device, pcv_route_tiles(n) x 64 x u16) and the 64 counts the ranks all-gather;
 *   pcv_route_scatter  once the plan (bucket -> owning rank) is known: the level-1 state of every point — the four planes of
 *                      pcv_route_state, plus points->intensity when set — computed from the coordinates again and written
 *                      straight to the point's place in its owner's buffer: row k (in input order) of the rows owned by rank
 *                      r goes to row k of dst[r]'s planes. Replaces ChildIndex::from_bounding_cube (node.rs:34-42) + the
 *                      first encode step (codec.rs:102-121) of generation.rs:78-99 for the multi-GPU exchange. */
/* pcv_route_plan, params->flags: ownership goes by ROOT OCTANT (BASELINE north_star: shard by the top-3-bit prefix) — the
 * bucket of a point is its level-1 digit alone (bucket = d1 << 3, the counts of the other buckets are 0): three comparisons
 * against the root cube's centre per point (node.rs:34-42) instead of a level step of the chain. pcv_route_scatter is the same. */
#define PCV_ROUTE_OCTANTS_ONLY 64u
typedef struct pcv_route_dst {
  uint32_t* oct_rgb;
  uint32_t* cx;
  uint32_t* cy;
  uint32_t* cz;
  float* intensity; /* nullable */
} pcv_route_dst;
uint64_t pcv_route_tiles(uint64_t n);
int pcv_route_plan(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, uint8_t* bucket, uint16_t* tile_hist,
                   uint64_t counts[64]);
int pcv_route_scatter(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, const uint8_t* bucket,
                      const uint16_t* tile_hist, uint32_t world, const uint8_t rank_of_bucket[64], const pcv_route_dst* dst /* [world] */);

/* Stable partition of up to 8 row-aligned planes by owner (owner[i] is a rank, or a bucket when rank_of_bucket maps the
 * 64 buckets to ranks): row k (in input order) of the rows owned by rank r goes to row k of dst[r * nplanes + p] for
 * every plane p. The caller points dst[r * nplanes + p] at its send buffer for rank r, and the own rank's entries
 * straight at the receive buffer. All pointers are device pointers; rows are 1..16 bytes. */
typedef struct pcv_plane {
  const void* src;
  uint32_t elem_bytes;
} pcv_plane;
int pcv_partition_by_owner(pcv_ctx* ctx, uint64_t n, const uint32_t* owner, uint32_t world,
                           const uint8_t* rank_of_bucket /* nullable host array of 64 */, uint32_t nplanes,
                           const pcv_plane* planes, void* const* dst /* [world][nplanes] */);

/* K4: the octree topology from SORTED path keys (split / should_split_node / split_node, generation.rs:58-193): a child
 * exists iff a key carries its prefix, a child is split iff count > max_points_per_node && child edge > resolution,
 * the root is always split. keys: pcv_chain_keys layout, ascending, full depth of params' level table (<= 21 levels).
 * nodes come back breadth first (level-major, prefix order inside a level), the children of a node consecutive in digit
 * order. *num_nodes may exceed `capacity`: only the first `capacity` are written. PCV_E_DEPTH: a node at the last key
 * level would still have to be split. */
typedef struct pcv_split_node {
  uint64_t id_high, id_low; /* NodeId halves (node.rs:101-111) */
  uint64_t first, count;    /* the subtree's points: a contiguous range of the key-sorted order */
  uint32_t level;
  uint32_t parent;          /* index in this table, 0xffffffff for the root */
  uint32_t first_child;     /* index of the first child (inner nodes) */
  uint32_t child_mask;      /* bit c: child c exists */
  uint32_t is_leaf;
  uint32_t reserved;
} pcv_split_node;
int pcv_node_split(pcv_ctx* ctx, const pcv_build_params* params, const uint64_t* sorted_keys, uint64_t n, int mem,
                   pcv_split_node* nodes, uint64_t capacity, uint64_t* num_nodes);

/* K5 (table part): the closed form of subsample_children_into (generation.rs:195-253, 335-387) on a node
 * table: stream_len = |pre(node)| (leaves: their points; inner: sum over children of ceil(|pre(child)| / 8)),
 * num_points = what the node keeps (root: everything it receives; others: |pre| - ceil(|pre| / 8)), child_offset =
 * where the node's promoted block starts inside its parent's stream. With node_of_slot / slot_in_node (nullable, n
 * entries): the final home of the record at every position of the leaf-sorted order — it climbs while its position j in
 * the current stream is a multiple of 8 (j' = child_offset + j / 8), otherwise it settles at slot j - j / 8 - 1
 * (the root keeps slot j). Host only. */
typedef struct pcv_promote_node {
  uint64_t stream_len;
  uint64_t num_points;
  uint64_t child_offset;
} pcv_promote_node;
int pcv_promote_assign(const pcv_split_node* nodes, uint64_t num_nodes, pcv_promote_node* per_node, uint64_t n,
                       uint32_t* node_of_slot, uint32_t* slot_in_node);

/* K5 + K6: leaf encode, stable grouping by leaf, promotion and final encode for a GIVEN topology (a node table as
 * pcv_node_split returns it, built for the same points / params): the finished octree, as pcv_build_octree returns it.
 * With pcv_chain_keys + pcv_sort_keys64 + pcv_node_split this is the whole build, stage by stage. */
int pcv_gather_encode(pcv_ctx* ctx, const pcv_build_params* params, const pcv_points* points, const pcv_split_node* nodes,
                      uint64_t num_nodes, pcv_octree** out);

/* K3: stable LSD radix sort of 64-bit keys on bits [begin_bit, end_bit), in place. */
int pcv_sort_keys64(pcv_ctx* ctx, uint64_t* keys, uint64_t n, int begin_bit, int end_bit, int mem);
/* K3: the 32-bit key variant the build uses when ten levels of path digits suffice. */
int pcv_sort_keys32(pcv_ctx* ctx, uint32_t* keys, uint64_t n, int begin_bit, int end_bit, int mem);
/* K3: stable sort of (u32 key, u32 value) pairs on bits [begin_bit, end_bit), in place. */
int pcv_sort_pairs32(pcv_ctx* ctx, uint32_t* keys, uint32_t* values, uint64_t n, int begin_bit, int end_bit,
                     int mem);

/* K3: the stable record sort of the build (leaf rank -> records), on its own. `keys` (n words), the payload and the planes
 * are sorted in place by the rank field of the key; everything else in a record only travels.
 *   record formats
 *     vec_bytes 0:  key + nwords planes (1..8).
 *     vec_bytes 16: key + one 16-byte payload (`vec`: n x 4 words) + nwords planes (0..8): the 20-byte records.
 *     vec_bytes 8:  key = rank << 8 | blue, one 8-byte payload (`vec`: n x 2 words; red | green << 8 in the upper half of the
 *                   second word) + nwords planes (0..8): the 12-byte records of the single-chain build. With at most one
 *                   plane they take the 12-byte record kernels (tiles of 8 192), otherwise the generic ones.
 *   the rank field: bits [8, 8 + key_bits) of the key with vec_bytes 8 (key_bits <= 24), bits [0, key_bits) otherwise
 *     (key_bits <= 32); key_bits >= 1.
 *   map (map_entries words, or null): the keys carry PREDICTED ranks < map_entries (needs a payload: vec_bytes 8 or 16); the
 *     sort's first pass replaces each by map[rank] & 0x3fffffff, which must be < 2^key_bits, and where map[rank] has bit 30 set
 *     (the replay mark) the record's first payload word becomes its input index. A map of <= 16 384 entries (10 000 / 5 000
 *     with a plane and digits of <= 7 / 8 bits) travels as half words in LDS when rows are given: key_bits <= 15 then.
 *   rows (map, 12-byte records with at most one plane): per sort workgroup g of pcv_sort_rec12_geometry the number of keys
 *     of chunk g with predicted rank b, rows[g * map_entries + b]. PCV_SORT_ROWS_GIVEN: the caller's, groups x map_entries
 *     words; PCV_SORT_ROWS_DEVICE: counted on the device as the build does, and copied to `rows` where that is not null.
 *   plane0_in (nwords >= 1, or null): the first pass reads plane 0 from this array, which is left as it is; planes[0]
 *     only receives the sorted plane.
 *   color_in (rows, or null): the keys arrive as rank << 8 and the upper half of the payload's second word empty; the first
 *     pass reads red, green, blue of record i at color_in + i * color_stride (3 or 4; n * color_stride bytes in all).
 *   flags & PCV_SORT_RECORDS_PACKED (vec_bytes 8, no plane, map of <= 65 536 entries, rows, color_in): the records arrive as
 *     the chain pass of the build hands them over — `vec` holds 8 bytes per record, first word as above, second word = third
 *     code | predicted rank << 16 — and there are no keys to read: `keys` only receives the sorted keys. On input its first
 *     2 n bytes hold the predicted ranks once more as half words, which PCV_SORT_ROWS_DEVICE counts (nothing else reads them).
 *     The first pass loads 8 bytes per record, joins the colour and writes the 12-byte records every later stage reads. The
 *     map stays in LDS up to 15 824 / 11 216 entries (digits of <= 7 / 8 bits; 11 728 / 7 120 at color_stride 4).
 *   hold_second: the sort gets a place to hold its second pass back in (the two-pass rows form does), and the entry then runs
 *     that pass in its plain form, as pcv_build_finish does for leaves the pass does not settle itself.
 *   flags & PCV_SORT_RECORDS_CHECK_KEYS: every predicted rank is compared with map_entries first (a pass of its own; a
 *     device array is copied to the host for it). Without it a rank outside the map reads outside the map.
 * `plan` (nullable) receives what the sort launched: the values of PcvSortHist / PcvSortDown of csrc/pcv_sort_plan.h.
 * PCV_E_INVALID (nothing is touched): null arrays, nwords > 8, a shape outside the list above, what the plan refuses. */
#define PCV_SORT_ROWS_NONE 0
#define PCV_SORT_ROWS_GIVEN 1
#define PCV_SORT_ROWS_DEVICE 2
#define PCV_SORT_RECORDS_CHECK_KEYS 1u
#define PCV_SORT_RECORDS_PACKED 2u
typedef struct pcv_sort_records_args {
  uint64_t n;
  uint32_t* keys;
  void* vec;
  uint32_t* planes[8];
  const uint32_t* plane0_in;
  const uint8_t* color_in;
  const uint32_t* map;
  uint32_t* rows;
  int32_t key_bits;
  int32_t vec_bytes;
  int32_t nwords;
  uint32_t color_stride;
  uint32_t map_entries;
  int32_t rows_mode;
  int32_t hold_second;
  int32_t mem;
  uint32_t flags;
  uint32_t reserved;
} pcv_sort_records_args;
typedef struct pcv_sort_pass_info {
  int32_t shift, nbits;
  int32_t hist, down;   /* PcvSortHist, PcvSortDown */
  int32_t R, MAP, PL;   /* 12-byte record kernels: digit values, the map's place (0 none, 1 LDS, 2 global memory), the plane */
  int32_t map_lds;      /* a counting pass that applies the map: the map in LDS */
  uint64_t dyn_lds;
} pcv_sort_pass_info;
typedef struct pcv_sort_plan_info {
  int32_t npasses;
  int32_t two_pass, held_back; /* the two-pass rows form; its second pass was left to the caller of the sort */
  int32_t pieces, blocks, gpb;
  int32_t groups;              /* geom.groups, geom.chunk */
  int32_t second_ran;          /* the entry ran the held-back pass */
  uint64_t chunk;
  pcv_sort_pass_info pass[8];
} pcv_sort_plan_info;
int pcv_sort_records(pcv_ctx* ctx, const pcv_sort_records_args* args, pcv_sort_plan_info* plan);
/* groups and chunk of the 12-byte record sort of n records (the shape of `rows`). */
void pcv_sort_records_geometry(uint64_t n, int32_t* groups, uint64_t* chunk);

/* Device self-test of the exact constant-divisor division used by the chain kernels (see pcv_chain_dev.h):
 * compares it bit-for-bit with IEEE f64 division for every integer code / 255 and / 65535 and for
 * samples_per_divisor pseudo-random numerators per divisor; *mismatches must come back 0. */
int pcv_selftest_division(pcv_ctx* ctx, const double* divisors, int ndiv, uint64_t samples_per_divisor,
                          uint64_t* mismatches);

/* ---- PLY ingest (host side) --------------------------------------------------------- */
/* Replaces PlyIterator (src/read_write/ply.rs:328-556): binary little-endian PLY, element `vertex` first; x/y/z of
 * any scalar type cast to f64 plus the header's `comment offset: x y z`; red/green/blue (uchar) -> colour;
 * `intensity` (float) kept; alpha and all other properties skipped. One pass; the arrays can go straight into
 * pcv_build_octree with PCV_BUILD_COMPUTE_BBOX (== build_octree_from_file, generation.rs:272-287).
 * `err` (nullable) receives a message on failure. */
typedef struct pcv_ply pcv_ply;
int pcv_ply_read(const char* path, pcv_ply** out, char* err, uint64_t errcap);
uint64_t pcv_ply_num_points(const pcv_ply* ply);
/* Fills `out` with host pointers owned by `ply` (color / intensity are NULL when the file has none). */
int pcv_ply_points(const pcv_ply* ply, pcv_points* out);
void pcv_ply_free(pcv_ply* ply);
/* 64-bit integer properties (longlong | int64 | ulonglong | uint64) are 8 bytes wide here — a departure: the reference
 * advances 4 bytes for them (ply.rs:262-267) and so cannot read the files its own writer makes. As the type of x / y / z they
 * stay refused. pcv_ply_read skips them by stride, as does pcv_build_octree_from_ply.
 * pcv_ply_read_ex with PCV_PLY_READ_EXTRAS also keeps every other scalar vertex property as an extra attribute of its own
 * type (pcv_ply_attributes: host columns owned by `ply`, in file order, as pcv_s2_split_ex takes them). All ten scalar types
 * come back; the reference keeps u8, i64, u64, f32, f64 and silently drops the rest (ply.rs:427-434). Never extras: x, y, z,
 * the colour properties (red | r, green | g, blue | b, and alpha | a, which is dropped), `intensity` when it is float (it is
 * the intensity column). Skipped, not errors: a name that ends in an ASCII digit (one component of a vector attribute, which
 * the reference's reader panics on, ply.rs:388), a name that breaks the rules for extras below, a name that
 * occurs twice, and whatever comes after the PCV_S2_MAX_EXTRAS-th extra. With flags == 0 it is pcv_ply_read. */
#define PCV_PLY_READ_EXTRAS 1u
int pcv_ply_read_ex(const char* path, uint32_t flags, pcv_ply** out, char* err, uint64_t errcap);
struct pcv_attribute;
int pcv_ply_attributes(const pcv_ply* ply, uint32_t* count, struct pcv_attribute* out /* nullable; PCV_S2_MAX_EXTRAS entries */);
/* build_octree_from_file (src/octree/generation.rs:272-287) with the decode on the device: the vertex records of the
 * file go up as they are (15 bytes per point for float x y z + uchar r g b instead of the 27 of f64 SoA arrays), one HIP
 * kernel casts x / y / z to f64 and adds the header offset like ply.rs:488-493, then the build runs with
 * PCV_BUILD_COMPUTE_BBOX (params->bbox_* are ignored). Same files as pcv_ply_read + pcv_build_octree; the PLY must
 * have colour, and `intensity` (float) when with_intensity != 0. */
int pcv_build_octree_from_ply(pcv_ctx* ctx, const pcv_build_params* params, const char* path, int with_intensity,
                              pcv_octree** out);

/* ---- octree loading (viewer side) ------------------------------------------------------------ */
/* Replaces Octree::from_data_provider over an OnDiskDataProvider (src/octree/mod.rs:156-215,
 * src/data_provider/on_disk.rs): parses meta.pb — versions 9..13 like the reference (9-11: top-level
 * deprecated_resolution / deprecated_nodes, Vector3f boxes and level/index NodeIds where present; 12: the box inside
 * OctreeMeta; 13: current), anything else is InvalidVersion — and derives every node's bounding cube
 * (NodeId::find_bounding_cube). Node files are read on demand by pcv_octree_node_data; the first point query
 * (pcv_query_points / pcv_cull_node_points) reads all node files once and keeps them device resident. */
int pcv_octree_open_dir(pcv_ctx* ctx, const char* directory, pcv_octree** out);

/* ---- queries: batched transform-and-cull ------------------------------------------------------ */
/* PointLocation variants (src/iterator.rs:12-20) that the octree path supports. params layout:
 *   PCV_SHAPE_ALL                   -                                          AllPoints
 *   PCV_SHAPE_AABB                  min xyz, max xyz                           geometry::Aabb
 *   PCV_SHAPE_FRUSTUM               clip_from_query (16, nalgebra memory order = column-major); the inverse is
 *                                   computed like Frustum::from_matrix4 (src/geometry/frustum.rs:111-117)
 *   PCV_SHAPE_FRUSTUM_WITH_INVERSE  clip_from_query (16) then query_from_clip (16), as Frustum::new stores them
 *                                   (frustum.rs:101-108)
 *   PCV_SHAPE_OBB                   query_from_obb isometry: translation xyz, unit quaternion i j k w; then the
 *                                   half extent xyz (src/geometry/obb.rs:13-45)
 *   PCV_SHAPE_WEB_MERCATOR_RECT     north_west.normalized (x, y) then south_east.normalized (x, y), each in [0, 1): the
 *                                   fields of geometry::WebMercatorRect (src/geometry/web_mercator_rect.rs:30-33); make
 *                                   them with pcv_wmr_from_zoomed. The query space is ECEF. pcv_shapes_create takes the
 *                                   four doubles as given, like the other kinds' parameters: it does not repeat the
 *                                   constructor's checks (NaN or inverted bounds give a shape that contains nothing).
 *   PCV_SHAPE_S2_CELL_UNION         -  (no params)                             PointLocation::S2Cells(CellUnion): `reserved`
 *                                   is the index of the shape's union among the unions handed to pcv_shapes_create_ex. The
 *                                   query space is ECEF.
 *   PCV_SHAPE_POLYGON               z_min, z_max, frame                        a polygon with holes, or several polygons, under
 *                                   the even-odd rule: `reserved` is the index of the shape's polygon among those handed to
 *                                   pcv_shapes_create_ex2, given as rings of (x, y) vertices, each ring implicitly closed.
 *                                   frame 0 (xy): the vertices are in the cloud's own x and y and the location is the prism
 *                                   polygon x [z_min, z_max], closed; either bound may be -inf / +inf, and z_min > z_max or a
 *                                   NaN bound contains nothing. frame 1 (web-mercator): the vertices are normalized
 *                                   web-mercator coordinates in [0, 1) as PCV_SHAPE_WEB_MERCATOR_RECT's, the query space is
 *                                   ECEF, z_min and z_max must be -inf and +inf, and nothing wraps across x = 0.
 *                                   Every other kind ignores `reserved`. */
#define PCV_SHAPE_ALL 0
#define PCV_SHAPE_AABB 1
#define PCV_SHAPE_FRUSTUM 2
#define PCV_SHAPE_OBB 3
#define PCV_SHAPE_FRUSTUM_WITH_INVERSE 4
#define PCV_SHAPE_WEB_MERCATOR_RECT 5
#define PCV_SHAPE_S2_CELL_UNION 6
#define PCV_SHAPE_POLYGON 7
typedef struct pcv_shape {
  int32_t kind;
  int32_t reserved; /* PCV_SHAPE_S2_CELL_UNION: index of the shape's union (pcv_shapes_create_ex); PCV_SHAPE_POLYGON: index of
                     * the shape's polygon (pcv_shapes_create_ex2); otherwise unused */
  double params[32];
} pcv_shape;
typedef struct pcv_shapes pcv_shapes;

/* Relation (src/math/sat.rs:37-45) */
#define PCV_REL_IN 0
#define PCV_REL_CROSS 1
#define PCV_REL_OUT 2

/* Q1: prepares `count` shapes on the device: corners, unique edges / face normals and the deduplicated
 * separating axes against AABBs (Intersector::cache_separating_axes_for_aabb, src/math/sat.rs:111-143). */
int pcv_shapes_create(pcv_ctx* ctx, const pcv_shape* shapes, uint32_t count, pcv_shapes** out);
/* The same with cell unions as locations over the octree (PointLocation::S2Cells; HasAabbIntersector for CellUnion,
 * src/geometry/s2_cell_union.rs). The unions are given as pcv_s2_cells_in_location takes them: host memory, union u's
 * cells union_cells[union_first[u] .. union_first[u + 1]), ascending, union_first[0] == 0; they are taken as given, not
 * normalized. A shape of kind PCV_SHAPE_S2_CELL_UNION names its union by `reserved`; unions and the other kinds mix in any
 * order, a union may be named by several shapes or by none, and an empty union is valid and contains nothing.
 * PCV_E_INVALID with pcv_s2_cells_in_location's messages for malformed unions, "union index out of range", and "a union
 * with a level-0 cell has no geometry" (Cell::rect_bound of a face is not provided). pcv_shapes_create itself refuses the
 * kind. Meaning over an octree: a node is listed and descended into iff the rect bound of the normalized leaf cells of its
 * bounding cube's 8 corners intersects a cell of the union (Rect::intersects_cell; the reference's misses, such as a corner
 * rect that does not cover its cube, included); a point is kept iff CellUnion::contains_cellid(CellID::from_point(p)) of
 * its decoded position, then the interval. pcv_nodes_in_location, pcv_cull_points, pcv_cull_node_points, pcv_query_points,
 * pcv_query_node_points and pcv_query_batch_run take such shapes; pcv_cull_nodes, pcv_cull_nodes_sparse and
 * pcv_visible_nodes refuse a table that holds one (a union has no Relation and no clip matrix), naming the first.
 * pcv_s2_cells_in_location, pcv_s2_query_run (and through it pcv_xray_run_s2's queries) treat a union member of the table
 * as the union location it is, at the shape's slot: CellUnion::intersects_cellid for the cells, contains_cellid per point. */
int pcv_shapes_create_ex(pcv_ctx* ctx, const pcv_shape* shapes, uint32_t count, uint32_t num_unions, const uint32_t* union_first,
                         const uint64_t* union_cells, pcv_shapes** out);
/* The cells of shape i, a PCV_SHAPE_S2_CELL_UNION: *num_cells is the union's length, of which the first
 * min(length, capacity) are written to `cells` (nullable with capacity 0). PCV_E_INVALID for any other kind. */
int pcv_shapes_union(pcv_shapes* shapes, uint32_t i, uint64_t capacity, uint64_t* cells, uint32_t* num_cells);
/* The same with polygons as locations (PCV_SHAPE_POLYGON). The unions are taken as pcv_shapes_create_ex takes them. The
 * polygons are host memory: polygon p's rings are polygon_first[p] .. polygon_first[p + 1], ring r's vertices
 * ring_first[r] .. ring_first[r + 1], `vertices` holds x, y pairs; polygon_first[0] == ring_first[0] == 0. Polygons mix with the
 * other six kinds in any order; a polygon may be named by several shapes or by none. pcv_shapes_create and
 * pcv_shapes_create_ex refuse the kind. PCV_E_INVALID with a message for: a polygon without a ring, a ring with fewer than 3
 * vertices, a vertex that is not finite, more than 65 535 vertices in one polygon, "polygon index out of range", a frame other
 * than 0 or 1, and in frame 1 a vertex outside [0, 1) or a z range other than -inf, +inf.
 *
 * The point rule. Per polygon an edge table is built once: horizontal edges are dropped; every other edge is stored from its
 * lower endpoint (lx, ly) to its upper (ux, uy), ly < uy, with slope = (ux - lx) / (uy - ly), one rounded f64 division.
 * inside(px, py) is the parity of the number of edges with ly <= py && py < uy && px < lx + (py - ly) * slope (product and
 * sum rounded separately). Two polygons that share an edge evaluate it identically whatever their orientation, so polygons
 * that tile a region keep every point in exactly one of them. A point is kept iff inside(x, y) && z_min <= z && z <= z_max of
 * its decoded f64 position (frame 0), or inside of its normalized projection, the chain pcv_wmr_project runs (frame 1); then
 * the interval.
 * The node rule, frame 0. For a node cube (min, edge) with hi = min + edge per axis: listed and descended into iff
 * z_min <= hi.z && z_max >= min.z, and inside(min.x, min.y) or some edge (horizontal ones included) hits the square
 * [min.x, hi.x] x [min.y, hi.y]: the edge's bounding interval overlaps the square's in x and in y, and the four corners'
 * side = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) are neither all > 0 nor all < 0. A polygon has no Relation.
 * The node and cell rule, frame 1: the node list over an octree and the cell list over an S2 cell cloud are those of the
 * PCV_SHAPE_WEB_MERCATOR_RECT (min x, min y), (max x, max y) over the polygon's vertices.
 * pcv_nodes_in_location, pcv_cull_points, pcv_cull_node_points, pcv_query_points, pcv_query_node_points and
 * pcv_query_batch_run (and what reads its batches: PLY output, terrain layers) take such shapes; pcv_s2_cells_in_location and
 * pcv_s2_query_run[_ex] take frame 1 and refuse frame 0 ("a polygon in the xy frame has no meaning over an ECEF cell cloud");
 * pcv_cull_nodes, pcv_cull_nodes_sparse and pcv_visible_nodes refuse a table that holds one, naming the first. */
int pcv_shapes_create_ex2(pcv_ctx* ctx, const pcv_shape* shapes, uint32_t count, uint32_t num_unions, const uint32_t* union_first,
                          const uint64_t* union_cells, uint32_t num_polygons, const uint32_t* polygon_first, const uint32_t* ring_first,
                          const double* vertices, pcv_shapes** out);
/* The rings of shape i, a PCV_SHAPE_POLYGON: *num_rings and *num_vertices are its counts; when ring_capacity >= *num_rings
 * and vertex_capacity >= *num_vertices (and ring_capacity > 0), ring_first receives *num_rings + 1 offsets from 0 and
 * `vertices` the x, y pairs, as given. PCV_E_INVALID for any other kind. */
int pcv_shapes_polygon(pcv_shapes* shapes, uint32_t i, uint32_t ring_capacity, uint32_t* ring_first, uint32_t* num_rings,
                       uint32_t vertex_capacity, double* vertices, uint32_t* num_vertices);
/* Host twins of the polygon rules (no device, no context; messages through pcv_host_last_error): one polygon as num_rings rings,
 * ring_first[0] == 0. _check_host: the validation above. _contains_host: the keep flag of n points in either frame, bit for
 * bit the device's. _intersects_cubes_host: the node rule of frame 0 for m cubes (m x 4: min xyz, edge). */
int pcv_polygon_check_host(uint32_t num_rings, const uint32_t* ring_first, const double* vertices, int32_t frame, double z_min, double z_max);
int pcv_polygon_contains_host(uint32_t num_rings, const uint32_t* ring_first, const double* vertices, int32_t frame, double z_min,
                              double z_max, uint64_t n, const double* x, const double* y, const double* z, uint8_t* keep);
int pcv_polygon_intersects_cubes_host(uint32_t num_rings, const uint32_t* ring_first, const double* vertices, double z_min, double z_max,
                                      uint64_t m, const double* cubes, uint8_t* intersects);
void pcv_shapes_free(pcv_shapes* shapes);
uint32_t pcv_shapes_count(const pcv_shapes* shapes);
/* Inspect one prepared shape (tests): 8 corners, up to 26 axes. valid == 0: the matrix is not invertible. PCV_E_INVALID for
 * a shape with more than 26 axes (a web-mercator rectangle may have up to 45): use pcv_shapes_get_ex. Both calls are
 * PCV_E_INVALID for a cell union, which has neither corners nor axes: pcv_shapes_union gives its cells; and for a polygon:
 * pcv_shapes_polygon gives its rings. */
int pcv_shapes_get(pcv_shapes* shapes, uint32_t i, double corners[24], double axes[78], uint32_t* num_axes, int* valid);
/* The same for any shape: `axes` holds 3 * axes_capacity doubles (PCV_MAX_SHAPE_AXES always suffices); *num_axes is the
 * shape's count, of which the first min(count, axes_capacity) are written. */
#define PCV_MAX_SHAPE_AXES 45
int pcv_shapes_get_ex(pcv_shapes* shapes, uint32_t i, double corners[24], double* axes, uint32_t axes_capacity,
                      uint32_t* num_axes, int* valid);

/* ---- web-mercator rectangles: host-only helpers (no device, no context) ------------------------------------------ */
/* WebMercatorRect::from_zoomed_coordinates (src/geometry/web_mercator_rect.rs:40-53, src/math/web_mercator.rs:84-97):
 * min / max are (x, y) map coordinates at zoom z, in [0, 256 * 2^z). PCV_E_INVALID where the reference returns None:
 * z > 23, a coordinate out of range, (max - min) / 2^z wider than 1 in x (after rem_euclid(256): x may wrap) or outside
 * [0, 1] in y. params receives the shape's four doubles. A rectangle that wraps in x (nw.x > se.x) is accepted and then
 * contains no point — the reference's behaviour (web_mercator_rect.rs:121-127). */
int pcv_wmr_from_zoomed(const double min[2], const double max[2], uint32_t z, double params[4]);
/* ConvexPolyhedron::compute_corners (web_mercator_rect.rs:61-83): to_lat_lng of both coordinates (web_mercator.rs:55-64,
 * both clamps), then WGS84 -> ECEF at -500 m and 10 000 m: NW NE SE SW down, NW NE SE SW up. Uses the host's libm. */
int pcv_wmr_corners(const double params[4], double corners[24]);
/* PointCulling::contains (web_mercator_rect.rs:121-127) on the host, point by point: ECEF -> WGS84,
 * WebMercatorCoord::from_lat_lng (web_mercator.rs:38-50), then nw.x <= u && nw.y <= v && u < se.x && v < se.y.
 * pcv_wmr_project hands out (u, v). The device's keep flag of every point query equals pcv_wmr_contains bit for bit: both
 * run the same arithmetic (no libm on either side). */
int pcv_wmr_project(uint64_t n, const double* x, const double* y, const double* z, double* u, double* v);
int pcv_wmr_contains(const double params[4], uint64_t n, const double* x, const double* y, const double* z, uint8_t* keep);
/* TEST HOOKS, not part of the query interface (the suite restates the reference's unit tests and measures the chain's
 * transcendentals through them): WebMercatorCoord::from_lat_lng (web_mercator.rs:38-50; radians) with the library's own
 * sin / ln, to_lat_lng (web_mercator.rs:55-64) with libm, as pcv_wmr_corners uses it, and pcv_wmr_math below. */
int pcv_wmr_from_lat_lng(uint64_t n, const double* lat, const double* lng, double* u, double* v);
int pcv_wmr_to_lat_lng(uint64_t n, const double* u, const double* v, double* lat, double* lng);
/* (test hook) The transcendentals of the per-point chain: out = atan2(a, b); out = sin a, out2 = cos a; out = ln a. */
#define PCV_WMR_FN_ATAN2 0
#define PCV_WMR_FN_SINCOS 1
#define PCV_WMR_FN_LN 2
int pcv_wmr_math(int fn, uint64_t n, const double* a, const double* b, double* out, double* out2);

/* Q2: Relation of every node cube against every shape (CachedAxesIntersector::intersect, sat.rs:167-194), row
 * major [shape][node] (node order as pcv_octree_node), host buffers. size_on_screen (nullable, same shape) is
 * relative_size_on_screen (src/octree/mod.rs:119-139) for the shape's clip_from_query; NaN where w == 0 — so NaN for
 * every shape without a clip matrix (Aabb, Obb, web-mercator rectangle). */
int pcv_cull_nodes(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, uint8_t* relation, double* size_on_screen);
/* Q2 as a list per shape (round 5): the nodes whose Relation is not Out (sat.rs:174-194), in node order —
 * node_indices / relation / size_on_screen are [shape][capacity] host arrays, counts[shape] the number of such nodes
 * (entries past `capacity` are dropped, the count is not). size_on_screen (nullable) is relative_size_on_screen
 * (octree/mod.rs:119-139), computed for the listed nodes only — the nodes the reference projects (octree/mod.rs:261-272).
 * The same Relations as pcv_cull_nodes without its shapes x nodes matrix (config 4: 60.7 M pairs, 0.24 % not Out).
 * Round 6: found by a walk down the tree, like the reference's own traversals (octree_iterator.rs:30-43) — a subtree is
 * skipped only under a node that is Out by a margin far above the rounding error of its descendants' bounds, and any shape
 * that meets an Out node without that margin is evaluated flat: the lists equal pcv_cull_nodes' rows in every case. */
int pcv_cull_nodes_sparse(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, uint32_t capacity, uint32_t* counts,
                          uint32_t* node_indices, uint8_t* relation, double* size_on_screen);

/* Q3: Octree::get_visible_nodes (src/octree/mod.rs:228-283) for every frustum: node indices in the order the
 * reference's BinaryHeap pops them. counts[f] = number of visible nodes (may exceed `capacity`; only the first
 * min(counts[f], capacity) entries of node_indices[f * capacity ..] are meaningful, the rest of the row is unspecified;
 * capacity 0 writes no list, node_indices may be NULL). status[f]: 0 ok; 1 matrix not invertible (the reference panics
 * before the traversal; counts[f] = 0); 2 the traversal pushed a node with a projected corner at w == 0 (the reference
 * panics at that push: a node that is Out or not in the tree is never projected). With status 2 the traversal stops
 * there: counts[f] and the list are the nodes with points popped until then, the one whose child panicked included.
 * The reference returns nothing in either case: where status[f] != 0 the list is not a visible-node list and must not
 * be drawn. */
int pcv_visible_nodes(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, uint32_t capacity, uint32_t* counts,
                      uint32_t* node_indices, int32_t* status);
/* PointCloud::nodes_in_location (src/octree/mod.rs:309-331, src/octree/octree_iterator.rs): breadth-first, a node
 * is reported and descended into iff its cube is not Relation::Out. */
int pcv_nodes_in_location(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, uint32_t capacity, uint32_t* counts,
                          uint32_t* node_indices);

/* Q4: FilteredIterator's keep mask (src/iterator.rs:96-119): shape.contains(p) AND, when `interval` is given,
 * interval[0] <= intensity <= interval[1] (ClosedInterval, src/math/mod.rs:86-88). keep lives where the points live;
 * kept (nullable) receives the number of ones. */
int pcv_cull_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, const pcv_points* points,
                    const double* interval, uint8_t* keep, uint64_t* kept);
/* Same on a built octree's node: positions are decoded on the fly from the node's device-resident bytes
 * (src/read_write/codec.rs:124-139); keep is a host buffer of num_points bytes. */
int pcv_cull_node_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, pcv_octree* tree, uint64_t node,
                         const double* interval, uint8_t* keep, uint64_t* kept);

/* Batched point query — the per-location work of ParallelIterator::try_for_each_batch
 * (src/iterator.rs:255-333): nodes_in_location, then for every reported node the FilteredIterator keep mask on the
 * node's decoded positions, then `retain` — here as a stable compaction in (node traversal order, point order).
 * Outputs (capacity entries each; `mem` says where they live): decoded f64 x/y/z, rgb (3 B per point) and, when
 * non-null and the octree has it, intensity. *count = number of points that passed (may exceed capacity: only the
 * first `capacity` are written). Works on built octrees and on octrees opened with pcv_octree_open_dir (the
 * reference's use: stream_points_for_query_in_node -> points_in_node -> NodeIterator over node files,
 * src/iterator.rs:185-223, src/octree/mod.rs:285-307, src/read_write/node_iterator.rs:24-119). */
int pcv_query_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, pcv_octree* tree, const double* interval,
                     uint64_t capacity, int mem, double* x, double* y, double* z, uint8_t* rgb, float* intensity,
                     uint64_t* count);

/* The same for ONE node: PointCloud::stream_points_for_query_in_node (src/iterator.rs:185-205) — the points of node
 * `node` (index as pcv_octree_node) that pass the shape and the interval, in file order. ParallelIterator hands the nodes
 * of nodes_in_location to its workers one by one; a veneer that keeps that structure calls this per node. */
int pcv_query_node_points(pcv_ctx* ctx, const pcv_shapes* shapes, uint32_t shape_index, pcv_octree* tree, uint64_t node,
                          const double* interval, uint64_t capacity, int mem, double* x, double* y, double* z, uint8_t* rgb,
                          float* intensity, uint64_t* count);

/* Point queries of MANY locations over one octree in one run: what ParallelIterator does per
 * location, for S shapes at once, with the result kept on the device as a segment table. One segment per (shape, node
 * that pcv_nodes_in_location reports for it), in that list's order, shapes one after another — nodes without points and
 * nodes where nothing passes included; a frustum whose matrix is not invertible has none. Segment k holds exactly the
 * points pcv_query_node_points(shape, node, interval) returns, so a shape's segments, concatenated, are its
 * pcv_query_points result.
 *   intervals      nullable: 2 x S doubles (lo, hi), the ClosedInterval on intensity of each shape;
 *   interval_used  nullable: S flags, which shapes the interval applies to (NULL with intervals != NULL: all).
 * An interval on an octree without intensity is PCV_E_INVALID. `shapes` may be freed after the run; `tree` must outlive
 * the batch (pcv_query_batch_points reads its device blobs); pcv_query_batch_free touches neither. A failed run frees
 * what it allocated. Works on built octrees and on octrees opened with pcv_octree_open_dir. */
typedef struct pcv_query_batch pcv_query_batch;
int pcv_query_batch_run(pcv_ctx* ctx, const pcv_shapes* shapes, pcv_octree* tree, const double* intervals,
                        const uint8_t* interval_used, pcv_query_batch** out);
int pcv_query_batch_sizes(const pcv_query_batch* b, uint64_t* num_segments, uint64_t* num_points);
/* Host arrays, each nullable: shape s's segments are shape_first_segment[s] .. shape_first_segment[s + 1] (S + 1 entries),
 * segment_node[k] the node index (num_segments entries), segment_offset[k] its first point, a u64 exclusive scan over all
 * segments (num_segments + 1 entries; the last is num_points). */
int pcv_query_batch_segments(const pcv_query_batch* b, uint64_t* shape_first_segment, uint32_t* segment_node,
                             uint64_t* segment_offset);
/* The points of segments [first_segment, first_segment + num_segments): decoded f64 x/y/z, rgb (3 B per point) and, when
 * non-null and the octree has it, intensity, into buffers of `capacity` points that live where `mem` says. A range past
 * the end or with more than `capacity` points is PCV_E_INVALID and writes nothing. */
int pcv_query_batch_points(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, uint64_t capacity, int mem,
                           double* x, double* y, double* z, uint8_t* rgb, float* intensity);
void pcv_query_batch_free(pcv_query_batch* b);

/* ---- xray leaf tiles (xray/src/generation.rs) ----------------------------------------------------------------------
 * The leaf level of build_xray_quadtree (:557-600) for one octree: the quadtree geometry on the host, one point query per
 * leaf tile through pcv_query_batch_run, and the points rasterised on the device into RGBA8 tiles that stay there. */
#define PCV_XRAY_XRAY 0          /* XRayColoringStrategy (:159-199): distinct z buckets per pixel */
#define PCV_XRAY_COLORED 1       /* PointColorColoringStrategy without binning (:294-345) */
#define PCV_XRAY_HEIGHT_STDDEV 2 /* HeightStddevColoringStrategy (:365-408) */
#define PCV_XRAY_COLORED_WITH_INTENSITY 3 /* IntensityColoringStrategy (:210-292): only through pcv_xray_run_ex */
#define PCV_XRAY_JET 0           /* colormap.rs Jet */
#define PCV_XRAY_PURPLISH 1      /* colormap.rs Monochrome(PURPLISH) */
#define PCV_XRAY_BG_WHITE 0      /* TileBackgroundColorArgument (:46-55) */
#define PCV_XRAY_BG_TRANSPARENT 1

/* XrayParameters (:452-461) + the coloring strategy. ColoredWithIntensity and binning take the extra pcv_xray_coloring of
 * pcv_xray_run_ex; an octree carries only color and intensity, so interval_attribute is "intensity" or NULL (S2 cell clouds
 * filter and bin on any scalar attribute: pcv_xray_run_s2_ex); several octrees go through pcv_xray_run_many or
 * pcv_xray_run_ex. */
typedef struct pcv_xray_params {
  uint32_t tile_size_px;        /* W = H, 1 ..= 32768 */
  uint32_t strategy;            /* PCV_XRAY_XRAY / _COLORED / _HEIGHT_STDDEV / _COLORED_WITH_INTENSITY (pcv_xray_run_ex only) */
  uint32_t colormap;            /* height_stddev: PCV_XRAY_JET / PCV_XRAY_PURPLISH */
  uint32_t background;          /* PCV_XRAY_BG_WHITE / PCV_XRAY_BG_TRANSPARENT: assign_background_color (:684) */
  double pixel_size_m;
  float max_stddev;             /* height_stddev: > 0 */
  uint32_t root_level;          /* root_node_id (quadtree NodeId): level and index; r = (0, 0) */
  uint64_t root_index;
  int32_t has_query_from_global;
  int32_t reserved;
  double query_from_global[7];  /* Isometry3: translation xyz, unit quaternion ijkw */
  const char* interval_attribute; /* NULL: no filter; "intensity": ClosedInterval [interval[0], interval[1]] on every tile */
  double interval[2];
  uint64_t max_workspace_bytes; /* device workspace of one tile group (records + bucket tables); 0: 2 GiB */
} pcv_xray_params;
typedef struct pcv_xray pcv_xray;

/* Host only, no context: get_bounding_box (:550, Aabb::transform aabb.rs:58-66 with an isometry),
 * find_quadtree_bounding_rect_and_levels (:515), Node::from_node_id_and_root_bounding_rect + get_child
 * (quadtree/src/lib.rs:59-97) and get_nodes_at_level (:534) below (root_level, root_index). rect = min x, min y, edge.
 * *num_leaves = 4^(deepest_level - root_level); the first `capacity` leaves are written in get_nodes_at_level's order:
 * leaf_index (their NodeId index at deepest_level), tile_bbox (6 per leaf: the Aabb of create_leaf_nodes :625-629, min xyz,
 * max xyz) and, with an isometry, query_obb (10 per leaf: Obb::from(tile).transformed(global_from_query) of
 * xray_from_points :470-476 as a pcv_shape OBB: translation, quaternion ijkw, half extent). More than 2^24 leaves, a
 * root_node_id outside the quadtree, tile_size_px == 0 or pixel_size_m <= 0 is PCV_E_INVALID (message in err). */
int pcv_xray_leaf_tiles(uint32_t tile_size_px, double pixel_size_m, const double bbox_min[3], const double bbox_max[3],
                        const double* query_from_global, uint32_t root_level, uint64_t root_index, uint64_t capacity, double rect[3],
                        uint32_t* deepest_level, uint64_t* num_leaves, uint64_t* leaf_index, double* tile_bbox, double* query_obb,
                        char* err, uint64_t errcap);
/* create_leaf_nodes (:618-648) + assign_background_color (:684) for the whole leaf level of `tree` (its meta bounding box).
 * A tile is created iff its query kept a point (xray_from_points :499-501); a created tile whose points all fall outside
 * its image is all background. The images stay on the device. An unknown strategy / colormap / background,
 * max_stddev <= 0, a filter attribute other than "intensity", a filter on an octree without intensity and more than 2^24
 * leaves are PCV_E_INVALID; a tile whose records alone exceed max_workspace_bytes is PCV_E_OOM. */
int pcv_xray_run(pcv_ctx* ctx, pcv_octree* tree, const pcv_xray_params* params, pcv_xray** out);
/* pcv_xray_run over several octrees at once, as build_xray_quadtree runs with several point_cloud_locations
 * (xray/src/build_quadtree.rs:84, :187-196) through one PointCloudClient (point_cloud_client/src/lib.rs). The bounding box
 * is the union of PointCloudClientBuilder::build (:102-125): the first octree's meta box grown by every octree's min and
 * then its max in list order (Aabb::grow), each octree included even where it keeps no point; query_from_global then
 * applies to the union as in pcv_xray_run. Every octree runs the same shape list through pcv_query_batch_run, and a tile
 * is created iff the sum of kept points over the octrees is > 0 (ParallelIterator::try_for_each_batch takes every cloud's
 * jobs, src/iterator.rs:262-270). kept and drawn are sums over the octrees; a created tile's image is the strategy over
 * the union of their kept points: exact for xray and colored, whose colours do not depend on point order, and for
 * height_stddev within the tolerance of pcv_xray_run. Octrees may differ in resolution and encodings, and one may appear
 * more than once. All num_trees query batches are alive at once, with the raster workspace; each raster pass is one
 * launch per tile group whatever num_trees. The result is a pcv_xray like pcv_xray_run's. num_trees == 0 ("No locations
 * specified"), more than PCV_XRAY_MAX_TREES octrees, a null octree, an octree of another context and an intensity filter
 * when some octree has no intensity are PCV_E_INVALID with a message, as are pcv_xray_run's own checks; nothing is
 * allocated then. Out of device memory is PCV_E_OOM with nothing left allocated. */
#define PCV_XRAY_MAX_TREES 4096
int pcv_xray_run_many(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t num_trees, const pcv_xray_params* params, pcv_xray** out);
/* Host only, no context: the parameter checks pcv_xray_run makes before any device work (strategy, colormap,
 * max_stddev, background, filter attribute; tree_has_intensity: whether the octree carries intensity). PCV_E_INVALID
 * with a message in err, or PCV_OK. */
int pcv_xray_check_params(const pcv_xray_params* params, int tree_has_intensity, char* err, uint64_t errcap);
/* What the reference's --coloring-strategy colored_with_intensity and --binning <attr>=<size> add
 * (xray/src/build_quadtree.rs:44-106, :141-158):
 *   min_intensity, max_intensity  IntensityColoringStrategy's min / max: read by PCV_XRAY_COLORED_WITH_INTENSITY only, any
 *                                 f32 (NaN and min > max included: the colour follows Rust's f32 rules, see
 *                                 PCV_XRAY_FN_INTENSITY);
 *   binning_attribute, bin_size   NULL: no binning; "intensity": bin = (intensity as f64 / bin_size) as i64 (Rust `as`:
 *                                 truncating, saturating, NaN -> 0; bin_size is not validated), generation.rs:138-157.
 *                                 Only "intensity" can be binned on here ("color" is a U8Vec3, on which the reference
 *                                 panics, src/attributes.rs:128); pcv_xray_run_s2_ex takes any scalar attribute of S2
 *                                 clouds. Binning applies to PCV_XRAY_COLORED (per pixel: the mean over bins, in
 *                                 ascending bin order, of each bin's mean colour, :294-362) and
 *                                 PCV_XRAY_COLORED_WITH_INTENSITY (the mean over bins of each bin's mean intensity,
 *                                 :210-292); xray and height_stddev never read it (attributes() :133) and their bytes do
 *                                 not change.
 * Both strategies, binned or not, reduce each (pixel, bin) in a fixed key order, so their images do not depend on
 * scheduling, tile grouping or octree order. */
typedef struct pcv_xray_coloring {
  float min_intensity, max_intensity;
  const char* binning_attribute;
  double bin_size;
} pcv_xray_coloring;
/* pcv_xray_run_many with a coloring (nullable: then exactly pcv_xray_run_many). Every octree must carry intensity when
 * the strategy is colored_with_intensity or binning applies. IntensityColoringStrategy stops processing a PointsBatch
 * at its first intensity < 0 (generation.rs:248), and the reference's batch boundaries depend on thread scheduling, so a
 * tile that keeps a negative intensity has no defined reference image: here such a tile is drawn from its points with
 * intensity >= 0 (NaN included, as NaN < 0 is false); the negative points are neither drawn nor counted in drawn, and
 * pcv_xray_negative reports how many there were. */
int pcv_xray_run_ex(pcv_ctx* ctx, pcv_octree* const* trees, uint32_t num_trees, const pcv_xray_params* params,
                    const pcv_xray_coloring* coloring, pcv_xray** out);
/* pcv_xray_check_params with a coloring (nullable): strategy colored_with_intensity needs one; a binning attribute other
 * than "intensity" is PCV_E_INVALID for every strategy; binning with colored / colored_with_intensity and
 * colored_with_intensity itself need tree_has_intensity. pcv_xray_run, pcv_xray_run_many and pcv_xray_check_params
 * refuse colored_with_intensity (it needs the coloring of the _ex entry points). */
int pcv_xray_check_params_ex(const pcv_xray_params* params, const pcv_xray_coloring* coloring, int tree_has_intensity, char* err,
                             uint64_t errcap);
/* Per created tile: the kept points with intensity < 0 (colored_with_intensity only; 0 elsewhere), counted over every kept
 * point of the tile, inside its image or not (:108-127). num_created entries. */
int pcv_xray_negative(const pcv_xray* x, uint64_t* negative);
/* Host only, no context: the tile groups a run makes for created tiles that keep kept[0 .. num_tiles) points, with
 * these params (tile_size_px, strategy, max_workspace_bytes) and coloring (nullable). Consecutive tiles whose records and
 * bucket tables fit max_workspace_bytes form a group; *num_groups is their count and the first `capacity` entries of
 * group_first (nullable) their first tiles. A tile whose records alone exceed the workspace is PCV_E_OOM. A tile of
 * colored_with_intensity or binned colored that keeps more than PCV_XRAY_MAX_SORTED_TILE_POINTS points is PCV_E_INVALID:
 * its one-workgroup sort has u32 indices. The same checks refuse such a run. Message in err. */
#define PCV_XRAY_MAX_SORTED_TILE_POINTS 1073741824ull
int pcv_xray_plan_groups(const uint64_t* kept, uint64_t num_tiles, const pcv_xray_params* params, const pcv_xray_coloring* coloring,
                         uint64_t capacity, uint64_t* num_groups, uint64_t* group_first, char* err, uint64_t errcap);
int pcv_xray_info(const pcv_xray* x, uint32_t* deepest_level, double rect[3], uint64_t* num_leaves, uint64_t* num_created);
/* Host arrays, each nullable: leaf_index (num_leaves: the leaf list), created (num_created: positions in the leaf list, in
 * leaf order), kept (points the tile's query kept) and drawn (points that landed inside the image). */
int pcv_xray_tiles(const pcv_xray* x, uint64_t* leaf_index, uint64_t* created, uint64_t* kept, uint64_t* drawn);
/* Created tiles [first, first + count) as RGBA8, W x W each, rows top to bottom (RgbaImage), into `capacity` bytes
 * that live where `mem` says. */
int pcv_xray_images(pcv_xray* x, uint64_t first, uint64_t count, uint64_t capacity, int mem, uint8_t* rgba);
void pcv_xray_free(pcv_xray* x);
/* The finalisation functions of the raster kernel, on the host (same code): fn = PCV_XRAY_FN_XRAY: in[i] = number of
 * distinct z buckets (0: no point); _COLORED: in[4i..4i+3] = exact r, g, b sums and the point count; _JET / _PURPLISH:
 * in[i] = value in [0, 1] (as f32); _TO_U8: in[4i..4i+3] = a Color<f32> (src/color.rs:29-36). Writes count RGBA8 pixels
 * before any background is applied. */
#define PCV_XRAY_FN_XRAY 0
#define PCV_XRAY_FN_COLORED 1
#define PCV_XRAY_FN_JET 2
#define PCV_XRAY_FN_PURPLISH 3
#define PCV_XRAY_FN_TO_U8 4
/* _INTENSITY: in[3i..3i+2] = mean, min, max (each as f32): IntensityColoringStrategy::get_pixel_color after the mean
 * (:270-284): mean.max(min).min(max) with Rust's NaN rules, then ln(mean - min) / ln(max - min) in f32, through the
 * kernel's own ln (an f64 series rounded to f32 once, no libm), as Color{b, b, b, 1}.to_u8(). */
#define PCV_XRAY_FN_INTENSITY 5
int pcv_xray_finalize(int fn, uint64_t count, const double* in, uint8_t* rgba);

/* ---- xray parent levels and the quadtree directory (create_non_leaf_nodes :656-682, build_node :726-759) -------------
 * Every level above the leaves up to root_node_id, on the device: a parent is build_parent (:410-450) of its four
 * children (a missing child is the background) shrunk from 2W x 2W to W x W by image 0.23.10's Lanczos3 resize, restated
 * bit for bit: the taps below, the vertical pass first into an f32 intermediate, then the horizontal pass, clamp to
 * [0, 255] and round half away from zero. All parent images are allocated before any launch: PCV_E_OOM leaves the
 * leaves valid. A second call is a no-op; with root_level == deepest_level or no created leaf there are no parents. */
int pcv_xray_build_parents(pcv_xray* x);
/* Meta.nodes in a fixed order: the created leaves (the positions of pcv_xray_images), then each parent level from
 * deepest_level - 1 up to root_level in ascending index. Before pcv_xray_build_parents only the leaves. *num_nodes is
 * the total; the first `capacity` are written (level and index of their quadtree NodeId, each array nullable). */
int pcv_xray_nodes(const pcv_xray* x, uint64_t* num_nodes, uint64_t capacity, uint32_t* level, uint64_t* index);
/* Nodes [first, first + count) of pcv_xray_nodes' order as RGBA8, W x W each, rows top to bottom, into `capacity`
 * bytes that live where `mem` says. A range past the end is PCV_E_INVALID and writes nothing. */
int pcv_xray_node_images(pcv_xray* x, uint64_t first, uint64_t count, uint64_t capacity, int mem, uint8_t* rgba);
/* build_xray_quadtree's output directory (created if missing, files overwritten): one "<NodeId>.png" per node ("r" and
 * base-4 digits) and get_meta_pb_path's meta file (root id with "r" -> "meta", ".pb": meta.pb for r, meta01.pb for
 * r01), xray_proto Meta version 3 as rust-protobuf 2.x writes proto3 (fields in number order, zero scalars omitted):
 * the root node's bounding rect, deepest_level, tile_size and every node in pcv_xray_nodes' order. The PNGs are those of
 * pcv_xray_png_encode: the same pixels as the reference's png 0.16.7 encoder, not the same bytes. PCV_E_INVALID when
 * parents exist but pcv_xray_build_parents has not run; PCV_E_IO when a file cannot be written. */
int pcv_xray_write_dir(pcv_xray* x, const char* directory);
/* Host only, no context: the taps of the 2:1 resize for a tile of tile_size_px = W (1 ..= 32768) pixels: for output
 * index o, left[o] and count[o] (the input rows / columns [left, left + count) of 2W), and weights[12 o ..= 12 o + 11]
 * (normalised, zero past count). Arrays of W entries (12 W weights), each nullable. */
int pcv_xray_lanczos_taps(uint32_t tile_size_px, uint32_t* left, uint32_t* count, float* weights);
/* Host only, no context: a w x h RGBA8 image (rows top to bottom) as PNG: colour type 6, depth 8, one IDAT, filter byte
 * 0 on every row, zlib with stored deflate blocks. *needed = the file size; it is written when out != NULL and
 * capacity >= *needed. w or h == 0 is PCV_E_INVALID. */
int pcv_xray_png_encode(const uint8_t* rgba, uint32_t w, uint32_t h, uint8_t* out, uint64_t capacity, uint64_t* needed);

/* ---- opt-in compressed tiles: run-length deflate, encoded on the device ------------------------------------------------
 * PCV_XRAY_PNG_STORED is what pcv_xray_png_encode and pcv_xray_write_dir write, byte for byte. PCV_XRAY_PNG_DEFLATE keeps
 * the signature, IHDR (filter method 0), one IDAT and IEND, and compresses the scanlines without a match search:
 *   scanlines  row 0 has filter byte 1 (Sub, 4 bytes per pixel), every other row filter byte 2 (Up)
 *   bands      PCV_XRAY_PNG_BAND_ROWS(w) consecutive rows (the last band may be shorter), each one deflate block with the
 *              fixed Huffman codes and BFINAL 0, followed by an empty stored block (3 header bits, padding, 00 00 FF FF):
 *              every band starts and ends on a byte boundary; the stored block after the last band carries BFINAL 1
 *   tokens     per maximal run of L equal bytes inside a band: one literal, then with r = L - 1 matches of min(r, 258)
 *              bytes at distance 1 while r >= 3, then r (0, 1 or 2) literals; end-of-block closes the band
 *   zlib       78 01, the bands, the Adler-32 of the scanlines
 * A band of n scanline bytes takes at most ceil((3 + 9 n + 7) / 8) + 5 bytes, a stream 2 + its bands + 4; every buffer is
 * sized from that bound (noise grows by about 6 %). Width or height above PCV_XRAY_PNG_DEFLATE_MAX_EDGE is
 * PCV_E_INVALID in deflate mode: one row must fit a band. */
#define PCV_XRAY_PNG_STORED 0
#define PCV_XRAY_PNG_DEFLATE 1
#define PCV_XRAY_PNG_BAND_BYTES 40960u /* scanline bytes a band may hold: its bit buffer (46 087 bytes) fits 48 KiB of LDS */
#define PCV_XRAY_PNG_DEFLATE_MAX_EDGE 8192u
/* rows per band: 8, fewer once 8 rows of 1 + 4 w bytes pass PCV_XRAY_PNG_BAND_BYTES, never less than 1 */
#define PCV_XRAY_PNG_BAND_ROWS(w)                                                   \
  (PCV_XRAY_PNG_BAND_BYTES / (1u + 4u * (uint32_t)(w)) >= 8u ? 8u                   \
   : PCV_XRAY_PNG_BAND_BYTES / (1u + 4u * (uint32_t)(w)) >= 1u ? PCV_XRAY_PNG_BAND_BYTES / (1u + 4u * (uint32_t)(w)) : 1u)
/* Host only, no context: pcv_xray_png_encode with the mode chosen. *needed is the size of this image's file (in deflate
 * mode it depends on the pixels, so rgba is read even when out == NULL; rgba == NULL then reports the bound). Nothing is
 * written unless out != NULL and capacity >= *needed. */
int pcv_xray_png_encode_ex(const uint8_t* rgba, uint32_t w, uint32_t h, int mode, uint8_t* out, uint64_t capacity, uint64_t* needed);
/* Host only: the largest file pcv_xray_png_encode_ex can make of a w x h image in `mode`; 0 for bad arguments. */
uint64_t pcv_xray_png_bound(uint32_t w, uint32_t h, int mode);
/* The complete PNG files of nodes [first, first + count) of pcv_xray_nodes' order, back to back in host memory:
 * offsets[i] .. offsets[i + 1] is node first + i (count + 1 offsets). out == NULL: the offsets alone. capacity below
 * offsets[count] is PCV_E_INVALID (the content of out is then unspecified). Built quadtrees, and the levels a merged
 * quadtree built itself, are compressed on the device in deflate mode and only compressed bytes come down; stored mode
 * gives the bytes of pcv_xray_write_dir. The nodes of opened quadtrees are handed out as the bytes of their files, whatever
 * the mode. Equal to pcv_xray_png_encode_ex of pcv_xray_node_images, byte for byte, for every node that is encoded. */
int pcv_xray_node_pngs(pcv_xray* x, uint64_t first, uint64_t count, int mode, uint64_t capacity, uint8_t* out, uint64_t* offsets);
/* pcv_xray_write_dir with the PNG mode chosen; pcv_xray_write_dir(x, d) is pcv_xray_write_dir_ex(x, d, PCV_XRAY_PNG_STORED).
 * File names and the meta file do not depend on the mode. In deflate mode the tiles are compressed on the device, chunk by
 * chunk through the same two pinned buffers, and the writer threads only wrap and write; a merged quadtree still copies the
 * files of opened parts byte for byte and applies the mode to the nodes it encodes. */
int pcv_xray_write_dir_ex(pcv_xray* x, const char* directory, int mode);
/* `count` w x w RGBA8 tiles (host or device memory, back to back) through the device encoder, as pcv_xray_node_pngs hands
 * nodes out (deflate mode, out / offsets / capacity alike). chunk_tiles > 0: tiles per device chunk (0: the context's). */
int pcv_xray_png_encode_tiles(pcv_ctx* ctx, const uint8_t* rgba, int mem, uint32_t w, uint64_t count, uint64_t chunk_tiles,
                              uint64_t capacity, uint8_t* out, uint64_t* offsets);
/* Bytes of node images per download chunk of pcv_xray_write_dir* and pcv_xray_node_pngs (default 64 MiB, at least one
 * tile; 0 restores the default). */
int pcv_ctx_set_xray_chunk_bytes(pcv_ctx* ctx, uint64_t bytes);

/* ---- reading a quadtree directory back, and merge_xray_quadtrees (xray/src/bin/merge_xray_quadtrees.rs) ----------------
 * Host only, no context: one PNG file as RGBA8, rows top to bottom, for the tiles the reference's png encoder or
 * pcv_xray_png_encode wrote (what image::open does for build_node, xray/src/generation.rs:742-750). Read: the signature,
 * every chunk CRC, IHDR colour type 6 at depth 8, not interlaced, any number of IDAT chunks, ancillary chunks skipped; the
 * zlib header, stored, fixed-Huffman and dynamic-Huffman deflate blocks (an inflate of the library's own: zlib is not
 * linked), the Adler-32; the row filters None, Sub, Up, Average and Paeth. *w and *h (each nullable) are set once the header
 * is accepted; with rgba == NULL nothing else happens. Another colour type, depth or interlacing, and capacity below
 * 4 * w * h, are PCV_E_INVALID; anything truncated or corrupt (a bad CRC or Adler-32, an invalid Huffman code, a distance
 * before the start of the output, more or fewer than h * (1 + 4 w) scanline bytes) is PCV_E_IO. The input is never read
 * past len, rgba is written only by a successful call and never past capacity. The message of a failure is
 * pcv_host_last_error's. */
int pcv_png_decode(const uint8_t* file, uint64_t len, uint32_t* w, uint32_t* h, uint8_t* rgba, uint64_t capacity);
/* The message of the calling thread's last failed call that had no context to keep it: pcv_png_decode, and the pcv_xray_*
 * calls on handles that pcv_xray_open_dir made without a context. */
const char* pcv_host_last_error(void);
/* Every meta*.pb of `directory` (read_metadata_from_directory :54-61) as one "opened" pcv_xray each, in ascending file
 * name order (the reference takes them in directory-walk order, which is not defined). xray_proto's Meta is parsed as
 * Meta::from_proto does (xray/src/lib.rs:81-116): version 3; version 2 with the deprecated f32 min / edge_length where
 * Rect.min is absent; any other version, and bytes that are no Meta, are PCV_E_INVALID (the reference panics on the
 * version). *num_parts is the number of meta files; handles are made only when capacity >= *num_parts. A directory that
 * cannot be read is PCV_E_IO.
 * An opened handle serves pcv_xray_info (rect: the file's bounding_rect, that of its root node; num_leaves and num_created:
 * the nodes at deepest_level), pcv_xray_tile_size, pcv_xray_nodes (descending level, then ascending index: a file keeps no
 * order, the reference holds a hash set) and pcv_xray_node_images, which decodes "<NodeId>.png" on demand: a missing or
 * undecodable file is PCV_E_IO, an image that is not tile_size x tile_size PCV_E_INVALID. pcv_xray_tiles, _images,
 * _negative and _build_parents on it are PCV_E_INVALID, and pcv_xray_write_dir too (merge it: a lone part merges to itself
 * plus the levels above its root).
 * ctx may be NULL: the handles are then host only (PCV_MEM_HOST images), can be passed to pcv_xray_merge_check and to a
 * pcv_xray_merge of any context, and report failures through pcv_host_last_error. */
int pcv_xray_open_dir(pcv_ctx* ctx, const char* directory, uint32_t capacity, pcv_xray** parts, uint32_t* num_parts);
/* Meta.tile_size of any quadtree handle; 0 for NULL. */
uint32_t pcv_xray_tile_size(const pcv_xray* x);
/* Host only, no context: validate_and_merge_metadata (:129-186) over `parts` in argument order. PCV_E_INVALID with the
 * reference's message in err for: num_parts == 0 ("No subquadtrees meta files found."); every part without nodes ("All
 * subquadtress are empty."); two parts with the same root ("Not all roots are unique."); roots of different levels ("Not
 * all roots have the same level."); different deepest_level or tile_size, empty parts included ("Not all meta files have
 * the same deepest level." / "... the same tile size."). A part's root is its node of minimum level
 * (Meta::get_root_node, xray/src/lib.rs:139-147); a part that holds several nodes at that level is PCV_E_INVALID here (the
 * reference takes whichever its hash set yields first). Also PCV_E_INVALID: a null or freed part, a device-built part
 * whose parents are not built, a root level above deepest_level.
 * *root_level = the roots' level L. rect = the merged bounding rect: the rect of the first non-empty part's root node
 * (an opened part: the file's; a built part: what pcv_xray_write_dir writes) under Node::parent (quadtree/src/lib.rs:100-120)
 * L times, each step min.y -= edge when child_index & 1, min.x -= edge when child_index & 2, then edge *= 2, in f64 and in
 * that order. */
int pcv_xray_merge_check(pcv_xray* const* parts, uint32_t num_parts, uint32_t* root_level, double rect[3], char* err,
                         uint64_t errcap);
/* merge (:188-205): the quadtree with root r over parts that passed pcv_xray_merge_check, device-built (pcv_xray_run*,
 * parents built) and opened ones mixed; a part of another context is PCV_E_INVALID. The levels L - 1 .. 0 above the roots
 * are create_non_leaf_nodes(roots, L, 0) (generation.rs:656-682): per level the parents of the level below in ascending
 * index, each build_parent of its four children and the Lanczos3 2:1 resize of pcv_xray_build_parents, on the device. A
 * child that is in no part is `background` (PCV_XRAY_BG_*): the reference asks whether the child's file exists in the
 * output directory (:742), which in a directory that holds only the merged trees is membership in the node set. The parts'
 * own images are never re-backgrounded. The root tiles are staged into one level array on the context's stream (device to
 * device from built parts, one pinned upload for opened ones), every new image is allocated before any launch
 * (PCV_E_OOM leaves nothing allocated), and L == 0 builds nothing.
 * The result serves pcv_xray_info (rect: the merged rect; leaves: the nodes at deepest_level), pcv_xray_nodes (every part's
 * nodes in part order, each in its own order, then the new levels L - 1 .. 0 in ascending index; unique roots at one level
 * make the parts disjoint), pcv_xray_node_images (a part's node is forwarded to the part) and pcv_xray_write_dir: the PNG
 * of an opened part's node is copied byte for byte from the part's directory (copy_images :28-46; not when that is the
 * output directory), the others are encoded by pcv_xray_png_encode, and meta.pb holds the merged rect, deepest_level,
 * tile_size and the union node list; other meta*.pb files of an in-place merge stay, as in the reference. It owns the new
 * images only: the parts must outlive it, and once one of them is freed the image calls and pcv_xray_write_dir return
 * PCV_E_INVALID. pcv_xray_tiles, _images, _negative and _build_parents on it are PCV_E_INVALID. */
int pcv_xray_merge(pcv_ctx* ctx, pcv_xray* const* parts, uint32_t num_parts, uint32_t background, pcv_xray** out);

/* ---- inpaint_xray_quadtree (xray/src/bin/inpaint_xray_quadtree.rs, xray/src/inpaint.rs): hole filling for leaf tiles ------
 * The leaves of a quadtree x whose background is transparent are stitched with their eight neighbours into tiles twice as
 * wide and high, the holes that a morphological close of the alpha mask covers are filled, overlapping enlarged tiles are
 * blended, the centre is cropped, the background is assigned and every parent level is rebuilt.
 * PARITY: the adjacent leaves (step 1, bin :41-71), the stitch (2, inpaint.rs:90-121), the masks (3, :27-31), the blend (5,
 * :132-161 with utils.rs:46-60), the crop (6, :163-173), assign_background_color and create_non_leaf_nodes (7,
 * generation.rs:684-708, :656-682) are the reference's, byte for byte. The fill (4) is NOT: the reference hands the target
 * pixels to the texture-synthesis crate (inpaint.rs:32-43); here a target pixel is a distance-weighted mean of the known
 * pixels around it. So the pixels that were filled, and what the blend and the Lanczos resize make of them, differ from the
 * reference's; every other pixel of every tile does not.
 * x and up to four neighbour quadtrees are device-built with PCV_XRAY_BG_TRANSPARENT (pcv_xray_run*), opened from a
 * directory, or results of pcv_xray_inpaint with a transparent background; a merged quadtree is refused. Leaves of diagonal
 * quadtrees are never taken: that is the reference's separate-directory mode (its in-place mode would find their files on
 * disk). distance_px is inpaint_distance_px, a u8: 0 inpaints nothing (perform_inpainting :222 returns early; the leaves
 * are re-backgrounded and the parents rebuilt); 255 is PCV_E_INVALID, because imageproc 0.21.0's distance transform saturates
 * at 255 and its close (Norm::LInf) is then no longer the morphological one. */
#define PCV_XRAY_INPAINT_MAX_TILE 8192u /* tile size of an inpainted quadtree: a group's target list has u32 pixel numbers */
/* Peak device bytes of pcv_xray_inpaint for tiles of w pixels: the result holds 4 w w per leaf and parent and an opened x is
 * staged whole (4 w w per leaf), the adjacent leaves of the neighbours likewise; the work of one enlarged tile (RGBA 16 w w,
 * three masks 3 x 4 w w, the target list 16 w w) is held for one group of leaves at a time: consecutive leaves whose
 * enlarged tiles (at most 9 per leaf: the leaf's and those it blends with) fit pcv_ctx_set_xray_chunk_bytes, at least one
 * leaf per group. */
#define PCV_XRAY_INPAINT_WORK_BYTES(w) (44ull * (uint64_t)(w) * (uint64_t)(w))
/* Host only, no context: what pcv_xray_inpaint refuses before any device work, PCV_E_INVALID with a message in err: a null,
 * freed or merged handle; a built x or neighbour whose background is white (its holes are gone); a tile size that is not a
 * power of two >= 2 (w = W / 2 must halve again, inpaint.rs:92-94) or above PCV_XRAY_INPAINT_MAX_TILE; distance_px >= 255;
 * more than four neighbours; a neighbour with another tile size or deepest level; a neighbour whose root is not
 * root.neighbor(Left / Top / Right / Bottom) at the root's level (bin :53-57), or two neighbours on one side; an opened
 * handle without nodes or with several nodes at its minimum level. */
int pcv_xray_inpaint_check(const pcv_xray* x, pcv_xray* const* neighbours, uint32_t num_neighbours, uint32_t distance_px, char* err,
                           uint64_t errcap);
/* Host only, no context: steps 1 and 2 as a table. get_adjacent_leaf_node_ids (bin :41-71): a leaf n of the neighbour in
 * direction D is taken iff n.neighbor(D.opposite()) is a leaf of x (Top is y + 1, quadtree/src/lib.rs:290-302);
 * *num_adjacent is their number. stitched_image (inpaint.rs:90-121): for the first `capacity` leaves of x, in
 * pcv_xray_nodes' order, 9 slots of 2 entries each (18 uint32_t per leaf), in the order TopLeft, Top, TopRight, Left, the
 * leaf itself, Right, BottomLeft, Bottom, BottomRight: (part, node) with part 0 = x and k + 1 = neighbours[k], node = the
 * position among that part's leaves (its pcv_xray_nodes order), or (0xffffffff, 0xffffffff) where no tile contributes. A
 * slot is filled by a leaf of x or by a taken leaf of a neighbour. The checks of pcv_xray_inpaint_check apply. */
int pcv_xray_inpaint_plan(const pcv_xray* x, pcv_xray* const* neighbours, uint32_t num_neighbours, uint64_t capacity, uint32_t* slots,
                          uint64_t* num_adjacent, char* err, uint64_t errcap);
/* Steps 1-7 on the device. background (PCV_XRAY_BG_*) is --tile-background-color: pixels whose alpha is below 128 after the
 * blend take it (generation.rs:697-701), and it is the missing child of the parent levels. A handle of another context and
 * an unknown background are PCV_E_INVALID, with pcv_xray_inpaint_check's refusals. Every image and work buffer is allocated
 * before the first launch: PCV_E_OOM leaves nothing allocated. x and the neighbours may be freed after the call.
 * The result owns its leaf and parent images. It serves pcv_xray_info (rect: that of x's root node), pcv_xray_tile_size,
 * pcv_xray_nodes (x's leaves in x's order, then each parent level from deepest_level - 1 up to the root in ascending
 * index: the node ids of x), pcv_xray_node_images, pcv_xray_node_pngs and pcv_xray_write_dir[_ex] (the meta file is named
 * after x's root, get_meta_pb_path); pcv_xray_merge_check and pcv_xray_merge take it as a part whose parents are built.
 * pcv_xray_tiles, _images, _negative and _build_parents on it are PCV_E_INVALID, as for a merged quadtree. */
int pcv_xray_inpaint(pcv_ctx* ctx, pcv_xray* x, pcv_xray* const* neighbours, uint32_t num_neighbours, uint32_t distance_px,
                     uint32_t background, pcv_xray** out);
/* Per leaf of the result (num_leaves entries each, nullable), counted within the final tile, the cropped centre of the
 * leaf's enlarged tile: target_pixels = pixels of the target mask (step 3); filled_pixels = pixels that were not known
 * (alpha 0 in x) and whose alpha after the blend is >= 128, so that they keep their colour; blended_pixels = pixels that
 * step 5 changed in any channel. All zero for distance_px == 0. PCV_E_INVALID for any other kind of handle. */
int pcv_xray_inpaint_info(const pcv_xray* x, uint64_t* target_pixels, uint64_t* filled_pixels, uint64_t* blended_pixels);

/* ---- the viewer's frame (sdl_viewer/src/lib.rs:158-209, node_drawer.rs:124-160, shaders/points.vs, points.fs) ----------
 * V cameras over one octree in one call, rasterised on the device into RGBA8 images that stay there. OpenGL leaves sub-pixel
 * snapping, the depth format and fused arithmetic to the driver, so the frame is a stated restatement:
 *  - nodes: the frustum's visible list in heap pop order, cut to its first max_nodes entries (take(max_nodes_to_display),
 *    lib.rs:180-186; 0 = all); level of detail 1, every point of a drawn node (lib.rs:194-199, node_drawer.rs:132-134);
 *  - position (points.vs): the vertex attribute as GL delivers it (Uint8 c / 255 and Uint16 c / 65535 in f32, Float32, Float64
 *    as f64), times edge_length plus min in f64; gl_Position = vec4(world_to_gl * dvec4) with the frustum's clip_from_query,
 *    f64, left to right, one rounding to f32;
 *  - a point is drawn iff 0 < w < inf and -w <= x, y, z <= w in f32; window coordinates in f32; it covers the pixels whose
 *    centre lies in [xw - point_size / 2, xw + point_size / 2) in x and likewise in y (PROGRAM_POINT_SIZE, node_drawer.rs:139);
 *  - DEPTH_TEST with the default GL_LESS over a black clear (node_drawer.rs:140, lib.rs:172-178): per pixel the smallest
 *    window depth wins, equal depths go to the point drawn first (position of its node in the cut list, then index in the node);
 *  - colour (points.vs): table[c] = round(255 * pow(c / 255, 1 / gamma)) in f32 per channel, alpha 255; background (0, 0, 0, 255). */
#define PCV_RENDER_MAX_POINT_SIZE 64
typedef struct pcv_render_params {
  uint32_t width, height;        /* 1 ..= 16384 each */
  float point_size;              /* 1 ..= PCV_RENDER_MAX_POINT_SIZE (the viewer's own floor is 1, lib.rs:152-156) */
  float gamma;                   /* finite, > 0 */
  uint32_t max_nodes;            /* max_nodes_to_display; 0: every visible node */
  uint64_t max_workspace_bytes;  /* the u64 key planes of one group of views; 0: 2 GiB */
} pcv_render_params;
typedef struct pcv_render pcv_render;
/* Host only, no context: PCV_E_INVALID for a width or height outside 1 ..= 16384, a point_size outside
 * 1 ..= PCV_RENDER_MAX_POINT_SIZE (or NaN), a gamma that is not a finite number > 0. */
int pcv_render_check_params(const pcv_render_params* params);
/* Host only, no context: the colour table of points.vs for `gamma` (finite, > 0), computed with the host's powf. */
int pcv_render_gamma_lut(float gamma, uint8_t lut[256]);
/* One frame per frustum of `frusta` (a shape of another kind is PCV_E_INVALID), as the viewer's draw loop produces it
 * (lib.rs:158-209). A frustum whose visible-node status is 1 or 2 (the reference panics there) yields a cleared image and
 * reports that status. A view whose drawn nodes hold 2^32 - 1 points or more is PCV_E_INVALID; a single view whose key plane
 * (8 bytes per pixel) exceeds max_workspace_bytes is PCV_E_OOM. A failed call leaves nothing allocated. The octree may be a
 * built one or one opened from a directory; it and `frusta` may be freed after the call. */
int pcv_render_views(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* params, pcv_render** out);
/* show_octree_nodes (lib.rs:202-208, box_drawer.rs): what pcv_render_views_ex draws on top of the points. With
 * PCV_RENDER_OUTLINE_NODES the wireframe of every drawn node's bounding cube is drawn right after the node's points, under
 * the same depth test, in outline_rgba stored as given (the outline shader applies no gamma; the viewer's YELLOW is
 * PCV_RENDER_OUTLINE_YELLOW). The restatement: the cube's 12 edges in box_drawer.rs's index order,
 * corners min | min + edge to clip space as a point's position; Liang-Barsky in f32 against w > 0, w + x, w - x, w + y,
 * w - y, w + z, w - z >= 0 in that order (t = d0 / (d0 - d1), endpoints a + t * (b - a)); a segment with a non-finite clip
 * coordinate, a clipped w outside (0, inf) or a non-finite window coordinate is dropped; width 1 along the major axis (a tie
 * goes to x): every pixel centre in [min, max), the other coordinate and zw interpolated in f32, zw clamped to [0, 1]. A
 * node owns n + 1 consecutive draw ranks, the last for its outline: at equal depth an outline loses to its own node's points
 * and to everything drawn before, and wins against every later node. The limit of 2^32 - 1 ranks per view includes them. */
#define PCV_RENDER_OUTLINE_NODES 1u
#define PCV_RENDER_OUTLINE_YELLOW {255, 255, 0, 255}
typedef struct pcv_render_overlay {
  uint32_t flags;           /* PCV_RENDER_OUTLINE_NODES or 0; any other bit is PCV_E_INVALID */
  uint8_t outline_rgba[4];  /* read only with PCV_RENDER_OUTLINE_NODES */
} pcv_render_overlay;
/* Host only, no context: PCV_E_INVALID for unknown flag bits, with the reason in `message` (NUL-terminated, cut to
 * `capacity`; nullable). A null overlay is valid: nothing is drawn on top. */
int pcv_render_check_overlay(const pcv_render_overlay* overlay, char* message, uint64_t capacity);
/* pcv_render_views with an overlay. A null overlay or flags == 0 is pcv_render_views itself: the same launches, the same
 * bytes. With outlines on, pixels_covered of pcv_render_info counts every pixel that is not background. */
int pcv_render_views_ex(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* params,
                        const pcv_render_overlay* overlay, pcv_render** out);
/* Per view (each output nullable): 12 per drawn node, the segments that survived the clip, the pixels of the final image an
 * outline won. All zero without PCV_RENDER_OUTLINE_NODES and for a view whose status is not 0. */
int pcv_render_outline_info(pcv_render* r, uint32_t view, uint64_t* segments_submitted, uint64_t* segments_drawn,
                            uint64_t* outline_pixels);
/* Per view (each output nullable): the visible-node status, the length of the visible list, the nodes drawn after the cut,
 * the points of the drawn nodes (node_drawer.rs:132-134), the points inside the clip volume, the pixels some point covers. */
int pcv_render_info(pcv_render* r, uint32_t view, int32_t* status, uint32_t* nodes_visible, uint32_t* nodes_drawn,
                    uint64_t* points_submitted, uint64_t* points_drawn, uint64_t* pixels_covered);
/* Views [first, first + count) as RGBA8, height x width each, rows top to bottom (the frame a window would show,
 * lib.rs:158-209), into memory that lives where `mem` says. A range past the end is PCV_E_INVALID and writes nothing. */
int pcv_render_images(pcv_render* r, uint32_t first, uint32_t count, void* rgba, int mem);
/* The same views' window depth as f32 (the depth buffer behind node_drawer.rs:140), 1.0 where no point was drawn. */
int pcv_render_depth(pcv_render* r, uint32_t first, uint32_t count, void* zw_f32, int mem);
void pcv_render_free(pcv_render* r);

/* The `/nodes_data` reply blob of octree_web_viewer (octree_web_viewer/src/backend.rs:90-177) for a list of nodes:
 * per node min xyz (3 x f64 LE), edge (f64), num_points (u32), bytes per coordinate (u8), pad to 8, raw .xyz, pad
 * to 8, raw .rgb, pad to 8. *needed = blob size; the blob is written when out != NULL and capacity >= *needed. */
int pcv_octree_nodes_blob(pcv_octree* t, const uint64_t* node_indices, uint64_t count, uint8_t* out, uint64_t capacity,
                          uint64_t* needed);

/* Q5: Isometry3 * Point3 for a batch (xray/src/generation.rs:493-497; Aabb::transform aabb.rs:58-66 uses the
 * same product). iso = translation xyz, unit quaternion i j k w. Outputs live where the inputs live. */
int pcv_transform_points(pcv_ctx* ctx, const double iso[7], const pcv_points* points, double* ox, double* oy, double* oz);

/* ---- S2 cell clouds ------------------------------------------------------------------ */
/* `CellID::from_point(p).parent(level)` of the s2 crate for every point (what S2Splitter::write asks of it,
 * src/read_write/s2.rs:75), restated from the public S2 definition: normalise, cube face, (u, v), the quadratic st, ij, the
 * Hilbert curve. level 0 ..= 30 (30 = leaf cells); anything else is PCV_E_INVALID. No validity test: any point gets an id.
 * `ids` lives where `mem` says; the points where points->mem says (colour and intensity are not read). The device's ids equal
 * pcv_s2_cell_ids_host's bit for bit: one chain of correctly rounded f64 operations on both sides. */
int pcv_s2_cell_ids(pcv_ctx* ctx, const pcv_points* points, uint32_t level, uint64_t* ids, int mem);
/* Host only, no context (failures: pcv_host_last_error). */
int pcv_s2_cell_ids_host(uint64_t n, const double* x, const double* y, const double* z, uint32_t level, uint64_t* ids);
/* CellID::to_token (the stem of a cell's files, s2.rs:122): 16 lower-case hex digits without trailing zeros, "X" for 0. */
int pcv_s2_cell_token(uint64_t id, char out[17]);

/* CellUnion::contains(p) per point (the point test of S2Cells' cell-union queries, src/s2_cells/mod.rs): contains_cellid of
 * the point's leaf cell over `cells`, num_cells cell ids of any levels in HOST memory, ascending by id (a list that descends
 * anywhere, or holds a 0, is PCV_E_INVALID). keep[i] = 1 / 0 lives where `mem` says. The cells of a cloud under a union:
 * pcv_s2_cells_in_location. */
int pcv_s2_union_contains(pcv_ctx* ctx, const uint64_t* cells, uint32_t num_cells, const pcv_points* points, uint8_t* keep, int mem);
/* Host only, no context: the same flags, bit for bit. */
int pcv_s2_union_contains_host(const uint64_t* cells, uint32_t num_cells, uint64_t n, const double* x, const double* y,
                               const double* z, uint8_t* keep);

/* S2Splitter::write + get_meta (src/read_write/s2.rs:60-173) for ONE batch: the points grouped by their cell at
 * split_level (0 ..= 30; DEFAULT_S2_SPLIT_LEVEL is 20), cells ascending by id, the points of a cell in input order, as
 * cell-contiguous device blobs: xyz as 24-byte AoS f64 (Encoding::Plain), rgb at 3 bytes, intensity at 4 bytes when
 * points->intensity is set. points->color is required. Fewer than 2^32 - 1 points per call.
 * A point whose radius sqrt(x*x + y*y + z*z) is above 6 384 400 or below 6 352 800 (s2.rs:64-65), or that has a NaN coordinate
 * (a departure: the reference lets NaN through both comparisons), is invalid: PCV_E_INVALID, pcv_last_error names the FIRST such
 * point in input order with its index and coordinates, *out is NULL. The bounding box is the exact min / max of the points.
 * A stream of batches, clouds larger than the device and OpenMode::Append: pcv_s2_stream_* below. */
typedef struct pcv_s2_cloud pcv_s2_cloud;
int pcv_s2_split(pcv_ctx* ctx, const pcv_points* points, uint32_t split_level, pcv_s2_cloud** out);
/* Any output may be NULL. */
int pcv_s2_info(const pcv_s2_cloud* cloud, uint64_t* num_cells, uint64_t* num_points, double bbox_min[3], double bbox_max[3],
                int* has_intensity, uint32_t* level);
/* Per cell (S2CellMeta, src/s2_cells/mod.rs): id, num_points, and the offset of its first point in the blobs (host arrays of
 * num_cells entries; any may be NULL). */
int pcv_s2_cells(const pcv_s2_cloud* cloud, uint64_t* ids, uint64_t* counts, uint64_t* offsets);
/* The permutation: input_index[slot] = index in the input of the point at `slot` of the blobs (num_points entries where `mem`
 * says) — a stable sort of the points by cell id. */
int pcv_s2_order(pcv_s2_cloud* cloud, uint32_t* input_index, int mem);
/* The points of cells [first_cell, first_cell + num_cells) as they would stand in the cells' files, one after the other, into
 * memory that lives where `mem` says (any output may be NULL). A range past the end, more points than `capacity`, or
 * `intensity` on a cloud without it is PCV_E_INVALID and writes nothing. */
int pcv_s2_cell_points(pcv_s2_cloud* cloud, uint64_t first_cell, uint64_t num_cells, uint64_t capacity, int mem, double* xyz,
                       uint8_t* rgb, float* intensity);
/* `<token>.xyz/.rgb[/.intensity]` per cell (s2.rs:121-136 over RawNodeWriter, Encoding::Plain) + meta.pb: version 13,
 * bounding_box, s2 { cells, attributes: color = U8Vec3 (27), intensity = F32 (11) } (proto.proto:92-133). The reference emits
 * cells and attributes in hash order; here cells ascend by id and color precedes intensity. PCV_E_IO names the file. */
int pcv_s2_write_dir(pcv_s2_cloud* cloud, const char* directory);
/* S2Cells::from_data_provider + S2Meta::from_proto (src/s2_cells/mod.rs:107-154, 199-212) over a directory: the same object
 * that pcv_s2_split makes; pcv_s2_info / _cells / _cell_points / _write_dir / _cells_in_location / _free work on it unchanged
 * (pcv_s2_order does not: there is no input). meta.pb of version < 12: PCV_E_INVALID "No S2 point cloud supported with version
 * N"; without the s2 arm: PCV_E_INVALID "This meta does not describe S2 point clouds" (the reference's messages). The cells
 * may be listed in any order and come out ascending by id; `color` (U8Vec3) is required, `intensity` (F32) optional, other
 * attributes are kept as extras (pcv_s2_attributes below). *level of pcv_s2_info is the common level of the ids, 0xffffffff when they differ. The cell files
 * are read and uploaded on first use (cell_points, write_dir): a file whose size is not that of the cell's num_points (24 / 3 /
 * 4 bytes each), or a missing file of a cell with points, is PCV_E_IO naming the file.
 * ctx may be NULL (as for pcv_xray_open_dir): a host-only cloud, whose failures go to pcv_host_last_error; info, cells,
 * cell_points into host memory and write_dir work, anything that needs the device is PCV_E_INVALID. */
int pcv_s2_open_dir(pcv_ctx* ctx, const char* directory, pcv_s2_cloud** out);
void pcv_s2_free(pcv_s2_cloud* cloud);

/* ---- S2 cell clouds from a stream of batches ----------------------------------------- */
/* S2Splitter as the NodeWriter<PointsBatch> it is (src/read_write/s2.rs:60-173): `write` once per batch for as long as the
 * input lasts, `get_meta` at the end. Every batch is split as pcv_s2_split splits it and waits on the device as a part; the
 * cloud is the parts' merge by cell, the batches in their order inside a cell (one kernel launch, planned by
 * pcv_s2_merge_plan_host's code).
 *   directory == NULL   in-memory: pcv_s2_stream_finish returns the cloud that pcv_s2_split of the concatenated batches returns
 *                       (cells, bbox, level, blobs, pcv_s2_order as indices into the concatenation). Fewer than 2^32 - 1 points in
 *                       all: the append that crosses it is PCV_E_INVALID.
 *   directory != NULL   the cells' files are written as the stream goes: whenever the pending parts hold flush_points points or
 *                       more (0: 2^26; at most 2^31) and once more at finish, if anything is pending, they are merged, copied to
 *                       pinned host memory and every cell's run is appended to <token>.xyz/.rgb[/.intensity] — a file is
 *                       truncated the first time THIS stream writes its cell and appended to afterwards (s2.rs:121-136); files of
 *                       cells the stream never sees are left alone. Only per-cell counts (u64) and the bounding box are held
 *                       between flushes: the total is unbounded. finish writes meta.pb as pcv_s2_write_dir does; the directory
 *                       is byte for byte that of pcv_s2_write_dir(pcv_s2_split(concatenation)), whatever the batching and
 *                       flush_points. No input order is kept.
 *   PCV_S2_APPEND       (OpenMode::Append) the directory must hold an S2 meta.pb (pcv_s2_open_dir's failures and messages) whose
 *                       cells are all of split_level (else PCV_E_INVALID); its intensity presence is the stream's; no file is
 *                       truncated; finish writes a meta.pb whose counts are the old plus the new and whose bbox is the union. A
 *                       departure: the reference's splitter in append mode reports only what it saw itself and leaves the
 *                       bookkeeping to its caller.
 * Checked in this order, each PCV_E_INVALID (with a NULL ctx the message is pcv_host_last_error's): params / out NULL,
 * struct_size, split_level above 30, open_mode, PCV_S2_APPEND without a directory, flush_points, the directory appended to, ctx
 * NULL. */
#define PCV_S2_TRUNCATE 0
#define PCV_S2_APPEND 1
typedef struct pcv_s2_stream_params {
  uint32_t struct_size; /* sizeof(pcv_s2_stream_params) */
  uint32_t split_level; /* 0 ..= 30 */
  const char* directory; /* NULL: in-memory */
  int32_t open_mode;     /* PCV_S2_TRUNCATE / PCV_S2_APPEND */
  uint32_t reserved;
  uint64_t flush_points; /* directory mode: pending points that trigger a flush; 0 = the default */
} pcv_s2_stream_params;
typedef struct pcv_s2_stream pcv_s2_stream;
int pcv_s2_stream_begin(pcv_ctx* ctx, const pcv_s2_stream_params* params, pcv_s2_stream** out);
/* S2Splitter::write for one batch (host or device memory, color_stride 3 or 4; pcv_s2_split's requirements). The first
 * non-empty batch decides whether the cloud has intensity; a later one that differs is PCV_E_INVALID "S2Splitter received
 * incompatible data types for attribute intensity" (s2.rs:155). An invalid point refuses the batch with pcv_s2_split's
 * message; every refusal of a batch ends in " (batch K of the stream)", K = the batches accepted so far. A refused batch
 * leaves nothing behind and does not count; the stream stays usable. An empty batch counts as a batch and changes nothing
 * else. A flush that fails (PCV_E_IO naming the file, PCV_E_OOM, PCV_E_HIP) leaves a stream that can only be finished (which
 * reports the failure again) or aborted. */
int pcv_s2_stream_append(pcv_s2_stream* stream, const pcv_points* batch);
/* Any output may be NULL: batches accepted, points (with those of the directory appended to), distinct cells so far (likewise),
 * points of the pending parts, flushes done. */
int pcv_s2_stream_info(const pcv_s2_stream* stream, uint64_t* batches, uint64_t* points, uint64_t* cells, uint64_t* pending_points,
                       uint64_t* flushes);
/* S2Splitter::get_meta (s2.rs:139-173). Consumes the stream, success or not. In-memory: *out is the cloud (required). Directory
 * mode: the last flush, meta.pb, and in *out (may be NULL) the cloud that pcv_s2_open_dir opens over the directory. No points at
 * all: what pcv_s2_split / pcv_s2_write_dir make of none. PCV_E_OOM at a merge is reported as such. */
int pcv_s2_stream_finish(pcv_s2_stream* stream, pcv_s2_cloud** out);
/* Drops the stream and its pending parts; files already written stay. NULL is ignored. */
void pcv_s2_stream_abort(pcv_s2_stream* stream);
/* For tests: lowers the point limit of an in-memory stream from 2^32 - 1 to max_points (1 ..= 2^32 - 1), so that the refusal
 * can be reached; it is decided from the host-side counts alone. */
int pcv_s2_stream_set_memory_cap(pcv_s2_stream* stream, uint64_t max_points);

/* The merge plan, host only, no context (failures: pcv_host_last_error). Input: num_parts parts, part p's cells at
 * [part_first[p], part_first[p + 1]) of part_ids / part_counts (part_first[0] == 0), ids ascending strictly inside a part and
 * never 0, counts above 0, fewer than 2^32 - 1 points per part — anything else is PCV_E_INVALID. chunk_points: 0 = the
 * kernel's 2 048. Output: the merged cells (ids ascending, counts, offsets in points); one segment per (cell, part that holds
 * it) ordered by cell, then by part, which tile [0, n) in that order; for every output chunk of chunk_points points the index of
 * the segment that holds its first point. The three sizes are always written; arrays that are NULL are skipped (call once for
 * the sizes, once for the arrays). Deterministic. */
typedef struct pcv_s2_merge_segment {
  uint64_t dst_offset; /* first point in the merged blobs */
  uint64_t src_offset; /* first point in the part's blobs */
  uint32_t part;
  uint32_t count;
} pcv_s2_merge_segment;
int pcv_s2_merge_plan_host(uint32_t num_parts, const uint64_t* part_first, const uint64_t* part_ids, const uint64_t* part_counts,
                           uint32_t chunk_points, uint64_t* num_cells, uint64_t* num_segments, uint64_t* num_chunks, uint64_t* ids,
                           uint64_t* counts, uint64_t* offsets, pcv_s2_merge_segment* segments, uint64_t* chunk_first_segment);

/* ---- S2 cell clouds: the region side -------------------------------------------------- */
/* What S2Cells::nodes_in_location (src/s2_cells/mod.rs:160-241) asks of the s2 crate, restated from the public S2 definition
 * as one chain of correctly rounded f64 operations (no libm), so that the device's decisions are these host twins', bit for
 * bit. A rect is four doubles: lat.lo, lat.hi (empty when lo > hi), lng.lo, lng.hi (an interval on the circle: inverted when
 * lo > hi, empty = (pi, -pi), full = (-pi, pi)). Cells of level 0 (the six faces) have no geometry here: PCV_E_INVALID.
 * Host only, no context (failures: pcv_host_last_error).
 *
 * Cell::from(id) as far as Rect::intersects_cell reads it, 30 doubles: rect_bound [0..4), lat / lng of the centre [4..6),
 * the face's (u, v) bounds u.lo u.hi v.lo v.hi [6..10), the four unit vertices (lo,lo) (hi,lo) (hi,hi) (lo,hi) [10..22), their
 * lat / lng [22..30). */
int pcv_s2_cell_geometry_host(uint64_t cell, double geometry[30]);
/* Cell::rect_bound alone. */
int pcv_s2_cell_rect_host(uint64_t cell, double rect[4]);
/* The region of cells_in_convex_polyhedron (mod.rs:224-231): CellID::from_point of the 8 corners (xyz each), normalize,
 * rect_bound of the union. */
int pcv_s2_corners_rect_host(const double corners[24], double rect[4]);
/* Rect::intersects_cell: *intersects = 1 / 0. */
int pcv_s2_rect_intersects_cell_host(const double rect[4], uint64_t cell, int* intersects);
/* CellUnion::normalize in place: sorted, cells inside another dropped, four siblings merged into their parent;
 * *num_cells is the length going in and coming out. */
int pcv_s2_union_normalize_host(uint64_t* cells, uint32_t* num_cells);
/* CellUnion::intersects_cellid for n cell ids against `cells` (ascending, as pcv_s2_union_contains takes them). */
int pcv_s2_union_intersects_host(const uint64_t* cells, uint32_t num_cells, uint64_t n, const uint64_t* ids, uint8_t* intersects);
/* cells_intersecting_polyhedron(cells, cube.to_aabb()) for n cubes (min xyz, edge; n x 4 doubles): the 8 corners' leaf
 * cells, normalized, their rect bound, Rect::intersects_cell against every cell of the union (ascending, level >= 1, not
 * normalized). The chain the device walks with: a cell union's node list over an octree is the breadth-first walk over this
 * predicate on the nodes' bounding cubes, bit for bit. */
int pcv_s2_union_intersects_cubes_host(const uint64_t* cells, uint32_t num_cells, uint64_t n, const double* cubes, uint8_t* intersects);

/* S2Cells::nodes_in_location (mod.rs:160-241) for many locations in one call: first the shapes (nullable), then num_unions
 * cell unions, union u being union_cells[union_first[u] .. union_first[u + 1]) in HOST memory, ascending by id, union_first[0] = 0.
 *   AllPoints                                 every cell of the cloud
 *   Aabb / Obb / Frustum / WebMercatorRect    the cells that the rect of pcv_s2_corners_rect_host(corners of the shape) intersects
 *                                             (Rect::intersects_cell); a frustum whose matrix is not invertible has none
 *   a cell union                              the cells with CellUnion::intersects_cellid
 * counts[l] = number of cells of location l (may exceed `capacity`); cells[l * capacity ..] = the first min(counts[l],
 * capacity) of them as indices into pcv_s2_cells' arrays, ASCENDING (the reference lists them in its hash map's order); the
 * rest of a row is unspecified. counts and cells are host arrays. The first geometric call builds the cloud's cell table on the
 * device (240 bytes per cell) and keeps it. A cloud with a level-0 cell takes AllPoints and unions only. The lists equal
 * pcv_s2_cells_in_location_host's, bit for bit. */
int pcv_s2_cells_in_location(pcv_s2_cloud* cloud, const pcv_shapes* shapes, uint32_t num_unions, const uint32_t* union_first,
                             const uint64_t* union_cells, uint32_t capacity, uint32_t* counts, uint32_t* cells);
/* The same over plain host arrays: the cloud's cell ids (ascending), and per shape its PCV_SHAPE_* kind, the `valid` flag and
 * the 24 doubles of its corners as pcv_shapes_get_ex returns them. */
int pcv_s2_cells_in_location_host(uint64_t num_cells, const uint64_t* cell_ids, uint32_t num_shapes, const int32_t* kinds,
                                  const int32_t* valid, const double* corners, uint32_t num_unions, const uint32_t* union_first,
                                  const uint64_t* union_cells, uint32_t capacity, uint32_t* counts, uint32_t* cells);

/* The batched point query over an S2 cell cloud, shaped like pcv_query_batch_*: FilteredIterator over NodeIterator with
 * Encoding::Plain (src/iterator.rs:96-119, src/s2_cells/mod.rs:171-191, stream_points_for_query_in_node) for every location
 * of one call — the shapes (nullable) first, then the unions, given as for pcv_s2_cells_in_location. intervals: NULL, or 2
 * doubles per location, a closed interval on intensity, read where interval_used is NULL or interval_used[l] != 0; an
 * interval on a cloud without intensity is PCV_E_INVALID. One segment per (location, cell of its pcv_s2_cells_in_location
 * list), locations one after another, cells ascending; a segment holds the cell's points, in file order, that pass
 * `contains` (the per-point tests of pcv_cull_points, pcv_wmr_contains, pcv_s2_union_contains) and the interval — positions are
 * the stored f64, untouched. Segments without points are present. The batch reads the cloud's blobs: free it first. */
typedef struct pcv_s2_query pcv_s2_query;
int pcv_s2_query_run(pcv_s2_cloud* cloud, const pcv_shapes* shapes, uint32_t num_unions, const uint32_t* union_first,
                     const uint64_t* union_cells, const double* intervals, const uint8_t* interval_used, pcv_s2_query** out);
int pcv_s2_query_sizes(const pcv_s2_query* q, uint64_t* num_segments, uint64_t* num_points);
/* location_first_segment[locations + 1], segment_cell[num_segments] (indices into pcv_s2_cells' arrays),
 * segment_offset[num_segments + 1] (the u64 scan of the segments' sizes); host arrays, any may be NULL. */
int pcv_s2_query_segments(const pcv_s2_query* q, uint64_t* location_first_segment, uint32_t* segment_cell, uint64_t* segment_offset);
/* The points of segments [first_segment, first_segment + num_segments) into buffers that live where `mem` says (any may be
 * NULL): x / y / z planes, rgb at 3 bytes, intensity. A range past the end, more points than `capacity`, or `intensity` on a
 * cloud without it is PCV_E_INVALID and writes nothing. */
int pcv_s2_query_points(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, uint64_t capacity, int mem, double* x,
                        double* y, double* z, uint8_t* rgb, float* intensity);
void pcv_s2_query_free(pcv_s2_query* q);

/* ---- S2 cell clouds: typed point attributes ------------------------------------- */
/* S2Splitter::write regroups EVERY attribute of a PointsBatch (src/read_write/s2.rs:85-107), get_meta lists them in meta.pb
 * (S2Meta.attributes, proto.proto:92-133) and a PointQuery filters on any scalar one (src/iterator.rs:66-119,
 * src/s2_cells/mod.rs:171-191). `color` (U8Vec3) and `intensity` (F32) stay the built-in columns of pcv_points; every other
 * column is an "extra": { name, data_type, data }.
 *   data_type  the proto enum value (src/attributes.rs:8-21): U8 1, U16 2, U32 3, U64 4, I8 6, I16 7, I32 8, I64 9, F32 11,
 *              F64 12, U8Vec3 27, F64Vec3 38 — elements of 1, 2, 4, 8, 1, 2, 4, 8, 4, 8, 3 and 24 bytes (attributes.rs:64-73);
 *              anything else is PCV_E_INVALID "Attribute data type invalid"
 *   name       not `color`, `intensity`, `position`, `xyz`, `rgb` or `meta`; 1 ..= 64 bytes; no '/', '.' or NUL inside; unique;
 *              at most PCV_S2_MAX_EXTRAS per cloud — each violation is PCV_E_INVALID with a message naming the attribute
 *   data       n elements, little endian, where points->mem says
 * A cell's file is `<token>.<name>`: the values of the cell's points in file order (src/lib.rs:74-80, read_write/raw.rs).
 * xray reads the extras through pcv_xray_run_s2_ex (filters and binning on any scalar one). Out of scope: clouds without
 * `color`; vector attributes as filters or bins; the octree path, which is fixed to color and
 * intensity as the reference's is (src/octree/mod.rs:63-72). */
#define PCV_ATTR_U8 1
#define PCV_ATTR_U16 2
#define PCV_ATTR_U32 3
#define PCV_ATTR_U64 4
#define PCV_ATTR_I8 6
#define PCV_ATTR_I16 7
#define PCV_ATTR_I32 8
#define PCV_ATTR_I64 9
#define PCV_ATTR_F32 11
#define PCV_ATTR_F64 12
#define PCV_ATTR_U8VEC3 27
#define PCV_ATTR_F64VEC3 38
#define PCV_S2_MAX_EXTRAS 16
#define PCV_S2_MAX_ATTR_NAME 64
typedef struct pcv_attribute {
  const char* name;
  int32_t data_type; /* PCV_ATTR_* */
  uint32_t reserved; /* 0 */
  const void* data;  /* n elements where points->mem says */
} pcv_attribute;
/* pcv_s2_split with extras (s2.rs:85-107): every column regrouped as the points are, out[slot] = in[pcv_s2_order[slot]]. With
 * num_attrs == 0 it is pcv_s2_split, bit for bit. */
int pcv_s2_split_ex(pcv_ctx* ctx, const pcv_points* points, const pcv_attribute* attrs, uint32_t num_attrs, uint32_t split_level,
                    pcv_s2_cloud** out);
/* Host only, no context: the rules above on a list of extras (names, data types, count, repeats; `data` is not read) — what
 * pcv_s2_split_ex and pcv_s2_stream_append_ex check first, with their messages (pcv_host_last_error). */
int pcv_s2_attributes_check_host(const pcv_attribute* attrs, uint32_t num_attrs);
/* pcv_s2_stream_append with extras. The first non-empty batch (in PCV_S2_APPEND mode, the directory) fixes the attribute set: a
 * later batch whose extra has another type, or a name the stream does not know, is PCV_E_INVALID "S2Splitter received
 * incompatible data types for attribute NAME (batch K of the stream)" (s2.rs:155). A batch that LACKS an extra of the stream is
 * refused in the same words (a departure: the reference lets it through, and the cell's files then disagree in length). The
 * stream stays usable after a refusal. pcv_s2_stream_append is this call with num_attrs == 0. */
int pcv_s2_stream_append_ex(pcv_s2_stream* stream, const pcv_points* batch, const pcv_attribute* attrs, uint32_t num_attrs);
/* The extras of a cloud, ascending by name (bytewise): *count, and — where non-NULL, PCV_S2_MAX_EXTRAS entries each — the names
 * (owned by the cloud, valid until it is freed) and the data types. */
int pcv_s2_attributes(const pcv_s2_cloud* cloud, uint32_t* count, const char** names, int32_t* data_types);
/* One extra of cells [first_cell, first_cell + num_cells) as it stands in the cells' files (lib.rs:74-80), one cell after the
 * other, into `out` where `mem` says; `capacity` counts elements. pcv_s2_cell_points' rules; an unknown name is PCV_E_INVALID
 * "Data type for attribute 'NAME' not found." (lib.rs:94). On a cloud opened from a directory the extra's files are read (and
 * uploaded) when a call first names that extra or the cloud is written — pcv_s2_open_dir itself reads meta.pb alone, so a
 * directory whose extra files are damaged still opens; a file of the wrong size, or a missing file of a cell with points, is
 * PCV_E_IO naming the file. A host-only cloud serves this call into host memory. */
int pcv_s2_cell_attribute(pcv_s2_cloud* cloud, const char* name, uint64_t first_cell, uint64_t num_cells, uint64_t capacity, int mem,
                          void* out);
/* pcv_s2_write_dir, the flushes of a stream and pcv_s2_stream_finish write `<token>.<name>` per extra and list the extras in
 * meta.pb after color and intensity, ascending by name; a cloud without extras writes the bytes it wrote before.
 * pcv_s2_open_dir keeps the extras that meta.pb lists: entries named `color` or `intensity` of another type are skipped, as
 * are entries that break the rules above. Writing an opened cloud reads every extra's files (a damaged one is PCV_E_IO); an
 * extra of which the directory holds no file at all has nothing to carry over and is left out of what is written. */

/* One ClosedInterval<f64> of a PointQuery's filter_intervals (iterator.rs:66-119): location `location` keeps a point only if
 * `attribute` of it, converted as Rust's `as f64` (round to nearest even for U64 / I64, exact for every other type), lies in
 * [lo, hi]. NaN (a value, or a bound) keeps nothing. */
typedef struct pcv_s2_filter {
  uint32_t location;
  uint32_t reserved; /* 0 */
  const char* attribute;
  double lo, hi;
} pcv_s2_filter;
/* pcv_s2_query_run with filters on any scalar attribute: the filters of one location are ANDed with `contains`
 * (iterator.rs:109-115). With num_filters == 0 it is pcv_s2_query_run with intervals == NULL; a filter on "intensity" is
 * pcv_s2_query_run's interval. PCV_E_INVALID: an unknown name ("Data type for attribute 'NAME' not found.", lib.rs:94); a
 * vector attribute, `color` included (the reference reaches unimplemented!()); two filters on one (location, attribute); a
 * location past the end. */
int pcv_s2_query_run_ex(pcv_s2_cloud* cloud, const pcv_shapes* shapes, uint32_t num_unions, const uint32_t* union_first,
                        const uint64_t* union_cells, const pcv_s2_filter* filters, uint32_t num_filters, pcv_s2_query** out);
/* One extra of the kept points of segments [first_segment, first_segment + num_segments), in segment order, into `out` where
 * `mem` says; `capacity` counts elements. pcv_s2_query_points' rules. */
int pcv_s2_query_attribute(pcv_s2_query* q, const char* name, uint64_t first_segment, uint64_t num_segments, uint64_t capacity, int mem,
                           void* out);
/* Host only, no context: keep[i] &= (data[i] as f64) in [lo, hi] for n values of a scalar data_type — the twin of the device's
 * filter, from the same function. A vector type is PCV_E_INVALID. */
int pcv_s2_filter_keep_host(int32_t data_type, uint64_t n, const void* data, double lo, double hi, uint8_t* keep);

/* ---- xray over S2 cell clouds -------------------------------------------------------- */
/* build_xray_quadtree's leaf level over S2 cell clouds: PointCloudClient opens every location as an S2Cells cloud when the
 * first one's meta.pb says so (point_cloud_client/src/lib.rs:107-132), and the tile queries run over either kind
 * (xray/src/generation.rs:464-513, 557-648). pcv_xray_run_ex with the clouds in place of the octrees (coloring nullable: then
 * colored_with_intensity is refused, as by pcv_xray_run_many): the bounding box is the first cloud's meta box grown by every
 * cloud's min and then its max in list order; query_from_global, root_level / root_index, leaf geometry and backgrounds as
 * in pcv_xray_run. One location per leaf tile (an Aabb, or an Obb with query_from_global), the intensity interval on every
 * location, every cloud through the machinery of pcv_s2_query_run: a tile sees the points of the cells that
 * pcv_s2_cells_in_location lists for its shape, and only those (the reference's misses included), filtered by `contains` and
 * the interval, their stored f64 positions untouched. A tile is created iff the kept points summed over the clouds are
 * > 0; kept, drawn and negative are sums over the clouds. All four strategies, binning and the negative-intensity rule
 * of pcv_xray_run_ex apply unchanged; each raster pass is one launch per tile group whatever num_clouds. The result is
 * an ordinary built pcv_xray, on which parents, node images, directories, merge and inpaint work, and holds no reference to
 * the clouds. PCV_E_INVALID with a message and nothing left allocated: num_clouds == 0 ("No locations specified for point
 * cloud client."), more than PCV_XRAY_MAX_TREES clouds, a null cloud, a cloud of another context, a host-only cloud
 * (opened with a NULL context), a strategy, filter or binning that reads intensity when some cloud has none,
 * pcv_xray_check_params_ex's own refusals, and a cloud with a level-0 cell (pcv_s2_cells_in_location's refusal of
 * geometric locations). Out of device memory is PCV_E_OOM with nothing left allocated. */
int pcv_xray_run_s2(pcv_ctx* ctx, pcv_s2_cloud* const* clouds, uint32_t num_clouds, const pcv_xray_params* params,
                    const pcv_xray_coloring* coloring /* nullable */, pcv_xray** out);
/* ---- xray over S2 cell clouds: filters and binning on any scalar attribute -------------- */
/* One --filter-interval <attribute>=<min>,<max> of build_xray_quadtree (xray/src/build_quadtree.rs:94-101): a
 * ClosedInterval<f64> on a scalar attribute of the clouds, an extra or `intensity`. */
typedef struct pcv_xray_filter {
  const char* attribute;
  double lo, hi;
} pcv_xray_filter;
/* pcv_xray_run_s2 with a list of filters and with binning on any scalar attribute. With num_filters == 0 and a
 * binning_attribute that is NULL or "intensity" it is pcv_xray_run_s2, byte for byte. Otherwise:
 *   binning   coloring->binning_attribute names a scalar attribute of every cloud, an extra or `intensity`; the bin of a
 *             point is `(value as f64 / bin_size) as i64` (BinnedColoringStrategy::bins, xray/src/generation.rs:138-157;
 *             pcv_xray_bins_host is the same function), each cloud converting with its own data type, so two clouds may hold
 *             one name as I64 and as U64. colored and colored_with_intensity read it; xray and height_stddev ignore it and
 *             their bytes do not change (the name is checked all the same).
 *   filters   every filter applies to every tile location of every cloud and is ANDed with `contains` (FilteredIterator over
 *             filter_intervals, generation.rs:478-487), by pcv_s2_query_run_ex's test (pcv_s2_filter_keep_host);
 *             params->interval_attribute ("intensity" or NULL) is ANDed with the list. A tile is created iff the kept points
 *             summed over the clouds are > 0, so filters remove tiles from the created set.
 * PCV_E_INVALID with a message and nothing left allocated: a filter attribute missing from some cloud ("Data type for
 * attribute 'NAME' not found.", src/lib.rs:94) or a binning attribute missing from one ("Binning attribute needs to be
 * available in points batch.", generation.rs:146), each naming the cloud's index; a vector attribute, `color` included; two
 * filters on one attribute (an entry on `intensity` beside interval_attribute counts as such); a filter with a NULL name;
 * and every refusal of pcv_xray_run_s2. A cloud opened from a directory loads the columns the run reads, and only those,
 * before any raster work: a damaged or missing file is PCV_E_IO naming the file, and the cloud stays usable.
 * Out of scope: vector attributes; the octree path (pcv_xray_run, _run_many, _run_ex and pcv_xray_check_params[_ex] keep
 * refusing every attribute but intensity, as an octree carries nothing else); xray over clouds without `color`. */
int pcv_xray_run_s2_ex(pcv_ctx* ctx, pcv_s2_cloud* const* clouds, uint32_t num_clouds, const pcv_xray_params* params,
                       const pcv_xray_coloring* coloring /* nullable */, const pcv_xray_filter* filters, uint32_t num_filters,
                       pcv_xray** out);
/* Host only: the checks of that call that need no device, given per cloud the names and data types of its extras
 * (cloud t's are entries [extras_first[t], extras_first[t + 1]) of names / data_types) and whether it has intensity. */
int pcv_xray_check_attrs_host(const pcv_xray_params* params, const pcv_xray_coloring* coloring, const pcv_xray_filter* filters,
                              uint32_t num_filters, uint32_t num_clouds, const uint32_t* extras_first /* num_clouds + 1 */,
                              const char* const* names, const int32_t* data_types, const uint8_t* has_intensity, char* err,
                              uint64_t errcap);
/* Host only, no context: out[i] = (data[i] as f64 / bin_size) as i64 for n values of a scalar data_type, from the function the
 * device compiles: `as f64` exact but for U64 / I64 (round to nearest, ties to even), a correctly rounded f64 division
 * (bin_size is not validated: 0 gives +-inf or NaN), `as i64` truncating, saturating, NaN -> 0. A vector type is
 * PCV_E_INVALID. */
int pcv_xray_bins_host(int32_t data_type, uint64_t n, const void* data, double bin_size, int64_t* out);

/* ---- query results as PLY files ------------------------------------------------------- */
/* PlyNodeWriter with Encoding::Plain (src/read_write/ply.rs:559-732), the reference's way of handing a query result to another
 * program, over the results of pcv_query_batch_run and pcv_s2_query_run[_ex]; the rows are packed on the device.
 *   row      position as three doubles x y z, then the attributes ascending by name (bytewise: BTreeMap order), each as its
 *            little-endian bytes, no padding; `color` and `intensity` take their place among the extras by name. Bits are
 *            copied: NaN payloads and -0.0 survive.
 *   header   "ply\nformat binary_little_endian 1.0\nelement vertex " + the count as 20 zero-padded digits + "\n", `property
 *            double x|y|z`, per attribute `property uchar red|green|blue` for color, `property <type> <name>0|1|2` for any
 *            other vector, `property <type> <name>` for a scalar (type words: ply.rs:582-593), "end_header\n".
 *   body     the rows, then one "\n" (ply.rs:646); the count field is patched last (:647-658).
 *   attributes  NULL: every attribute the cloud has (an octree: color, and intensity if it has it; an S2 cloud: those and every
 *            extra). Otherwise exactly the named ones (PointQuery::attributes; none: positions only), in any order. An unknown
 *            name is PCV_E_INVALID "Data type for attribute 'NAME' not found." (lib.rs:94), a repeated one PCV_E_INVALID. A cloud
 *            opened from a directory loads the named extras only.
 * The rows alone, into a host or device buffer of capacity_bytes: row r of the output is point r of segments [first_segment,
 * first_segment + num_segments), at r * *stride. pcv_query_batch_points' rules: a range past the end, or more rows than
 * the capacity holds, is PCV_E_INVALID and writes nothing. *stride and *num_rows (nullable) are set whenever the range and the
 * attributes are valid, also when the capacity is too small: they say what the range needs. */
int pcv_query_batch_ply_rows(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const char* const* attributes,
                             uint32_t num_attributes, uint64_t capacity_bytes, int mem, void* out, uint32_t* stride, uint64_t* num_rows);
int pcv_s2_query_ply_rows(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const char* const* attributes,
                          uint32_t num_attributes, uint64_t capacity_bytes, int mem, void* out, uint32_t* stride, uint64_t* num_rows);
/* The file. The rows are cut into pieces of at most chunk_points rows (0: 2^20), at any row — neither a segment nor a chunk
 * of the query sets a piece's size; two device buffers and two pinned blocks alternate, piece k + 1 packed while piece k is
 * copied and written by the context's host threads, so device and pinned memory are O(chunk_points * stride) whatever the
 * result's size.
 *   PCV_PLY_TRUNCATE  the file is written anew. A range without points leaves no file behind (DataWriter's drop,
 *                     node_writer.rs:78-84) and touches none that is there.
 *   PCV_PLY_APPEND    OpenMode::Append (ply.rs:663-689): the old count is read from the fixed field, the rows go over the
 *                     trailing newline, the count becomes the sum. A missing file, or one shorter than the fixed prefix, is
 *                     written anew. A departure: the header that the requested attributes give is first compared with the
 *                     file's, byte for byte, and a file of other columns is PCV_E_INVALID naming the first property line that
 *                     differs (the reference appends whatever it is given). A range without points leaves the file as it is.
 * A failure after the file was opened removes a truncated file and cuts an appended one back to its old length and count;
 * PCV_E_IO names the path. *written (nullable): the rows written. Out of scope: the ScaledToCube position encodings of
 * PlyNodeWriter (node files, not an exchange format), ascii and big-endian bodies, host-only S2 clouds. */
#define PCV_PLY_TRUNCATE 0
#define PCV_PLY_APPEND 1
typedef struct pcv_ply_write_params {
  uint32_t struct_size;          /* sizeof(pcv_ply_write_params) */
  int32_t open_mode;             /* PCV_PLY_TRUNCATE / PCV_PLY_APPEND */
  const char* const* attributes; /* NULL: every attribute of the cloud */
  uint32_t num_attributes;
  uint32_t reserved;
  uint64_t chunk_points; /* rows per piece; 0 = the default */
} pcv_ply_write_params;
int pcv_query_batch_write_ply(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const char* path,
                              const pcv_ply_write_params* params, uint64_t* written);
int pcv_s2_query_write_ply(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const char* path,
                           const pcv_ply_write_params* params, uint64_t* written);
/* Host only, no context (messages: pcv_host_last_error). The layout of a row for n (name, PCV_ATTR_* data type) pairs in any
 * order: offsets[i] is where the i-th GIVEN attribute stands in the row, *stride the row's bytes (24 with n == 0). A data
 * type of 0 is PCV_E_INVALID "Data type for attribute 'NAME' not found.", any other unknown one "Attribute data type
 * invalid", a repeated name PCV_E_INVALID. */
int pcv_ply_layout_host(const char* const* names, const int32_t* data_types, uint32_t n, uint32_t* offsets, uint32_t* stride);
/* The header for `count` vertices: *len its length, the first min(cap, *len) bytes into buf (nullable with cap == 0). */
int pcv_ply_header_host(const char* const* names, const int32_t* data_types, uint32_t n, uint64_t count, char* buf, uint64_t cap,
                        uint64_t* len);
/* What PCV_PLY_APPEND checks before it touches `path`: *old_count the file's count (0 for a missing file or one shorter
 * than the fixed prefix). PCV_E_INVALID: no PLY of this writer, a header of other columns (the message names the first
 * line that differs), a length that is not header + count rows + newline. PCV_E_IO: the file cannot be read. */
int pcv_ply_append_check_host(const char* path, const char* const* names, const int32_t* data_types, uint32_t n, uint64_t* old_count);
/* The device pool of a context: the bytes handed out now and the most since the last reset (reset_peak != 0 sets the mark to the
 * current figure after reading it). Either output may be NULL. */
int pcv_ctx_pool_stats(pcv_ctx* ctx, uint64_t* live_bytes, uint64_t* peak_bytes, int reset_peak);
/* The pool's contract: a block comes with arbitrary contents, and a request owns exactly the bytes it asked for. The guard is
 * the test hook that holds every kernel to it (DESIGN "The pool's contract"); off unless set, no environment variable sets it.
 *   mode 0  off.
 *   mode 1  fill: every device block handed out, fresh or recycled, holds `fill` (0..255) over the requested bytes before the
 *           request returns (set on the context's stream, and waited for); pinned result blocks likewise, by the host. The
 *           staging blocks that callers keep across calls are left alone; the node-table block of the build is filled.
 *   mode 2  fill and fence: also 256 canary bytes in front of the pointer handed out, and canary bytes from pointer + requested
 *           to the end of the block, at least 256 past the rounded request. pcv_ctx_pool_stats counts the fences.
 * Legal only while no block of the pool is live (PCV_E_INVALID otherwise); trims the cache, and resets the serial numbers and
 * the report. With mode 2 the fences of a block are copied back and scanned when it is released (after a wait for the
 * context's streams), at pcv_ctx_destroy for blocks still live, and for all live blocks by pcv_ctx_pool_guard_check. A damaged
 * fence is counted, never an error. */
int pcv_ctx_set_pool_guard(pcv_ctx* ctx, int mode, int fill);
int pcv_ctx_pool_guard_check(pcv_ctx* ctx);
/* *checked blocks whose fences were scanned, *damaged those with a byte that is not the canary (a live block scanned twice
 * counts twice); of the first damaged one: the bytes it asked for, its serial number (the first request after
 * pcv_ctx_set_pool_guard is 1), and the first damaged byte relative to the pointer handed out (negative: the front fence,
 * which is scanned first). Any output may be NULL. */
int pcv_ctx_pool_guard_report(pcv_ctx* ctx, uint64_t* checked, uint64_t* damaged, uint64_t* first_bytes, uint64_t* first_serial,
                              int64_t* first_offset);
/* Mode 2 only; host code and memsets, no kernel. Requests `bytes`, copies the block back and requires `fill` in every byte,
 * writes another pattern over it and releases it; requests `bytes` again, which must return the cached block, filled again;
 * sets the byte at pointer + offset (inside the block: [-256, block - 256)) and releases the block. Serial numbers 1 and 2 when
 * called right after pcv_ctx_set_pool_guard; the report then names the second. PCV_E_INVALID with a message for a step that
 * fails. */
int pcv_ctx_pool_guard_selftest(pcv_ctx* ctx, uint64_t bytes, int64_t offset);

/* ---- terrain layers -------------------------------------------------------------------- */
/* The directory `sdl_viewer --terrain <dir>` draws (sdl_viewer/src/terrain_drawer/{read_write,layer,mod}.rs,
 * graphic/tiled_texture_loader.rs, shaders/terrain.{vs,gs}): a sparse, tiled elevation model, per grid vertex a height, a
 * colour and the quad adjacency mask the geometry shader ANDs over a triangle. The reference ships the reader only; the
 * reduction from points to vertices is this library's and is stated here.
 *   per point, in f64, nothing fused:  d = p - t;  l = M d, each row as (m_r0 d_x + m_r1 d_y) + m_r2 d_z;
 *     u = (l_x - o_x) / res;  v = (l_y - o_y) / res;  i = floor(u + 0.5);  j = floor(v + 0.5);  h = (float)(l_z - o_z)
 *   with M, t the 12 doubles of pcv_terrain_frame_host (terrain_from_world). The tile of vertex (i, j) is (floor(i / T),
 *   floor(j / T)). Dropped and counted as `outside`: u, v or h not finite (or |i|, |j| >= 2^62), a vertex outside the range
 *   declared at begin, |l_z - o_z| >= 2^21 with PCV_TERRAIN_MEAN.
 *   count    points on the vertex; the vertex is SET iff count >= min_points
 *   MAX/MIN  the point with the largest / smallest h in f32 total order (-0 < +0), among equal h the largest (r, g, b);
 *            height = its h, colour = its rgb, alpha 255: independent of order, of the split over calls and of scheduling
 *   MEAN     hq = rint((l_z - o_z) * 1024) as i64; height = (float)(((double)sum hq / (double)count) / 1024.0);
 *            channel = (sum_c + count / 2) / count; alpha 255; all sums exact integers
 *   unset    height 0.0f, mask 0, colour 0 0 0 0
 *   mask     quad (qx, qy), corners (qx .. qx + 1, qy .. qy + 1), is rendered iff its four corners are set; a vertex's mask is
 *            the OR over its up to four adjacent rendered quads of bit (qx mod 3) + 3 (qy mod 3), floor mod on GLOBAL indices,
 *            stored as the f32 of that integer (<= 511) in the height texture's second channel. */
#define PCV_TERRAIN_MAX 0
#define PCV_TERRAIN_MIN 1
#define PCV_TERRAIN_MEAN 2
typedef struct pcv_terrain_params {
  uint32_t tile_size;           /* T, 1 ..= 4096 vertices per tile edge */
  uint32_t statistic;           /* PCV_TERRAIN_MAX / _MIN / _MEAN */
  double resolution_m;          /* > 0 */
  double origin[3];             /* the grid origin, in the terrain frame */
  double world_from_terrain[7]; /* Isometry3: translation xyz, unit quaternion ijkw (as pcv_xray_params.query_from_global) */
  uint32_t min_points;          /* >= 1 */
  uint32_t reserved;
  uint64_t max_pool_bytes;      /* cap on the per-vertex storage of the touched tiles; 0: 2 GiB */
  uint64_t staging_points;      /* points per piece of the two query adders; 0: 2^22 */
} pcv_terrain_params;
typedef struct pcv_terrain_info {
  uint64_t points_added;   /* every point handed in, dropped ones included */
  uint64_t outside;        /* the dropped ones */
  uint64_t set_vertices;   /* after finish */
  uint64_t rendered_quads; /* after finish */
  uint64_t tiles;          /* after finish: tiles with a set vertex; before: tiles touched so far */
  uint64_t pool_bytes;     /* per-vertex storage held for the touched tiles */
  int32_t vertex_min[2], vertex_max[2]; /* the declared range when it fits i32 (else saturated) */
  uint32_t finished, reserved;
} pcv_terrain_info;
typedef struct pcv_terrain pcv_terrain;
/* The world box's eight corners go through the chain; the vertex range is their (i, j) hull widened by one vertex, the
 * tile-slot table is dense over the range's tiles. PCV_E_INVALID: what pcv_terrain_check_params_host refuses, a box with a
 * non-finite corner, tile positions outside i32, more than 2^22 tiles in the range. Per-vertex storage is allocated for the
 * tiles a point touches only. */
int pcv_terrain_begin(pcv_ctx* ctx, const pcv_terrain_params* params, const double bbox_min[3], const double bbox_max[3], pcv_terrain** out);
/* n points: f64 planes and 3-byte colours that live where `mem` says. More than 2^32 - 1 points in total is PCV_E_INVALID
 * (nothing of the call is added). Touched tiles that would take the storage past max_pool_bytes are PCV_E_OOM: everything
 * the terrain holds on the device is released, and the handle can only be freed. */
int pcv_terrain_add_points(pcv_terrain* t, uint64_t n, const double* x, const double* y, const double* z, const uint8_t* rgb, int mem);
/* The points of segments [first_segment, first_segment + num_segments) of a query result, pulled into a device staging
 * buffer piece by piece: a piece is at most staging_points rows of the result, cut at any row — neither a segment nor a chunk
 * of the query sets its size — packed by the PLY output's packer (pcv_*_ply_rows' kernels) as x y z r g b rows and spread into
 * planes, so the staging costs O(staging_points) (54 bytes per point) whatever the result's size. The result's bytes do not
 * depend on the pieces. */
int pcv_terrain_add_query_batch(pcv_terrain* t, pcv_query_batch* batch, uint64_t first_segment, uint64_t num_segments);
int pcv_terrain_add_s2_query(pcv_terrain* t, pcv_s2_query* query, uint64_t first_segment, uint64_t num_segments);
/* Resolves the vertices, runs the mask pass (it reads set flags through the tile table: a vertex on a tile edge depends on up
 * to three other tiles) and keeps the tiles with a set vertex on the device, ascending by (x, y). No points after it. A finish
 * that fails releases everything the terrain holds on the device, and the handle can only be freed. */
int pcv_terrain_finish(pcv_terrain* t);
int pcv_terrain_info_get(const pcv_terrain* t, pcv_terrain_info* out);
/* After finish. positions: 2 x i32 per tile (host). heights: tiles x T x T x 2 f32 (height, mask); colors: tiles x T x T x 4
 * u8; counts: tiles x T x T u32; row = j mod T, column = i mod T (ImageBuffer's row-major layout), into memory that lives
 * where `mem` says. A range past the end is PCV_E_INVALID and writes nothing. */
int pcv_terrain_tiles(const pcv_terrain* t, uint64_t capacity, int32_t* positions, uint64_t* num_tiles);
int pcv_terrain_heights(pcv_terrain* t, uint64_t first_tile, uint64_t num_tiles, int mem, float* out);
int pcv_terrain_colors(pcv_terrain* t, uint64_t first_tile, uint64_t num_tiles, int mem, uint8_t* out);
int pcv_terrain_counts(pcv_terrain* t, uint64_t first_tile, uint64_t num_tiles, int mem, uint32_t* out);
/* x{:08}_y{:08}.height (T T 2 little-endian f32) and .color (T T 4 bytes) per tile, the sign counting toward the width as in
 * Rust's formatting of an i32, and meta.json (pcv_terrain_meta_json_host); the files are written by the context's host
 * threads. A terrain without a set vertex writes meta.json with an empty tile list only. PCV_E_IO names the file. */
int pcv_terrain_write_dir(pcv_terrain* t, const char* directory);
void pcv_terrain_free(pcv_terrain* t);
/* Host only, no context (messages: pcv_host_last_error). PCV_E_INVALID: tile_size 0 or above 4096, resolution_m <= 0 or not
 * finite, a non-finite origin or translation, a quaternion whose squared norm is further than 1e-9 from 1, min_points 0, an
 * unknown statistic. */
int pcv_terrain_check_params_host(const pcv_terrain_params* params);
/* terrain_from_world as 12 doubles: the rotation rows m00 m01 m02 m10 .. m22, then t (= the translation of
 * world_from_terrain): l = M (p - t). The formula is in DESIGN §9g; matrices of 90-degree turns come out in {0, +-1}. */
int pcv_terrain_frame_host(const pcv_terrain_params* params, double frame[12]);
/* The chain for n points: i, j (0 where ok is 0), h, and ok[k] = 1 iff u, v, h are finite and |i|, |j| < 2^62. Any output
 * may be NULL. Neither the declared range nor MEAN's height bound is applied. */
int pcv_terrain_vertex_host(const pcv_terrain_params* params, uint64_t n, const double* x, const double* y, const double* z,
                            int64_t* i, int64_t* j, float* h, uint8_t* ok);
/* A set bitmap (w x h bytes, row = j - j0, column = i - i0, nonzero = set; everything outside the window unset) into the
 * masks of its vertices (w x h u32). */
int pcv_terrain_quad_masks_host(int64_t i0, int64_t j0, uint32_t w, uint32_t h, const uint8_t* set, uint32_t* masks);
/* "x{:08}_y{:08}" for a tile position, NUL-terminated (at most 23 bytes with it). */
int pcv_terrain_tile_name_host(int32_t x, int32_t y, char* buf, uint64_t cap);
/* meta.json: {"tile_size":T,"world_from_terrain":{"rotation":[i,j,k,w],"translation":[x,y,z]},"origin":[x,y,z],
 * "resolution_m":r,"tile_positions":[[x,y],...]} — every f64 with the fewest of 15, 16 or 17 significant digits that parse
 * back to the same double, integral values with ".0". *len its length, the first min(cap, *len) bytes into buf. */
int pcv_terrain_meta_json_host(const pcv_terrain_params* params, uint64_t num_tiles, const int32_t* positions, char* buf, uint64_t cap,
                               uint64_t* len);
/* The reader of that schema (terrain_drawer/read_write.rs, serde_json): `len` bytes of meta.json, the five keys in any order,
 * world_from_terrain as {"rotation":[i,j,k,w],"translation":[x,y,z]} (its two keys in any order), unknown keys skipped.
 * Fills tile_size, resolution_m, origin and world_from_terrain of *params; statistic, min_points (1) and the limits are set
 * to their defaults, and the result goes through pcv_terrain_check_params_host. *num_tiles the tiles listed, the first
 * min(capacity, *num_tiles) positions into `positions` (nullable). PCV_E_INVALID names the key that is missing, of the
 * wrong type or cut off (pcv_host_last_error). */
int pcv_terrain_meta_read_host(const char* json, uint64_t len, pcv_terrain_params* params, uint64_t capacity, int32_t* positions,
                               uint64_t* num_tiles);
/* A finished terrain from tiles that were not built in this process: num_tiles positions (2 x i32 each, host), heights
 * (tiles x T x T x 2 f32) and colors (tiles x T x T x 4 u8) in the layout of pcv_terrain_heights / pcv_terrain_colors, in memory
 * that lives where `mem` says. The tiles are stored ascending by (x, y), whatever order they come in. It serves
 * pcv_terrain_tiles, _heights, _colors, _info_get (tiles and finished; the counts of a build are zero) and _write_dir, and is a
 * layer of pcv_render_views_terrain; pcv_terrain_counts and every pcv_terrain_add_* on it are PCV_E_INVALID with a message.
 * PCV_E_INVALID: what pcv_terrain_check_params_host refuses (a tile_size outside 1 ..= 4096 among it), a tile position given
 * twice, null arrays with num_tiles > 0, more than 2^22 tiles. */
int pcv_terrain_from_tiles(pcv_ctx* ctx, const pcv_terrain_params* params, uint64_t num_tiles, const int32_t* positions,
                           const float* heights, const uint8_t* colors, int mem, pcv_terrain** out);
/* pcv_terrain_from_tiles over a directory as pcv_terrain_write_dir leaves it: meta.json through the reader above, then
 * x{:08}_y{:08}.height / .color per listed tile. A file that is missing or unreadable is PCV_E_IO, one whose length is not
 * T T 8 / T T 4 bytes PCV_E_INVALID; both name the file. */
int pcv_terrain_open_dir(pcv_ctx* ctx, const char* directory, pcv_terrain** out);

/* ---- terrain layers in the viewer's frame (sdl_viewer --terrain) ---------------------------------
 * The viewer draws its terrain layers right after the points, under the same depth test, as a wireframe
 * (sdl_viewer/src/lib.rs:602-606, terrain_drawer/mod.rs:152-187, shaders/terrain.vs, terrain.gs, terrain.fs). The restatement:
 *  - window: l = M (c - t) for the view's camera position c (world frame) with pcv_terrain_frame_host's doubles; gx =
 *    floor((l_x - o_x) / res), gy likewise; pos = (gx, gy) - (window / 2, window / 2) (layer.rs:222-235);
 *  - vertices: window vertex (ax, ay) is global vertex pos + (ax, ay); height, mask and colour through the tile table, zeros
 *    where the tile is missing; loc = (o_x + res ((double)ax + (double)pos_x), .. , o_z + (double)height); world = M^T loc + t
 *    in f64, unfused; clip as a point's position (f64 dot, one rounding to f32); the mask is the stored f32 truncated to u32
 *    (negative, non-finite or >= 2^32 reads as 0);
 *  - triangles T1 = (ax,ay) (ax+1,ay) (ax,ay+1) and T2 = (ax+1,ay) (ax,ay+1) (ax+1,ay+1) of quad (ax, ay) are rendered iff the
 *    AND of their three masks is non-zero; every edge H (ax,ay)->(ax+1,ay), V (ax,ay)->(ax,ay+1), D (ax+1,ay)->(ax,ay+1) is
 *    drawn once iff a triangle that owns it is rendered; its index is 3 (ay window + ax) + kind (H 0, V 1, D 2);
 *  - clip, window transform and width-1 raster as a node outline's segment; colour per channel (float)c0 + s ((float)c1 -
 *    (float)c0) with s = t_in + t (t_out - t_in), clamped to [0, 255], plus 0.5, truncated; alpha 255; no gamma;
 *  - layers are drawn after all nodes (and outlines), in the order given; layer k of a view owns 3 window^2 consecutive draw
 *    ranks, a fragment's rank is its edge's index: at equal depth terrain loses to every point, outline and earlier layer.
 *    The limit of 2^32 - 1 ranks per view includes them. A view whose status is 1 or 2 draws no terrain. */
typedef struct pcv_render_terrain_layers {
  uint32_t num_layers;
  uint32_t window;                 /* the window's edge in vertices: even, 2 ..= 1024; the viewer's is 1024 */
  pcv_terrain* const* layers;      /* num_layers finished terrains of the context; a terrain may be given more than once */
  const double* camera_positions;  /* views x 3, host: the camera of every frustum, world frame */
} pcv_render_terrain_layers;
#define PCV_RENDER_TERRAIN_WINDOW 1024
/* Host only, no context: PCV_E_INVALID with the reason in `message` (NUL-terminated, cut to `capacity`; nullable) for a window
 * that is odd, 0 or above 1024, a null layer array or entry, null camera positions. A null `terrain` and num_layers == 0 are
 * valid: nothing is drawn. */
int pcv_render_check_terrain_host(const pcv_render_terrain_layers* terrain, char* message, uint64_t capacity);
/* Host only, no context: the window position of one camera over one layer's grid, pos = 2 x i64. PCV_E_INVALID "Terrain
 * location not representable." (layer.rs:176-183, 226-233) when gx or gy is not finite or |gx|, |gy| >= 2^53. */
int pcv_render_terrain_window_host(const pcv_terrain_params* params, const double camera_position[3], uint32_t window, int64_t pos[2]);
/* pcv_render_views_ex with terrain layers. A null `terrain` or num_layers == 0 is pcv_render_views_ex itself: the same
 * launches, the same bytes. The window vertices (24 bytes each, per view and layer) count against max_workspace_bytes beside
 * the key planes when views are grouped; a single view over the limit is PCV_E_OOM before anything is allocated. PCV_E_INVALID:
 * what pcv_render_check_terrain_host refuses, a layer that is not finished or of another context, a window position that is
 * not representable, 2^32 - 1 draw ranks or more in a view. The layers may be freed after the call. */
int pcv_render_views_terrain(pcv_ctx* ctx, const pcv_shapes* frusta, pcv_octree* tree, const pcv_render_params* params,
                             const pcv_render_overlay* overlay, const pcv_render_terrain_layers* terrain, pcv_render** out);
/* Per view and layer (each output nullable): the window position, the edges step 15 draws, those that survived the clip, the
 * pixels of the final image the layer won. Counters are zero for a view whose status is not 0. PCV_E_INVALID past the end. */
int pcv_render_terrain_info(pcv_render* r, uint32_t view, uint32_t layer, int64_t pos[2], uint64_t* edges_submitted,
                            uint64_t* edges_drawn, uint64_t* pixels_won);

/* Host only: which arm PointCloudClientBuilder::build (point_cloud_client/src/lib.rs:107-132) would take for this
 * directory's meta.pb: `version <= 11 || has_octree()` is PCV_CLOUD_OCTREE, anything else PCV_CLOUD_S2. The reference
 * opens every location as the first one's kind; the entry points here take one kind each, and the caller decides. A missing
 * or unreadable meta.pb is PCV_E_IO naming the file (pcv_host_last_error). */
#define PCV_CLOUD_OCTREE 0
#define PCV_CLOUD_S2 1
int pcv_cloud_kind(const char* directory, int* kind);

/* ---- map tiles ---------------------------------------------------------------------------- */
/* z/x/y PNG pyramids of Earth-fixed (ECEF) clouds, the tiles of a slippy web map. The reference has the coordinates
 * (src/math/web_mercator.rs: TILE_SIZE = 256 and MAX_ZOOM = 23 at :18-23, WebMercatorCoord::to_zoomed_coordinate at :70-77,
 * from_zoomed_coordinate at :84-93) and WebMercatorRect::from_zoomed_coordinates; it ships no generator. The product is this
 * library's and is stated here.
 *   pixel   (u, v) = the chain of pcv_wmr_project; S = 256 * 2^zoom; gx = floor(u S), gy = floor(v S) (exact: S is a power
 *           of two) = floor(to_zoomed_coordinate(zoom)). The point is DRAWN iff x, y, z, u S and v S are finite and u S, v S
 *           are >= 0 and < S, else it is DROPPED and counted (NaN or infinite coordinates, also where the chain's atan2
 *           would give them a finite (u, v); lng = pi; a clamped latitude whose v rounds outside). Its
 *           tile is (gx >> 8, gy >> 8), its pixel in the tile (gx & 255, gy & 255); row 0 is north. Tile membership equals
 *           what pcv_wmr_from_zoomed((256 x, 256 y), (256 (x + 1), 256 (y + 1)), zoom) keeps in a point query, bit for bit.
 *   value   per pixel the exact integer sums of r, g, b and the count n of its drawn points; the image is xray's `colored`
 *           (PCV_XRAY_FN_COLORED) of them, a pixel without a point is transparent, and pixels with alpha < 128 take
 *           `background`. The bytes depend on the multiset of points only. A pixel with more than 2^24 points fails finish.
 *   parents tile (x, y) of zoom k has the children (2x + dx, 2y + dy) of zoom k + 1; the 2:1 Lanczos3 resize of
 *           pcv_xray_build_parents over the quadtree index of pcv_maptiles_quad_index_host; a missing child is background.
 *   files   <dir>/<z>/<x>/<y>.png and <dir>/tiles.json (pcv_maptiles_json_host). */
#define PCV_MAPTILES_MAX_ZOOM 23
#define PCV_MAPTILES_TILE_PX 256
typedef struct pcv_maptiles_params {
  uint32_t zoom;            /* 0 ..= 23: the zoom the points are drawn at */
  uint32_t background;      /* packed RGBA8, r | g << 8 | b << 16 | a << 24; 0: transparent black */
  uint64_t max_tiles;       /* 1 ..= 2^22: tiles the points may touch (the tile table holds twice as many keys) */
  uint64_t max_pool_bytes;  /* cap on the accumulators of the touched tiles (1 MiB each); 0: 2 GiB */
  uint64_t staging_points;  /* points per piece (16 bytes of keys and staging each); 0: 2^22 */
} pcv_maptiles_params;
typedef struct pcv_maptiles_info {
  uint64_t points_added;    /* every point handed in, dropped ones included */
  uint64_t dropped;         /* after finish */
  uint64_t drawn;           /* after finish: points_added - dropped */
  uint64_t pool_bytes;      /* accumulators held for the touched tiles (none after finish) */
  uint32_t zoom, min_zoom;  /* min_zoom < zoom once pcv_maptiles_build_parents has run */
  uint32_t finished, reserved;
  uint64_t tiles[24];       /* per zoom; at `zoom` before finish: tiles touched so far */
} pcv_maptiles_info;
typedef struct pcv_maptiles pcv_maptiles;
/* PCV_E_INVALID: what pcv_maptiles_check_params_host refuses. No tile range is declared: tiles are found by a mark pass
 * into a device hash table keyed by (x, y), and accumulators are allocated for the tiles a point touches only. */
int pcv_maptiles_begin(pcv_ctx* ctx, const pcv_maptiles_params* params, pcv_maptiles** out);
/* n ECEF points: f64 planes and 3-byte colours that live where `mem` says, taken in pieces of staging_points. More than
 * 2^32 - 1 points in total is PCV_E_INVALID (nothing of the call is added). More than max_tiles touched tiles, or
 * accumulators past max_pool_bytes, is PCV_E_OOM: everything held on the device is released and the handle can only be freed. */
int pcv_maptiles_add_points(pcv_maptiles* m, uint64_t n, const double* x, const double* y, const double* z, const uint8_t* rgb, int mem);
/* The points of segments [first_segment, first_segment + num_segments) of a query result, pulled through a staging buffer
 * of staging_points rows filled by the PLY output's packer, as pcv_terrain_add_query_batch; pieces are cut at any row. */
int pcv_maptiles_add_query_batch(pcv_maptiles* m, pcv_query_batch* batch, uint64_t first_segment, uint64_t num_segments);
int pcv_maptiles_add_s2_query(pcv_maptiles* m, pcv_s2_query* query, uint64_t first_segment, uint64_t num_segments);
/* Accumulators -> RGBA8 images and u32 count planes of the touched tiles, ascending by (x, y). No points after it.
 * PCV_E_INVALID "choose a larger zoom": a pixel holds more than 2^24 points. A finish that fails releases everything held on
 * the device, and the handle can only be freed. */
int pcv_maptiles_finish(pcv_maptiles* m);
/* After finish: the levels zoom - 1 down to min_zoom (<= zoom; == zoom builds nothing). Calling it again with the same
 * min_zoom is PCV_OK; with another one PCV_E_INVALID. */
int pcv_maptiles_build_parents(pcv_maptiles* m, uint32_t min_zoom);
/* After finish. The tiles of `zoom` (min_zoom ..= zoom), 2 x u32 (x, y) each, ascending by (x, y), into host memory. */
int pcv_maptiles_tiles(const pcv_maptiles* m, uint32_t zoom, uint64_t capacity, uint32_t* xy, uint64_t* num_tiles);
/* Tiles [first, first + count) of that list: count x 256 x 256 x 4 bytes (row 0 north), into memory that lives where `mem`
 * says. pcv_maptiles_counts: count x 256 x 256 u32 points per pixel, of the tiles of the maximum zoom. */
int pcv_maptiles_images(pcv_maptiles* m, uint32_t zoom, uint64_t first, uint64_t count, int mem, uint8_t* rgba);
int pcv_maptiles_counts(pcv_maptiles* m, uint64_t first, uint64_t count, int mem, uint32_t* out);
/* Complete PNG files of tiles [first, first + count) of `zoom`, back to back in `out` (host; NULL: the offsets alone), file i
 * at offsets[i] .. offsets[i + 1] (count + 1 offsets), as pcv_xray_node_pngs; mode: PCV_XRAY_PNG_STORED or _DEFLATE. */
int pcv_maptiles_tile_pngs(pcv_maptiles* m, uint32_t zoom, uint64_t first, uint64_t count, int mode, uint64_t capacity, uint8_t* out,
                           uint64_t* offsets);
/* <directory>/<z>/<x>/<y>.png for every tile of every built zoom, encoded as pcv_maptiles_tile_pngs and written by the host
 * threads of the xray quadtree's writer (pcv_xray_write_dir_ex), then <directory>/tiles.json. PCV_E_IO names the file. */
int pcv_maptiles_write_dir(pcv_maptiles* m, const char* directory, int png_mode);
int pcv_maptiles_info_get(const pcv_maptiles* m, pcv_maptiles_info* out);
void pcv_maptiles_free(pcv_maptiles* m);
/* Host only, no context (messages: pcv_host_last_error). PCV_E_INVALID: zoom above 23, max_tiles 0 or above 2^22. min_zoom is
 * checked against zoom as pcv_maptiles_build_parents does; pass zoom itself where no parents are wanted. */
int pcv_maptiles_check_params_host(const pcv_maptiles_params* params, uint32_t min_zoom);
/* The pixel rule on the host, the kernels' twin (web_mercator.rs:70-77): gx, gy (u32, 0 where dropped) and ok (1 drawn,
 * 0 dropped) of n points; each output nullable. */
int pcv_maptiles_pixels_host(uint32_t zoom, uint64_t n, const double* x, const double* y, const double* z, uint32_t* gx, uint32_t* gy,
                             uint8_t* ok);
/* The xray quadtree index (pcv_xray_nodes' index at level `zoom`) of slippy tile (x, y), and back: digit 2 xbit + (1 - ybit)
 * per level from the most significant bit. PCV_E_INVALID: zoom above 23, x or y >= 2^zoom, index >= 4^zoom. */
int pcv_maptiles_quad_index_host(uint32_t zoom, uint32_t x, uint32_t y, uint64_t* index);
int pcv_maptiles_quad_tile_host(uint32_t zoom, uint64_t index, uint32_t* x, uint32_t* y);
/* tiles.json: {"scheme":"xyz","format":"png","tile_size":256,"minzoom":a,"maxzoom":z,"bounds":[west,south,east,north],
 * "tiles":{"<a>":[[x,y],...],...,"<z>":[...]}}. counts: tiles per zoom, a ..= z; xy: their (x, y), zoom after zoom. bounds in
 * degrees: the hull of the corners of the tiles of zoom z through pcv_wmr_to_lat_lng (from_zoomed_coordinate :84-93, then
 * to_lat_lng), zeros without a tile; doubles as in the terrain's meta.json. *len: the length; buf takes min(cap, *len) bytes. */
int pcv_maptiles_json_host(uint32_t min_zoom, uint32_t max_zoom, const uint64_t* counts, const uint32_t* xy, char* buf, uint64_t cap,
                           uint64_t* len);

/* ---- LAS point clouds as input ---------------------------------------------------------- */
/* ASPRS LAS 1.0 - 1.4, point data record formats 0 - 10, little endian, read at the fixed offsets of the public header block;
 * VLRs and EVLRs are skipped, a record longer than its format's minimum is read by stride. The records are decoded and filtered
 * on the device; the host parses the header and moves bytes. Not read: LAZ, extra-bytes descriptors, waveform data, CRS VLRs. */
typedef struct pcv_las_header {
  uint8_t version_major, version_minor;
  uint8_t point_format; /* 0 ..= 10 */
  uint8_t reserved0;
  uint16_t header_size;
  uint16_t record_length;
  uint32_t offset_to_points;
  uint32_t reserved1;
  uint64_t num_points; /* 1.4: the 64-bit field; earlier versions: the legacy field */
  double scale[3];
  double offset[3];
} pcv_las_header;

#define PCV_LAS_COLOR_AUTO 0      /* RGB16 / RGB8 by the largest channel value of the file; INTENSITY for a format without RGB */
#define PCV_LAS_COLOR_RGB16 1     /* c >> 8 */
#define PCV_LAS_COLOR_RGB8 2      /* min(c, 255) */
#define PCV_LAS_COLOR_INTENSITY 3 /* r = g = b = Imax == 0 ? 0 : (uint32)I * 255 / Imax */
#define PCV_LAS_COLOR_CONSTANT 4  /* constant_color */
#define PCV_LAS_MAX_EXTRAS 12
/* The device holds at most this many raw pieces of piece_points records next to the outputs (and, for the AUTO and INTENSITY
 * rules, 6 or 2 bytes of parked 16-bit values per record until the file's maxima are known). */
#define PCV_LAS_RAW_PIECES 2
typedef struct pcv_las_params {
  uint32_t color_mode; /* PCV_LAS_COLOR_* */
  uint8_t constant_color[3];
  uint8_t drop_withheld;    /* 1: records with the withheld flag are dropped */
  uint32_t keep_intensity;  /* 1: the intensity column (float)I is kept */
  uint32_t piece_points;    /* records per piece; 0 = as many as one 32 MiB staging chunk holds, which is also the most */
  uint32_t use_transform;   /* 1: global_from_local is applied (the arithmetic of pcv_transform_points) */
  uint32_t num_extras;
  uint64_t class_mask[4];   /* bit c of the 256 keeps class c; all zero keeps every class */
  double global_from_local[7]; /* translation xyz, unit quaternion i j k w */
  const char* extras[PCV_LAS_MAX_EXTRAS]; /* names of the table below, each at most once */
} pcv_las_params;
/* Extras (name, PCV_ATTR_* type): classification U8, classification_flags U8 (bit 0 synthetic, 1 key-point, 2 withheld,
 * 3 overlap), return_number U8, number_of_returns U8, scan_direction_flag U8, edge_of_flight_line U8, scanner_channel U8
 * (formats 6-10), scan_angle F32 (degrees), user_data U8, point_source_id U16, gps_time F64 (formats 1, 3-10; the eight bytes as
 * they are), nir U16 (formats 8, 10). A name the format lacks is PCV_E_INVALID naming it. */

typedef struct pcv_las_info {
  uint64_t num_records, num_kept;
  uint64_t dropped_class;    /* records whose class the mask does not keep */
  uint64_t dropped_withheld; /* records the mask keeps and drop_withheld drops */
  uint32_t max_color;        /* largest R, G or B over ALL records (0 for a format without RGB) */
  uint32_t max_intensity;    /* largest intensity over ALL records */
  uint32_t color_rule;       /* the PCV_LAS_COLOR_* that was applied (never AUTO) */
  uint32_t num_pieces;
  uint64_t class_hist[256];  /* over all records */
  uint64_t return_hist[16];  /* return number, over all records */
  uint64_t flag_counts[4];   /* synthetic, key-point, withheld, overlap, over all records */
} pcv_las_info;

/* Output columns of the stage entries: capacity n each (3 n bytes of colour); intensity when keep_intensity; extras[k] the
 * column of params->extras[k] in its type. The first num_kept elements are written. */
typedef struct pcv_las_columns {
  double* x;
  double* y;
  double* z;
  uint8_t* color;
  float* intensity;
  void* extras[PCV_LAS_MAX_EXTRAS];
} pcv_las_columns;

/* Host only, no context (messages: pcv_host_last_error). */
/* PCV_E_INVALID naming the field: a wrong signature, a major version other than 1 or a minor version above 4, a header size
 * below the version's (227, 227, 227, 235, 375), an offset to point data below the header size, a format above 10, a record
 * length below the format's minimum (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67), one of the top two bits of the format byte set
 * (a LAZ file), a non-finite scale or offset, a 1.4 file whose non-zero legacy count differs from the 64-bit count, 2^32 - 1 or
 * more records. PCV_E_IO: the file cannot be read, ends inside the header, or is shorter than header plus records. */
int pcv_las_header_host(const char* path, pcv_las_header* out);
/* PCV_E_INVALID: an unknown colour mode, RGB16 / RGB8 on a format without colour, an extra the format lacks or that is named
 * twice or unknown, more than PCV_LAS_MAX_EXTRAS, a non-finite transform. */
int pcv_las_check_params_host(const pcv_las_header* header, const pcv_las_params* params);
/* The extras a format has, in the table's order: names[k] are static strings, types[k] PCV_ATTR_*; each nullable. */
int pcv_las_extras_host(uint32_t point_format, const char** names, int32_t* types, uint32_t* count);
/* The decode on the host, the device's twin bit for bit: n raw records of header->record_length bytes -> columns and info. */
int pcv_las_decode_host(const pcv_las_header* header, const pcv_las_params* params, const void* raw, uint64_t n, pcv_las_columns* out,
                        pcv_las_info* info);
/* The one-pass host reader, shaped like pcv_ply_read_ex: host columns owned by the handle. */
typedef struct pcv_las pcv_las;
int pcv_las_read(const char* path, const pcv_las_params* params, pcv_las** out);
uint64_t pcv_las_num_points(const pcv_las* las);
int pcv_las_points(const pcv_las* las, pcv_points* out);
int pcv_las_attributes(const pcv_las* las, uint32_t* count, struct pcv_attribute* out /* nullable; PCV_LAS_MAX_EXTRAS entries */);
int pcv_las_info_get(const pcv_las* las, pcv_las_info* out);
void pcv_las_free(pcv_las* las);

/* The device path. The file goes up in pieces of piece_points records, pread by the context's host threads into the pinned
 * ring; piece k is decoded on the context's stream while piece k + 1 is copied on its side stream. PCV_E_IO (a truncated
 * file) leaves the context usable. */
typedef struct pcv_las_cloud pcv_las_cloud;
int pcv_las_load(pcv_ctx* ctx, const char* path, const pcv_las_params* params, pcv_las_cloud** out);
int pcv_las_cloud_info(const pcv_las_cloud* c, pcv_las_info* out);
/* PCV_MEM_DEVICE planes owned by the cloud (intensity NULL unless kept): as pcv_build_octree (with PCV_BUILD_COMPUTE_BBOX),
 * pcv_s2_split_ex, pcv_s2_stream_append_ex, pcv_terrain_add_points and pcv_maptiles_add_points take them. */
int pcv_las_cloud_points(const pcv_las_cloud* c, pcv_points* out);
int pcv_las_cloud_attributes(const pcv_las_cloud* c, uint32_t* count, struct pcv_attribute* out /* nullable; PCV_LAS_MAX_EXTRAS entries */);
/* One column into host memory: "x", "y", "z", "color", "intensity" or an extra's name; capacity_bytes must hold it. */
int pcv_las_cloud_read(const pcv_las_cloud* c, const char* name, void* out, uint64_t capacity_bytes);
void pcv_las_cloud_free(pcv_las_cloud* c);
/* The stage entry: n raw records where `mem` says -> columns where `mem` says; the outputs of pcv_las_decode_host. */
int pcv_las_decode(pcv_ctx* ctx, const pcv_las_header* header, const pcv_las_params* params, const void* raw, uint64_t n, int mem,
                   pcv_las_columns* out, pcv_las_info* info);
/* pcv_las_load + pcv_build_octree with PCV_BUILD_COMPUTE_BBOX; the octree carries intensity when keep_intensity. */
int pcv_build_octree_from_las(pcv_ctx* ctx, const pcv_build_params* params, const char* path, const pcv_las_params* las_params,
                              pcv_octree** out);

/* ---- 3D Tiles export --------------------------------------------------------------------- */
/* An octree as an OGC 3D Tiles 1.0 tileset: <dir>/tileset.json and one Point Cloud file <dir>/<NodeId>.pnts per node that
 * holds points. The reference has no such writer; the product is this library's and is stated here. Every point of the octree
 * is in exactly one node and a parent holds a sample of its subtree, which is "refine":"ADD"; a node's cube is the tile's box.
 *   tiles    a node with num_points > 0 is a tile with content "<NodeId>.pnts"; a node with 0 points and a non-empty
 *            descendant is a tile without content; a node whose whole subtree holds 0 points is left out. Children ascend
 *            by child index.
 *   json     {"asset":{"version":"1.0"},"geometricError":G,"root":T}, no whitespace, with
 *            T = {"boundingVolume":{"box":[cx,cy,cz,h,0.0,0.0,0.0,h,0.0,0.0,0.0,h]},"geometricError":g,"refine":"ADD"
 *                 [,"transform":[16 doubles, column-major]][,"content":{"uri":"<id>.pnts"}][,"children":[T,...]]}
 *            c = cube_min + cube_edge / 2, h = cube_edge / 2; refine and transform on the root only; g = cube_edge *
 *            error_factor for a tile with child tiles and 0.0 for one without; G = the root's edge. Doubles as in the
 *            terrain's meta.json: the shortest of %.15g .. %.17g that round-trips, ".0" after an integral value.
 *   .pnts    little endian. 28-byte header: "pnts", u32 version 1, u32 byteLength, u32 lengths of the feature table JSON, the
 *            feature table binary, the batch table JSON, the batch table binary; then those four sections. A JSON is padded
 *            with 0x20 and a binary with 0x00 so that each section and the file end on a multiple of 8 from the file's start;
 *            the lengths include the padding.
 *            feature JSON, quantized: {"POINTS_LENGTH":n,"RTC_CENTER":[a,b,c],"QUANTIZED_VOLUME_OFFSET":[a,b,c],
 *              "QUANTIZED_VOLUME_SCALE":[e,e,e],"POSITION_QUANTIZED":{"byteOffset":0},"RGB":{"byteOffset":6n}}
 *            feature JSON, float: {"POINTS_LENGTH":n,"RTC_CENTER":[a,b,c],"POSITION":{"byteOffset":0},"RGB":{"byteOffset":12n}}
 *            feature binary: n x 3 u16 or n x 3 f32, then the node's .rgb bytes without a gap.
 *            With PCV_TILES3D_INTENSITY the batch JSON is {"INTENSITY":{"byteOffset":0,"componentType":"FLOAT","type":"SCALAR"}}
 *            and the batch binary the node's .intensity bytes; without it both lengths are 0.
 *   centre   RTC_CENTER[a] = rc[a] = (double)(float)(cube_min[a] + cube_edge / 2): a reader may round these globals to
 *            float32, and a centre that is a float32 value already loses nothing. QUANTIZED_VOLUME_OFFSET[a] = cube_min[a] -
 *            rc[a] (exact in f64), QUANTIZED_VOLUME_SCALE = cube_edge. A reader's position is rc + offset + q * scale / 65535,
 *            or rc + (double)f.
 *   chain    quantized: a u8 code c -> c * 257; a u16 code verbatim; an f32 / f64 unit value t -> (uint16)trunc(65535.0 * t).
 *            float: (float)(fma(u, cube_edge, cube_min) - rc) with u = c / 255.0, c / 65535.0 or t.
 *            PCV_TILES3D_POS_AUTO: quantized for PCV_ENC_UINT8 / UINT16 nodes (every bit of the codes is kept), float for
 *            PCV_ENC_FLOAT32 / FLOAT64 nodes; _QUANTIZED and _FLOAT force one form for every tile. */
#define PCV_TILES3D_INTENSITY 1u /* flags: the INTENSITY batch table; the octree must carry intensity */
#define PCV_TILES3D_POS_AUTO 0
#define PCV_TILES3D_POS_QUANTIZED 1
#define PCV_TILES3D_POS_FLOAT 2
#define PCV_TILES3D_DEFAULT_ERROR_FACTOR 0.0625 /* a node refines when its edge covers about 256 px at a 16 px screen-space error */
#define PCV_TILES3D_MIN_CHUNK_BYTES (4ull << 20)
#define PCV_TILES3D_DEFAULT_CHUNK_BYTES (256ull << 20)
typedef struct pcv_tiles3d_params {
  double error_factor;    /* geometricError of a tile with children = cube_edge * error_factor; finite, >= 0 */
  double transform[16];   /* the root's "transform", column-major; all zero: none */
  uint32_t flags;         /* PCV_TILES3D_INTENSITY */
  uint32_t position_mode; /* PCV_TILES3D_POS_* */
  uint64_t chunk_bytes;   /* whole files per piece of pcv_tiles3d_write_dir; 0: 256 MiB, else at least 4 MiB */
} pcv_tiles3d_params;
typedef struct pcv_tiles3d_info {
  uint64_t tiles;            /* tiles of tileset.json, those without content among them */
  uint64_t content_tiles;    /* .pnts files */
  uint64_t points;
  uint64_t total_file_bytes; /* of the .pnts files */
  uint32_t chunk_points;     /* points per work item of the packer (one workgroup each) */
  uint32_t reserved;
} pcv_tiles3d_info;
typedef struct pcv_tiles3d_tile {
  uint64_t node;          /* index into the octree's node table (pcv_octree_node) */
  uint64_t num_points;
  uint32_t mode;          /* PCV_TILES3D_POS_QUANTIZED or _FLOAT */
  uint32_t reserved;
  uint64_t file_bytes;
  uint64_t feature_json_offset, feature_binary_offset, batch_json_offset, batch_binary_offset; /* from the file's start */
} pcv_tiles3d_tile;

/* Host only, no context (messages: pcv_host_last_error). */
/* PCV_E_INVALID: a NULL argument, a non-finite or negative error_factor, a non-finite transform, an unknown flag or position
 * mode, a chunk_bytes that is set and below PCV_TILES3D_MIN_CHUNK_BYTES. */
int pcv_tiles3d_check_params_host(const pcv_tiles3d_params* params);
/* rc[3] of a node (only cube_min and cube_edge are read). */
int pcv_tiles3d_rtc_host(const pcv_node_info* node, double rc[3]);
/* One complete .pnts file from a node's record and its host bytes (xyz: the .xyz content, rgb: 3 n bytes, intensity: n f32,
 * NULL without PCV_TILES3D_INTENSITY), the device's twin bit for bit. *len: the file's length; out (nullable) takes
 * min(capacity, *len) bytes; tile (nullable): the plan of the file, its `node` 0. PCV_E_INVALID: what check_params refuses,
 * 0 points, the flag without intensity, a file of 4 GiB or more. */
int pcv_tiles3d_tile_host(const pcv_node_info* node, const pcv_tiles3d_params* params, const uint8_t* xyz, const uint8_t* rgb,
                          const float* intensity, uint8_t* out, uint64_t capacity, uint64_t* len, pcv_tiles3d_tile* tile);
/* tileset.json of a node table: `count` nodes ascending by (level, index), the root first, every other node's parent among
 * them (anything else is PCV_E_INVALID, as is a table without a point). id_high, id_low, num_points, level, cube_min and
 * cube_edge are read. *len: the length; buf (nullable) takes min(cap, *len) bytes. */
int pcv_tiles3d_tileset_json_host(const pcv_node_info* nodes, uint64_t count, const pcv_tiles3d_params* params, char* buf, uint64_t cap,
                                  uint64_t* len);

/* The plan of a tileset over a built octree or one from pcv_octree_open_dir (whose node files are read and uploaded once): which
 * nodes are tiles, every file's size and section offsets. The octree must outlive the plan. PCV_E_INVALID: what
 * check_params refuses, PCV_TILES3D_INTENSITY on an octree without intensity, an octree without a point, a single file larger
 * than chunk_bytes (the message names the node). A failed call leaves nothing allocated. */
typedef struct pcv_tiles3d pcv_tiles3d;
int pcv_tiles3d_plan(pcv_octree* tree, const pcv_tiles3d_params* params, pcv_tiles3d** out);
int pcv_tiles3d_info_get(const pcv_tiles3d* t, pcv_tiles3d_info* out);
/* The content tiles in node-table order into host memory: *num_tiles (nullable) their number, the first `capacity` are written. */
int pcv_tiles3d_tiles(const pcv_tiles3d* t, uint64_t capacity, pcv_tiles3d_tile* out, uint64_t* num_tiles);
/* Complete .pnts files of content tiles [first, first + count), back to back in `out`, which lives where `mem` says (NULL: the
 * offsets alone), file i at offsets[i] .. offsets[i + 1] (count + 1 offsets, host), as pcv_maptiles_tile_pngs. Packed by one
 * launch of tiles3d_pack_kernel from the node blobs on the device. PCV_E_INVALID: a range past the end, a capacity below
 * offsets[count]. A copy to device memory is complete on return as well. */
int pcv_tiles3d_tile_files(pcv_tiles3d* t, uint64_t first, uint64_t count, int mem, uint64_t capacity, uint8_t* out, uint64_t* offsets);
/* tileset.json of the plan's octree, as pcv_tiles3d_tileset_json_host. */
int pcv_tiles3d_tileset_json(const pcv_tiles3d* t, char* buf, uint64_t cap, uint64_t* len);
/* <directory>/<NodeId>.pnts for every content tile, then <directory>/tileset.json. Whole files are grouped into pieces of at
 * most chunk_bytes; piece k + 1 is packed (one launch) while piece k crosses to the host and is written by the context's host
 * threads. Two device buffers and two pinned blocks of the largest piece are held whatever the octree's size. PCV_E_IO names the
 * file. */
int pcv_tiles3d_write_dir(pcv_tiles3d* t, const char* directory);
void pcv_tiles3d_free(pcv_tiles3d* t);

/* ---- query results as LAS files --------------------------------------------------------- */
/* The results of pcv_query_batch_run and pcv_s2_query_run[_ex] as ASPRS LAS: 1.2 with point data record formats 0 - 3, 1.4 with
 * formats 0 - 3 and 6 - 8; little endian, no VLRs, no EVLRs, no extra bytes, record_length the format's minimum. The records are
 * quantised and bit-packed on the device. The reference has no LAS code; the contract is this library's.
 *   format   PCV_LAS_FORMAT_AUTO: 8 if the source has an extra `nir`, else 7 with `scanner_channel`, else 3 with `gps_time`,
 *            else 2. version_minor 0: 2 for formats <= 3, 4 otherwise. Formats 4, 5, 9, 10 and minors 1, 3 are PCV_E_INVALID.
 *   fields   `color`, `intensity` and the twelve names of pcv_las_extras_host. An extra of the source fills its field when it
 *            has that table's data type (another type under such a name is PCV_E_INVALID naming it); an extra of any other name
 *            is not written and counted in skipped_extras. fields == NULL: every field the source has and the format holds;
 *            otherwise the named ones: one the source lacks is PCV_E_INVALID "Data type for attribute 'NAME' not found.", one
 *            the format lacks PCV_E_INVALID naming it. A field nobody supplies is 0, return_number and number_of_returns 1.
 *   record   the inverse of the reader's decode, offset for offset. A value wider than its bit field is masked to it and
 *            counted in masked_values. gps_time is copied as its eight bytes.
 *   X Y Z    q = (x - offset) / scale (one subtraction, one IEEE division); the record holds (int32)rint(q), ties to even, when
 *            -2147483648.5 < q < 2147483647.5; otherwise (NaN included) it holds 0 and counts in out_of_range. scale must be
 *            finite and > 0, offset finite. auto_offset != 0: offset[a] = floor(min of axis a over the rows of the range), found
 *            by a launch of its own; 0 for a range without rows.
 *   intensity  v = intensity * intensity_scale in f32 (0 stands for the default scale 1); NaN -> 0, otherwise clamped to
 *            [0, 65535] and rounded by rintf; clamped_intensity counts the NaNs and the values outside. 0 without intensity.
 *   colour   PCV_LAS_WRITE_COLOR_X257: c * 257 (the reader's RGB16 rule returns c); _SHIFT8: c << 8; _RGB8: c. NIR: the extra.
 *   angle    formats 0 - 3: (int8)clamp(rintf(a), -128, 127); formats 6 - 8: (int16)clamp(rintf(a / 0.006f), -32768, 32767); NaN 0.
 *   header   file_source_id, global_encoding, day, year and the two 32-byte names from the params (names all NUL: "OTHER" and
 *            "point_cloud_viewer_amd"), GUID zero, header size 227 / 375 = offset to point data; legacy count and five legacy
 *            by-return counts for 1.2 and for 1.4 with formats <= 3, zero for formats >= 6; the 64-bit count and 15 by-return
 *            counts in 1.4. Return r counts in slot r - 1; return 0 and returns above the slots count nowhere. Bounds max x,
 *            min x, max y, min y, max z, min z = (double)Xmax * scale + offset over the records' integers.
 * pcv_*_las_records: the records alone under pcv_*_ply_rows' rules (*record_length and *num_records are set whenever range and
 * params are valid); out-of-range records are written with 0 and reported in info, the call is PCV_OK.
 * pcv_*_write_las: pieces of chunk_points records (0: 2^20) through two device buffers and two pinned blocks, the header last.
 * A range without rows writes no file and touches none. out_of_range != 0 is PCV_E_INVALID naming the count and the axis extent
 * and leaves no file (an appended one is cut back to its old bytes). 2^32 - 1 records or more are PCV_E_INVALID.
 *   PCV_LAS_APPEND  the file must be one this writer writes with these params (signature, version, header size, offset to point
 *            data, no VLRs, format, record length, no EVLRs, length = header + count x record; PCV_E_INVALID names the first
 *            field that differs). Its scale and offset are used; explicit ones (auto_offset == 0) must equal them bit for bit.
 *            Records go behind the old ones; counts and bounds are merged and the header is rewritten last. A missing file is
 *            written anew. info describes the records of this call. */
#define PCV_LAS_FORMAT_AUTO 255u
#define PCV_LAS_WRITE_COLOR_X257 0
#define PCV_LAS_WRITE_COLOR_SHIFT8 1
#define PCV_LAS_WRITE_COLOR_RGB8 2
#define PCV_LAS_TRUNCATE 0
#define PCV_LAS_APPEND 1
typedef struct pcv_las_write_params {
  uint32_t struct_size;   /* sizeof(pcv_las_write_params) */
  int32_t open_mode;      /* PCV_LAS_TRUNCATE / PCV_LAS_APPEND (ignored by pcv_*_las_records) */
  uint32_t point_format;  /* 0 - 3, 6 - 8 or PCV_LAS_FORMAT_AUTO */
  uint32_t version_minor; /* 0, 2 or 4 */
  double scale[3];
  double offset[3];
  uint32_t auto_offset;   /* != 0: offset is floor(min) per axis (in append mode: the file's) */
  uint32_t color_rule;    /* PCV_LAS_WRITE_COLOR_* */
  float intensity_scale;  /* 0: 1 */
  uint32_t num_fields;
  const char* const* fields; /* NULL: every field the source has and the format holds */
  uint64_t chunk_points;  /* records per piece of pcv_*_write_las; 0 = the default */
  uint16_t file_source_id, global_encoding, day, year;
  char system_identifier[32];   /* all NUL: "OTHER" */
  char generating_software[32]; /* all NUL: "point_cloud_viewer_amd" */
} pcv_las_write_params;
typedef struct pcv_las_write_info {
  uint32_t point_format, version_minor, record_length, header_size; /* as chosen */
  double scale[3], offset[3];                                       /* as resolved */
  int32_t min_xyz[3], max_xyz[3]; /* the integer extremes of the records (0 without records) */
  double bounds[6];               /* max x, min x, max y, min y, max z, min z */
  uint64_t num_records;
  uint64_t by_return[15];
  uint64_t out_of_range, clamped_intensity, masked_values;
  uint32_t skipped_extras, reserved;
} pcv_las_write_info;
int pcv_query_batch_las_records(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const pcv_las_write_params* params,
                                uint64_t capacity_bytes, int mem, void* out, uint32_t* record_length, uint64_t* num_records,
                                pcv_las_write_info* info);
int pcv_s2_query_las_records(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const pcv_las_write_params* params,
                             uint64_t capacity_bytes, int mem, void* out, uint32_t* record_length, uint64_t* num_records,
                             pcv_las_write_info* info);
int pcv_query_batch_write_las(pcv_query_batch* b, uint64_t first_segment, uint64_t num_segments, const char* path,
                              const pcv_las_write_params* params, pcv_las_write_info* info);
int pcv_s2_query_write_las(pcv_s2_query* q, uint64_t first_segment, uint64_t num_segments, const char* path,
                           const pcv_las_write_params* params, pcv_las_write_info* info);
/* Host only, no context (messages: pcv_host_last_error). The source is described by has_intensity and its extras (name, PCV_ATTR_*
 * type); *info receives the format, version, record length, header size and skipped_extras chosen. */
int pcv_las_write_check_params_host(const pcv_las_write_params* params, int has_intensity, const char* const* extra_names,
                                    const int32_t* extra_types, uint32_t num_extras, pcv_las_write_info* info);
/* The host twin of the device packer: n points (x, y, z; color 3 n bytes or NULL; intensity or NULL; extras[k] the column of
 * extra k or NULL) -> n records in out (n * record_length bytes) and *info, byte for byte what the kernels write. With
 * auto_offset the offset is floor(min) of these points. */
int pcv_las_encode_host(const pcv_las_write_params* params, uint64_t n, const double* x, const double* y, const double* z,
                        const uint8_t* color, const float* intensity, const char* const* extra_names, const int32_t* extra_types,
                        const void* const* extras, uint32_t num_extras, void* out, uint64_t capacity_bytes, pcv_las_write_info* info);
/* The header of a file whose records `info` describes (format, version, scale, offset, extremes, counts), `buf` of at least
 * info->header_size bytes; *len its length. */
int pcv_las_write_header_host(const pcv_las_write_params* params, const pcv_las_write_info* info, void* buf, uint64_t cap, uint64_t* len);
/* What PCV_LAS_APPEND checks before it touches `path`, for a file of `info`'s format, version (and, with auto_offset == 0, the
 * params' scale and offset): *old_count the file's records (0 for a missing file). */
int pcv_las_append_check_host(const char* path, const pcv_las_write_params* params, const pcv_las_write_info* info, uint64_t* old_count);

#ifdef __cplusplus
}
#endif
#endif /* PCV_HIP_H */
