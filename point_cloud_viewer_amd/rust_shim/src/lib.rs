//! 1:1 veneer over include/pcv_hip.h that keeps the reference crate's public surface for the hot path:
//! `build_octree` (src/octree/generation.rs:289-295), `Octree::get_visible_nodes` (src/octree/mod.rs:228), and the
//! `PointCloud` trait (src/iterator.rs:169-206: `nodes_in_location`, `encoding_for_node`, `points_in_node`,
//! `bounding_box`, `stream_points_for_query_in_node`) as `HipOctree`, which `ParallelIterator` / `PointCloudClient`
//! take unchanged. All logic lives behind the C ABI; this file only marshals `PointsBatch` / nalgebra types into plain
//! pointers. Uncompiled here (no Rust toolchain in the build container) — see INTEGRATION.md for how it slots into the
//! reference workspace and for the four accessor one-liners it needs on `Frustum` / `Obb` (their fields are private).
use nalgebra::{Matrix4, Point3, Vector3};
use point_viewer::data_provider::{DataProvider, OnDiskDataProvider};
use point_viewer::errors::{ErrorKind, Result};
use point_viewer::geometry::Aabb;
use point_viewer::iterator::{PointCloud, PointLocation, PointQuery};
use point_viewer::octree::{NodeId, Octree};
use point_viewer::read_write::{Encoding, NodeIterator, NodeWriter, OpenMode, PositionEncoding};
use point_viewer::{AttributeData, NumberOfPoints, PointsBatch};
use std::collections::{BTreeMap, HashMap};
use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_double, c_float, c_int, c_void};
use std::path::{Path, PathBuf};
use std::sync::Mutex;

#[repr(C)]
pub struct PcvPoints {
    n: u64,
    x: *const c_double,
    y: *const c_double,
    z: *const c_double,
    color: *const u8,
    color_stride: u32,
    intensity: *const c_float,
    mem: i32,
}

#[repr(C)]
pub struct PcvBuildParams {
    resolution: c_double,
    bbox_min: [c_double; 3],
    bbox_max: [c_double; 3],
    max_points_per_node: u32,
    flags: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct PcvShape {
    kind: i32,
    reserved: i32,
    params: [c_double; 32],
}

#[repr(C)]
#[derive(Default, Clone, Copy)]
pub struct PcvNodeInfo {
    id_high: u64,
    id_low: u64,
    num_points: i64,
    level: u32,
    encoding: u32,
    cube_min: [c_double; 3],
    cube_edge: c_double,
    xyz_offset: u64,
    point_offset: u64,
}

#[allow(non_camel_case_types)]
type pcv_ctx = c_void;
#[allow(non_camel_case_types)]
type pcv_octree = c_void;
#[allow(non_camel_case_types)]
type pcv_shapes = c_void;
#[allow(non_camel_case_types)]
type pcv_ingest = c_void;
#[allow(non_camel_case_types)]
type pcv_ooc = c_void;
#[allow(non_camel_case_types)]
type pcv_query_batch = c_void;
#[allow(non_camel_case_types)]
type pcv_terrain = c_void;
#[allow(non_camel_case_types)]
type pcv_maptiles = c_void;
#[allow(non_camel_case_types)]
type pcv_render = c_void;
#[allow(non_camel_case_types)]
type pcv_tiles3d = c_void;

/// include/pcv_hip.h pcv_render_params: one frame of the viewer (sdl_viewer/src/lib.rs:158-209).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PcvRenderParams {
    pub width: u32,
    pub height: u32,
    pub point_size: c_float,
    pub gamma: c_float,
    pub max_nodes: u32,
    pub max_workspace_bytes: u64,
}

/// include/pcv_hip.h pcv_render_overlay: what pcv_render_views_ex draws on top of the points (flags: 1 =
/// PCV_RENDER_OUTLINE_NODES, the viewer's show_octree_nodes, sdl_viewer/src/lib.rs:202-208).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PcvRenderOverlay {
    pub flags: u32,
    pub outline_rgba: [u8; 4],
}

/// include/pcv_hip.h pcv_render_terrain_layers: the terrain layers pcv_render_views_terrain draws after the nodes
/// (sdl_viewer --terrain). `camera_positions`: views x 3 doubles, world frame.
#[repr(C)]
pub struct PcvRenderTerrainLayers {
    pub num_layers: u32,
    pub window: u32,
    pub layers: *const *mut pcv_terrain,
    pub camera_positions: *const c_double,
}

/// include/pcv_hip.h pcv_ooc_stats: what an out-of-core build did (points, nodes, partitions, host spill, link traffic, phase times).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PcvOocStats {
    pub points: u64,
    pub nodes: u64,
    pub partitions: u64,
    pub largest_bucket: u64,
    pub spill_bytes: u64,
    pub h2d_bytes: u64,
    pub d2h_bytes: u64,
    pub h2d_ms: f64,
    pub d2h_ms: f64,
    pub stream_ms: f64,
    pub topology_ms: f64,
    pub build_ms: f64,
    pub merge_ms: f64,
    pub write_ms: f64,
    pub split_mask: u32,
    pub routed: u32,
}

extern "C" {
    fn pcv_abi_version() -> c_int;
    fn pcv_ctx_create(device: c_int, stream: *mut c_void, out: *mut *mut pcv_ctx) -> c_int;
    fn pcv_ctx_destroy(ctx: *mut pcv_ctx);
    fn pcv_last_error(ctx: *const pcv_ctx) -> *const c_char;
    #[allow(dead_code)]
    fn pcv_build_octree(ctx: *mut pcv_ctx, params: *const PcvBuildParams, points: *const PcvPoints, out: *mut *mut pcv_octree) -> c_int;
    // streaming batch ingest: `impl Iterator<Item = PointsBatch>` of generation.rs:289-295, one batch per call
    fn pcv_ingest_begin(ctx: *mut pcv_ctx, num_points_hint: u64, has_intensity: c_int, out: *mut *mut pcv_ingest) -> c_int;
    fn pcv_ingest_append(ingest: *mut pcv_ingest, xyz: *const c_double, rgb: *const u8, intensity: *const c_float, n: u64) -> c_int;
    fn pcv_ingest_finish(ingest: *mut pcv_ingest, params: *const PcvBuildParams, out: *mut *mut pcv_octree) -> c_int;
    fn pcv_ingest_abort(ingest: *mut pcv_ingest);
    // out-of-core build: the same batches, for clouds larger than the device (host spills, partitions built one after another)
    fn pcv_ooc_begin(ctx: *mut pcv_ctx, params: *const PcvBuildParams, has_intensity: c_int, max_points_per_pass: u64, out: *mut *mut pcv_ooc) -> c_int;
    fn pcv_ooc_append(ooc: *mut pcv_ooc, xyz: *const c_double, rgb: *const u8, intensity: *const c_float, n: u64) -> c_int;
    fn pcv_ooc_finish(ooc: *mut pcv_ooc, directory: *const c_char, stats: *mut PcvOocStats) -> c_int;
    fn pcv_ooc_abort(ooc: *mut pcv_ooc);
    fn pcv_build_octree_from_ply(ctx: *mut pcv_ctx, params: *const PcvBuildParams, path: *const c_char, with_intensity: c_int, out: *mut *mut pcv_octree) -> c_int;
    // a LAS 1.0 - 1.4 file decoded and filtered on the device, then the build with the box computed there
    fn pcv_build_octree_from_las(ctx: *mut pcv_ctx, params: *const PcvBuildParams, path: *const c_char, las_params: *const PcvLasParams, out: *mut *mut pcv_octree) -> c_int;
    fn pcv_octree_write_dir(t: *mut pcv_octree, directory: *const c_char) -> c_int;
    fn pcv_octree_open_dir(ctx: *mut pcv_ctx, directory: *const c_char, out: *mut *mut pcv_octree) -> c_int;
    fn pcv_octree_num_nodes(t: *const pcv_octree) -> u64;
    fn pcv_octree_node(t: *const pcv_octree, i: u64, out: *mut PcvNodeInfo) -> c_int;
    fn pcv_octree_free(t: *mut pcv_octree);
    fn pcv_shapes_create(ctx: *mut pcv_ctx, shapes: *const PcvShape, count: u32, out: *mut *mut pcv_shapes) -> c_int;
    fn pcv_shapes_create_ex(ctx: *mut pcv_ctx, shapes: *const PcvShape, count: u32, num_unions: u32, union_first: *const u32, union_cells: *const u64,
                            out: *mut *mut pcv_shapes) -> c_int;
    fn pcv_shapes_create_ex2(ctx: *mut pcv_ctx, shapes: *const PcvShape, count: u32, num_unions: u32, union_first: *const u32, union_cells: *const u64,
                             num_polygons: u32, polygon_first: *const u32, ring_first: *const u32, vertices: *const f64, out: *mut *mut pcv_shapes) -> c_int;
    fn pcv_shapes_free(s: *mut pcv_shapes);
    fn pcv_visible_nodes(ctx: *mut pcv_ctx, frusta: *const pcv_shapes, t: *mut pcv_octree, capacity: u32, counts: *mut u32, node_indices: *mut u32, status: *mut i32) -> c_int;
    // per frustum the nodes whose Relation is not Out, with relation and relative_size_on_screen (octree/mod.rs:119-139, 261-272)
    #[allow(dead_code)]
    fn pcv_cull_nodes_sparse(ctx: *mut pcv_ctx, shapes: *const pcv_shapes, t: *mut pcv_octree, capacity: u32, counts: *mut u32, node_indices: *mut u32, relation: *mut u8, size_on_screen: *mut c_double) -> c_int;
    fn pcv_nodes_in_location(ctx: *mut pcv_ctx, shapes: *const pcv_shapes, t: *mut pcv_octree, capacity: u32, counts: *mut u32, node_indices: *mut u32) -> c_int;
    fn pcv_query_node_points(ctx: *mut pcv_ctx, shapes: *const pcv_shapes, shape_index: u32, t: *mut pcv_octree, node: u64, interval: *const c_double, capacity: u64, mem: c_int, x: *mut c_double, y: *mut c_double, z: *mut c_double, rgb: *mut u8, intensity: *mut c_float, count: *mut u64) -> c_int;
    fn pcv_octree_has_intensity(t: *const pcv_octree) -> c_int;
    fn pcv_query_batch_run(ctx: *mut pcv_ctx, shapes: *const pcv_shapes, t: *mut pcv_octree, intervals: *const c_double, interval_used: *const u8, out: *mut *mut pcv_query_batch) -> c_int;
    fn pcv_query_batch_sizes(b: *const pcv_query_batch, num_segments: *mut u64, num_points: *mut u64) -> c_int;
    fn pcv_query_batch_segments(b: *const pcv_query_batch, shape_first_segment: *mut u64, segment_node: *mut u32, segment_offset: *mut u64) -> c_int;
    fn pcv_query_batch_points(b: *mut pcv_query_batch, first_segment: u64, num_segments: u64, capacity: u64, mem: c_int, x: *mut c_double, y: *mut c_double, z: *mut c_double, rgb: *mut u8, intensity: *mut c_float) -> c_int;
    fn pcv_query_batch_free(b: *mut pcv_query_batch);
    // PlyNodeWriter over a query's result (ply.rs:559-732): the rows packed on the device, the file written in pieces
    fn pcv_query_batch_write_ply(b: *mut pcv_query_batch, first_segment: u64, num_segments: u64, path: *const c_char, params: *const PcvPlyWriteParams, written: *mut u64) -> c_int;
    // the same result as an ASPRS LAS file: the records quantised and packed on the device
    fn pcv_query_batch_write_las(b: *mut pcv_query_batch, first_segment: u64, num_segments: u64, path: *const c_char, params: *const PcvLasWriteParams, info: *mut PcvLasWriteInfo) -> c_int;
    // terrain layers: a query's result reduced to grid vertices on the device, the directory sdl_viewer --terrain reads
    fn pcv_terrain_begin(ctx: *mut pcv_ctx, params: *const PcvTerrainParams, bbox_min: *const c_double, bbox_max: *const c_double, out: *mut *mut pcv_terrain) -> c_int;
    fn pcv_terrain_add_query_batch(t: *mut pcv_terrain, b: *mut pcv_query_batch, first_segment: u64, num_segments: u64) -> c_int;
    fn pcv_terrain_finish(t: *mut pcv_terrain) -> c_int;
    fn pcv_terrain_write_dir(t: *mut pcv_terrain, directory: *const c_char) -> c_int;
    fn pcv_terrain_free(t: *mut pcv_terrain);
    // map tiles: a query's result drawn into z/x/y PNG tiles on the device
    fn pcv_maptiles_begin(ctx: *mut pcv_ctx, params: *const PcvMapTilesParams, out: *mut *mut pcv_maptiles) -> c_int;
    fn pcv_maptiles_add_query_batch(m: *mut pcv_maptiles, b: *mut pcv_query_batch, first_segment: u64, num_segments: u64) -> c_int;
    fn pcv_maptiles_finish(m: *mut pcv_maptiles) -> c_int;
    fn pcv_maptiles_build_parents(m: *mut pcv_maptiles, min_zoom: u32) -> c_int;
    fn pcv_maptiles_write_dir(m: *mut pcv_maptiles, directory: *const c_char, png_mode: c_int) -> c_int;
    fn pcv_maptiles_free(m: *mut pcv_maptiles);
    // 3D Tiles: the octree's node blobs packed into .pnts files on the device
    fn pcv_tiles3d_plan(tree: *mut pcv_octree, params: *const PcvTiles3dParams, out: *mut *mut pcv_tiles3d) -> c_int;
    fn pcv_tiles3d_info_get(t: *const pcv_tiles3d, out: *mut PcvTiles3dInfo) -> c_int;
    fn pcv_tiles3d_write_dir(t: *mut pcv_tiles3d, directory: *const c_char) -> c_int;
    fn pcv_tiles3d_free(t: *mut pcv_tiles3d);
    // the viewer's frame: get_visible_nodes + GL_POINTS under a depth test, rasterised on the device
    fn pcv_s2_open_dir(ctx: *mut pcv_ctx, directory: *const c_char, out: *mut *mut pcv_s2_cloud) -> c_int;
    fn pcv_s2_info(c: *const pcv_s2_cloud, num_cells: *mut u64, num_points: *mut u64, bbox_min: *mut c_double, bbox_max: *mut c_double, has_intensity: *mut c_int, level: *mut u32) -> c_int;
    fn pcv_s2_cells(c: *const pcv_s2_cloud, ids: *mut u64, counts: *mut u64, offsets: *mut u64) -> c_int;
    fn pcv_s2_cells_in_location(c: *mut pcv_s2_cloud, shapes: *const pcv_shapes, num_unions: u32, union_first: *const u32, union_cells: *const u64, capacity: u32, counts: *mut u32, cells: *mut u32) -> c_int;
    fn pcv_s2_query_run(c: *mut pcv_s2_cloud, shapes: *const pcv_shapes, num_unions: u32, union_first: *const u32, union_cells: *const u64, intervals: *const c_double, interval_used: *const u8, out: *mut *mut pcv_s2_query) -> c_int;
    fn pcv_s2_query_segments(q: *const pcv_s2_query, location_first_segment: *mut u64, segment_cell: *mut u32, segment_offset: *mut u64) -> c_int;
    fn pcv_s2_query_sizes(q: *const pcv_s2_query, num_segments: *mut u64, num_points: *mut u64) -> c_int;
    fn pcv_s2_query_points(q: *mut pcv_s2_query, first_segment: u64, num_segments: u64, capacity: u64, mem: c_int, x: *mut c_double, y: *mut c_double, z: *mut c_double, rgb: *mut u8, intensity: *mut c_float) -> c_int;
    fn pcv_s2_query_free(q: *mut pcv_s2_query);
    fn pcv_s2_free(c: *mut pcv_s2_cloud);
    fn pcv_render_views(ctx: *mut pcv_ctx, frusta: *const pcv_shapes, t: *mut pcv_octree, params: *const PcvRenderParams, out: *mut *mut pcv_render) -> c_int;
    fn pcv_render_views_ex(ctx: *mut pcv_ctx, frusta: *const pcv_shapes, t: *mut pcv_octree, params: *const PcvRenderParams, overlay: *const PcvRenderOverlay, out: *mut *mut pcv_render) -> c_int;
    fn pcv_render_views_terrain(ctx: *mut pcv_ctx, frusta: *const pcv_shapes, t: *mut pcv_octree, params: *const PcvRenderParams, overlay: *const PcvRenderOverlay, terrain: *const PcvRenderTerrainLayers, out: *mut *mut pcv_render) -> c_int;
    fn pcv_terrain_open_dir(ctx: *mut pcv_ctx, directory: *const std::os::raw::c_char, out: *mut *mut pcv_terrain) -> c_int;
    fn pcv_render_images(r: *mut pcv_render, first: u32, count: u32, rgba: *mut c_void, mem: c_int) -> c_int;
    fn pcv_render_free(r: *mut pcv_render);
}

/// pcv_las_write_params (include/pcv_hip.h)
#[repr(C)]
pub struct PcvLasWriteParams {
    pub struct_size: u32,
    pub open_mode: i32,
    pub point_format: u32,
    pub version_minor: u32,
    pub scale: [f64; 3],
    pub offset: [f64; 3],
    pub auto_offset: u32,
    pub color_rule: u32,
    pub intensity_scale: f32,
    pub num_fields: u32,
    pub fields: *const *const c_char,
    pub chunk_points: u64,
    pub file_source_id: u16,
    pub global_encoding: u16,
    pub day: u16,
    pub year: u16,
    pub system_identifier: [c_char; 32],
    pub generating_software: [c_char; 32],
}

/// pcv_las_write_info (include/pcv_hip.h)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PcvLasWriteInfo {
    pub point_format: u32,
    pub version_minor: u32,
    pub record_length: u32,
    pub header_size: u32,
    pub scale: [f64; 3],
    pub offset: [f64; 3],
    pub min_xyz: [i32; 3],
    pub max_xyz: [i32; 3],
    pub bounds: [f64; 6],
    pub num_records: u64,
    pub by_return: [u64; 15],
    pub out_of_range: u64,
    pub clamped_intensity: u64,
    pub masked_values: u64,
    pub skipped_extras: u32,
    pub reserved: u32,
}

/// pcv_ply_write_params (include/pcv_hip.h)
#[repr(C)]
pub struct PcvPlyWriteParams {
    pub struct_size: u32,
    pub open_mode: i32,
    pub attributes: *const *const c_char,
    pub num_attributes: u32,
    pub reserved: u32,
    pub chunk_points: u64,
}

/// pcv_maptiles_params (include/pcv_hip.h); background: packed RGBA8, r in the low byte
#[repr(C)]
pub struct PcvMapTilesParams {
    pub zoom: u32,
    pub background: u32,
    pub max_tiles: u64,
    pub max_pool_bytes: u64,
    pub staging_points: u64,
}

/// pcv_tiles3d_params (include/pcv_hip.h); transform: column-major, all zero = none; flags: 1 = the INTENSITY
/// batch table; position_mode: 0 auto, 1 quantized, 2 float; chunk_bytes: 0 = 256 MiB
#[repr(C)]
pub struct PcvTiles3dParams {
    pub error_factor: f64,
    pub transform: [f64; 16],
    pub flags: u32,
    pub position_mode: u32,
    pub chunk_bytes: u64,
}

impl Default for PcvTiles3dParams {
    fn default() -> Self {
        PcvTiles3dParams { error_factor: 0.0625, transform: [0.0; 16], flags: 0, position_mode: 0, chunk_bytes: 0 }
    }
}

/// pcv_tiles3d_info (include/pcv_hip.h)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct PcvTiles3dInfo {
    pub tiles: u64,
    pub content_tiles: u64,
    pub points: u64,
    pub total_file_bytes: u64,
    pub chunk_points: u32,
    pub reserved: u32,
}

/// pcv_las_params (include/pcv_hip.h); color_mode: 0 auto, 1 rgb16, 2 rgb8, 3 intensity, 4 constant
#[repr(C)]
pub struct PcvLasParams {
    pub color_mode: u32,
    pub constant_color: [u8; 3],
    pub drop_withheld: u8,
    pub keep_intensity: u32,
    pub piece_points: u32,
    pub use_transform: u32,
    pub num_extras: u32,
    pub class_mask: [u64; 4],
    pub global_from_local: [f64; 7],
    pub extras: [*const c_char; 12],
}

impl Default for PcvLasParams {
    /// Every class, colour by AUTO, intensity kept (the octree's second attribute), no extras, no transform.
    fn default() -> Self {
        PcvLasParams { color_mode: 0, constant_color: [0; 3], drop_withheld: 0, keep_intensity: 1, piece_points: 0, use_transform: 0, num_extras: 0,
                       class_mask: [0; 4], global_from_local: [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], extras: [std::ptr::null(); 12] }
    }
}

/// pcv_terrain_params (include/pcv_hip.h); statistic: 0 max, 1 min, 2 mean
#[repr(C)]
pub struct PcvTerrainParams {
    pub tile_size: u32,
    pub statistic: u32,
    pub resolution_m: f64,
    pub origin: [f64; 3],
    pub world_from_terrain: [f64; 7],
    pub min_points: u32,
    pub reserved: u32,
    pub max_pool_bytes: u64,
    pub staging_points: u64,
}

pub struct HipContext(*mut pcv_ctx);

impl HipContext {
    pub fn new(device: i32) -> Result<Self, String> {
        // include/pcv_hip.h PCV_ABI_VERSION these declarations were written against (2: pcv_ingest_*, PCV_STAGE_SORT_SECOND)
        if unsafe { pcv_abi_version() } != 2 {
            return Err(format!("libpcv_hip.so has ABI version {}, this veneer expects 2", unsafe { pcv_abi_version() }));
        }
        let mut ctx = std::ptr::null_mut();
        match unsafe { pcv_ctx_create(device, std::ptr::null_mut(), &mut ctx) } {
            0 => Ok(HipContext(ctx)),
            rc => Err(format!("pcv_ctx_create failed: {}", rc)),
        }
    }
    fn check(&self, rc: c_int) {
        if rc != 0 {
            // The reference's builder panics on every error (generation.rs:99,177,376); keep that contract.
            let msg = unsafe { CStr::from_ptr(pcv_last_error(self.0)) }.to_string_lossy().into_owned();
            panic!("pcv_hip error {}: {}", rc, msg);
        }
    }
}

impl Drop for HipContext {
    fn drop(&mut self) {
        unsafe { pcv_ctx_destroy(self.0) }
    }
}

thread_local! {
    /// One context per host thread for the lifetime of the thread (a `pcv_ctx` is bound to one device and one stream
    /// and is not thread-safe; creating one costs a stream, events and the first pinned allocations).
    static CONTEXT: HipContext = HipContext::new(0).expect("no MI355X visible (there is no CPU fallback)");
}

/// Same signature and behaviour as `point_viewer::octree::build_octree` (generation.rs:289-295). The batches go to the
/// device ONE AT A TIME and AS THEY ARE (pcv_ingest_append): `batch.position` is a `Vec<Point3<f64>>` — `Point3<f64>` is
/// `#[repr(C)]` over `[f64; 3]`, so the vector is n x 3 contiguous doubles — "color" a `Vec<Vector3<u8>>` (n x 3 bytes),
/// "intensity" a `Vec<f32>`. The library copies the three slices into its pinned ring, queues one DMA and one kernel that
/// transposes AoS -> SoA on the device, and returns; the iterator produces its next batch meanwhile. No whole-cloud host
/// vector exists at any time (host memory: the ring, 3 x 32 MiB), nothing is transposed on the host.
pub fn build_octree(
    output_directory: impl AsRef<Path>,
    resolution: f64,
    bounding_box: Aabb,
    input: impl Iterator<Item = PointsBatch> + NumberOfPoints + Send,
    attributes: &[&str],
) {
    let want_intensity = attributes.contains(&"intensity");
    CONTEXT.with(|ctx| {
        let mut ingest = std::ptr::null_mut();
        ctx.check(unsafe { pcv_ingest_begin(ctx.0, input.num_points() as u64, want_intensity as c_int, &mut ingest) });
        for batch in input {
            let color = match batch.attributes.get("color") {
                Some(AttributeData::U8Vec3(c)) => c.as_ptr() as *const u8,
                _ => panic!("color attribute (U8Vec3) is required"), // on_disk.rs:20-22
            };
            let intensity = if want_intensity {
                match batch.attributes.get("intensity") {
                    Some(AttributeData::F32(i)) => i.as_ptr(),
                    _ => panic!("intensity requested but missing"), // generation.rs:167-177 unwrap()
                }
            } else {
                std::ptr::null()
            };
            let rc = unsafe { pcv_ingest_append(ingest, batch.position.as_ptr() as *const c_double, color, intensity, batch.position.len() as u64) };
            if rc != 0 {
                unsafe { pcv_ingest_abort(ingest) };
                ctx.check(rc);
            }
            // `batch` is dropped here: the library has copied it into pinned memory before returning
        }
        let params = PcvBuildParams {
            resolution,
            bbox_min: [bounding_box.min().x, bounding_box.min().y, bounding_box.min().z],
            bbox_max: [bounding_box.max().x, bounding_box.max().y, bounding_box.max().z],
            max_points_per_node: 0,
            flags: 0,
        };
        let mut tree = std::ptr::null_mut();
        ctx.check(unsafe { pcv_ingest_finish(ingest, &params, &mut tree) }); // consumes the ingest whatever it returns
        let dir = CString::new(output_directory.as_ref().to_str().unwrap()).unwrap();
        ctx.check(unsafe { pcv_octree_write_dir(tree, dir.as_ptr()) });
        unsafe { pcv_octree_free(tree) };
    });
}

/// `build_octree` for clouds larger than the device: the same batches stream through pcv_ooc_append into host spills, and
/// pcv_ooc_finish builds the tree partition by partition of at most `max_points_per_pass` points (0 = derived from the free
/// device memory) straight into `output_directory` — the same directory, byte for byte. Every attribute vector's length is
/// checked against `position.len()` before its pointer crosses the boundary. Panics like the reference on any error.
pub fn build_octree_out_of_core(
    output_directory: impl AsRef<Path>,
    resolution: f64,
    bounding_box: Aabb,
    input: impl Iterator<Item = PointsBatch>,
    attributes: &[&str],
    max_points_per_pass: u64,
) -> PcvOocStats {
    let want_intensity = attributes.contains(&"intensity");
    CONTEXT.with(|ctx| {
        let params = PcvBuildParams {
            resolution,
            bbox_min: [bounding_box.min().x, bounding_box.min().y, bounding_box.min().z],
            bbox_max: [bounding_box.max().x, bounding_box.max().y, bounding_box.max().z],
            max_points_per_node: 0,
            flags: 0,
        };
        let mut ooc = std::ptr::null_mut();
        ctx.check(unsafe { pcv_ooc_begin(ctx.0, &params, want_intensity as c_int, max_points_per_pass, &mut ooc) });
        for batch in input {
            let n = batch.position.len();
            let color = match batch.attributes.get("color") {
                Some(AttributeData::U8Vec3(c)) if c.len() == n => c.as_ptr() as *const u8,
                Some(AttributeData::U8Vec3(c)) => {
                    unsafe { pcv_ooc_abort(ooc) };
                    panic!("color has {} entries for {} positions", c.len(), n)
                }
                _ => {
                    unsafe { pcv_ooc_abort(ooc) };
                    panic!("color attribute (U8Vec3) is required") // on_disk.rs:20-22
                }
            };
            let intensity = if want_intensity {
                match batch.attributes.get("intensity") {
                    Some(AttributeData::F32(i)) if i.len() == n => i.as_ptr(),
                    _ => {
                        unsafe { pcv_ooc_abort(ooc) };
                        panic!("intensity requested but missing or not one value per position") // generation.rs:167-177
                    }
                }
            } else {
                std::ptr::null()
            };
            let rc = unsafe { pcv_ooc_append(ooc, batch.position.as_ptr() as *const c_double, color, intensity, n as u64) };
            if rc != 0 {
                unsafe { pcv_ooc_abort(ooc) };
                ctx.check(rc);
            }
        }
        let dir = CString::new(output_directory.as_ref().to_str().unwrap()).unwrap();
        let mut stats = PcvOocStats::default();
        ctx.check(unsafe { pcv_ooc_finish(ooc, dir.as_ptr(), &mut stats) }); // consumes the handle whatever it returns
        stats
    })
}

/// Same signature and behaviour as `point_viewer::octree::build_octree_from_file` (generation.rs:272-287), which is what
/// `src/bin/build_octree.rs:47-52` calls: the PLY's vertex records go to the device as they are in the file and are
/// decoded there (cast to f64 + `comment offset`, ply.rs:488-493), the bounding box is computed on the device
/// (find_bounding_box, generation.rs:256-270), then build + directory write. Panics like the reference on any error,
/// including a PLY without the `intensity` the attribute list asks for.
pub fn build_octree_from_file(output_directory: impl AsRef<Path>, resolution: f64, filename: impl AsRef<Path>, attributes: &[&str]) {
    CONTEXT.with(|ctx| {
        let params = PcvBuildParams { resolution, bbox_min: [0.0; 3], bbox_max: [0.0; 3], max_points_per_node: 0, flags: 0 };
        let file = CString::new(filename.as_ref().to_str().unwrap()).unwrap();
        let mut tree = std::ptr::null_mut();
        let with_intensity = attributes.contains(&"intensity") as c_int;
        ctx.check(unsafe { pcv_build_octree_from_ply(ctx.0, &params, file.as_ptr(), with_intensity, &mut tree) });
        let dir = CString::new(output_directory.as_ref().to_str().unwrap()).unwrap();
        ctx.check(unsafe { pcv_octree_write_dir(tree, dir.as_ptr()) });
        unsafe { pcv_octree_free(tree) };
    });
}

/// `Octree::get_visible_nodes` (octree/mod.rs:228-283) for one matrix over an octree directory.
pub fn get_visible_nodes(ctx: &HipContext, directory: &Path, projection_matrix: &Matrix4<f64>) -> Vec<NodeId> {
    let dir = CString::new(directory.to_str().unwrap()).unwrap();
    let mut tree = std::ptr::null_mut();
    ctx.check(unsafe { pcv_octree_open_dir(ctx.0, dir.as_ptr(), &mut tree) });
    let mut shape = PcvShape { kind: 2, reserved: 0, params: [0.0; 32] };
    shape.params[..16].copy_from_slice(projection_matrix.as_slice()); // nalgebra storage is column-major
    let mut shapes = std::ptr::null_mut();
    ctx.check(unsafe { pcv_shapes_create(ctx.0, &shape, 1, &mut shapes) });
    let m = unsafe { pcv_octree_num_nodes(tree) } as usize;
    let (mut count, mut status) = (0u32, 0i32);
    let mut idx = vec![0u32; m.max(1)];
    ctx.check(unsafe { pcv_visible_nodes(ctx.0, shapes, tree, m as u32, &mut count, idx.as_mut_ptr(), &mut status) });
    assert!(status == 0, "Invalid projection matrix."); // octree/mod.rs:230 .expect(...)
    let ids = idx[..count as usize]
        .iter()
        .map(|&i| {
            let mut info = PcvNodeInfo::default();
            unsafe { pcv_octree_node(tree, i as u64, &mut info) };
            NodeId::from_level_index(info.level as u8, ((info.id_high as u128 & 0x00ff_ffff_ffff_ffff) << 64) | info.id_low as u128)
        })
        .collect();
    unsafe {
        pcv_shapes_free(shapes);
        pcv_octree_free(tree);
    }
    ids
}


// ------------------------------------------------------------------------------------------------------------------
// PointCloud over an octree directory: what ParallelIterator (src/iterator.rs:226-333), PointCloudClient
// (point_cloud_client/src/lib.rs:27-50) and xray tile generation (xray/src/generation.rs:464-513) call.
// ------------------------------------------------------------------------------------------------------------------

/// An octree on disk served by the GPU library. The reference `Octree` is kept alongside for the two things that stay
/// on the host: `points_in_node` (a plain `NodeIterator` over one node's files) and locations the library has no
/// kernel for (S2 cells, web-mercator rectangles: third-party math).
pub struct HipOctree {
    ctx: HipContext,
    tree: *mut pcv_octree,
    lock: Mutex<BatchCache>, // a pcv_ctx is not thread-safe; ParallelIterator calls from several workers
    ids: Vec<NodeId>,
    index_of: HashMap<NodeId, u64>,
    infos: Vec<PcvNodeInfo>,
    inner: Octree,
}

// The raw handles are only touched under `lock`.
unsafe impl Send for HipOctree {}
unsafe impl Sync for HipOctree {}

/// Locations the library offers beyond the reference's `PointLocation` (which has no polygon variant): rings of (x, y) vertices
/// under the even-odd rule, each ring implicitly closed — in the cloud's own x and y with a closed height range, or, with
/// `web_mercator`, as normalized web-mercator coordinates over an ECEF cloud (z_min / z_max then -inf / +inf).
pub enum HipLocation {
    Polygon { rings: Vec<Vec<nalgebra::Point2<f64>>>, z_min: f64, z_max: f64, web_mercator: bool },
}

impl HipOctree {
    pub fn from_directory(directory: impl AsRef<Path>) -> Result<Self> {
        let ctx = HipContext::new(0).map_err(|e| ErrorKind::InvalidInput(e))?;
        let dir = CString::new(directory.as_ref().to_str().unwrap()).unwrap();
        let mut tree = std::ptr::null_mut();
        if unsafe { pcv_octree_open_dir(ctx.0, dir.as_ptr(), &mut tree) } != 0 {
            let msg = unsafe { CStr::from_ptr(pcv_last_error(ctx.0)) }.to_string_lossy().into_owned();
            return Err(ErrorKind::InvalidInput(msg).into());
        }
        let m = unsafe { pcv_octree_num_nodes(tree) };
        let mut ids = Vec::with_capacity(m as usize);
        let mut infos = Vec::with_capacity(m as usize);
        let mut index_of = HashMap::with_capacity(m as usize);
        for i in 0..m {
            let mut info = PcvNodeInfo::default();
            unsafe { pcv_octree_node(tree, i, &mut info) };
            let id = NodeId::from_level_index(info.level as u8, ((info.id_high as u128 & 0x00ff_ffff_ffff_ffff) << 64) | info.id_low as u128);
            index_of.insert(id, i);
            ids.push(id);
            infos.push(info);
        }
        let inner = Octree::from_data_provider(Box::new(OnDiskDataProvider { directory: directory.as_ref().to_path_buf() }))?;
        Ok(HipOctree { ctx, tree, lock: Mutex::new(BatchCache::default()), ids, index_of, infos, inner })
    }

    /// PointLocation -> pcv_shape (include/pcv_hip.h). None: a location the library has no kernel for.
    /// Needs `Frustum::clip_from_query()/query_from_clip()` and `Obb::query_from_obb()/half_extent()` accessors on
    /// the reference types (their fields are private; INTEGRATION.md lists the four one-liners), and
    /// `WebMercatorRect::north_west()/south_east()` (two more).
    fn shape_of(location: &PointLocation) -> Option<PcvShape> {
        let mut s = PcvShape { kind: 0, reserved: 0, params: [0.0; 32] };
        match location {
            PointLocation::AllPoints => s.kind = 0,
            PointLocation::Aabb(b) => {
                s.kind = 1;
                s.params[..3].copy_from_slice(&[b.min().x, b.min().y, b.min().z]);
                s.params[3..6].copy_from_slice(&[b.max().x, b.max().y, b.max().z]);
            }
            PointLocation::Frustum(f) => {
                s.kind = 4; // PCV_SHAPE_FRUSTUM_WITH_INVERSE: exactly the two matrices Frustum::new stored
                s.params[..16].copy_from_slice(f.clip_from_query().as_slice());
                s.params[16..32].copy_from_slice(f.query_from_clip().as_slice());
            }
            PointLocation::Obb(o) => {
                s.kind = 3;
                let iso = o.query_from_obb();
                let (t, q, h) = (iso.translation.vector, iso.rotation.coords, o.half_extent());
                s.params[..3].copy_from_slice(&[t.x, t.y, t.z]);
                s.params[3..7].copy_from_slice(&[q.x, q.y, q.z, q.w]); // i j k w
                s.params[7..10].copy_from_slice(&[h.x, h.y, h.z]);
            }
            PointLocation::WebMercatorRect(r) => {
                // PCV_SHAPE_WEB_MERCATOR_RECT: the two normalized coordinates. WebMercatorCoord's field is private too, but
                // to_zoomed_coordinate(0) is 256 * normalized (web_mercator.rs:70-78) and a division by 256 undoes it exactly.
                s.kind = 5;
                let nw = r.north_west().to_zoomed_coordinate(0)? / 256.0;
                let se = r.south_east().to_zoomed_coordinate(0)? / 256.0;
                s.params[..4].copy_from_slice(&[nw.x, nw.y, se.x, se.y]);
            }
            // PCV_SHAPE_S2_CELL_UNION: no parameters; the union's cells travel beside the shape (union_cells, create_shapes)
            PointLocation::S2Cells(_) => s.kind = 6,
        }
        Some(s)
    }

    /// The cells of a cell-union location as pcv_shapes_create_ex takes them (ascending, as given otherwise: the library does
    /// not normalize, and neither does the reference); empty for every other location.
    fn union_cells(location: &PointLocation) -> Vec<u64> {
        match location {
            PointLocation::S2Cells(u) => {
                let mut v: Vec<u64> = u.0.iter().map(|c| c.0).collect();
                v.sort_unstable();
                v
            }
            _ => Vec::new(),
        }
    }

    /// One prepared table: `cells[i]` are the cells of shape i where it is a cell union (each such shape gets a union of its
    /// own, named by `reserved`), ignored otherwise.
    fn create_shapes(&self, shapes: &[PcvShape], cells: &[Vec<u64>]) -> *mut pcv_shapes {
        let mut table = shapes.to_vec();
        let mut first = vec![0u32];
        let mut flat: Vec<u64> = Vec::new();
        for (s, c) in table.iter_mut().zip(cells) {
            if s.kind == 6 {
                s.reserved = (first.len() - 1) as i32;
                flat.extend_from_slice(c);
                first.push(flat.len() as u32);
            }
        }
        let mut out = std::ptr::null_mut();
        self.ctx.check(unsafe {
            if first.len() == 1 {
                pcv_shapes_create(self.ctx.0, table.as_ptr(), table.len() as u32, &mut out)
            } else {
                pcv_shapes_create_ex(self.ctx.0, table.as_ptr(), table.len() as u32, (first.len() - 1) as u32, first.as_ptr(), flat.as_ptr(), &mut out)
            }
        });
        out
    }

    /// One prepared table of polygon locations (PCV_SHAPE_POLYGON): shape i is `locations[i]`, each with a polygon
    /// of its own, named by `reserved`.
    pub fn create_polygon_shapes(&self, locations: &[HipLocation]) -> *mut pcv_shapes {
        let (mut table, mut polygon_first, mut ring_first, mut vertices) = (Vec::new(), vec![0u32], vec![0u32], Vec::<f64>::new());
        for location in locations {
            let HipLocation::Polygon { rings, z_min, z_max, web_mercator } = location;
            let mut s = PcvShape { kind: 7, reserved: (polygon_first.len() - 1) as i32, params: [0.0; 32] };
            s.params[..3].copy_from_slice(&[*z_min, *z_max, if *web_mercator { 1.0 } else { 0.0 }]);
            table.push(s);
            for ring in rings {
                for v in ring {
                    vertices.extend_from_slice(&[v.x, v.y]);
                }
                ring_first.push((vertices.len() / 2) as u32);
            }
            polygon_first.push((ring_first.len() - 1) as u32);
        }
        let mut out = std::ptr::null_mut();
        self.ctx.check(unsafe {
            pcv_shapes_create_ex2(self.ctx.0, table.as_ptr(), table.len() as u32, 0, std::ptr::null(), std::ptr::null(), (polygon_first.len() - 1) as u32,
                                  polygon_first.as_ptr(), ring_first.as_ptr(), vertices.as_ptr(), &mut out)
        });
        out
    }

    fn with_shape<R>(&self, shape: &PcvShape, cells: &[u64], f: impl FnOnce(*mut pcv_shapes) -> R) -> R {
        let shapes = self.create_shapes(std::slice::from_ref(shape), &[cells.to_vec()]);
        let r = f(shapes);
        unsafe { pcv_shapes_free(shapes) };
        r
    }
}

impl Drop for HipOctree {
    fn drop(&mut self) {
        for e in self.lock.get_mut().unwrap().entries.drain(..) {
            unsafe { pcv_query_batch_free(e.batch) } // before the tree its points are read from
        }
        unsafe { pcv_octree_free(self.tree) } // before the context (field order: ctx is dropped after this body)
    }
}

/// One live pcv_query_batch: a query's points of every node of its location, culled once and kept on the device.
struct BatchEntry {
    key: String, // Debug form of (location, intervals, attributes)
    batch: *mut pcv_query_batch,
    node_segment: HashMap<u64, u64>, // node index -> segment (the segments of one shape)
    offset: Vec<u64>,
}

/// The few most recent queries' batches: `stream_points_for_query_in_node` is called once per node of the same query.
#[derive(Default)]
struct BatchCache {
    entries: Vec<BatchEntry>,
}
const BATCH_CACHE_ENTRIES: usize = 4;

fn query_key(query: &PointQuery) -> String {
    format!("{:?}|{:?}|{:?}", query.location, query.filter_intervals, query.attributes)
}

/// Shape + intensity interval of a query the library serves; None: the reference's host path.
fn library_query(query: &PointQuery) -> Option<(PcvShape, Option<[f64; 2]>, Vec<u64>)> {
    if !query.filter_intervals.keys().all(|k| *k == "intensity") {
        return None; // an interval on another attribute
    }
    let shape = HipOctree::shape_of(&query.location)?;
    Some((shape, query.filter_intervals.get("intensity").map(|iv| [iv.lower_bound, iv.upper_bound]), HipOctree::union_cells(&query.location)))
}

/// Host arrays of n points handed to `callback` as PointsBatches of `batch_size` with the query's attributes.
fn emit_points<F>(query: &PointQuery, p: &HostPoints, batch_size: usize, mut callback: F) -> Result<()>
where
    F: FnMut(PointsBatch) -> Result<()>,
{
    let want_intensity = query.attributes.contains(&"intensity");
    let mut at = 0;
    while at < p.n {
        let end = (at + batch_size).min(p.n);
        let position = (at..end).map(|i| Point3::new(p.x[i], p.y[i], p.z[i])).collect();
        let mut attributes = BTreeMap::new();
        if query.attributes.contains(&"color") {
            attributes.insert("color".to_string(), AttributeData::U8Vec3((at..end).map(|i| Vector3::new(p.rgb[3 * i], p.rgb[3 * i + 1], p.rgb[3 * i + 2])).collect()));
        }
        if want_intensity {
            attributes.insert("intensity".to_string(), AttributeData::F32(p.intensity[at..end].to_vec()));
        }
        callback(PointsBatch { position, attributes })?;
        at = end;
    }
    Ok(())
}

struct HostPoints {
    n: usize,
    x: Vec<f64>,
    y: Vec<f64>,
    z: Vec<f64>,
    rgb: Vec<u8>,
    intensity: Vec<f32>,
}

impl HipOctree {
    /// Runs one batch over `shapes` (with per-shape intensity intervals) and returns it with its segment table.
    fn run_batch(&self, shapes: &[PcvShape], cells: &[Vec<u64>], intervals: &[Option<[f64; 2]>]) -> (*mut pcv_query_batch, Vec<u64>, Vec<u32>, Vec<u64>) {
        let mut handle = std::ptr::null_mut();
        let prepared = self.create_shapes(shapes, cells);
        let flat: Vec<f64> = intervals.iter().flat_map(|iv| iv.unwrap_or([0.0, 0.0])).collect();
        let used: Vec<u8> = intervals.iter().map(|iv| iv.is_some() as u8).collect();
        let rc = unsafe { pcv_query_batch_run(self.ctx.0, prepared, self.tree, flat.as_ptr(), used.as_ptr(), &mut handle) };
        unsafe { pcv_shapes_free(prepared) }; // the batch does not need the shapes
        self.ctx.check(rc);
        let (mut nseg, mut npts) = (0u64, 0u64);
        self.ctx.check(unsafe { pcv_query_batch_sizes(handle, &mut nseg, &mut npts) });
        let mut first = vec![0u64; shapes.len() + 1];
        let mut node = vec![0u32; nseg as usize];
        let mut offset = vec![0u64; nseg as usize + 1];
        self.ctx.check(unsafe { pcv_query_batch_segments(handle, first.as_mut_ptr(), node.as_mut_ptr(), offset.as_mut_ptr()) });
        (handle, first, node, offset)
    }

    /// One node through pcv_query_node_points (a node the query's location does not list). Called under `lock`.
    fn node_points_single(&self, shape: &PcvShape, cells: &[u64], interval: Option<[f64; 2]>, node: u64, want_intensity: bool) -> HostPoints {
        let cap = self.infos[node as usize].num_points as usize;
        let mut p = HostPoints { n: 0, x: vec![0f64; cap], y: vec![0f64; cap], z: vec![0f64; cap], rgb: vec![0u8; 3 * cap], intensity: vec![0f32; if want_intensity { cap } else { 0 }] };
        let has_int = unsafe { pcv_octree_has_intensity(self.tree) } != 0;
        let mut count = 0u64;
        self.with_shape(shape, cells, |shapes| {
            self.ctx.check(unsafe {
                pcv_query_node_points(self.ctx.0, shapes, 0, self.tree, node, interval.as_ref().map_or(std::ptr::null(), |iv| iv.as_ptr()), cap as u64, 0,
                                      p.x.as_mut_ptr(), p.y.as_mut_ptr(), p.z.as_mut_ptr(), p.rgb.as_mut_ptr(),
                                      if want_intensity && has_int { p.intensity.as_mut_ptr() } else { std::ptr::null_mut() }, &mut count)
            })
        });
        p.n = count as usize;
        p
    }

    /// Segments [first, first + count) of a batch to host arrays.
    fn batch_points(&self, batch: *mut pcv_query_batch, offset: &[u64], first: u64, count: u64, want_intensity: bool) -> HostPoints {
        let n = (offset[(first + count) as usize] - offset[first as usize]) as usize;
        let mut p = HostPoints { n, x: vec![0f64; n], y: vec![0f64; n], z: vec![0f64; n], rgb: vec![0u8; 3 * n], intensity: vec![0f32; if want_intensity { n } else { 0 }] };
        if n > 0 {
            let has_int = unsafe { pcv_octree_has_intensity(self.tree) } != 0;
            self.ctx.check(unsafe {
                pcv_query_batch_points(batch, first, count, n as u64, 0, p.x.as_mut_ptr(), p.y.as_mut_ptr(), p.z.as_mut_ptr(), p.rgb.as_mut_ptr(),
                                       if want_intensity && has_int { p.intensity.as_mut_ptr() } else { std::ptr::null_mut() })
            });
        }
        p
    }

    /// xray-style tile batches: the points of every query, `f(query index, batch)` in query order. The queries the library
    /// serves go through pcv_query_batch_run together; the others keep the reference's host path, node by node.
    pub fn query_many<F>(&self, queries: &[PointQuery], batch_size: usize, mut f: F) -> Result<()>
    where
        F: FnMut(usize, PointsBatch) -> Result<()>,
    {
        let served: Vec<Option<(PcvShape, Option<[f64; 2]>, Vec<u64>)>> = queries.iter().map(library_query).collect();
        let shapes: Vec<PcvShape> = served.iter().flatten().map(|(s, _, _)| *s).collect();
        let intervals: Vec<Option<[f64; 2]>> = served.iter().flatten().map(|(_, iv, _)| *iv).collect();
        let cells: Vec<Vec<u64>> = served.iter().flatten().map(|(_, _, c)| c.clone()).collect();
        let mut batch = None;
        if !shapes.is_empty() {
            let _g = self.lock.lock().unwrap();
            batch = Some(self.run_batch(&shapes, &cells, &intervals));
        }
        let mut s = 0usize;
        let mut result = Ok(());
        for (q, query) in queries.iter().enumerate() {
            result = if served[q].is_some() {
                let (handle, first, _, offset) = batch.as_ref().unwrap();
                let p = {
                    let _g = self.lock.lock().unwrap();
                    self.batch_points(*handle, offset, first[s], first[s + 1] - first[s], query.attributes.contains(&"intensity"))
                };
                s += 1;
                emit_points(query, &p, batch_size, |b| f(q, b))
            } else {
                self.nodes_in_location(&query.location).into_iter().try_for_each(|id| self.stream_points_for_query_in_node(query, id, batch_size, |b| f(q, b)))
            };
            if result.is_err() {
                break;
            }
        }
        if let Some((handle, ..)) = batch {
            let _g = self.lock.lock().unwrap();
            unsafe { pcv_query_batch_free(handle) };
        }
        result
    }

    /// The points of every query into ONE binary PLY, query after query: what a PlyNodeWriter with Encoding::Plain fed from
    /// stream_points_for_query would write (ply.rs:559-732) — double positions, then the attributes of the FIRST query's
    /// `attributes` list ascending by name — with the rows packed on the device and written in pieces, so no point crosses
    /// to the host as a PointsBatch. OpenMode::Append adds to a file of the same columns. Every query must be one the library
    /// serves (as in query_many); queries without points leave no file. Returns the number of points written.
    pub fn write_ply(&self, queries: &[PointQuery], path: impl AsRef<Path>, open_mode: OpenMode) -> Result<u64> {
        let served: Vec<Option<(PcvShape, Option<[f64; 2]>, Vec<u64>)>> = queries.iter().map(library_query).collect();
        if queries.is_empty() || served.iter().any(|s| s.is_none()) {
            return Err(ErrorKind::InvalidInput("write_ply: every query must be one the library serves".to_string()).into());
        }
        let shapes: Vec<PcvShape> = served.iter().flatten().map(|(s, _, _)| *s).collect();
        let intervals: Vec<Option<[f64; 2]>> = served.iter().flatten().map(|(_, iv, _)| *iv).collect();
        let cells: Vec<Vec<u64>> = served.iter().flatten().map(|(_, _, c)| c.clone()).collect();
        let names: Vec<CString> = queries[0].attributes.iter().map(|a| CString::new(*a).expect("attribute name with a NUL byte")).collect();
        let name_ptrs: Vec<*const c_char> = names.iter().map(|n| n.as_ptr()).collect();
        let file = CString::new(path.as_ref().to_str().unwrap()).unwrap();
        let params = PcvPlyWriteParams {
            struct_size: std::mem::size_of::<PcvPlyWriteParams>() as u32,
            open_mode: match open_mode {
                OpenMode::Truncate => 0,
                OpenMode::Append => 1,
            },
            attributes: name_ptrs.as_ptr(),
            num_attributes: name_ptrs.len() as u32,
            reserved: 0,
            chunk_points: 0,
        };
        let _g = self.lock.lock().unwrap();
        let (handle, _, _, offset) = self.run_batch(&shapes, &cells, &intervals);
        let mut written = 0u64;
        let rc = unsafe { pcv_query_batch_write_ply(handle, 0, offset.len() as u64 - 1, file.as_ptr(), &params, &mut written) };
        let msg = if rc != 0 { unsafe { CStr::from_ptr(pcv_last_error(self.ctx.0)) }.to_string_lossy().into_owned() } else { String::new() };
        unsafe { pcv_query_batch_free(handle) };
        if rc != 0 {
            return Err(ErrorKind::InvalidInput(format!("write_ply failed ({}): {}", rc, msg)).into());
        }
        Ok(written)
    }

    /// The points of `queries`, one after another, as an ASPRS LAS file: format 2 in LAS 1.2 (colour; intensity if
    /// the octree carries it), coordinates quantised at `scale` around floor(min) per axis, the records packed on the device and
    /// written in pieces. OpenMode::Append adds to a file of the same format, whose scale and offset are used. Queries without
    /// points leave no file. Returns what the library reports about the records written.
    pub fn write_las(&self, queries: &[PointQuery], path: impl AsRef<Path>, scale: f64, open_mode: OpenMode) -> Result<PcvLasWriteInfo> {
        let served: Vec<Option<(PcvShape, Option<[f64; 2]>, Vec<u64>)>> = queries.iter().map(library_query).collect();
        if queries.is_empty() || served.iter().any(|s| s.is_none()) {
            return Err(ErrorKind::InvalidInput("write_las: every query must be one the library serves".to_string()).into());
        }
        let shapes: Vec<PcvShape> = served.iter().flatten().map(|(s, _, _)| *s).collect();
        let intervals: Vec<Option<[f64; 2]>> = served.iter().flatten().map(|(_, iv, _)| *iv).collect();
        let cells: Vec<Vec<u64>> = served.iter().flatten().map(|(_, _, c)| c.clone()).collect();
        let file = CString::new(path.as_ref().to_str().unwrap()).unwrap();
        let mut params: PcvLasWriteParams = unsafe { std::mem::zeroed() };
        params.struct_size = std::mem::size_of::<PcvLasWriteParams>() as u32;
        params.open_mode = match open_mode {
            OpenMode::Truncate => 0,
            OpenMode::Append => 1,
        };
        params.point_format = 255; // PCV_LAS_FORMAT_AUTO
        params.scale = [scale; 3];
        params.auto_offset = 1;
        let _g = self.lock.lock().unwrap();
        let (handle, _, _, offset) = self.run_batch(&shapes, &cells, &intervals);
        let mut info: PcvLasWriteInfo = unsafe { std::mem::zeroed() };
        let rc = unsafe { pcv_query_batch_write_las(handle, 0, offset.len() as u64 - 1, file.as_ptr(), &params, &mut info) };
        let msg = if rc != 0 { unsafe { CStr::from_ptr(pcv_last_error(self.ctx.0)) }.to_string_lossy().into_owned() } else { String::new() };
        unsafe { pcv_query_batch_free(handle) };
        if rc != 0 {
            return Err(ErrorKind::InvalidInput(format!("write_las failed ({}): {}", rc, msg)).into());
        }
        Ok(info)
    }
}

impl HipOctree {
    /// A LAS file as an octree: `pcv_build_octree_from_las` (records decoded and filtered on the device, bounding box computed
    /// there), the directory written, and the directory opened as `from_directory` does. The reference has no LAS reader; the
    /// contract is DESIGN §9j. Uncompiled, like the rest of this veneer.
    pub fn from_las(output_directory: impl AsRef<Path>, resolution: f64, filename: impl AsRef<Path>, las: &PcvLasParams) -> Result<Self> {
        let ctx = HipContext::new(0).map_err(|e| ErrorKind::InvalidInput(e))?;
        let params = PcvBuildParams { resolution, bbox_min: [0.0; 3], bbox_max: [0.0; 3], max_points_per_node: 0, flags: 0 };
        let file = CString::new(filename.as_ref().to_str().unwrap()).unwrap();
        let dir = CString::new(output_directory.as_ref().to_str().unwrap()).unwrap();
        let mut tree = std::ptr::null_mut();
        let mut rc = unsafe { pcv_build_octree_from_las(ctx.0, &params, file.as_ptr(), las, &mut tree) };
        if rc == 0 {
            rc = unsafe { pcv_octree_write_dir(tree, dir.as_ptr()) };
        }
        let msg = if rc != 0 { unsafe { CStr::from_ptr(pcv_last_error(ctx.0)) }.to_string_lossy().into_owned() } else { String::new() };
        unsafe { pcv_octree_free(tree) };
        if rc != 0 {
            return Err(ErrorKind::InvalidInput(format!("from_las failed ({}): {}", rc, msg)).into());
        }
        drop(ctx);
        HipOctree::from_directory(output_directory)
    }

    /// This octree as an OGC 3D Tiles 1.0 tileset: `<dir>/tileset.json` and one `<NodeId>.pnts` per node that holds points,
    /// packed on the device (`pcv_tiles3d_plan` + `pcv_tiles3d_write_dir`). Returns what was written.
    pub fn tiles3d(&self, params: &PcvTiles3dParams, output_directory: impl AsRef<Path>) -> Result<PcvTiles3dInfo> {
        let dir = CString::new(output_directory.as_ref().to_str().unwrap()).unwrap();
        let _g = self.lock.lock().unwrap();
        let mut t: *mut pcv_tiles3d = std::ptr::null_mut();
        let mut info = PcvTiles3dInfo::default();
        let mut rc = unsafe { pcv_tiles3d_plan(self.tree, params, &mut t) };
        if rc == 0 {
            rc = unsafe { pcv_tiles3d_write_dir(t, dir.as_ptr()) };
        }
        if rc == 0 {
            rc = unsafe { pcv_tiles3d_info_get(t, &mut info) };
        }
        let msg = if rc != 0 { unsafe { CStr::from_ptr(pcv_last_error(self.ctx.0)) }.to_string_lossy().into_owned() } else { String::new() };
        unsafe { pcv_tiles3d_free(t) };
        if rc != 0 {
            return Err(ErrorKind::InvalidInput(format!("tiles3d failed ({}): {}", rc, msg)).into());
        }
        Ok(info)
    }

    /// The z/x/y map-tile pyramid (`<dir>/<z>/<x>/<y>.png`, `tiles.json`) of the points `queries` select from this ECEF octree,
    /// drawn at `params.zoom` with the parent levels down to `min_zoom`; png_mode: 0 stored, 1 deflate. Every query must be
    /// one the library serves (as in query_many).
    pub fn map_tiles(&self, queries: &[PointQuery], params: &PcvMapTilesParams, min_zoom: u32, png_mode: i32, output_directory: impl AsRef<Path>) -> Result<()> {
        let served: Vec<Option<(PcvShape, Option<[f64; 2]>, Vec<u64>)>> = queries.iter().map(library_query).collect();
        if queries.is_empty() || served.iter().any(|s| s.is_none()) {
            return Err(ErrorKind::InvalidInput("map_tiles: every query must be one the library serves".to_string()).into());
        }
        let shapes: Vec<PcvShape> = served.iter().flatten().map(|(s, _, _)| *s).collect();
        let intervals: Vec<Option<[f64; 2]>> = served.iter().flatten().map(|(_, iv, _)| *iv).collect();
        let cells: Vec<Vec<u64>> = served.iter().flatten().map(|(_, _, c)| c.clone()).collect();
        let dir = CString::new(output_directory.as_ref().to_str().unwrap()).unwrap();
        let _g = self.lock.lock().unwrap();
        let (handle, _, _, offset) = self.run_batch(&shapes, &cells, &intervals);
        let mut m: *mut pcv_maptiles = std::ptr::null_mut();
        let mut rc = unsafe { pcv_maptiles_begin(self.ctx.0, params, &mut m) };
        if rc == 0 {
            rc = unsafe { pcv_maptiles_add_query_batch(m, handle, 0, offset.len() as u64 - 1) };
        }
        if rc == 0 {
            rc = unsafe { pcv_maptiles_finish(m) };
        }
        if rc == 0 {
            rc = unsafe { pcv_maptiles_build_parents(m, min_zoom) };
        }
        if rc == 0 {
            rc = unsafe { pcv_maptiles_write_dir(m, dir.as_ptr(), png_mode) };
        }
        let msg = if rc != 0 { unsafe { CStr::from_ptr(pcv_last_error(self.ctx.0)) }.to_string_lossy().into_owned() } else { String::new() };
        unsafe {
            pcv_maptiles_free(m);
            pcv_query_batch_free(handle);
        }
        if rc != 0 {
            return Err(ErrorKind::InvalidInput(format!("map_tiles failed ({}): {}", rc, msg)).into());
        }
        Ok(())
    }

    /// The terrain layer `sdl_viewer --terrain <dir>` reads, of the points `queries` select, over this octree's bounding box:
    /// the queries' segments go into the grid on the device, one after the other (a point that two queries select counts
    /// twice). Every query must be one the library serves (as in query_many).
    pub fn terrain(&self, queries: &[PointQuery], params: &PcvTerrainParams, output_directory: impl AsRef<Path>) -> Result<()> {
        let served: Vec<Option<(PcvShape, Option<[f64; 2]>, Vec<u64>)>> = queries.iter().map(library_query).collect();
        if queries.is_empty() || served.iter().any(|s| s.is_none()) {
            return Err(ErrorKind::InvalidInput("terrain: every query must be one the library serves".to_string()).into());
        }
        let shapes: Vec<PcvShape> = served.iter().flatten().map(|(s, _, _)| *s).collect();
        let intervals: Vec<Option<[f64; 2]>> = served.iter().flatten().map(|(_, iv, _)| *iv).collect();
        let cells: Vec<Vec<u64>> = served.iter().flatten().map(|(_, _, c)| c.clone()).collect();
        let dir = CString::new(output_directory.as_ref().to_str().unwrap()).unwrap();
        let bbox = self.bounding_box();
        let (lo, hi) = ([bbox.min().x, bbox.min().y, bbox.min().z], [bbox.max().x, bbox.max().y, bbox.max().z]);
        let _g = self.lock.lock().unwrap();
        let (handle, _, _, offset) = self.run_batch(&shapes, &cells, &intervals);
        let mut t: *mut pcv_terrain = std::ptr::null_mut();
        let mut rc = unsafe { pcv_terrain_begin(self.ctx.0, params, lo.as_ptr(), hi.as_ptr(), &mut t) };
        if rc == 0 {
            rc = unsafe { pcv_terrain_add_query_batch(t, handle, 0, offset.len() as u64 - 1) };
        }
        if rc == 0 {
            rc = unsafe { pcv_terrain_finish(t) };
        }
        if rc == 0 {
            rc = unsafe { pcv_terrain_write_dir(t, dir.as_ptr()) };
        }
        let msg = if rc != 0 { unsafe { CStr::from_ptr(pcv_last_error(self.ctx.0)) }.to_string_lossy().into_owned() } else { String::new() };
        unsafe {
            pcv_terrain_free(t);
            pcv_query_batch_free(handle);
        }
        if rc != 0 {
            return Err(ErrorKind::InvalidInput(format!("terrain failed ({}): {}", rc, msg)).into());
        }
        Ok(())
    }
}

impl PointCloud for HipOctree {
    type Id = NodeId;

    /// src/octree/mod.rs:329-331 + octree_iterator.rs: breadth first, a node is reported iff its cube is not Out.
    fn nodes_in_location(&self, location: &PointLocation) -> Vec<NodeId> {
        let shape = match Self::shape_of(location) {
            Some(s) => s,
            None => return self.inner.nodes_in_location(location),
        };
        let _g = self.lock.lock().unwrap();
        self.with_shape(&shape, &Self::union_cells(location), |shapes| {
            let cap = self.ids.len().max(1);
            let mut count = 0u32;
            let mut idx = vec![0u32; cap];
            self.ctx.check(unsafe { pcv_nodes_in_location(self.ctx.0, shapes, self.tree, cap as u32, &mut count, idx.as_mut_ptr()) });
            idx[..count as usize].iter().map(|&i| self.ids[i as usize]).collect()
        })
    }

    /// src/octree/mod.rs:76-84
    fn encoding_for_node(&self, id: NodeId) -> Encoding {
        let info = &self.infos[self.index_of[&id] as usize];
        let enc = match info.encoding {
            1 => PositionEncoding::Uint8,
            2 => PositionEncoding::Uint16,
            3 => PositionEncoding::Float32,
            _ => PositionEncoding::Float64,
        };
        Encoding::ScaledToCube(Point3::new(info.cube_min[0], info.cube_min[1], info.cube_min[2]), info.cube_edge, enc)
    }

    fn points_in_node(&self, attributes: &[&str], node_id: NodeId, batch_size: usize) -> Result<NodeIterator> {
        self.inner.points_in_node(attributes, node_id, batch_size)
    }

    fn bounding_box(&self) -> &Aabb {
        self.inner.bounding_box()
    }

    /// src/iterator.rs:185-205: decode + FilteredIterator + retain of ONE node on the GPU (decode on load from the
    /// node's bytes, keep mask, stable compaction), handed to the callback in batches of `batch_size`; an `Err` from
    /// the callback aborts the stream like in the reference.
    fn stream_points_for_query_in_node<F>(&self, query: &PointQuery, node_id: NodeId, batch_size: usize, mut callback: F) -> Result<()>
    where
        F: FnMut(PointsBatch) -> Result<()>,
    {
        let (shape, interval, cells) = match library_query(query) {
            Some(v) => v,
            None => {
                // no kernel for this location / an interval on another attribute: the reference's host path
                let it = self.inner.points_in_node(&query.attributes, node_id, batch_size)?;
                return point_viewer::iterator::stream_dispatch(&query.location, &query.filter_intervals, it, callback);
            }
        };
        let node = self.index_of[&node_id];
        if self.infos[node as usize].num_points == 0 {
            return Ok(());
        }
        // one pcv_query_batch_run per distinct query (ParallelIterator hands its nodes over one by one); each node then costs
        // one copy of its segment — no shape, no cull
        let key = query_key(query);
        let points = {
            let mut cache = self.lock.lock().unwrap();
            let k = match cache.entries.iter().position(|e| e.key == key) {
                Some(k) => k,
                None => {
                    let (batch, _, nodes, offset) = self.run_batch(&[shape], &[cells.clone()], &[interval]);
                    let node_segment = nodes.iter().enumerate().map(|(k, &n)| (n as u64, k as u64)).collect();
                    if cache.entries.len() == BATCH_CACHE_ENTRIES {
                        unsafe { pcv_query_batch_free(cache.entries.remove(0).batch) };
                    }
                    cache.entries.push(BatchEntry { key, batch, node_segment, offset });
                    cache.entries.len() - 1
                }
            };
            let e = &cache.entries[k];
            match e.node_segment.get(&node) {
                Some(&seg) => self.batch_points(e.batch, &e.offset, seg, 1, query.attributes.contains(&"intensity")),
                None => self.node_points_single(&shape, &cells, interval, node, query.attributes.contains(&"intensity")), // not in the location's list
            }
        };
        emit_points(query, &points, batch_size, callback)
    }
}

impl HipOctree {
    /// `Octree::get_visible_nodes` (octree/mod.rs:228-283) on the open tree: node ids in the order the reference's
    /// BinaryHeap pops them. Panics like the reference on a matrix that cannot be inverted.
    pub fn get_visible_nodes(&self, projection_matrix: &Matrix4<f64>) -> Vec<NodeId> {
        let mut shape = PcvShape { kind: 2, reserved: 0, params: [0.0; 32] };
        shape.params[..16].copy_from_slice(projection_matrix.as_slice()); // nalgebra storage is column-major
        let _g = self.lock.lock().unwrap();
        self.with_shape(&shape, &[], |shapes| {
            let m = self.ids.len().max(1);
            let (mut count, mut status) = (0u32, 0i32);
            let mut idx = vec![0u32; m];
            self.ctx.check(unsafe { pcv_visible_nodes(self.ctx.0, shapes, self.tree, m as u32, &mut count, idx.as_mut_ptr(), &mut status) });
            assert!(status == 0, "Invalid projection matrix."); // octree/mod.rs:230 .expect(...)
            idx[..count as usize].iter().map(|&i| self.ids[i as usize]).collect()
        })
    }

    /// One frame as `sdl_viewer` draws it (src/lib.rs:158-209: the visible nodes' points as GL_POINTS of `point_size`
    /// pixels under a depth test, colours through `gamma`, over black) for the camera `world_to_gl`, rasterised on the
    /// device: RGBA8, `height` rows of `width` pixels, top row first. `show_octree_nodes` (the viewer's `O` key,
    /// lib.rs:202-208) draws every drawn node's cube as BoxDrawer::draw_outlines does, in the viewer's YELLOW. Panics like
    /// the reference on a matrix that cannot be inverted.
    pub fn render(&self, world_to_gl: &Matrix4<f64>, width: u32, height: u32, point_size: f32, gamma: f32, max_nodes_to_display: usize,
                  show_octree_nodes: bool) -> Vec<u8> {
        let mut shape = PcvShape { kind: 2, reserved: 0, params: [0.0; 32] };
        shape.params[..16].copy_from_slice(world_to_gl.as_slice()); // nalgebra storage is column-major
        let params = PcvRenderParams { width, height, point_size, gamma, max_nodes: max_nodes_to_display.min(u32::MAX as usize) as u32, max_workspace_bytes: 0 };
        let _g = self.lock.lock().unwrap();
        self.with_shape(&shape, &[], |shapes| {
            let mut frame = std::ptr::null_mut();
            let overlay = PcvRenderOverlay { flags: show_octree_nodes as u32, outline_rgba: [255, 255, 0, 255] };
            self.ctx.check(unsafe { pcv_render_views_ex(self.ctx.0, shapes, self.tree, &params, &overlay, &mut frame) });
            let mut rgba = vec![0u8; 4 * width as usize * height as usize];
            let rc = unsafe { pcv_render_images(frame, 0, 1, rgba.as_mut_ptr() as *mut c_void, 0) };
            unsafe { pcv_render_free(frame) };
            self.ctx.check(rc);
            rgba
        })
    }

    /// `render` with the terrain layers of `sdl_viewer --terrain <dir>...` (src/lib.rs:602-606, terrain_drawer/mod.rs:152-187):
    /// every directory is opened on the device and drawn after the nodes as the viewer's wireframe, in a window of
    /// `terrain_window` vertices (the viewer's is 1024) around `camera_position`, the camera's place in the world frame
    /// (the translation of the viewer's `local_from_global` inverse, which `TerrainDrawer::camera_changed` takes).
    pub fn render_with_terrain(&self, world_to_gl: &Matrix4<f64>, camera_position: &[f64; 3], terrain_directories: &[std::path::PathBuf],
                               terrain_window: u32, width: u32, height: u32, point_size: f32, gamma: f32, max_nodes_to_display: usize,
                               show_octree_nodes: bool) -> Vec<u8> {
        use std::os::unix::ffi::OsStrExt;
        let mut shape = PcvShape { kind: 2, reserved: 0, params: [0.0; 32] };
        shape.params[..16].copy_from_slice(world_to_gl.as_slice());
        let params = PcvRenderParams { width, height, point_size, gamma, max_nodes: max_nodes_to_display.min(u32::MAX as usize) as u32, max_workspace_bytes: 0 };
        let _g = self.lock.lock().unwrap();
        let mut layers: Vec<*mut pcv_terrain> = Vec::new();
        for dir in terrain_directories {
            let path = std::ffi::CString::new(dir.as_os_str().as_bytes()).expect("a path without NUL");
            let mut t = std::ptr::null_mut();
            let rc = unsafe { pcv_terrain_open_dir(self.ctx.0, path.as_ptr(), &mut t) };
            if rc != 0 {
                layers.iter().for_each(|&l| unsafe { pcv_terrain_free(l) });
                self.ctx.check(rc);
            }
            layers.push(t);
        }
        let rgba = self.with_shape(&shape, &[], |shapes| {
            let mut frame = std::ptr::null_mut();
            let overlay = PcvRenderOverlay { flags: show_octree_nodes as u32, outline_rgba: [255, 255, 0, 255] };
            let terrain = PcvRenderTerrainLayers { num_layers: layers.len() as u32, window: terrain_window, layers: layers.as_ptr(),
                                                   camera_positions: camera_position.as_ptr() };
            let mut rc = unsafe { pcv_render_views_terrain(self.ctx.0, shapes, self.tree, &params, &overlay, &terrain, &mut frame) };
            let mut rgba = vec![0u8; 4 * width as usize * height as usize];
            if rc == 0 {
                rc = unsafe { pcv_render_images(frame, 0, 1, rgba.as_mut_ptr() as *mut c_void, 0) };
                unsafe { pcv_render_free(frame) };
            }
            (rc, rgba)
        });
        layers.iter().for_each(|&l| unsafe { pcv_terrain_free(l) });
        self.ctx.check(rgba.0);
        rgba.1
    }
}

// ------------------------------------------------------------------------------------------------------------------
// merge_xray_quadtrees (xray/src/bin/merge_xray_quadtrees.rs): partial quadtrees of several directories into one.
// ------------------------------------------------------------------------------------------------------------------
#[repr(C)]
pub struct PcvXray {
    _private: [u8; 0],
}

extern "C" {
    fn pcv_xray_open_dir(ctx: *mut pcv_ctx, directory: *const std::os::raw::c_char, capacity: u32, parts: *mut *mut PcvXray, num_parts: *mut u32) -> i32;
    fn pcv_xray_merge(ctx: *mut pcv_ctx, parts: *const *mut PcvXray, num_parts: u32, background: u32, out: *mut *mut PcvXray) -> i32;
    fn pcv_xray_write_dir_ex(x: *mut PcvXray, directory: *const std::os::raw::c_char, mode: i32) -> i32;
    fn pcv_xray_free(x: *mut PcvXray);
}

/// The body of the reference binary after argument parsing (:207-223): every `meta*.pb` of `input_directories` is opened,
/// validated and merged on the device, and the quadtree with root `r` is written to `output_directory`, which may be one
/// of the inputs. `transparent_background` is `--tile-background-color transparent`. Errors carry the library's message,
/// which for the reference's own checks is the reference's text.
pub fn merge_xray_quadtrees(device: i32, input_directories: &[std::path::PathBuf], output_directory: &std::path::Path, transparent_background: bool) -> std::io::Result<()> {
    merge_xray_quadtrees_png(device, input_directories, output_directory, transparent_background, false)
}

/// `merge_xray_quadtrees` with the PNG mode of the levels the merge builds: `deflate` compresses them on the device
/// (PCV_XRAY_PNG_DEFLATE: Sub / Up filters, run-length deflate); the parts' files are copied as they are either way.
pub fn merge_xray_quadtrees_png(device: i32, input_directories: &[std::path::PathBuf], output_directory: &std::path::Path, transparent_background: bool, deflate: bool) -> std::io::Result<()> {
    use std::os::unix::ffi::OsStrExt;
    let c = |p: &std::path::Path| std::ffi::CString::new(p.as_os_str().as_bytes()).expect("path with a NUL byte");
    let ctx = HipContext::new(device).map_err(|e| std::io::Error::new(std::io::ErrorKind::Other, e))?;
    let mut parts: Vec<*mut PcvXray> = Vec::new();
    let mut rc = 0;
    for dir in input_directories {
        let (name, mut n) = (c(dir), 0u32);
        rc = unsafe { pcv_xray_open_dir(ctx.0, name.as_ptr(), 0, std::ptr::null_mut(), &mut n) };
        if rc != 0 {
            break;
        }
        let at = parts.len();
        parts.resize(at + n as usize, std::ptr::null_mut());
        rc = unsafe { pcv_xray_open_dir(ctx.0, name.as_ptr(), n, parts[at..].as_mut_ptr(), &mut n) };
        if rc != 0 {
            parts.truncate(at);
            break;
        }
    }
    let mut merged = std::ptr::null_mut();
    if rc == 0 {
        rc = unsafe { pcv_xray_merge(ctx.0, parts.as_ptr(), parts.len() as u32, transparent_background as u32, &mut merged) };
    }
    if rc == 0 {
        std::fs::create_dir_all(output_directory)?;
        rc = unsafe { pcv_xray_write_dir_ex(merged, c(output_directory).as_ptr(), deflate as i32) };
    }
    let message = if rc == 0 { String::new() } else { unsafe { CStr::from_ptr(pcv_last_error(ctx.0)) }.to_string_lossy().into_owned() };
    unsafe {
        pcv_xray_free(merged);
        for p in parts {
            pcv_xray_free(p);
        }
    }
    if rc == 0 {
        Ok(())
    } else {
        Err(std::io::Error::new(if rc == -3 { std::io::ErrorKind::Other } else { std::io::ErrorKind::InvalidData }, message))
    }
}


// ------------------------------------------------------------------------------------------------------------------
// PointCloud over an S2 cell cloud directory (src/s2_cells/mod.rs): S2Cells::from_data_provider, nodes_in_location and
// stream_points_for_query_in_node on the GPU library (include/pcv_hip.h, "S2 cell clouds: the region side"). Like the rest
// of this file it is written against the reference's types and has not been compiled here.
// ------------------------------------------------------------------------------------------------------------------
#[repr(C)]
pub struct pcv_s2_cloud {
    _private: [u8; 0],
}
#[repr(C)]
pub struct pcv_s2_query {
    _private: [u8; 0],
}

/// pcv_xray_params / pcv_xray_coloring of include/pcv_hip.h, field for field.
#[repr(C)]
pub struct PcvXrayParams {
    pub tile_size_px: u32,
    pub strategy: u32,
    pub colormap: u32,
    pub background: u32,
    pub pixel_size_m: c_double,
    pub max_stddev: c_float,
    pub root_level: u32,
    pub root_index: u64,
    pub has_query_from_global: i32,
    pub reserved: i32,
    pub query_from_global: [c_double; 7],
    pub interval_attribute: *const c_char,
    pub interval: [c_double; 2],
    pub max_workspace_bytes: u64,
}
#[repr(C)]
pub struct PcvXrayColoring {
    pub min_intensity: c_float,
    pub max_intensity: c_float,
    pub binning_attribute: *const c_char,
    pub bin_size: c_double,
}
/// One `--filter-interval <attribute>=<min>,<max>` (pcv_xray_filter): a ClosedInterval<f64> on a scalar attribute.
#[repr(C)]
pub struct PcvXrayFilter {
    pub attribute: *const c_char,
    pub lo: c_double,
    pub hi: c_double,
}

extern "C" {
    /// pcv_xray_run_s2 with filters and binning on any scalar attribute of the clouds (XrayParameters::filter_intervals,
    /// BinnedColoringStrategy::bins); with no filter and intensity binning it is pcv_xray_run_s2
    fn pcv_xray_run_s2_ex(ctx: *mut pcv_ctx, clouds: *const *mut pcv_s2_cloud, num_clouds: u32, params: *const PcvXrayParams, coloring: *const PcvXrayColoring, filters: *const PcvXrayFilter, num_filters: u32, out: *mut *mut PcvXray) -> c_int;
    /// the checks of pcv_xray_run_s2_ex that need no device
    pub fn pcv_xray_check_attrs_host(params: *const PcvXrayParams, coloring: *const PcvXrayColoring, filters: *const PcvXrayFilter, num_filters: u32, num_clouds: u32, extras_first: *const u32, names: *const *const c_char, data_types: *const i32, has_intensity: *const u8, err: *mut c_char, errcap: u64) -> c_int;
    /// `(data[i] as f64 / bin_size) as i64` for n values of a scalar data type, from the function the device compiles
    pub fn pcv_xray_bins_host(data_type: i32, n: u64, data: *const std::ffi::c_void, bin_size: c_double, out: *mut i64) -> c_int;
    fn pcv_xray_run_s2(ctx: *mut pcv_ctx, clouds: *const *mut pcv_s2_cloud, num_clouds: u32, params: *const PcvXrayParams, coloring: *const PcvXrayColoring, out: *mut *mut PcvXray) -> c_int;
    fn pcv_xray_build_parents(x: *mut PcvXray) -> c_int;
    /// PointCloudClientBuilder::build's choice for a directory (0: octree, 1: S2 cells), by its meta.pb
    pub fn pcv_cloud_kind(directory: *const c_char, kind: *mut c_int) -> c_int;
}

/// An S2 cell cloud on disk served by the GPU library. The reference `S2Cells` is kept alongside for `points_in_node` (a plain
/// `NodeIterator` over one cell's files) and for intervals on attributes other than intensity.
pub struct HipS2Cells {
    ctx: HipContext,
    cloud: *mut pcv_s2_cloud,
    lock: Mutex<()>, // a pcv_ctx is not thread-safe; ParallelIterator calls from several workers
    ids: Vec<s2::cellid::CellID>,
    index_of: HashMap<s2::cellid::CellID, u32>,
    inner: point_viewer::s2_cells::S2Cells,
}

unsafe impl Send for HipS2Cells {}
unsafe impl Sync for HipS2Cells {}

impl HipS2Cells {
    pub fn from_directory(directory: impl AsRef<Path>) -> Result<Self> {
        let ctx = HipContext::new(0).map_err(|e| ErrorKind::InvalidInput(e))?;
        let dir = CString::new(directory.as_ref().to_str().unwrap()).unwrap();
        let mut cloud = std::ptr::null_mut();
        if unsafe { pcv_s2_open_dir(ctx.0, dir.as_ptr(), &mut cloud) } != 0 {
            // the reference's own messages ("No S2 point cloud supported with version N", "This meta does not describe ...")
            let msg = unsafe { CStr::from_ptr(pcv_last_error(ctx.0)) }.to_string_lossy().into_owned();
            return Err(ErrorKind::InvalidInput(msg).into());
        }
        let mut n = 0u64;
        unsafe { pcv_s2_info(cloud, &mut n, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut()) };
        let mut raw = vec![0u64; n as usize];
        unsafe { pcv_s2_cells(cloud, raw.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut()) };
        let ids: Vec<_> = raw.iter().map(|&id| s2::cellid::CellID(id)).collect();
        let index_of = ids.iter().enumerate().map(|(k, id)| (*id, k as u32)).collect();
        let inner = point_viewer::s2_cells::S2Cells::from_data_provider(Box::new(OnDiskDataProvider { directory: directory.as_ref().to_path_buf() }))?;
        Ok(HipS2Cells { ctx, cloud, lock: Mutex::new(()), ids, index_of, inner })
    }

    /// The cells of one location: a prepared shape, or the ascending cell ids of a union (`CellUnion.0`, sorted).
    fn cells_of(&self, shape: Option<&PcvShape>, union: &[u64]) -> Vec<u32> {
        let cap = self.ids.len().max(1);
        let (mut count, mut idx) = (0u32, vec![0u32; cap]);
        let first = [0u32, union.len() as u32];
        let mut shapes = std::ptr::null_mut();
        if let Some(s) = shape {
            self.ctx.check(unsafe { pcv_shapes_create(self.ctx.0, s, 1, &mut shapes) });
        }
        let unions = if shape.is_some() { 0 } else { 1 };
        self.ctx.check(unsafe { pcv_s2_cells_in_location(self.cloud, shapes, unions, first.as_ptr(), union.as_ptr(), cap as u32, &mut count, idx.as_mut_ptr()) });
        if !shapes.is_null() {
            unsafe { pcv_shapes_free(shapes) };
        }
        idx.truncate(count as usize);
        idx
    }

    /// `build_xray_quadtree` over this cloud (PointClouds::S2Cells, point_cloud_client/src/lib.rs:120-131): the leaf tiles
    /// rasterised on the device from the S2 query's candidates (pcv_xray_run_s2), the parents built, the quadtree written to
    /// `output_directory`. `coloring` is needed by colored_with_intensity and binning, as for pcv_xray_run_ex. Several
    /// clouds of one context go through pcv_xray_run_s2 in one call; this veneer holds one.
    pub fn build_xray_quadtree(&self, params: &PcvXrayParams, coloring: Option<&PcvXrayColoring>, output_directory: &Path, deflate: bool) -> Result<()> {
        self.build_xray_quadtree_filtered(params, coloring, &[], output_directory, deflate)
    }

    /// `build_xray_quadtree` with `XrayParameters::filter_intervals` (name, lower bound, upper bound) on any scalar attribute of the cloud, and with a
    /// `coloring.binning_attribute` that may name any scalar attribute (pcv_xray_run_s2_ex).
    pub fn build_xray_quadtree_filtered(&self, params: &PcvXrayParams, coloring: Option<&PcvXrayColoring>, filter_intervals: &[(String, f64, f64)],
                                        output_directory: &Path, deflate: bool) -> Result<()> {
        use std::os::unix::ffi::OsStrExt;
        let _guard = self.lock.lock().unwrap();
        let dir = CString::new(output_directory.as_os_str().as_bytes()).expect("path with a NUL byte");
        let clouds = [self.cloud];
        let mut x = std::ptr::null_mut();
        let names: Vec<CString> = filter_intervals.iter().map(|(name, _, _)| CString::new(name.as_str()).expect("attribute name with a NUL byte")).collect();
        let filters: Vec<PcvXrayFilter> =
            filter_intervals.iter().zip(&names).map(|((_, lo, hi), name)| PcvXrayFilter { attribute: name.as_ptr(), lo: *lo, hi: *hi }).collect();
        let mut rc = unsafe {
            pcv_xray_run_s2_ex(self.ctx.0, clouds.as_ptr(), 1, params, coloring.map_or(std::ptr::null(), |c| c as *const _), filters.as_ptr(), filters.len() as u32, &mut x)
        };
        if rc == 0 {
            rc = unsafe { pcv_xray_build_parents(x) };
        }
        if rc == 0 {
            rc = unsafe { pcv_xray_write_dir_ex(x, dir.as_ptr(), deflate as i32) };
        }
        let message = if rc == 0 { String::new() } else { unsafe { CStr::from_ptr(pcv_last_error(self.ctx.0)) }.to_string_lossy().into_owned() };
        unsafe { pcv_xray_free(x) };
        if rc == 0 {
            Ok(())
        } else {
            Err(ErrorKind::InvalidInput(message).into())
        }
    }

    fn sorted_union(location: &PointLocation) -> Option<Vec<u64>> {
        match location {
            PointLocation::S2Cells(u) => {
                let mut v: Vec<u64> = u.0.iter().map(|c| c.0).collect();
                v.sort_unstable();
                Some(v)
            }
            _ => None,
        }
    }
}

impl Drop for HipS2Cells {
    fn drop(&mut self) {
        unsafe { pcv_s2_free(self.cloud) } // before the context
    }
}

impl PointCloud for HipS2Cells {
    type Id = s2::cellid::CellID;

    /// src/s2_cells/mod.rs:160-169; the list ascends by cell id (the reference: its hash map's order).
    fn nodes_in_location(&self, location: &PointLocation) -> Vec<Self::Id> {
        let _g = self.lock.lock().unwrap();
        let idx = match Self::sorted_union(location) {
            Some(u) => self.cells_of(None, &u),
            None => self.cells_of(Some(&HipOctree::shape_of(location).expect("every other location has a shape")), &[]),
        };
        idx.iter().map(|&i| self.ids[i as usize]).collect()
    }

    fn encoding_for_node(&self, _: Self::Id) -> Encoding {
        Encoding::Plain
    }

    fn points_in_node(&self, attributes: &[&str], node_id: Self::Id, batch_size: usize) -> Result<NodeIterator> {
        self.inner.points_in_node(attributes, node_id, batch_size)
    }

    fn bounding_box(&self) -> &Aabb {
        self.inner.bounding_box()
    }

    /// src/iterator.rs:185-205 for ONE cell: one pcv_s2_query_run over the query's location, the cell's segment copied out.
    /// (A caller that streams many cells of one query should keep the batch, as HipOctree's BatchCache does.)
    fn stream_points_for_query_in_node<F>(&self, query: &PointQuery, node_id: Self::Id, batch_size: usize, callback: F) -> Result<()>
    where
        F: FnMut(PointsBatch) -> Result<()>,
    {
        if !query.filter_intervals.keys().all(|k| *k == "intensity") {
            // an interval on another attribute: the reference's host path
            let it = self.inner.points_in_node(&query.attributes, node_id, batch_size)?;
            return point_viewer::iterator::stream_dispatch(&query.location, &query.filter_intervals, it, callback);
        }
        let interval = query.filter_intervals.get("intensity").map(|iv| [iv.lower_bound, iv.upper_bound]);
        let _g = self.lock.lock().unwrap();
        let union = Self::sorted_union(&query.location);
        let shape = if union.is_none() { HipOctree::shape_of(&query.location) } else { None };
        let mut shapes = std::ptr::null_mut();
        if let Some(s) = &shape {
            self.ctx.check(unsafe { pcv_shapes_create(self.ctx.0, s, 1, &mut shapes) });
        }
        let cells = union.unwrap_or_default();
        let first = [0u32, cells.len() as u32];
        let iv = interval.unwrap_or([0.0, 0.0]);
        let used = [interval.is_some() as u8];
        let mut batch = std::ptr::null_mut();
        self.ctx.check(unsafe {
            pcv_s2_query_run(self.cloud, shapes, if shape.is_some() { 0 } else { 1 }, first.as_ptr(), cells.as_ptr(), iv.as_ptr(), used.as_ptr(), &mut batch)
        });
        let (mut nseg, mut kept) = (0u64, 0u64);
        unsafe { pcv_s2_query_sizes(batch, &mut nseg, &mut kept) };
        let (mut loc_first, mut seg_cell, mut offset) = ([0u64; 2], vec![0u32; nseg as usize], vec![0u64; nseg as usize + 1]);
        unsafe { pcv_s2_query_segments(batch, loc_first.as_mut_ptr(), seg_cell.as_mut_ptr(), offset.as_mut_ptr()) };
        let want = self.index_of[&node_id];
        let want_intensity = query.attributes.contains(&"intensity");
        let mut points = HostPoints { n: 0, x: vec![], y: vec![], z: vec![], rgb: vec![], intensity: vec![] };
        if let Some(seg) = seg_cell.iter().position(|&c| c == want) {
            let n = (offset[seg + 1] - offset[seg]) as usize;
            points = HostPoints { n, x: vec![0.0; n], y: vec![0.0; n], z: vec![0.0; n], rgb: vec![0; 3 * n], intensity: vec![0.0; if want_intensity { n } else { 0 }] };
            let ip = if want_intensity { points.intensity.as_mut_ptr() } else { std::ptr::null_mut() };
            self.ctx.check(unsafe {
                pcv_s2_query_points(batch, seg as u64, 1, n as u64, 0, points.x.as_mut_ptr(), points.y.as_mut_ptr(), points.z.as_mut_ptr(), points.rgb.as_mut_ptr(), ip)
            });
        }
        unsafe { pcv_s2_query_free(batch) };
        if !shapes.is_null() {
            unsafe { pcv_shapes_free(shapes) };
        }
        drop(_g);
        emit_points(query, &points, batch_size, callback)
    }
}

// ------------------------------------------------------------------------------------------------------------------
// S2Splitter over the GPU library (src/read_write/s2.rs:19-173): NodeWriter<PointsBatch> whose `write` hands one batch to
// pcv_s2_stream_append and whose `get_meta` finishes the stream (include/pcv_hip.h, "S2 cell clouds from a stream of
// batches"). Like the rest of this file it is written against the reference's types and has not been compiled here.
// ------------------------------------------------------------------------------------------------------------------
#[repr(C)]
pub struct pcv_s2_stream {
    _private: [u8; 0],
}
/// pcv_attribute of include/pcv_hip.h, field for field: one extra attribute of a batch (every attribute of a PointsBatch but
/// `color` and `intensity`, s2.rs:85-107); data_type is the proto enum value of AttributeDataType.
#[repr(C)]
pub struct PcvAttribute {
    pub name: *const c_char,
    pub data_type: i32,
    pub reserved: u32,
    pub data: *const std::ffi::c_void,
}

/// (proto enum value, first element) of an attribute's column: attributes.rs:8-21; nalgebra's Vector3 is three components in a row.
fn attribute_column(data: &AttributeData) -> (i32, *const std::ffi::c_void, usize) {
    match data {
        AttributeData::U8(v) => (1, v.as_ptr() as *const _, v.len()),
        AttributeData::U16(v) => (2, v.as_ptr() as *const _, v.len()),
        AttributeData::U32(v) => (3, v.as_ptr() as *const _, v.len()),
        AttributeData::U64(v) => (4, v.as_ptr() as *const _, v.len()),
        AttributeData::I8(v) => (6, v.as_ptr() as *const _, v.len()),
        AttributeData::I16(v) => (7, v.as_ptr() as *const _, v.len()),
        AttributeData::I32(v) => (8, v.as_ptr() as *const _, v.len()),
        AttributeData::I64(v) => (9, v.as_ptr() as *const _, v.len()),
        AttributeData::F32(v) => (11, v.as_ptr() as *const _, v.len()),
        AttributeData::F64(v) => (12, v.as_ptr() as *const _, v.len()),
        AttributeData::U8Vec3(v) => (27, v.as_ptr() as *const _, v.len()),
        AttributeData::F64Vec3(v) => (38, v.as_ptr() as *const _, v.len()),
    }
}

/// pcv_s2_stream_params of include/pcv_hip.h, field for field.
#[repr(C)]
pub struct PcvS2StreamParams {
    pub struct_size: u32,
    pub split_level: u32,
    pub directory: *const c_char,
    pub open_mode: i32,
    pub reserved: u32,
    pub flush_points: u64,
}

extern "C" {
    fn pcv_s2_stream_begin(ctx: *mut pcv_ctx, params: *const PcvS2StreamParams, out: *mut *mut pcv_s2_stream) -> c_int;
    fn pcv_s2_stream_append(stream: *mut pcv_s2_stream, batch: *const PcvPoints) -> c_int;
    fn pcv_s2_stream_append_ex(stream: *mut pcv_s2_stream, batch: *const PcvPoints, attrs: *const PcvAttribute, num_attrs: u32) -> c_int;
    fn pcv_s2_stream_info(stream: *const pcv_s2_stream, batches: *mut u64, points: *mut u64, cells: *mut u64, pending_points: *mut u64, flushes: *mut u64) -> c_int;
    fn pcv_s2_stream_finish(stream: *mut pcv_s2_stream, out: *mut *mut pcv_s2_cloud) -> c_int;
    fn pcv_s2_stream_abort(stream: *mut pcv_s2_stream);
}

/// `S2Splitter<RawNodeWriter>` on the device: the cells' files grow flush by flush, `get_meta` writes nothing itself but
/// returns the Meta of what `meta.pb` now says. OpenMode::Append adds to the directory that is there — and, a departure
/// from the reference, counts its points in the Meta.
pub struct S2Stream {
    ctx: HipContext,
    stream: *mut pcv_s2_stream,
    directory: PathBuf,
}

impl S2Stream {
    /// S2Splitter::with_split_level (s2.rs:32-54).
    pub fn with_split_level(split_level: u8, path: impl Into<PathBuf>, open_mode: OpenMode) -> Result<Self> {
        use std::os::unix::ffi::OsStrExt;
        let ctx = HipContext::new(0).map_err(|e| ErrorKind::InvalidInput(e))?;
        let directory: PathBuf = path.into();
        let dir = CString::new(directory.as_os_str().as_bytes()).expect("path with a NUL byte");
        let params = PcvS2StreamParams {
            struct_size: std::mem::size_of::<PcvS2StreamParams>() as u32,
            split_level: split_level as u32,
            directory: dir.as_ptr(),
            open_mode: match open_mode {
                OpenMode::Truncate => 0,
                OpenMode::Append => 1,
            },
            reserved: 0,
            flush_points: 0,
        };
        let mut stream = std::ptr::null_mut();
        if unsafe { pcv_s2_stream_begin(ctx.0, &params, &mut stream) } != 0 {
            let msg = unsafe { CStr::from_ptr(pcv_last_error(ctx.0)) }.to_string_lossy().into_owned();
            return Err(ErrorKind::InvalidInput(msg).into());
        }
        Ok(S2Stream { ctx, stream, directory })
    }

    fn io_error(&self) -> std::io::Error {
        let msg = unsafe { CStr::from_ptr(pcv_last_error(self.ctx.0)) }.to_string_lossy().into_owned();
        std::io::Error::new(std::io::ErrorKind::InvalidInput, msg)
    }

    /// (batches, points, cells, pending points, flushes) so far.
    pub fn info(&self) -> (u64, u64, u64, u64, u64) {
        let mut v = [0u64; 5];
        let p = v.as_mut_ptr();
        unsafe { pcv_s2_stream_info(self.stream, p, p.add(1), p.add(2), p.add(3), p.add(4)) };
        (v[0], v[1], v[2], v[3], v[4])
    }

    /// S2Splitter::get_meta (s2.rs:139-173): the last flush, meta.pb, and the Meta read back from it.
    pub fn get_meta(mut self) -> Result<point_viewer::s2_cells::S2Meta> {
        let stream = std::mem::replace(&mut self.stream, std::ptr::null_mut());
        if unsafe { pcv_s2_stream_finish(stream, std::ptr::null_mut()) } != 0 {
            return Err(ErrorKind::InvalidInput(self.io_error().to_string()).into());
        }
        let provider = OnDiskDataProvider { directory: self.directory.clone() };
        point_viewer::s2_cells::S2Meta::from_proto(provider.meta_proto()?)
    }
}

impl NodeWriter<PointsBatch> for S2Stream {
    /// S2Splitter::new (s2.rs:56-58): DEFAULT_S2_SPLIT_LEVEL; the cells' files are Encoding::Plain whatever `_encoding` says, as
    /// S2Cells reads them. Panics where the stream cannot be begun (no device, OpenMode::Append on a directory that is no S2 cloud).
    fn new(path: impl Into<PathBuf>, _encoding: Encoding, open_mode: OpenMode) -> Self {
        Self::with_split_level(20, path, open_mode).unwrap_or_else(|e| panic!("S2Stream: {}", e))
    }

    /// S2Splitter::write (s2.rs:60-137) for one batch: the positions transposed to the planes pcv_points wants, colour and
    /// intensity as they are, every other attribute as an extra of pcv_s2_stream_append_ex (s2.rs:85-107).
    fn write(&mut self, batch: &PointsBatch) -> std::io::Result<()> {
        let n = batch.position.len();
        let (mut x, mut y, mut z) = (Vec::with_capacity(n), Vec::with_capacity(n), Vec::with_capacity(n));
        for p in &batch.position {
            x.push(p.x);
            y.push(p.y);
            z.push(p.z);
        }
        let color = match batch.attributes.get("color") {
            Some(AttributeData::U8Vec3(c)) if c.len() == n => c.as_ptr() as *const u8,
            _ => return Err(std::io::Error::new(std::io::ErrorKind::InvalidInput, "color attribute (U8Vec3), one per position, is required")),
        };
        let intensity = match batch.attributes.get("intensity") {
            Some(AttributeData::F32(i)) if i.len() == n => i.as_ptr(),
            Some(_) => return Err(std::io::Error::new(std::io::ErrorKind::InvalidInput, "S2Splitter received incompatible data types for attribute intensity")),
            None => std::ptr::null(),
        };
        let points = PcvPoints { n: n as u64, x: x.as_ptr(), y: y.as_ptr(), z: z.as_ptr(), color, color_stride: 3, intensity, mem: 0 };
        let mut names = Vec::new(); // kept alive until the call returns
        let mut extras = Vec::new();
        for (name, data) in batch.attributes.iter().filter(|(k, _)| k.as_str() != "color" && k.as_str() != "intensity") {
            let (data_type, ptr, len) = attribute_column(data);
            if len != n {
                return Err(std::io::Error::new(std::io::ErrorKind::InvalidInput, format!("attribute {} holds {} values for {} positions", name, len, n)));
            }
            names.push(CString::new(name.as_str()).map_err(|e| std::io::Error::new(std::io::ErrorKind::InvalidInput, e))?);
            extras.push(PcvAttribute { name: names.last().unwrap().as_ptr(), data_type, reserved: 0, data: ptr });
        }
        if unsafe { pcv_s2_stream_append_ex(self.stream, &points, extras.as_ptr(), extras.len() as u32) } != 0 {
            return Err(self.io_error());
        }
        Ok(())
    }
}

impl Drop for S2Stream {
    fn drop(&mut self) {
        unsafe { pcv_s2_stream_abort(self.stream) } // (null after get_meta) before the context
    }
}
