/* Struct layouts the FFI mirrors (Rust #[repr(C)] in point_cloud_viewer_amd/rust_shim/src/lib.rs, ctypes in
 * point_cloud_viewer_amd/_lib.py) rely on, asserted by the C and the C++ compiler against include/pcv_hip.h.
 * LP64, natural alignment — what #[repr(C)] lays out on x86_64-unknown-linux-gnu. */
#ifndef PCV_LAYOUT_CHECK_H
#define PCV_LAYOUT_CHECK_H
#include <stddef.h>

#include "pcv_hip.h"

#ifdef __cplusplus
#define PCV_SA(cond, msg) static_assert(cond, msg)
#else
#define PCV_SA(cond, msg) _Static_assert(cond, msg)
#endif

PCV_SA(sizeof(pcv_points) == 64, "pcv_points");
PCV_SA(offsetof(pcv_points, n) == 0 && offsetof(pcv_points, x) == 8 && offsetof(pcv_points, y) == 16 &&
           offsetof(pcv_points, z) == 24 && offsetof(pcv_points, color) == 32 && offsetof(pcv_points, color_stride) == 40 &&
           offsetof(pcv_points, intensity) == 48 && offsetof(pcv_points, mem) == 56,
       "pcv_points fields");
PCV_SA(sizeof(pcv_build_params) == 64, "pcv_build_params");
PCV_SA(offsetof(pcv_build_params, resolution) == 0 && offsetof(pcv_build_params, bbox_min) == 8 &&
           offsetof(pcv_build_params, bbox_max) == 32 && offsetof(pcv_build_params, max_points_per_node) == 56 &&
           offsetof(pcv_build_params, flags) == 60,
       "pcv_build_params fields");
PCV_SA(sizeof(pcv_node_info) == 80, "pcv_node_info");
PCV_SA(offsetof(pcv_node_info, id_high) == 0 && offsetof(pcv_node_info, id_low) == 8 && offsetof(pcv_node_info, num_points) == 16 &&
           offsetof(pcv_node_info, level) == 24 && offsetof(pcv_node_info, encoding) == 28 && offsetof(pcv_node_info, cube_min) == 32 &&
           offsetof(pcv_node_info, cube_edge) == 56 && offsetof(pcv_node_info, xyz_offset) == 64 &&
           offsetof(pcv_node_info, point_offset) == 72,
       "pcv_node_info fields");
PCV_SA(sizeof(pcv_shape) == 264 && offsetof(pcv_shape, kind) == 0 && offsetof(pcv_shape, params) == 8, "pcv_shape");
PCV_SA(sizeof(pcv_top_streams) == 584 && offsetof(pcv_top_streams, l2) == 64 && offsetof(pcv_top_streams, l1_split_mask) == 576,
       "pcv_top_streams");
PCV_SA(sizeof(pcv_top_layout) == 360 && offsetof(pcv_top_layout, l1_stream) == 8 && offsetof(pcv_top_layout, l1_offset) == 72 &&
           offsetof(pcv_top_layout, l2_offset) == 104,
       "pcv_top_layout");
PCV_SA(sizeof(pcv_routed_points) == 48 && offsetof(pcv_routed_points, oct_rgb) == 32 && offsetof(pcv_routed_points, intensity) == 40,
       "pcv_routed_points");
PCV_SA(sizeof(pcv_route_state) == 32, "pcv_route_state");
PCV_SA(sizeof(pcv_plane) == 16 && offsetof(pcv_plane, elem_bytes) == 8, "pcv_plane");
PCV_SA(sizeof(pcv_split_node) == 56 && offsetof(pcv_split_node, first) == 16 && offsetof(pcv_split_node, level) == 32 &&
           offsetof(pcv_split_node, is_leaf) == 48,
       "pcv_split_node");
PCV_SA(sizeof(pcv_promote_node) == 24 && offsetof(pcv_promote_node, child_offset) == 16, "pcv_promote_node");
PCV_SA(sizeof(pcv_sort_records_args) == 160 && offsetof(pcv_sort_records_args, planes) == 24 &&
           offsetof(pcv_sort_records_args, plane0_in) == 88 && offsetof(pcv_sort_records_args, rows) == 112 &&
           offsetof(pcv_sort_records_args, key_bits) == 120 && offsetof(pcv_sort_records_args, flags) == 152,
       "pcv_sort_records_args");
PCV_SA(sizeof(pcv_sort_pass_info) == 40 && offsetof(pcv_sort_pass_info, dyn_lds) == 32, "pcv_sort_pass_info");
PCV_SA(sizeof(pcv_sort_plan_info) == 360 && offsetof(pcv_sort_plan_info, chunk) == 32 && offsetof(pcv_sort_plan_info, pass) == 40,
       "pcv_sort_plan_info");

PCV_SA(sizeof(pcv_ooc_stats) == 120, "pcv_ooc_stats");
PCV_SA(offsetof(pcv_ooc_stats, spill_bytes) == 32 && offsetof(pcv_ooc_stats, h2d_ms) == 56 && offsetof(pcv_ooc_stats, write_ms) == 104 &&
           offsetof(pcv_ooc_stats, split_mask) == 112 && offsetof(pcv_ooc_stats, routed) == 116,
       "pcv_ooc_stats fields");
PCV_SA(sizeof(pcv_render_params) == 32, "pcv_render_params");
PCV_SA(offsetof(pcv_render_params, width) == 0 && offsetof(pcv_render_params, height) == 4 && offsetof(pcv_render_params, point_size) == 8 &&
           offsetof(pcv_render_params, gamma) == 12 && offsetof(pcv_render_params, max_nodes) == 16 &&
           offsetof(pcv_render_params, max_workspace_bytes) == 24,
       "pcv_render_params fields");
PCV_SA(sizeof(pcv_render_overlay) == 8, "pcv_render_overlay");
PCV_SA(offsetof(pcv_render_overlay, flags) == 0 && offsetof(pcv_render_overlay, outline_rgba) == 4, "pcv_render_overlay fields");
PCV_SA(sizeof(pcv_s2_stream_params) == 32, "pcv_s2_stream_params");
PCV_SA(offsetof(pcv_s2_stream_params, struct_size) == 0 && offsetof(pcv_s2_stream_params, split_level) == 4 &&
           offsetof(pcv_s2_stream_params, directory) == 8 && offsetof(pcv_s2_stream_params, open_mode) == 16 &&
           offsetof(pcv_s2_stream_params, flush_points) == 24,
       "pcv_s2_stream_params fields");
PCV_SA(sizeof(pcv_s2_merge_segment) == 24 && offsetof(pcv_s2_merge_segment, src_offset) == 8 && offsetof(pcv_s2_merge_segment, part) == 16 &&
           offsetof(pcv_s2_merge_segment, count) == 20,
       "pcv_s2_merge_segment");
PCV_SA(sizeof(pcv_attribute) == 24 && offsetof(pcv_attribute, name) == 0 && offsetof(pcv_attribute, data_type) == 8 &&
           offsetof(pcv_attribute, reserved) == 12 && offsetof(pcv_attribute, data) == 16,
       "pcv_attribute");
PCV_SA(sizeof(pcv_ply_write_params) == 32, "pcv_ply_write_params");
PCV_SA(offsetof(pcv_ply_write_params, struct_size) == 0 && offsetof(pcv_ply_write_params, open_mode) == 4 &&
           offsetof(pcv_ply_write_params, attributes) == 8 && offsetof(pcv_ply_write_params, num_attributes) == 16 &&
           offsetof(pcv_ply_write_params, chunk_points) == 24,
       "pcv_ply_write_params fields");
PCV_SA(sizeof(pcv_terrain_params) == 120 && offsetof(pcv_terrain_params, tile_size) == 0 && offsetof(pcv_terrain_params, statistic) == 4 &&
           offsetof(pcv_terrain_params, resolution_m) == 8 && offsetof(pcv_terrain_params, origin) == 16 &&
           offsetof(pcv_terrain_params, world_from_terrain) == 40 && offsetof(pcv_terrain_params, min_points) == 96 &&
           offsetof(pcv_terrain_params, max_pool_bytes) == 104 && offsetof(pcv_terrain_params, staging_points) == 112,
       "pcv_terrain_params");
PCV_SA(sizeof(pcv_terrain_info) == 72 && offsetof(pcv_terrain_info, points_added) == 0 && offsetof(pcv_terrain_info, tiles) == 32 &&
           offsetof(pcv_terrain_info, pool_bytes) == 40 && offsetof(pcv_terrain_info, vertex_min) == 48 &&
           offsetof(pcv_terrain_info, vertex_max) == 56 && offsetof(pcv_terrain_info, finished) == 64,
       "pcv_terrain_info");
PCV_SA(sizeof(pcv_maptiles_params) == 32 && offsetof(pcv_maptiles_params, zoom) == 0 && offsetof(pcv_maptiles_params, background) == 4 &&
           offsetof(pcv_maptiles_params, max_tiles) == 8 && offsetof(pcv_maptiles_params, max_pool_bytes) == 16 &&
           offsetof(pcv_maptiles_params, staging_points) == 24,
       "pcv_maptiles_params");
PCV_SA(sizeof(pcv_maptiles_info) == 240 && offsetof(pcv_maptiles_info, points_added) == 0 && offsetof(pcv_maptiles_info, dropped) == 8 &&
           offsetof(pcv_maptiles_info, drawn) == 16 && offsetof(pcv_maptiles_info, pool_bytes) == 24 && offsetof(pcv_maptiles_info, zoom) == 32 &&
           offsetof(pcv_maptiles_info, min_zoom) == 36 && offsetof(pcv_maptiles_info, finished) == 40 && offsetof(pcv_maptiles_info, tiles) == 48,
       "pcv_maptiles_info");
PCV_SA(sizeof(pcv_las_header) == 72 && offsetof(pcv_las_header, point_format) == 2 && offsetof(pcv_las_header, header_size) == 4 &&
           offsetof(pcv_las_header, record_length) == 6 && offsetof(pcv_las_header, offset_to_points) == 8 &&
           offsetof(pcv_las_header, num_points) == 16 && offsetof(pcv_las_header, scale) == 24 && offsetof(pcv_las_header, offset) == 48,
       "pcv_las_header");
PCV_SA(sizeof(pcv_las_params) == 208 && offsetof(pcv_las_params, constant_color) == 4 && offsetof(pcv_las_params, drop_withheld) == 7 &&
           offsetof(pcv_las_params, keep_intensity) == 8 && offsetof(pcv_las_params, piece_points) == 12 &&
           offsetof(pcv_las_params, use_transform) == 16 && offsetof(pcv_las_params, num_extras) == 20 &&
           offsetof(pcv_las_params, class_mask) == 24 && offsetof(pcv_las_params, global_from_local) == 56 &&
           offsetof(pcv_las_params, extras) == 112,
       "pcv_las_params");
PCV_SA(sizeof(pcv_las_info) == 2256 && offsetof(pcv_las_info, num_kept) == 8 && offsetof(pcv_las_info, dropped_class) == 16 &&
           offsetof(pcv_las_info, dropped_withheld) == 24 && offsetof(pcv_las_info, max_color) == 32 &&
           offsetof(pcv_las_info, max_intensity) == 36 && offsetof(pcv_las_info, color_rule) == 40 && offsetof(pcv_las_info, num_pieces) == 44 &&
           offsetof(pcv_las_info, class_hist) == 48 && offsetof(pcv_las_info, return_hist) == 2096 && offsetof(pcv_las_info, flag_counts) == 2224,
       "pcv_las_info");
PCV_SA(sizeof(pcv_las_columns) == 136 && offsetof(pcv_las_columns, color) == 24 && offsetof(pcv_las_columns, intensity) == 32 &&
           offsetof(pcv_las_columns, extras) == 40,
       "pcv_las_columns");
PCV_SA(sizeof(pcv_las_write_params) == 168 && offsetof(pcv_las_write_params, open_mode) == 4 && offsetof(pcv_las_write_params, point_format) == 8 &&
           offsetof(pcv_las_write_params, version_minor) == 12 && offsetof(pcv_las_write_params, scale) == 16 &&
           offsetof(pcv_las_write_params, offset) == 40 && offsetof(pcv_las_write_params, auto_offset) == 64 &&
           offsetof(pcv_las_write_params, color_rule) == 68 && offsetof(pcv_las_write_params, intensity_scale) == 72 &&
           offsetof(pcv_las_write_params, num_fields) == 76 && offsetof(pcv_las_write_params, fields) == 80 &&
           offsetof(pcv_las_write_params, chunk_points) == 88 && offsetof(pcv_las_write_params, file_source_id) == 96 &&
           offsetof(pcv_las_write_params, year) == 102 && offsetof(pcv_las_write_params, system_identifier) == 104 &&
           offsetof(pcv_las_write_params, generating_software) == 136,
       "pcv_las_write_params");
PCV_SA(sizeof(pcv_las_write_info) == 296 && offsetof(pcv_las_write_info, header_size) == 12 && offsetof(pcv_las_write_info, scale) == 16 &&
           offsetof(pcv_las_write_info, offset) == 40 && offsetof(pcv_las_write_info, min_xyz) == 64 && offsetof(pcv_las_write_info, max_xyz) == 76 &&
           offsetof(pcv_las_write_info, bounds) == 88 && offsetof(pcv_las_write_info, num_records) == 136 &&
           offsetof(pcv_las_write_info, by_return) == 144 && offsetof(pcv_las_write_info, out_of_range) == 264 &&
           offsetof(pcv_las_write_info, clamped_intensity) == 272 && offsetof(pcv_las_write_info, masked_values) == 280 &&
           offsetof(pcv_las_write_info, skipped_extras) == 288,
       "pcv_las_write_info");
PCV_SA(sizeof(pcv_render_terrain_layers) == 24 && offsetof(pcv_render_terrain_layers, num_layers) == 0 &&
           offsetof(pcv_render_terrain_layers, window) == 4 && offsetof(pcv_render_terrain_layers, layers) == 8 &&
           offsetof(pcv_render_terrain_layers, camera_positions) == 16,
       "pcv_render_terrain_layers");
PCV_SA(sizeof(pcv_s2_filter) == 32 && offsetof(pcv_s2_filter, location) == 0 && offsetof(pcv_s2_filter, reserved) == 4 &&
           offsetof(pcv_s2_filter, attribute) == 8 && offsetof(pcv_s2_filter, lo) == 16 && offsetof(pcv_s2_filter, hi) == 24,
       "pcv_s2_filter");
PCV_SA(sizeof(pcv_xray_filter) == 24 && offsetof(pcv_xray_filter, attribute) == 0 && offsetof(pcv_xray_filter, lo) == 8 &&
           offsetof(pcv_xray_filter, hi) == 16,
       "pcv_xray_filter");
PCV_SA(sizeof(pcv_tiles3d_params) == 152 && offsetof(pcv_tiles3d_params, error_factor) == 0 && offsetof(pcv_tiles3d_params, transform) == 8 &&
           offsetof(pcv_tiles3d_params, flags) == 136 && offsetof(pcv_tiles3d_params, position_mode) == 140 &&
           offsetof(pcv_tiles3d_params, chunk_bytes) == 144,
       "pcv_tiles3d_params");
PCV_SA(sizeof(pcv_tiles3d_info) == 40 && offsetof(pcv_tiles3d_info, tiles) == 0 && offsetof(pcv_tiles3d_info, content_tiles) == 8 &&
           offsetof(pcv_tiles3d_info, points) == 16 && offsetof(pcv_tiles3d_info, total_file_bytes) == 24 &&
           offsetof(pcv_tiles3d_info, chunk_points) == 32,
       "pcv_tiles3d_info");
PCV_SA(sizeof(pcv_tiles3d_tile) == 64 && offsetof(pcv_tiles3d_tile, node) == 0 && offsetof(pcv_tiles3d_tile, num_points) == 8 &&
           offsetof(pcv_tiles3d_tile, mode) == 16 && offsetof(pcv_tiles3d_tile, file_bytes) == 24 &&
           offsetof(pcv_tiles3d_tile, feature_json_offset) == 32 && offsetof(pcv_tiles3d_tile, feature_binary_offset) == 40 &&
           offsetof(pcv_tiles3d_tile, batch_json_offset) == 48 && offsetof(pcv_tiles3d_tile, batch_binary_offset) == 56,
       "pcv_tiles3d_tile");

#endif
