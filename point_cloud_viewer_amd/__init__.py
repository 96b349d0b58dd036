"""MI355X-native octree build / cull hot path of point_cloud_viewer (hand-written HIP for gfx950 behind a C ABI).

The package is a thin host mirror of the reference's interface for this path; all compute lives in
libpcv_hip.so (point_cloud_viewer_amd/csrc). Importing does not require a GPU; calling does.
"""
from . import _lib
from ._lib import (PCV_E_DEPTH, PCV_E_HIP, PCV_E_INVALID, PCV_E_IO, PCV_E_NOT_FOUND, PCV_E_OOM, PCV_OK,  # noqa: F401
                   PcvError, load_library)
from .octree import (Aabb, Context, OctreeResult, QueryBatch, RenderedViews, S2Cloud, S2QueryBatch, Shapes, XrayTiles, build_octree, build_octree_from_file,  # noqa: F401
                     build_s2_cells, build_xray_quadtree, cloud_kind, s2_cell_ids, s2_cell_token, s2_union_contains,
                     s2_cell_geometry, s2_cell_rect, s2_cells_in_location, s2_corners_rect, s2_rect_intersects_cell, s2_union_intersects, s2_union_intersects_cubes,
                     s2_open_host, s2_union_normalize, S2Stream, s2_merge_plan, s2_filter_keep, s2_check_attributes,
                     level_shortcuts, level_table, node_name, quadtree_node_id, quadtree_node_name, read_ply,
                     DeviceColumn, LasCloud, las_decode_host, las_extras, las_params, read_las, read_las_header,
                     ply_append_check, ply_header, ply_layout,
                     las_append_check, las_encode_host, las_write_check_params, las_write_header, las_write_params,
                     Terrain, build_terrain, read_terrain, terrain_check_params, terrain_frame, terrain_meta_json, terrain_params,
                     terrain_quad_masks, terrain_tile_name, terrain_vertex, terrain_meta_read,
                     MapTiles, build_map_tiles, map_tile_from_quad_index, map_tile_pixels, map_tile_quad_index, map_tiles_check_params,
                     map_tiles_json, map_tiles_params, read_map_tiles,
                     Tiles3D, build_3d_tiles, read_3d_tiles, tiles3d_check_params, tiles3d_params, tiles3d_rtc, tiles3d_tile_host,
                     tiles3d_tileset_json,
                     render_check_overlay, render_check_params, render_gamma_lut, render_overlay, render_params,
                     render_check_terrain, render_terrain_window,
                     polygon_check, polygon_contains, polygon_from_lat_lng, polygon_intersects_cubes,
                     web_mercator_rect_from_zoomed, wmr_contains, wmr_corners, wmr_from_lat_lng, wmr_math, wmr_project, wmr_to_lat_lng,
                     inpaint_xray_quadtree, merge_xray_quadtrees, png_decode, xray_check_params, xray_coloring, xray_finalize, xray_lanczos_taps, xray_leaf_tiles,
                     xray_bins, xray_check_attrs, xray_filters, xray_inpaint_check, xray_inpaint_plan, xray_merge_check, xray_open_host, xray_params, xray_png_encode, xray_png_encode_tiles)

__all__ = ["Aabb", "Context", "OctreeResult", "QueryBatch", "RenderedViews", "XrayTiles", "build_octree", "level_table", "node_name", "PcvError",
           "load_library"]
