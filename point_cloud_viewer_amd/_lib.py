"""ctypes binding of libpcv_hip.so (the C ABI of include/pcv_hip.h).

There is no CPU fallback: if the HIP library is missing or no MI355X is visible, calls fail loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PCV_HIP_LIBRARY: an alternative in-tree build of the same sources — "exp" = libpcv_hip_exp.so, the build with
# -DPCV_EXPERIMENTS whose environment switches are live (A/B scripts under tools/, tests of the alternative kernels), or
# a path (tools/build_variants.sh). The default library reads no environment variable.
_alt = os.environ.get("PCV_HIP_LIBRARY")
LIB_PATH = os.path.join(_HERE, "libpcv_hip_exp.so") if _alt == "exp" else (_alt or os.path.join(_HERE, "libpcv_hip.so"))

PCV_OK = 0
ABI_VERSION = 2  # include/pcv_hip.h PCV_ABI_VERSION
PCV_E_INVALID, PCV_E_HIP, PCV_E_IO, PCV_E_OOM, PCV_E_DEPTH, PCV_E_NOT_FOUND = -1, -2, -3, -4, -5, -6
MEM_HOST, MEM_DEVICE = 0, 1
ENC_UINT8, ENC_UINT16, ENC_FLOAT32, ENC_FLOAT64 = 1, 2, 3, 4
BUILD_COMPUTE_BBOX = 1
BUILD_NO_SPECULATION = 2
BUILD_FORCE_SINGLE_CHAIN = 4
BUILD_NO_SINGLE_CHAIN = 8
BUILD_CHECK_RESOLVE = 16
BUILD_STAGE_TIMES = 32
ROUTE_OCTANTS_ONLY = 64
MAX_KEY_LEVELS = 21
NUM_STAGES = 10
STAGE_NAMES = ["aabb", "chain_keys", "sort_keys", "node_split", "table", "leaf_encode", "sort_records",
               "promote_encode", "sort_second", "total"]

_ERR_NAMES = {PCV_E_INVALID: "PCV_E_INVALID", PCV_E_HIP: "PCV_E_HIP", PCV_E_IO: "PCV_E_IO", PCV_E_OOM: "PCV_E_OOM",
              PCV_E_DEPTH: "PCV_E_DEPTH", PCV_E_NOT_FOUND: "PCV_E_NOT_FOUND"}


class PcvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class Points(C.Structure):
    _fields_ = [("n", C.c_uint64), ("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("color", C.c_void_p),
                ("color_stride", C.c_uint32), ("intensity", C.c_void_p), ("mem", C.c_int32)]


class NodeCopy(C.Structure):
    _fields_ = [("node", C.c_uint64), ("dst_offset", C.c_uint64 * 3)]


class BuildParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("bbox_min", C.c_double * 3), ("bbox_max", C.c_double * 3),
                ("max_points_per_node", C.c_uint32), ("flags", C.c_uint32)]


class Shape(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("params", C.c_double * 32)]


SHAPE_ALL, SHAPE_AABB, SHAPE_FRUSTUM, SHAPE_OBB, SHAPE_FRUSTUM_WITH_INVERSE, SHAPE_WEB_MERCATOR_RECT = 0, 1, 2, 3, 4, 5
SHAPE_S2_CELL_UNION = 6  # PCV_SHAPE_S2_CELL_UNION: Shape.reserved is the union's index (pcv_shapes_create_ex)
SHAPE_POLYGON = 7  # PCV_SHAPE_POLYGON: Shape.reserved is the polygon's index (pcv_shapes_create_ex2); params z_min, z_max, frame
MAX_SHAPE_AXES = 45  # PCV_MAX_SHAPE_AXES
WMR_FN_ATAN2, WMR_FN_SINCOS, WMR_FN_LN = 0, 1, 2


class XrayParams(C.Structure):
    _fields_ = [("tile_size_px", C.c_uint32), ("strategy", C.c_uint32), ("colormap", C.c_uint32), ("background", C.c_uint32),
                ("pixel_size_m", C.c_double), ("max_stddev", C.c_float), ("root_level", C.c_uint32), ("root_index", C.c_uint64),
                ("has_query_from_global", C.c_int32), ("reserved", C.c_int32), ("query_from_global", C.c_double * 7),
                ("interval_attribute", C.c_char_p), ("interval", C.c_double * 2), ("max_workspace_bytes", C.c_uint64)]


class XrayColoring(C.Structure):
    _fields_ = [("min_intensity", C.c_float), ("max_intensity", C.c_float), ("binning_attribute", C.c_char_p),
                ("bin_size", C.c_double)]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("point_size", C.c_float), ("gamma", C.c_float),
                ("max_nodes", C.c_uint32), ("max_workspace_bytes", C.c_uint64)]


class RenderOverlay(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("outline_rgba", C.c_uint8 * 4)]


class RenderTerrainLayers(C.Structure):  # pcv_render_terrain_layers
    _fields_ = [("num_layers", C.c_uint32), ("window", C.c_uint32), ("layers", C.POINTER(C.c_void_p)), ("camera_positions", C.c_void_p)]


RENDER_TERRAIN_WINDOW = 1024  # PCV_RENDER_TERRAIN_WINDOW: the viewer's window edge in vertices
RENDER_MAX_POINT_SIZE = 64  # PCV_RENDER_MAX_POINT_SIZE
RENDER_OUTLINE_NODES = 1  # PCV_RENDER_OUTLINE_NODES
RENDER_OUTLINE_YELLOW = (255, 255, 0, 255)  # PCV_RENDER_OUTLINE_YELLOW: the viewer's YELLOW
XRAY_XRAY, XRAY_COLORED, XRAY_HEIGHT_STDDEV, XRAY_COLORED_WITH_INTENSITY = 0, 1, 2, 3
XRAY_JET, XRAY_PURPLISH = 0, 1
XRAY_BG_WHITE, XRAY_BG_TRANSPARENT = 0, 1
XRAY_PNG_STORED, XRAY_PNG_DEFLATE = 0, 1  # PCV_XRAY_PNG_*: the mode of pcv_xray_write_dir_ex / _node_pngs / _png_encode_ex
XRAY_INPAINT_MAX_TILE = 8192  # PCV_XRAY_INPAINT_MAX_TILE
XRAY_INPAINT_ABSENT = 0xFFFFFFFF  # an empty slot of pcv_xray_inpaint_plan
XRAY_MAX_TREES = 4096  # PCV_XRAY_MAX_TREES: octrees of one pcv_xray_run_many
CLOUD_OCTREE, CLOUD_S2 = 0, 1  # pcv_cloud_kind
XRAY_FN_XRAY, XRAY_FN_COLORED, XRAY_FN_JET, XRAY_FN_PURPLISH, XRAY_FN_TO_U8, XRAY_FN_INTENSITY = 0, 1, 2, 3, 4, 5
REL_IN, REL_CROSS, REL_OUT = 0, 1, 2


class RouteState(C.Structure):
    _fields_ = [("cx", C.c_void_p), ("cy", C.c_void_p), ("cz", C.c_void_p), ("oct_rgb", C.c_void_p)]


class RouteDst(C.Structure):
    _fields_ = [("oct_rgb", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p), ("cz", C.c_void_p), ("intensity", C.c_void_p)]


class Plane(C.Structure):
    _fields_ = [("src", C.c_void_p), ("elem_bytes", C.c_uint32)]


class RoutedPoints(C.Structure):
    _fields_ = [("n", C.c_uint64), ("cx", C.c_void_p), ("cy", C.c_void_p), ("cz", C.c_void_p), ("oct_rgb", C.c_void_p),
                ("intensity", C.c_void_p)]


class TopStreams(C.Structure):
    _fields_ = [("l1", C.c_uint64 * 8), ("l2", C.c_uint64 * 64), ("l1_split_mask", C.c_uint32), ("reserved", C.c_uint32)]


class TopLayout(C.Structure):
    _fields_ = [("root_points", C.c_uint64), ("l1_stream", C.c_uint64 * 8), ("l1_offset", C.c_uint32 * 8),
                ("l2_offset", C.c_uint32 * 64)]


class SplitNode(C.Structure):
    _fields_ = [("id_high", C.c_uint64), ("id_low", C.c_uint64), ("first", C.c_uint64), ("count", C.c_uint64),
                ("level", C.c_uint32), ("parent", C.c_uint32), ("first_child", C.c_uint32), ("child_mask", C.c_uint32),
                ("is_leaf", C.c_uint32), ("reserved", C.c_uint32)]


class PromoteNode(C.Structure):
    _fields_ = [("stream_len", C.c_uint64), ("num_points", C.c_uint64), ("child_offset", C.c_uint64)]


class NodeInfo(C.Structure):
    _fields_ = [("id_high", C.c_uint64), ("id_low", C.c_uint64), ("num_points", C.c_int64), ("level", C.c_uint32),
                ("encoding", C.c_uint32), ("cube_min", C.c_double * 3), ("cube_edge", C.c_double),
                ("xyz_offset", C.c_uint64), ("point_offset", C.c_uint64)]


SORT_ROWS_NONE, SORT_ROWS_GIVEN, SORT_ROWS_DEVICE = 0, 1, 2  # PCV_SORT_ROWS_*
SORT_RECORDS_CHECK_KEYS = 1  # PCV_SORT_RECORDS_CHECK_KEYS
SORT_RECORDS_PACKED = 2  # PCV_SORT_RECORDS_PACKED


class SortRecordsArgs(C.Structure):
    _fields_ = [("n", C.c_uint64), ("keys", C.c_void_p), ("vec", C.c_void_p), ("planes", C.c_void_p * 8), ("plane0_in", C.c_void_p),
                ("color_in", C.c_void_p), ("map", C.c_void_p), ("rows", C.c_void_p), ("key_bits", C.c_int32), ("vec_bytes", C.c_int32),
                ("nwords", C.c_int32), ("color_stride", C.c_uint32), ("map_entries", C.c_uint32), ("rows_mode", C.c_int32),
                ("hold_second", C.c_int32), ("mem", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class SortPassInfo(C.Structure):
    _fields_ = [("shift", C.c_int32), ("nbits", C.c_int32), ("hist", C.c_int32), ("down", C.c_int32), ("R", C.c_int32),
                ("MAP", C.c_int32), ("PL", C.c_int32), ("map_lds", C.c_int32), ("dyn_lds", C.c_uint64)]


class SortPlanInfo(C.Structure):
    _fields_ = [("npasses", C.c_int32), ("two_pass", C.c_int32), ("held_back", C.c_int32), ("pieces", C.c_int32),
                ("blocks", C.c_int32), ("gpb", C.c_int32), ("groups", C.c_int32), ("second_ran", C.c_int32), ("chunk", C.c_uint64),
                ("passes", SortPassInfo * 8)]


class S2StreamParams(C.Structure):  # pcv_s2_stream_params
    _fields_ = [("struct_size", C.c_uint32), ("split_level", C.c_uint32), ("directory", C.c_char_p), ("open_mode", C.c_int32),
                ("reserved", C.c_uint32), ("flush_points", C.c_uint64)]


class S2MergeSegment(C.Structure):  # pcv_s2_merge_segment
    _fields_ = [("dst_offset", C.c_uint64), ("src_offset", C.c_uint64), ("part", C.c_uint32), ("count", C.c_uint32)]


S2_TRUNCATE, S2_APPEND = 0, 1  # pcv_s2_stream_params.open_mode


class Attribute(C.Structure):  # pcv_attribute
    _fields_ = [("name", C.c_char_p), ("data_type", C.c_int32), ("reserved", C.c_uint32), ("data", C.c_void_p)]


class XrayFilter(C.Structure):  # pcv_xray_filter
    _fields_ = [("attribute", C.c_char_p), ("lo", C.c_double), ("hi", C.c_double)]


class S2Filter(C.Structure):  # pcv_s2_filter
    _fields_ = [("location", C.c_uint32), ("reserved", C.c_uint32), ("attribute", C.c_char_p), ("lo", C.c_double), ("hi", C.c_double)]


# PCV_ATTR_*: type string -> (proto enum value, numpy dtype, components)
ATTR_TYPES = {"u8": (1, "u1", 1), "u16": (2, "<u2", 1), "u32": (3, "<u4", 1), "u64": (4, "<u8", 1), "i8": (6, "i1", 1), "i16": (7, "<i2", 1),
              "i32": (8, "<i4", 1), "i64": (9, "<i8", 1), "f32": (11, "<f4", 1), "f64": (12, "<f8", 1), "u8vec3": (27, "u1", 3),
              "f64vec3": (38, "<f8", 3)}
ATTR_NAMES = {v[0]: k for k, v in ATTR_TYPES.items()}
S2_MAX_EXTRAS = 16
PLY_TRUNCATE, PLY_APPEND = 0, 1  # pcv_ply_write_params.open_mode
PLY_READ_EXTRAS = 1  # PCV_PLY_READ_EXTRAS


class PlyWriteParams(C.Structure):  # pcv_ply_write_params
    _fields_ = [("struct_size", C.c_uint32), ("open_mode", C.c_int32), ("attributes", C.POINTER(C.c_char_p)), ("num_attributes", C.c_uint32),
                ("reserved", C.c_uint32), ("chunk_points", C.c_uint64)]


TERRAIN_STATISTICS = {"max": 0, "min": 1, "mean": 2}  # PCV_TERRAIN_MAX / _MIN / _MEAN


class TerrainParams(C.Structure):  # pcv_terrain_params
    _fields_ = [("tile_size", C.c_uint32), ("statistic", C.c_uint32), ("resolution_m", C.c_double), ("origin", C.c_double * 3),
                ("world_from_terrain", C.c_double * 7), ("min_points", C.c_uint32), ("reserved", C.c_uint32), ("max_pool_bytes", C.c_uint64),
                ("staging_points", C.c_uint64)]


class TerrainInfo(C.Structure):  # pcv_terrain_info
    _fields_ = [("points_added", C.c_uint64), ("outside", C.c_uint64), ("set_vertices", C.c_uint64), ("rendered_quads", C.c_uint64),
                ("tiles", C.c_uint64), ("pool_bytes", C.c_uint64), ("vertex_min", C.c_int32 * 2), ("vertex_max", C.c_int32 * 2),
                ("finished", C.c_uint32), ("reserved", C.c_uint32)]


class MapTilesParams(C.Structure):  # pcv_maptiles_params
    _fields_ = [("zoom", C.c_uint32), ("background", C.c_uint32), ("max_tiles", C.c_uint64), ("max_pool_bytes", C.c_uint64),
                ("staging_points", C.c_uint64)]


class MapTilesInfo(C.Structure):  # pcv_maptiles_info
    _fields_ = [("points_added", C.c_uint64), ("dropped", C.c_uint64), ("drawn", C.c_uint64), ("pool_bytes", C.c_uint64),
                ("zoom", C.c_uint32), ("min_zoom", C.c_uint32), ("finished", C.c_uint32), ("reserved", C.c_uint32), ("tiles", C.c_uint64 * 24)]


LAS_COLOR_AUTO, LAS_COLOR_RGB16, LAS_COLOR_RGB8, LAS_COLOR_INTENSITY, LAS_COLOR_CONSTANT = range(5)
LAS_COLOR_NAMES = ["auto", "rgb16", "rgb8", "intensity", "constant"]
LAS_MAX_EXTRAS = 12
LAS_RAW_PIECES = 2  # PCV_LAS_RAW_PIECES: the raw pieces a load holds on the device


class LasHeader(C.Structure):  # pcv_las_header
    _fields_ = [("version_major", C.c_uint8), ("version_minor", C.c_uint8), ("point_format", C.c_uint8), ("reserved0", C.c_uint8),
                ("header_size", C.c_uint16), ("record_length", C.c_uint16), ("offset_to_points", C.c_uint32), ("reserved1", C.c_uint32),
                ("num_points", C.c_uint64), ("scale", C.c_double * 3), ("offset", C.c_double * 3)]


class LasParams(C.Structure):  # pcv_las_params
    _fields_ = [("color_mode", C.c_uint32), ("constant_color", C.c_uint8 * 3), ("drop_withheld", C.c_uint8), ("keep_intensity", C.c_uint32),
                ("piece_points", C.c_uint32), ("use_transform", C.c_uint32), ("num_extras", C.c_uint32), ("class_mask", C.c_uint64 * 4),
                ("global_from_local", C.c_double * 7), ("extras", C.c_char_p * LAS_MAX_EXTRAS)]


class LasInfo(C.Structure):  # pcv_las_info
    _fields_ = [("num_records", C.c_uint64), ("num_kept", C.c_uint64), ("dropped_class", C.c_uint64), ("dropped_withheld", C.c_uint64),
                ("max_color", C.c_uint32), ("max_intensity", C.c_uint32), ("color_rule", C.c_uint32), ("num_pieces", C.c_uint32),
                ("class_hist", C.c_uint64 * 256), ("return_hist", C.c_uint64 * 16), ("flag_counts", C.c_uint64 * 4)]


class LasColumns(C.Structure):  # pcv_las_columns
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("color", C.c_void_p), ("intensity", C.c_void_p),
                ("extras", C.c_void_p * LAS_MAX_EXTRAS)]


LAS_FORMAT_AUTO = 255  # PCV_LAS_FORMAT_AUTO
LAS_WRITE_COLOR_NAMES = ["x257", "shift8", "rgb8"]  # PCV_LAS_WRITE_COLOR_*
LAS_TRUNCATE, LAS_APPEND = 0, 1


class LasWriteParams(C.Structure):  # pcv_las_write_params
    _fields_ = [("struct_size", C.c_uint32), ("open_mode", C.c_int32), ("point_format", C.c_uint32), ("version_minor", C.c_uint32),
                ("scale", C.c_double * 3), ("offset", C.c_double * 3), ("auto_offset", C.c_uint32), ("color_rule", C.c_uint32),
                ("intensity_scale", C.c_float), ("num_fields", C.c_uint32), ("fields", C.POINTER(C.c_char_p)), ("chunk_points", C.c_uint64),
                ("file_source_id", C.c_uint16), ("global_encoding", C.c_uint16), ("day", C.c_uint16), ("year", C.c_uint16),
                ("system_identifier", C.c_char * 32), ("generating_software", C.c_char * 32)]


class LasWriteInfo(C.Structure):  # pcv_las_write_info
    _fields_ = [("point_format", C.c_uint32), ("version_minor", C.c_uint32), ("record_length", C.c_uint32), ("header_size", C.c_uint32),
                ("scale", C.c_double * 3), ("offset", C.c_double * 3), ("min_xyz", C.c_int32 * 3), ("max_xyz", C.c_int32 * 3),
                ("bounds", C.c_double * 6), ("num_records", C.c_uint64), ("by_return", C.c_uint64 * 15), ("out_of_range", C.c_uint64),
                ("clamped_intensity", C.c_uint64), ("masked_values", C.c_uint64), ("skipped_extras", C.c_uint32), ("reserved", C.c_uint32)]


TILES3D_INTENSITY = 1
TILES3D_POS_AUTO, TILES3D_POS_QUANTIZED, TILES3D_POS_FLOAT = range(3)
TILES3D_POS_NAMES = ["auto", "quantized", "float"]
TILES3D_DEFAULT_ERROR_FACTOR = 0.0625
TILES3D_MIN_CHUNK_BYTES = 4 << 20


class Tiles3dParams(C.Structure):  # pcv_tiles3d_params
    _fields_ = [("error_factor", C.c_double), ("transform", C.c_double * 16), ("flags", C.c_uint32), ("position_mode", C.c_uint32),
                ("chunk_bytes", C.c_uint64)]


class Tiles3dInfo(C.Structure):  # pcv_tiles3d_info
    _fields_ = [("tiles", C.c_uint64), ("content_tiles", C.c_uint64), ("points", C.c_uint64), ("total_file_bytes", C.c_uint64),
                ("chunk_points", C.c_uint32), ("reserved", C.c_uint32)]


class Tiles3dTile(C.Structure):  # pcv_tiles3d_tile
    _fields_ = [("node", C.c_uint64), ("num_points", C.c_uint64), ("mode", C.c_uint32), ("reserved", C.c_uint32), ("file_bytes", C.c_uint64),
                ("feature_json_offset", C.c_uint64), ("feature_binary_offset", C.c_uint64), ("batch_json_offset", C.c_uint64),
                ("batch_binary_offset", C.c_uint64)]


class OocStats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("nodes", C.c_uint64), ("partitions", C.c_uint64), ("largest_bucket", C.c_uint64),
                ("spill_bytes", C.c_uint64), ("h2d_bytes", C.c_uint64), ("d2h_bytes", C.c_uint64), ("h2d_ms", C.c_double),
                ("d2h_ms", C.c_double), ("stream_ms", C.c_double), ("topology_ms", C.c_double), ("build_ms", C.c_double),
                ("merge_ms", C.c_double), ("write_ms", C.c_double), ("split_mask", C.c_uint32), ("routed", C.c_uint32)]


# every symbol include/pcv_hip.h declares: name -> (restype, argtypes)
_vp = C.c_void_p
_SIGNATURES = {
    "pcv_abi_version": (C.c_int, []),
    "pcv_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "pcv_ctx_destroy": (None, [_vp]),
    "pcv_last_error": (C.c_char_p, [_vp]),
    "pcv_ctx_trim": (C.c_int, [_vp]),
    "pcv_ctx_synchronize": (C.c_int, [_vp]),
    "pcv_ctx_wait_stream": (C.c_int, [_vp, _vp]),
    "pcv_ctx_signal_stream": (C.c_int, [_vp, _vp]),
    "pcv_ctx_set_profiling": (C.c_int, [_vp, C.c_int]),
    "pcv_ctx_reset_kernel_stats": (C.c_int, [_vp]),
    "pcv_ctx_kernel_stats": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_double)]),
    "pcv_build_octree": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(Points), C.POINTER(_vp)]),
    "pcv_ingest_begin": (C.c_int, [_vp, C.c_uint64, C.c_int, C.POINTER(_vp)]),
    "pcv_ingest_append": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64]),
    "pcv_ingest_num_points": (C.c_uint64, [_vp]),
    "pcv_ingest_bbox": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pcv_ingest_finish": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(_vp)]),
    "pcv_ingest_abort": (None, [_vp]),
    "pcv_ooc_begin": (C.c_int, [_vp, C.POINTER(BuildParams), C.c_int, C.c_uint64, C.POINTER(_vp)]),
    "pcv_ooc_append": (C.c_int, [_vp, _vp, _vp, _vp, C.c_uint64]),
    "pcv_ooc_finish": (C.c_int, [_vp, C.c_char_p, C.POINTER(OocStats)]),
    "pcv_ooc_abort": (None, [_vp]),
    "pcv_ooc_plan": (C.c_int, [C.POINTER(C.c_uint64), C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_uint32),
                               C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_char_p, C.c_uint64]),
    "pcv_ooc_top_layout": (C.c_int, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(TopLayout)]),
    "pcv_ooc_bucket_runs": (C.c_int, [_vp, C.POINTER(BuildParams), _vp, _vp, _vp, C.c_uint64, C.c_int, C.POINTER(_vp), _vp,
                                      C.POINTER(C.c_uint64)]),
    "pcv_octree_num_nodes": (C.c_uint64, [_vp]),
    "pcv_octree_num_points": (C.c_uint64, [_vp]),
    "pcv_octree_has_intensity": (C.c_int, [_vp]),
    "pcv_octree_node": (C.c_int, [_vp, C.c_uint64, C.POINTER(NodeInfo)]),
    "pcv_octree_meta": (None, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_int)]),
    "pcv_octree_node_data": (C.c_int, [_vp, C.c_uint64, C.c_int, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "pcv_octree_device_blob": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_uint64)]),
    "pcv_octree_write_dir": (C.c_int, [_vp, C.c_char_p]),
    "pcv_octree_free": (None, [_vp]),
    "pcv_octree_stage_ms": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int]),
    "pcv_octree_build_info": (None, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pcv_octree_spec_stats": (None, [_vp, C.POINTER(C.c_uint64)]),
    "pcv_octree_record_bytes": (C.c_int, [_vp]),
    "pcv_octree_packed_handover": (C.c_int, [_vp]),
    "pcv_octree_spec_continued": (C.c_uint64, [_vp]),
    "pcv_octree_wide_pool_entries": (C.c_uint64, [_vp]),
    "pcv_octree_settled_in_sort": (C.c_uint64, [_vp]),
    "pcv_aabb_reduce": (C.c_int, [_vp, C.POINTER(Points), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pcv_level_table": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int,
                                  C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "pcv_level_shortcuts": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_double)]),
    "pcv_chain_keys": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(Points), C.c_int, _vp]),
    "pcv_route_buckets": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(Points), _vp, C.POINTER(C.c_uint64),
                                    C.POINTER(RouteState)]),
    "pcv_route_tiles": (C.c_uint64, [C.c_uint64]),
    "pcv_route_plan": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(Points), _vp, _vp, C.POINTER(C.c_uint64)]),
    "pcv_route_scatter": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(Points), _vp, _vp, C.c_uint32, _vp, C.POINTER(RouteDst)]),
    "pcv_partition_by_owner": (C.c_int, [_vp, C.c_uint64, _vp, C.c_uint32, _vp, C.c_uint32, C.POINTER(Plane),
                                         C.POINTER(C.c_void_p)]),
    "pcv_build_begin_routed": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(RoutedPoints), C.POINTER(_vp)]),
    "pcv_octree_write_nodes": (C.c_int, [_vp, C.c_char_p, C.c_uint32]),
    "pcv_write_meta": (C.c_int, [C.c_char_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(NodeInfo),
                                 C.c_uint64]),
    "pcv_octree_copy_node": (C.c_int, [_vp, C.c_uint64, C.c_int, _vp, C.c_uint64, C.c_int]),
    "pcv_octree_copy_nodes": (C.c_int, [_vp, C.POINTER(NodeCopy), C.c_uint64, _vp, C.c_uint64, C.c_int]),
    "pcv_build_begin": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(Points), C.POINTER(_vp)]),
    "pcv_build_top_streams": (C.c_int, [_vp, C.POINTER(TopStreams)]),
    "pcv_build_finish": (C.c_int, [_vp, C.POINTER(TopLayout)]),
    "pcv_node_split": (C.c_int, [_vp, C.POINTER(BuildParams), _vp, C.c_uint64, C.c_int, C.POINTER(SplitNode), C.c_uint64,
                                 C.POINTER(C.c_uint64)]),
    "pcv_promote_assign": (C.c_int, [C.POINTER(SplitNode), C.c_uint64, C.POINTER(PromoteNode), C.c_uint64, _vp, _vp]),
    "pcv_gather_encode": (C.c_int, [_vp, C.POINTER(BuildParams), C.POINTER(Points), C.POINTER(SplitNode), C.c_uint64,
                                    C.POINTER(_vp)]),
    "pcv_sort_keys64": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int]),
    "pcv_sort_keys32": (C.c_int, [_vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int]),
    "pcv_sort_pairs32": (C.c_int, [_vp, _vp, _vp, C.c_uint64, C.c_int, C.c_int, C.c_int]),
    "pcv_sort_records": (C.c_int, [_vp, C.POINTER(SortRecordsArgs), C.POINTER(SortPlanInfo)]),
    "pcv_sort_records_geometry": (None, [C.c_uint64, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]),
    "pcv_selftest_division": (C.c_int, [_vp, C.POINTER(C.c_double), C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_ply_read": (C.c_int, [C.c_char_p, C.POINTER(_vp), C.c_char_p, C.c_uint64]),
    "pcv_ply_num_points": (C.c_uint64, [_vp]),
    "pcv_ply_points": (C.c_int, [_vp, C.POINTER(Points)]),
    "pcv_ply_free": (None, [_vp]),
    "pcv_build_octree_from_ply": (C.c_int, [_vp, C.POINTER(BuildParams), C.c_char_p, C.c_int, C.POINTER(_vp)]),
    "pcv_octree_open_dir": (C.c_int, [_vp, C.c_char_p, C.POINTER(_vp)]),
    "pcv_shapes_create": (C.c_int, [_vp, C.POINTER(Shape), C.c_uint32, C.POINTER(_vp)]),
    "pcv_shapes_create_ex": (C.c_int, [_vp, C.POINTER(Shape), C.c_uint32, C.c_uint32, _vp, _vp, C.POINTER(_vp)]),
    "pcv_shapes_union": (C.c_int, [_vp, C.c_uint32, C.c_uint64, _vp, C.POINTER(C.c_uint32)]),
    "pcv_shapes_create_ex2": (C.c_int, [_vp, C.POINTER(Shape), C.c_uint32, C.c_uint32, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "pcv_shapes_polygon": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, C.POINTER(C.c_uint32), C.c_uint32, _vp, C.POINTER(C.c_uint32)]),
    "pcv_polygon_check_host": (C.c_int, [C.c_uint32, _vp, _vp, C.c_int32, C.c_double, C.c_double]),
    "pcv_polygon_contains_host": (C.c_int, [C.c_uint32, _vp, _vp, C.c_int32, C.c_double, C.c_double, C.c_uint64, _vp, _vp, _vp, _vp]),
    "pcv_polygon_intersects_cubes_host": (C.c_int, [C.c_uint32, _vp, _vp, C.c_double, C.c_double, C.c_uint64, _vp, _vp]),
    "pcv_shapes_free": (None, [_vp]),
    "pcv_shapes_count": (C.c_uint32, [_vp]),
    "pcv_shapes_get": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "pcv_shapes_get_ex": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32,
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "pcv_wmr_from_zoomed": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_double)]),
    "pcv_wmr_corners": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pcv_wmr_project": (C.c_int, [C.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "pcv_wmr_contains": (C.c_int, [C.POINTER(C.c_double), C.c_uint64, _vp, _vp, _vp, _vp]),
    "pcv_wmr_from_lat_lng": (C.c_int, [C.c_uint64, _vp, _vp, _vp, _vp]),
    "pcv_wmr_to_lat_lng": (C.c_int, [C.c_uint64, _vp, _vp, _vp, _vp]),
    "pcv_wmr_math": (C.c_int, [C.c_int, C.c_uint64, _vp, _vp, _vp, _vp]),
    "pcv_cull_nodes": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "pcv_cull_nodes_sparse": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    "pcv_visible_nodes": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "pcv_nodes_in_location": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    "pcv_cull_points": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(Points), C.POINTER(C.c_double), _vp,
                                  C.POINTER(C.c_uint64)]),
    "pcv_cull_node_points": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_double), _vp,
                                       C.POINTER(C.c_uint64)]),
    "pcv_query_points": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.POINTER(C.c_double), C.c_uint64, C.c_int, _vp, _vp, _vp, _vp,
                                   _vp, C.POINTER(C.c_uint64)]),
    "pcv_query_node_points": (C.c_int, [_vp, _vp, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_double), C.c_uint64, C.c_int, _vp, _vp,
                                        _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "pcv_query_batch_run": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(_vp)]),
    "pcv_query_batch_sizes": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcv_query_batch_segments": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pcv_query_batch_points": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "pcv_query_batch_free": (None, [_vp]),
    "pcv_xray_leaf_tiles": (C.c_int, [C.c_uint32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint64), _vp, _vp, _vp, C.c_char_p, C.c_uint64]),
    "pcv_xray_run": (C.c_int, [_vp, _vp, C.POINTER(XrayParams), C.POINTER(_vp)]),
    "pcv_xray_run_many": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(XrayParams), C.POINTER(_vp)]),
    "pcv_xray_check_params": (C.c_int, [C.POINTER(XrayParams), C.c_int, C.c_char_p, C.c_uint64]),
    "pcv_xray_run_ex": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(XrayParams), C.POINTER(XrayColoring), C.POINTER(_vp)]),
    "pcv_xray_check_params_ex": (C.c_int, [C.POINTER(XrayParams), C.POINTER(XrayColoring), C.c_int, C.c_char_p, C.c_uint64]),
    "pcv_xray_negative": (C.c_int, [_vp, _vp]),
    "pcv_xray_plan_groups": (C.c_int, [_vp, C.c_uint64, C.POINTER(XrayParams), C.POINTER(XrayColoring), C.c_uint64,
                                       C.POINTER(C.c_uint64), _vp, C.c_char_p, C.c_uint64]),
    "pcv_xray_info": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcv_xray_tiles": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "pcv_xray_images": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_xray_free": (None, [_vp]),
    "pcv_xray_finalize": (C.c_int, [C.c_int, C.c_uint64, _vp, _vp]),
    "pcv_xray_build_parents": (C.c_int, [_vp]),
    "pcv_xray_nodes": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_uint64, _vp, _vp]),
    "pcv_xray_node_images": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_xray_write_dir": (C.c_int, [_vp, C.c_char_p]),
    "pcv_xray_lanczos_taps": (C.c_int, [C.c_uint32, _vp, _vp, _vp]),
    "pcv_xray_png_encode": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_xray_png_encode_ex": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_xray_png_bound": (C.c_uint64, [C.c_uint32, C.c_uint32, C.c_int]),
    "pcv_xray_node_pngs": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _vp, _vp]),
    "pcv_xray_write_dir_ex": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "pcv_xray_png_encode_tiles": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _vp, _vp]),
    "pcv_ctx_set_xray_chunk_bytes": (C.c_int, [_vp, C.c_uint64]),
    "pcv_png_decode": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _vp, C.c_uint64]),
    "pcv_host_last_error": (C.c_char_p, []),
    "pcv_xray_open_dir": (C.c_int, [_vp, C.c_char_p, C.c_uint32, C.POINTER(_vp), C.POINTER(C.c_uint32)]),
    "pcv_xray_tile_size": (C.c_uint32, [_vp]),
    "pcv_xray_merge_check": (C.c_int, [C.POINTER(_vp), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_char_p, C.c_uint64]),
    "pcv_xray_merge": (C.c_int, [_vp, C.POINTER(_vp), C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "pcv_xray_inpaint_check": (C.c_int, [_vp, C.POINTER(_vp), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64]),
    "pcv_xray_inpaint_plan": (C.c_int, [_vp, C.POINTER(_vp), C.c_uint32, C.c_uint64, _vp, C.POINTER(C.c_uint64), C.c_char_p, C.c_uint64]),
    "pcv_xray_inpaint": (C.c_int, [_vp, _vp, C.POINTER(_vp), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "pcv_xray_inpaint_info": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pcv_render_check_params": (C.c_int, [C.POINTER(RenderParams)]),
    "pcv_render_gamma_lut": (C.c_int, [C.c_float, _vp]),
    "pcv_render_views": (C.c_int, [_vp, _vp, _vp, C.POINTER(RenderParams), C.POINTER(_vp)]),
    "pcv_render_info": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcv_render_images": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_int]),
    "pcv_render_depth": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, C.c_int]),
    "pcv_render_free": (None, [_vp]),
    "pcv_render_check_overlay": (C.c_int, [C.POINTER(RenderOverlay), C.c_char_p, C.c_uint64]),
    "pcv_render_views_ex": (C.c_int, [_vp, _vp, _vp, C.POINTER(RenderParams), C.POINTER(RenderOverlay), C.POINTER(_vp)]),
    "pcv_render_outline_info": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcv_octree_nodes_blob": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_transform_points": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(Points), _vp, _vp, _vp]),
    "pcv_s2_cell_ids": (C.c_int, [_vp, C.POINTER(Points), C.c_uint32, _vp, C.c_int]),
    "pcv_s2_cell_ids_host": (C.c_int, [C.c_uint64, _vp, _vp, _vp, C.c_uint32, _vp]),
    "pcv_s2_cell_token": (C.c_int, [C.c_uint64, C.c_char_p]),
    "pcv_s2_union_contains": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(Points), _vp, C.c_int]),
    "pcv_s2_union_contains_host": (C.c_int, [_vp, C.c_uint32, C.c_uint64, _vp, _vp, _vp, _vp]),
    "pcv_s2_split": (C.c_int, [_vp, C.POINTER(Points), C.c_uint32, C.POINTER(_vp)]),
    "pcv_s2_info": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "pcv_s2_cells": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pcv_s2_order": (C.c_int, [_vp, _vp, C.c_int]),
    "pcv_s2_cell_points": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp, _vp, _vp]),
    "pcv_s2_write_dir": (C.c_int, [_vp, C.c_char_p]),
    "pcv_s2_query_run": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, C.POINTER(_vp)]),
    "pcv_s2_query_sizes": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcv_s2_query_segments": (C.c_int, [_vp, _vp, _vp, _vp]),
    "pcv_s2_query_points": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "pcv_s2_query_free": (None, [_vp]),
    "pcv_s2_open_dir": (C.c_int, [_vp, C.c_char_p, C.POINTER(_vp)]),
    "pcv_s2_split_ex": (C.c_int, [_vp, C.POINTER(Points), _vp, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "pcv_s2_stream_append_ex": (C.c_int, [_vp, C.POINTER(Points), _vp, C.c_uint32]),
    "pcv_s2_attributes_check_host": (C.c_int, [_vp, C.c_uint32]),
    "pcv_s2_attributes": (C.c_int, [_vp, C.POINTER(C.c_uint32), _vp, _vp]),
    "pcv_s2_cell_attribute": (C.c_int, [_vp, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_s2_query_run_ex": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.POINTER(_vp)]),
    "pcv_s2_query_attribute": (C.c_int, [_vp, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_s2_filter_keep_host": (C.c_int, [C.c_int32, C.c_uint64, _vp, C.c_double, C.c_double, _vp]),
    "pcv_s2_free": (None, [_vp]),
    "pcv_s2_stream_begin": (C.c_int, [_vp, C.POINTER(S2StreamParams), C.POINTER(_vp)]),
    "pcv_s2_stream_append": (C.c_int, [_vp, C.POINTER(Points)]),
    "pcv_s2_stream_info": (C.c_int, [_vp] + [C.POINTER(C.c_uint64)] * 5),
    "pcv_s2_stream_finish": (C.c_int, [_vp, C.POINTER(_vp)]),
    "pcv_s2_stream_abort": (None, [_vp]),
    "pcv_s2_stream_set_memory_cap": (C.c_int, [_vp, C.c_uint64]),
    "pcv_s2_merge_plan_host": (C.c_int, [C.c_uint32, _vp, _vp, _vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64), _vp, _vp, _vp, _vp, _vp]),
    "pcv_s2_cell_geometry_host": (C.c_int, [C.c_uint64, _vp]),
    "pcv_s2_cell_rect_host": (C.c_int, [C.c_uint64, _vp]),
    "pcv_s2_corners_rect_host": (C.c_int, [_vp, _vp]),
    "pcv_s2_rect_intersects_cell_host": (C.c_int, [_vp, C.c_uint64, C.POINTER(C.c_int)]),
    "pcv_s2_union_normalize_host": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "pcv_s2_union_intersects_host": (C.c_int, [_vp, C.c_uint32, C.c_uint64, _vp, _vp]),
    "pcv_s2_union_intersects_cubes_host": (C.c_int, [_vp, C.c_uint32, C.c_uint64, _vp, _vp]),
    "pcv_s2_cells_in_location": (C.c_int, [_vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, _vp, _vp]),
    "pcv_s2_cells_in_location_host": (C.c_int, [C.c_uint64, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, _vp, _vp]),
    "pcv_xray_run_s2": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(XrayParams), C.POINTER(XrayColoring), C.POINTER(_vp)]),
    "pcv_xray_run_s2_ex": (C.c_int, [_vp, _vp, C.c_uint32, C.POINTER(XrayParams), C.POINTER(XrayColoring), C.POINTER(XrayFilter), C.c_uint32,
                                     C.POINTER(_vp)]),
    "pcv_xray_check_attrs_host": (C.c_int, [C.POINTER(XrayParams), C.POINTER(XrayColoring), C.POINTER(XrayFilter), C.c_uint32, C.c_uint32,
                                            _vp, C.POINTER(C.c_char_p), _vp, _vp, C.c_char_p, C.c_uint64]),
    "pcv_xray_bins_host": (C.c_int, [C.c_int32, C.c_uint64, _vp, C.c_double, _vp]),
    "pcv_cloud_kind": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "pcv_ply_read_ex": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(_vp), C.c_char_p, C.c_uint64]),
    "pcv_ply_attributes": (C.c_int, [_vp, C.POINTER(C.c_uint32), _vp]),
    "pcv_query_batch_ply_rows": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64, C.c_int, _vp,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "pcv_s2_query_ply_rows": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint64, C.c_int, _vp,
                                        C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "pcv_query_batch_write_ply": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(PlyWriteParams), C.POINTER(C.c_uint64)]),
    "pcv_s2_query_write_ply": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(PlyWriteParams), C.POINTER(C.c_uint64)]),
    "pcv_ply_layout_host": (C.c_int, [C.POINTER(C.c_char_p), _vp, C.c_uint32, _vp, C.POINTER(C.c_uint32)]),
    "pcv_ply_header_host": (C.c_int, [C.POINTER(C.c_char_p), _vp, C.c_uint32, C.c_uint64, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_ply_append_check_host": (C.c_int, [C.c_char_p, C.POINTER(C.c_char_p), _vp, C.c_uint32, C.POINTER(C.c_uint64)]),
    "pcv_ctx_pool_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]),
    "pcv_ctx_set_pool_guard": (C.c_int, [_vp, C.c_int, C.c_int]),
    "pcv_ctx_pool_guard_check": (C.c_int, [_vp]),
    "pcv_ctx_pool_guard_report": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_int64)]),
    "pcv_ctx_pool_guard_selftest": (C.c_int, [_vp, C.c_uint64, C.c_int64]),
    "pcv_render_check_terrain_host": (C.c_int, [C.POINTER(RenderTerrainLayers), C.c_char_p, C.c_uint64]),
    "pcv_render_terrain_window_host": (C.c_int, [C.POINTER(TerrainParams), _vp, C.c_uint32, _vp]),
    "pcv_render_views_terrain": (C.c_int, [_vp, _vp, _vp, C.POINTER(RenderParams), C.POINTER(RenderOverlay), C.POINTER(RenderTerrainLayers),
                                           C.POINTER(_vp)]),
    "pcv_render_terrain_info": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pcv_terrain_meta_read_host": (C.c_int, [C.c_char_p, C.c_uint64, C.POINTER(TerrainParams), C.c_uint64, _vp, C.POINTER(C.c_uint64)]),
    "pcv_terrain_from_tiles": (C.c_int, [_vp, C.POINTER(TerrainParams), C.c_uint64, _vp, _vp, _vp, C.c_int, C.POINTER(_vp)]),
    "pcv_terrain_open_dir": (C.c_int, [_vp, C.c_char_p, C.POINTER(_vp)]),
    "pcv_terrain_begin": (C.c_int, [_vp, C.POINTER(TerrainParams), _vp, _vp, C.POINTER(_vp)]),
    "pcv_terrain_add_points": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, C.c_int]),
    "pcv_terrain_add_query_batch": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64]),
    "pcv_terrain_add_s2_query": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64]),
    "pcv_terrain_finish": (C.c_int, [_vp]),
    "pcv_terrain_info_get": (C.c_int, [_vp, C.POINTER(TerrainInfo)]),
    "pcv_terrain_tiles": (C.c_int, [_vp, C.c_uint64, _vp, C.POINTER(C.c_uint64)]),
    "pcv_terrain_heights": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_terrain_colors": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_terrain_counts": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_terrain_write_dir": (C.c_int, [_vp, C.c_char_p]),
    "pcv_terrain_free": (None, [_vp]),
    "pcv_terrain_check_params_host": (C.c_int, [C.POINTER(TerrainParams)]),
    "pcv_terrain_frame_host": (C.c_int, [C.POINTER(TerrainParams), _vp]),
    "pcv_terrain_vertex_host": (C.c_int, [C.POINTER(TerrainParams), C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcv_terrain_quad_masks_host": (C.c_int, [C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, _vp, _vp]),
    "pcv_terrain_tile_name_host": (C.c_int, [C.c_int32, C.c_int32, C.c_char_p, C.c_uint64]),
    "pcv_terrain_meta_json_host": (C.c_int, [C.POINTER(TerrainParams), C.c_uint64, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_maptiles_begin": (C.c_int, [_vp, C.POINTER(MapTilesParams), C.POINTER(_vp)]),
    "pcv_maptiles_add_points": (C.c_int, [_vp, C.c_uint64, _vp, _vp, _vp, _vp, C.c_int]),
    "pcv_maptiles_add_query_batch": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64]),
    "pcv_maptiles_add_s2_query": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64]),
    "pcv_maptiles_finish": (C.c_int, [_vp]),
    "pcv_maptiles_build_parents": (C.c_int, [_vp, C.c_uint32]),
    "pcv_maptiles_tiles": (C.c_int, [_vp, C.c_uint32, C.c_uint64, _vp, C.POINTER(C.c_uint64)]),
    "pcv_maptiles_images": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_maptiles_counts": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, _vp]),
    "pcv_maptiles_tile_pngs": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _vp, _vp]),
    "pcv_maptiles_write_dir": (C.c_int, [_vp, C.c_char_p, C.c_int]),
    "pcv_maptiles_info_get": (C.c_int, [_vp, C.POINTER(MapTilesInfo)]),
    "pcv_maptiles_free": (None, [_vp]),
    "pcv_maptiles_check_params_host": (C.c_int, [C.POINTER(MapTilesParams), C.c_uint32]),
    "pcv_maptiles_pixels_host": (C.c_int, [C.c_uint32, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pcv_maptiles_quad_index_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "pcv_maptiles_quad_tile_host": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "pcv_maptiles_json_host": (C.c_int, [C.c_uint32, C.c_uint32, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_las_header_host": (C.c_int, [C.c_char_p, C.POINTER(LasHeader)]),
    "pcv_las_check_params_host": (C.c_int, [C.POINTER(LasHeader), C.POINTER(LasParams)]),
    "pcv_las_extras_host": (C.c_int, [C.c_uint32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)]),
    "pcv_las_decode_host": (C.c_int, [C.POINTER(LasHeader), C.POINTER(LasParams), _vp, C.c_uint64, C.POINTER(LasColumns), C.POINTER(LasInfo)]),
    "pcv_las_read": (C.c_int, [C.c_char_p, C.POINTER(LasParams), C.POINTER(_vp)]),
    "pcv_las_num_points": (C.c_uint64, [_vp]),
    "pcv_las_points": (C.c_int, [_vp, C.POINTER(Points)]),
    "pcv_las_attributes": (C.c_int, [_vp, C.POINTER(C.c_uint32), _vp]),
    "pcv_las_info_get": (C.c_int, [_vp, C.POINTER(LasInfo)]),
    "pcv_las_free": (None, [_vp]),
    "pcv_las_load": (C.c_int, [_vp, C.c_char_p, C.POINTER(LasParams), C.POINTER(_vp)]),
    "pcv_las_cloud_info": (C.c_int, [_vp, C.POINTER(LasInfo)]),
    "pcv_las_cloud_points": (C.c_int, [_vp, C.POINTER(Points)]),
    "pcv_las_cloud_attributes": (C.c_int, [_vp, C.POINTER(C.c_uint32), _vp]),
    "pcv_las_cloud_read": (C.c_int, [_vp, C.c_char_p, _vp, C.c_uint64]),
    "pcv_las_cloud_free": (None, [_vp]),
    "pcv_las_decode": (C.c_int, [_vp, C.POINTER(LasHeader), C.POINTER(LasParams), _vp, C.c_uint64, C.c_int, C.POINTER(LasColumns),
                                 C.POINTER(LasInfo)]),
    "pcv_query_batch_las_records": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(LasWriteParams), C.c_uint64, C.c_int, _vp,
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(LasWriteInfo)]),
    "pcv_s2_query_las_records": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.POINTER(LasWriteParams), C.c_uint64, C.c_int, _vp,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(LasWriteInfo)]),
    "pcv_query_batch_write_las": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(LasWriteParams), C.POINTER(LasWriteInfo)]),
    "pcv_s2_query_write_las": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_char_p, C.POINTER(LasWriteParams), C.POINTER(LasWriteInfo)]),
    "pcv_las_write_check_params_host": (C.c_int, [C.POINTER(LasWriteParams), C.c_int, C.POINTER(C.c_char_p), _vp, C.c_uint32,
                                                  C.POINTER(LasWriteInfo)]),
    "pcv_las_encode_host": (C.c_int, [C.POINTER(LasWriteParams), C.c_uint64, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_char_p), _vp,
                                      C.POINTER(_vp), C.c_uint32, _vp, C.c_uint64, C.POINTER(LasWriteInfo)]),
    "pcv_las_write_header_host": (C.c_int, [C.POINTER(LasWriteParams), C.POINTER(LasWriteInfo), _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_las_append_check_host": (C.c_int, [C.c_char_p, C.POINTER(LasWriteParams), C.POINTER(LasWriteInfo), C.POINTER(C.c_uint64)]),
    "pcv_build_octree_from_las": (C.c_int, [_vp, C.POINTER(BuildParams), C.c_char_p, C.POINTER(LasParams), C.POINTER(_vp)]),
    "pcv_tiles3d_check_params_host": (C.c_int, [C.POINTER(Tiles3dParams)]),
    "pcv_tiles3d_rtc_host": (C.c_int, [C.POINTER(NodeInfo), C.POINTER(C.c_double * 3)]),
    "pcv_tiles3d_tile_host": (C.c_int, [C.POINTER(NodeInfo), C.POINTER(Tiles3dParams), _vp, _vp, _vp, _vp, C.c_uint64, C.POINTER(C.c_uint64),
                                        C.POINTER(Tiles3dTile)]),
    "pcv_tiles3d_tileset_json_host": (C.c_int, [_vp, C.c_uint64, C.POINTER(Tiles3dParams), _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_tiles3d_plan": (C.c_int, [_vp, C.POINTER(Tiles3dParams), C.POINTER(_vp)]),
    "pcv_tiles3d_info_get": (C.c_int, [_vp, C.POINTER(Tiles3dInfo)]),
    "pcv_tiles3d_tiles": (C.c_int, [_vp, C.c_uint64, _vp, C.POINTER(C.c_uint64)]),
    "pcv_tiles3d_tile_files": (C.c_int, [_vp, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _vp, _vp]),
    "pcv_tiles3d_tileset_json": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pcv_tiles3d_write_dir": (C.c_int, [_vp, C.c_char_p]),
    "pcv_tiles3d_free": (None, [_vp]),
}

_lib = None


def exported_symbols():
    return sorted(_SIGNATURES)


def load_library():
    """Load libpcv_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C point_cloud_viewer_amd/csrc). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if lib.pcv_abi_version() != ABI_VERSION:  # a stale libpcv_hip.so next to newer bindings: fail loudly, not subtly
        raise ImportError(f"{LIB_PATH} has ABI version {lib.pcv_abi_version()}, these bindings are written for {ABI_VERSION}: "
                          "rebuild it (make -C point_cloud_viewer_amd/csrc)")
    _lib = lib
    return lib
