"""ctypes binding of libohmhip.so (the C ABI declared in include/ohmhip.h).

The product path is the HIP library: there is NO CPU fallback.  Importing this module when the shared library is
missing raises ImportError loudly; calling into it without a GPU returns OHMHIP_ERR_NO_DEVICE which is raised as
OhmHipError.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# OHMHIP_LIB: development knob for A/B timing runs of differently built libraries (scripts/build_variant.sh).
LIB_PATH = os.environ.get("OHMHIP_LIB") or os.path.join(_HERE, "lib", "libohmhip.so")


class OhmHipError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib.ohmhip_error_string(status).decode() if "lib" in globals() else str(status)
        super().__init__(f"{what}: [{status}] {msg}" if what else f"[{status}] {msg}")


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950). ohm_amd has no CPU fallback.")

lib = C.CDLL(LIB_PATH)

OK = 0
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_CAPACITY, ERR_UNSUPPORTED, ERR_NOT_FOUND, ERR_INTERNAL, ERR_PEER = (-1, -2, -3, -4,
                                                                                                       -5, -6, -7)
MERGE_SHARED_ONLY, MERGE_FULL_UNION = 0, 1

(LID_OCCUPANCY, LID_MEAN, LID_COVARIANCE, LID_TRAVERSAL, LID_TOUCH_TIME, LID_INCIDENT, LID_INTENSITY, LID_HIT_MISS,
 LID_TSDF, LID_CLEARANCE, LID_COUNT) = range(11)
MODE_OCCUPANCY, MODE_NDT_OM, MODE_NDT_TM, MODE_TSDF = range(4)
FILTER_NONE, FILTER_GOOD, FILTER_CLIP = range(3)


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 256), ("arch", C.c_char * 64), ("total_memory", C.c_uint64),
                ("max_allocation", C.c_uint64), ("compute_units", C.c_int), ("lds_bytes_per_block", C.c_int),
                ("unified_memory", C.c_int)]


class ClearanceParams(C.Structure):
    """ohmhip_clearance_params"""
    _fields_ = [("search_radius", C.c_float), ("axis_scaling", C.c_float * 3), ("flags", C.c_uint)]


class HeightmapParams(C.Structure):
    """ohmhip_heightmap_params"""
    _fields_ = [("reference_pos", C.c_double * 3), ("cull_min", C.c_double * 3), ("cull_max", C.c_double * 3),
                ("grid_resolution", C.c_double), ("origin", C.c_double * 3), ("region_size", C.c_uint8),
                ("up_axis", C.c_int8), ("mode", C.c_uint8), ("floor", C.c_double), ("ceiling", C.c_double),
                ("min_clearance", C.c_double), ("flags", C.c_uint)]


class HeightmapExtents(C.Structure):
    """ohmhip_heightmap_extents"""
    _fields_ = [("min_region", C.c_int16 * 3), ("min_local", C.c_uint8 * 4), ("max_region", C.c_int16 * 3),
                ("max_local", C.c_uint8 * 4), ("na", C.c_uint32), ("nb", C.c_uint32), ("first_region", C.c_int16 * 2),
                ("first_local", C.c_uint8 * 2), ("use_mean", C.c_uint8), ("populated", C.c_uint8), ("ma", C.c_uint32),
                ("mb", C.c_uint32)]


class HeightmapFillStats(C.Structure):
    """ohmhip_heightmap_fill_stats"""
    _fields_ = [("visits", C.c_uint64), ("populated", C.c_uint64), ("cells", C.c_uint64), ("revisits", C.c_uint64),
                ("generations", C.c_uint32), ("largest_generation", C.c_uint32)]


class HeightmapLayeredParams(C.Structure):
    """ohmhip_heightmap_layered_params"""
    _fields_ = [("base", HeightmapParams), ("virtual_surface_filter_threshold", C.c_uint32), ("reserved", C.c_uint32)]


class HeightmapLayeredStats(C.Structure):
    """ohmhip_heightmap_layered_stats"""
    _fields_ = [("visits", C.c_uint64), ("populated", C.c_uint64), ("cells", C.c_uint64), ("voxels", C.c_uint64),
                ("repeats", C.c_uint64), ("too_close", C.c_uint64), ("filtered", C.c_uint64),
                ("multi_layer_columns", C.c_uint64), ("layers", C.c_uint32), ("generations", C.c_uint32),
                ("largest_generation", C.c_uint32)]


HM_GENERATE_VIRTUAL_SURFACE, HM_PROMOTE_VIRTUAL_BELOW, HM_IGNORE_VOXEL_MEAN, HM_SURFACE_NORMALS = 1, 2, 4, 8


class CloudParams(C.Structure):
    """ohmhip_cloud_params"""
    _fields_ = [("min_extents", C.c_double * 3), ("max_extents", C.c_double * 3), ("density_threshold", C.c_float),
                ("surface_distance", C.c_float), ("colour_range", C.c_float), ("export_type", C.c_int32),
                ("flags", C.c_uint32), ("mode", C.c_uint8)]


CLOUD_OCCUPANCY, CLOUD_DENSITY, CLOUD_TSDF, CLOUD_CLEARANCE = range(4)
CLOUD_EXPORT_FREE, CLOUD_IGNORE_VOXEL_MEAN, CLOUD_USE_EXTENTS = 1, 2, 4
CLOUD_CHUNK_VOXELS = 4096  # OHMHIP_CLOUD_CHUNK_VOXELS


class NeighboursParams(C.Structure):
    """ohmhip_neighbours_params"""
    _fields_ = [("search_radius", C.c_float), ("query_flags", C.c_uint)]


QF_UNKNOWN_AS_OCCUPIED, QF_NEAREST_RESULT = 1, 2


class PointFilterParams(C.Structure):
    """ohmhip_point_filter_params"""
    _fields_ = [("expected_value_tolerance", C.c_double), ("flags", C.c_uint32)]


COV_ABSENT, COV_DECOMPOSED, COV_NON_FINITE = range(3)  # OHMHIP_COV_*

PF_OCCUPANCY_ONLY = 1
PF_PIECE_POINTS = 1 << 18  # OHMHIP_PF_PIECE_POINTS


class CopyParams(C.Structure):
    """ohmhip_copy_params"""
    _fields_ = [("flags", C.c_uint), ("layers", C.c_uint), ("min_extents", C.c_double * 3),
                ("max_extents", C.c_double * 3), ("keys_xyz", C.c_void_p), ("key_count", C.c_size_t)]


class CopyStats(C.Structure):
    """ohmhip_copy_stats"""
    _fields_ = [("regions_passed", C.c_uint64), ("regions_created", C.c_uint64), ("keys_absent", C.c_uint64),
                ("bytes_copied", C.c_uint64), ("layers_copied", C.c_uint)]


COPY_DIRTY_ONLY, COPY_USE_EXTENTS = 1, 2

CMP_CONTINUE = 1
CMP_MAX_MEMBERS = 6  # OHMHIP_CMP_MAX_MEMBERS


class CompareParams(C.Structure):
    """ohmhip_compare_params"""
    _fields_ = [("flags", C.c_uint), ("layer_id", C.c_int), ("tolerance_members", C.c_uint),
                ("tolerance_bits", C.c_uint64 * CMP_MAX_MEMBERS), ("keys_xyz", C.c_void_p), ("key_count", C.c_size_t)]


class CompareResult(C.Structure):
    """ohmhip_compare_result"""
    _fields_ = [("voxels_passed", C.c_uint64), ("voxels_failed", C.c_uint64), ("layout_match", C.c_int32),
                ("member_count", C.c_uint32), ("regions_compared", C.c_uint64), ("regions_missing", C.c_uint64),
                ("keys_absent", C.c_uint64), ("mismatch_count", C.c_uint64), ("missing_count", C.c_uint64),
                ("member_failed", C.c_uint64 * CMP_MAX_MEMBERS), ("member_max_diff", C.c_uint64 * CMP_MAX_MEMBERS)]


EDIT_HIT, EDIT_MISS, EDIT_HIT_SAMPLE = 1, 2, 3  # OHMHIP_EDIT_*


class VoxelEditStats(C.Structure):
    """ohmhip_voxel_edit_stats"""
    _fields_ = [("applied", C.c_uint64), ("null_keys", C.c_uint64), ("distinct_voxels", C.c_uint64),
                ("regions_touched", C.c_uint64), ("regions_created", C.c_uint64)]


LAYOUT_DISCARD_MAP = 1  # OHMHIP_LAYOUT_DISCARD_MAP


class LayerChangeStats(C.Structure):
    """ohmhip_layer_change_stats"""
    _fields_ = [("layers_before", C.c_uint), ("layers_after", C.c_uint), ("regions_resident", C.c_uint64),
                ("regions_in_store", C.c_uint64), ("regions_evicted", C.c_uint64),
                ("bytes_per_region_before", C.c_uint64), ("bytes_per_region_after", C.c_uint64)]


class MapConfig(C.Structure):
    _fields_ = [("resolution", C.c_double), ("region_dim", C.c_int * 3), ("origin", C.c_double * 3),
                ("layers", C.c_uint), ("mode", C.c_int), ("hit_value", C.c_float), ("miss_value", C.c_float),
                ("threshold_value", C.c_float), ("min_value", C.c_float), ("max_value", C.c_float),
                ("saturate_at_min", C.c_int), ("saturate_at_max", C.c_int), ("ray_filter", C.c_int),
                ("ray_filter_range", C.c_double), ("ndt_sensor_noise", C.c_float),
                ("ndt_sample_threshold", C.c_uint), ("ndt_adaptation_rate", C.c_float),
                ("ndt_reinit_threshold", C.c_float), ("ndt_reinit_count", C.c_uint),
                ("ndt_initial_intensity_cov", C.c_float), ("tsdf_max_weight", C.c_float), ("tsdf_trunc", C.c_float),
                ("tsdf_dropoff", C.c_float), ("tsdf_sparsity", C.c_float), ("gpu_mem_size", C.c_uint64),
                ("region_capacity", C.c_uint32)]


RFS_GOOD, RFS_CLIP, RFS_CLIP_BOUNDED, RFS_CLIP_TO_BOUNDS = 1, 2, 3, 4  # OHMHIP_RFS_*
MAX_RAY_FILTER_STAGES = 4  # OHMHIP_MAX_RAY_FILTER_STAGES


class RayFilterStage(C.Structure):
    """ohmhip_ray_filter_stage"""
    _fields_ = [("kind", C.c_int), ("reserved", C.c_int), ("range", C.c_double), ("box_min", C.c_double * 3),
                ("box_max", C.c_double * 3)]


class MergeStats(C.Structure):
    _fields_ = [("regions_local", C.c_uint32), ("regions_union", C.c_uint32), ("regions_shared", C.c_uint32),
                ("payload_bytes", C.c_uint64), ("key_bytes", C.c_uint64), ("ms_total", C.c_float)]


class CacheStats(C.Structure):
    _fields_ = [("hits", C.c_uint64), ("misses", C.c_uint64), ("full", C.c_uint64), ("regions_resident", C.c_uint32),
                ("region_capacity", C.c_uint32), ("bytes_per_region", C.c_uint64), ("memory_limit", C.c_uint64),
                ("evictions", C.c_uint64), ("readmissions", C.c_uint64), ("regions_spilled", C.c_uint32),
                ("spill_enabled", C.c_uint32), ("writebacks", C.c_uint64), ("writeback_hits", C.c_uint64),
                ("writeback_stale", C.c_uint64)]


class Partition(C.Structure):
    _fields_ = [("world_size", C.c_uint32), ("rank", C.c_uint32), ("block_shift", C.c_int32),
                ("grid_origin", C.c_int32 * 3), ("grid_dims", C.c_uint32 * 3), ("owners", C.c_void_p)]


COMM_ID_BYTES = 128


class BatchStats(C.Structure):
    _fields_ = [("rays_in", C.c_uint64), ("rays_integrated", C.c_uint64), ("voxel_visits", C.c_uint64),
                ("ray_region_segments", C.c_uint64), ("regions_touched", C.c_uint32),
                ("regions_resident", C.c_uint32), ("ms_total", C.c_float), ("ms_setup", C.c_float),
                ("ms_walk", C.c_float), ("ms_apply", C.c_float)]


_vp = C.c_void_p
_sigs = {
    "ohmhip_error_string": (C.c_char_p, [C.c_int]),
    "ohmhip_build_id": (C.c_char_p, []),
    "ohmhip_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ohmhip_device_select": (C.c_int, [C.c_int]),
    "ohmhip_device_get_info": (C.c_int, [C.c_int, C.POINTER(DeviceInfo)]),
    "ohmhip_stream_create": (C.c_int, [C.POINTER(_vp)]),
    "ohmhip_stream_destroy": (C.c_int, [_vp]),
    "ohmhip_stream_finish": (C.c_int, [_vp]),
    "ohmhip_stream_wait_event": (C.c_int, [_vp, _vp]),
    "ohmhip_event_create": (C.c_int, [C.POINTER(_vp)]),
    "ohmhip_event_destroy": (C.c_int, [_vp]),
    "ohmhip_event_record": (C.c_int, [_vp, _vp]),
    "ohmhip_event_wait": (C.c_int, [_vp]),
    "ohmhip_event_is_complete": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "ohmhip_event_elapsed_ms": (C.c_int, [_vp, _vp, C.POINTER(C.c_float)]),
    "ohmhip_buffer_create": (C.c_int, [C.POINTER(_vp), C.c_size_t, C.c_uint]),
    "ohmhip_buffer_destroy": (C.c_int, [_vp]),
    "ohmhip_buffer_resize": (C.c_int, [_vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ohmhip_buffer_size": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "ohmhip_buffer_ptr": (C.c_int, [_vp, C.POINTER(_vp)]),
    "ohmhip_buffer_write": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp]),
    "ohmhip_buffer_read": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp]),
    "ohmhip_buffer_fill": (C.c_int, [_vp, C.c_int, C.c_size_t, C.c_size_t, _vp]),
    "ohmhip_device_synchronize": (C.c_int, []),
    "ohmhip_buffer_fill_pattern": (C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, C.c_size_t, _vp, _vp, _vp]),
    "ohmhip_buffer_copy": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp]),
    "ohmhip_buffer_flags": (C.c_int, [_vp, C.POINTER(C.c_uint)]),
    "ohmhip_host_alloc": (C.c_int, [C.POINTER(_vp), C.c_size_t]),
    "ohmhip_host_free": (C.c_int, [_vp]),
    "ohmhip_layer_voxel_bytes": (C.c_size_t, [C.c_int]),
    "ohmhip_map_config_default": (None, [C.POINTER(MapConfig)]),
    "ohmhip_map_create": (C.c_int, [C.POINTER(_vp), C.POINTER(MapConfig)]),
    "ohmhip_map_destroy": (C.c_int, [_vp]),
    "ohmhip_map_integrate_rays": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_uint, C.POINTER(C.c_size_t)]),
    "ohmhip_map_integrate_rays_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_uint,
                                                   C.POINTER(C.c_size_t)]),
    "ohmhip_map_sync": (C.c_int, [_vp]),
    "ohmhip_map_last_stats": (C.c_int, [_vp, C.POINTER(BatchStats)]),
    "ohmhip_map_region_count": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "ohmhip_map_regions": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ohmhip_map_dirty_regions": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ohmhip_map_clear_dirty": (C.c_int, [_vp]),
    "ohmhip_map_read_regions": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp]),
    "ohmhip_map_write_regions": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp]),
    "ohmhip_map_clear": (C.c_int, [_vp]),
    "ohmhip_map_remove_regions": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ohmhip_transform_samples": (C.c_int, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, C.c_double, _vp, _vp,
                                           C.POINTER(C.c_uint32)]),
    "ohmhip_pattern_create": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "ohmhip_pattern_destroy": (C.c_int, [_vp]),
    "ohmhip_pattern_ray_count": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "ohmhip_pattern_build_rays": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_double, _vp]),
    "ohmhip_pattern_last_rays": (C.c_int, [_vp, _vp, C.POINTER(C.c_size_t)]),
    "ohmhip_map_apply_pattern": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_int, C.c_double, C.c_float, C.c_uint,
                                           C.POINTER(C.c_size_t)]),
    "ohmhip_map_can_copy": (C.c_int, [_vp, _vp]),
    "ohmhip_map_copy": (C.c_int, [_vp, _vp, C.POINTER(CopyParams), C.POINTER(CopyStats)]),
    "ohmhip_map_compare": (C.c_int, [_vp, _vp, C.POINTER(CompareParams), C.c_uint64, _vp, C.c_uint64, _vp,
                                     C.POINTER(CompareResult)]),
    "ohmhip_map_compare_device": (C.c_int, [_vp, _vp, C.POINTER(CompareParams), C.c_uint64, _vp, C.c_uint64, _vp, _vp]),
    "ohmhip_map_batch_timings": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_float)]),
    "ohmhip_comm_exchange_side": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp]),
    "ohmhip_gather_rows": (C.c_int, [_vp, _vp, C.c_size_t, C.c_uint32, _vp, _vp]),
    "ohmhip_map_reserve_rays": (C.c_int, [_vp, C.c_size_t]),
    "ohmhip_map_set_first_ray_time": (C.c_int, [_vp, C.c_double]),
    "ohmhip_map_first_ray_time": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "ohmhip_map_set_phase_timing": (C.c_int, [_vp, C.c_int]),
    "ohmhip_map_batches_launched": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "ohmhip_map_pipeline_counts": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ohmhip_map_order_counts": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "ohmhip_map_rays_beyond_tiles": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "ohmhip_map_line_keys": (C.c_int, [_vp, _vp, C.c_size_t, C.c_uint32, _vp, _vp]),
    "ohmhip_map_rays_query": (C.c_int, [_vp, _vp, C.c_size_t, C.c_double, _vp, _vp, _vp, _vp]),
    "ohmhip_map_rays_query_device": (C.c_int, [_vp, _vp, C.c_size_t, C.c_double, _vp, _vp, _vp, _vp]),
    "ohmhip_map_clearance_regions": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    "ohmhip_map_clearance_regions_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    "ohmhip_map_clearance_keys": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    "ohmhip_map_clearance_stale_regions": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ohmhip_map_clearance_update": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ohmhip_map_clearance_update_regions": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_int, C.POINTER(C.c_size_t)]),
    "ohmhip_map_heightmap_extents": (C.c_int, [_vp, C.POINTER(HeightmapParams), C.POINTER(HeightmapExtents)]),
    "ohmhip_map_heightmap": (C.c_int, [_vp, C.POINTER(HeightmapParams), _vp, _vp, _vp, _vp, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]),
    "ohmhip_map_heightmap_device": (C.c_int, [_vp, C.POINTER(HeightmapParams), _vp, _vp, _vp, _vp, _vp]),
    "ohmhip_map_heightmap_fill_extents": (C.c_int, [_vp, C.POINTER(HeightmapParams), C.POINTER(HeightmapExtents)]),
    "ohmhip_map_heightmap_fill": (C.c_int, [_vp, C.POINTER(HeightmapParams), _vp, _vp, _vp, _vp, _vp, C.c_uint64,
                                            C.POINTER(HeightmapFillStats)]),
    "ohmhip_map_heightmap_fill_device": (C.c_int, [_vp, C.POINTER(HeightmapParams), _vp, _vp, _vp, _vp, _vp, C.c_uint64,
                                                   C.POINTER(HeightmapFillStats)]),
    "ohmhip_map_heightmap_layered_extents": (C.c_int, [_vp, C.POINTER(HeightmapLayeredParams),
                                                       C.POINTER(HeightmapExtents)]),
    "ohmhip_map_heightmap_layered": (C.c_int, [_vp, C.POINTER(HeightmapLayeredParams), C.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                               _vp, C.c_uint64, C.POINTER(HeightmapLayeredStats)]),
    "ohmhip_map_heightmap_layered_device": (C.c_int, [_vp, C.POINTER(HeightmapLayeredParams), C.c_uint32, _vp, _vp, _vp,
                                                      _vp, _vp, _vp, C.c_uint64, C.POINTER(HeightmapLayeredStats)]),
    "ohmhip_map_cloud_count": (C.c_int, [_vp, C.POINTER(CloudParams), C.POINTER(C.c_uint64)]),
    "ohmhip_map_cloud": (C.c_int, [_vp, C.POINTER(CloudParams), C.c_uint64, _vp, _vp, _vp, C.POINTER(C.c_uint64)]),
    "ohmhip_map_cloud_device": (C.c_int, [_vp, C.POINTER(CloudParams), C.c_uint64, _vp, _vp, _vp, _vp]),
    "ohmhip_map_nearest_neighbours": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(NeighboursParams), C.c_uint64, _vp, _vp,
                                                _vp, C.POINTER(C.c_uint64)]),
    "ohmhip_map_nearest_neighbours_device": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(NeighboursParams), C.c_uint64,
                                                       _vp, _vp, _vp, _vp]),
    "ohmhip_map_voxel_keys": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "ohmhip_map_read_voxels": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp]),
    "ohmhip_map_read_voxels_device": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, _vp]),
    "ohmhip_covariance_decompose": (C.c_int, [_vp, C.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    "ohmhip_map_covariance_eigen": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, _vp]),
    "ohmhip_map_covariance_eigen_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, _vp]),
    "ohmhip_map_covariance_ellipsoids_count": (C.c_int, [_vp, C.POINTER(CloudParams), C.POINTER(C.c_uint64)]),
    "ohmhip_map_covariance_ellipsoids": (C.c_int, [_vp, C.POINTER(CloudParams), C.c_uint64, _vp, _vp, _vp, _vp, _vp,
                                                   C.POINTER(C.c_uint64)]),
    "ohmhip_map_covariance_ellipsoids_device": (C.c_int, [_vp, C.POINTER(CloudParams), C.c_uint64, _vp, _vp, _vp, _vp,
                                                          _vp, _vp]),
    "ohmhip_map_write_voxels": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(VoxelEditStats)]),
    "ohmhip_map_write_voxels_device": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.POINTER(VoxelEditStats)]),
    "ohmhip_map_integrate_voxels": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_size_t, C.POINTER(VoxelEditStats)]),
    "ohmhip_map_integrate_voxels_device": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, C.c_size_t,
                                                     C.POINTER(VoxelEditStats)]),
    "ohmhip_map_filter_points": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(PointFilterParams), C.c_uint64, _vp, _vp, _vp,
                                           _vp, C.POINTER(C.c_uint64)]),
    "ohmhip_map_filter_points_device": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.POINTER(PointFilterParams),
                                                  C.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "ohmhip_map_device_layer_ptr": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "ohmhip_map_region_slot": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32)]),
    "ohmhip_map_ensure_regions": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "ohmhip_map_mark_dirty": (C.c_int, [_vp, _vp, C.c_size_t]),
    "ohmhip_map_integrate_rays_filtered": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_uint, _vp,
                                                    C.POINTER(C.c_size_t)]),
    "ohmhip_map_set_ray_filter_stages": (C.c_int, [_vp, C.POINTER(RayFilterStage), C.c_uint]),
    "ohmhip_map_ray_filter_stages": (C.c_int, [_vp, C.POINTER(RayFilterStage), C.c_uint, C.POINTER(C.c_uint)]),
    "ohmhip_map_apply_ray_filter": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.POINTER(C.c_size_t)]),
    "ohmhip_map_apply_ray_filter_device": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.POINTER(C.c_size_t)]),
    "ohmhip_map_update_config": (C.c_int, [_vp, C.POINTER(MapConfig)]),
    "ohmhip_map_update_layers": (C.c_int, [_vp, C.c_uint, C.c_uint, C.POINTER(LayerChangeStats)]),
    "ohmhip_map_layers": (C.c_int, [_vp, C.POINTER(C.c_uint)]),
    "ohmhip_map_set_batch_coalescing": (C.c_int, [_vp, C.c_size_t]),
    "ohmhip_map_set_async_launch": (C.c_int, [_vp, C.c_int]),
    "ohmhip_map_set_region_ownership": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.c_int]),
    "ohmhip_region_owner": (C.c_int, [_vp, C.c_size_t, C.c_int, C.c_uint32, _vp]),
    "ohmhip_map_set_region_partition": (C.c_int, [_vp, C.POINTER(Partition)]),
    "ohmhip_map_region_owners": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "ohmhip_partition_owners": (C.c_int, [C.POINTER(Partition), _vp, C.c_size_t, _vp]),
    "ohmhip_map_route_rays": (C.c_int, [_vp, _vp, C.c_size_t, C.c_uint, _vp, _vp, C.c_size_t, _vp,
                                        C.POINTER(C.c_uint64)]),
    "ohmhip_comm_exchange_counts": (C.c_int, [_vp, _vp, _vp, _vp]),
    "ohmhip_comm_exchange_rays": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ohmhip_map_cache_stats": (C.c_int, [_vp, C.POINTER(CacheStats), C.c_int]),
    "ohmhip_map_set_memory_limit": (C.c_int, [_vp, C.c_uint64]),
    "ohmhip_map_set_spill_to_host": (C.c_int, [_vp, C.c_int]),
    "ohmhip_map_set_spill_writeback": (C.c_int, [_vp, C.c_int]),
    "ohmhip_comm_unique_id": (C.c_int, [_vp]),
    "ohmhip_comm_init_rank": (C.c_int, [C.POINTER(_vp), _vp, C.c_int, C.c_int]),
    "ohmhip_comm_destroy": (C.c_int, [_vp]),
    "ohmhip_map_enable_merge": (C.c_int, [_vp]),
    "ohmhip_map_merge_replicas": (C.c_int, [_vp, _vp, C.POINTER(MergeStats)]),
    "ohmhip_map_merge_keys": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "ohmhip_map_merge_pack": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    "ohmhip_map_merge_apply": (C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp]),
    "ohmhip_map_merge_finish": (C.c_int, [_vp]),
    "ohmhip_map_set_merge_mode": (C.c_int, [_vp, C.c_int]),
}

EXPORTED_SYMBOLS = sorted(_sigs)

for _name, (_res, _args) in _sigs.items():
    _fn = getattr(lib, _name)  # AttributeError here == the library does not export what include/ohmhip.h declares
    _fn.restype = _res
    _fn.argtypes = _args


def check(status, what=""):
    if status != OK:
        raise OhmHipError(status, what)
