"""Point clouds out of the device-resident map of a GpuMap (ohmhip_map_cloud: include/ohmhip.h, "POINT CLOUDS"): what
ohmtools::saveCloud, saveDensityCloud, saveTsdfCloud and saveClearanceCloud (ohmtools/OhmCloud.cpp) collect after a
syncVoxels(), compacted on the device.  Only the points cross to the host."""
import ctypes as C
import enum

import numpy as np

from . import _lib as L


class CloudMode(enum.IntEnum):
    OCCUPANCY = L.CLOUD_OCCUPANCY
    DENSITY = L.CLOUD_DENSITY
    TSDF = L.CLOUD_TSDF
    CLEARANCE = L.CLOUD_CLEARANCE


#: ohm::GpuKey (ohmgpu/GpuKey.h:37-46)
GPU_KEY_DTYPE = np.dtype([("region", "<i2", (3,)), ("voxel", "u1", (4,))])
assert GPU_KEY_DTYPE.itemsize == 10
#: voxels per unit of device work (OHMHIP_CLOUD_CHUNK_VOXELS)
CLOUD_CHUNK_VOXELS = L.CLOUD_CHUNK_VOXELS


class VoxelCloud:
    """positions (n, 3) float64, keys (n,) GPU_KEY_DTYPE, values (n,) float32 -- the first len(positions) points in
    the library's fixed order -- and count, the number of all matching voxels."""

    def __init__(self, positions, keys, values, count, mode=CloudMode.OCCUPANCY):
        self.positions = positions
        self.keys = keys
        self.values = values
        self.count = int(count)
        self.mode = CloudMode(mode)

    def __len__(self):
        return self.positions.shape[0]


def cloud_params(mode=CloudMode.OCCUPANCY, export_free=False, ignore_voxel_mean=False, density_threshold=0.0,
                 surface_distance=float("inf"), colour_range=0.0, export_type=0, extents=None):
    """The ohmhip_cloud_params of a request; extents = (min, max) or None."""
    p = L.CloudParams()
    p.mode = int(mode)
    p.flags = ((L.CLOUD_EXPORT_FREE if export_free else 0) | (L.CLOUD_IGNORE_VOXEL_MEAN if ignore_voxel_mean else 0) |
               (L.CLOUD_USE_EXTENTS if extents is not None else 0))
    p.density_threshold = float(density_threshold)
    p.surface_distance = float(surface_distance)
    p.colour_range = float(colour_range)
    p.export_type = int(export_type)
    if extents is not None:
        for i in range(3):
            p.min_extents[i] = float(extents[0][i])
            p.max_extents[i] = float(extents[1][i])
    return p


def count_cloud(gpu_map, **kw):
    """ohmhip_map_cloud_count: the number of matching voxels."""
    p = cloud_params(**kw)
    n = C.c_uint64(0)
    L.check(L.lib.ohmhip_map_cloud_count(gpu_map._handle, C.byref(p), C.byref(n)), "ohmhip_map_cloud_count")
    return int(n.value)


def extract_cloud(gpu_map, mode=CloudMode.OCCUPANCY, export_free=False, ignore_voxel_mean=False, density_threshold=0.0,
                  surface_distance=float("inf"), colour_range=0.0, export_type=0, extents=None, capacity=None):
    """The cloud of gpu_map's device map.  capacity=None: a count call first, then arrays of exactly that size."""
    p = cloud_params(mode, export_free, ignore_voxel_mean, density_threshold, surface_distance, colour_range,
                     export_type, extents)
    handle = gpu_map._handle
    n = C.c_uint64(0)
    if capacity is None:
        L.check(L.lib.ohmhip_map_cloud_count(handle, C.byref(p), C.byref(n)), "ohmhip_map_cloud_count")
        capacity = int(n.value)
    capacity = int(capacity)
    positions = np.empty((capacity, 3), dtype=np.float64)
    keys = np.empty(capacity, dtype=GPU_KEY_DTYPE)
    values = np.empty(capacity, dtype=np.float32)
    L.check(L.lib.ohmhip_map_cloud(handle, C.byref(p), capacity, positions.ctypes.data if capacity else None,
                                   keys.ctypes.data if capacity else None, values.ctypes.data if capacity else None,
                                   C.byref(n)), "ohmhip_map_cloud")
    held = min(int(n.value), capacity)
    return VoxelCloud(positions[:held], keys[:held], values[:held], n.value, mode)


def write_ply(file_name, cloud, colour=None):
    """Binary little-endian PLY: x y z as doubles, plus red green blue uchar when `colour` is an (n, 3) array or a
    callable on the cloud that returns one.  Returns the number of points written."""
    positions = np.ascontiguousarray(cloud.positions, dtype="<f8").reshape(-1, 3)
    n = positions.shape[0]
    if callable(colour):
        colour = colour(cloud)
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n, "property double x",
              "property double y", "property double z"]
    if colour is not None:
        colour = np.asarray(colour, dtype=np.uint8).reshape(n, 3)
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header.append("end_header")
    vertices = np.empty(n, dtype=np.dtype(fields))
    vertices["x"], vertices["y"], vertices["z"] = positions[:, 0], positions[:, 1], positions[:, 2]
    if colour is not None:
        vertices["red"], vertices["green"], vertices["blue"] = colour[:, 0], colour[:, 1], colour[:, 2]
    with open(file_name, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vertices.tobytes())
    return n


def save_cloud(file_name, gpu_map, colour=None, ignore_voxel_mean=False, export_free=False):
    """ohmtools::saveCloud(file_name, map, SaveCloudOptions) (ohmtools/OhmCloud.cpp:453-493)."""
    return write_ply(file_name, extract_cloud(gpu_map, CloudMode.OCCUPANCY, export_free=export_free,
                                              ignore_voxel_mean=ignore_voxel_mean), colour)


def save_density_cloud(file_name, gpu_map, density_threshold=0.0, colour=None, ignore_voxel_mean=False):
    """ohmtools::saveDensityCloud(file_name, map, SaveDensityCloudOptions), by the rule it documents."""
    return write_ply(file_name, extract_cloud(gpu_map, CloudMode.DENSITY, density_threshold=density_threshold,
                                              ignore_voxel_mean=ignore_voxel_mean), colour)


def save_tsdf_cloud(file_name, gpu_map, surface_distance, colour=None):
    """ohmtools::saveTsdfCloud(file_name, map, surface_distance, colour_select) (:950-987)."""
    return write_ply(file_name, extract_cloud(gpu_map, CloudMode.TSDF, surface_distance=surface_distance), colour)


def save_clearance_cloud(file_name, gpu_map, min_extents, max_extents, colour_range, export_type=0, colour=None):
    """ohmtools::saveClearanceCloud(file_name, map, min_extents, max_extents, colour_range, export_type) (:879-947):
    export_type is an ohm::OccupancyType, -1 unobserved and up, 0 free and up, 1 occupied."""
    return write_ply(file_name, extract_cloud(gpu_map, CloudMode.CLEARANCE, colour_range=colour_range,
                                              export_type=export_type, extents=(min_extents, max_extents)), colour)


def write_filtered_ply(file_name, points, timestamps):
    """The cloud ohmfilter writes (utils/ohmfilter/ohmfilter.cpp:226-256), in write_ply's conventions: binary little-endian
    PLY with x y z time, all doubles, one vertex per row of points.  Returns the number of points written."""
    points = np.ascontiguousarray(points, dtype="<f8").reshape(-1, 3)
    n = points.shape[0]
    timestamps = np.ascontiguousarray(timestamps, dtype="<f8").reshape(n)
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n, "property double x",
              "property double y", "property double z", "property double time", "end_header"]
    vertices = np.empty(n, dtype=np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("time", "<f8")]))
    vertices["x"], vertices["y"], vertices["z"], vertices["time"] = points[:, 0], points[:, 1], points[:, 2], timestamps
    with open(file_name, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vertices.tobytes())
    return n


def filter_cloud(file_name, gpu_map, points, timestamps, expected_value_tolerance=-1.0, occupancy_only=False):
    """ohmfilter's filterCloud (utils/ohmfilter/ohmfilter.cpp:158-279) against gpu_map's device map: the points that fall
    in an occupied voxel -- and, on an NDT map with a tolerance >= 0, inside its Gaussian -- written with their time stamps
    in input order (GpuMap.filterPoints, write_filtered_ply).  timestamps=None writes zeros.  Returns (points exported,
    points removed)."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    timestamps = np.zeros(points.shape[0]) if timestamps is None else np.asarray(timestamps, dtype=np.float64).reshape(-1)
    if timestamps.shape[0] != points.shape[0]:
        raise ValueError("one time stamp per point")
    _, kept, _, _ = gpu_map.filterPoints(points, expected_value_tolerance, occupancy_only)
    kept = kept.astype(np.int64)
    exported = write_filtered_ply(file_name, points[kept], timestamps[kept])
    return exported, points.shape[0] - exported
