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


class EllipsoidCloud(VoxelCloud):
    """A VoxelCloud whose rows also carry the covariance ellipsoid of their voxel: axes (n, 3, 3) float64 with
    axes[i, c] the unit axis of scale c (the rotation of covarianceUnitSphereTransformation, column by column) and
    scales (n, 3) float64, ascending -- one standard deviation, without ohm2ply's display factor."""

    def __init__(self, positions, axes, scales, keys, values, count):
        super().__init__(positions, keys, values, count, CloudMode.OCCUPANCY)
        self.axes = axes
        self.scales = scales


def extract_covariance_ellipsoids(gpu_map, extents=None, capacity=None):
    """ohm2ply --mode covariance without the download (ohmhip_map_covariance_ellipsoids): for every occupied voxel of
    an NDT map -- the selection and the order of extract_cloud(gpu_map, extents=extents), row for row -- its mean
    position and the rotation and scale that deform a unit sphere into its covariance's ellipsoid, decomposed on the
    device by the rule D1-D5 of include/ohmhip.h.  capacity=None: a count call first, then arrays of that size."""
    p = cloud_params(CloudMode.OCCUPANCY, extents=extents)
    handle = gpu_map._handle
    n = C.c_uint64(0)
    if capacity is None:
        L.check(L.lib.ohmhip_map_covariance_ellipsoids_count(handle, C.byref(p), C.byref(n)),
                "ohmhip_map_covariance_ellipsoids_count")
        capacity = int(n.value)
    capacity = int(capacity)
    positions = np.empty((capacity, 3), dtype=np.float64)
    axes = np.empty((capacity, 3, 3), dtype=np.float64)
    scales = np.empty((capacity, 3), dtype=np.float64)
    keys = np.empty(capacity, dtype=GPU_KEY_DTYPE)
    values = np.empty(capacity, dtype=np.float32)
    arrays = [a.ctypes.data if capacity else None for a in (positions, axes, scales, keys, values)]
    L.check(L.lib.ohmhip_map_covariance_ellipsoids(handle, C.byref(p), capacity, *arrays, C.byref(n)),
            "ohmhip_map_covariance_ellipsoids")
    held = min(int(n.value), capacity)
    return EllipsoidCloud(positions[:held], axes[:held], scales[:held], keys[:held], values[:held], n.value)


def icosphere(subdivisions=1):
    """A unit sphere as (vertices (V, 3) float64, faces (F, 3) int32): an icosahedron whose faces are split in four
    `subdivisions` times, the new vertices pushed onto the sphere.  1: 42 vertices, 80 faces."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    vertices = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    vertices = [tuple(np.array(v, dtype=np.float64) / np.linalg.norm(v)) for v in vertices]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
             (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
             (8, 6, 7), (9, 8, 1)]
    for _ in range(int(subdivisions)):
        midpoint = {}

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in midpoint:
                m = (np.array(vertices[i]) + np.array(vertices[j])) * 0.5
                vertices.append(tuple(m / np.linalg.norm(m)))
                midpoint[key] = len(vertices) - 1
            return midpoint[key]

        split = []
        for a, b, c in faces:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            split += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = split
    return np.array(vertices, dtype=np.float64), np.array(faces, dtype=np.int32)


COVARIANCE_DISPLAY_SCALE = float(np.sqrt(3.0))  #: ohm2ply's factor on the scales (utils/ohm2ply/ohm2ply.cpp:845-1018)


def write_ellipsoid_ply(file_name, ellipsoids, subdivisions=1, display_scale=COVARIANCE_DISPLAY_SCALE):
    """Binary little-endian PLY mesh: per ellipsoid one icosphere, each unit vertex u mapped to position + R (scale *
    display_scale * u); vertices x y z as doubles, faces as uchar-counted int lists.  Returns (vertices, faces)."""
    sphere, faces = icosphere(subdivisions)
    n = len(ellipsoids)
    scaled = sphere[None, :, :] * (ellipsoids.scales * display_scale)[:, None, :]      # (n, V, 3): along the axes
    # axes[i, c, r]: column c of the rotation -- world = sum_c scaled[c] * axis_c
    world = np.einsum("nvc,ncr->nvr", scaled, ellipsoids.axes) + ellipsoids.positions[:, None, :]
    vertices = np.ascontiguousarray(world.reshape(-1, 3), dtype="<f8")
    index = faces[None, :, :] + (np.arange(n, dtype=np.int64) * sphere.shape[0])[:, None, None]
    face_records = np.empty(n * faces.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    face_records["n"] = 3
    face_records["v"] = index.reshape(-1, 3)
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % vertices.shape[0], "property double x",
              "property double y", "property double z", "element face %d" % face_records.shape[0],
              "property list uchar int vertex_indices", "end_header"]
    with open(file_name, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vertices.tobytes())
        fh.write(face_records.tobytes())
    return vertices.shape[0], face_records.shape[0]


def save_covariance_cloud(file_name, gpu_map, extents=None, subdivisions=1):
    """ohm2ply --mode covariance: the ellipsoid of every occupied voxel of an NDT map as a triangle mesh, with ohm2ply's
    sqrt(3) display factor on the scales.  The sphere is this module's icosphere, not ohm2ply's tessellation: the
    surfaces agree, the vertex lists do not.  Returns the number of ellipsoids written."""
    ellipsoids = extract_covariance_ellipsoids(gpu_map, extents=extents)
    write_ellipsoid_ply(file_name, ellipsoids, subdivisions)
    return len(ellipsoids)
