"""CPU restatement of the point clouds (include/ohmhip.h, "POINT CLOUDS") over OccupancyMap.chunks -- TEST
INFRASTRUCTURE.  The device cloud (ohmhip_map_cloud) is held to it at exact equality: count and every byte of the three
arrays.

Written from the reference's exporters (ohmtools/OhmCloud.cpp) rule by rule:
  OCCUPANCY  saveCloud :453-493, isOccupied / isFree ohm/VoxelOccupancy.h:161-164, positionSafe ohm/VoxelMean.h:47-54
  DENSITY    the rule of ohm/Density.h:34-55 and SaveDensityCloudOptions (the function as written never sets its
             voxels' key, :524-538, so its own output specifies nothing)
  TSDF       saveTsdfCloud :950-987, voxelCentreLocal
  CLEARANCE  saveClearanceCloud :879-947, occupancyType ohm/VoxelOccupancy.h:116-128
  extents    OccupancyMap::regionKey ohm/OccupancyMap.cpp:746-750, MapRegion.cpp:32-38
Order: regions ascending (rz, ry, rx), voxels ascending MapChunk index x + y * dx + z * dx * dy.
Arithmetic is numpy's IEEE fp32 / fp64, one operation per statement in the reference's order."""
import numpy as np

from heightmap_ref import point_to_region_coord

OCCUPANCY, DENSITY, TSDF, CLEARANCE = range(4)
INF32 = np.float32(np.inf)
GPU_KEY = np.dtype([("region", "<i2", (3,)), ("voxel", "u1", (4,))])
assert GPU_KEY.itemsize == 10  # ohmgpu/GpuKey.h:37-46

#: what a voxel of a block the chunk does not hold reads (ohm/DefaultLayer.cpp: occupancy +inf, clearance -1, else 0)
_CLEARED = {"occupancy": (np.float32, 1, np.inf), "mean": (np.uint32, 2, 0), "traversal": (np.float32, 1, 0.0),
            "tsdf": (np.float32, 2, 0.0), "clearance": (np.float32, 1, -1.0)}


class Params:
    def __init__(self, mode=OCCUPANCY, export_free=False, ignore_voxel_mean=False, density_threshold=0.0,
                 surface_distance=float("inf"), colour_range=0.0, export_type=0, extents=None):
        self.mode = int(mode)
        self.export_free = bool(export_free)
        self.ignore_voxel_mean = bool(ignore_voxel_mean)
        self.density_threshold = np.float32(density_threshold)
        self.surface_distance = np.float32(surface_distance)
        self.colour_range = np.float32(colour_range)
        self.export_type = int(export_type)
        self.extents = extents

    def kwargs(self):
        """The same request as keyword arguments of ohm_amd.extract_cloud."""
        return dict(mode=self.mode, export_free=self.export_free, ignore_voxel_mean=self.ignore_voxel_mean,
                    density_threshold=float(self.density_threshold), surface_distance=float(self.surface_distance),
                    colour_range=float(self.colour_range), export_type=self.export_type, extents=self.extents)


class Cloud:
    def __init__(self, positions, keys, values, considered):
        self.positions = positions
        self.keys = keys
        self.values = values
        self.count = positions.shape[0]
        self.considered = considered  # voxels of the regions that took part


def voxel_centres(region, dim, resolution, origin):
    """OccupancyMap::voxelCentre (ohm/OccupancyMap.h:757-778) of every voxel of `region`, in MapChunk order: (n, 3)."""
    n = dim[0] * dim[1] * dim[2]
    index = np.arange(n, dtype=np.int64)
    local = np.stack([index % dim[0], (index // dim[0]) % dim[1], index // (dim[0] * dim[1])], axis=1)
    out = np.empty((n, 3), dtype=np.float64)
    for a in range(3):
        region_dim = dim[a] * float(resolution)  # regionSpatialResolution (ohm/OccupancyMap.cpp:200-202)
        v = np.full(n, np.float64(np.float32(region[a])))
        v = v * region_dim
        v = v - 0.5 * region_dim
        v = v + float(origin[a])
        v = v + local[:, a].astype(np.float64) * float(resolution)
        v = v + 0.5 * float(resolution)
        out[:, a] = v
    return out, local


def sub_voxel_to_local(coord, resolution):
    """subVoxelToLocalCoord (ohm/VoxelMeanCompute.h:102-122) of an array of patterns: (n, 3).  Always decodes."""
    coord = np.asarray(coord, dtype=np.uint32)
    mean_resolution = float(resolution) / 1023.0
    offset = float(np.float32(0.5)) * float(resolution)
    out = np.empty(coord.shape + (3,), dtype=np.float64)
    for a in range(3):
        out[..., a] = ((coord >> np.uint32(10 * a)) & np.uint32(1023)).astype(np.float64) * mean_resolution - offset
    return out


def region_key(point, origin, dim, resolution):
    """OccupancyMap::regionKey: MapRegion's quantisation, stored in an int16."""
    out = []
    for a in range(3):
        coord = point_to_region_coord(float(point[a]) - float(origin[a]), dim[a] * float(resolution))
        out.append(((coord + 32768) & 0xffff) - 32768)
    return tuple(out)


def _block(chunk, name, n):
    dtype, comps, cleared = _CLEARED[name]
    block = chunk.get(name)
    if block is None:
        return np.full((n, comps) if comps > 1 else n, cleared, dtype=dtype)
    return np.asarray(block, dtype=dtype).reshape((n, comps) if comps > 1 else n)


def extract(chunks, resolution, dim, origin, threshold, layers, p):
    """The cloud of a map with `layers` whose regions are `chunks` ({region: {layer: block}})."""
    dim = tuple(int(d) for d in dim)
    n = dim[0] * dim[1] * dim[2]
    layers = set(layers)
    needs = {OCCUPANCY: {"occupancy"}, DENSITY: {"traversal", "mean"}, TSDF: {"tsdf"},
             CLEARANCE: {"occupancy", "clearance"}}[p.mode]
    empty = Cloud(np.zeros((0, 3)), np.zeros(0, dtype=GPU_KEY), np.zeros(0, dtype=np.float32), 0)
    if not needs <= layers:
        return empty
    regions = sorted((tuple(int(v) for v in r) for r in chunks), key=lambda r: (r[2], r[1], r[0]))
    if p.extents is not None:
        lo = region_key(p.extents[0], origin, dim, resolution)
        hi = region_key(p.extents[1], origin, dim, resolution)
        regions = [r for r in regions if all(lo[a] <= r[a] <= hi[a] for a in range(3))]
    threshold = np.float32(threshold)
    use_mean = "mean" in layers and not p.ignore_voxel_mean and p.mode in (OCCUPANCY, DENSITY)
    local_positions = p.mode in (TSDF, CLEARANCE)
    positions, keys, values = [], [], []
    with np.errstate(all="ignore"):
        for r in regions:
            c = chunks[r]
            if p.mode == OCCUPANCY:
                v = _block(c, "occupancy", n)
                occupied = (v != INF32) & (v >= threshold)
                free = (v != INF32) & (v < threshold)
                keep = occupied | (free if p.export_free else np.zeros(n, dtype=bool))
                value = v
            elif p.mode == DENSITY:
                traversal = _block(c, "traversal", n)
                count = _block(c, "mean", n)[:, 1]
                ratio = count.astype(np.float32) / traversal
                value = np.where(count > 0, np.where(traversal > 0, ratio, INF32), np.float32(0)).astype(np.float32)
                keep = value >= p.density_threshold
            elif p.mode == TSDF:
                t = _block(c, "tsdf", n)
                keep = (t[:, 0] > 0) & (np.abs(t[:, 1]) < p.surface_distance)
                value = t[:, 1]
            else:
                v = _block(c, "occupancy", n)
                occupancy_type = np.where(v < INF32, np.where(v < threshold, 0, 1), -1)
                rng = _block(c, "clearance", n)
                rng = np.where(rng < 0, p.colour_range, rng).astype(np.float32)
                keep = (occupancy_type >= p.export_type) & (rng >= 0)
                value = rng
            if not keep.any():
                continue
            centre, local = voxel_centres(r, dim, resolution, (0.0, 0.0, 0.0) if local_positions else origin)
            pos = centre[keep]
            if use_mean:
                pos = pos + sub_voxel_to_local(_block(c, "mean", n)[:, 0][keep], resolution)
            k = np.zeros(int(keep.sum()), dtype=GPU_KEY)
            k["region"] = r
            k["voxel"][:, :3] = local[keep]
            positions.append(pos)
            keys.append(k)
            values.append(np.ascontiguousarray(value[keep], dtype=np.float32))
    considered = n * len(regions)
    if not positions:
        empty.considered = considered
        return empty
    return Cloud(np.concatenate(positions), np.concatenate(keys), np.concatenate(values), considered)


def extract_map(map_, p, chunks=None):
    """extract() of an ohm_amd.OccupancyMap (its chunks as synced, or `chunks`)."""
    return extract(chunks if chunks is not None else map_.chunks, map_.resolution, map_.region_voxel_dimensions,
                   map_.origin, map_.occupancy_threshold_value, map_.layers, p)
