"""CPU restatement of ohm::NearestNeighbours (ohm/NearestNeighbours.cpp:35-181, 240-284) and of the voxel reads by key
(include/ohmhip.h, "POINT QUERIES") over {region: occupancy block} -- TEST INFRASTRUCTURE.  The device query
(ohmhip_map_nearest_neighbours) is held to it at exact equality: counts, keys, the bits of every range, and the order.

Per near point, as the CPU writes it:
  regions   regionKey(near - r) <= key <= regionKey(near + r) per axis (:251-263), r the float radius widened to double;
            visited ascending z, then y, then x (ohm/private/OccupancyQueryAlg.h:47-58); voxels in MapChunk order
  obstructs v == +inf ? kQfUnknownAsOccupied : v >= threshold (:78-85: a NaN never); a region the map does not hold:
            nothing without the flag, every voxel with it (:54-69)
  range     q = vec3(near - origin), a double subtract then narrowed; d = vec3(voxelCentreLocal(key)) - q;
            r2 = (d.x * d.x + d.y * d.y) + d.z * d.z in float32; passes when r2 <= radius * radius; range sqrt(r2) (:108-114)
  nearest   kQfNearestResult: the first result whose r2 is strictly smaller than every earlier one (:116-120, ClosestResult
            starts at DBL_MAX, ohm/private/QueryDetail.h:39-43)
Arithmetic is numpy's IEEE fp32 / fp64, one operation per statement in the reference's order."""
import numpy as np

from clearance_ref import centre
from cloud_ref import GPU_KEY, region_key, voxel_centres

QF_UNKNOWN_AS_OCCUPIED = 1 << 0
QF_NEAREST_RESULT = 1 << 1
INF32 = np.float32(np.inf)
NULL_KEY = np.zeros(1, dtype=GPU_KEY)
NULL_KEY["region"] = -32768  # Key::kNull (ohm/Key.cpp:14)

_CENTRES = {}


def local_centres(region, dim, resolution):
    """glm::vec3(voxelCentreLocal(key)) of every voxel of `region` in MapChunk order: ((n, 3) float32, (n, 3) locals)."""
    key = (tuple(int(v) for v in region), tuple(int(d) for d in dim), float(resolution))
    if key not in _CENTRES:
        c, local = voxel_centres(key[0], key[1], key[2], (0.0, 0.0, 0.0))
        _CENTRES[key] = (c.astype(np.float32), local.astype(np.uint8))
    return _CENTRES[key]


def obstructs(values, threshold, unknown_as_occupied):
    values = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(values == INF32, bool(unknown_as_occupied), values >= np.float32(threshold))


def query_regions(point, radius, origin, dim, resolution):
    """The regions of one query in visiting order."""
    r = float(np.float32(radius))
    lo = region_key([float(point[a]) - r for a in range(3)], origin, dim, resolution)
    hi = region_key([float(point[a]) + r for a in range(3)], origin, dim, resolution)
    return [(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1) for x in range(lo[0], hi[0] + 1)]


def nearest_neighbours(blocks, resolution, dim, origin, threshold, points, radius, flags=0):
    """blocks: {region: flat float32 occupancy block}.  Returns (counts (Q,) uint64, keys GPU_KEY, ranges float32)."""
    dim = tuple(int(d) for d in dim)
    n = dim[0] * dim[1] * dim[2]
    blocks = {tuple(int(v) for v in k): np.asarray(b, dtype=np.float32).reshape(-1) for k, b in blocks.items()}
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    radius = np.float32(radius)
    radius2 = radius * radius
    uao = bool(flags & QF_UNKNOWN_AS_OCCUPIED)
    counts = np.zeros(points.shape[0], dtype=np.uint64)
    all_keys, all_ranges = [], []
    for qi, point in enumerate(points):
        q = np.array([np.float32(float(point[a]) - float(origin[a])) for a in range(3)], dtype=np.float32)
        keys, r2s = [], []
        for region in query_regions(point, radius, origin, dim, resolution):
            block = blocks.get(region)
            if block is None:
                if not uao:
                    continue
                candidate = np.ones(n, dtype=bool)
            else:
                assert block.size == n
                candidate = obstructs(block, threshold, uao)
            if not candidate.any():
                continue
            c, local = local_centres(region, dim, resolution)
            d = c[candidate] - q[None, :]
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            assert r2.dtype == np.float32
            passed = r2 <= radius2
            k = np.zeros(int(passed.sum()), dtype=GPU_KEY)
            k["region"] = region
            k["voxel"][:, :3] = local[candidate][passed]
            keys.append(k)
            r2s.append(r2[passed])
        if not keys:
            continue
        keys, r2s = np.concatenate(keys), np.concatenate(r2s)
        if (flags & QF_NEAREST_RESULT) and keys.size:
            first = int(np.argmin(r2s))  # the first of the smallest: strict `<` over the visiting order
            keys, r2s = keys[first:first + 1], r2s[first:first + 1]
        counts[qi] = keys.size
        all_keys.append(keys)
        all_ranges.append(np.sqrt(r2s).astype(np.float32))
    if not all_keys:
        return counts, np.zeros(0, dtype=GPU_KEY), np.zeros(0, dtype=np.float32)
    return counts, np.concatenate(all_keys), np.concatenate(all_ranges)


def occupancy_types(values, present, threshold):
    """kNull (-2) when not present, else occupancyType (ohm/VoxelOccupancy.h:116-128): a NaN is unobserved."""
    values = np.asarray(values, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        types = np.where(values < INF32, np.where(values < np.float32(threshold), 0, 1), -1)
    return np.where(np.asarray(present, dtype=bool), types, -2).astype(np.int8)


__all__ = ["nearest_neighbours", "occupancy_types", "query_regions", "local_centres", "obstructs", "centre", "GPU_KEY",
           "QF_UNKNOWN_AS_OCCUPIED", "QF_NEAREST_RESULT", "NULL_KEY"]
