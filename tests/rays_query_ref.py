"""CPU restatement of ohm::RaysQuery::onExecute (ohm/RaysQuery.cpp:102-203) over the oracle's line walk -- TEST
INFRASTRUCTURE.  The device query (ohmhip_map_rays_query) is held to it at exact equality.

Per ray, in input order: the map's built-in ray filter (ohm/RayFilter.cpp, as oracle/ohm_oracle.c applies it); then
walkSegmentKeys with flags 0 (OracleMap.walk: keys and the fp64 enter / exit ranges); per visited voxel the visit
lambda's arithmetic, in its order, stopping after the first occupied voxel.  Range and volume restart at 0 for every
ray; the terminal type and key do not (they are declared outside the ray loop, :116-117): a ray that passes the filter
but visits no voxel repeats those of the last ray that did."""
import math

import numpy as np

K_NULL, K_UNOBSERVED, K_FREE, K_OCCUPIED = -2, -1, 0, 1
NULL_KEY = ((-32768, -32768, -32768), (0, 0, 0))  # Key::kNull (ohm/Key.cpp:14)


def filter_ray(ray_filter, start, end):
    """goodRayFilter / clipRayFilter (ohm/RayFilter.cpp:12-58): (passed, start, end) with the end possibly clipped."""
    mode, rng = ray_filter if ray_filter else ("none", 0.0)
    if mode == "none":
        return True, start, end
    good = all(math.isfinite(v) for v in start) and all(math.isfinite(v) for v in end)
    rx, ry, rz = end[0] - start[0], end[1] - start[1], end[2] - start[2]
    len2 = (rx * rx + ry * ry) + rz * rz
    if mode == "good":
        return good and (rng <= 0 or len2 <= rng * rng), start, end
    if good and rng > 0 and len2 > rng * rng:
        length = math.sqrt(len2)
        end = (start[0] + (rx / length) * rng, start[1] + (ry / length) * rng, start[2] + (rz / length) * rng)
    return good, start, end


class OracleBlocks:
    """Occupancy blocks of an OracleMap by region key (None: no such region), cached."""

    def __init__(self, om):
        self._om = om
        self._cache = {}

    def __call__(self, region):
        if region not in self._cache:
            self._cache[region] = self._om.region_layer(region, "occupancy")
        return self._cache[region]


class ChunkBlocks:
    """Occupancy blocks of a {region: {layer: block}} dict (an OccupancyMap's chunks after syncVoxels)."""

    def __init__(self, chunks):
        self._chunks = chunks

    def __call__(self, region):
        c = self._chunks.get(tuple(int(v) for v in region))
        return None if c is None or "occupancy" not in c else np.asarray(c["occupancy"], dtype=np.float32)


def rays_query(om, rays, threshold_value, volume_coefficient=1.0, ray_filter=("good", 1e10), blocks=None):
    """om: the OracleMap whose geometry the walk uses; blocks: region key -> flat float32 occupancy block or None
    (default: om's own).  Returns (ranges f64, volumes f64, types i8, regions (N, 3) i16, locals (N, 3) u8) and the
    number of voxels visited."""
    rays = np.asarray(rays, dtype=np.float64).reshape(-1, 3)
    n = rays.shape[0] // 2
    blocks = blocks or OracleBlocks(om)
    dx, dy, _ = om.region_dim
    threshold = np.float32(threshold_value)
    coef = float(volume_coefficient)
    ranges = np.zeros(n, dtype=np.float64)
    volumes = np.zeros(n, dtype=np.float64)
    types = np.zeros(n, dtype=np.int8)
    regions = np.zeros((n, 3), dtype=np.int16)
    locals_ = np.zeros((n, 3), dtype=np.uint8)
    terminal_type, terminal_key = K_NULL, NULL_KEY
    visits = 0
    for i in range(n):
        start = tuple(float(v) for v in rays[2 * i])
        end = tuple(float(v) for v in rays[2 * i + 1])
        volume = 0.0
        rng = np.float32(0.0)
        passed, start, end = filter_ray(ray_filter, start, end)
        if not passed:
            ranges[i], volumes[i], types[i] = 0.0, 0.0, K_NULL
            regions[i], locals_[i] = NULL_KEY
            continue
        length = math.sqrt(sum((e - s) ** 2 for s, e in zip(start, end)))
        # (a walk visits at most |dx| + |dy| + |dz| + 1 voxels; rays whose keys are null visit none)
        cap = min(int(length / om.resolution * 1.7320508075688772) + 16, 1 << 20) if math.isfinite(length) else 16
        keys, enter, exit_ = om.walk(start, end, 0, cap=cap)
        for key, t0, t1 in zip(keys, enter, exit_):
            visits += 1
            block = blocks(key[0])
            lx, ly, lz = key[1]
            v = np.float32(np.inf) if block is None else block[lx + ly * dx + lz * dx * dy]
            is_unobserved = v == np.float32(np.inf)
            is_occupied = (not is_unobserved) and v > threshold
            volume += (coef * (t1 * t1 * t1 - t0 * t0 * t0)) if is_unobserved else 0.0
            rng = rng if is_occupied else np.float32(t1)
            terminal_type = K_UNOBSERVED if is_unobserved else (K_OCCUPIED if is_occupied else K_FREE)
            terminal_key = key
            if is_occupied:
                break
        ranges[i], volumes[i], types[i] = float(rng), volume, terminal_type
        regions[i], locals_[i] = terminal_key
    return (ranges, volumes, types, regions, locals_), visits
