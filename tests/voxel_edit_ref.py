"""The model of the voxel edits by key (test infrastructure; include/ohmhip.h, VOXEL EDITS): tests/test_voxel_edit_ref.py
(CPU) ties it to the oracle, tests/test_gpu_voxel_edit.py (-m gpu) holds the device to it on uint32 views.

apply() is the sequential Voxel API: element by element in input order on numpy region blocks,
  SET         the voxel's bytes of one layer become the value (E2),
  HIT / MISS  occupancy_ref.adjust_hit / adjust_miss with flags = 0 -- occupancyAdjustHit / Miss with the argument lists
              of ohm/VoxelOccupancy.h:63-65 and :94-96 (E3),
  HIT_SAMPLE  HIT on voxelKey(point); then, where the map has a mean layer, mean_ref.update_ref's coordinate with the
              SATURATING count of ohm/VoxelMean.h:162, min(count, 0xfffffffe) + 1 (E4),
a null key or a point without a key skipped and counted (E7), a region the blocks do not hold created cleared (E5).
The one mutant, "zero_length_ray", is the shortcut the issue rules out: HIT_SAMPLE as the ray mapper's sample update,
whose count wraps at 2^32.

key_range() restates ohm::KeyRange's order (ohm/KeyRange.cpp:105-129): x fastest, then y, then z."""
from collections import namedtuple

import numpy as np

import mean_ref as M
import occupancy_ref as O

SET, HIT, MISS, HIT_SAMPLE = 0, 1, 2, 3
NULL_REGION = (-32768, -32768, -32768)
LAYER_SHAPES = {"occupancy": (np.float32, 1), "mean": (np.uint32, 2), "covariance": (np.float32, 6),
                "traversal": (np.float32, 1), "touch_time": (np.uint32, 1), "incident_normal": (np.uint32, 1),
                "intensity": (np.float32, 2), "hit_miss_count": (np.uint32, 2), "tsdf": (np.float32, 2),
                "clearance": (np.float32, 1)}
CLEAR = {"occupancy": np.float32(np.inf), "clearance": np.float32(-1.0)}

Geometry = namedtuple("Geometry", "res dim origin layers")          # dim: voxels per region per axis; layers: names
Element = namedtuple("Element", "op key point layer value", defaults=(None, None, None, None))


def geometry(res, dim, layers=("occupancy",), origin=(0.0, 0.0, 0.0)):
    dim = (dim,) * 3 if np.isscalar(dim) else tuple(int(d) for d in dim)
    return Geometry(float(res), dim, tuple(float(v) for v in origin), tuple(layers))


def volume(geo):
    return geo.dim[0] * geo.dim[1] * geo.dim[2]


def voxel_index(geo, local):
    return int(local[0]) + geo.dim[0] * (int(local[1]) + geo.dim[1] * int(local[2]))


def clear_block(geo, name):
    dtype, comps = LAYER_SHAPES[name]
    return np.full(volume(geo) * comps, CLEAR.get(name, 0), dtype=dtype)


def _region_voxel(coord, res, region_res):
    """ohm/MapCoord.h:45-80"""
    eps = float(np.float32(1e-6))
    if -eps <= coord < 0:
        coord = 0.0
    elif coord >= region_res and coord - eps < region_res:
        coord -= eps
    return M.host_int(M._floor(coord / res))


def voxel_key(geo, point):
    """OccupancyMap::voxelKey (ohm/OccupancyMap.cpp:859-886): (region, local), or None where the reference hands out
    Key::kNull."""
    region, local = [], []
    for a in range(3):
        rd = geo.dim[a] * geo.res
        p = float(point[a]) - geo.origin[a]
        coord = M.host_int(M._floor(p / rd + 0.5))
        if not -32768 <= coord <= 32767:
            return None
        q = _region_voxel(p - (coord * rd - 0.5 * rd), geo.res, rd)
        if not 0 <= q < geo.dim[a]:
            return None
        region.append(coord)
        local.append(q)
    return tuple(region), tuple(local)


def voxel_centre(geo, key):
    return tuple(M.centre_ref(geo.origin[a], geo.dim[a] * geo.res, geo.res, key[0][a], key[1][a]) for a in range(3))


def sample_update(coord, count, point, centre, res, mutant=None):
    """updatePosition (ohm/VoxelMean.h:158-163)."""
    new_coord, wrapped = M.update_ref(int(coord), int(count), point, centre, res)
    return new_coord, wrapped if mutant == "zero_length_ray" else min(int(count), 0xfffffffe) + 1


def apply(blocks, geo, cfg, elements, mutant=None):
    """The elements, in order, on blocks = {region: {layer name: flat array}} (changed in place; regions are added).
    Returns the stats of ohmhip_voxel_edit_stats as a dict."""
    held = set(blocks)
    voxels, regions, null_keys, applied = set(), set(), 0, 0
    for e in elements:
        key = e.key if e.point is None else voxel_key(geo, e.point)
        if key is None or tuple(key[0]) == NULL_REGION:
            null_keys += 1
            continue
        region, local = tuple(int(v) for v in key[0]), tuple(int(v) for v in key[1])
        if region not in blocks:
            blocks[region] = {name: clear_block(geo, name) for name in geo.layers}
        layers = blocks[region]
        vi = voxel_index(geo, local)
        if e.op == SET:
            dtype, comps = LAYER_SHAPES[e.layer]
            layers[e.layer][vi * comps:(vi + 1) * comps] = np.asarray(e.value, dtype=dtype).reshape(comps)
        else:
            occ = layers["occupancy"]
            occ[vi] = O.adjust_miss(cfg, occ[vi]) if e.op == MISS else O.adjust_hit(cfg, occ[vi])
            if e.op == HIT_SAMPLE and "mean" in layers:
                assert e.point is not None
                mean = layers["mean"]
                mean[2 * vi], mean[2 * vi + 1] = sample_update(mean[2 * vi], mean[2 * vi + 1], e.point,
                                                               voxel_centre(geo, (region, local)), geo.res, mutant)
        applied += 1
        voxels.add((region, vi))
        regions.add(region)
    return {"applied": applied, "null_keys": null_keys, "distinct_voxels": len(voxels), "regions_touched": len(regions),
            "regions_created": len(regions - held)}


def key_range(geo, min_key, max_key):
    """[(region, local)] of the closed box, in KeyRange::walkNext's order."""
    lo = [min_key[0][a] * geo.dim[a] + min_key[1][a] for a in range(3)]
    hi = [max_key[0][a] * geo.dim[a] + max_key[1][a] for a in range(3)]
    out = []
    for z in range(lo[2], hi[2] + 1):
        for y in range(lo[1], hi[1] + 1):
            for x in range(lo[0], hi[0] + 1):
                g = (x, y, z)
                out.append((tuple(g[a] // geo.dim[a] for a in range(3)), tuple(g[a] % geo.dim[a] for a in range(3))))
    return out
