"""CPU restatement of what ohm::copyMap selects (test infrastructure): C2 and C3 of include/ohmhip.h, MAP COPY, written
from ohm/CopyUtil.cpp:37-126 and held to hand-derived cases by tests/test_copy_ref.py.  The device tests
(tests/test_gpu_copy.py) predict ohmhip_copy_stats and the copied set with it.

Arithmetic is IEEE double in the reference's operation order (Python floats):
    half = 0.5 * region_spatial_dimensions          CopyUtil.cpp:40
    lo   = centre - half;  hi = centre + half       :41-42
    pass = not any(hi < min_ext) and not any(lo > max_ext)   :43
with centre = coord * region_spatial_dimensions (ohm/MapRegion.cpp:40-42 through ohm/MapCoord.h:37-40): the map origin
is NOT added, so on a map whose origin is not zero the box is relative to the origin.  `origin` is an argument of the
functions below only to say so: they do not use it."""

LAYER_IDS = {"occupancy": 0, "mean": 1, "covariance": 2, "traversal": 3, "touch_time": 4, "incident_normal": 5,
             "intensity": 6, "hit_miss_count": 7, "tsdf": 8, "clearance": 9}
LAYER_BYTES = {"occupancy": 4, "mean": 8, "covariance": 24, "traversal": 4, "touch_time": 4, "incident_normal": 4,
               "intensity": 8, "hit_miss_count": 8, "tsdf": 8, "clearance": 4}


def spatial_dimensions(resolution, region_voxel_dimensions):
    """ohm/OccupancyMap.cpp:200-202"""
    return tuple(float(d) * float(resolution) for d in region_voxel_dimensions)


def region_centre(coord, spatial, origin=(0.0, 0.0, 0.0)):
    return tuple(float(int(c)) * s for c, s in zip(coord, spatial))


def passes_extents(coord, spatial, min_ext, max_ext, origin=(0.0, 0.0, 0.0)):
    centre = region_centre(coord, spatial, origin)
    any_below = any_above = False
    for a in range(3):
        half = 0.5 * spatial[a]
        lo = centre[a] - half
        hi = centre[a] + half
        any_below = any_below or hi < min_ext[a]
        any_above = any_above or lo > max_ext[a]
    return (not any_below) and (not any_above)


def common_layers(src_layers, dst_layers):
    """calculateOverlappingLayerSet: the layers both maps hold, in layer-id order."""
    return sorted(set(src_layers) & set(dst_layers), key=LAYER_IDS.get)


def copied_layers(src_layers, dst_layers, layer_filter=None):
    """None: no layer in common, copyMap returns false (CopyUtil.cpp:78-82).  Else the common layers the filter passes,
    judged on the source layer's name (:86-100) -- possibly none, and the copy still creates the regions."""
    common = common_layers(src_layers, dst_layers)
    if not common:
        return None
    return [name for name in common if layer_filter is None or layer_filter(name)]


def select_regions(src_regions, spatial, keys=None, extents=None, dirty=None, origin=(0.0, 0.0, 0.0)):
    """(regions copied, keys absent).  src_regions: the source's region coordinates; keys: an optional list naming the
    candidates (one the source lacks is absent, a repeated one counts once); extents: optional (min_ext, max_ext); dirty:
    optional set of the source's changed regions (DIRTY_ONLY).  A region is copied when it passes every filter given."""
    have = set(tuple(int(v) for v in r) for r in src_regions)
    absent = 0
    if keys is None:
        candidates = sorted(have, key=lambda r: (r[2], r[1], r[0]))
    else:
        candidates, seen = [], set()
        for k in keys:
            k = tuple(int(v) for v in k)
            if k in seen:
                continue
            seen.add(k)
            if k in have:
                candidates.append(k)
            else:
                absent += 1
    passed = []
    for r in candidates:
        if dirty is not None and r not in dirty:
            continue
        if extents is not None and not passes_extents(r, spatial, extents[0], extents[1], origin):
            continue
        passed.append(r)
    return passed, absent


def predict_stats(src_regions, dst_regions, spatial, src_layers, dst_layers, region_voxels, layer_filter=None, keys=None,
                  extents=None, dirty=None, src_tiles_per_region=None, tiles_per_region=1):
    """ohmhip_copy_stats of a copy that succeeds.  bytes_copied counts the blocks that have a source: for a tiled map
    src_tiles_per_region[region] says how many of a region's tiles the source holds (default: all)."""
    layers = copied_layers(src_layers, dst_layers, layer_filter)
    passed, absent = select_regions(src_regions, spatial, keys, extents, dirty)
    held = set(tuple(int(v) for v in r) for r in dst_regions)
    per_voxel = sum(LAYER_BYTES[name] for name in layers)
    blocks = 0
    for r in passed:
        blocks += tiles_per_region if src_tiles_per_region is None else src_tiles_per_region[r]
    mask = 0
    for name in layers:
        mask |= 1 << LAYER_IDS[name]
    return {"regions_passed": len(passed), "regions_created": sum(1 for r in passed if r not in held),
            "keys_absent": absent, "bytes_copied": blocks * (region_voxels // tiles_per_region) * per_voxel,
            "layers_copied": mask if passed else 0}
