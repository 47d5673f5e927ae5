"""Python mirror of ohm/CopyUtil.h over ohmhip_map_copy (include/ohmhip.h, MAP COPY): canCopy, copyMap and the filter
helpers, on two GpuMaps.  The copy runs device to device in one kernel launch; nothing here touches voxel data.

A chunk filter is a callable on a ChunkView -- what a CopyChunkFilter sees of a MapChunk: `region.coord`, `region.centre`
(coord * region spatial dimensions, WITHOUT the map origin: ohm/MapRegion.cpp:40-42), `dirty` and
`map.region_spatial_dimensions`.  copyMap evaluates it over the source's regions on the host and passes the surviving
keys; copyFilterExtents and copyFilterDirty used alone go down as flags.  As in the reference an empty filter (None) is
an implied pass, which decides what copyFilterAnd / Or / Negate make of one (CopyUtil.h:50-91)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib as L
from .gpumap import LAYERS

Region = namedtuple("Region", "coord centre")
MapView = namedtuple("MapView", "region_spatial_dimensions")
ChunkView = namedtuple("ChunkView", "region dirty map")

_LAYER_NAMES = {lid: name for name, (lid, _, _) in LAYERS.items()}


def region_spatial_dimensions(map_):
    """OccupancyMap::regionSpatialResolution (ohm/OccupancyMap.cpp:200-202): voxels per axis * resolution, in double."""
    return tuple(float(d) * float(map_.resolution) for d in map_.region_voxel_dimensions)


def chunk_view(coord, spatial, dirty=False):
    """The ChunkView of region `coord` of a map whose regions measure `spatial`."""
    coord = tuple(int(c) for c in coord)
    return ChunkView(Region(coord, tuple(float(c) * s for c, s in zip(coord, spatial))), bool(dirty), MapView(tuple(spatial)))


class _ExtentsFilter:
    """copyFilterExtents (CopyUtil.cpp:37-45) in its operation order."""

    def __init__(self, min_ext, max_ext):
        self.min_ext = tuple(float(v) for v in min_ext)
        self.max_ext = tuple(float(v) for v in max_ext)

    def __call__(self, chunk):
        below = above = False
        for a in range(3):
            half = 0.5 * chunk.map.region_spatial_dimensions[a]
            lo = chunk.region.centre[a] - half
            hi = chunk.region.centre[a] + half
            below = below or hi < self.min_ext[a]
            above = above or lo > self.max_ext[a]
        return not below and not above


class _DirtyFilter:
    """In the place of copyFilterStamp (CopyUtil.cpp:47-50): changed since the last syncVoxels() / clear_dirty."""

    def __call__(self, chunk):
        return bool(chunk.dirty)


def copyFilterExtents(min_ext, max_ext):
    return _ExtentsFilter(min_ext, max_ext)


def copyFilterDirty():
    return _DirtyFilter()


def copyFilterAnd(filter_a, filter_b):
    """CopyUtil.h:50-57: with an empty operand, the other one (empty when both are)."""
    if filter_a is None or filter_b is None:
        return filter_a if filter_a is not None else filter_b
    return lambda chunk: filter_a(chunk) and filter_b(chunk)


def copyFilterOr(filter_a, filter_b):
    """CopyUtil.h:67-75: an empty operand is an implied pass, so the result is empty."""
    if filter_a is None or filter_b is None:
        return None
    return lambda chunk: filter_a(chunk) or filter_b(chunk)


def copyFilterNegate(filter_):
    """CopyUtil.h:81-91 and :107-117, for chunk and layer filters alike: the negation of an empty filter passes nothing."""
    if filter_ is not None:
        return lambda subject: not filter_(subject)
    return lambda subject: False


def copyLayersFilter(layers):
    """CopyUtil.h:96-101"""
    layers = list(layers)
    return lambda layer_name: layer_name in layers


def canCopy(dst, src):
    """ohm::canCopy (CopyUtil.cpp:52-56)."""
    return L.lib.ohmhip_map_can_copy(dst._handle, src._handle) == L.OK


def _layer_mask(dst, src, copy_layer_filter):
    """(common layer bits, the mask to pass): the filter judged on the SOURCE layer's name (CopyUtil.cpp:86-100)."""
    common = dst._layer_bits & src._layer_bits
    if copy_layer_filter is None:
        return common, 0
    mask = 0
    for lid in range(L.LID_COUNT):
        if (common >> lid) & 1 and copy_layer_filter(_LAYER_NAMES[lid]):
            mask |= 1 << lid
    if mask == 0:
        # every common layer is filtered out: the regions are still created (:117-126).  A mask of 0 means "all" in the
        # C ABI, so the request is spelt with layers that are not common.
        mask = ((1 << L.LID_COUNT) - 1) & ~common
        if mask == 0:
            raise L.OhmHipError(L.ERR_UNSUPPORTED, "copyMap: two maps with every layer and a filter that passes none")
    return common, mask


def copyMap(dst, src, copy_chunk_filter=None, copy_layer_filter=None):
    """ohm::copyMap (CopyUtil.cpp:58-165) from GpuMap `src` into GpuMap `dst`.  False where the reference returns false
    (canCopy fails, no layer in common); errors of the device call (OHMHIP_ERR_CAPACITY under dst's memory limit,
    OHMHIP_ERR_UNSUPPORTED for partitioned or merging maps) raise OhmHipError.  dst.lastCopyStats() holds the call's
    ohmhip_copy_stats."""
    dst._last_copy_stats = {name: 0 for name, _ in L.CopyStats._fields_}
    if not canCopy(dst, src):
        return False
    common, mask = _layer_mask(dst, src, copy_layer_filter)
    if common == 0:
        return False
    params = L.CopyParams()
    params.layers = mask
    keys = None
    if isinstance(copy_chunk_filter, _ExtentsFilter):
        params.flags = L.COPY_USE_EXTENTS
        for a in range(3):
            params.min_extents[a] = copy_chunk_filter.min_ext[a]
            params.max_extents[a] = copy_chunk_filter.max_ext[a]
    elif isinstance(copy_chunk_filter, _DirtyFilter):
        params.flags = L.COPY_DIRTY_ONLY
    elif copy_chunk_filter is not None:
        spatial = region_spatial_dimensions(src.map())
        dirty = set(tuple(int(v) for v in k) for k in src.regionKeys(dirty_only=True))
        keep = [tuple(int(v) for v in k) for k in src.regionKeys()]
        keep = [k for k in keep if copy_chunk_filter(chunk_view(k, spatial, k in dirty))]
        if not keep:
            return True  # (every chunk excluded: CopyUtil.cpp:117-123 visits none)
        keys = np.ascontiguousarray(keep, dtype=np.int16).reshape(-1, 3)
        params.keys_xyz = keys.ctypes.data
        params.key_count = len(keys)
    stats = L.CopyStats()
    status = L.lib.ohmhip_map_copy(dst._handle, src._handle, C.byref(params), C.byref(stats))
    dst._last_copy_stats = {name: int(getattr(stats, name)) for name, _ in L.CopyStats._fields_}
    if status == L.ERR_NOT_FOUND:
        return False
    L.check(status, "copyMap")
    return True
