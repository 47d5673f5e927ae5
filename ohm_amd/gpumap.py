"""Host-side mirror (Python) of the reference interface for the ray-integration path.

Names, argument meaning and error behaviour follow the reference so the parity tests read like the reference's own
(tests/ohmtestgpu/GpuMapTest.cpp):

  ohm::OccupancyMap  (ohm/OccupancyMap.h:291)  -> OccupancyMap   : parameters + MapChunk/VoxelBlock-layout host blocks
  ohm::RayMapper     (ohm/RayMapper.h:22-65)   -> RayMapper
  ohm::GpuMap        (ohmgpu/GpuMap.h:143-384) -> GpuMap
  ohm::GpuNdtMap     (ohmgpu/GpuNdtMap.h:63)   -> GpuNdtMap
  ohm::GpuTsdfMap    (ohmgpu/GpuTsdfMap.h:37)  -> GpuTsdfMap

All compute goes through libohmhip.so (include/ohmhip.h).  There is no CPU implementation here.
The C++14 mirror of the same classes lives in ohm_amd/host/ (header-only, over the same C ABI).
"""
import ctypes as C
import enum
import math
import time

import numpy as np

from . import _lib as L
from . import rayfilter as _rayfilter


class RayFlag(enum.IntFlag):
    """ohm/RayFlag.h:16-60"""
    kRfDefault = 0
    kRfEndPointAsFree = 1 << 0
    kRfStopOnFirstOccupied = 1 << 1
    kRfExcludeOrigin = 1 << 2
    kRfExcludeSample = 1 << 3
    kRfExcludeRay = 1 << 4
    kRfExcludeUnobserved = 1 << 5
    kRfExcludeFree = 1 << 6
    kRfExcludeOccupied = 1 << 7
    kRfReverseWalk = 1 << 8


class OccupancyType(enum.IntEnum):
    """ohm::OccupancyType (ohm/OccupancyType.h:14-24): the terminal state RaysQuery reports per ray."""
    kNull = -2
    kUnobserved = -1
    kFree = 0
    kOccupied = 1


class QueryFlag(enum.IntFlag):
    """ohm::QueryFlag (ohm/QueryFlag.h:35-60), bit for bit."""
    kQfZero = 0
    kQfUnknownAsOccupied = 1 << 0
    kQfNearestResult = 1 << 1
    kQfGpuEvaluate = 1 << 2
    kQfNoCache = 1 << 3
    kQfReportUnscaledResults = 1 << 4
    kQfSpecialised = 1 << 16


class MappingProcessResult(enum.IntEnum):
    """ohm::MappingProcessResult (ohm/MappingProcess.h:18-24)."""
    kMprUpToDate = 0
    kMprProgressing = 1


def _clearance_params(search_radius, flags, axis_scaling):
    p = L.ClearanceParams()
    p.search_radius = float(search_radius)
    for i, v in enumerate(axis_scaling):
        p.axis_scaling[i] = float(v)
    p.flags = int(flags) & 0xffffffff
    return p


def _key_records(keys):
    """10-byte GpuKey records (N, 10) uint8 from such records or from a (regions (N, 3), locals (N, 3)) pair."""
    if isinstance(keys, tuple):
        regions = np.ascontiguousarray(keys[0], dtype=np.int16).reshape(-1, 3)
        locals_ = np.asarray(keys[1], dtype=np.uint8).reshape(-1, 3)
        rec = np.zeros((regions.shape[0], 10), dtype=np.uint8)
        rec[:, :6] = regions.view(np.uint8).reshape(-1, 6)
        rec[:, 6:9] = locals_
        return rec
    return np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 10)


#: ohm::GpuKey (ohmgpu/GpuKey.h:37-46), the record of ohm_amd.GPU_KEY_DTYPE
_GPU_KEY = np.dtype([("region", "<i2", (3,)), ("voxel", "u1", (4,))])


class VoxelEdit(enum.IntEnum):
    """OHMHIP_EDIT_*: what GpuMap.integrateVoxels does to a voxel."""
    kHit = L.EDIT_HIT               # ohm::integrateHit(map, key)
    kMiss = L.EDIT_MISS             # ohm::integrateMiss(map, key)
    kHitSample = L.EDIT_HIT_SAMPLE  # ohm::integrateHit(map, sample): points only


def key_range(min_key, max_key, region_voxel_dimensions):
    """The keys of ohm::KeyRange(min_key, max_key, region_voxel_dimensions) as GPU_KEY_DTYPE records, in the order
    KeyRange::walkNext visits them (ohm/KeyRange.cpp:105-129): x fastest, then y, then z, across region borders."""
    dims = np.asarray(region_voxel_dimensions, dtype=np.int64)
    lo = np.asarray(min_key["region"], dtype=np.int64) * dims + np.asarray(min_key["voxel"][:3], dtype=np.int64)
    hi = np.asarray(max_key["region"], dtype=np.int64) * dims + np.asarray(max_key["voxel"][:3], dtype=np.int64)
    if np.any(hi < lo):
        return np.zeros(0, dtype=_GPU_KEY)
    gz, gy, gx = np.meshgrid(*(np.arange(lo[a], hi[a] + 1) for a in (2, 1, 0)), indexing="ij")
    g = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    keys = np.zeros(g.shape[0], dtype=_GPU_KEY)
    keys["region"] = np.floor_divide(g, dims).astype(np.int16)
    keys["voxel"][:, :3] = np.mod(g, dims).astype(np.uint8)
    return keys


class NdtMode(enum.IntEnum):
    """ohm/NdtMode.h"""
    kNone = 0
    kOccupancy = 1
    kTraversability = 2


# Layer name -> (layer id, numpy dtype, components).  ohm/DefaultLayer.cpp:76-311
LAYERS = {
    "occupancy": (L.LID_OCCUPANCY, np.float32, 1),
    "mean": (L.LID_MEAN, np.uint32, 2),
    "covariance": (L.LID_COVARIANCE, np.float32, 6),
    "traversal": (L.LID_TRAVERSAL, np.float32, 1),
    "touch_time": (L.LID_TOUCH_TIME, np.uint32, 1),
    "incident_normal": (L.LID_INCIDENT, np.uint32, 1),
    "intensity": (L.LID_INTENSITY, np.float32, 2),
    "hit_miss_count": (L.LID_HIT_MISS, np.uint32, 2),
    "tsdf": (L.LID_TSDF, np.float32, 2),
    "clearance": (L.LID_CLEARANCE, np.float32, 1),
}


def layer_clear_block(name, region_voxels):
    """A region's block of layer `name` as a cleared MapChunk holds it (ohm/DefaultLayer.cpp: occupancy +inf, clearance
    -1, every other layer zero bytes)."""
    _, dtype, comps = LAYERS[name]
    value = {"occupancy": np.inf, "clearance": -1.0}.get(name, 0)
    return np.full(region_voxels * comps, value, dtype=dtype)


_libm = C.CDLL("libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]
_libm.expf.restype = C.c_float
_libm.expf.argtypes = [C.c_float]


def probability_to_value(p):
    """ohm/MapProbability.h:33-36, float instantiation: std::log(float) == libm logf (numpy's float32 log is not
    bit-identical to libm, and these constants must match the C++ host / CPU mapper exactly)."""
    p = np.float32(p)
    return np.float32(_libm.logf(float(p / (np.float32(1.0) - p))))


def value_to_probability(v):
    """ohm/MapProbability.h:20-27"""
    v = np.float32(v)
    if v == -np.inf:
        return np.float32(0)
    return np.float32(1) - (np.float32(1) / (np.float32(1) + np.float32(_libm.expf(float(v)))))


class OccupancyMap:
    """Host-side map description + chunk storage in the reference's MapChunk layout.

    chunks[(rx, ry, rz)][layer_name] is a flat numpy array indexed x + y*dx + z*dx*dy (ohm/MapChunk.h:33-50), i.e. the
    bytes of VoxelBlock::voxelBytes() for that layer (ohm/VoxelBlock.h:270-278).
    """

    def __init__(self, resolution=0.1, region_voxel_dimensions=(32, 32, 32), layers=("occupancy",)):
        self.resolution = float(resolution)
        self.region_voxel_dimensions = tuple(int(d) if d > 0 else 32 for d in region_voxel_dimensions)
        self.origin = (0.0, 0.0, 0.0)
        self.layers = list(layers)
        # ohm/OccupancyMap.cpp:205-213
        self.min_voxel_value = np.float32(-2.0)
        self.max_voxel_value = np.float32(3.511)
        self.hit_value = probability_to_value(0.9)
        self.miss_value = probability_to_value(0.45)
        self.occupancy_threshold_value = probability_to_value(0.5)
        self.saturate_at_min_value = False
        self.saturate_at_max_value = False
        self.ray_filter = ("good", 1e10)  # ohm/OccupancyMap.cpp:215-218
        self.chunks = {}

    # -- ohm::OccupancyMap setters used by the tests ---------------------------------------------------------------
    def setOrigin(self, origin):
        self.origin = tuple(float(v) for v in origin)

    def setHitProbability(self, p):
        self.hit_value = probability_to_value(p)

    def setMissProbability(self, p):
        self.miss_value = probability_to_value(p)

    def setOccupancyThresholdProbability(self, p):
        self.occupancy_threshold_value = probability_to_value(p)

    def setHitValue(self, value):
        """ohm/OccupancyMap.h:623: the log-odds adjustment of a hit, set directly."""
        self.hit_value = float(np.float32(value))

    def setMissValue(self, value):
        self.miss_value = float(np.float32(value))

    def hitValue(self):
        return self.hit_value

    def missValue(self):
        return self.miss_value

    def missProbability(self):
        return value_to_probability(self.miss_value)

    def regionVoxelVolume(self):
        d = self.region_voxel_dimensions
        return d[0] * d[1] * d[2]

    def addLayer(self, name):
        if name not in LAYERS:
            raise KeyError(name)
        if name not in self.layers:
            self.layers.append(name)

    def removeLayer(self, name):
        """The layout without layer `name` (MapLayout::removeLayer + OccupancyMap::updateLayout): the chunks lose its
        blocks."""
        if name not in LAYERS:
            raise KeyError(name)
        self.updateLayout([n for n in self.layers if n != name])

    def updateLayout(self, layers, preserve_map=True):
        """OccupancyMap::updateLayout (ohm/OccupancyMap.cpp:670-682) with MapChunk::updateLayout (ohm/MapChunk.cpp:
        93-143) for every chunk: the blocks of layers in both layouts stay, an added layer gets a block of its clear
        value (layer_clear_block), a removed layer's blocks go.  preserve_map=False drops the chunks instead."""
        layers = list(dict.fromkeys(layers))
        for name in layers:
            if name not in LAYERS:
                raise KeyError(name)
        if not preserve_map:
            self.chunks.clear()
        rv = self.regionVoxelVolume()
        for chunk in self.chunks.values():
            for name in [n for n in chunk if n not in layers]:
                del chunk[name]
            for name in layers:
                if name not in chunk:
                    chunk[name] = layer_clear_block(name, rv)
        self.layers[:] = layers

    def regionCount(self):
        return len(self.chunks)


class RayMapper:
    """ohm/RayMapper.h:22-65"""

    def valid(self):
        raise NotImplementedError

    def integrateRays(self, rays, intensities=None, timestamps=None, ray_update_flags=RayFlag.kRfDefault):
        raise NotImplementedError


class GpuMap(RayMapper):
    """ohm::GpuMap (ohmgpu/GpuMap.h:143-384) over libohmhip.so.

    integrateRays() is asynchronous like the reference (returns once the batch is queued); syncVoxels() is the fence
    and copies modified regions back into map.chunks.
    """
    _mode = L.MODE_OCCUPANCY

    def __init__(self, map_, borrowed_map=True, expected_element_count=2048, gpu_mem_size=0, region_capacity=0):
        self._map = map_
        self._borrowed = borrowed_map
        self._handle = L._vp()
        self._ok = False
        self._block_addr = {}  # layer name -> {region key: (block, address)}: syncVoxels' destination pointers
        self._ray_segment_length = 0.0
        self._configure_layers()
        cfg = L.MapConfig()
        L.lib.ohmhip_map_config_default(C.byref(cfg))
        cfg.resolution = map_.resolution
        for a in range(3):
            cfg.region_dim[a] = map_.region_voxel_dimensions[a]
            cfg.origin[a] = map_.origin[a]
        layer_bits = 0
        for name in map_.layers:
            layer_bits |= 1 << LAYERS[name][0]
        cfg.layers = layer_bits
        self._layer_bits = layer_bits
        cfg.mode = self._mode
        self._fill_map_values(cfg)
        cfg.gpu_mem_size = int(gpu_mem_size)
        cfg.region_capacity = int(region_capacity)
        self._fill_config(cfg)
        self._cfg = cfg
        status = L.lib.ohmhip_map_create(C.byref(self._handle), C.byref(cfg))
        # gputil::Exception from the ctor on allocation failure (ohmgpu/GpuMap.h:53-54,159-160)
        L.check(status, "GpuMap: ohmhip_map_create")
        self._ok = True
        if expected_element_count > 2048:
            # the reference sizes its ray / key buffers for expected_element_count points in the constructor
            # (ohmgpu/GpuMap.cpp:429-470); the default (2048) is left to the first batch
            # best effort: a reservation the device cannot hold is not an error, the batches grow their buffers on demand
            L.lib.ohmhip_map_reserve_rays(self._handle, int(expected_element_count) // 2)
        self._upload_existing()

    def _fill_map_values(self, cfg):
        """The host map's probabilities, clamps and built-in filter: re-read before every batch, like the reference,
        whose GpuMap takes them from the OccupancyMap at each launch (ohmgpu/GpuMap.cpp:1036-1191)."""
        map_ = self._map
        cfg.hit_value = float(map_.hit_value)
        cfg.miss_value = float(map_.miss_value)
        cfg.threshold_value = float(map_.occupancy_threshold_value)
        cfg.min_value = float(map_.min_voxel_value)
        cfg.max_value = float(map_.max_voxel_value)
        cfg.saturate_at_min = int(map_.saturate_at_min_value)
        cfg.saturate_at_max = int(map_.saturate_at_max_value)
        mode, rng = map_.ray_filter if map_.ray_filter else ("none", 0.0)
        cfg.ray_filter = {"none": L.FILTER_NONE, "good": L.FILTER_GOOD, "clip": L.FILTER_CLIP}[mode]
        cfg.ray_filter_range = float(rng)

    def _push_config_if_changed(self):
        now = L.MapConfig.from_buffer_copy(bytes(self._cfg))
        self._fill_map_values(now)
        self._fill_config(now)
        if bytes(now) != bytes(self._cfg):
            L.check(L.lib.ohmhip_map_update_config(self._handle, C.byref(now)), "update_config")
            self._cfg = now

    # hooks for subclasses ---------------------------------------------------------------------------------------
    def _configure_layers(self):
        if "occupancy" not in self._map.layers:
            self._map.addLayer("occupancy")

    def _fill_config(self, cfg):
        pass

    # ------------------------------------------------------------------------------------------------------------
    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self):
        if self._handle:
            L.lib.ohmhip_map_destroy(self._handle)
            self._handle = L._vp()
            self._ok = False

    def gpuOk(self):
        return self._ok

    def valid(self):
        return self._ok

    def map(self):
        return self._map

    def borrowedMap(self):
        return self._borrowed

    def hitValue(self):
        return self._map.hit_value

    def missValue(self):
        return self._map.miss_value

    def setHitValue(self, value):
        """Pass-through to OccupancyMap::setHitValue for API compatibility (ohmgpu/GpuMap.h:234-236); the device takes
        the new value with the next batch."""
        self._map.setHitValue(value)

    def setMissValue(self, value):
        """ohmgpu/GpuMap.h:242-244."""
        self._map.setMissValue(value)

    def setGroupedRays(self, group):
        """ohmgpu/GpuMap.h:271, 323: the reference can sort a batch's rays by region before upload to help its GPU
        threads.  Here every batch is binned per region on the device: the flag is stored and otherwise ignored."""
        self._grouped_rays = bool(group)

    def groupedRays(self):
        return getattr(self, "_grouped_rays", False)

    def setRaySegmentLength(self, length):
        """ohmgpu/GpuMap.h:246-262.  Segmentation exists in the reference to balance GPU threads; this backend bins
        rays per region instead, so the value is stored and otherwise ignored (results follow the CPU mapper)."""
        self._ray_segment_length = float(length)

    def raySegmentLength(self):
        return self._ray_segment_length

    # GpuMap::setRayFilter / rayFilter / effectiveRayFilter / clearRayFilter (ohmgpu/GpuMap.cpp:348-369).  A filter is a
    # callable of the vectorised form described in ohm_amd/rayfilter.py; without one the map's built-in filter
    # (OccupancyMap.ray_filter) runs on the device.
    # A rayfilter.DeviceRayFilter (RF.on_device(...): a chain of the stock filters) is set on the device instead: the map
    # evaluates it for every batch -- integrateRays, integrateRaysDevice, collected calls, patterns -- with no host pass
    # (include/ohmhip.h: ohmhip_map_set_ray_filter_stages).  Not on a partitioned map; RaysQueryGpu keeps the built-in
    # filter.
    def setRayFilter(self, ray_filter):
        if isinstance(ray_filter, _rayfilter.DeviceRayFilter):
            self._set_device_chain(ray_filter.stages)
            self._device_ray_filter = ray_filter
            self._ray_filter = None
            return
        if getattr(self, "_device_ray_filter", None) is not None:
            self._set_device_chain(())
        self._device_ray_filter = None
        self._ray_filter = ray_filter

    def _set_device_chain(self, stages):
        records = (L.RayFilterStage * max(len(stages), 1))()
        for record, stage in zip(records, stages):
            record.kind, record.reserved, record.range = stage.kind, 0, stage.range
            record.box_min[:] = [float(v) for v in stage.box.min]
            record.box_max[:] = [float(v) for v in stage.box.max]
        L.check(L.lib.ohmhip_map_set_ray_filter_stages(self._handle, records if stages else None, len(stages)),
                "set_ray_filter_stages")

    def rayFilter(self):
        device = getattr(self, "_device_ray_filter", None)
        return device if device is not None else getattr(self, "_ray_filter", None)

    def effectiveRayFilter(self):
        return self.rayFilter()

    def clearRayFilter(self):
        if getattr(self, "_device_ray_filter", None) is not None:
            self._set_device_chain(())
        self._device_ray_filter = None
        self._ray_filter = None

    def applyRayFilterDevice(self, d_rays_ptr, element_count, d_rays_out_ptr=None, d_flags_out_ptr=None):
        """applyRayFilter on arrays resident in HBM: raw device pointers to element_count dvec3 in and out and to one
        flag byte per ray (the outputs may be None).  Returns the number of rays kept."""
        done = C.c_size_t(0)
        L.check(L.lib.ohmhip_map_apply_ray_filter_device(self._handle, d_rays_ptr, element_count, d_rays_out_ptr,
                                                         d_flags_out_ptr, C.byref(done)), "apply_ray_filter_device")
        return int(done.value)

    def applyRayFilter(self, rays):
        """What the device chain does to `rays` ((2N, 3) origin / sample pairs) without touching the map: (keep, rays as
        the chain leaves them, RayFilterFlag bytes), every ray reported (ohmhip_map_apply_ray_filter)."""
        done = C.c_size_t(0)
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 3)
        n = rays.shape[0] // 2
        out = np.empty((2 * n, 3), dtype=np.float64)
        flags = np.empty(n, dtype=np.uint8)
        L.check(L.lib.ohmhip_map_apply_ray_filter(self._handle, rays.ctypes.data, rays.shape[0], out.ctypes.data,
                                                  flags.ctypes.data, C.byref(done)), "apply_ray_filter")
        keep = (flags & 1) == 0
        assert int(keep.sum()) == int(done.value)
        return keep, out, flags

    def integrateRays(self, rays, intensities=None, timestamps=None, ray_update_flags=RayFlag.kRfDefault):
        """rays: (2N, 3) float64 origin/sample pairs.  Returns number of POINTS integrated (2 per ray), 0 on failure
        (ohmgpu/GpuMap.cpp:416, 548-551, 874)."""
        if not self._ok:
            return 0
        self._push_config_if_changed()
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 3)
        element_count = rays.shape[0]
        if element_count < 2:
            return 0
        ints = None if intensities is None else np.ascontiguousarray(intensities, dtype=np.float32)
        ts = None if timestamps is None else np.ascontiguousarray(timestamps, dtype=np.float64)
        done = C.c_size_t(0)
        host_filter = getattr(self, "_ray_filter", None)  # (a DeviceRayFilter is the device's: nothing to do here)
        if host_filter is not None:
            # The reference runs the RayFilterFunction per ray on the host before upload (ohmgpu/GpuMap.cpp:736-746):
            # rejected rays are dropped, the others go on with their (possibly moved) end points and filter flags.
            if ts is not None and len(ts) and not getattr(self, "_time_base_checked", False):
                # The reference takes the map's time base from the first stamp of the call BEFORE it filters
                # (ohmgpu/GpuMap.cpp:593 against :736-746): the library only sees the kept rays' stamps, so a base still
                # unset is set here -- also by a call whose rays are all rejected.
                if self.firstRayTime() < 0:
                    self.setFirstRayTime(ts[0])
                self._time_base_checked = True
            keep, starts, ends, fflags = host_filter(rays[0::2].copy(), rays[1::2].copy())
            keep = np.asarray(keep, dtype=bool)
            n_keep = int(keep.sum())
            if n_keep == 0:
                return 0
            kept = np.empty((2 * n_keep, 3), dtype=np.float64)
            kept[0::2] = np.asarray(starts, dtype=np.float64)[keep]
            kept[1::2] = np.asarray(ends, dtype=np.float64)[keep]
            fflags = np.ascontiguousarray(np.asarray(fflags, dtype=np.uint8)[keep])
            ints = None if ints is None else np.ascontiguousarray(ints[keep])
            ts = None if ts is None else np.ascontiguousarray(ts[keep])
            status = L.lib.ohmhip_map_integrate_rays_filtered(
                self._handle, kept.ctypes.data, kept.shape[0], None if ints is None else ints.ctypes.data,
                None if ts is None else ts.ctypes.data, int(ray_update_flags), fflags.ctypes.data, C.byref(done))
            if status == L.ERR_UNSUPPORTED:
                raise L.OhmHipError(status, "GpuMap.integrateRays")
            if status != L.OK:
                self._last_error = status
                return 0
            return int(done.value)
        status = L.lib.ohmhip_map_integrate_rays(
            self._handle, rays.ctypes.data, element_count, None if ints is None else ints.ctypes.data,
            None if ts is None else ts.ctypes.data, int(ray_update_flags), C.byref(done))
        if status == L.ERR_UNSUPPORTED:
            raise L.OhmHipError(status, "GpuMap.integrateRays")
        if status != L.OK:
            self._last_error = status
            self._last_partial = int(done.value)  # leading elements a split batch did integrate (include/ohmhip.h)
            return 0
        return int(done.value)

    def lastPartialCount(self):
        """After a failed integrateRays: how many leading elements of that call WERE integrated (non-zero only when a
        batch over the residency limit was split and a later part still did not fit); do not present those again."""
        return getattr(self, "_last_partial", 0)

    def integrateRaysDevice(self, d_rays_ptr, element_count, ray_update_flags=RayFlag.kRfDefault, d_intensities=None,
                            d_timestamps=None):
        """Rays already resident in HBM (bench path): d_rays_ptr is a raw device pointer to element_count dvec3
        (d_intensities / d_timestamps: optional device pointers to one float / double per ray).  The arrays must be
        complete when the call is made (synchronise the stream that produced them): the map reads them on streams of its
        own."""
        done = C.c_size_t(0)
        status = L.lib.ohmhip_map_integrate_rays_device(self._handle, d_rays_ptr, element_count, d_intensities,
                                                        d_timestamps, int(ray_update_flags), C.byref(done))
        if status != L.OK:
            self._last_partial = int(done.value)
            raise L.OhmHipError(status, "GpuMap.integrateRaysDevice (%d leading elements integrated)" % done.value)
        return int(done.value)

    def stats(self):
        st = L.BatchStats()
        L.check(L.lib.ohmhip_map_last_stats(self._handle, C.byref(st)), "stats")
        return {name: getattr(st, name) for name, _ in L.BatchStats._fields_}

    def batchTimings(self, batches_back=0):
        """Device phase times (ms) of one of the last 32 batches: total, setup + bin, walk kernel, order + apply."""
        ms = (C.c_float * 4)()
        L.check(L.lib.ohmhip_map_batch_timings(self._handle, batches_back, ms), "batch_timings")
        return {"ms_total": ms[0], "ms_setup": ms[1], "ms_walk": ms[2], "ms_apply": ms[3]}

    def setFirstRayTime(self, time):
        """OccupancyMap::setFirstRayTime (ohm/OccupancyMap.h:346): the base the touch-time layer is encoded against.  The
        ranks of a partitioned map share one (PartitionedIntegrator sets it from the first stamp of the whole job)."""
        L.check(L.lib.ohmhip_map_set_first_ray_time(self._handle, float(time)), "set_first_ray_time")
        self._time_base_checked = False

    def firstRayTime(self):
        t = C.c_double(-1.0)
        L.check(L.lib.ohmhip_map_first_ray_time(self._handle, C.byref(t)), "first_ray_time")
        return float(t.value)

    def setPhaseTiming(self, enable=True):
        """Record the start markers of the set-up and binning passes too (ms_setup, and ms_total of a batch on its own as
        first kernel start -> last kernel end): a few microseconds per batch, off by default (include/ohmhip.h)."""
        L.check(L.lib.ohmhip_map_set_phase_timing(self._handle, 1 if enable else 0), "set_phase_timing")

    def batchesLaunched(self):
        """Device batches launched so far (calls that only collect their rays launch none)."""
        n = C.c_uint64(0)
        L.check(L.lib.ohmhip_map_batches_launched(self._handle, C.byref(n)), "batches_launched")
        return int(n.value)

    def pipelineCounts(self):
        """(device batches completed, those whose binning pass ran early on the front stream and stood) since the map
        was created (include/ohmhip.h: ohmhip_map_pipeline_counts).  Read only."""
        batches, early = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib.ohmhip_map_pipeline_counts(self._handle, C.byref(batches), C.byref(early)), "pipeline_counts")
        return int(batches.value), int(early.value)

    def orderCounts(self):
        """(regions ordered by bucket and rank, regions ordered by the bitonic network) by the per-region ordering step
        of plain occupancy batches since the map was created (include/ohmhip.h: ohmhip_map_order_counts).  Waits for
        the batches launched so far."""
        ranked, network = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib.ohmhip_map_order_counts(self._handle, C.byref(ranked), C.byref(network)), "order_counts")
        return int(ranked.value), int(network.value)

    def raysBeyondTiles(self):
        """Maps with regions above 32768 voxels: rays cut because a tile coordinate left the key range although the
        reference addresses the region (include/ohmhip.h: ohmhip_map_rays_beyond_tiles).  0 for ordinary regions."""
        n = C.c_uint64(0)
        L.check(L.lib.ohmhip_map_rays_beyond_tiles(self._handle, C.byref(n)), "rays_beyond_tiles")
        return int(n.value)

    def wait(self):
        L.check(L.lib.ohmhip_map_sync(self._handle), "sync")

    def gpuCache(self):
        """GpuMap::gpuCache(): the MapRegionCache face of the reference's GpuCache (flush / clear / remove) as a view of
        this map -- the whole map is resident, there is no separate cache object."""
        owner = self

        class _GpuCacheView:
            def flush(self):
                owner.syncVoxels()

            def clear(self):
                owner.clear()

            def remove(self, region_key):
                owner.removeRegions([region_key])

            def reinitialise(self):
                """ohmgpu/GpuCache.h:103: the device map keeps its layout for life, so this is clear()."""
                owner.clear()

            def targetGpuAllocSize(self):
                """ohmgpu/GpuCache.h:139: byte budget of the device-side voxel storage (0: the device's free memory)."""
                return int(owner.cacheStats()["memory_limit"])

            def layerCount(self):
                """ohmgpu/GpuCache.h:143"""
                return len(owner.map().layers)

        return _GpuCacheView()

    def removeRegions(self, keys):
        """MapRegionCache::remove (what OccupancyMap::cullRegions calls on the GPU cache, ohm/OccupancyMap.cpp:1202-1234):
        drop the listed regions from the device map.  Returns how many were resident."""
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        removed = C.c_size_t(0)
        L.check(L.lib.ohmhip_map_remove_regions(self._handle, keys.ctypes.data, len(keys), C.byref(removed)),
                "removeRegions")
        return int(removed.value)

    def clear(self):
        """OccupancyMap::clear() as the GPU cache sees it (GpuCache::clear, ohmgpu/GpuCache.cpp): drop every resident
        region; the host map's chunks are the caller's to clear."""
        L.check(L.lib.ohmhip_map_clear(self._handle), "clear")

    def regionKeys(self, dirty_only=False):
        n = C.c_size_t(0)
        fn = L.lib.ohmhip_map_dirty_regions if dirty_only else L.lib.ohmhip_map_regions
        L.check(fn(self._handle, None, 0, C.byref(n)), "regions")
        keys = np.zeros((n.value, 3), dtype=np.int16)
        if n.value:
            L.check(fn(self._handle, keys.ctypes.data, n.value, C.byref(n)), "regions")
        return keys

    def syncVoxels(self, layer_names=None):
        """ohmgpu/GpuMap.cpp:308-345: fence + copy modified regions back into the host MapChunk blocks -- every layer,
        or only `layer_names` (the regions then stay marked as modified: there is one mark per region, not per layer, so
        a later full syncVoxels() still brings the other layers over)."""
        if not self._ok:
            return
        keys = self.regionKeys(dirty_only=True)
        names = layer_names if layer_names is not None else self._map.layers
        rv = self._map.regionVoxelVolume()
        key_tuples = [tuple(k) for k in keys.tolist()]
        chunks = self._map.chunks
        for name in names:
            lid, dtype, comps = LAYERS[name]
            # (block addresses are remembered per chunk: `ndarray.ctypes` costs a microsecond per block, which at C1's
            # 1243 regions is a third of the copy itself)
            cache = self._block_addr.setdefault(name, {})
            ptrs = np.empty(len(key_tuples), dtype=np.uint64)
            for i, k in enumerate(key_tuples):
                chunk = chunks.get(k)
                if chunk is None:
                    chunk = chunks[k] = {}
                block = chunk.get(name)
                if block is None:
                    block = chunk[name] = np.empty(rv * comps, dtype=dtype)  # fully overwritten by the copy below
                cached = cache.get(k)
                if cached is None or cached[0] is not block:
                    cached = cache[k] = (block, block.ctypes.data)
                ptrs[i] = cached[1]
            if not len(key_tuples):
                continue
            L.check(L.lib.ohmhip_map_read_regions(self._handle, lid, keys.ctypes.data, len(key_tuples),
                                                  ptrs.ctypes.data_as(C.POINTER(C.c_void_p))), "syncVoxels")
        if layer_names is None:
            L.check(L.lib.ohmhip_map_clear_dirty(self._handle), "clear_dirty")
        self.wait()

    def cacheStats(self, reset=False):
        """GpuLayerCache::queryStats (ohmgpu/GpuLayerCache.h:334-339) for the resident region pool: hits / misses / full
        plus the pool's size (include/ohmhip.h: ohmhip_cache_stats)."""
        st = L.CacheStats()
        L.check(L.lib.ohmhip_map_cache_stats(self._handle, C.byref(st), 1 if reset else 0), "cache_stats")
        return {name: getattr(st, name) for name, _ in L.CacheStats._fields_}

    def setMemoryLimit(self, nbytes):
        """Bound the region pool (include/ohmhip.h "RESIDENCY LIMIT"): a batch that needs more fails with
        OHMHIP_ERR_CAPACITY and leaves the map as it was.  0 removes the bound."""
        L.check(L.lib.ohmhip_map_set_memory_limit(self._handle, int(nbytes)), "set_memory_limit")

    def setSpillToHost(self, enable=True):
        """With a memory limit set: instead of failing, a batch that needs more regions than fit moves the least
        recently used resident regions to a host store inside the library and repeats; stored regions stay part of the
        map (listed, synced, brought back when touched).  include/ohmhip.h "SPILL TO HOST"; the reference's LRU reuse
        of cache slots (ohmgpu/GpuLayerCache.cpp:530-584) serves the same purpose."""
        L.check(L.lib.ohmhip_map_set_spill_to_host(self._handle, 1 if enable else 0), "set_spill_to_host")

    def setSpillWriteback(self, enable=True):
        """Opt-in background write-back of the spill path (include/ohmhip.h "WRITE-BACK"): the regions the eviction
        policy would take next are copied to the host store while batches run, so an eviction finds them clean."""
        L.check(L.lib.ohmhip_map_set_spill_writeback(self._handle, 1 if enable else 0), "set_spill_writeback")

    def setBatchCoalescing(self, min_rays):
        """Collect consecutive small host batches and run them as one device batch of >= min_rays rays
        (include/ohmhip.h: ohmhip_map_set_batch_coalescing; on by default with 65536).  0 turns it off."""
        L.check(L.lib.ohmhip_map_set_batch_coalescing(self._handle, int(min_rays)), "setBatchCoalescing")

    def setAsyncLaunch(self, enable=True):
        """Large host-pointer batches return once their rays are staged; the launch sequence runs on a thread of the map
        (include/ohmhip.h: ohmhip_map_set_async_launch).  Off by default."""
        L.check(L.lib.ohmhip_map_set_async_launch(self._handle, 1 if enable else 0), "setAsyncLaunch")

    def setRegionOwnership(self, world_size, rank, block_shift=0):
        """Owner-computes multi-GPU mode (include/ohmhip.h: ohmhip_map_set_region_ownership): integrate only what falls
        in the regions `rank` owns among `world_size` region-partitioned maps.  Call before the first integrateRays."""
        L.check(L.lib.ohmhip_map_set_region_ownership(self._handle, int(world_size), int(rank), int(block_shift)),
                "setRegionOwnership")
        self._ownership = (int(world_size), int(rank), int(block_shift))

    def setRegionPartition(self, partition):
        """Partitioned multi-GPU mode (include/ohmhip.h "Partitioned map"): like setRegionOwnership, with the region blocks
        dealt by `partition` (ohm_amd.distributed.RegionPartition: a block -> rank table, or the block hash).  Call
        before the first integrateRays."""
        L.check(L.lib.ohmhip_map_set_region_partition(self._handle, C.byref(partition.c_struct(self_rank=True))),
                "setRegionPartition")
        self._partition = partition
        self._ownership = (partition.world_size, partition.rank, partition.block_shift)

    def regionOwners(self, keys):
        """Owner rank of each int16 (n, 3) region key under this map's partition."""
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        owners = np.zeros(len(keys), dtype=np.uint32)
        L.check(L.lib.ohmhip_map_region_owners(self._handle, keys.ctypes.data, len(keys), owners.ctypes.data),
                "regionOwners")
        return owners

    def routeRays(self, d_rays, ray_count, d_routed, capacity, ray_update_flags=0, d_index=None):
        """ohmhip_map_route_rays: destinations of `ray_count` rays in device memory under this map's partition, compacted
        per destination into `d_routed` (device pointer, `capacity` rays).  Returns (counts per rank, voxel visits of the
        input rays, fits): fits is False when the routed rays exceed `capacity` (grow and repeat)."""
        world = max(1, self._ownership[0]) if getattr(self, "_ownership", None) else 1
        counts = np.zeros(world, dtype=np.uint32)
        visits = C.c_uint64(0)
        status = L.lib.ohmhip_map_route_rays(self._handle, d_rays, int(ray_count), int(ray_update_flags), d_routed,
                                             d_index, int(capacity), counts.ctypes.data, C.byref(visits))
        if status not in (L.OK, L.ERR_CAPACITY):
            L.check(status, "routeRays")
        return counts, int(visits.value), status == L.OK

    def lineKeys(self, lines, max_keys_per_line=1024):
        """LineKeysQueryGpu equivalent: voxel keys along each query line (start/end pairs, (2N, 3) float64).
        Returns (keys, counts): keys is (N, max_keys, 10) uint8 viewed as int16 region[3] + uint8 voxel[4]."""
        lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 6)
        n = lines.shape[0]
        keys = np.zeros((n, max_keys_per_line, 10), dtype=np.uint8)
        counts = np.zeros(n, dtype=np.uint32)
        L.check(L.lib.ohmhip_map_line_keys(self._handle, lines.ctypes.data, n, max_keys_per_line, keys.ctypes.data,
                                           counts.ctypes.data), "lineKeys")
        regions = keys[:, :, :6].copy().view(np.int16).reshape(n, max_keys_per_line, 3)
        voxels = keys[:, :, 6:9]
        return regions, voxels, counts

    def raysQuery(self, rays, volume_coefficient=1.0):
        """RaysQuery on the device (ohmhip_map_rays_query; ohm/RaysQuery.cpp:102-203, bit for bit): rays are (2N, 3)
        float64 origin / end point pairs (an odd trailing point is not a ray).  Returns (ranges f64, unobserved volumes
        f64, terminal types i8 (OccupancyType), terminal voxel regions (N, 3) int16, local keys (N, 3) uint8).  The map's
        current parameters (threshold, built-in ray filter) apply; the map is read, never changed."""
        self._push_config_if_changed()
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 3)
        n = rays.shape[0] // 2
        ranges = np.zeros(n, dtype=np.float64)
        volumes = np.zeros(n, dtype=np.float64)
        types = np.zeros(n, dtype=np.int8)
        keys = np.zeros((n, 10), dtype=np.uint8)
        L.check(L.lib.ohmhip_map_rays_query(self._handle, rays.ctypes.data, rays.shape[0], float(volume_coefficient),
                                            ranges.ctypes.data, volumes.ctypes.data, types.ctypes.data,
                                            keys.ctypes.data), "raysQuery")
        return ranges, volumes, types, keys[:, :6].copy().view(np.int16).reshape(n, 3), keys[:, 6:9].copy()

    def clearanceRegions(self, keys, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0)):
        """Clearance of every voxel of each region in keys ((N, 3) int16, present in the map or not) on the device
        (ohmhip_map_clearance_regions; calculateNearestNeighbour, ohm/private/VoxelAlgorithms.cpp:22-98, bit for bit):
        (N, dz, dy, dx) float32, the distance to the nearest obstructing voxel within search_radius, 0 for an
        obstructing voxel, -1 when none.  flags: QueryFlag.kQfUnknownAsOccupied, kQfReportUnscaledResults (others are
        ignored).  The map is read, never changed."""
        self._push_config_if_changed()
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        n = keys.shape[0]
        dx, dy, dz = self._map.region_voxel_dimensions
        out = np.zeros((n, dz, dy, dx), dtype=np.float32)
        dsts = (C.c_void_p * max(n, 1))(*[out[i].ctypes.data for i in range(n)])
        L.check(L.lib.ohmhip_map_clearance_regions(self._handle, keys.ctypes.data, n,
                                                   C.byref(_clearance_params(search_radius, flags, axis_scaling)),
                                                   dsts), "clearanceRegions")
        return out

    def clearanceRegionsDevice(self, keys, d_out, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0), sync=True):
        """clearanceRegions into device memory (ohmhip_map_clearance_regions_device): d_out is a raw device pointer to
        N * region voxels float32 (a torch tensor's data_ptr(), ...), written on the map's stream; with sync=False the
        values are valid after wait()."""
        self._push_config_if_changed()
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        L.check(L.lib.ohmhip_map_clearance_regions_device(self._handle, keys.ctypes.data, keys.shape[0],
                                                          C.byref(_clearance_params(search_radius, flags,
                                                                                    axis_scaling)), d_out),
                "clearanceRegionsDevice")
        if sync:
            self.wait()

    def clearanceKeys(self, keys, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0)):
        """The clearance of arbitrary voxels (ohmhip_map_clearance_keys): keys are (N, 10) GpuKey records, as lineKeys
        returns them, or a (regions (N, 3), locals (N, 3)) pair.  Returns (N,) float32, the values clearanceRegions
        gives those voxels."""
        self._push_config_if_changed()
        rec = _key_records(keys)
        n = rec.shape[0]
        out = np.zeros(n, dtype=np.float32)
        L.check(L.lib.ohmhip_map_clearance_keys(self._handle, rec.ctypes.data, n,
                                                C.byref(_clearance_params(search_radius, flags, axis_scaling)),
                                                out.ctypes.data), "clearanceKeys")
        return out

    def hasLayer(self, name):
        """Whether the device map holds layer `name` (LAYERS)."""
        return bool(self._layer_bits & (1 << LAYERS[name][0]))

    # OccupancyMap::updateLayout and the add*Layer calls (ohm/OccupancyMap.cpp:521-682) on the live map: the device map
    # and the host map it wraps change together (include/ohmhip.h "LAYER CHANGES": the layers that stay do not move).
    def updateLayout(self, layers, preserve_map=True):
        """The map holds exactly `layers` (names of LAYERS) from the next batch on: added layers start cleared, removed
        ones are released, the others keep their voxels.  preserve_map=False also drops every region.  Raises
        OhmHipError -- and changes nothing -- for a layer the map's mode needs, a partitioned or merging map, or a
        memory limit the new set does not fit."""
        layers = list(dict.fromkeys(layers))
        bits = 0
        for name in layers:
            bits |= 1 << LAYERS[name][0]
        stats = L.LayerChangeStats()
        L.check(L.lib.ohmhip_map_update_layers(self._handle, bits, 0 if preserve_map else L.LAYOUT_DISCARD_MAP,
                                               C.byref(stats)), "GpuMap.updateLayout")
        self._last_layer_change = {name: getattr(stats, name) for name, _ in L.LayerChangeStats._fields_}
        self._layer_bits = bits
        self._cfg.layers = bits
        self._map.updateLayout(layers, preserve_map)
        # (the chunks' blocks of the new layers are new arrays, the removed layers' are gone)
        self._block_addr = {name: cache for name, cache in self._block_addr.items() if name in layers}
        if not preserve_map:
            self._block_addr = {}

    def addLayer(self, name):
        if not self.hasLayer(name):
            self.updateLayout(list(self._map.layers) + [name])

    def removeLayer(self, name):
        if self.hasLayer(name):
            self.updateLayout([n for n in self._map.layers if n != name])

    def addVoxelMeanLayer(self):
        """OccupancyMap::addVoxelMeanLayer (ohm/OccupancyMap.cpp:521)."""
        self.addLayer("mean")

    def addTraversalLayer(self):
        self.addLayer("traversal")

    def addTouchTimeLayer(self):
        self.addLayer("touch_time")

    def addIncidentNormalLayer(self):
        self.addLayer("incident_normal")

    def voxelMeanEnabled(self):
        return self.hasLayer("mean")

    def traversalEnabled(self):
        return self.hasLayer("traversal")

    def touchTimeEnabled(self):
        return self.hasLayer("touch_time")

    def incidentNormalEnabled(self):
        return self.hasLayer("incident_normal")

    def lastLayerChangeStats(self):
        """ohmhip_layer_change_stats of the last updateLayout / addLayer / removeLayer that changed the map (None before
        the first)."""
        return getattr(self, "_last_layer_change", None)

    def clearanceStaleRegions(self, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0)):
        """The regions whose clearance layer is stale for these parameters, (N, 3) int16 in processing order
        (ascending z, y, x): ohmhip_map_clearance_stale_regions."""
        self._push_config_if_changed()
        params = _clearance_params(search_radius, flags, axis_scaling)
        n = C.c_size_t(0)
        L.check(L.lib.ohmhip_map_clearance_stale_regions(self._handle, C.byref(params), None, 0, C.byref(n)),
                "clearanceStaleRegions")
        keys = np.zeros((n.value, 3), dtype=np.int16)
        if n.value:
            L.check(L.lib.ohmhip_map_clearance_stale_regions(self._handle, C.byref(params), keys.ctypes.data, n.value,
                                                             C.byref(n)), "clearanceStaleRegions")
        return keys[:n.value]

    def clearanceUpdate(self, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0), max_regions=0):
        """Bring up to max_regions (0: all) stale regions' clearance layer up to date (ohmhip_map_clearance_update).
        Returns (processed, remaining)."""
        self._push_config_if_changed()
        processed, remaining = C.c_size_t(0), C.c_size_t(0)
        L.check(L.lib.ohmhip_map_clearance_update(self._handle, C.byref(_clearance_params(search_radius, flags,
                                                                                          axis_scaling)),
                                                  int(max_regions), C.byref(processed), C.byref(remaining)),
                "clearanceUpdate")
        return int(processed.value), int(remaining.value)

    def clearanceUpdateRegions(self, keys, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0), force=True):
        """Write the clearance layer of the listed regions that are present in the map -- all of them with force, the
        stale ones otherwise (ohmhip_map_clearance_update_regions).  Returns how many were written."""
        self._push_config_if_changed()
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        processed = C.c_size_t(0)
        L.check(L.lib.ohmhip_map_clearance_update_regions(self._handle, keys.ctypes.data, keys.shape[0],
                                                          C.byref(_clearance_params(search_radius, flags,
                                                                                    axis_scaling)),
                                                          1 if force else 0, C.byref(processed)),
                "clearanceUpdateRegions")
        return int(processed.value)

    def nearestNeighbours(self, points, search_radius, flags=0, capacity=None):
        """ohm::NearestNeighbours on the device for every row of points ((Q, 3) float64) at once (ohmhip_map_nearest_
        neighbours; ohm/NearestNeighbours.cpp:35-181, 240-284, operation for operation): every obstructing voxel within
        search_radius of a point, in the CPU query's visiting order, or with QueryFlag.kQfNearestResult only the closest.
        flags: kQfUnknownAsOccupied, kQfNearestResult.  Returns (counts (Q,) uint64, keys GPU_KEY_DTYPE, ranges float32);
        the results of query q start at counts[:q].sum().  capacity: at most that many results are fetched (None: all;
        0: count only) -- counts are always the full numbers.  The map is read, never changed."""
        self._push_config_if_changed()
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        nq = points.shape[0]
        params = L.NeighboursParams(float(search_radius), int(flags) & 0xffffffff)
        counts = np.zeros(nq, dtype=np.uint64)
        total = C.c_uint64(0)
        def call(cap, keys, ranges):
            L.check(L.lib.ohmhip_map_nearest_neighbours(self._handle, points.ctypes.data, nq, C.byref(params), cap,
                                                        counts.ctypes.data, keys.ctypes.data if cap else None,
                                                        ranges.ctypes.data if cap else None, C.byref(total)),
                    "nearestNeighbours")

        keys, ranges = np.zeros(0, dtype=_GPU_KEY), np.zeros(0, dtype=np.float32)
        if capacity is None:
            call(0, keys, ranges)  # count, then fetch exactly that many
            capacity = int(total.value)
            if capacity == 0:
                return counts, keys, ranges
        capacity = int(capacity)
        keys, ranges = np.zeros(capacity, dtype=_GPU_KEY), np.zeros(capacity, dtype=np.float32)
        call(capacity, keys, ranges)
        n = min(capacity, int(total.value))
        return counts, keys[:n], ranges[:n]

    def voxelKeys(self, points):
        """OccupancyMap::voxelKey of every row of points ((N, 3) float64) in the map's geometry (ohmhip_map_voxel_keys):
        (N,) GPU_KEY_DTYPE records, Key::kNull (region -32768 x 3, voxel 0) where the reference yields it."""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        keys = np.zeros(points.shape[0], dtype=_GPU_KEY)
        L.check(L.lib.ohmhip_map_voxel_keys(self._handle, points.ctypes.data, points.shape[0], keys.ctypes.data),
                "voxelKeys")
        return keys

    def readVoxels(self, keys, layer_name):
        """The voxels of layer `layer_name` at keys -- GPU_KEY_DTYPE / (N, 10) uint8 records or a (regions, locals) pair --
        read on the device (ohmhip_map_read_voxels): (values, present), values typed through LAYERS ((N,) or (N,
        components)), present (N,) uint8: 1 when the map holds the key's region.  A voxel the map does not hold reads the
        layer's clear value."""
        self._push_config_if_changed()
        lid, dtype, comps = LAYERS[layer_name]
        rec = _key_records(keys.view(np.uint8) if isinstance(keys, np.ndarray) and keys.dtype == _GPU_KEY else keys)
        n = rec.shape[0]
        values = np.zeros((n, comps) if comps > 1 else n, dtype=dtype)
        present = np.zeros(n, dtype=np.uint8)
        L.check(L.lib.ohmhip_map_read_voxels(self._handle, lid, rec.ctypes.data, n, values.ctypes.data,
                                             present.ctypes.data), "readVoxels")
        return values, present

    def occupancyTypes(self, keys):
        """OccupancyType of the voxels at keys: kNull where the map does not hold the region, else occupancyType (ohm/
        VoxelOccupancy.h:116-128: a NaN is unobserved).  (N,) int8."""
        values, present = self.readVoxels(keys, "occupancy")
        with np.errstate(invalid="ignore"):
            types = np.where(values < np.float32(np.inf),
                             np.where(values < np.float32(self._map.occupancy_threshold_value), OccupancyType.kFree,
                                      OccupancyType.kOccupied), OccupancyType.kUnobserved)
        return np.where(present != 0, types, OccupancyType.kNull).astype(np.int8)

    def covarianceEigen(self, keys):
        """covarianceEigenDecomposition (ohm/CovarianceVoxel.cpp:147-154) of the voxels at keys -- in every form
        readVoxels takes -- by the rule D1-D4 of include/ohmhip.h, on the device (ohmhip_map_covariance_eigen):
        (eigenvalues (N, 3) float64 ascending, eigenvectors (N, 3, 3) float64 with eigenvectors[i, c] the column of
        eigenvalue c, status (N,) uint8: 0 the map holds no such region or the key is null, 1 decomposed, 2 a non-finite
        covariance).  Only the results cross to the host; the map is read, never changed."""
        self._push_config_if_changed()
        rec = _key_records(keys.view(np.uint8) if isinstance(keys, np.ndarray) and keys.dtype == _GPU_KEY else keys)
        n = rec.shape[0]
        values = np.zeros((n, 3), dtype=np.float64)
        vectors = np.zeros((n, 3, 3), dtype=np.float64)
        status = np.zeros(n, dtype=np.uint8)
        L.check(L.lib.ohmhip_map_covariance_eigen(self._handle, rec.ctypes.data, n, values.ctypes.data,
                                                  vectors.ctypes.data, status.ctypes.data), "covarianceEigen")
        return values, vectors, status

    # -- voxel edits by key (include/ohmhip.h, VOXEL EDITS) -----------------------------------------------------------
    def _edit_keys(self, keys):
        return _key_records(keys.view(np.uint8) if isinstance(keys, np.ndarray) and keys.dtype == _GPU_KEY else keys)

    def _edit_done(self, status, stats, what):
        self._last_edit_stats = {name: int(getattr(stats, name)) for name, _ in L.VoxelEditStats._fields_}
        L.check(status, what)
        return self._last_edit_stats["applied"]

    def writeVoxels(self, keys, layer_name, values):
        """Voxel<T>::write for many voxels (ohmhip_map_write_voxels): the voxels of layer `layer_name` at keys -- in
        every form readVoxels takes -- become values ((N,) or (N, components), converted to the layer's type; the bytes
        are stored as given).  Among duplicate keys the last wins; null keys are skipped; regions the map does not hold
        are created.  Returns the number of elements applied; lastEditStats() has the rest."""
        self._push_config_if_changed()
        lid, dtype, comps = LAYERS[layer_name]
        rec = self._edit_keys(keys)
        n = rec.shape[0]
        values = np.ascontiguousarray(values, dtype=dtype).reshape((n, comps) if comps > 1 else n)
        stats = L.VoxelEditStats()
        status = L.lib.ohmhip_map_write_voxels(self._handle, lid, rec.ctypes.data if n else None, n,
                                               values.ctypes.data if n else None, C.byref(stats))
        return self._edit_done(status, stats, "writeVoxels")

    def integrateVoxels(self, ops, keys=None, points=None):
        """One VoxelEdit per element (an array, or one value for all) at keys, or at the voxels of points ((N, 3)
        float64) (ohmhip_map_integrate_voxels): ohm::integrateHit(map, key), ohm::integrateMiss(map, key) and -- points
        only -- ohm::integrateHit(map, sample), per voxel in input order.  Returns the number of elements applied."""
        self._push_config_if_changed()
        if (keys is None) == (points is None):
            raise ValueError("integrateVoxels takes keys or points")
        rec = pts = None
        if keys is not None:
            rec = self._edit_keys(keys)
            n = rec.shape[0]
        else:
            pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
            n = pts.shape[0]
        op_array = None
        op = 0
        if np.ndim(ops) == 0:
            op = int(ops)
        else:
            op_array = np.ascontiguousarray(ops, dtype=np.uint8).reshape(-1)
            if op_array.shape[0] != n:
                raise ValueError("one op per element")
        stats = L.VoxelEditStats()
        status = L.lib.ohmhip_map_integrate_voxels(self._handle, op_array.ctypes.data if op_array is not None else None,
                                                   op, rec.ctypes.data if rec is not None else None,
                                                   pts.ctypes.data if pts is not None else None, n, C.byref(stats))
        return self._edit_done(status, stats, "integrateVoxels")

    def integrateHits(self, keys=None, points=None, update_mean=False):
        """ohm::integrateHit(map, key) at every key / at the voxel of every point; with update_mean (points only)
        ohm::integrateHit(map, sample): the voxel mean takes the point as well."""
        if update_mean and points is None:
            raise ValueError("update_mean needs points")
        return self.integrateVoxels(VoxelEdit.kHitSample if update_mean else VoxelEdit.kHit, keys, points)

    def integrateMisses(self, keys=None, points=None):
        """ohm::integrateMiss(map, key) at every key / at the voxel of every point."""
        return self.integrateVoxels(VoxelEdit.kMiss, keys, points)

    def lastEditStats(self):
        """ohmhip_voxel_edit_stats of the last edit as a dict (all zero after one that failed)."""
        return dict(getattr(self, "_last_edit_stats", {name: 0 for name, _ in L.VoxelEditStats._fields_}))

    def keyRange(self, lo, hi):
        """ohm::KeyRange (ohm/KeyRange.h) of the closed box between two keys (GPU_KEY_DTYPE records) or two points
        (3 floats each, through voxelKeys): its keys as GPU_KEY_DTYPE records, x fastest, then y, then z -- the order
        KeyRange::walkNext visits them in (ohm/KeyRange.cpp:105-129).  Empty when max lies below min on any axis."""
        def as_key(v):
            if isinstance(v, (np.ndarray, np.void)) and getattr(v, "dtype", None) == _GPU_KEY:
                return np.asarray(v).reshape(1)[0]
            return self.voxelKeys(np.asarray(v, dtype=np.float64).reshape(1, 3))[0]
        return key_range(as_key(lo), as_key(hi), self._map.region_voxel_dimensions)

    def filterPoints(self, points, expected_value_tolerance=-1.0, occupancy_only=False, capacity=None):
        """ohmfilter's test of every row of points ((N, 3) float64) on the device (ohmhip_map_filter_points; utils/
        ohmfilter/ohmfilter.cpp:150-279): a point is kept when its voxel is occupied and -- on a map with the mean and
        covariance layers, unless occupancy_only is set or the tolerance is negative -- it lies inside the voxel's
        Gaussian, a < 3 + expected_value_tolerance (filterPointByCovariance, :67-91).  Returns (status (N,) uint8: 0 not
        occupied, 1 kept, 2 removed by the covariance test; kept indices uint64, ascending; values (N,) float64: a where
        the covariance test ran, NaN elsewhere; keys (N,) GPU_KEY_DTYPE).  capacity: at most that many kept indices are
        fetched (None: room for all; 0: none).  lastFilterKept() is always the full number of kept points.  The map is
        read, never changed."""
        self._push_config_if_changed()
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = points.shape[0]
        capacity = n if capacity is None else int(capacity)
        params = L.PointFilterParams(float(expected_value_tolerance), L.PF_OCCUPANCY_ONLY if occupancy_only else 0)
        status = np.zeros(n, dtype=np.uint8)
        indices = np.zeros(capacity, dtype=np.uint64)
        values = np.zeros(n, dtype=np.float64)
        keys = np.zeros(n, dtype=_GPU_KEY)
        kept = C.c_uint64(0)
        L.check(L.lib.ohmhip_map_filter_points(self._handle, points.ctypes.data if n else None, n, C.byref(params),
                                               capacity, status.ctypes.data, indices.ctypes.data if capacity else None,
                                               values.ctypes.data, keys.ctypes.data, C.byref(kept)), "filterPoints")
        self._last_filter_kept = int(kept.value)
        return status, indices[:min(capacity, int(kept.value))], values, keys

    def lastFilterKept(self):
        """The number of points the last filterPoints() kept, whatever its capacity."""
        return getattr(self, "_last_filter_kept", 0)

    def raysQueryDevice(self, d_rays, element_count, d_ranges, d_volumes, d_types, d_keys=None,
                        volume_coefficient=1.0, sync=True):
        """raysQuery on device memory (ohmhip_map_rays_query_device), for rays already in HBM: raw device pointers
        (ohmhip_buffer_ptr of a library buffer, a torch tensor's data_ptr(), ...) to element_count dvec3 and to the
        outputs -- n = element_count // 2 doubles (ranges, volumes), n int8 (types), n 10-byte GpuKey records (keys,
        optional).  The rays must be complete when the call is made (synchronise the stream that produced them).  The
        query runs on the map's stream: with sync=False the outputs are valid after wait()."""
        self._push_config_if_changed()
        L.check(L.lib.ohmhip_map_rays_query_device(self._handle, d_rays, int(element_count), float(volume_coefficient),
                                                   d_ranges, d_volumes, d_types, d_keys), "raysQueryDevice")
        if sync:
            self.wait()

    def lastCopyStats(self):
        """ohmhip_copy_stats of the last copyMap() into this map (ohm_amd.copyutil), as a dict."""
        return dict(getattr(self, "_last_copy_stats", {}))

    def _clone_arguments(self):
        """Constructor arguments, beyond the map and the sizes, that make a map of the same configuration."""
        return {}

    def clone(self, min_ext=None, max_ext=None):
        """OccupancyMap::clone (ohm/OccupancyMap.cpp:953-1004) on the device: a new map of the same class, configuration
        and layers, then the regions that pass the extents rule of copyFilterExtents (every region without extents:
        +-inf) -- copied device to device by ohmhip_map_copy.  Returns the new GpuMap; its host map holds no chunks
        until its syncVoxels()."""
        from . import copyutil
        src_map = self._map
        new_map = OccupancyMap(src_map.resolution, src_map.region_voxel_dimensions, layers=tuple(src_map.layers))
        for name in ("origin", "min_voxel_value", "max_voxel_value", "hit_value", "miss_value",
                     "occupancy_threshold_value", "saturate_at_min_value", "saturate_at_max_value", "ray_filter"):
            setattr(new_map, name, getattr(src_map, name))
        other = type(self)(new_map, True, gpu_mem_size=int(self._cfg.gpu_mem_size),
                           region_capacity=int(self._cfg.region_capacity), **self._clone_arguments())
        inf = float("inf")
        chunk_filter = copyutil.copyFilterExtents((-inf,) * 3 if min_ext is None else min_ext,
                                                  (inf,) * 3 if max_ext is None else max_ext)
        if not copyutil.copyMap(other, self, chunk_filter):
            raise L.OhmHipError(L.ERR_INTERNAL, "GpuMap.clone")
        return other

    def _upload_existing(self):
        """gpumap::enableGpu + GpuLayerCache::upload for regions the CPU map already holds."""
        self.uploadRegions()

    def uploadRegions(self, keys=None):
        """Push host chunks to the device: all of them, or the listed regions -- what GpuLayerCache::upload does for a
        region whose CPU copy is newer than the device's (ohmgpu/GpuLayerCache.cpp:172-182), e.g. after CPU-side
        integration into the host map.  Layers a chunk does not hold keep their device contents."""
        if not self._map.chunks:
            return 0
        if keys is None:
            keys = sorted(self._map.chunks.keys())
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        keys = np.array([k for k in keys if tuple(int(v) for v in k) in self._map.chunks], dtype=np.int16).reshape(-1, 3)
        for name in self._map.layers:
            lid, dtype, comps = LAYERS[name]
            have = [k for k in keys if name in self._map.chunks[tuple(int(v) for v in k)]]
            if not have:
                continue
            sub = np.ascontiguousarray(np.array(have, dtype=np.int16).reshape(-1, 3))
            blocks = [np.ascontiguousarray(self._map.chunks[tuple(int(v) for v in k)][name], dtype=dtype) for k in sub]
            ptrs = (C.c_void_p * len(blocks))(*[b.ctypes.data for b in blocks])
            L.check(L.lib.ohmhip_map_write_regions(self._handle, lid, sub.ctypes.data, len(blocks), ptrs), "upload")
        return len(keys)


class GpuNdtMap(GpuMap):
    """ohm::GpuNdtMap (ohmgpu/GpuNdtMap.h:63-132)."""
    _mode = L.MODE_NDT_OM

    def __init__(self, map_, borrowed_map=True, expected_element_count=2048, gpu_mem_size=0,
                 ndt_mode=NdtMode.kOccupancy, region_capacity=0):
        self._ndt_mode = NdtMode(ndt_mode)
        self._mode = L.MODE_NDT_TM if self._ndt_mode == NdtMode.kTraversability else L.MODE_NDT_OM
        # ohm/private/NdtMapDetail.h:20-45
        self.sensor_noise = 0.05
        self.sample_threshold = 3
        mp = float(map_.missProbability())
        # ohm/NdtMap.h:146-149
        self.adaptation_rate = float(np.float32(max(0.0, min(np.float32(2.0) * (np.float32(1.0) - np.float32(2.0) *
                                                                                   np.float32(mp)), 1.0))))
        self.reinitialise_covariance_threshold = float(probability_to_value(0.2))
        self.reinitialise_covariance_point_count = 100
        self.initial_intensity_covariance = 1.0
        super().__init__(map_, borrowed_map, expected_element_count, gpu_mem_size, region_capacity)

    def _configure_layers(self):
        # NdtMap::enableNdt adds mean + covariance (+ intensity, hit/miss for TM). ohm/NdtMap.cpp:194-213
        for name in ("occupancy", "mean", "covariance"):
            self._map.addLayer(name)
        if self._ndt_mode == NdtMode.kTraversability:
            self._map.addLayer("intensity")
            self._map.addLayer("hit_miss_count")

    def _fill_config(self, cfg):
        cfg.ndt_sensor_noise = self.sensor_noise
        cfg.ndt_sample_threshold = self.sample_threshold
        cfg.ndt_adaptation_rate = self.adaptation_rate
        cfg.ndt_reinit_threshold = self.reinitialise_covariance_threshold
        cfg.ndt_reinit_count = self.reinitialise_covariance_point_count
        cfg.ndt_initial_intensity_cov = self.initial_intensity_covariance

    def _clone_arguments(self):
        return {"ndt_mode": self._ndt_mode}

    def clone(self, min_ext=None, max_ext=None):
        other = super().clone(min_ext, max_ext)
        for name in ("sensor_noise", "sample_threshold", "adaptation_rate", "reinitialise_covariance_threshold",
                     "reinitialise_covariance_point_count", "initial_intensity_covariance"):
            setattr(other, name, getattr(self, name))  # (taken by the clone's next batch)
        return other

    def setSensorNoise(self, noise):
        """GpuNdtMap::setSensorNoise (ohmgpu/GpuNdtMap.h:63-132): applies from the next batch."""
        self.sensor_noise = float(noise)

    def sensorNoise(self):
        return self.sensor_noise


class GpuTsdfMap(GpuMap):
    """ohm::GpuTsdfMap (ohmgpu/GpuTsdfMap.h:37-94)."""
    _mode = L.MODE_TSDF

    def __init__(self, map_, borrowed_map=True, expected_element_count=2048, gpu_mem_size=0, max_weight=1e4,
                 default_truncation_distance=0.1, dropoff_epsilon=0.0, sparsity_compensation_factor=1.0,
                 region_capacity=0):
        self.tsdf_options = (max_weight, default_truncation_distance, dropoff_epsilon, sparsity_compensation_factor)
        super().__init__(map_, borrowed_map, expected_element_count, gpu_mem_size, region_capacity)

    def _configure_layers(self):
        self._map.addLayer("tsdf")

    def _fill_config(self, cfg):
        (cfg.tsdf_max_weight, cfg.tsdf_trunc, cfg.tsdf_dropoff, cfg.tsdf_sparsity) = self.tsdf_options

    def _clone_arguments(self):
        return dict(zip(("max_weight", "default_truncation_distance", "dropoff_epsilon",
                         "sparsity_compensation_factor"), self.tsdf_options))

    # ohmgpu/GpuTsdfMap.h:64-79: the option setters / getters under the reference's names (they apply from the next batch;
    # `tsdf_options` = (max_weight, default_truncation_distance, dropoff_epsilon, sparsity_compensation_factor)).
    def setTsdfOptions(self, max_weight, default_truncation_distance, dropoff_epsilon, sparsity_compensation_factor):
        self.tsdf_options = (float(max_weight), float(default_truncation_distance), float(dropoff_epsilon),
                             float(sparsity_compensation_factor))

    def _set_option(self, index, value):
        opts = list(self.tsdf_options)
        opts[index] = float(value)
        self.tsdf_options = tuple(opts)

    def setMaxWeight(self, max_weight):
        self._set_option(0, max_weight)

    def maxWeight(self):
        return self.tsdf_options[0]

    def setDefaultTruncationDistance(self, default_truncation_distance):
        self._set_option(1, default_truncation_distance)

    def defaultTruncationDistance(self):
        return self.tsdf_options[1]

    def setDropoffEpsilon(self, dropoff_epsilon):
        self._set_option(2, dropoff_epsilon)

    def dropoffEpsilon(self):
        return self.tsdf_options[2]

    def setSparsityCompensationFactor(self, sparsity_compensation_factor):
        self._set_option(3, sparsity_compensation_factor)

    def sparsityCompensationFactor(self):
        return self.tsdf_options[3]


class GpuTransformSamples:
    """ohm::GpuTransformSamples (ohmgpu/GpuTransformSamples.h:30-83): local sensor samples + a timestamped trajectory ->
    world-frame ray pairs in a device buffer that integrateRaysDevice() consumes directly."""

    def __init__(self):
        self._buffer = L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(self._buffer), 48, 3), "buffer_create")

    def close(self):
        if self._buffer:
            L.lib.ohmhip_buffer_destroy(self._buffer)
            self._buffer = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform(self, transform_times, transform_translations, transform_rotations_xyzw, sample_times, local_samples,
                  max_range=float("inf")):
        """Returns (device pointer, element_count): element_count = 2 x valid samples, as the reference returns."""
        times = np.ascontiguousarray(transform_times, dtype=np.float64)
        tr = np.ascontiguousarray(transform_translations, dtype=np.float64).reshape(-1, 3)
        rot = np.ascontiguousarray(transform_rotations_xyzw, dtype=np.float64).reshape(-1, 4)
        st = np.ascontiguousarray(sample_times, dtype=np.float64)
        pts = np.ascontiguousarray(local_samples, dtype=np.float64).reshape(-1, 3)
        count = C.c_uint32(0)
        L.check(L.lib.ohmhip_transform_samples(times.ctypes.data, tr.ctypes.data, rot.ctypes.data, times.shape[0],
                                               st.ctypes.data, pts.ctypes.data, pts.shape[0], float(max_range), None,
                                               self._buffer, C.byref(count)), "transform_samples")
        ptr = L._vp()
        L.check(L.lib.ohmhip_buffer_ptr(self._buffer, C.byref(ptr)), "buffer_ptr")
        return ptr, int(count.value)

    def read(self, element_count):
        """Copy the transformed rays back to the host ((element_count, 3) float64)."""
        out = np.zeros((element_count, 3), dtype=np.float64)
        if element_count:
            L.check(L.lib.ohmhip_buffer_read(self._buffer, out.ctypes.data, out.nbytes, 0, None, None, None), "buffer_read")
        return out


class LineKeysQueryGpu:
    """ohm::LineKeysQueryGpu (ohmgpu/LineKeysQueryGpu.h; interface of ohm/LineKeysQuery.h:47-101 + ohm/Query.h:51-121): the
    voxel keys along a set of query lines, walked on the device with the CPU walk's fp64 semantics
    (ohmhip_map_line_keys).  Given the GpuMap that holds the device handle (the query reads the map's geometry only)."""

    def __init__(self, gpu_map, query_flags=0):
        self._gpu_map = gpu_map
        self._query_flags = int(query_flags)
        self._rays = np.zeros((0, 3), dtype=np.float64)
        self.reset()

    def queryFlags(self):
        return self._query_flags

    def setQueryFlags(self, flags):
        self._query_flags = int(flags)

    def setRays(self, rays):
        """(2N, 3) start / end point pairs."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 3)
        self._rays = rays[:rays.shape[0] & ~1].copy()

    def rays(self):
        return self._rays

    def rayPointCount(self):
        return self._rays.shape[0]

    def reset(self, hard_reset=True):
        self._indices = np.zeros(0, dtype=np.uint64)
        self._counts = np.zeros(0, dtype=np.uint64)
        self._regions = np.zeros((0, 3), dtype=np.int16)
        self._locals = np.zeros((0, 3), dtype=np.uint8)

    def execute(self):
        self.reset(False)
        n = self._rays.shape[0] // 2
        if n == 0:
            return True
        # worst case keys per line, as the reference sizes its buffer (ohmgpu/LineKeysQueryGpu.cpp:112-119)
        length = np.linalg.norm(self._rays[1::2] - self._rays[0::2], axis=1)
        max_keys = int(np.ceil(length.max() / self._gpu_map.map().resolution * math.sqrt(3.0))) + 4
        regions, voxels, counts = self._gpu_map.lineKeys(self._rays, max_keys_per_line=max_keys)
        counts = np.minimum(counts.astype(np.uint64), np.uint64(max_keys))
        self._counts = counts
        self._indices = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        keep = np.arange(max_keys)[None, :] < counts[:, None]
        self._regions = regions[keep]
        self._locals = voxels[keep]
        return True

    def executeAsync(self):
        """The device call is synchronous: the asynchronous forms complete at once (ohm/Query.h:103-121)."""
        return self.execute()

    def wait(self, timeout_ms=0xffffffff):
        return True

    def numberOfResults(self):
        return int(self._counts.shape[0])

    def resultIndices(self):
        return self._indices

    def resultCounts(self):
        return self._counts

    def intersectedVoxels(self):
        """(regions (K, 3) int16, local keys (K, 3) uint8): all rays' keys in walk order, ray after ray."""
        return self._regions, self._locals

    def ranges(self):
        return None


def device_count():
    n = C.c_int(0)
    status = L.lib.ohmhip_device_count(C.byref(n))
    return n.value if status == L.OK else 0


def device_info(device=0):
    info = L.DeviceInfo()
    L.check(L.lib.ohmhip_device_get_info(device, C.byref(info)), "device_get_info")
    return {"name": info.name.decode(), "arch": info.arch.decode(), "total_memory": info.total_memory,
            "compute_units": info.compute_units, "lds_bytes_per_block": info.lds_bytes_per_block}


class RaysQueryGpu:
    """ohm::RaysQueryGpu (ohmgpu/RaysQueryGpu.h; interface of ohm/RaysQuery.h + ohm/Query.h:51-121): for each ray, how far
    it sees into the map (range to the first occupied voxel), the unobserved volume it crosses, the state and key of the
    voxel it ends in -- evaluated on the device against the resident map (GpuMap.raysQuery), bit-identical to the CPU
    query.  Given the GpuMap that holds the device handle."""

    kQfGpuEvaluate = 1 << 2  # ohm/QueryFlag.h:42

    def __init__(self, gpu_map, query_flags=0):
        self._gpu_map = gpu_map
        self._query_flags = int(query_flags) | self.kQfGpuEvaluate
        self._volume_coefficient = 1.0
        self._rays = np.zeros((0, 3), dtype=np.float64)
        self.reset()

    def queryFlags(self):
        return self._query_flags

    def setQueryFlags(self, flags):
        self._query_flags = int(flags) | self.kQfGpuEvaluate

    def setVolumeCoefficient(self, coefficient):
        self._volume_coefficient = float(coefficient)

    def volumeCoefficient(self):
        return self._volume_coefficient

    def setRays(self, rays):
        """(2N, 3) origin / end point pairs (an odd trailing point is dropped)."""
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 3)
        self._rays = rays[:rays.shape[0] & ~1].copy()

    def addRays(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 3)
        self._rays = np.concatenate([self._rays, rays[:rays.shape[0] & ~1]])

    def addRay(self, origin, end_point):
        self.addRays(np.array([origin, end_point], dtype=np.float64))

    def clearRays(self):
        self._rays = np.zeros((0, 3), dtype=np.float64)

    def rays(self):
        return self._rays

    def numberOfRays(self):
        return self._rays.shape[0] // 2

    def reset(self, hard_reset=True):
        """Drops the results; hard_reset also drops the rays (ohm/RaysQuery.cpp onReset)."""
        if hard_reset:
            self.clearRays()
        self._ranges = np.zeros(0, dtype=np.float64)
        self._volumes = np.zeros(0, dtype=np.float64)
        self._types = np.zeros(0, dtype=np.int8)
        self._regions = np.zeros((0, 3), dtype=np.int16)
        self._locals = np.zeros((0, 3), dtype=np.uint8)

    def execute(self):
        self.reset(False)
        (self._ranges, self._volumes, self._types, self._regions,
         self._locals) = self._gpu_map.raysQuery(self._rays, self._volume_coefficient)
        return True

    def executeAsync(self):
        """The device call is synchronous: the asynchronous forms complete at once (ohm/Query.h:103-121)."""
        return self.execute()

    def wait(self, timeout_ms=0xffffffff):
        return True

    def numberOfResults(self):
        return int(self._ranges.shape[0])

    def ranges(self):
        return self._ranges

    def unobservedVolumes(self):
        return self._volumes

    def terminalOccupancyTypes(self):
        return self._types

    def intersectedVoxels(self):
        """(regions (N, 3) int16, local keys (N, 3) uint8): each ray's terminal voxel."""
        return self._regions, self._locals


def _region_coord(value, origin, region_dim):
    """pointToRegionCoord (ohm/MapCoord.h:85-93) into the int16 of glm::i16vec3 (MapRegion, ohm/MapRegion.cpp:32-37)."""
    c = int(math.floor((float(value) - float(origin)) / region_dim + 0.5))
    return (c + 32768) % 65536 - 32768


class ClearanceProcess:
    """ohm::ClearanceProcess (ohmgpu/ClearanceProcess.h): the clearance of every voxel of a set of regions -- the distance
    to the nearest obstructing voxel within the search radius, per calculateNearestNeighbour (ohm/private/
    VoxelAlgorithms.cpp:22-98) -- evaluated exactly on the device (GpuMap.clearanceRegions), not by the reference's
    approximate flood fill.  The results of calculateForExtents are kept here per region.  On a map created with the
    clearance layer (ensureClearanceLayer before the GpuMap is made) the process also keeps that layer current:
    update() recomputes the regions whose neighbourhood changed since they were last written (ohmhip_map_clearance_update),
    and calculateForExtents writes the layer too, skipping up-to-date regions unless forced.  Not provided:
    serialisation."""

    kQfInstantiateUnknown = int(QueryFlag.kQfSpecialised) << 0  # ohmgpu/ClearanceProcess.h

    def __init__(self, search_radius=0.0, query_flags=0):
        self._search_radius = float(search_radius)
        self._query_flags = int(query_flags)
        self._axis_scaling = (1.0, 1.0, 1.0)
        self._results = {}
        self._region_dim = None

    def searchRadius(self):
        return self._search_radius

    def setSearchRadius(self, radius):
        self._search_radius = float(radius)

    def queryFlags(self):
        return self._query_flags

    def setQueryFlags(self, flags):
        self._query_flags = int(flags)

    def axisScaling(self):
        return self._axis_scaling

    def setAxisScaling(self, scaling):
        self._axis_scaling = tuple(float(v) for v in scaling)

    def reset(self):
        self._results = {}

    @staticmethod
    def ensureClearanceLayer(map_):
        """ClearanceProcess::ensureClearanceLayer (ohm/DefaultLayer.cpp:174-193): add the clearance layer (float,
        cleared to -1) to an OccupancyMap before its GpuMap is created.  Given a live GpuMap without the layer this
        raises: adding a layer there is the caller's decision -- GpuMap.addLayer("clearance") does it in place."""
        if isinstance(map_, GpuMap):
            if not map_.hasLayer("clearance"):
                raise RuntimeError("ensureClearanceLayer: the device map does not hold the clearance layer; "
                                   "add it with GpuMap.addLayer(\"clearance\"), or to the OccupancyMap before creating "
                                   "the GpuMap")
            return
        map_.addLayer("clearance")

    def update(self, gpu_map, time_slice=0.0, max_regions=0):
        """ClearanceProcess::update (ohmgpu/ClearanceProcess.cpp:418-470): recompute the clearance layer of stale
        regions, in ascending (z, y, x) key order, max_regions (0: all) per device call -- until time_slice seconds have
        passed, or until nothing is stale when time_slice <= 0.  Returns a MappingProcessResult."""
        self.ensureClearanceLayer(gpu_map)
        start = time.perf_counter()
        while True:
            _, remaining = gpu_map.clearanceUpdate(self._search_radius, self._query_flags, self._axis_scaling,
                                                   max_regions)
            if remaining == 0:
                return MappingProcessResult.kMprUpToDate
            if time_slice > 0 and time.perf_counter() - start >= time_slice:
                return MappingProcessResult.kMprProgressing

    def calculateForExtents(self, gpu_map, min_extents, max_extents, force=True):
        """ClearanceProcess::calculateForExtents (ohmgpu/ClearanceProcess.cpp:474-510): every region from
        regionKey(min_extents) to regionKey(max_extents) that exists in the map -- every one with kQfInstantiateUnknown,
        without creating it on the device.  Returns the regions computed.  With the clearance layer, the layer of the
        regions present in the map is written as well: every one with force, the stale ones otherwise."""
        m = gpu_map.map()
        rdim = [m.region_voxel_dimensions[i] * m.resolution for i in range(3)]
        lo = [_region_coord(min_extents[i], m.origin[i], rdim[i]) for i in range(3)]
        hi = [_region_coord(max_extents[i], m.origin[i], rdim[i]) for i in range(3)]
        if self._query_flags & self.kQfInstantiateUnknown:
            keys = [(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1)
                    for x in range(lo[0], hi[0] + 1)]
        else:
            present = set(tuple(int(v) for v in k) for k in gpu_map.regionKeys())
            keys = [(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1)
                    for x in range(lo[0], hi[0] + 1) if (x, y, z) in present]
        self._region_dim = tuple(m.region_voxel_dimensions)
        if keys:
            out = gpu_map.clearanceRegions(np.array(keys, dtype=np.int16), self._search_radius, self._query_flags,
                                           self._axis_scaling)
            for key, block in zip(keys, out):
                self._results[key] = block
            if gpu_map.hasLayer("clearance"):
                gpu_map.clearanceUpdateRegions(np.array(keys, dtype=np.int16), self._search_radius, self._query_flags,
                                               self._axis_scaling, force=force)
        return keys

    def regionClearance(self, region_key):
        """(dz, dy, dx) float32 of a computed region, None otherwise."""
        return self._results.get(tuple(int(v) for v in region_key))

    def voxelClearance(self, key):
        """The clearance of one voxel, key = (region key, local key), of a computed region; None otherwise."""
        region_key, local_key = key
        block = self.regionClearance(region_key)
        if block is None:
            return None
        return float(block[int(local_key[2]), int(local_key[1]), int(local_key[0])])


class Mapper:
    """ohm::Mapper (ohm/Mapper.h): runs its mapping processes (a ClearanceProcess) over one GpuMap between
    integrateRays batches."""

    def __init__(self, gpu_map=None):
        self._map = gpu_map
        self._processes = []

    def setMap(self, gpu_map):
        self._map = gpu_map

    def map(self):
        return self._map

    def addProcess(self, process):
        self._processes.append(process)

    def processes(self):
        return list(self._processes)

    def update(self, time_slice=0.0, max_regions=0):
        """Mapper::update: each process in turn shares time_slice seconds (<= 0: run each until it is up to date).
        Returns kMprUpToDate when every process is."""
        start = time.perf_counter()
        result = MappingProcessResult.kMprUpToDate
        if self._map is None:
            return result
        for process in self._processes:
            left = 0.0
            if time_slice > 0:
                left = time_slice - (time.perf_counter() - start)
                if left <= 0:
                    return MappingProcessResult.kMprProgressing
            if process.update(self._map, left, max_regions) != MappingProcessResult.kMprUpToDate:
                result = MappingProcessResult.kMprProgressing
        return result


class LineQueryGpu:
    """ohm::LineQueryGpu (ohmgpu/LineQueryGpu.{h,cpp}; interface of ohm/LineQuery.h): the voxels a line segment passes
    through and the clearance of each -- how close the path passes to an obstacle.  Composed of the device line walk
    (GpuMap.lineKeys, calculateSegmentKeys' keys) and the device clearance of those keys (GpuMap.clearanceKeys), with
    LineQueryGpu::onExecute's post-processing: a voxel outside every region of the map, or with no obstruction within
    the search radius (-1), reports defaultRange(); kQfUnknownAsOccupied is passed on to the clearance (and nothing
    else: the reference's GPU query ignores kQfReportUnscaledResults).  With kQfNearestResult only the voxel of the
    smallest range is kept, chosen as the GPU query chooses it: the first voxel, then any later one with range >= 0 and
    (range < closest or closest < 0).  The CPU LineQuery selects differently -- `range * range < closest`
    (ohm/LineQuery.cpp:75-84), so a default range of -1 counts as 1 there -- and is not what this class follows."""

    def __init__(self, gpu_map, start_point=(0.0, 0.0, 0.0), end_point=(0.0, 0.0, 0.0), search_radius=0.0,
                 query_flags=0):
        self._gpu_map = gpu_map
        self._start = tuple(float(v) for v in start_point)
        self._end = tuple(float(v) for v in end_point)
        self._search_radius = float(search_radius)
        self._query_flags = int(query_flags) | int(QueryFlag.kQfGpuEvaluate)
        self._default_range = -1.0
        self._axis_scaling = (1.0, 1.0, 1.0)
        self.reset()

    def startPoint(self):
        return self._start

    def setStartPoint(self, point):
        self._start = tuple(float(v) for v in point)

    def endPoint(self):
        return self._end

    def setEndPoint(self, point):
        self._end = tuple(float(v) for v in point)

    def searchRadius(self):
        return self._search_radius

    def setSearchRadius(self, radius):
        self._search_radius = float(radius)

    def defaultRange(self):
        return self._default_range

    def setDefaultRange(self, value):
        self._default_range = float(np.float32(value))

    def axisScaling(self):
        return self._axis_scaling

    def setAxisScaling(self, scaling):
        self._axis_scaling = tuple(float(v) for v in scaling)

    def queryFlags(self):
        return self._query_flags

    def setQueryFlags(self, flags):
        self._query_flags = int(flags) | int(QueryFlag.kQfGpuEvaluate)

    def reset(self, hard_reset=True):
        self._regions = np.zeros((0, 3), dtype=np.int16)
        self._locals = np.zeros((0, 3), dtype=np.uint8)
        self._ranges = np.zeros(0, dtype=np.float32)
        self._number_of_results = 0

    def execute(self):
        self.reset(False)
        gm = self._gpu_map
        res = gm.map().resolution
        start = np.array(self._start, dtype=np.float64)
        end = np.array(self._end, dtype=np.float64)
        length = float(np.linalg.norm(end - start))
        max_keys = int(math.ceil(length / res * math.sqrt(3.0))) + 4
        regions, voxels, counts = gm.lineKeys(np.array([start, end]), max_keys_per_line=max_keys)
        n = int(min(int(counts[0]), max_keys))
        regions = np.ascontiguousarray(regions[0, :n])
        locals_ = np.ascontiguousarray(voxels[0, :n])
        flags = int(QueryFlag.kQfUnknownAsOccupied) if self._query_flags & QueryFlag.kQfUnknownAsOccupied else 0
        ranges = gm.clearanceKeys((regions, locals_), self._search_radius, flags, self._axis_scaling)
        present = set(tuple(int(v) for v in k) for k in gm.regionKeys())
        known = np.array([tuple(int(v) for v in r) in present for r in regions], dtype=bool)
        ranges = np.where(known & (ranges >= 0), ranges, np.float32(self._default_range)).astype(np.float32)
        if (self._query_flags & QueryFlag.kQfNearestResult) and n:
            closest_index, closest = 0, np.float32(-1.0)
            for i in range(n):
                r = ranges[i]
                if i == 0 or (r >= 0 and (r < closest or closest < 0)):
                    closest_index, closest = i, r
            regions = regions[closest_index:closest_index + 1]
            locals_ = locals_[closest_index:closest_index + 1]
            ranges = ranges[closest_index:closest_index + 1]
        self._regions, self._locals, self._ranges = regions.copy(), locals_.copy(), ranges.copy()
        self._number_of_results = int(ranges.shape[0])
        return True

    def executeAsync(self):
        """The device calls are synchronous: the asynchronous forms complete at once (ohm/Query.h:103-121)."""
        return self.execute()

    def wait(self, timeout_ms=0xffffffff):
        return True

    def numberOfResults(self):
        return self._number_of_results

    def intersectedVoxels(self):
        """(regions (K, 3) int16, local keys (K, 3) uint8) in walk order (one with kQfNearestResult)."""
        return self._regions, self._locals

    def ranges(self):
        return self._ranges


class NearestNeighbours:
    """ohm::NearestNeighbours (ohm/NearestNeighbours.h) against the device-resident map: the obstructing voxels within
    search_radius of near_point, or with kQfNearestResult the closest one -- the CPU query's results in its order
    (GpuMap.nearestNeighbours).  Ranges are float results widened to double, as the reference stores them."""

    def __init__(self, gpu_map, near_point=(0.0, 0.0, 0.0), search_radius=0.0, query_flags=0):
        self._map = gpu_map
        self._near_point = tuple(float(v) for v in near_point)
        self._search_radius = float(np.float32(search_radius))
        self._flags = int(query_flags)
        self.reset()

    def nearPoint(self):
        return self._near_point

    def setNearPoint(self, point):
        self._near_point = tuple(float(v) for v in point)

    def searchRadius(self):
        return self._search_radius

    def setSearchRadius(self, radius):
        self._search_radius = float(np.float32(radius))

    def queryFlags(self):
        return self._flags

    def setQueryFlags(self, flags):
        self._flags = int(flags)

    def reset(self, hard_reset=True):
        self._keys = np.zeros(0, dtype=_GPU_KEY)
        self._ranges = np.zeros(0, dtype=np.float64)

    def execute(self):
        self.reset()
        if self._map is None:
            return False
        honoured = int(QueryFlag.kQfUnknownAsOccupied | QueryFlag.kQfNearestResult)
        _, keys, ranges = self._map.nearestNeighbours([self._near_point], self._search_radius, self._flags & honoured)
        self._keys = keys
        self._ranges = ranges.astype(np.float64)
        return True

    def executeAsync(self):
        return False  # as the reference's CPU query (ohm/NearestNeighbours.cpp:287-290)

    def wait(self, timeout_ms=0xffffffff):
        return True

    def numberOfResults(self):
        return int(self._keys.shape[0])

    def intersectedVoxels(self):
        """GPU_KEY_DTYPE records."""
        return self._keys

    def ranges(self):
        return self._ranges
