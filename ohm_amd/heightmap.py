"""ohm::Heightmap (ohmheightmap/Heightmap.h) in planar and simple-fill mode, built on the device from the resident map of
a GpuMap (ohmhip_map_heightmap, ohmhip_map_heightmap_fill: include/ohmhip.h, "HEIGHTMAP").  Only the results cross to
the host: three dense (mb, ma) arrays over the heightmap cells the source's extents cover.  LayeredHeightmap builds the
two layered modes (ohmhip_map_heightmap_layered): the same arrays with a leading slot axis."""
import ctypes as C
import enum

import numpy as np

from . import _lib as L


class UpAxis(enum.IntEnum):
    """ohm::UpAxis (ohmheightmap/UpAxis.h)"""
    kNegZ = -3
    kNegY = -2
    kNegX = -1
    kX = 0
    kY = 1
    kZ = 2


class HeightmapVoxelType(enum.IntEnum):
    """ohm::HeightmapVoxelType (ohmheightmap/HeightmapVoxelType.h)"""
    kUnknown = 0
    kVacant = 1
    kSurface = 2
    kVirtualSurface = 3


class HeightmapMode(enum.IntEnum):
    """ohm::HeightmapMode (ohmheightmap/HeightmapMode.h); Heightmap builds kPlanar and kSimpleFill, LayeredHeightmap the
    two layered modes."""
    kPlanar = 0
    kSimpleFill = 1
    kLayeredFillUnordered = 2
    kLayeredFill = 3


#: ohm::HeightmapVoxel (ohmheightmap/HeightmapVoxel.h:68-97)
HEIGHTMAP_VOXEL_DTYPE = np.dtype([("height", "<f4"), ("clearance", "<f4"), ("normal_x", "<f4"), ("normal_y", "<f4"),
                                  ("normal_z", "<f4"), ("layer", "u1"), ("flags", "u1"),
                                  ("contributing_samples", "<u2")])
kHvfObservedAbove = 1
kNoSourceColumn = 0xFFFFFFFF
kNoSourceVisit = 0xFFFFFFFF


class Heightmap:
    """Heightmap(grid_resolution, min_clearance, up_axis=UpAxis.kZ, region_size=0): the reference's setters are
    properties.  After build_heightmap(): occupancy (float32: +1 surface, -1 virtual surface, +inf nothing), voxels
    (HEIGHTMAP_VOXEL_DTYPE), mean ((mb, ma, 2) uint32 or None), source_column (walk index of the source column that
    wrote the cell), populated_count, cell_count, extents (the _lib.HeightmapExtents of the build).
    mode = HeightmapMode.kSimpleFill builds the flood fill: source_visit (sequence number of the visit that wrote the
    cell) stands in place of source_column, fill_stats is the _lib.HeightmapFillStats of the build and, with
    keep_visit_log set, visit_log the (visits, 3) uint32 array ia, ib, h of every visit in the reference's FIFO order."""

    kDefaultRegionSize = 128

    def __init__(self, grid_resolution, min_clearance, up_axis=UpAxis.kZ, region_size=0):
        self.grid_resolution = float(grid_resolution)
        self.min_clearance = float(min_clearance)
        self.up_axis = UpAxis(int(up_axis))
        self.region_size = int(region_size) if region_size else self.kDefaultRegionSize
        self.ceiling = 0.0
        self.floor = 0.0
        self.ignore_voxel_mean = False
        self.generate_virtual_surface = False
        self.promote_virtual_below = False
        #: surface normals of occupied cells from the source's covariance layer (OHMHIP_HM_SURFACE_NORMALS): what the
        #: reference always computes on an NDT map; off, normal_x / y / z stay 0
        self.surface_normals = False
        self.mode = HeightmapMode.kPlanar
        self.keep_visit_log = False
        self.heightmap_origin = (0.0, 0.0, 0.0)
        self._gpu_map = None
        self._clear()

    def _clear(self):
        self.occupancy = self.voxels = self.mean = self.source_column = None
        self.source_visit = self.visit_log = self.fill_stats = None
        self.populated_count = 0
        self.cell_count = 0
        self.extents = None

    def set_occupancy_map(self, gpu_map):
        self._gpu_map = gpu_map

    def up_axis_index(self):
        return int(self.up_axis) if self.up_axis >= 0 else -int(self.up_axis) - 1

    def up_axis_normal(self):
        n = [0.0, 0.0, 0.0]
        n[self.up_axis_index()] = 1.0 if self.up_axis >= 0 else -1.0
        return tuple(n)

    def surface_axis_indices(self):
        """heightmapAxisIndices (ohmheightmap/HeightmapUtil.cpp:86-116): (a, b)."""
        return {0: (1, 2), 1: (0, 2), 2: (0, 1)}[self.up_axis_index()]

    def params(self, reference_pos, cull_to=None):
        p = L.HeightmapParams()
        for i in range(3):
            p.reference_pos[i] = float(reference_pos[i])
            p.origin[i] = float(self.heightmap_origin[i])
            if cull_to is not None:
                p.cull_min[i] = float(cull_to[0][i])
                p.cull_max[i] = float(cull_to[1][i])
        p.grid_resolution = self.grid_resolution
        p.region_size = 0 if self.region_size == self.kDefaultRegionSize else self.region_size
        p.up_axis = int(self.up_axis)
        p.mode = int(self.mode)
        p.floor, p.ceiling, p.min_clearance = float(self.floor), float(self.ceiling), float(self.min_clearance)
        p.flags = ((L.HM_GENERATE_VIRTUAL_SURFACE if self.generate_virtual_surface else 0) |
                   (L.HM_PROMOTE_VIRTUAL_BELOW if self.promote_virtual_below else 0) |
                   (L.HM_IGNORE_VOXEL_MEAN if self.ignore_voxel_mean else 0) |
                   (L.HM_SURFACE_NORMALS if self.surface_normals else 0))
        return p

    def build_heightmap(self, reference_pos, cull_to=None):
        """Heightmap::buildHeightmap (ohmheightmap/Heightmap.cpp:335-412); cull_to = (min, max) or None.  True when
        any cell was populated."""
        self._clear()
        if self._gpu_map is None:
            return False
        handle = self._gpu_map._handle
        p = self.params(reference_pos, cull_to)
        if self.mode == HeightmapMode.kSimpleFill:
            return self._build_fill(handle, p)
        e = L.HeightmapExtents()
        L.check(L.lib.ohmhip_map_heightmap_extents(handle, C.byref(p), C.byref(e)), "ohmhip_map_heightmap_extents")
        self.extents = e
        if not e.populated:
            return False
        shape = (int(e.mb), int(e.ma))
        self.occupancy = np.empty(shape, dtype=np.float32)
        self.voxels = np.empty(shape, dtype=HEIGHTMAP_VOXEL_DTYPE)
        self.mean = np.empty(shape + (2,), dtype=np.uint32) if e.use_mean else None
        self.source_column = np.empty(shape, dtype=np.uint32)
        populated, cells = C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib.ohmhip_map_heightmap(handle, C.byref(p), self.occupancy.ctypes.data, self.voxels.ctypes.data,
                                           self.mean.ctypes.data if self.mean is not None else None,
                                           self.source_column.ctypes.data, C.byref(populated), C.byref(cells)),
                "ohmhip_map_heightmap")
        self.populated_count = int(populated.value)
        self.cell_count = int(cells.value)
        return self.populated_count != 0

    def _build_fill(self, handle, p):
        e = L.HeightmapExtents()
        L.check(L.lib.ohmhip_map_heightmap_fill_extents(handle, C.byref(p), C.byref(e)),
                "ohmhip_map_heightmap_fill_extents")
        self.extents = e
        if not e.populated:
            return False
        shape = (int(e.mb), int(e.ma))
        self.occupancy = np.empty(shape, dtype=np.float32)
        self.voxels = np.empty(shape, dtype=HEIGHTMAP_VOXEL_DTYPE)
        self.mean = np.empty(shape + (2,), dtype=np.uint32) if e.use_mean else None
        self.source_visit = np.empty(shape, dtype=np.uint32)
        stats = L.HeightmapFillStats()
        # the number of visits is known after the walk: a log too small for it is fetched by a second build
        capacity = 4 * int(e.na) * int(e.nb) if self.keep_visit_log else 0
        while True:
            log = np.empty((capacity, 3), dtype=np.uint32) if capacity else None
            L.check(L.lib.ohmhip_map_heightmap_fill(handle, C.byref(p), self.occupancy.ctypes.data,
                                                    self.voxels.ctypes.data,
                                                    self.mean.ctypes.data if self.mean is not None else None,
                                                    self.source_visit.ctypes.data,
                                                    log.ctypes.data if log is not None else None, capacity,
                                                    C.byref(stats)), "ohmhip_map_heightmap_fill")
            if log is None or int(stats.visits) <= capacity:
                break
            capacity = int(stats.visits)
        self.fill_stats = stats
        self.visit_log = log[:int(stats.visits)].copy() if log is not None else None
        self.populated_count = int(stats.populated)
        self.cell_count = int(stats.cells)
        return self.populated_count != 0

    def _hm_dims(self):
        dims = [self.region_size] * 3
        dims[self.up_axis_index()] = 1
        return dims

    def voxel_centre(self, key):
        """voxelCentreGlobal of the heightmap's own OccupancyMap (ohm/OccupancyMap.h:757-778)."""
        region, local = key
        dims = self._hm_dims()
        out = []
        for c in range(3):
            v = float(np.float32(region[c]))
            v *= dims[c] * self.grid_resolution
            v -= 0.5 * (dims[c] * self.grid_resolution)
            v += float(self.heightmap_origin[c])
            v += float(local[c]) * self.grid_resolution
            v += 0.5 * self.grid_resolution
            out.append(v)
        return tuple(out)

    def cell_of_key(self, key):
        """Dense (ca, cb) of heightmap key (region (3), local (3)), or None outside the built grid."""
        if self.extents is None or not self.extents.populated:
            return None
        a, b = self.surface_axis_indices()
        e = self.extents
        region, local = key
        ca = (region[a] - e.first_region[0]) * self.region_size + local[a] - e.first_local[0]
        cb = (region[b] - e.first_region[1]) * self.region_size + local[b] - e.first_local[1]
        if 0 <= ca < e.ma and 0 <= cb < e.mb:
            return int(ca), int(cb)
        return None

    def get_heightmap_voxel_info(self, key):
        """Heightmap::getHeightmapVoxelInfo (ohmheightmap/Heightmap.cpp:415-461): (HeightmapVoxelType, pos, voxel)."""
        cell = self.cell_of_key(key)
        if cell is None:
            return HeightmapVoxelType.kUnknown, None, None
        ca, cb = cell
        up = self.up_axis_index()
        region = list(key[0])
        local = list(key[1])
        region[up] = 0
        local[up] = 0
        centre = self.voxel_centre((region, local))
        occ = self.occupancy[cb, ca]
        if occ == np.float32(np.inf):
            return HeightmapVoxelType.kUnknown, centre, None
        voxel = self.voxels[cb, ca]
        n = self.up_axis_normal()
        pos = tuple(centre[c] + n[c] * float(voxel["height"]) for c in range(3))
        if occ == 0:
            return HeightmapVoxelType.kVacant, pos, voxel
        return (HeightmapVoxelType.kSurface if occ > 0 else HeightmapVoxelType.kVirtualSurface), pos, voxel


#: HeightmapVoxelLayer (ohmheightmap/HeightmapVoxel.h:17-28)
kHvlBaseLayer, kHvlExtended, kHvlInvalid = 0, 1, 2


class LayeredHeightmap(Heightmap):
    """Heightmap in HeightmapMode.kLayeredFill (the default here) or kLayeredFillUnordered: rules L1-L7 of
    include/ohmhip.h.  After build_heightmap(): occupancy, voxels, mean and source_visit as (slots, mb, ma) arrays --
    slot k of a column is the heightmap voxel at the cell's key moved k steps along the raw up axis, empty slots hold
    +inf / zeros / 0xffffffff --, layer_count (mb, ma) uint8, layered_stats (the _lib.HeightmapLayeredStats of the build)
    and, with keep_visit_log set, visit_log.  slots is at least 1 and otherwise what the tallest column needed.
    Modes kPlanar and kSimpleFill are the parent's."""

    kInitialLayerCapacity = 4

    def __init__(self, grid_resolution, min_clearance, up_axis=UpAxis.kZ, region_size=0):
        super().__init__(grid_resolution, min_clearance, up_axis, region_size)
        self.mode = HeightmapMode.kLayeredFill
        self._virtual_surface_filter_threshold = 0

    @property
    def virtual_surface_filter_threshold(self):
        """Heightmap::virtualSurfaceFilterThreshold: 0 is off; applied in kLayeredFill only."""
        return self._virtual_surface_filter_threshold

    @virtual_surface_filter_threshold.setter
    def virtual_surface_filter_threshold(self, value):
        value = int(value)
        if not 0 <= value <= 0xFFFFFFFF:
            raise ValueError("virtual_surface_filter_threshold is an unsigned 32 bit count")
        self._virtual_surface_filter_threshold = value

    def _clear(self):
        super()._clear()
        self.layer_count = self.layered_stats = None

    def layered_params(self, reference_pos, cull_to=None):
        p = L.HeightmapLayeredParams()
        p.base = self.params(reference_pos, cull_to)
        p.virtual_surface_filter_threshold = self._virtual_surface_filter_threshold
        return p

    def build_heightmap(self, reference_pos, cull_to=None):
        if self.mode not in (HeightmapMode.kLayeredFill, HeightmapMode.kLayeredFillUnordered):
            return super().build_heightmap(reference_pos, cull_to)
        self._clear()
        if self._gpu_map is None:
            return False
        handle = self._gpu_map._handle
        p = self.layered_params(reference_pos, cull_to)
        e = L.HeightmapExtents()
        L.check(L.lib.ohmhip_map_heightmap_layered_extents(handle, C.byref(p), C.byref(e)),
                "ohmhip_map_heightmap_layered_extents")
        self.extents = e
        if not e.populated:
            return False
        plane = (int(e.mb), int(e.ma))
        stats = L.HeightmapLayeredStats()
        # the slots and the visits are known after the walk: what was too small is fetched by a second build
        slots = self.kInitialLayerCapacity
        capacity = 4 * int(e.na) * int(e.nb) if self.keep_visit_log else 0
        while True:
            shape = (slots,) + plane
            occupancy = np.empty(shape, dtype=np.float32)
            voxels = np.empty(shape, dtype=HEIGHTMAP_VOXEL_DTYPE)
            mean = np.empty(shape + (2,), dtype=np.uint32) if e.use_mean else None
            source_visit = np.empty(shape, dtype=np.uint32)
            layer_count = np.empty(plane, dtype=np.uint8)
            log = np.empty((capacity, 3), dtype=np.uint32) if capacity else None
            L.check(L.lib.ohmhip_map_heightmap_layered(handle, C.byref(p), slots, occupancy.ctypes.data,
                                                       voxels.ctypes.data,
                                                       mean.ctypes.data if mean is not None else None,
                                                       source_visit.ctypes.data, layer_count.ctypes.data,
                                                       log.ctypes.data if log is not None else None, capacity,
                                                       C.byref(stats)), "ohmhip_map_heightmap_layered")
            if int(stats.layers) <= slots and (log is None or int(stats.visits) <= capacity):
                break
            slots = max(slots, int(stats.layers))
            capacity = max(capacity, int(stats.visits)) if log is not None else 0
        keep = max(1, int(stats.layers))
        self.occupancy, self.voxels = occupancy[:keep].copy(), voxels[:keep].copy()
        self.mean = mean[:keep].copy() if mean is not None else None
        self.source_visit, self.layer_count = source_visit[:keep].copy(), layer_count
        self.layered_stats = stats
        self.visit_log = log[:int(stats.visits)].copy() if log is not None else None
        self.populated_count = int(stats.populated)
        self.cell_count = int(stats.cells)
        return self.populated_count != 0

    def get_heightmap_voxel_info(self, key):
        """Heightmap::getHeightmapVoxelInfo: the key's up-axis coordinate (region * 1 + local) is the slot."""
        if self.occupancy is None or self.occupancy.ndim != 3:
            return super().get_heightmap_voxel_info(key)
        cell = self.cell_of_key(key)
        up = self.up_axis_index()
        slot = int(key[0][up]) + int(key[1][up])
        if cell is None or not 0 <= slot < self.occupancy.shape[0]:
            return HeightmapVoxelType.kUnknown, None, None
        ca, cb = cell
        centre = self.voxel_centre(key)
        occ = self.occupancy[slot, cb, ca]
        if occ == np.float32(np.inf):
            return HeightmapVoxelType.kUnknown, centre, None
        voxel = self.voxels[slot, cb, ca]
        n = self.up_axis_normal()
        pos = tuple(centre[c] + n[c] * float(voxel["height"]) for c in range(3))
        if occ == 0:
            return HeightmapVoxelType.kVacant, pos, voxel
        return (HeightmapVoxelType.kSurface if occ > 0 else HeightmapVoxelType.kVirtualSurface), pos, voxel
