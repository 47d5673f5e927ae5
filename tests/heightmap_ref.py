"""CPU restatement of the planar heightmap, ohm::Heightmap::buildHeightmap in HeightmapMode::kPlanar -- TEST
INFRASTRUCTURE.  The device heightmap (ohmhip_map_heightmap) is held to it at exact equality, every cell, every field.

Written from the reference line by line; the rule numbers are those of the heightmap block of include/ohmhip.h:
  1 extents   ohmheightmap/Heightmap.cpp:349-365, ohm/OccupancyMap.cpp:397-459
  2 walk      ohmheightmap/PlaneWalker.cpp:24-52, ohmheightmap/HeightmapUtil.cpp:86-116
  3 support   ohmheightmap/private/HeightmapOperations.cpp:186-419
  4 ground    ohmheightmap/private/HeightmapOperations.cpp:422-512
  5 cell      ohmheightmap/Heightmap.cpp:619-671, :703-835
  6 collide   planar mode overwrites: the larger walk index stands
Voxels are addressed by their global voxel coordinate g = region * dim + local per axis; the source map is a
{region: {layer: block}} dict like rays_query_ref.ChunkBlocks takes."""
import ctypes as C
import math

import numpy as np

from oracle.oracle import OracleMap, lib as _olib

K_NULL, K_UNOBSERVED, K_FREE, K_OCCUPIED = -2, -1, 0, 1
HM_UNKNOWN, HM_VACANT, HM_SURFACE, HM_VIRTUAL = 0, 1, 2, 3  # HeightmapVoxelType (ohmheightmap/HeightmapVoxelType.h)
INF32 = np.float32(np.inf)
HVF_OBSERVED_ABOVE = 1
NO_COLUMN = 0xFFFFFFFF

HEIGHTMAP_VOXEL = np.dtype([("height", "<f4"), ("clearance", "<f4"), ("normal_x", "<f4"), ("normal_y", "<f4"),
                            ("normal_z", "<f4"), ("layer", "u1"), ("flags", "u1"), ("contributing_samples", "<u2")])
assert HEIGHTMAP_VOXEL.itemsize == 24  # ohmheightmap/HeightmapVoxel.h:68-97

# findNearestSupportingVoxel flags (private/HeightmapOperations.h:45-63)
F_VIRTUAL, F_BIAS_ABOVE, F_PROMOTE_BELOW, F_IGNORE_VIRTUAL_ABOVE = 1, 2, 4, 8


def axis_indices(up_axis):
    """heightmapAxisIndices (HeightmapUtil.cpp:86-116): (a, b, up index)."""
    up = up_axis if up_axis >= 0 else -up_axis - 1
    return {0: (1, 2, 0), 1: (0, 2, 1), 2: (0, 1, 2)}[up]


def point_to_region_coord(v, res):
    return int(_olib.oracle_point_to_region_coord(float(v), float(res)))


def sub_voxel_to_local(coord, res):
    out = (C.c_double * 3)()
    _olib.oracle_sub_voxel_to_local(int(coord), float(res), out)
    return [out[0], out[1], out[2]]


def sub_voxel_coord(v, res):
    return int(_olib.oracle_sub_voxel_coord((C.c_double * 3)(*[float(x) for x in v]), float(res)))


def dot(p, up):
    return (p[0] * up[0] + p[1] * up[1]) + p[2] * up[2]  # glm::dot


class Params:
    def __init__(self, grid_resolution, min_clearance=0.0, up_axis=2, region_size=0, reference_pos=(0.0, 0.0, 0.0),
                 cull_min=(0.0, 0.0, 0.0), cull_max=(0.0, 0.0, 0.0), origin=(0.0, 0.0, 0.0), floor=0.0, ceiling=0.0,
                 virtual_surface=False, promote_virtual_below=False, ignore_voxel_mean=False):
        self.grid_resolution = float(grid_resolution)
        self.min_clearance = float(min_clearance)
        self.up_axis = int(up_axis)
        self.region_size = int(region_size) if region_size else 128  # Heightmap::kDefaultRegionSize
        self.reference_pos = tuple(float(v) for v in reference_pos)
        self.cull_min = tuple(float(v) for v in cull_min)
        self.cull_max = tuple(float(v) for v in cull_max)
        self.origin = tuple(float(v) for v in origin)
        self.floor = float(floor)
        self.ceiling = float(ceiling)
        self.virtual_surface = bool(virtual_surface)
        self.promote_virtual_below = bool(promote_virtual_below)
        self.ignore_voxel_mean = bool(ignore_voxel_mean)


class Source:
    """The source map: geometry (an OracleMap: voxel_key / voxel_centre), threshold, and the chunks."""

    def __init__(self, resolution, region_dim, chunks, threshold_value, origin=(0.0, 0.0, 0.0), has_mean=None):
        self.resolution = float(resolution)
        self.dim = tuple(int(v) for v in region_dim)
        self.origin = tuple(float(v) for v in origin)
        self.om = OracleMap(resolution, self.dim)
        self.om.set_origin(self.origin)
        self.threshold = np.float32(threshold_value)
        self.chunks = {tuple(int(v) for v in k): c for k, c in chunks.items()}
        if has_mean is None:
            has_mean = any("mean" in c for c in self.chunks.values())
        self.has_mean = bool(has_mean)
        self.inspected = 0  # occupancy reads of rules 3 and 4

    def split(self, g):
        return tuple(g[a] // self.dim[a] for a in range(3)), tuple(g[a] % self.dim[a] for a in range(3))

    def to_global(self, key):
        return [key[0][a] * self.dim[a] + key[1][a] for a in range(3)]

    def voxel(self, g):
        """(has chunk, occupancy value): a voxel of a missing region reads +inf."""
        region, local = self.split(g)
        c = self.chunks.get(region)
        self.inspected += 1
        if c is None:
            return False, INF32
        vi = local[0] + local[1] * self.dim[0] + local[2] * self.dim[0] * self.dim[1]
        return True, np.float32(np.asarray(c["occupancy"]).reshape(-1)[vi])

    def mean(self, g):
        region, local = self.split(g)
        c = self.chunks.get(region)
        if c is None or "mean" not in c:
            return None
        vi = local[0] + local[1] * self.dim[0] + local[2] * self.dim[0] * self.dim[1]
        m = np.asarray(c["mean"], dtype=np.uint32).reshape(-1, 2)[vi]
        return int(m[0]), int(m[1])

    def occupancy_type(self, g):
        """SrcVoxel::occupancyType (private/HeightmapOperations.h:94-108)."""
        has, v = self.voxel(g)
        if not has:
            return K_NULL
        if v == INF32:
            return K_UNOBSERVED
        return K_OCCUPIED if v >= self.threshold else K_FREE

    def centre(self, g):
        region, local = self.split(g)
        return list(self.om.voxel_centre(region, local))

    def position(self, g, use_mean):
        """SrcVoxel::position (:111-125): the centre plus the decoded mean (a never written coord of 0 decodes too)."""
        pos = self.centre(g)
        if use_mean:
            m = self.mean(g)
            if m is not None:
                off = sub_voxel_to_local(m[0], self.resolution)
                pos = [pos[a] + off[a] for a in range(3)]
        return pos


def extents(src, p):
    """Rule 1: (min_ext global voxel, max_ext global voxel) or None for an empty map / a null key."""
    if not src.chunks:
        return None
    rd = [src.dim[a] * src.resolution for a in range(3)]  # regionSpatialResolution
    lo = [min(r[a] * rd[a] - 0.5 * rd[a] for r in src.chunks) for a in range(3)]  # MapRegion::centre holds no origin
    hi = [max(r[a] * rd[a] + 0.5 * rd[a] for r in src.chunks) for a in range(3)]
    for a in range(3):
        if p.cull_max[a] - p.cull_min[a] > 0:
            lo[a], hi[a] = p.cull_min[a], p.cull_max[a]
    kmin, kmax = src.om.voxel_key(lo), src.om.voxel_key(hi)
    if kmin is None or kmax is None:
        return None
    return src.to_global(kmin), src.to_global(kmax)


def _search(src, seed, to, up, step_limit, search_up, flags):
    """findNearestSupportingVoxel2 (:186-343): (key or None, offset, is_virtual)."""
    allow_virtual = (flags & F_VIRTUAL) != 0
    vertical_range = (to[up] - seed[up]) + 1  # rangeBetween(from, to)[up] + 1
    step = 1 if vertical_range >= 0 else -1
    vertical_range = abs(vertical_range)
    if step_limit > 0:
        vertical_range = min(vertical_range, step_limit)
    best_virtual = None
    last_unobserved = last_free = False
    last_key = None
    cur = list(seed)
    if search_up:
        _, v = src.voxel(seed)
        last_unobserved = bool(v == INF32)  # isUnobservedOrNull
        last_key = list(seed)
        cur[up] += step
    else:
        vertical_range += 1
    offset = 0
    dim_up = src.dim[up]
    i = 0
    while i < vertical_range:
        offset = (i + 1) if i > 0 else (0 if search_up else 1)
        has, v = src.voxel(cur)
        occupied = bool(v >= src.threshold and v != INF32)
        free = bool(v < src.threshold)
        unobserved = not occupied and not free
        if occupied:
            return list(cur), offset, False
        if allow_virtual and search_up and free and last_unobserved and best_virtual is None:
            best_virtual = last_key
        if allow_virtual and not search_up and unobserved and last_free:
            best_virtual = list(cur)
        last_unobserved, last_free, last_key = unobserved, free, list(cur)
        next_step = step
        if not has:  # :321-328 the jump over a region that does not exist
            local = cur[up] % dim_up
            next_step = (dim_up - local) if step > 0 else -(1 + local)
            i += abs(next_step) - 1
        cur[up] += next_step
        i += 1
    if best_virtual is None:
        offset = -1
    return best_virtual, offset, best_virtual is not None


def supporting_voxel(src, seed, up_axis, min_key, max_key, voxel_floor, voxel_ceiling, clearance_permissive, flags):
    """findNearestSupportingVoxel (:346-419)."""
    up = up_axis if up_axis >= 0 else -up_axis - 1
    down_to = min_key if up_axis >= 0 else max_key
    up_to = max_key if up_axis >= 0 else min_key
    below, offset_below, virtual_below = _search(src, seed, down_to, up, voxel_floor, False, flags)
    above, offset_above, virtual_above = _search(src, seed, up_to, up, voxel_ceiling, True, flags)
    have_below = offset_below >= 0
    have_above = offset_above >= 0
    promote = (flags & F_PROMOTE_BELOW) != 0
    virtual_below = have_below and virtual_below and not promote
    if flags & F_BIAS_ABOVE:
        if have_below and have_above:
            return below if offset_below < offset_above else above
    if have_below and virtual_above and not virtual_below:
        return below
    if have_above and not virtual_above and virtual_below:
        return above
    if flags & F_IGNORE_VIRTUAL_ABOVE:
        if have_below and virtual_above and virtual_below:
            return below
    if have_below and (not have_above or offset_below <= offset_above or
                       (have_below and have_above and not virtual_above and
                        offset_below + offset_above >= clearance_permissive)):
        return below
    return above


def find_ground(src, seed, min_key, max_key, up_axis, up_vec, p, use_mean):
    """findGround (:422-512): None or (ground key, clearance, observed_above)."""
    up = up_axis if up_axis >= 0 else -up_axis - 1
    step_dir = 1 if up_axis >= 0 else -1
    observed_above = False
    column_height = column_clearance_height = float(np.finfo(np.float64).max)
    candidate_type = last_type = K_NULL
    ground_key = None
    key = list(seed)
    while min_key[up] <= key[up] <= max_key[up]:
        voxel_type = src.occupancy_type(key)
        # sourceVoxelHeight (:167-184)
        pos = src.position(key, use_mean) if voxel_type == K_OCCUPIED else src.centre(key)
        height = dot(pos, up_vec)
        last_is_unobserved = last_type in (K_UNOBSERVED, K_NULL)
        observed_above = observed_above or (voxel_type != K_NULL and voxel_type != K_UNOBSERVED)
        if voxel_type == K_OCCUPIED or (p.virtual_surface and last_is_unobserved and voxel_type == K_FREE and
                                        candidate_type == K_NULL):
            if candidate_type != K_NULL:
                column_clearance_height = height
                if column_clearance_height - column_height >= p.min_clearance:
                    break
                column_height = column_clearance_height = height
                ground_key = list(key)
                candidate_type = voxel_type
                observed_above = False
            else:
                ground_key = list(key)
                column_height = column_clearance_height = height
                candidate_type = voxel_type
                observed_above = False
        last_type = voxel_type
        key[up] += step_dir
    if candidate_type != K_NULL:
        return ground_key, column_clearance_height - column_height, observed_above
    return None


class Result:
    pass


def heightmap_geometry(src, p, ext):
    """The heightmap's OracleMap and the dense cell range: (hm, first cell (ga, gb), ma, mb)."""
    a, b, up = axis_indices(p.up_axis)
    dims = [p.region_size] * 3
    dims[up] = 1
    hm = OracleMap(p.grid_resolution, tuple(dims))
    hm.set_origin(p.origin)
    lo = src.centre(ext[0])
    hi = src.centre(ext[1])
    lo = [v - 0.5 * src.resolution for v in lo]
    hi = [v + 0.5 * src.resolution for v in hi]
    lo[up] = hi[up] = 0.0
    klo, khi = hm.voxel_key(lo), hm.voxel_key(hi)
    first = [klo[0][c] * dims[c] + klo[1][c] for c in range(3)]
    last = [khi[0][c] * dims[c] + khi[1][c] for c in range(3)]
    return hm, dims, (first[a], first[b]), last[a] - first[a] + 1, last[b] - first[b] + 1


def build_heightmap(src, p):
    """Rules 1-6.  Returns None for an empty map, else a Result with the dense arrays (mb, ma), `a` fastest:
    occupancy f32 (+inf where nothing was written), voxels HEIGHTMAP_VOXEL, mean (mb, ma, 2) u32 or None,
    source_column u32 (walk index, NO_COLUMN where none), populated, plus na, nb, first_cell, min_ext, max_ext."""
    ext = extents(src, p)
    if ext is None:
        return None
    min_key, max_key = ext
    a, b, up = axis_indices(p.up_axis)
    up_vec = [0.0, 0.0, 0.0]
    up_vec[up] = 1.0 if p.up_axis >= 0 else -1.0
    use_mean = src.has_mean and not p.ignore_voxel_mean
    flags = F_IGNORE_VIRTUAL_ABOVE | (F_VIRTUAL if p.virtual_surface else 0) | \
        (F_PROMOTE_BELOW if p.promote_virtual_below else 0)
    voxel_floor = point_to_region_coord(p.floor, src.resolution)
    voxel_ceiling = point_to_region_coord(p.ceiling, src.resolution)
    clearance_permissive = max(1, point_to_region_coord(p.min_clearance, src.resolution) - 1)
    # rule 2: the plane key, clamped on the up axis (PlaneWalker::begin)
    ref_key = src.om.voxel_key(p.reference_pos)
    if ref_key is None:
        return None
    plane = min(max(src.to_global(ref_key)[up], min_key[up]), max_key[up])
    na = max_key[a] - min_key[a] + 1
    nb = max_key[b] - min_key[b] + 1
    hm, hm_dims, first_cell, ma, mb = heightmap_geometry(src, p, ext)
    res = Result()
    res.min_ext, res.max_ext, res.na, res.nb = min_key, max_key, na, nb
    res.first_cell, res.ma, res.mb = first_cell, ma, mb
    res.occupancy = np.full((mb, ma), np.inf, dtype=np.float32)
    res.voxels = np.zeros((mb, ma), dtype=HEIGHTMAP_VOXEL)
    res.mean = np.zeros((mb, ma, 2), dtype=np.uint32) if use_mean else None
    res.source_column = np.full((mb, ma), NO_COLUMN, dtype=np.uint32)
    res.populated = 0
    if na <= 0 or nb <= 0:
        return res
    for ib in range(nb):
        for ia in range(na):
            walk = [0, 0, 0]
            walk[a], walk[b], walk[up] = min_key[a] + ia, min_key[b] + ib, plane
            candidate = supporting_voxel(src, walk, p.up_axis, min_key, max_key, voxel_floor, voxel_ceiling,
                                         clearance_permissive, flags)
            ground = find_ground(src, candidate, min_key, max_key, p.up_axis, up_vec, p, use_mean) \
                if candidate is not None else None
            ground_key = ground[0] if ground is not None else walk
            voxel_type = src.occupancy_type(ground_key) if candidate is not None else K_NULL  # Heightmap.cpp:637
            if not (voxel_type == K_OCCUPIED or (voxel_type == K_FREE and p.virtual_surface)):
                continue
            pos = src.position(ground_key, use_mean) if voxel_type == K_OCCUPIED else src.centre(ground_key)
            # addSurfaceVoxel (:703-835)
            src_height = dot(up_vec, pos)
            pos[up] = 0.0
            hk = hm.voxel_key(pos)
            assert hk is not None
            hr, hl = list(hk[0]), list(hk[1])
            hr[up], hl[up] = 0, 0  # project()
            centre = hm.voxel_centre(hr, hl)
            ca = hr[a] * hm_dims[a] + hl[a] - first_cell[0]
            cb = hr[b] * hm_dims[b] + hl[b] - first_cell[1]
            assert 0 <= ca < ma and 0 <= cb < mb, (ca, cb, ma, mb)
            res.populated += 1  # rule 6: every write counts, the later one stands
            res.occupancy[cb, ca] = 1.0 if voxel_type == K_OCCUPIED else -1.0
            v = np.zeros((), dtype=HEIGHTMAP_VOXEL)
            v["height"] = np.float32(src_height - dot(centre, up_vec))
            v["clearance"] = np.float32(ground[1]) if ground is not None else np.float32(0.0)
            v["flags"] = HVF_OBSERVED_ABOVE if (ground is not None and ground[2]) else 0
            if use_mean:
                m = src.mean(ground_key)
                v["contributing_samples"] = min(m[1], 0xFFFF) if m is not None else 0
                res.mean[cb, ca, 0] = sub_voxel_coord([pos[c] - centre[c] for c in range(3)], p.grid_resolution)
                res.mean[cb, ca, 1] = 1
            res.voxels[cb, ca] = v
            res.source_column[cb, ca] = ib * na + ia
    return res


def voxel_info(res, src, p, cell):
    """getHeightmapVoxelInfo (Heightmap.cpp:415-461) of dense cell (ca, cb): (HeightmapVoxelType, pos, voxel)."""
    a, b, up = axis_indices(p.up_axis)
    ca, cb = cell
    if not (0 <= ca < res.ma and 0 <= cb < res.mb):
        return HM_UNKNOWN, None, None
    hm, hm_dims, first_cell, _, _ = heightmap_geometry(src, p, (res.min_ext, res.max_ext))
    g = [0, 0, 0]
    g[a], g[b] = first_cell[0] + ca, first_cell[1] + cb
    region = [g[c] // hm_dims[c] for c in range(3)]
    local = [g[c] % hm_dims[c] for c in range(3)]
    centre = hm.voxel_centre(region, local)
    occ = res.occupancy[cb, ca]
    if occ == INF32:
        return HM_UNKNOWN, list(centre), None
    up_vec = [0.0, 0.0, 0.0]
    up_vec[up] = 1.0 if p.up_axis >= 0 else -1.0
    v = res.voxels[cb, ca]
    pos = [centre[c] + up_vec[c] * float(v["height"]) for c in range(3)]
    if occ == 0:
        return HM_VACANT, pos, v
    return (HM_SURFACE if occ > 0 else HM_VIRTUAL), pos, v
