"""CPU restatement of calculateNearestNeighbour (ohm/private/VoxelAlgorithms.cpp:22-98) -- TEST INFRASTRUCTURE.  The
device clearance queries (ohmhip_map_clearance_regions / _keys) are held to it at exact equality.

Per target voxel v, as the CPU writes it: v itself obstructing -> 0; otherwise every neighbour moveKey(v, x, y, z) for
x, y, z in [-h, h] (z outermost, x innermost; the region key adds in int16 and wraps, ohm/private/
OccupancyMapDetail.cpp:27-93), h = int(ceil(double(radius) / resolution)).  A neighbour obstructs when its region exists
and value != +inf and value >= threshold (isOccupied, ohm/VoxelOccupancy.h:161), or, with unknown_as_occupied, when it is
unobserved or in no region.  Arithmetic in float32 with rounding after every operation: the centres are the fp64
voxelCentre (ohm/OccupancyMap.h:757-777, origin 0) rounded to float; sep = c(n) - c(v); r2 = (x*x + y*y) + z*z; the same
of sep * axis_scaling is s2; r2 = s2 unless report_unscaled; counted when radius == 0 or r2 <= radius * radius; taken
when s2 < the best s2 (strictly: ties go to the earliest in scan order).  Result sqrt(r2) of the one taken, -1 if none.

Two evaluations, both exact: offsets outermost over a whole region (cheap for small windows) and targets outermost over
the candidates of each window (cheap for large windows); clearance_regions picks by cost."""
import math

import numpy as np

QF_UNKNOWN_AS_OCCUPIED = 1 << 0
QF_REPORT_UNSCALED = 1 << 4
F32_INF = np.float32(np.inf)


class DictBlocks:
    """Occupancy blocks of a {region: flat float32 block} dict (crafted maps)."""

    def __init__(self, blocks):
        self._blocks = {tuple(int(v) for v in k): np.asarray(b, dtype=np.float32).reshape(-1) for k, b in blocks.items()}

    def __call__(self, region):
        return self._blocks.get(tuple(int(v) for v in region))


def half_extent(search_radius, resolution):
    """calculateVoxelSearchHalfExtents (VoxelAlgorithms.cpp:16): float radius / double resolution, ceil."""
    return int(math.ceil(float(np.float32(search_radius)) / float(resolution)))


def move(r, l, step, kd):
    """moveKeyAlongAxis on one axis: (region, local) of local key l of region r moved by step (int16 region wrap)."""
    ll = l + step
    q = ll // kd
    return (r + q + 32768) % 65536 - 32768, ll - q * kd


def centre(r, l, resolution, kd):
    """One component of glm::vec3(map.voxelCentreLocal(key)), fp64 in voxelCentre's order, origin 0."""
    rsd = kd * resolution
    c = float(np.float32(r))
    c = c * rsd
    c = c - 0.5 * rsd
    c = c + float(l) * resolution
    c = c + 0.5 * resolution
    return np.float32(c)


class Geometry:
    def __init__(self, resolution, region_dim, threshold):
        self.resolution = float(resolution)
        self.kd = tuple(int(v) for v in region_dim)
        self.threshold = np.float32(threshold)


def _axis(geom, axis, r, l0, n):
    """Per-axis arrays of n consecutive coordinates starting at local l0 of region r: regions, locals, centres."""
    kd = geom.kd[axis]
    rr = np.empty(n, dtype=np.int64)
    ll = np.empty(n, dtype=np.int64)
    cc = np.empty(n, dtype=np.float32)
    for i in range(n):
        rr[i], ll[i] = move(r, 0, l0 + i, kd)
        cc[i] = centre(rr[i], ll[i], geom.resolution, kd)
    return rr, ll, cc


def _candidates(geom, blocks, ax, unknown_as_occupied):
    """Candidate mask [z][y][x] over the box spanned by the per-axis (regions, locals) arrays ax[0..2]."""
    (rx, lx, _), (ry, ly, _), (rz, lz, _) = ax
    dx, dy, _ = geom.kd
    out = np.zeros((len(rz), len(ry), len(rx)), dtype=bool)
    for zr in np.unique(rz):
        zi = np.nonzero(rz == zr)[0]
        for yr in np.unique(ry):
            yi = np.nonzero(ry == yr)[0]
            for xr in np.unique(rx):
                xi = np.nonzero(rx == xr)[0]
                block = blocks((int(xr), int(yr), int(zr)))
                if block is None:
                    out[np.ix_(zi, yi, xi)] = bool(unknown_as_occupied)
                    continue
                idx = lx[xi][None, None, :] + ly[yi][None, :, None] * dx + lz[zi][:, None, None] * dx * dy
                v = np.asarray(block, dtype=np.float32)[idx]
                unobserved = v == F32_INF
                occupied = (~unobserved) & (v >= geom.threshold)
                out[np.ix_(zi, yi, xi)] = occupied | (unobserved & bool(unknown_as_occupied))
    return out


def _select(ex, ey, ez, scale, radius, report_unscaled):
    """Vectors of separations of candidates in scan order -> the CPU's selection: (s2, r2) of the one taken or None."""
    r2 = (ex * ex + ey * ey) + ez * ez
    sx, sy, sz = ex * scale[0], ey * scale[1], ez * scale[2]
    s2 = (sx * sx + sy * sy) + sz * sz
    if not report_unscaled:
        r2 = s2
    ok = (radius == np.float32(0)) | (r2 <= radius * radius)
    masked = np.where(ok, s2, F32_INF)
    if masked.size == 0:
        return None
    i = int(np.argmin(masked))  # first of the smallest: the CPU's strict `<` over its scan order
    if not masked[i] < F32_INF:
        return None
    return r2[i]


def _result(r2):
    return np.float32(-1.0) if r2 is None or not r2 < F32_INF else np.sqrt(np.float32(r2))


def _window(geom, blocks, region, local, h, uao):
    ax = [_axis(geom, a, int(region[a]), int(local[a]) - h, 2 * h + 1) for a in range(3)]
    return ax, _candidates(geom, blocks, ax, uao)


def clearance_keys(geom, blocks, regions, locals_, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0)):
    """Clearance of each voxel (regions (N, 3), locals (N, 3)): (N,) float32."""
    h = half_extent(search_radius, geom.resolution)
    uao = bool(flags & QF_UNKNOWN_AS_OCCUPIED)
    unscaled = bool(flags & QF_REPORT_UNSCALED)
    radius = np.float32(search_radius)
    scale = [np.float32(v) for v in axis_scaling]
    regions = np.asarray(regions).reshape(-1, 3)
    locals_ = np.asarray(locals_).reshape(-1, 3)
    out = np.empty(regions.shape[0], dtype=np.float32)
    for i in range(regions.shape[0]):
        ax, cand = _window(geom, blocks, regions[i], locals_[i], h, uao)
        out[i] = _target(ax, cand, h, h, h, h, scale, radius, unscaled)
    return out


def _target(ax, cand, h, px, py, pz, scale, radius, unscaled):
    """The target at padded coordinates (px, py, pz) of the per-axis arrays / candidate box."""
    if cand[pz, py, px]:
        return np.float32(0.0)
    sub = cand[pz - h:pz + h + 1, py - h:py + h + 1, px - h:px + h + 1]
    z, y, x = np.nonzero(sub)  # C order: z, y, x ascending = the CPU's scan order
    cx, cy, cz = ax[0][2], ax[1][2], ax[2][2]
    ex = cx[px - h + x] - cx[px]
    ey = cy[py - h + y] - cy[py]
    ez = cz[pz - h + z] - cz[pz]
    return _result(_select(ex, ey, ez, scale, radius, unscaled))


def clearance_regions(geom, blocks, regions, search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0), method=None):
    """Every voxel of each region: (N, dz, dy, dx) float32.  method: None (by cost), "offsets" or "targets"."""
    h = half_extent(search_radius, geom.resolution)
    uao = bool(flags & QF_UNKNOWN_AS_OCCUPIED)
    unscaled = bool(flags & QF_REPORT_UNSCALED)
    radius = np.float32(search_radius)
    scale = [np.float32(v) for v in axis_scaling]
    dx, dy, dz = geom.kd
    regions = np.asarray(regions).reshape(-1, 3)
    out = np.empty((regions.shape[0], dz, dy, dx), dtype=np.float32)
    if method is None:
        method = "offsets" if (2 * h + 1) ** 3 <= 4 * dx * dy * dz else "targets"
    for n, region in enumerate(regions):
        ax = [_axis(geom, a, int(region[a]), -h, geom.kd[a] + 2 * h) for a in range(3)]
        cand = _candidates(geom, blocks, ax, uao)
        if method == "targets":
            for z in range(dz):
                for y in range(dy):
                    for x in range(dx):
                        out[n, z, y, x] = _target(ax, cand, h, x + h, y + h, z + h, scale, radius, unscaled)
            continue
        cx, cy, cz = ax[0][2], ax[1][2], ax[2][2]
        c0x = cx[h:h + dx][None, None, :]
        c0y = cy[h:h + dy][None, :, None]
        c0z = cz[h:h + dz][:, None, None]
        best_s2 = np.full((dz, dy, dx), F32_INF, dtype=np.float32)
        best_r2 = np.full((dz, dy, dx), F32_INF, dtype=np.float32)
        for oz in range(2 * h + 1):
            ez = cz[oz:oz + dz][:, None, None] - c0z
            for oy in range(2 * h + 1):
                ey = cy[oy:oy + dy][None, :, None] - c0y
                for ox in range(2 * h + 1):
                    c = cand[oz:oz + dz, oy:oy + dy, ox:ox + dx]
                    if not c.any():
                        continue
                    ex = cx[ox:ox + dx][None, None, :] - c0x
                    r2 = (ex * ex + ey * ey) + ez * ez
                    sx, sy, sz = ex * scale[0], ey * scale[1], ez * scale[2]
                    s2 = (sx * sx + sy * sy) + sz * sz
                    if not unscaled:
                        r2 = s2
                    take = c & ((radius == np.float32(0)) | (r2 <= radius * radius)) & (s2 < best_s2)
                    best_s2 = np.where(take, s2, best_s2)
                    best_r2 = np.where(take, r2, best_r2)
        res = np.where(best_r2 < F32_INF, np.sqrt(best_r2), np.float32(-1.0)).astype(np.float32)
        res[cand[h:h + dz, h:h + dy, h:h + dx]] = np.float32(0.0)
        out[n] = res
    return out
