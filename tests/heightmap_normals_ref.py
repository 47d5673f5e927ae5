"""What a heightmap built with surface normals must hold in normal_x / y / z (include/ohmhip.h, HEIGHTMAP: SURFACE
NORMALS), from the existing restatement's own functions (tests/heightmap_ref.py) and the decomposition model
(tests/covariance_eigen_ref.py): the ground voxel of a cell's winning source column is re-derived by supporting_voxel
and find_ground exactly as build_heightmap calls them, and an OCCUPIED ground voxel's covariance goes through D1-D6 and
the flip towards up.  Every other cell holds zeros."""
import numpy as np

import covariance_eigen_ref as cov_ref
import heightmap_ref as R


def up_vector(up_axis):
    up = up_axis if up_axis >= 0 else -up_axis - 1
    vec = [0.0, 0.0, 0.0]
    vec[up] = 1.0 if up_axis >= 0 else -1.0
    return vec


def column_ground(src, p, ext, ia, ib):
    """(ground key, its occupancy type) of source column (ia, ib): rules 2-5 of build_heightmap for one column."""
    min_key, max_key = ext
    a, b, up = R.axis_indices(p.up_axis)
    up_vec = up_vector(p.up_axis)
    use_mean = src.has_mean and not p.ignore_voxel_mean
    flags = R.F_IGNORE_VIRTUAL_ABOVE | (R.F_VIRTUAL if p.virtual_surface else 0) | \
        (R.F_PROMOTE_BELOW if p.promote_virtual_below else 0)
    voxel_floor = R.point_to_region_coord(p.floor, src.resolution)
    voxel_ceiling = R.point_to_region_coord(p.ceiling, src.resolution)
    clearance_permissive = max(1, R.point_to_region_coord(p.min_clearance, src.resolution) - 1)
    plane = min(max(src.to_global(src.om.voxel_key(p.reference_pos))[up], min_key[up]), max_key[up])
    walk = [0, 0, 0]
    walk[a], walk[b], walk[up] = min_key[a] + ia, min_key[b] + ib, plane
    candidate = R.supporting_voxel(src, walk, p.up_axis, min_key, max_key, voxel_floor, voxel_ceiling,
                                   clearance_permissive, flags)
    if candidate is None:
        return walk, R.K_NULL
    ground = R.find_ground(src, candidate, min_key, max_key, p.up_axis, up_vec, p, use_mean)
    ground_key = ground[0] if ground is not None else walk
    return ground_key, src.occupancy_type(ground_key)


def voxel_normal(src, g, up_axis):
    """Model D6 for the covariance of global voxel g, turned towards up: float32[3]."""
    region, local = src.split(g)
    vi = local[0] + local[1] * src.dim[0] + local[2] * src.dim[0] * src.dim[1]
    p = np.asarray(src.chunks[region]["covariance"], dtype=np.float32).reshape(-1, 6)[vi]
    return cov_ref.normal_for_up(cov_ref.decompose(p), up_vector(up_axis))


def expected_normals(src, p, ext, na, source_column):
    """(mb, ma, 3) float32 for a planar heightmap whose cells were written by the columns of source_column."""
    out = np.zeros(source_column.shape + (3,), dtype=np.float32)
    occupied = 0
    for cb, ca in zip(*np.nonzero(source_column != R.NO_COLUMN)):
        column = int(source_column[cb, ca])
        ground_key, voxel_type = column_ground(src, p, ext, column % na, column // na)
        if voxel_type == R.K_OCCUPIED:
            out[cb, ca] = voxel_normal(src, ground_key, p.up_axis)
            occupied += 1
    return out, occupied
