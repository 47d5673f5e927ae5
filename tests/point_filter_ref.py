"""CPU restatement of the point filter (include/ohmhip.h, "POINT FILTER"; utils/ohmfilter/ohmfilter.cpp:67-91, 150-279)
in numpy fp64, operation for operation in the order the header states, and an EXACT evaluator of the covariance test
on fractions.Fraction that the restatement and the kernels are both held to.

    covariance_value(c, d)          a = |inverse(S) d|^2 as the header orders it          (n,) float64
    filter_points(...)              status / values of points with known keys, over chunks read back from a map
    exact_value(c, d)               a, T-independent, and the band scale s, as Fractions   (None: S is singular)
    exact_limit(tolerance)          T = fl(3.0 + tolerance) as a Fraction
    random_cases(n, seed)           square roots and offsets with a spread around T

A numpy elementwise product or sum is one IEEE operation: nothing here contracts."""
from fractions import Fraction

import numpy as np

from cloud_ref import GPU_KEY, sub_voxel_to_local

DROPPED, KEPT, REMOVED = 0, 1, 2
BAND = Fraction(1, 2 ** 40)  # decisions are compared outside |a - T| <= BAND * s; values within BAND * s


def covariance_value(c, d):
    """filterPointByCovariance's value for packed square roots c (n, 6) float32 and offsets d (n, 3) float64."""
    c = np.asarray(c, dtype=np.float32).reshape(-1, 6).astype(np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    zero = np.zeros(c.shape[0])
    # m[column][row]: covarianceSqrtMatrix (ohm/CovarianceVoxel.h:71-91)
    m = [[c[:, 0], c[:, 1], c[:, 3]], [zero, c[:, 2], c[:, 4]], [zero, zero, c[:, 5]]]
    with np.errstate(all="ignore"):
        r = 1.0 / (m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) - m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2]) +
                   m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]))
        i00 = (m[1][1] * m[2][2] - m[2][1] * m[1][2]) * r
        i10 = -(m[1][0] * m[2][2] - m[2][0] * m[1][2]) * r
        i20 = (m[1][0] * m[2][1] - m[2][0] * m[1][1]) * r
        i01 = -(m[0][1] * m[2][2] - m[2][1] * m[0][2]) * r
        i11 = (m[0][0] * m[2][2] - m[2][0] * m[0][2]) * r
        i21 = -(m[0][0] * m[2][1] - m[2][0] * m[0][1]) * r
        i02 = (m[0][1] * m[1][2] - m[1][1] * m[0][2]) * r
        i12 = -(m[0][0] * m[1][2] - m[1][0] * m[0][2]) * r
        i22 = (m[0][0] * m[1][1] - m[1][0] * m[0][1]) * r
        vx = (i00 * d[:, 0] + i10 * d[:, 1]) + i20 * d[:, 2]
        vy = (i01 * d[:, 0] + i11 * d[:, 1]) + i21 * d[:, 2]
        vz = (i02 * d[:, 0] + i12 * d[:, 1]) + i22 * d[:, 2]
        return (vx * vx + vy * vy) + vz * vz


def decide(values, tolerance):
    """KEPT / REMOVED per value: kept iff fabs(a) < 3.0 + tolerance, the sum in fp64 (a NaN is removed)."""
    with np.errstate(invalid="ignore"):
        return np.where(np.fabs(values) < np.float64(3.0) + np.float64(tolerance), KEPT, REMOVED).astype(np.uint8)


def mean_positions(keys, coords, resolution, dim, origin):
    """positionUnsafe (ohm/VoxelMean.h:47-54): voxelCentreGlobal(key) (ohm/OccupancyMap.h:757-778), then the decoded mean
    added."""
    keys = np.asarray(keys, dtype=GPU_KEY)
    out = np.empty((len(keys), 3), dtype=np.float64)
    off = sub_voxel_to_local(coords, resolution)
    for a in range(3):
        region_dim = dim[a] * float(resolution)
        v = keys["region"][:, a].astype(np.float32).astype(np.float64)
        v = v * region_dim
        v = v - 0.5 * region_dim
        v = v + float(origin[a])
        v = v + keys["voxel"][:, a].astype(np.float64) * float(resolution)
        v = v + 0.5 * float(resolution)
        out[:, a] = v + off[:, a]
    return out


def gather(keys, chunks, dim, names):
    """The voxels at keys out of chunks {(rx, ry, rz): {layer: block}}: occupancy +inf (mean, covariance zeros) for a
    null key, a region the map does not hold and a layer its chunk does not hold."""
    keys = np.asarray(keys, dtype=GPU_KEY)
    n = len(keys)
    out = {"occupancy": np.full(n, np.inf, dtype=np.float32), "mean": np.zeros((n, 2), dtype=np.uint32),
           "covariance": np.zeros((n, 6), dtype=np.float32)}
    regions = keys["region"].astype(np.int64)
    index = (keys["voxel"][:, 0].astype(np.int64) + dim[0] * keys["voxel"][:, 1].astype(np.int64) +
             dim[0] * dim[1] * keys["voxel"][:, 2].astype(np.int64))
    packed = (regions[:, 0] + 32768) | ((regions[:, 1] + 32768) << 16) | ((regions[:, 2] + 32768) << 32)
    for value in np.unique(packed):
        region = (int(value & 0xffff) - 32768, int((value >> 16) & 0xffff) - 32768, int((value >> 32) & 0xffff) - 32768)
        chunk = chunks.get(region)
        if chunk is None or region == (-32768, -32768, -32768):
            continue
        rows = np.nonzero(packed == value)[0]
        for name in names:
            if name in chunk:
                block = np.asarray(chunk[name], dtype=out[name].dtype).reshape((-1,) + out[name].shape[1:])
                out[name][rows] = block[index[rows]]
    return out


def filter_points(points, keys, chunks, resolution, dim, origin, threshold, tolerance=-1.0, occupancy_only=False,
                  layers=("occupancy", "mean", "covariance")):
    """Status (n,) uint8 and values (n,) float64 of points whose keys are known (OccupancyMap::voxelKey: GpuMap.voxelKeys,
    held to the oracle elsewhere), over the map's chunks."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(points)
    test = (not occupancy_only) and "mean" in layers and "covariance" in layers and tolerance >= 0
    voxels = gather(keys, chunks, dim, ("occupancy", "mean", "covariance") if test else ("occupancy",))
    v = voxels["occupancy"]
    with np.errstate(invalid="ignore"):
        occupied = (v != np.float32(np.inf)) & (v >= np.float32(threshold))  # a NaN is not
    status = np.where(occupied, KEPT, DROPPED).astype(np.uint8)
    values = np.full(n, np.nan)
    if test and occupied.any():
        rows = np.nonzero(occupied)[0]
        mean = mean_positions(np.asarray(keys, dtype=GPU_KEY)[rows], voxels["mean"][rows, 0], resolution, dim, origin)
        values[rows] = covariance_value(voxels["covariance"][rows], points[rows] - mean)
        status[rows] = decide(values[rows], tolerance)
    return status, values


def random_cases(n, seed, spread=1.0):
    """Square roots with entries of a few centimetres, offsets d = S z with z ~ N(0, spread^2): a ~ spread^2 * chi^2(3)."""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, 6), dtype=np.float32)
    c[:, [0, 2, 5]] = rng.uniform(0.02, 0.1, size=(n, 3))
    c[:, [1, 3, 4]] = rng.uniform(-0.05, 0.05, size=(n, 3))
    z = rng.normal(0.0, spread, size=(n, 3))
    cd = c.astype(np.float64)
    d = np.stack([cd[:, 0] * z[:, 0], cd[:, 1] * z[:, 0] + cd[:, 2] * z[:, 1],
                  cd[:, 3] * z[:, 0] + cd[:, 4] * z[:, 1] + cd[:, 5] * z[:, 2]], axis=1)
    return c, d


def exact_limit(tolerance):
    """T = fl(3.0 + tolerance)."""
    return Fraction(float(np.float64(3.0) + np.float64(tolerance)))


def exact_value(c, d):
    """(a, s) in exact arithmetic for one voxel's six floats and one fp64 offset: S v = d solved exactly, a = v . v, and
    s = sum_i (sum_j |inverse(S)_ij d_j|)^2, the scale of the roundings the fp64 formula makes.  None when S is singular
    (a zero on the diagonal: the fp64 formula divides by a zero determinant and the point is removed)."""
    c = [Fraction(float(np.float32(x))) for x in c]
    d = [Fraction(float(x)) for x in d]
    s_rows = [[c[0], 0, 0], [c[1], c[2], 0], [c[3], c[4], c[5]]]
    if c[0] == 0 or c[2] == 0 or c[5] == 0:
        return None
    # the inverse of a lower triangular matrix, column by column (forward substitution on the unit vectors)
    inv = [[Fraction(0)] * 3 for _ in range(3)]
    for col in range(3):
        for row in range(3):
            rhs = Fraction(1 if row == col else 0) - sum(s_rows[row][k] * inv[k][col] for k in range(row))
            inv[row][col] = rhs / s_rows[row][row]
    v = [sum(inv[i][j] * d[j] for j in range(3)) for i in range(3)]
    a = sum(x * x for x in v)
    s = sum(sum(abs(inv[i][j] * d[j]) for j in range(3)) ** 2 for i in range(3))
    return a, s


def check_against_exact(c, d, tolerance, values, status):
    """Holds fp64 values / decisions (of the restatement or of the device) to the exact evaluator.  Returns the number of
    cases inside the band, where only the value is asserted.  Cases with a singular S must be REMOVED."""
    limit = exact_limit(tolerance)
    in_band = 0
    for i in range(len(values)):
        exact = exact_value(c[i], d[i])
        if exact is None:
            assert status[i] == REMOVED, (i, c[i], values[i])
            continue
        a, s = exact
        assert np.isfinite(values[i]), (i, c[i], d[i])
        assert abs(Fraction(float(values[i])) - a) <= BAND * s, (i, float(a), values[i], float(s))
        if abs(a - limit) <= BAND * s:
            in_band += 1
            continue
        assert status[i] == (KEPT if a < limit else REMOVED), (i, float(a), float(limit), status[i])
    return in_band
