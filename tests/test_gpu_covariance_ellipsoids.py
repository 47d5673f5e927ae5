"""-m gpu: covariance ellipsoids of the occupied voxels of an NDT map (ohmhip_map_covariance_ellipsoids / _count /
_device, ohm_amd.extract_covariance_ellipsoids, save_covariance_cloud).  Selection and order are extract_cloud's, byte
for byte; axes and scales equal the model of tests/covariance_eigen_ref.py applied to the voxel read back by key, bit
for bit.  The maps are those of tests/test_gpu_covariance_eigen.py with occupancy planted so that occupied, free,
unobserved and NaN voxels all occur."""
import ctypes as C

import numpy as np
import pytest

import covariance_cases as cases
import covariance_eigen_ref as cov_ref
from ohm_amd import (GPU_KEY_DTYPE, GpuMap, GpuNdtMap, OccupancyMap, cloud_params, count_cloud, extract_cloud,
                     extract_covariance_ellipsoids, icosphere, save_covariance_cloud)
from ohm_amd import _lib as L
from ohm_amd.cloud import COVARIANCE_DISPLAY_SCALE, CloudMode
from test_gpu_covariance_eigen import DeviceBuffer, locals_of, ndt_map, spread

pytestmark = pytest.mark.gpu

OCCUPIED, FREE = np.float32(2.0), np.float32(-1.0)


def plant(dims, regions, forced):
    """Every case's covariance in turn into `regions`; occupancy by case index mod 7: 3 free, 5 never written
    (unobserved), 6 NaN, otherwise occupied; a mean with a non-zero count in every planted voxel."""
    map_, gm = ndt_map(dims)
    P = cases.all_p()
    n = P.shape[0]
    region_of = np.arange(n) % len(regions)
    key_regions = np.array(regions, dtype=np.int16)[region_of]
    key_locals = np.zeros((n, 3), dtype=np.uint8)
    for r in range(len(regions)):
        mine = np.flatnonzero(region_of == r)
        key_locals[mine] = locals_of(dims, spread(dims, mine.size, forced))
    keys = (key_regions, key_locals)
    assert gm.writeVoxels(keys, "covariance", P) == n
    rng = np.random.default_rng(77)
    mean = np.stack([rng.integers(0, 1 << 30, size=n, dtype=np.uint64).astype(np.uint32) | np.uint32(1 << 31),
                     np.arange(1, n + 1, dtype=np.uint32)], axis=1)
    assert gm.writeVoxels(keys, "mean", mean) == n
    kind = np.arange(n) % 7
    occupancy = np.where(kind == 3, FREE, np.where(kind == 6, np.float32(np.nan), OCCUPIED)).astype(np.float32)
    written = np.flatnonzero(kind != 5)
    assert gm.writeVoxels((key_regions[written], key_locals[written]), "occupancy", occupancy[written]) == written.size
    return map_, gm, int((kind[kind != 5] < 3).sum() + (kind == 4).sum())


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_rows(gm, e, cloud, what=""):
    """Rows equal the cloud's, and axes / scales equal the model on the covariance read back at each row's key."""
    assert e.count == cloud.count and len(e) == len(cloud), what
    assert np.array_equal(raw(e.keys), raw(cloud.keys)), what
    assert np.array_equal(raw(e.positions), raw(cloud.positions)), what
    assert np.array_equal(raw(e.values), raw(cloud.values)), what
    covariance, present = gm.readVoxels(e.keys, "covariance")
    assert present.all()
    cache = {}
    for i, p in enumerate(covariance):
        d = cache.get(p.tobytes())
        if d is None:
            d = cache[p.tobytes()] = cov_ref.decompose(p)
        assert np.array_equal(e.axes[i].reshape(9).view(np.uint64), d.eigenvectors.view(np.uint64)), (what, i, p)
        assert np.array_equal(e.scales[i].view(np.uint64), d.scale.view(np.uint64)), (what, i, p)


@pytest.fixture(scope="module")
def cubic(gpu):
    map_, gm, occupied = plant((16, 16, 16), [(0, 0, 0), (1, 0, 0), (3, 0, 0)], forced=(0, 4095))
    yield gm, occupied
    gm.close()


def test_rows_are_the_clouds_rows(cubic):
    gm, occupied = cubic
    cloud = extract_cloud(gm)
    assert cloud.count == occupied > 200  # free, unobserved and NaN voxels are not selected
    e = extract_covariance_ellipsoids(gm)
    assert_rows(gm, e, cloud, "16^3")
    assert {tuple(v[:3]) for v in e.keys["voxel"].tolist()} >= {(0, 0, 0), (15, 15, 15)}


def test_capacity_and_count_only(cubic):
    gm, occupied = cubic
    full = extract_covariance_ellipsoids(gm)
    half = extract_covariance_ellipsoids(gm, capacity=occupied // 2)
    assert half.count == occupied and len(half) == occupied // 2
    for name in ("positions", "axes", "scales", "keys", "values"):
        assert np.array_equal(raw(getattr(half, name)), raw(getattr(full, name)[:occupied // 2])), name
    none = extract_covariance_ellipsoids(gm, capacity=0)
    assert none.count == occupied and len(none) == 0
    n = C.c_uint64(0)
    p = cloud_params()
    L.check(L.lib.ohmhip_map_covariance_ellipsoids_count(gm._handle, C.byref(p), C.byref(n)), "count")
    assert int(n.value) == occupied == count_cloud(gm)
    # keys and values are optional
    positions, axes, scales = np.zeros((occupied, 3)), np.zeros((occupied, 3, 3)), np.zeros((occupied, 3))
    L.check(L.lib.ohmhip_map_covariance_ellipsoids(gm._handle, C.byref(p), occupied, positions.ctypes.data,
                                                   axes.ctypes.data, scales.ctypes.data, None, None, C.byref(n)), "bare")
    assert np.array_equal(raw(axes), raw(full.axes)) and np.array_equal(raw(positions), raw(full.positions))


def test_use_extents(cubic):
    gm, occupied = cubic
    box = ((0.0, -0.5, -0.5), (2.0, 0.3, 0.4))
    cloud = extract_cloud(gm, extents=box)
    assert 0 < cloud.count < occupied
    assert_rows(gm, extract_covariance_ellipsoids(gm, extents=box), cloud, "extents")


def _call(gm, p, capacity=4):
    positions, axes, scales = np.zeros((4, 3)), np.zeros((4, 3, 3)), np.zeros((4, 3))
    n = C.c_uint64(0)
    return L.lib.ohmhip_map_covariance_ellipsoids(gm._handle, C.byref(p), capacity, positions.ctypes.data,
                                                  axes.ctypes.data, scales.ctypes.data, None, None, C.byref(n))


def test_refusals(cubic):
    gm, _ = cubic
    assert _call(gm, cloud_params()) == L.OK
    assert _call(gm, cloud_params(export_free=True)) == L.ERR_INVALID_ARG
    assert _call(gm, cloud_params(ignore_voxel_mean=True)) == L.ERR_INVALID_ARG
    for mode in (CloudMode.DENSITY, CloudMode.TSDF, CloudMode.CLEARANCE):
        assert _call(gm, cloud_params(mode)) == L.ERR_INVALID_ARG
    p = cloud_params()
    n = C.c_uint64(0)
    some = np.zeros(36)
    for null in range(3):  # positions, axes, scales
        arrays = [some.ctypes.data] * 3
        arrays[null] = None
        assert L.lib.ohmhip_map_covariance_ellipsoids(gm._handle, C.byref(p), 4, *arrays, None, None,
                                                      C.byref(n)) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_covariance_ellipsoids(gm._handle, None, 0, None, None, None, None, None,
                                                  C.byref(n)) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_covariance_ellipsoids(gm._handle, C.byref(p), 0, None, None, None, None, None,
                                                  None) == L.ERR_INVALID_ARG
    bad = cloud_params(extents=((0.0, 0.0, float("nan")), (1.0, 1.0, 1.0)))
    assert _call(gm, bad) == L.ERR_INVALID_ARG  # as for the cloud call
    for layers in (("occupancy", "mean"), ("occupancy",)):
        plain = GpuMap(OccupancyMap(0.1, (16, 16, 16), layers=layers))
        assert _call(plain, cloud_params()) == L.ERR_UNSUPPORTED
        assert L.lib.ohmhip_map_covariance_ellipsoids_count(plain._handle, C.byref(p), C.byref(n)) == L.ERR_UNSUPPORTED
        plain.close()
    owner = GpuNdtMap(OccupancyMap(0.1, (16, 16, 16), layers=("occupancy", "mean", "covariance")))
    owner.setRegionOwnership(2, 0)
    assert _call(owner, cloud_params()) == L.ERR_UNSUPPORTED
    owner.close()


def test_device_variant_equals_host_variant(cubic):
    gm, occupied = cubic
    host = extract_covariance_ellipsoids(gm)
    capacity = occupied + 5  # rows past the count stay unwritten
    bufs = [DeviceBuffer(24 * capacity), DeviceBuffer(72 * capacity), DeviceBuffer(24 * capacity),
            DeviceBuffer(10 * capacity), DeviceBuffer(4 * capacity), DeviceBuffer(8)]
    try:
        sentinel = np.full(9 * capacity, -7.0)
        bufs[1].write(sentinel)
        p = cloud_params()
        L.check(L.lib.ohmhip_map_covariance_ellipsoids_device(gm._handle, C.byref(p), capacity,
                                                              *[b.ptr for b in bufs]), "device")
        gm.wait()
        assert int(bufs[5].read(np.uint64, (1,))[0]) == occupied
        assert np.array_equal(raw(bufs[0].read(np.float64, (capacity, 3))[:occupied]), raw(host.positions))
        axes = bufs[1].read(np.float64, (capacity, 3, 3))
        assert np.array_equal(raw(axes[:occupied]), raw(host.axes)) and (axes[occupied:] == -7.0).all()
        assert np.array_equal(raw(bufs[2].read(np.float64, (capacity, 3))[:occupied]), raw(host.scales))
        assert np.array_equal(raw(bufs[3].read(GPU_KEY_DTYPE, (capacity,))[:occupied]), raw(host.keys))
        assert np.array_equal(raw(bufs[4].read(np.float32, (capacity,))[:occupied]), raw(host.values))
    finally:
        for b in bufs:
            b.close()


@pytest.mark.parametrize("dims,regions,forced", [
    ((32, 32, 8), [(0, 0, 0), (-1, 2, 0)], (0, 4095, 4096, 8191)),                          # a region of two chunks
    ((64, 64, 16), [(0, 0, 0), (1, -1, 0)], (0, 65535, 32767, 32768, 2047, 2048))])          # a tiled region
def test_other_region_shapes(gpu, dims, regions, forced):
    map_, gm, occupied = plant(dims, regions, forced)
    cloud = extract_cloud(gm)
    assert cloud.count == occupied
    assert_rows(gm, extract_covariance_ellipsoids(gm), cloud, str(dims))
    gm.close()


def read_ply_mesh(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    header = data[:end].decode("ascii").splitlines()
    n_vertices = int(next(ln for ln in header if ln.startswith("element vertex")).split()[-1])
    n_faces = int(next(ln for ln in header if ln.startswith("element face")).split()[-1])
    vertices = np.frombuffer(data, dtype="<f8", count=3 * n_vertices, offset=end).reshape(-1, 3)
    faces = np.frombuffer(data, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=n_faces,
                          offset=end + 24 * n_vertices)
    assert end + 24 * n_vertices + 13 * n_faces == len(data)
    return vertices, faces


def test_save_covariance_cloud_round_trip(cubic, tmp_path):
    """Every vertex of an ellipsoid lies on (v - pos)^T C^-1 (v - pos) = 3: ohm2ply's sqrt(3) factor, squared.

    The form is evaluated with mpmath on the exact C of the six floats, so the check carries no error of its own, and
    holds to 1e-9 relative for every voxel whose fp64 decomposition can meet it.  To first order a decomposition with
    eigenvalue errors of eps |C| and eigenvector errors of eps |C| / gap moves the form by about eps * cond (the
    smallest eigenvalue's relative error, and the mixing of two axes, in which the gap cancels: eps |C| / (s_i s_j)),
    and writing a vertex as position + offset in fp64 moves it by eps |pos| / s_min.  Checked are the voxels with
    8 eps cond + 4 eps |pos| / s_min <= 1e-9 whose eigenvalues all lie above D5's 1e-9 (at or below it the scale is the
    eigenvalue, not its root, and the mesh is not C's ellipsoid): cond up to about 5e5."""
    import mpmath
    mpmath.mp.dps = 40
    eps = 2.0 ** -52
    gm, occupied = cubic
    path = str(tmp_path / "ellipsoids.ply")
    assert save_covariance_cloud(path, gm) == occupied
    vertices, faces = read_ply_mesh(path)
    sphere, sphere_faces = icosphere(1)
    assert vertices.shape[0] == occupied * sphere.shape[0] and faces.shape[0] == occupied * sphere_faces.shape[0]
    assert (faces["n"] == 3).all() and faces["v"].min() == 0 and faces["v"].max() == vertices.shape[0] - 1
    e = extract_covariance_ellipsoids(gm)
    covariance, _ = gm.readVoxels(e.keys, "covariance")
    vertices = vertices.reshape(occupied, sphere.shape[0], 3)
    checked, worst = 0, 0.0
    for i, p in enumerate(covariance.astype(np.float64)):
        s = np.array([[p[0], 0, 0], [p[1], p[2], 0], [p[3], p[4], p[5]]])
        with np.errstate(all="ignore"):
            c = s @ s.T
        if not np.isfinite(c).all():
            continue
        lam = np.linalg.eigvalsh(c)
        if not lam[0] > 2e-9:
            continue
        if 8 * eps * lam[2] / lam[0] + 4 * eps * np.abs(e.positions[i]).max() / np.sqrt(lam[0]) + 16 * eps > 1e-9:
            continue
        m = [mpmath.mpf(float(x)) for x in p]
        root = mpmath.matrix([[m[0], 0, 0], [m[1], m[2], 0], [m[3], m[4], m[5]]])
        inverse = (root * root.T) ** -1
        for v in vertices[i]:
            offset = mpmath.matrix([mpmath.mpf(float(v[k])) - mpmath.mpf(float(e.positions[i][k])) for k in range(3)])
            form = (offset.T * inverse * offset)[0]
            error = abs(float(form / COVARIANCE_DISPLAY_SCALE ** 2 - 1))
            assert error <= 1e-9, (i, p, float(form))
            worst = max(worst, error)
        checked += 1
    print("ellipsoids checked %d of %d, worst relative error %.3g" % (checked, occupied, worst))
    assert checked >= 125
