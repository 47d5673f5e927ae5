"""-m gpu: the point filter (ohmhip_map_filter_points / _device, GpuMap.filterPoints, filter_cloud) against the CPU
restatement run on the layers read back (tests/point_filter_ref.py) and, where the covariance test runs, against exact
rational arithmetic: decisions equal outside the band |a - T| <= 2^-40 s, values within it (the bound is derived in
tests/test_point_filter_ref.py).  Keys equal ohmhip_map_voxel_keys; kept indices equal nonzero(status == 1)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (GPU_KEY_DTYPE, GpuMap, GpuNdtMap, GpuTsdfMap, OccupancyMap, OhmHipError, filter_cloud)
from ohm_amd import _lib as L
from ohm_amd import distributed as D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_filter_ref as PF  # noqa: E402
from heightmap_cases import two_level_scene  # noqa: E402

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
NULL = (-32768, -32768, -32768)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def restated(gm, map_, points, tolerance=-1.0, occupancy_only=False, chunks=None):
    keys = gm.voxelKeys(points)
    status, values = PF.filter_points(points, keys, map_.chunks if chunks is None else chunks, map_.resolution,
                                      map_.region_voxel_dimensions, map_.origin, map_.occupancy_threshold_value, tolerance,
                                      occupancy_only, map_.layers)
    return keys, status, values


def check_occupancy_only(gm, map_, points, **kw):
    """Exact equality with the restatement where no covariance test runs."""
    keys, want_status, _ = restated(gm, map_, points, **kw)
    status, kept, values, got_keys = gm.filterPoints(points, kw.get("tolerance", -1.0), kw.get("occupancy_only", False))
    assert np.array_equal(raw(got_keys), raw(keys))
    assert np.array_equal(status, want_status)
    assert np.isnan(values).all() and (values.view(np.uint64) == 0x7ff8000000000000).all()
    assert kept.dtype == np.uint64 and np.array_equal(kept, np.nonzero(status == 1)[0])
    assert gm.lastFilterKept() == len(kept)
    return status, kept


def check_tested(gm, map_, points, tolerance, constructed=None, chunks=None):
    """The covariance test against the exact evaluator.  constructed: rows left out of the in-band share.  Returns
    (status, values, rows inside the band)."""
    chunks = map_.chunks if chunks is None else chunks
    keys, want_status, _ = restated(gm, map_, points, tolerance, chunks=chunks)
    status, kept, values, got_keys = gm.filterPoints(points, tolerance)
    assert np.array_equal(raw(got_keys), raw(keys))
    assert np.array_equal(status == 0, want_status == 0)  # status 2 against 0 as specified: only occupied points are tested
    assert np.array_equal(kept, np.nonzero(status == 1)[0]) and gm.lastFilterKept() == len(kept)
    rows = np.nonzero(status != 0)[0]
    assert (values[status == 0].view(np.uint64) == 0x7ff8000000000000).all()
    voxels = PF.gather(keys[rows], chunks, map_.region_voxel_dimensions, ("occupancy", "mean", "covariance"))
    mean = PF.mean_positions(keys[rows], voxels["mean"][:, 0], map_.resolution, map_.region_voxel_dimensions, map_.origin)
    d = points[rows] - mean
    c = voxels["covariance"]
    finite = np.isfinite(c).all(axis=1)
    assert (status[rows][~finite] == PF.REMOVED).all()
    in_band = PF.check_against_exact(c[finite], d[finite], tolerance, values[rows][finite], status[rows][finite])
    plain = len(rows) if constructed is None else int((~np.isin(rows, constructed)).sum())
    assert in_band <= plain // 100, (in_band, plain)
    return status, values


@pytest.fixture(scope="module")
def scene(gpu):
    """Occupancy + mean from ~2 000 rays at 0.1 m, origin off zero; samples on a floor across several regions."""
    map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
    map_.setOrigin((0.35, -1.2, 0.05))
    gm = GpuMap(map_)
    rng = np.random.default_rng(21)
    ends = np.zeros((2000, 3))
    ends[:, :2] = rng.uniform(-3.0, 3.0, size=(2000, 2))
    ends[:, 2] = rng.uniform(-0.3, 0.1, size=2000)
    rays = np.empty((4000, 3))
    rays[0::2] = (0.1, -0.2, 1.4)
    rays[1::2] = ends
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    return map_, gm, rays


def scene_points(map_, rays, n, seed):
    """n points: around the samples, on voxel and region faces, at negative coordinates, beyond the region range."""
    rng = np.random.default_rng(seed)
    ends = rays[1::2]
    points = ends[rng.integers(0, len(ends), size=n)] + rng.normal(0.0, 0.04, size=(n, 3))
    origin = np.asarray(map_.origin)
    special = []
    for face in (-1.6, 1.6, -4.8, 0.0, 0.1, -0.1):
        for delta in (-1e-6, -1e-9, 0.0, 1e-9, 1e-6):
            for axis in (0, 1):
                p = ends[rng.integers(0, len(ends))].copy()
                p[axis] = origin[axis] + face + delta
                special.append(p)
    special += [(2.0e5, 0.0, 0.0), (0.0, -2.0e5, 0.0), (1.0, 2.0, 1e12), (-104855.0, -1.0, 0.0)]
    special = np.array(special)
    take = min(len(special), n // 2)
    points[:take] = special[rng.permutation(len(special))[:take]]
    return points


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_occupancy_only(scene, n):
    map_, gm, rays = scene
    points = scene_points(map_, rays, n, seed=n)
    status, kept = check_occupancy_only(gm, map_, points)
    if n >= 255:
        assert 0 < len(kept) < n
        keys = gm.voxelKeys(points)
        assert (keys["region"] == NULL).all(axis=1).sum() >= 3 and (keys["region"] < 0).any()
        # capacity truncates the indices, never the count; capacity 0 only counts
        few = gm.filterPoints(points, capacity=5)
        assert np.array_equal(few[1], kept[:5]) and gm.lastFilterKept() == len(kept) and np.array_equal(few[0], status)
        none = gm.filterPoints(points, capacity=0)
        assert len(none[1]) == 0 and gm.lastFilterKept() == len(kept) and np.array_equal(none[0], status)
    if n == 0:
        assert len(status) == 0 and gm.lastFilterKept() == 0


CONSTRUCTED = {  # voxel index of chunk (0, 0, 0) -> covariance state
    10: [0.0, 0.01, 0.04, -0.02, 0.005, 0.03], 11: [0.05, 0.01, 0.0, -0.02, 0.005, 0.03],
    12: [0.05, 0.01, 0.04, -0.02, 0.005, 0.0], 13: [np.nan, 0.01, 0.04, -0.02, 0.005, 0.03],
    14: [0.05, 0.01, 0.04, np.inf, 0.005, 0.03], 15: [0.05, 0.01, 0.04, -0.02, 0.005, -np.inf],
    16: [-0.05, 0.01, 0.04, -0.02, 0.005, 0.03], 17: [0.05, 0.01, -0.04, -0.02, 0.005, -0.03],
}


@pytest.fixture(scope="module")
def ndt_constructed(gpu):
    """Two regions of 8^3 voxels of an occupancy + mean + covariance map, written through write_regions."""
    dim = (8, 8, 8)
    map_ = OccupancyMap(0.25, dim, layers=("occupancy", "mean", "covariance"))
    map_.setOrigin((0.1, -0.3, 0.2))
    threshold = np.float32(map_.occupancy_threshold_value)
    rng = np.random.default_rng(5)
    for region in ((0, 0, 0), (-1, 0, 1)):
        occupancy = np.full(512, 2.0, dtype=np.float32)
        occupancy[rng.integers(20, 512, size=60)] = np.float32(-1.0)
        occupancy[0:4] = [INF, np.nan, threshold, np.nextafter(threshold, np.float32(-1))]
        mean = np.zeros((512, 2), dtype=np.uint32)
        mean[:, 0] = rng.integers(0, 1 << 30, size=512)
        mean[::3, 0] = 0  # a coord of 0 decodes like any other
        mean[:, 1] = 5
        covariance, _ = PF.random_cases(512, 17 + region[2])
        if region == (0, 0, 0):
            for index, state in CONSTRUCTED.items():
                covariance[index] = state
        map_.chunks[region] = {"occupancy": occupancy, "mean": mean, "covariance": covariance}
    gm = GpuNdtMap(map_)  # (uploads the chunks)
    return map_, gm


def constructed_points(map_, per_voxel, seed, spread=1.0):
    """per_voxel points in every voxel of the map's chunks, p = mean + S z: kept and removed in comparable numbers."""
    rng = np.random.default_rng(seed)
    dim = map_.region_voxel_dimensions
    keys = []
    for region in sorted(map_.chunks):
        k = np.zeros(512 * per_voxel, dtype=GPU_KEY_DTYPE)
        index = np.repeat(np.arange(512), per_voxel)
        k["region"] = region
        k["voxel"][:, 0], k["voxel"][:, 1], k["voxel"][:, 2] = index % dim[0], (index // dim[0]) % dim[1], index // (dim[0] * dim[1])
        keys.append(k)
    keys = np.concatenate(keys)
    voxels = PF.gather(keys, map_.chunks, dim, ("occupancy", "mean", "covariance"))
    mean = PF.mean_positions(keys, voxels["mean"][:, 0], map_.resolution, dim, map_.origin)
    c = np.nan_to_num(voxels["covariance"].astype(np.float64), nan=0.05, posinf=0.05, neginf=-0.05)
    z = rng.normal(0.0, spread, size=(len(keys), 3))
    d = np.stack([c[:, 0] * z[:, 0], c[:, 1] * z[:, 0] + c[:, 2] * z[:, 1], c[:, 3] * z[:, 0] + c[:, 4] * z[:, 1] + c[:, 5] * z[:, 2]],
                 axis=1)
    # (the Gaussians are centimetres wide and the means anywhere in a 0.25 m voxel: keep the points in their voxel)
    centre = PF.mean_positions(keys, np.full(len(keys), 511 | (511 << 10) | (511 << 20), dtype=np.uint32), map_.resolution, dim,
                               map_.origin)
    points = np.clip(mean + d, centre - 0.12, centre + 0.12)
    return points, keys


@pytest.mark.parametrize("tolerance", [0.0, 0.75])
def test_covariance_test_against_exact_arithmetic(ndt_constructed, tolerance):
    map_, gm = ndt_constructed
    points, keys = constructed_points(map_, 2, seed=3, spread=1.4)  # a ~ 2 chi^2(3): kept and removed both well over 20 %
    assert np.array_equal(raw(gm.voxelKeys(points)), raw(keys))
    first = np.nonzero((keys["region"] == (0, 0, 0)).all(axis=1))[0]
    voxel = keys["voxel"].astype(int)
    index = voxel[:, 0] + 8 * voxel[:, 1] + 64 * voxel[:, 2]
    constructed = first[np.isin(index[first], list(CONSTRUCTED))]
    status, values = check_tested(gm, map_, points, tolerance, constructed)
    tested = status != 0
    assert (status[tested] == 1).mean() >= 0.2 and (status[tested] == 2).mean() >= 0.2
    by_voxel = {int(index[r]): int(status[r]) for r in first}
    assert [by_voxel[i] for i in (0, 1, 3)] == [0, 0, 0] and by_voxel[2] != 0  # +inf, NaN, below; the threshold itself
    for i in (10, 11, 12, 13, 14, 15):
        assert by_voxel[i] == 2, i  # a zero on the diagonal, a NaN or infinite entry: removed
    assert {by_voxel[16], by_voxel[17]} <= {1, 2}
    assert (status[np.isin(index, [0, 1, 3]) | ~tested] == 0).all()


def test_selection_of_the_test(ndt_constructed, scene):
    map_, gm = ndt_constructed
    points, _ = constructed_points(map_, 1, seed=9, spread=3.0)
    tested = gm.filterPoints(points, 0.0)[0]
    assert (tested == 2).sum() > len(points) // 4
    for kw in ({"tolerance": -1.0}, {"tolerance": -1e-300}, {"tolerance": 0.0, "occupancy_only": True},
               {"tolerance": float("-inf")}):
        status, kept = check_occupancy_only(gm, map_, points, **kw)
        assert np.array_equal(status != 0, tested != 0) and set(status.tolist()) == {0, 1}
    plain_map, plain, rays = scene  # no covariance layer: occupancy alone, whatever the tolerance
    check_occupancy_only(plain, plain_map, scene_points(plain_map, rays, 300, seed=4), tolerance=0.0)
    status = gm.filterPoints(points, float("inf"))[0]  # an infinite tolerance keeps what has a finite value
    assert (status[tested == 1] == 1).all()


def device_buffers(sizes):
    handles, ptrs = [], []
    for nbytes in sizes:
        handle, ptr = L._vp(), L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(handle), max(nbytes, 16), 3), "buffer_create")
        handles.append(handle)
        L.check(L.lib.ohmhip_buffer_ptr(handle, C.byref(ptr)), "buffer_ptr")
        ptrs.append(ptr.value)
    return handles, ptrs


def run_device(gm, data, offset_doubles, stride, n, tolerance, capacity):
    """filter_points_device over `data` (float64 array) uploaded as it is; returns status, kept indices, values, keys,
    kept -- read back after ohmhip_map_sync."""
    handles, ptrs = device_buffers([data.nbytes, n, 8 * capacity, 8 * n, 10 * n, 8])
    try:
        L.check(L.lib.ohmhip_buffer_write(handles[0], data.ctypes.data, data.nbytes, 0, None, None, None), "write")
        params = L.PointFilterParams(tolerance, 0)
        L.check(L.lib.ohmhip_map_filter_points_device(gm._handle, ptrs[0] + 8 * offset_doubles, stride, n, C.byref(params),
                                                      capacity, ptrs[1], ptrs[2] if capacity else None, ptrs[3], ptrs[4],
                                                      ptrs[5]), "filter_points_device")
        gm.wait()
        out = [np.zeros(n, dtype=np.uint8), np.zeros(capacity, dtype=np.uint64), np.zeros(n, dtype=np.float64),
               np.zeros(n, dtype=GPU_KEY_DTYPE), np.zeros(1, dtype=np.uint64)]
        for handle, array in zip(handles[1:], out):
            if array.nbytes:
                L.check(L.lib.ohmhip_buffer_read(handle, array.ctypes.data, array.nbytes, 0, None, None, None), "read")
        return out
    finally:
        for handle in handles:
            L.lib.ohmhip_buffer_destroy(handle)


def test_device_variant(ndt_constructed):
    map_, gm = ndt_constructed
    points, _ = constructed_points(map_, 1, seed=13)
    n = len(points)
    host = gm.filterPoints(points, 0.25)
    host_kept = gm.lastFilterKept()
    # stride 6: the sample ends of a ray buffer, the pointer advanced by 3; one sample is a NaN
    rays = np.zeros((n + 1, 6))
    rays[:n, 3:] = points
    rays[:, :3] = 7.0
    rays[n, 3:] = (0.1, np.nan, 0.2)
    status, kept, values, keys, total = run_device(gm, rays, 3, 6, n + 1, 0.25, n + 1)
    assert status[n] == 0 and tuple(keys[n]["region"]) == NULL and not keys[n]["voxel"].any()
    assert values[n:].view(np.uint64)[0] == 0x7ff8000000000000
    assert np.array_equal(status[:n], host[0]) and np.array_equal(raw(values[:n]), raw(host[2]))
    assert np.array_equal(raw(keys[:n]), raw(host[3]))
    assert int(total[0]) == host_kept and np.array_equal(kept[:host_kept], host[1])
    # stride 3, a capacity below the count, and no capacity at all
    status, kept, values, keys, total = run_device(gm, points, 0, 3, n, 0.25, 7)
    assert np.array_equal(status, host[0]) and np.array_equal(raw(values), raw(host[2])) and np.array_equal(raw(keys), raw(host[3]))
    assert int(total[0]) == host_kept > 7 and np.array_equal(kept, host[1][:7])
    status, kept, values, keys, total = run_device(gm, points, 0, 3, n, 0.25, 0)
    assert np.array_equal(status, host[0]) and int(total[0]) == host_kept
    # null status / values / keys: the count alone
    handles, ptrs = device_buffers([points.nbytes, 8])
    try:
        L.check(L.lib.ohmhip_buffer_write(handles[0], points.ctypes.data, points.nbytes, 0, None, None, None), "write")
        params = L.PointFilterParams(0.25, 0)
        L.check(L.lib.ohmhip_map_filter_points_device(gm._handle, ptrs[0], 3, n, C.byref(params), 0, None, None, None, None,
                                                      ptrs[1]), "filter_points_device")
        L.check(L.lib.ohmhip_map_filter_points_device(gm._handle, ptrs[0], 3, 0, C.byref(params), 0, None, None, None, None,
                                                      ptrs[1]), "filter_points_device")  # count 0 writes 0
        gm.wait()
        total = np.ones(1, dtype=np.uint64)
        L.check(L.lib.ohmhip_buffer_read(handles[1], total.ctypes.data, 8, 0, None, None, None), "read")
        assert int(total[0]) == 0
    finally:
        for handle in handles:
            L.lib.ohmhip_buffer_destroy(handle)


def test_tiled_regions(gpu):
    """Regions of 64 x 64 x 32 voxels are four tiles of 8 layers.  Uploaded regions hold data in every tile; a region built
    from rays that stay in its lowest layers holds only that tile, and the others read as unobserved."""
    dim = (64, 64, 32)
    nv = dim[0] * dim[1] * dim[2]
    map_ = OccupancyMap(0.1, dim, layers=("occupancy", "mean", "covariance"))
    map_.setOrigin((0.0, 0.5, -0.25))
    rng = np.random.default_rng(8)
    for region in ((0, 0, 0), (-1, 0, 1)):
        occupancy = rng.choice(np.array([2.0, -1.0, np.inf], dtype=np.float32), size=nv, p=(0.6, 0.2, 0.2))
        mean = np.zeros((nv, 2), dtype=np.uint32)
        mean[:, 0] = rng.integers(0, 1 << 30, size=nv)
        covariance = np.tile(np.array([0.05, 0.01, 0.04, -0.02, 0.005, 0.03], dtype=np.float32), (nv, 1))
        covariance[:, 0] = rng.uniform(0.02, 0.08, size=nv)
        map_.chunks[region] = {"occupancy": occupancy, "mean": mean, "covariance": covariance}
    gm = GpuMap(map_)
    n = 1500
    lo = np.array([-9.6, -3.2, -1.6]) + np.asarray(map_.origin)
    points = rng.uniform(lo, lo + np.array([12.8, 6.4, 6.4]), size=(n, 3))
    status, values = check_tested(gm, map_, points, 40.0)
    keys = gm.voxelKeys(points)
    for region in map_.chunks:
        in_region = (keys["region"] == region).all(axis=1)
        for tile in range(4):
            assert (status[in_region & (keys["voxel"][:, 2] // 8 == tile)] != 0).any(), (region, tile)
    held = (keys["region"] == (0, 0, 0)).all(axis=1) | (keys["region"] == (-1, 0, 1)).all(axis=1)
    assert (~held).sum() > n // 4 and (status[~held] == 0).all()

    low_map = OccupancyMap(0.1, dim, layers=("occupancy", "mean"))
    low = GpuMap(low_map)
    starts = rng.uniform((-3.0, -3.0, -1.5), (3.0, 3.0, -0.9), size=(600, 3))
    ends = rng.uniform((-3.0, -3.0, -1.5), (3.0, 3.0, -0.9), size=(600, 3))
    rays = np.stack([starts, ends], axis=1).reshape(-1, 3)
    assert low.integrateRays(rays) == rays.shape[0]
    low.syncVoxels()
    assert sorted(low_map.chunks) == [(0, 0, 0)] and low.cacheStats()["regions_resident"] == 1
    points = np.concatenate([ends + rng.normal(0.0, 0.03, size=ends.shape), ends + (0.0, 0.0, 0.9), ends + (0.0, 0.0, 2.0)])
    status, kept = check_occupancy_only(low, low_map, points)
    assert len(kept) > 100 and (status[600:] == 0).all()


def _observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


def test_spilled_regions_read_only(gpu):
    layers = ("occupancy", "mean", "covariance")
    map_ = OccupancyMap(0.1, layers=layers)
    gm = GpuNdtMap(map_, region_capacity=8)
    gm.setMemoryLimit(7 * gm.cacheStats()["bytes_per_region"])  # the scene holds 9 regions
    gm.setSpillToHost(True)
    ref_map = OccupancyMap(0.1, layers=layers)
    ref = GpuNdtMap(ref_map)
    pairs = two_level_scene().reshape(-1, 2, 3)
    pairs = pairs[np.argsort(pairs[:, 1, 0], kind="stable")]
    for part in np.array_split(pairs, 8):
        part = part.reshape(-1, 3)
        for g in (gm, ref):
            assert g.integrateRays(part) == part.shape[0]
    assert gm.cacheStats()["regions_spilled"] > 0
    rng = np.random.default_rng(31)
    points = pairs[::5, 1] + rng.normal(0.0, 0.01, size=(len(pairs[::5]), 3))  # (the floor's Gaussians are millimetres thick)
    before = _observe(gm)
    first = gm.filterPoints(points, 0.5)
    again = gm.filterPoints(points, 0.5)
    plain = gm.filterPoints(points)
    assert _observe(gm) == before
    want = ref.filterPoints(points, 0.5)
    for a, b, c in zip(first, again, want):
        assert np.array_equal(raw(a), raw(b)) and np.array_equal(raw(a), raw(c))
    for a, c in zip(plain, ref.filterPoints(points)):
        assert np.array_equal(raw(a), raw(c))
    assert (first[0] == 1).sum() > 50 and (first[0] == 2).sum() > 50
    regions = set(map(tuple, ref.regionKeys()))
    assert len(regions) == 9 and regions <= {tuple(r) for r in first[3]["region"].tolist()}  # spilled ones are asked too
    ref.syncVoxels()
    check_tested(ref, ref_map, points, 0.5)


def test_piece_boundary(scene):
    map_, gm, rays = scene
    n = L.PF_PIECE_POINTS + 65
    rng = np.random.default_rng(2)
    ends = rays[1::2]
    points = ends[rng.integers(0, len(ends), size=n)] + rng.normal(0.0, 0.05, size=(n, 3))
    status, kept = check_occupancy_only(gm, map_, points)
    assert (kept[1:] > kept[:-1]).all() and kept[-1] >= L.PF_PIECE_POINTS and (kept < L.PF_PIECE_POINTS).sum() > 1000
    tail = gm.filterPoints(points[L.PF_PIECE_POINTS - 3:])
    assert np.array_equal(tail[0], status[L.PF_PIECE_POINTS - 3:])
    few = gm.filterPoints(points, capacity=len(kept) - 2)  # a capacity that ends inside the last piece
    assert np.array_equal(few[1], kept[:-2]) and gm.lastFilterKept() == len(kept)


def test_filter_cloud_file(scene, tmp_path):
    map_, gm, rays = scene
    points = scene_points(map_, rays, 400, seed=77)
    times = np.linspace(5.0, 6.0, len(points))
    path = tmp_path / "filtered.ply"
    exported, removed = filter_cloud(str(path), gm, points, times)
    kept = gm.filterPoints(points)[1].astype(np.int64)
    assert exported == len(kept) > 0 and removed == len(points) - exported > 0
    data = path.read_bytes()
    body = data[data.index(b"end_header\n") + 11:]
    rows = np.frombuffer(body, dtype="<f8").reshape(-1, 4)
    assert b"element vertex %d\n" % exported in data and b"property double time\n" in data
    assert np.array_equal(rows[:, :3], points[kept]) and np.array_equal(rows[:, 3], times[kept])


def _status(call):
    try:
        call()
    except OhmHipError as err:
        return err.status
    return L.OK


def test_refusals_on_live_maps(scene):
    map_, gm, rays = scene
    points = rays[1::2][:10].copy()
    assert _status(lambda: gm.filterPoints(points)) == L.OK
    assert _status(lambda: gm.filterPoints(points, float("nan"))) == L.ERR_INVALID_ARG
    bad = points.copy()
    bad[3, 1] = np.inf
    assert _status(lambda: gm.filterPoints(bad)) == L.ERR_INVALID_ARG
    params = L.PointFilterParams(0.0, 2)
    kept = C.c_uint64(0)
    assert L.lib.ohmhip_map_filter_points(gm._handle, points.ctypes.data, 10, C.byref(params), 0, None, None, None, None,
                                          C.byref(kept)) == L.ERR_INVALID_ARG
    params = L.PointFilterParams(0.0, 0)
    assert L.lib.ohmhip_map_filter_points(gm._handle, points.ctypes.data, 10, C.byref(params), 4, None, None, None, None,
                                          C.byref(kept)) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_filter_points(gm._handle, points.ctypes.data, 10, C.byref(params), 0, None, None, None, None,
                                          C.byref(kept)) == L.OK and kept.value > 0  # every array is optional
    assert L.lib.ohmhip_map_filter_points(gm._handle, None, 0, C.byref(params), 0, None, None, None, None,
                                          C.byref(kept)) == L.OK and kept.value == 0
    owner = GpuMap(OccupancyMap(0.1))
    owner.setRegionOwnership(2, 0)
    assert _status(lambda: owner.filterPoints(points)) == L.ERR_UNSUPPORTED
    part = D.territories_from_origins([(0.0, 0.0, 0.0), (20.0, 0.0, 0.0)], 2, 0, (3.2, 3.2, 3.2), block_shift=0, margin=5.0)
    partitioned = GpuMap(OccupancyMap(0.1))
    partitioned.setRegionPartition(part)
    assert _status(lambda: partitioned.filterPoints(points)) == L.ERR_UNSUPPORTED
    tsdf = GpuTsdfMap(OccupancyMap(0.1, layers=()), default_truncation_distance=0.2)
    assert _status(lambda: tsdf.filterPoints(points)) == L.ERR_UNSUPPORTED  # no occupancy layer
