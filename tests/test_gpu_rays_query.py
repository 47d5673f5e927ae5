"""-m gpu: RaysQueryGpu (ohmhip_map_rays_query) against the CPU query (tests/rays_query_ref.py, a restatement of
ohm/RaysQuery.cpp:102-203) at EXACT equality -- range, unobserved volume, terminal type and terminal key of every ray.
Restates RaysQuery.Gpu and RaysQuery.CpuVsGpu (tests/ohmtestgpu/GpuRaysQueryTests.cpp:26-128), whose own tolerance
(mismatched rays allowed, 2.5 x resolution of volume error) is not used here; adds the strict threshold, the filter, the
terminal carry-over of rays that visit no voxel, edge rays, tiled regions, spill to host, observation order, the device
variant, NDT / TSDF maps and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (GpuMap, GpuNdtMap, GpuTsdfMap, OccupancyMap, OccupancyType, OhmHipError, RaysQueryGpu, synth)
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from parity import make_oracle  # noqa: E402
from rays_query_ref import ChunkBlocks, rays_query  # noqa: E402
from test_rays_query_ref import QUERY_SCALE, hits_only, reference_rays, scaled  # noqa: E402

pytestmark = pytest.mark.gpu

FAR = 32768 * 3.2 + 10.0  # beyond the int16 region range at 0.1 m / 32 voxels: Key::kNull


def cpu_query(map_, om, rays, coef=1.0, blocks=None):
    res, _ = rays_query(om, rays, map_.occupancy_threshold_value, coef, map_.ray_filter, blocks=blocks)
    return res


def assert_same(got, want, what=""):
    names = ("ranges", "volumes", "types", "regions", "locals")
    for name, g, w in zip(names, got, want):
        g = np.asarray(g)
        w = np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (what, name, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


def build(map_, rays, cls=GpuMap, **kw):
    gm = cls(map_, **kw)
    om = make_oracle(map_)
    assert gm.integrateRays(rays) == rays.shape[0]
    om.integrate_occupancy(rays)
    return gm, om


def test_rays_query_gpu_restated(gpu):
    """RaysQuery.Gpu: samples only, then the full rays, over the three query scales."""
    map_ = OccupancyMap(0.1)
    rays = reference_rays()
    gm, om = build(map_, hits_only(rays))
    expected = (OccupancyType.kOccupied, OccupancyType.kOccupied, OccupancyType.kFree)
    for iteration, scale in enumerate(QUERY_SCALE):
        q = scaled(rays, scale)
        got = gm.raysQuery(q)
        assert_same(got, cpu_query(map_, om, q), iteration)
        assert (got[2] == expected[iteration]).all()
        assert (got[1] > 0).all() if iteration == 0 else (got[1] == 0).all()
        if iteration == 0:
            assert gm.integrateRays(rays) == rays.shape[0]
            om.integrate_occupancy(rays)


@pytest.mark.parametrize("n", [10, 100, 1000, 10000])
def test_cpu_vs_gpu_random_rays(gpu, n):
    """RaysQuery.CpuVsGpu: random rays in +-10 m build the map, the same rays scaled by 1.2 query it: no mismatch."""
    map_ = OccupancyMap(0.1)
    rays = synth.random_rays(n, extent=10.0, seed=900 + n)
    gm, om = build(map_, rays)
    q = scaled(rays, 1.2)
    got = gm.raysQuery(q)
    assert_same(got, cpu_query(map_, om, q), n)
    assert (got[2] == OccupancyType.kOccupied).any()


def test_cpu_vs_gpu_c1_rays(gpu):
    map_ = OccupancyMap(0.1)
    rays = synth.rays_c1(n=50_000, max_range=12.0)
    gm, om = build(map_, rays)
    q = scaled(rays - rays[0], 1.2) + rays[0]
    assert_same(gm.raysQuery(q), cpu_query(map_, om, q), "c1")


def test_strict_threshold(gpu):
    """threshold_value itself is free, one ulp above it occupied (`>`, not RaysQuery.cl:111's `>=`)."""
    map_ = OccupancyMap(0.1)
    map_.setOccupancyThresholdProbability(0.6)
    thr = np.float32(map_.occupancy_threshold_value)
    assert thr > 0.1
    block = np.full(32 * 32 * 32, np.float32(-1.0), dtype=np.float32)
    block[10 + 0 * 32] = thr                                      # voxel (10, 0, 0)
    block[10 + 1 * 32] = np.nextafter(thr, np.float32(np.inf))   # voxel (10, 1, 0)
    map_.chunks[(0, 0, 0)] = {"occupancy": block}
    gm = GpuMap(map_)
    gm.uploadRegions([(0, 0, 0)])
    # along x through local rows y = 0 and y = 1 of region (0, 0, 0), which spans [-1.6, 1.6)
    rays = np.array([[-1.55, -1.55, -1.55], [1.45, -1.55, -1.55], [-1.55, -1.45, -1.55], [1.45, -1.45, -1.55]])
    got = gm.raysQuery(rays)
    assert list(got[2]) == [OccupancyType.kFree, OccupancyType.kOccupied]
    assert abs(got[0][1] - 0.95) < 1e-6 and abs(got[0][0] - 3.0) < 1e-6
    om = make_oracle(map_)
    assert_same(got, cpu_query(map_, om, rays, blocks=ChunkBlocks(map_.chunks)))


def _filter_rays():
    rays = synth.random_rays(500, extent=6.0, seed=61)
    odd = np.array([
        [np.nan, 0.0, 0.0], [1.0, 1.0, 1.0],
        [0.0, 0.0, 0.0], [np.inf, 1.0, 1.0],
        [0.0, 0.0, 0.0], [FAR, 0.0, 0.0],        # passes, visits nothing: carries
        [0.05, 0.05, 0.05], [9.0, -7.0, 4.0],    # long: clipped / rejected by a short filter range
        [0.0, 0.0, 0.0], [0.0, 0.0, -FAR],
        [-FAR, 0.0, 0.0], [0.0, 0.0, 0.0],
    ])
    return np.concatenate([odd[4:6], rays[:200], odd, rays[200:]])


@pytest.mark.parametrize("ray_filter", [("good", 1e10), ("good", 5.0), ("clip", 5.0), ("clip", 1e10), None])
def test_filter_and_terminal_carry(gpu, ray_filter):
    map_ = OccupancyMap(0.1)
    gm, om = build(map_, synth.random_rays(2000, extent=6.0, seed=60))
    map_.ray_filter = ray_filter
    om.set_ray_filter(*(ray_filter or ("none", 0.0)))
    rays = _filter_rays()
    if ray_filter is None:
        rays = rays[np.isfinite(rays).all(axis=1).reshape(-1, 2).all(axis=1).repeat(2)]
    got = gm.raysQuery(rays)
    want = cpu_query(map_, om, rays)
    assert_same(got, want, ray_filter)
    # the first ray visits nothing and nothing precedes it: kNull and Key::kNull; the carried ones inherit
    if ray_filter != ("clip", 5.0):  # (which walks it, clipped)
        assert got[2][0] == OccupancyType.kNull and tuple(got[3][0]) == (-32768,) * 3
        assert (got[0][0], got[1][0]) == (0.0, 0.0)


def test_edge_rays(gpu):
    map_ = OccupancyMap(0.1)
    gm, om = build(map_, synth.random_rays(1000, extent=3.0, seed=62, origin_spread=1.0))
    occupied_start = np.tile([[0.05, 0.05, 0.05]], (10, 1))  # five hits: occupied whatever the misses before
    gm.integrateRays(occupied_start)
    om.integrate_occupancy(occupied_start)
    special = [[0.05, 0.05, 0.05, 2.0, 0.3, -0.4], [0.05, 0.05, 0.05, 0.05, 0.05, 0.05],
               [0.0501, 0.05, 0.05, 0.0502, 0.05, 0.05]]
    for s in range(1, 6):
        for d in [(1, 0, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (-1, 1, 0), (1, 1, 1), (-1, -1, 1), (1, -1, -1)]:
            special.append([0, 0, 0] + [v * s * 0.7 for v in d])
            special.append([0.05, 0.05, 0.05] + [0.05 + v * s * 0.4 for v in d])
    for k in range(50):
        c = 0.1 * k
        special.append([c - 1e-9, c, c, c + 1e-9, c, c])
        special.append([c, c, c, c, c, c])
        special.append([c, c, c, c + 1e-7, c - 1e-7, c])
    rays = np.array(special, dtype=np.float64).reshape(-1, 3)
    got = gm.raysQuery(rays)
    assert_same(got, cpu_query(map_, om, rays))
    # a start inside an occupied voxel: range 0, occupied
    assert got[2][0] == OccupancyType.kOccupied and got[0][0] == 0.0


@pytest.mark.parametrize("dims,origin", [((64, 64, 64), (0.37, -1.1, 0.25)), ((255, 255, 3), (-0.73, 0.41, 0.15))])
def test_tiled_regions(gpu, dims, origin):
    map_ = OccupancyMap(0.1, dims)
    map_.setOrigin(origin)
    rays = synth.random_rays(3000, extent=12.0, seed=63, origin_spread=2.0)
    gm, om = build(map_, rays)
    q = scaled(rays, 1.2)
    got = gm.raysQuery(q)
    assert_same(got, cpu_query(map_, om, q), dims)
    assert (got[2] == OccupancyType.kOccupied).any() and (got[2] == OccupancyType.kUnobserved).any()


def _spill_rays(k):
    origin = np.array([9.0 * k, 0.3 * k, 0.0])
    return synth.random_rays(4000, extent=4.0, seed=700 + k) + origin


def test_spill_to_host_is_observed_without_side_effects(gpu):
    map_ = OccupancyMap(0.1)
    gm = GpuMap(map_, region_capacity=64)
    gm.setMemoryLimit(100 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    ref_map = OccupancyMap(0.1)
    ref = GpuMap(ref_map)
    twin_map = OccupancyMap(0.1)
    twin = GpuMap(twin_map, region_capacity=64)
    twin.setMemoryLimit(100 * twin.cacheStats()["bytes_per_region"])
    twin.setSpillToHost(True)
    for k in range(5):
        for g in (gm, ref, twin):
            rays = _spill_rays(k)
            assert g.integrateRays(rays) == rays.shape[0]
    st = gm.cacheStats()
    assert st["regions_spilled"] > 0
    q = np.concatenate([_spill_rays(k) for k in range(5)])
    q = scaled(q - q[0], 1.1) + q[0]
    before = (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())
    got = gm.raysQuery(q)
    after = (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())
    assert before == after
    assert_same(got, ref.raysQuery(q), "spill vs unbounded")
    # what follows is what a never-queried map does
    rays = _spill_rays(1)
    for g in (gm, twin):
        assert g.integrateRays(rays) == rays.shape[0]
        g.syncVoxels()
    assert gm.cacheStats() == twin.cacheStats()
    assert map_.chunks.keys() == twin_map.chunks.keys()
    for key in map_.chunks:
        assert np.array_equal(map_.chunks[key]["occupancy"].view(np.uint32), twin_map.chunks[key]["occupancy"].view(np.uint32))


@pytest.mark.parametrize("async_launch", [False, True])
def test_query_observes_collected_rays(gpu, async_launch):
    """Host batches below the coalescing threshold are still collected when the query comes: it launches them first."""
    map_ = OccupancyMap(0.1)
    gm = GpuMap(map_)
    gm.setAsyncLaunch(async_launch)
    om = make_oracle(map_)
    rays = synth.random_rays(3000, extent=5.0, seed=64)
    for part in np.split(rays, 6):
        assert gm.integrateRays(part) == part.shape[0]
        om.integrate_occupancy(part)
    q = scaled(rays, 1.2)
    got = gm.raysQuery(q)
    assert_same(got, cpu_query(map_, om, q))
    assert (got[2] == OccupancyType.kOccupied).sum() > 100


class DeviceBuffer:
    """A library device buffer (ohmhip_buffer_*): what a pipeline that keeps its rays in HBM hands the query."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.handle = L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(self.handle), max(nbytes, 16), 3), "buffer_create")
        self.ptr = L._vp()
        L.check(L.lib.ohmhip_buffer_ptr(self.handle, C.byref(self.ptr)), "buffer_ptr")

    def write(self, array):
        array = np.ascontiguousarray(array)
        L.check(L.lib.ohmhip_buffer_write(self.handle, array.ctypes.data, array.nbytes, 0, None, None, None), "write")

    def read(self, dtype, shape):
        out = np.zeros(shape, dtype=dtype)
        L.check(L.lib.ohmhip_buffer_read(self.handle, out.ctypes.data, out.nbytes, 0, None, None, None), "read")
        return out

    def close(self):
        L.lib.ohmhip_buffer_destroy(self.handle)


def test_device_variant_equals_host_variant(gpu):
    map_ = OccupancyMap(0.1)
    rays = synth.random_rays(5000, extent=8.0, seed=65)
    gm, _ = build(map_, rays)
    q = scaled(rays, 1.2)
    n = q.shape[0] // 2
    host = gm.raysQuery(q, volume_coefficient=0.25)
    bufs = [DeviceBuffer(b) for b in (q.nbytes, 8 * n, 8 * n, n, 10 * n)]
    try:
        bufs[0].write(q)
        gm.raysQueryDevice(bufs[0].ptr, q.shape[0], *[b.ptr for b in bufs[1:]], volume_coefficient=0.25, sync=False)
        gm.wait()
        keys = bufs[4].read(np.uint8, (n, 10))
        dev = (bufs[1].read(np.float64, n), bufs[2].read(np.float64, n), bufs[3].read(np.int8, n),
               keys[:, :6].copy().view(np.int16).reshape(-1, 3), keys[:, 6:9])
        assert_same(dev, host, "device vs host")
        # without keys (the output is optional)
        gm.raysQueryDevice(bufs[0].ptr, q.shape[0], bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, None, volume_coefficient=0.25)
        assert np.array_equal(bufs[3].read(np.int8, n), host[2])
    finally:
        for b in bufs:
            b.close()


def test_ndt_map_occupancy_layer(gpu):
    map_ = OccupancyMap(0.1)
    gm = GpuNdtMap(map_)
    rays = synth.random_rays(3000, extent=6.0, seed=66)
    assert gm.integrateRays(rays) == rays.shape[0]
    q = scaled(rays, 1.2)
    got = gm.raysQuery(q)
    gm.syncVoxels()
    om = make_oracle(map_)
    assert_same(got, cpu_query(map_, om, q, blocks=ChunkBlocks(map_.chunks)))
    assert (got[2] == OccupancyType.kOccupied).any()


def test_tsdf_map_with_the_occupancy_layer(gpu):
    map_ = OccupancyMap(0.1)
    gm = GpuTsdfMap(map_, default_truncation_distance=0.2)
    rays = synth.random_rays(2000, extent=5.0, seed=67)
    assert gm.integrateRays(rays) == rays.shape[0]
    q = scaled(rays, 1.2)
    got = gm.raysQuery(q)
    gm.syncVoxels()
    assert_same(got, cpu_query(map_, make_oracle(map_), q, blocks=ChunkBlocks(map_.chunks)))


def test_refusals(gpu):
    rays = synth.random_rays(10, extent=2.0, seed=68)
    gt = GpuTsdfMap(OccupancyMap(0.1, layers=()), default_truncation_distance=0.2)
    with pytest.raises(OhmHipError) as err:
        gt.raysQuery(rays)
    assert err.value.status == L.ERR_UNSUPPORTED
    owner = GpuMap(OccupancyMap(0.1))
    owner.setRegionOwnership(2, 0)
    with pytest.raises(OhmHipError) as err:
        owner.raysQuery(rays)
    assert err.value.status == L.ERR_UNSUPPORTED


def test_rays_query_gpu_object(gpu):
    map_ = OccupancyMap(0.1)
    rays = synth.random_rays(300, extent=4.0, seed=69)
    gm, om = build(map_, rays)
    query = RaysQueryGpu(gm)
    assert query.queryFlags() & RaysQueryGpu.kQfGpuEvaluate
    query.setVolumeCoefficient(2.0)
    assert query.volumeCoefficient() == 2.0
    q = scaled(rays, 1.2)
    query.setRays(q[:200])
    for i in range(200, q.shape[0], 2):
        query.addRay(q[i], q[i + 1])
    assert query.numberOfRays() == 300
    assert query.execute() and query.wait()
    assert query.numberOfResults() == 300
    want = cpu_query(map_, om, q, coef=2.0)
    got = (query.ranges(), query.unobservedVolumes(), query.terminalOccupancyTypes()) + query.intersectedVoxels()
    assert_same(got, want)
    query.reset(False)
    assert query.numberOfResults() == 0 and query.numberOfRays() == 300
    assert query.executeAsync() and query.wait() and query.numberOfResults() == 300
    query.reset(True)
    assert query.numberOfRays() == 0 and query.numberOfResults() == 0
    query.addRays(q[:20])
    assert query.execute() and query.numberOfResults() == 10
