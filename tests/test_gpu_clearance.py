"""-m gpu: the device clearance queries (ohmhip_map_clearance_regions / _regions_device / _keys) against the CPU
restatement of calculateNearestNeighbour (tests/clearance_ref.py) at EXACT equality.  Restates Ranges.Simple,
OuterEdge, OuterEdgeFromUnknown, OuterEdgeBordered, OuterCorners and Scaling / ScalingGpu (tests/ohmtestgpu/
GpuRangesTests.cpp), whose own tolerances (1e-2, a counted number of failures) are not used here; adds random occupancy
at three densities, half extents from 0 to 40 (the LDS window and the large-window path), odd and tiled region
dimensions, regions far from the origin, the int16 edge, spill to host, an NDT map, the three entry points against each
other, the read-only guarantee and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import ClearanceProcess, GpuMap, GpuNdtMap, GpuTsdfMap, OccupancyMap, OhmHipError, QueryFlag, synth
from ohm_amd import _lib as L
from ohm_amd import distributed as D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clearance_ref import (QF_REPORT_UNSCALED, QF_UNKNOWN_AS_OCCUPIED, DictBlocks, Geometry,  # noqa: E402
                           clearance_keys, clearance_regions, half_extent)
from rays_query_ref import ChunkBlocks  # noqa: E402

pytestmark = pytest.mark.gpu

UAO = QF_UNKNOWN_AS_OCCUPIED
INF = np.float32(np.inf)
HIT = np.float32(np.log(np.float32(0.9) / np.float32(0.1)))
MISS = np.float32(np.log(np.float32(0.45) / np.float32(0.55)))


def crafted(resolution, kd, blocks, origin=None, cls=GpuMap, **kw):
    """A device map holding exactly `blocks` ({region: flat float32 occupancy}) through host chunks + uploadRegions."""
    map_ = OccupancyMap(resolution, kd)
    if origin is not None:
        map_.setOrigin(origin)
    for key, block in blocks.items():
        map_.chunks[key] = {"occupancy": np.asarray(block, dtype=np.float32).copy()}
    gm = cls(map_, **kw)
    gm.uploadRegions(list(blocks))
    return map_, gm


def geometry(map_):
    return Geometry(map_.resolution, map_.region_voxel_dimensions, map_.occupancy_threshold_value)


def assert_equal(got, want, what=""):
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))[0]
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def check_regions(gm, map_, regions, radius, flags=0, scaling=(1.0, 1.0, 1.0), blocks=None, what=""):
    got = gm.clearanceRegions(regions, radius, flags, scaling)
    want = clearance_regions(geometry(map_), blocks or DictBlocks({k: c["occupancy"] for k, c in map_.chunks.items()}),
                             regions, radius, flags, scaling)
    assert_equal(got, want, what)
    return got


def random_blocks(kd, centre, density, seed, missing=(), spread=1):
    """Regions around `centre` (+-spread per axis) of random occupancy: `density` occupied (half of them exactly at the
    threshold 0), the rest free or unobserved; regions in `missing` are left out."""
    rng = np.random.default_rng(seed)
    n = kd[0] * kd[1] * kd[2]
    out = {}
    for dz in range(-spread, spread + 1):
        for dy in range(-spread, spread + 1):
            for dx in range(-spread, spread + 1):
                key = (centre[0] + dx, centre[1] + dy, centre[2] + dz)
                if (dx, dy, dz) in missing:
                    continue
                u = rng.random(n)
                v = np.where(rng.random(n) < 0.2, INF, MISS).astype(np.float32)
                v[u < density] = np.where(rng.random(int((u < density).sum())) < 0.5, HIT, np.float32(0.0))
                out[key] = v
    return out


def radius_for(h, resolution):
    r = 0.0 if h == 0 else float(np.float32((h - 0.5) * resolution))
    assert half_extent(r, resolution) == h
    return r


# -- the reference's Ranges tests, restated at exact equality --------------------------------------------------------

def free_region(kd):
    return np.full(kd[0] * kd[1] * kd[2], MISS, dtype=np.float32)


def test_ranges_simple(gpu):
    """Ranges.Simple: region 0 free but voxel (0, 0, 0), radius 32 voxels: every voxel reports its distance to it."""
    kd = (32, 32, 32)
    block = free_region(kd)
    block[0] = HIT
    map_, gm = crafted(1.0, kd, {(0, 0, 0): block})
    cp = ClearanceProcess(32.0, QueryFlag.kQfGpuEvaluate)
    assert cp.calculateForExtents(gm, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) == [(0, 0, 0)]
    got = cp.regionClearance((0, 0, 0))
    z, y, x = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    d2 = (x * x + y * y + z * z).astype(np.float32)  # centres are exact at resolution 1
    assert_equal(got, np.where(d2 <= 1024, np.sqrt(d2), np.float32(-1.0)))
    rng = np.random.default_rng(1)
    sample = rng.integers(0, 32, size=(200, 3))
    want = clearance_keys(geometry(map_), DictBlocks({(0, 0, 0): block}), np.zeros((200, 3), int), sample, 32.0)
    assert_equal(got[sample[:, 2], sample[:, 1], sample[:, 0]], want)
    assert cp.voxelClearance(((0, 0, 0), (1, 2, 2))) == np.float32(3.0)


@pytest.mark.parametrize("unknown_as_occupied", [False, True])
def test_ranges_outer_edge(gpu, unknown_as_occupied):
    """Ranges.OuterEdge / OuterEdgeFromUnknown: region 0 free, nothing around it, radius 2 voxels."""
    kd = (32, 32, 32)
    map_, gm = crafted(1.0, kd, {(0, 0, 0): free_region(kd)})
    got = check_regions(gm, map_, [(0, 0, 0)], 2.0, UAO if unknown_as_occupied else 0)
    if unknown_as_occupied:
        assert got[0, 0, 5, 5] == 1.0 and got[0, 5, 5, 5] == -1.0 and got[0, 0, 0, 0] == 1.0
    else:
        assert (got == -1.0).all()


def test_ranges_outer_edge_bordered(gpu):
    """Ranges.OuterEdgeBordered: a box room whose walls are the layers of the six neighbouring regions next to
    region 0."""
    kd = (32, 32, 32)
    blocks = {(0, 0, 0): free_region(kd)}
    for axis in range(3):
        for side in (-1, 1):
            key = [0, 0, 0]
            key[axis] = side
            b = free_region(kd).reshape(32, 32, 32)  # [z][y][x]
            sl = [slice(None)] * 3
            sl[2 - axis] = 31 if side < 0 else 0
            b[tuple(sl)] = HIT
            blocks[tuple(key)] = b.reshape(-1)
    map_, gm = crafted(1.0, kd, blocks)
    got = check_regions(gm, map_, [(0, 0, 0)], 2.0)
    assert got[0, 5, 5, 0] == 1.0 and got[0, 5, 5, 1] == 2.0 and got[0, 5, 5, 5] == -1.0


def test_ranges_outer_corners(gpu):
    """Ranges.OuterCorners: obstacles diagonally outside region 0's eight corners, radius 8 voxels."""
    kd = (32, 32, 32)
    blocks = {(0, 0, 0): free_region(kd)}
    thr = np.float32(0.0)
    for cz in (-1, 1):
        for cy in (-1, 1):
            for cx in (-1, 1):
                b = free_region(kd)
                lx, ly, lz = (31 if cx < 0 else 0), (31 if cy < 0 else 0), (31 if cz < 0 else 0)
                b[lx + ly * 32 + lz * 1024] = thr + HIT
                blocks[(cx, cy, cz)] = b
    map_, gm = crafted(1.0, kd, blocks)
    got = check_regions(gm, map_, [(0, 0, 0)], 8.0)
    for z in (0, 31):
        for y in (0, 31):
            for x in (0, 31):
                assert got[0, z, y, x] == np.sqrt(np.float32(3.0))


@pytest.mark.parametrize("region_dim", [8, 32])
def test_ranges_scaling(gpu, region_dim):
    """Ranges.Scaling / ScalingGpu: res 0.25, origin -0.125, hits 2, 3 and 4 voxels from the voxel at the origin; the
    four axis scalings select each in turn (exact values)."""
    kd = (region_dim,) * 3
    map_ = OccupancyMap(0.25, kd)
    map_.setOrigin((-0.125, -0.125, -0.125))
    gm = GpuMap(map_)
    hits = np.array([[0.5, 0, 0], [0, 0.75, 0], [0, 0, 1.0]], dtype=np.float64)
    gm.integrateRays(np.repeat(hits, 2, axis=0))  # zero-length rays: integrateHit
    gm.syncVoxels()
    cp = ClearanceProcess(2.0, QueryFlag.kQfGpuEvaluate)
    origin_key = ((0, 0, 0), (region_dim // 2,) * 3)
    for scaling, expected, report_scaled in [((1.0, 1.0, 1.0), 0.5, False), ((4.0, 1.0, 1.0), 0.75, False),
                                             ((1.0, 1.0, 1.0 / 3.0), 1.0, False), ((1.1, 1.1, 0.25), 0.25, True)]:
        cp.setQueryFlags(QueryFlag.kQfGpuEvaluate | (0 if report_scaled else QueryFlag.kQfReportUnscaledResults))
        cp.setAxisScaling(scaling)
        cp.reset()
        assert cp.calculateForExtents(gm, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)) == [(0, 0, 0)]
        assert cp.voxelClearance(origin_key) == np.float32(expected), scaling
        want = clearance_regions(geometry(map_), ChunkBlocks(map_.chunks), [(0, 0, 0)], 2.0, cp.queryFlags(),
                                 [np.float32(v) for v in scaling])
        assert_equal(cp.regionClearance((0, 0, 0)), want[0], scaling)


# -- random occupancy, window sizes, region shapes ---------------------------------------------------------------------

@pytest.mark.parametrize("density", [0.001, 0.05, 0.5])
@pytest.mark.parametrize("flags", [0, UAO])
def test_random_density(gpu, density, flags):
    kd = (32, 32, 32)
    blocks = random_blocks(kd, (0, 0, 0), density, seed=int(density * 1000) + flags, missing=((1, 0, 0), (0, -1, 1)))
    map_, gm = crafted(0.1, kd, blocks)
    for h in (2, 5):
        check_regions(gm, map_, [(0, 0, 0), (1, 0, 0)], radius_for(h, 0.1), flags, what=(h, density))


@pytest.mark.parametrize("h", [0, 1, 2, 5, 16, 32, 40])
def test_half_extents_small_regions(gpu, h):
    """8^3 regions: h <= 32 runs the LDS window, 40 the large-window path."""
    kd = (8, 8, 8)
    spread = max(1, (h + 7) // 8)
    blocks = random_blocks(kd, (0, 0, 0), 0.002 if h > 5 else 0.05, seed=40 + h, spread=spread,
                           missing=((1, 1, 1), (-1, 0, 0)))
    map_, gm = crafted(0.1, kd, blocks)
    for flags, scaling in ((0, (1.0, 1.0, 1.0)), (UAO | QF_REPORT_UNSCALED, (1.0, 0.5, 2.0))):
        check_regions(gm, map_, [(0, 0, 0), (-1, 0, 0)], radius_for(h, 0.1), flags, scaling, what=(h, flags))


@pytest.mark.parametrize("h", [16, 32])
def test_large_windows_full_regions(gpu, h):
    """32^3 regions at h = 16 and 32 (the LDS window's upper end): a sample of voxels against the reference, all of them
    against key mode."""
    kd = (32, 32, 32)
    blocks = random_blocks(kd, (0, 0, 0), 0.0005, seed=70 + h, missing=((0, 0, 1),))
    map_, gm = crafted(0.1, kd, blocks)
    radius = radius_for(h, 0.1)
    got = gm.clearanceRegions([(0, 0, 0)], radius)[0]
    rng = np.random.default_rng(h)
    sample = rng.integers(0, 32, size=(60, 3))
    want = clearance_keys(geometry(map_), DictBlocks(blocks), np.zeros((60, 3), int), sample, radius)
    assert_equal(got[sample[:, 2], sample[:, 1], sample[:, 0]], want)
    z, y, x = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    locals_ = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)
    keyed = gm.clearanceKeys((np.zeros_like(locals_), locals_), radius)
    assert_equal(got.reshape(-1), keyed)
    assert (got > 0).any()


@pytest.mark.parametrize("h", [2, 5, 16])
def test_odd_region_dims(gpu, h):
    kd = (10, 12, 7)
    blocks = random_blocks(kd, (0, 0, 0), 0.03, seed=80 + h, spread=2 if h == 16 else 1)
    map_, gm = crafted(0.1, kd, blocks)
    check_regions(gm, map_, [(0, 0, 0), (1, -1, 0)], radius_for(h, 0.1), UAO if h == 5 else 0, (1.0, 1.0, 0.7))


def test_tiled_regions(gpu):
    """64^3 regions are cut into tiles inside the library; results are in the caller's region coordinates."""
    kd = (64, 64, 64)
    blocks = random_blocks(kd, (0, 0, 0), 0.01, seed=90, missing=((0, 1, 0),))
    map_, gm = crafted(0.1, kd, blocks)
    check_regions(gm, map_, [(0, 0, 0), (1, 1, 1)], radius_for(2, 0.1), UAO)
    check_regions(gm, map_, [(-1, 0, 0)], radius_for(3, 0.1), 0, (1.0, 2.0, 1.0))


@pytest.mark.parametrize("centre", [(1000, -1000, 999), (-1001, 998, -1000)])
def test_far_from_origin(gpu, centre):
    """Far from the origin fp32 centres round: separations are not multiples of the resolution, integer reasoning
    would select differently.  A non-zero map origin does not enter (voxelCentreLocal)."""
    kd = (32, 32, 32)
    blocks = random_blocks(kd, centre, 0.05, seed=abs(centre[0]))
    map_, gm = crafted(0.1, kd, blocks, origin=(12.3, -4.5, 0.7))
    got = check_regions(gm, map_, [centre], radius_for(3, 0.1), QF_REPORT_UNSCALED, (1.0, 1.0, 1.0))
    check_regions(gm, map_, [centre], radius_for(4, 0.1), UAO, (np.float32(0.9), 1.0, np.float32(1.1)))
    # the fp32 separations really are not the integer ones
    vals = np.unique(got[got > 0])
    ints = np.sqrt(np.arange(1, 28, dtype=np.float32) * np.float32(0.01))
    assert not np.isin(vals, ints).all()


def test_int16_edge(gpu):
    """A window that crosses the int16 edge: region 32767's neighbour in +x is region -32768 (moveKey wraps)."""
    kd = (8, 8, 8)
    blocks = {}
    for rx in (32766, 32767, -32768, -32767):
        blocks[(rx, 0, 0)] = random_blocks(kd, (0, 0, 0), 0.05, seed=rx & 0xff, spread=0)[(0, 0, 0)]
    map_, gm = crafted(0.1, kd, blocks)
    scaling = (np.float32(1e-6), 1.0, 1.0)
    got = check_regions(gm, map_, [(32767, 0, 0), (-32768, 0, 0)], radius_for(5, 0.1), 0, scaling)
    check_regions(gm, map_, [(32767, 0, 0), (-32768, 0, 0)], radius_for(5, 0.1), UAO)
    assert (got > 0).any()


# -- the map as it is used: spill to host, NDT, entry points, read only ------------------------------------------------

def _spill_rays(k):
    origin = np.array([9.0 * k, 0.3 * k, 0.0])
    return synth.random_rays(3000, extent=4.0, seed=710 + k) + origin


def _observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


def _region_bytes(gm, keys):
    keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
    n = gm.map().regionVoxelVolume()
    out = np.zeros((keys.shape[0], n), dtype=np.float32)
    dsts = (C.c_void_p * max(1, keys.shape[0]))(*[out[i].ctypes.data for i in range(keys.shape[0])])
    L.check(L.lib.ohmhip_map_read_regions(gm._handle, L.LID_OCCUPANCY, keys.ctypes.data, keys.shape[0], dsts), "read")
    return out


def test_spill_to_host_read_only(gpu):
    """Regions in the host store answer from their pinned records, without re-admission; the query changes nothing."""
    map_ = OccupancyMap(0.1)
    gm = GpuMap(map_, region_capacity=64)
    gm.setMemoryLimit(100 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    ref_map = OccupancyMap(0.1)
    ref = GpuMap(ref_map)
    for k in range(5):
        for g in (gm, ref):
            rays = _spill_rays(k)
            assert g.integrateRays(rays) == rays.shape[0]
    assert gm.cacheStats()["regions_spilled"] > 0
    keys = gm.regionKeys()
    assert sorted(map(tuple, keys)) == sorted(map(tuple, ref.regionKeys()))
    before_bytes = _region_bytes(gm, keys)
    before = _observe(gm)
    flags = UAO
    got = gm.clearanceRegions(keys, 0.25, flags)
    keyed = gm.clearanceKeys((keys[:3], np.array([[0, 0, 0], [31, 5, 17], [4, 31, 0]])), 0.25, flags)
    assert _observe(gm) == before
    assert np.array_equal(_region_bytes(gm, keys).view(np.uint32), before_bytes.view(np.uint32))
    assert_equal(got, ref.clearanceRegions(keys, 0.25, flags), "spill vs unbounded")
    assert_equal(keyed, [got[0, 0, 0, 0], got[1, 17, 5, 31], got[2, 0, 31, 4]])
    ref.syncVoxels()
    sample = keys[:: max(1, keys.shape[0] // 4)][:4]
    want = clearance_regions(geometry(ref_map), ChunkBlocks(ref_map.chunks), sample, 0.25, flags)
    idx = [int(np.nonzero((keys == s).all(axis=1))[0][0]) for s in sample]
    assert_equal(got[idx], want)


def test_ndt_map(gpu):
    map_ = OccupancyMap(0.1)
    gm = GpuNdtMap(map_)
    rays = synth.random_rays(3000, extent=6.0, seed=666)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    keys = np.array(sorted(map_.chunks)[:3], dtype=np.int16)
    check_regions(gm, map_, keys, 0.3, 0, blocks=ChunkBlocks(map_.chunks))
    check_regions(gm, map_, keys[:1], 0.3, UAO, blocks=ChunkBlocks(map_.chunks))


class DeviceBuffer:
    def __init__(self, nbytes):
        self.handle = L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(self.handle), max(nbytes, 16), 3), "buffer_create")
        self.ptr = L._vp()
        L.check(L.lib.ohmhip_buffer_ptr(self.handle, C.byref(self.ptr)), "buffer_ptr")

    def read(self, dtype, shape):
        out = np.zeros(shape, dtype=dtype)
        L.check(L.lib.ohmhip_buffer_read(self.handle, out.ctypes.data, out.nbytes, 0, None, None, None), "read")
        return out

    def close(self):
        L.lib.ohmhip_buffer_destroy(self.handle)


@pytest.mark.parametrize("h", [3, 40])
def test_host_device_and_key_variants_agree(gpu, h):
    kd = (16, 16, 16)
    blocks = random_blocks(kd, (0, 0, 0), 0.02, seed=120 + h, spread=1 if h < 16 else 3)
    map_, gm = crafted(0.1, kd, blocks)
    keys = np.array([(0, 0, 0), (1, 0, -1), (5, 5, 5)], dtype=np.int16)
    radius = radius_for(h, 0.1)
    host = gm.clearanceRegions(keys, radius, UAO)
    buf = DeviceBuffer(host.nbytes)
    try:
        gm.clearanceRegionsDevice(keys, buf.ptr, radius, UAO, sync=False)
        gm.wait()
        assert_equal(buf.read(np.float32, host.shape), host)
    finally:
        buf.close()
    z, y, x = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    locals_ = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1)
    for i, key in enumerate(keys):
        keyed = gm.clearanceKeys((np.repeat(key[None, :], locals_.shape[0], axis=0), locals_), radius, UAO)
        assert_equal(keyed, host[i].reshape(-1))
    assert (host[2] == 0).all()  # a region not in the map: unknown, so every voxel obstructs
    if h == 3:
        want = clearance_regions(geometry(map_), DictBlocks(blocks), keys[:2], radius, UAO)
        assert_equal(host[:2], want)


def test_threshold_change_is_seen(gpu):
    kd = (8, 8, 8)
    block = free_region(kd)
    block[3 + 3 * 8 + 3 * 64] = np.float32(0.5)
    map_, gm = crafted(0.1, kd, {(0, 0, 0): block})
    assert gm.clearanceKeys(((np.zeros((1, 3), int)), np.array([[3, 3, 3]])), 0.3)[0] == 0.0
    map_.setOccupancyThresholdProbability(0.7)
    assert gm.clearanceKeys(((np.zeros((1, 3), int)), np.array([[3, 3, 3]])), 0.3)[0] == -1.0
    check_regions(gm, map_, [(0, 0, 0)], 0.3)


def test_refusals(gpu):
    map_, gm = crafted(0.1, (8, 8, 8), {(0, 0, 0): free_region((8, 8, 8))})
    keys = [(0, 0, 0)]

    def status(fn):
        with pytest.raises(OhmHipError) as err:
            fn()
        return err.value.status

    assert status(lambda: gm.clearanceRegions(keys, -0.5)) == L.ERR_INVALID_ARG
    assert status(lambda: gm.clearanceRegions(keys, float("nan"))) == L.ERR_INVALID_ARG
    assert status(lambda: gm.clearanceRegions(keys, float("inf"))) == L.ERR_INVALID_ARG
    assert status(lambda: gm.clearanceRegions(keys, 0.5, 0, (1.0, 0.0, 1.0))) == L.ERR_INVALID_ARG
    assert status(lambda: gm.clearanceRegions(keys, 0.5, 0, (1.0, 1.0, float("inf")))) == L.ERR_INVALID_ARG
    assert status(lambda: gm.clearanceKeys((np.zeros((1, 3), int), np.array([[8, 0, 0]])), 0.5)) == L.ERR_INVALID_ARG
    assert status(lambda: gm.clearanceRegions(keys, 12.75)) == L.ERR_UNSUPPORTED   # h = 128
    assert gm.clearanceRegions(keys, 12.65).shape == (1, 8, 8, 8)                  # h = 127
    p = L.ClearanceParams()
    p.search_radius = 0.5
    for i in range(3):
        p.axis_scaling[i] = 1.0
    k = np.zeros((1, 3), dtype=np.int16)
    assert L.lib.ohmhip_map_clearance_regions(gm._handle, k.ctypes.data, 1, C.byref(p), None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_regions(gm._handle, None, 1, C.byref(p), None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_keys(gm._handle, k.ctypes.data, 1, None, k.ctypes.data) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_regions_device(gm._handle, k.ctypes.data, 1, C.byref(p), None) == \
        L.ERR_INVALID_ARG
    gt = GpuTsdfMap(OccupancyMap(0.1, layers=()), default_truncation_distance=0.2)
    assert status(lambda: gt.clearanceRegions(keys, 0.5)) == L.ERR_UNSUPPORTED
    owner = GpuMap(OccupancyMap(0.1))
    owner.setRegionOwnership(2, 0)
    assert status(lambda: owner.clearanceRegions(keys, 0.5)) == L.ERR_UNSUPPORTED
    part = D.territories_from_origins([(0.0, 0.0, 0.0), (20.0, 0.0, 0.0)], 2, 0, (3.2, 3.2, 3.2), block_shift=0,
                                     margin=5.0)
    partitioned = GpuMap(OccupancyMap(0.1))
    partitioned.setRegionPartition(part)
    assert status(lambda: partitioned.clearanceKeys((np.zeros((1, 3), int), np.zeros((1, 3), int)), 0.5)) == \
        L.ERR_UNSUPPORTED
