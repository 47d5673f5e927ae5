"""-m gpu: the clearance layer kept by ohmhip_map_clearance_update (ClearanceProcess.update / Mapper.update).  Every value
is compared with `==`: the layer against the clearance query over the map as it stands (itself held to tests/
clearance_ref.py) and against clearance_ref directly on samples; the stale list against the log restatement of tests/
clearance_update_ref.py.  Restates Mapper.Clearance (tests/ohmtestgpu/GpuMapperTests.cpp) on the reference's inputs,
exactly instead of within compareMaps' tolerance."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (ClearanceProcess, GpuMap, GpuNdtMap, Mapper, MappingProcessResult, OccupancyMap, OhmHipError,
                     QueryFlag, synth)
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clearance_ref import QF_UNKNOWN_AS_OCCUPIED, Geometry, clearance_regions, half_extent  # noqa: E402
from clearance_update_ref import ClearanceLog, params_of  # noqa: E402
from rays_query_ref import ChunkBlocks  # noqa: E402
from stdrandom import Mt19937  # noqa: E402

pytestmark = pytest.mark.gpu

UAO = QF_UNKNOWN_AS_OCCUPIED
MISS = np.float32(np.log(np.float32(0.45) / np.float32(0.55)))
HIT = np.float32(np.log(np.float32(0.9) / np.float32(0.1)))


def radius_for(h, resolution):
    r = float(np.float32((h - 0.5) * resolution))
    assert half_extent(r, resolution) == h
    return r


def keyset(keys):
    return sorted(tuple(int(v) for v in k) for k in np.asarray(keys).reshape(-1, 3))


def read_layer(gm, keys, lid=L.LID_CLEARANCE, dtype=np.float32, comps=1):
    """A layer of the listed regions, (N, dz, dy, dx[, comps]), without touching the dirty set."""
    keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
    dx, dy, dz = gm.map().region_voxel_dimensions
    out = np.zeros((keys.shape[0], dz * dy * dx * comps), dtype=dtype)
    dsts = (C.c_void_p * max(1, keys.shape[0]))(*[out[i].ctypes.data for i in range(keys.shape[0])])
    L.check(L.lib.ohmhip_map_read_regions(gm._handle, lid, keys.ctypes.data, keys.shape[0], dsts), "read")
    return out.reshape((keys.shape[0], dz, dy, dx) + ((comps,) if comps > 1 else ()))


def assert_equal(got, want, what=""):
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.reshape(-1).view(np.uint32) != want.reshape(-1).view(np.uint32))[0]
    assert bad.size == 0, (what, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def assert_layer_exact(gm, radius, flags=0, scaling=(1.0, 1.0, 1.0), what=""):
    keys = gm.regionKeys()
    assert_equal(read_layer(gm, keys), gm.clearanceRegions(keys, radius, flags, scaling), what)
    return keys


def new_map(resolution=0.1, kd=(32, 32, 32), cls=GpuMap, **kw):
    map_ = OccupancyMap(resolution, kd, layers=("occupancy",))
    ClearanceProcess.ensureClearanceLayer(map_)
    return map_, cls(map_, **kw)


def rays_at(n, centre, extent, seed):
    return synth.random_rays(n, extent=extent, seed=seed) + np.asarray(centre, dtype=np.float64)


def integrate(gm, rays):
    assert gm.integrateRays(rays) == rays.shape[0]


# -- 1. no regression ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [GpuMap, GpuNdtMap])
def test_layer_changes_nothing_else(gpu, cls):
    plain_map = OccupancyMap(0.1, (32, 32, 32))
    plain = cls(plain_map)
    layer_map, with_layer = new_map(cls=cls)
    assert with_layer.hasLayer("clearance") and not plain.hasLayer("clearance")
    for k in range(3):
        rays = rays_at(6000, (0.5 * k, 0.0, 0.0), 5.0, 900 + k)
        for g in (plain, with_layer):
            integrate(g, rays)
        with_layer.wait()
        plain.wait()
        counts = [{k: v for k, v in g.stats().items() if not k.startswith("ms_")} for g in (plain, with_layer)]
        assert counts[0] == counts[1]
    keys = plain.regionKeys()
    assert keyset(keys) == keyset(with_layer.regionKeys())
    assert keyset(plain.regionKeys(True)) == keyset(with_layer.regionKeys(True))
    assert np.all(read_layer(with_layer, keys) == np.float32(-1.0))
    plain.syncVoxels()
    with_layer.syncVoxels()
    for k in plain_map.chunks:
        for name in plain_map.layers:
            a, b = plain_map.chunks[k][name], layer_map.chunks[k][name]
            assert a.tobytes() == b.tobytes(), (k, name)
        assert np.all(layer_map.chunks[k]["clearance"] == np.float32(-1.0))


# -- 2. full update --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,flags,scaling", [(2, 0, (1.0, 1.0, 1.0)), (2, UAO, (1.0, 1.0, 1.0)),
                                             (5, 0, (1.0, 1.0, 1.0)), (5, UAO, (1.0, 1.0, 1.0)),
                                             (5, 0, (1.0, 2.0, 0.5)), (33, 0, (1.0, 1.0, 1.0))])
def test_full_update(gpu, h, flags, scaling):
    map_, gm = new_map()
    for k in range(2):
        integrate(gm, rays_at(8000, (0.0, 0.3 * k, 0.0), 6.0, 920 + k))
    radius = radius_for(h, 0.1)
    cp = ClearanceProcess(radius, flags)
    cp.setAxisScaling(scaling)
    assert cp.update(gm) == MappingProcessResult.kMprUpToDate
    keys = gm.regionKeys()
    want = gm.clearanceRegions(keys, radius, flags, scaling)
    gm.syncVoxels()
    got = np.stack([map_.chunks[tuple(int(v) for v in k)]["clearance"].reshape(want.shape[1:]) for k in keys])
    assert_equal(got, want, "layer vs query")
    if h <= 5:
        sample = keys[:: max(1, len(keys) // 3)][:3]
        ref = clearance_regions(Geometry(0.1, (32, 32, 32), map_.occupancy_threshold_value), ChunkBlocks(map_.chunks),
                                sample, radius, flags, scaling)
        idx = [int(np.nonzero((keys == s).all(axis=1))[0][0]) for s in sample]
        assert_equal(got[idx], ref, "layer vs clearance_ref")
    assert gm.clearanceStaleRegions(radius, flags, scaling).shape[0] == 0


# -- 3. incremental --------------------------------------------------------------------------------------------------

def test_incremental_update(gpu):
    map_, gm = new_map()
    radius = radius_for(5, 0.1)
    p = params_of(radius)
    log = ClearanceLog(0.1, (32, 32, 32))
    integrate(gm, rays_at(20000, (0.0, 0.0, 0.0), 8.0, 930))
    log.change(gm.regionKeys(True))
    assert keyset(gm.clearanceStaleRegions(radius)) == keyset(log.stale(gm.regionKeys(), p))
    assert gm.clearanceUpdate(radius) == (len(gm.regionKeys()), 0)
    log.written(gm.regionKeys(), p)
    gm.syncVoxels()
    # B: a small local batch
    integrate(gm, rays_at(300, (2.0, 1.0, 0.5), 0.6, 931))
    gm.wait()
    changed = keyset(gm.regionKeys(True))
    assert 0 < len(changed) < len(gm.regionKeys())
    log.change(changed)
    stale = [tuple(int(v) for v in k) for k in gm.clearanceStaleRegions(radius)]
    want = log.stale(gm.regionKeys(), p)
    assert stale == want  # (in processing order)
    assert len(stale) < len(gm.regionKeys())
    assert gm.clearanceUpdate(radius) == (len(stale), 0)
    assert keyset(gm.regionKeys(True)) == sorted(set(changed) | set(stale))
    assert_layer_exact(gm, radius, what="incremental")


# -- 4. D = 2 --------------------------------------------------------------------------------------------------------

def test_reach_two_regions(gpu):
    """16^3 regions, h = 20: a change two regions away reaches R.  A one-region pad misses it."""
    kd = (16, 16, 16)
    map_, gm = new_map(0.1, kd)
    for x in range(5):
        map_.chunks[(x, 0, 0)] = {"occupancy": np.full(16 ** 3, MISS, dtype=np.float32)}
    gm.uploadRegions()
    radius = radius_for(20, 0.1)
    gm.clearanceUpdate(radius)
    before = read_layer(gm, [(0, 0, 0)])
    assert np.all(before == np.float32(-1.0))  # nothing within reach
    occ = np.full(16 ** 3, MISS, dtype=np.float32)
    occ[(8 * 16 + 8) * 16 + 0] = HIT  # local (0, 8, 8) of region (2, 0, 0): 17 voxels from region 0's far face
    map_.chunks[(2, 0, 0)] = {"occupancy": occ}
    gm.uploadRegions([(2, 0, 0)])
    stale = keyset(gm.clearanceStaleRegions(radius))
    assert stale == keyset([(x, 0, 0) for x in range(5)])
    gm.clearanceUpdate(radius)
    after = read_layer(gm, [(0, 0, 0)])
    assert np.any(after != np.float32(-1.0))
    assert_layer_exact(gm, radius, what="D = 2")


# -- 5. partial updates ----------------------------------------------------------------------------------------------

def test_partial_updates(gpu):
    map_, gm = new_map()
    integrate(gm, rays_at(10000, (0.0, 0.0, 0.0), 7.0, 940))
    radius = radius_for(5, 0.1)
    order = [tuple(int(v) for v in k) for k in gm.clearanceStaleRegions(radius)]
    assert order == sorted(order, key=lambda k: (k[2], k[1], k[0]))
    assert len(order) > 6
    gm.syncVoxels()
    processed, remaining = gm.clearanceUpdate(radius, max_regions=4)
    assert (processed, remaining) == (4, len(order) - 4)
    assert keyset(gm.regionKeys(True)) == sorted(order[:4])
    assert [tuple(int(v) for v in k) for k in gm.clearanceStaleRegions(radius)] == order[4:]
    assert_equal(read_layer(gm, order[:4]), gm.clearanceRegions(order[:4], radius))
    assert np.all(read_layer(gm, order[4:]) == np.float32(-1.0))
    cp = ClearanceProcess(radius)
    while cp.update(gm, time_slice=1e-9, max_regions=3) != MappingProcessResult.kMprUpToDate:
        pass
    assert_layer_exact(gm, radius, what="partial")
    gm.syncVoxels()
    assert gm.clearanceUpdate(radius) == (0, 0)
    assert cp.update(gm) == MappingProcessResult.kMprUpToDate
    assert gm.regionKeys(True).shape[0] == 0


# -- 6. parameter changes --------------------------------------------------------------------------------------------

def test_parameter_changes(gpu):
    map_, gm = new_map()
    integrate(gm, rays_at(6000, (0.0, 0.0, 0.0), 5.0, 950))
    radius = radius_for(3, 0.1)
    gm.clearanceUpdate(radius)
    all_keys = keyset(gm.regionKeys())
    assert gm.clearanceStaleRegions(radius).shape[0] == 0
    assert keyset(gm.clearanceStaleRegions(radius_for(4, 0.1))) == all_keys
    assert keyset(gm.clearanceStaleRegions(radius, UAO)) == all_keys
    assert keyset(gm.clearanceStaleRegions(radius, 0, (1.0, 1.0, 2.0))) == all_keys
    assert gm.clearanceStaleRegions(radius, int(QueryFlag.kQfNoCache)).shape[0] == 0  # (changes no result)
    gm.clearanceUpdate(radius, UAO)
    assert_layer_exact(gm, radius, UAO, what="new flags")
    assert keyset(gm.clearanceStaleRegions(radius)) == all_keys


# -- 7. host writes --------------------------------------------------------------------------------------------------

def test_host_writes(gpu):
    map_, gm = new_map()
    integrate(gm, rays_at(8000, (0.0, 0.0, 0.0), 6.0, 960))
    radius = radius_for(5, 0.1)
    p = params_of(radius)
    log = ClearanceLog(0.1, (32, 32, 32))
    gm.clearanceUpdate(radius)
    log.written(gm.regionKeys(), p)
    gm.syncVoxels()
    keys = gm.regionKeys()
    target = tuple(int(v) for v in keys[len(keys) // 2])
    # occupancy upload (uploadRegions of a chunk holding occupancy only): the neighbourhood
    occ = map_.chunks[target]["occupancy"].copy()
    occ[::97] = HIT
    saved = map_.chunks[target]
    map_.chunks[target] = {"occupancy": occ}
    gm.uploadRegions([target])
    map_.chunks[target] = saved
    log.change([target])
    assert [tuple(int(v) for v in k) for k in gm.clearanceStaleRegions(radius)] == log.stale(gm.regionKeys(), p)
    gm.clearanceUpdate(radius)
    log.written(gm.regionKeys(), p)
    assert_layer_exact(gm, radius, what="after occupancy upload")
    # clearance layer written by the host: that region only
    block = np.zeros(32 ** 3, dtype=np.float32)
    k = np.array([target], dtype=np.int16)
    ptrs = (C.c_void_p * 1)(block.ctypes.data)
    L.check(L.lib.ohmhip_map_write_regions(gm._handle, L.LID_CLEARANCE, k.ctypes.data, 1, ptrs), "write")
    log.host_write([target])
    assert keyset(gm.clearanceStaleRegions(radius)) == [target] == log.stale(gm.regionKeys(), p)
    gm.clearanceUpdate(radius)
    assert_layer_exact(gm, radius, what="after clearance write")


# -- 8. removal ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, UAO])
def test_removal(gpu, flags):
    map_, gm = new_map()
    integrate(gm, rays_at(8000, (0.0, 0.0, 0.0), 6.0, 970))
    radius = radius_for(5, 0.1)
    p = params_of(radius, flags)
    log = ClearanceLog(0.1, (32, 32, 32))
    gm.clearanceUpdate(radius, flags)
    log.written(gm.regionKeys(), p)
    keys = gm.regionKeys()
    target = tuple(int(v) for v in keys[len(keys) // 3])
    assert gm.removeRegions([target]) == 1
    log.remove([target])
    stale = [tuple(int(v) for v in k) for k in gm.clearanceStaleRegions(radius, flags)]
    assert stale == log.stale(gm.regionKeys(), p) and stale
    gm.clearanceUpdate(radius, flags)
    assert_layer_exact(gm, radius, flags, what="after removal")


# -- 9. spill to host ------------------------------------------------------------------------------------------------

def test_spill_to_host(gpu):
    map_, gm = new_map(region_capacity=64)
    gm.setMemoryLimit(100 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    for k in range(5):
        integrate(gm, rays_at(3000, (9.0 * k, 0.3 * k, 0.0), 4.0, 710 + k))
    stats = gm.cacheStats()
    assert stats["regions_spilled"] > 0
    keys = keyset(gm.regionKeys())
    radius = radius_for(4, 0.1)
    gm.clearanceUpdate(radius, UAO)
    assert gm.cacheStats() == stats
    assert keyset(gm.regionKeys()) == keys
    assert_layer_exact(gm, radius, UAO, what="spilled")
    # re-admission of spilled regions (and the evictions it forces) is no change
    arr = np.array(keys, dtype=np.int16)
    occ_before, layer_before = read_layer(gm, arr, L.LID_OCCUPANCY), read_layer(gm, arr)
    L.check(L.lib.ohmhip_map_ensure_regions(gm._handle, arr[:40].ctypes.data, 40, None), "ensure")
    L.check(L.lib.ohmhip_map_ensure_regions(gm._handle, arr[-40:].ctypes.data, 40, None), "ensure")
    moved = gm.cacheStats()
    assert moved["readmissions"] > stats["readmissions"] and moved["evictions"] > stats["evictions"]
    assert gm.clearanceStaleRegions(radius, UAO).shape[0] == 0
    assert_equal(read_layer(gm, arr, L.LID_OCCUPANCY), occ_before, "occupancy moved with the regions")
    assert_equal(read_layer(gm, arr), layer_before, "clearance moved with the regions")


# -- 10. tiled and odd regions ---------------------------------------------------------------------------------------

def test_tiled_regions(gpu):
    """64^3 regions are cut into 64 x 64 x 8 tiles; a tile no ray reached is not created and reads -1."""
    map_, gm = new_map(0.1, (64, 64, 64))
    integrate(gm, rays_at(6000, (0.0, 0.0, 0.0), 6.0, 980))
    radius = radius_for(5, 0.1)
    gm.clearanceUpdate(radius)
    keys = gm.regionKeys()
    got = read_layer(gm, keys)
    want = gm.clearanceRegions(keys, radius)
    occ = read_layer(gm, keys, L.LID_OCCUPANCY)
    for r in range(len(keys)):
        for z0 in range(0, 64, 8):
            g, w = got[r, z0:z0 + 8], want[r, z0:z0 + 8]
            if np.all(np.isinf(occ[r, z0:z0 + 8])) and np.all(g == np.float32(-1.0)):
                continue  # (an absent tile)
            assert_equal(g, w, (tuple(keys[r]), z0))
    assert gm.clearanceStaleRegions(radius).shape[0] == 0


@pytest.mark.parametrize("h", [5, 12])
def test_odd_regions(gpu, h):
    map_, gm = new_map(0.1, (5, 7, 9))
    integrate(gm, rays_at(4000, (0.0, 0.0, 0.0), 2.0, 990))
    radius = radius_for(h, 0.1)
    gm.clearanceUpdate(radius)
    assert_layer_exact(gm, radius, what="odd")
    log = ClearanceLog(0.1, (5, 7, 9))
    p = params_of(radius)
    log.written(gm.regionKeys(), p)
    gm.syncVoxels()
    integrate(gm, rays_at(50, (0.5, 0.5, 0.5), 0.3, 991))
    gm.wait()
    log.change(gm.regionKeys(True))
    stale = [tuple(int(v) for v in k) for k in gm.clearanceStaleRegions(radius)]
    assert stale == log.stale(gm.regionKeys(), p) and len(stale) < len(gm.regionKeys())
    gm.clearanceUpdate(radius)
    assert_layer_exact(gm, radius, what="odd, incremental")


# -- 11. refusals ----------------------------------------------------------------------------------------------------

def test_refusals(gpu):
    def status(fn):
        with pytest.raises(OhmHipError) as err:
            fn()
        return err.value.status

    plain = GpuMap(OccupancyMap(0.1))
    assert status(lambda: plain.clearanceUpdate(0.5)) == L.ERR_UNSUPPORTED
    assert status(lambda: plain.clearanceStaleRegions(0.5)) == L.ERR_UNSUPPORTED
    assert status(lambda: plain.clearanceUpdateRegions([(0, 0, 0)], 0.5)) == L.ERR_UNSUPPORTED
    with pytest.raises(RuntimeError):
        ClearanceProcess.ensureClearanceLayer(plain)
    _, owner = new_map()
    owner.setRegionOwnership(2, 0)
    assert status(lambda: owner.clearanceUpdate(0.5)) == L.ERR_UNSUPPORTED
    _, gm = new_map()
    assert status(lambda: gm.clearanceUpdate(12.75)) == L.ERR_UNSUPPORTED  # h = 128
    assert status(lambda: gm.clearanceStaleRegions(-0.5)) == L.ERR_INVALID_ARG
    assert status(lambda: gm.clearanceUpdate(0.5, 0, (1.0, 0.0, 1.0))) == L.ERR_INVALID_ARG
    k = np.zeros((1, 3), dtype=np.int16)
    assert L.lib.ohmhip_map_clearance_update_regions(gm._handle, None, 1, None, 1, None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_stale_regions(gm._handle, None, k.ctypes.data, 1, None) == L.ERR_INVALID_ARG
    # kQfInstantiateUnknown creates nothing
    cp = ClearanceProcess(0.5, ClearanceProcess.kQfInstantiateUnknown)
    assert cp.calculateForExtents(gm, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    assert gm.regionKeys().shape[0] == 0


# -- calculateForExtents ---------------------------------------------------------------------------------------------

def test_calculate_for_extents_writes_the_layer(gpu):
    map_, gm = new_map()
    integrate(gm, rays_at(6000, (0.0, 0.0, 0.0), 5.0, 995))
    radius = radius_for(4, 0.1)
    cp = ClearanceProcess(radius)
    keys = cp.calculateForExtents(gm, (-6.0, -6.0, -6.0), (6.0, 6.0, 6.0))
    assert keyset(keys) == keyset(gm.regionKeys())
    for k in keys:
        assert_equal(read_layer(gm, [k])[0], cp.regionClearance(k))
    assert gm.clearanceStaleRegions(radius).shape[0] == 0
    gm.syncVoxels()
    cp.calculateForExtents(gm, (-6.0, -6.0, -6.0), (6.0, 6.0, 6.0), force=False)
    assert gm.regionKeys(True).shape[0] == 0  # nothing was stale: nothing rewritten
    cp.calculateForExtents(gm, (-6.0, -6.0, -6.0), (6.0, 6.0, 6.0), force=True)
    assert keyset(gm.regionKeys(True)) == keyset(keys)


# -- 12. Mapper.Clearance --------------------------------------------------------------------------------------------

def mapper_rays():
    """tests/ohmtestgpu/GpuMapperTests.cpp: 128 k rays from (0.05, 0.05, 0.05) to a spherical shell of radius 9-10 m,
    drawn from a default std::mt19937 (x, y, z in [-1, 1), then the length, per ray)."""
    n = 1024 * 128
    u = Mt19937().uniform(0.0, 1.0, 4 * n).reshape(n, 4)
    d = u[:, :3] * 2.0 + -1.0
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    length = u[:, 3] * 1.0 + 9.0
    rays = np.empty((2 * n, 3), dtype=np.float64)
    rays[0::2] = 0.05
    rays[1::2] = d * length[:, None]
    return rays


def test_mapper_clearance(gpu):
    map_ = OccupancyMap(0.25, (32, 32, 32))
    cp = ClearanceProcess(3.0, int(QueryFlag.kQfGpuEvaluate))
    cp.ensureClearanceLayer(map_)
    gm = GpuMap(map_, True, 2048 * 2)
    mapper = Mapper(gm)
    mapper.addProcess(cp)
    rays = mapper_rays()
    for i in range(0, rays.shape[0], 2048 * 2):
        integrate(gm, rays[i:i + 2048 * 2])
        mapper.update(0.001, max_regions=2)
    gm.syncVoxels()
    assert mapper.update(0.0) == MappingProcessResult.kMprUpToDate
    gm.syncVoxels()
    # the clone: the same occupancy in a fresh map, clearance calculated for the whole extent
    clone_map = OccupancyMap(0.25, (32, 32, 32))
    ClearanceProcess.ensureClearanceLayer(clone_map)
    for k, c in map_.chunks.items():
        clone_map.chunks[k] = {"occupancy": c["occupancy"].copy()}
    clone = GpuMap(clone_map)
    clone_cp = ClearanceProcess(3.0, int(QueryFlag.kQfGpuEvaluate))
    keys = clone_cp.calculateForExtents(clone, (-11.0, -11.0, -11.0), (11.0, 11.0, 11.0))
    assert keyset(keys) == keyset(list(map_.chunks))
    clone.syncVoxels()
    for k in keys:
        assert_equal(map_.chunks[k]["clearance"], clone_map.chunks[k]["clearance"], k)
        assert_equal(map_.chunks[k]["clearance"].reshape(32, 32, 32), clone_cp.regionClearance(k), k)
