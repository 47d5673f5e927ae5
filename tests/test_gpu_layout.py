"""-m gpu: layers added to and removed from a live device map (include/ohmhip.h "LAYER CHANGES", ohmhip_map_update_layers;
OccupancyMap::updateLayout and the add*Layer calls, ohm/OccupancyMap.cpp:521-682).

The yardstick is never the code under test alone: it is a TWIN map created with the final layer set and brought to the
same state through create, integrateRays and ohmhip_map_write_regions.  Comparisons are bit for bit -- the bytes
ohmhip_map_read_regions returns for every region and layer, equal region-key sets, compareVoxels with no tolerance --
but for the covariance floats of the NDT case (1e-5, as tests/test_gpu_ndt_tsdf.py)."""
import ctypes as C

import numpy as np
import pytest

import layout_ref as R
from ohm_amd import (ClearanceProcess, GpuMap, GpuNdtMap, GpuTsdfMap, LAYERS, NdtMode, OccupancyMap, OhmHipError,
                     compareVoxels, extract_cloud, synth)
from ohm_amd import _lib as L
from parity import compare_layer

pytestmark = pytest.mark.gpu

ALL_SECONDARY = ("mean", "traversal", "touch_time", "incident_normal")


def new_map(layers=("occupancy",), dims=(16, 16, 16), resolution=0.1, cls=GpuMap, capacity=32, **kwargs):
    map_ = OccupancyMap(resolution, dims, layers=layers)
    return cls(map_, region_capacity=capacity, **kwargs)


def stamps(rays, start):
    return start + 0.01 * np.arange(rays.shape[0] // 2, dtype=np.float64)


def integrate(gm, rays, start=None):
    ts = None if start is None else stamps(rays, start)
    assert gm.integrateRays(rays, timestamps=ts) == rays.shape[0]


def region_set(gm):
    return sorted(tuple(k) for k in gm.regionKeys().tolist())


def snapshot(gm, layers=None):
    """(sorted region keys, {layer: (regions, words) uint32}) through ohmhip_map_read_regions."""
    keys = np.array(region_set(gm), dtype=np.int16).reshape(-1, 3)
    rv = gm.map().regionVoxelVolume()
    out = {}
    for name in (layers if layers is not None else gm.map().layers):
        lid = LAYERS[name][0]
        blocks = np.zeros((len(keys), rv * R.LAYER_BYTES[name] // 4), dtype=np.uint32)
        ptrs = (C.c_void_p * max(len(keys), 1))(*[blocks[i].ctypes.data for i in range(len(keys))])
        L.check(L.lib.ohmhip_map_read_regions(gm._handle, lid, keys.ctypes.data, len(keys), ptrs), "read_regions")
        out[name] = blocks
    return [tuple(k) for k in keys.tolist()], out


def assert_same(a, b, layers=None):
    keys_a, blocks_a = a
    keys_b, blocks_b = b
    assert keys_a == keys_b
    for name in (layers if layers is not None else sorted(set(blocks_a) | set(blocks_b))):
        differing = int(np.count_nonzero(blocks_a[name] != blocks_b[name]))
        assert differing == 0, "%s: %d words differ" % (name, differing)


def reset_layers(gm, names):
    """Every region's block of the named layers becomes a cleared block, through ohmhip_map_write_regions."""
    keys = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16).reshape(-1, 3)
    rv = gm.map().regionVoxelVolume()
    for name in names:
        block = R.clear_block(name, rv)
        ptrs = (C.c_void_p * len(keys))(*([block.ctypes.data] * len(keys)))
        L.check(L.lib.ohmhip_map_write_regions(gm._handle, LAYERS[name][0], keys.ctypes.data, len(keys), ptrs), "write")


def device_layers(gm):
    mask = C.c_uint(0)
    L.check(L.lib.ohmhip_map_layers(gm._handle, C.byref(mask)), "layers")
    return int(mask.value)


def layer_ptr(gm, name):
    ptr, stride = C.c_void_p(0), C.c_size_t(0)
    status = L.lib.ohmhip_map_device_layer_ptr(gm._handle, LAYERS[name][0], C.byref(ptr), C.byref(stride))
    return status, ptr.value, int(stride.value)


def status_of(fn):
    with pytest.raises(OhmHipError) as err:
        fn()
    return err.value.status


# -- 1 -------------------------------------------------------------------------------------------------------------------
def test_voxel_mean_layout_toggle(gpu):
    """VoxelMean.LayoutToggle (tests/ohmtestgpu/GpuVoxelMeanTests.cpp:143-244) with its numbers."""
    import mean_ref
    resolution = 0.5
    gm = new_map(dims=(32, 32, 32), resolution=resolution, capacity=8)
    cached_layout = list(gm.map().layers)
    sample = np.array([[1.1, 1.1, 1.1]])
    assert gm.integrateHits(points=sample) == 1
    key = gm.voxelKeys(sample)
    centre = np.array([1.25, 1.25, 1.25])
    threshold = np.float32(gm.map().occupancy_threshold_value)

    def position():
        cloud = extract_cloud(gm)
        assert cloud.count == 1 and len(cloud) == 1  # the one voxel, occupied
        return cloud.positions[0]

    assert np.array_equal(position(), centre)
    occupancy_before = snapshot(gm, ["occupancy"])

    gm.addVoxelMeanLayer()
    assert gm.voxelMeanEnabled() and gm.map().layers == ["occupancy", "mean"]
    assert device_layers(gm) == R.layer_mask(["occupancy", "mean"])  # two layers
    assert_same(snapshot(gm, ["occupancy"]), occupancy_before)
    value, present = gm.readVoxels(key, "occupancy")
    assert present[0] == 1 and value[0] >= threshold
    mean, present = gm.readVoxels(key, "mean")
    assert present[0] == 1 and mean.tolist() == [[0, 0]]

    coord = mean_ref.coord_ref(tuple(float(v) for v in (sample[0] - centre)), resolution)
    assert gm.writeVoxels(key, "mean", np.array([[coord, 1]], dtype=np.uint32)) == 1
    moved = position()
    assert np.all(np.abs(moved - sample[0]) <= resolution / 1000.0) and np.all(moved != centre)

    gm.updateLayout(cached_layout)
    assert not gm.voxelMeanEnabled() and gm.map().layers == ["occupancy"]
    assert device_layers(gm) == R.layer_mask(["occupancy"])  # one layer
    assert_same(snapshot(gm, ["occupancy"]), occupancy_before)
    value, _ = gm.readVoxels(key, "occupancy")
    assert value[0] >= threshold
    assert status_of(lambda: gm.readVoxels(key, "mean")) == L.ERR_UNSUPPORTED
    assert np.array_equal(position(), centre)


# -- 2, 6 ----------------------------------------------------------------------------------------------------------------
def added_layers_case(dims, rays1, rays2, capacity):
    start = ("occupancy",)
    final = start + ALL_SECONDARY
    gm = new_map(start, dims, capacity=capacity)
    integrate(gm, rays1, 100.0)
    first_regions = set(region_set(gm))
    ptr_before = layer_ptr(gm, "occupancy")
    gm.updateLayout(final)
    assert layer_ptr(gm, "occupancy") == ptr_before
    stats = gm.lastLayerChangeStats()
    rv = gm.map().regionVoxelVolume()
    assert (stats["layers_before"], stats["layers_after"]) == (R.layer_mask(start), R.layer_mask(final))
    assert stats["bytes_per_region_before"] == R.bytes_per_region(start, min(rv, 1 << 15))
    assert stats["bytes_per_region_after"] == R.bytes_per_region(final, min(rv, 1 << 15))
    assert stats["regions_evicted"] == 0 and stats["regions_in_store"] == 0
    integrate(gm, rays2, 200.0)
    assert set(region_set(gm)) - first_regions, "the second batch must enter a region the first never touched"

    twin = new_map(final, dims, capacity=capacity)
    integrate(twin, rays1, 100.0)
    reset_layers(twin, ALL_SECONDARY)
    integrate(twin, rays2, 200.0)
    assert_same(snapshot(gm), snapshot(twin))
    for name in final:
        assert compareVoxels(gm, twin, name), name
    return gm, twin


def test_added_layers_start_now(gpu):
    # (32 slots: the second batch outgrows the pool, so the pool is rebuilt with the new set as well)
    gm, _ = added_layers_case((16, 16, 16), synth.random_rays(150, extent=1.5, seed=11),
                              synth.random_rays(200, extent=4.0, seed=12), capacity=32)
    assert gm.cacheStats()["region_capacity"] > 32
    for name in ALL_SECONDARY:
        assert snapshot(gm, [name])[1][name].any(), name  # (the comparison is of layers that hold something)


def test_added_layers_on_tiled_regions(gpu):
    """Regions of 64 x 32 x 32 voxels: two tiles each."""
    added_layers_case((64, 32, 32), synth.random_rays(100, extent=2.0, seed=21),
                      synth.random_rays(120, extent=4.0, seed=22), capacity=32)


# -- 3 -------------------------------------------------------------------------------------------------------------------
def test_tsdf_map_gains_and_loses_traversal(gpu):
    rays = [synth.random_rays(120, extent=e, seed=s) for e, s in ((1.5, 31), (3.0, 32), (3.0, 33))]
    gm = new_map(("tsdf",), cls=GpuTsdfMap)
    integrate(gm, rays[0])
    tsdf_ptr = layer_ptr(gm, "tsdf")
    gm.addTraversalLayer()
    assert gm.traversalEnabled() and layer_ptr(gm, "tsdf") == tsdf_ptr
    integrate(gm, rays[1])
    twin = new_map(("tsdf", "traversal"), cls=GpuTsdfMap)
    integrate(twin, rays[0])
    reset_layers(twin, ["traversal"])
    integrate(twin, rays[1])
    assert_same(snapshot(gm), snapshot(twin))
    tsdf_ptr = layer_ptr(gm, "tsdf")  # (the second batch may have outgrown the pool)
    gm.removeLayer("traversal")
    assert not gm.traversalEnabled() and layer_ptr(gm, "tsdf") == tsdf_ptr
    assert layer_ptr(gm, "traversal")[0] == L.ERR_NOT_FOUND
    integrate(gm, rays[2])
    plain = new_map(("tsdf",), cls=GpuTsdfMap)
    for r in rays:
        integrate(plain, r)
    assert gm.map().layers == ["tsdf"]
    assert_same(snapshot(gm), snapshot(plain))


# -- 4 -------------------------------------------------------------------------------------------------------------------
def test_ndt_map_gains_touch_time_and_hit_miss(gpu):
    def clustered(n, extent, seed):
        rays = synth.random_rays(n, extent=extent, seed=seed)
        rays[1::2] = np.round(rays[1::2] / 0.4) * 0.4 + 0.013 * np.sin(np.arange(n))[:, None]
        return rays
    rays1, rays2 = clustered(300, 1.5, 41), clustered(300, 3.0, 42)
    added = ("touch_time", "hit_miss_count")
    gm = new_map(cls=GpuNdtMap)
    integrate(gm, rays1, 50.0)
    gm.addTouchTimeLayer()
    gm.addLayer("hit_miss_count")
    assert gm.touchTimeEnabled() and gm.hasLayer("hit_miss_count")
    integrate(gm, rays2, 60.0)
    twin = new_map(("occupancy", "mean", "covariance") + added, cls=GpuNdtMap)
    integrate(twin, rays1, 50.0)
    reset_layers(twin, added)
    integrate(twin, rays2, 60.0)
    (keys, have), (twin_keys, expect) = snapshot(gm), snapshot(twin)
    assert keys == twin_keys and sorted(have) == sorted(expect)
    for name in have:
        if name == "covariance":  # float members: 1e-5 relative
            assert compare_layer(name, expect[name].view(np.float32).ravel(), have[name].view(np.float32).ravel()) == 0
        else:
            assert np.array_equal(have[name], expect[name]), name
    assert have["touch_time"].any() and have["covariance"].any()


# -- 5, 9 ----------------------------------------------------------------------------------------------------------------
def stop_rays(stop, n, seed):
    """Rays that stay inside region (stop, 0, 0) of a 16^3 map at 0.1 m, which spans 1.6 (stop +- 0.5): one region per
    batch."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.empty((2 * n, 3), dtype=np.float64)
    rays[0::2] = np.array([1.6 * stop, 0.0, 0.0]) + 0.013
    rays[1::2] = rays[0::2] + d * rng.uniform(0.2, 0.6, n)[:, None]
    return rays


STOPS = 12
RV16 = 16 * 16 * 16


def sweep(gm, seed, order):
    for stop in order:
        integrate(gm, stop_rays(stop, 24, seed + stop))


def spilling_map(layers, regions):
    gm = new_map(layers, capacity=4)  # (the limit bounds the pool's growth: the pool starts below it)
    per_region = gm.cacheStats()["bytes_per_region"]
    assert per_region == R.bytes_per_region(layers, RV16)
    gm.setMemoryLimit(regions * per_region)
    gm.setSpillToHost(True)
    return gm, regions * per_region


@pytest.mark.parametrize("writeback", [False, True])
def test_layer_changes_on_a_spilling_map(gpu, writeback):
    gm, limit = spilling_map(("occupancy",), 6)
    gm.setSpillWriteback(writeback)
    forward, backward = list(range(STOPS)), list(range(STOPS - 1, -1, -1))
    sweep(gm, 500, forward)
    before = gm.cacheStats()
    assert before["regions_resident"] + before["regions_spilled"] == STOPS and before["regions_spilled"] >= STOPS - 6
    dirty_before = sorted(tuple(k) for k in gm.regionKeys(dirty_only=True).tolist())
    occupancy_before = snapshot(gm, ["occupancy"])

    gm.addLayer("mean")
    stats = gm.lastLayerChangeStats()
    with_mean = ("occupancy", "mean")
    assert stats["bytes_per_region_after"] == R.bytes_per_region(with_mean, RV16) == gm.cacheStats()["bytes_per_region"]
    evicted = R.regions_to_evict(before["regions_resident"], limit, with_mean, RV16)
    assert evicted > 0 and stats["regions_evicted"] == evicted
    assert stats["regions_resident"] == before["regions_resident"] - evicted
    assert stats["regions_in_store"] == before["regions_spilled"] + evicted
    assert_same(snapshot(gm, ["occupancy"]), occupancy_before)  # resident and stored regions alike
    assert not snapshot(gm, ["mean"])[1]["mean"].any()
    assert sorted(tuple(k) for k in gm.regionKeys(dirty_only=True).tolist()) == dirty_before  # U6

    sweep(gm, 600, backward)  # re-admits regions from rewritten records
    after = gm.cacheStats()
    assert after["readmissions"] > before["readmissions"]
    assert after["regions_resident"] <= limit // R.bytes_per_region(with_mean, RV16)
    twin = new_map(with_mean, capacity=32)
    sweep(twin, 500, forward)
    reset_layers(twin, ["mean"])
    sweep(twin, 600, backward)
    assert_same(snapshot(gm), snapshot(twin))

    gm.removeLayer("mean")
    assert gm.lastLayerChangeStats()["regions_evicted"] == 0
    assert gm.cacheStats()["bytes_per_region"] == R.bytes_per_region(("occupancy",), RV16)
    sweep(gm, 700, forward)
    plain = new_map(("occupancy",), capacity=32)
    for seed, order in ((500, forward), (600, backward), (700, forward)):
        sweep(plain, seed, order)
    assert_same(snapshot(gm), snapshot(plain))


def test_remove_and_add_again_yields_a_cleared_layer(gpu):
    gm, _ = spilling_map(("occupancy", "mean"), 5)
    sweep(gm, 800, range(STOPS))
    st = gm.cacheStats()
    assert st["regions_resident"] > 0 and st["regions_spilled"] > 0
    keys, before = snapshot(gm)
    assert before["mean"].any(axis=1).all()  # every region, resident or stored, holds means
    gm.removeLayer("mean")
    gm.addLayer("mean")
    keys_after, after = snapshot(gm)
    assert keys_after == keys and not after["mean"].any()
    assert np.array_equal(after["occupancy"], before["occupancy"])
    assert gm.cacheStats()["regions_spilled"] > 0  # (still a map with stored regions)


# -- 7 -------------------------------------------------------------------------------------------------------------------
def test_pending_rays_run_under_the_old_layer_set(gpu):
    rays1 = synth.random_rays(200, extent=2.0, seed=71)
    rays2 = synth.random_rays(150, extent=2.5, seed=72)
    gm = new_map()
    for at in range(0, rays1.shape[0], 100):  # calls of 50 rays: collected, not launched
        part = rays1[at:at + 100]
        assert gm.integrateRays(part) == part.shape[0]  # each call reports its own count
    assert gm.batchesLaunched() == 0
    gm.addTraversalLayer()
    assert gm.batchesLaunched() == 1  # the collected rays ran as one batch, before the layer existed
    integrate(gm, rays2)
    gm.syncVoxels()
    twin = new_map(("occupancy", "traversal"))
    integrate(twin, rays1)
    reset_layers(twin, ["traversal"])
    integrate(twin, rays2)
    have, expect = snapshot(gm), snapshot(twin)
    assert_same(have, expect)
    assert have[1]["traversal"].any()
    only_second = new_map(("occupancy", "traversal"))
    integrate(only_second, rays2)
    keys2, second = snapshot(only_second, ["traversal"])
    rows = [have[0].index(k) for k in keys2]
    assert np.array_equal(have[1]["traversal"][rows], second["traversal"])  # the second batch's lengths only
    assert not np.delete(have[1]["traversal"], rows, axis=0).any()


# -- 8 -------------------------------------------------------------------------------------------------------------------
def test_clearance_layer_added_and_removed(gpu):
    rays = synth.random_rays(150, extent=2.0, seed=81)
    gm = new_map()
    integrate(gm, rays)
    with pytest.raises(RuntimeError):
        ClearanceProcess.ensureClearanceLayer(gm)
    gm.addLayer("clearance")
    ClearanceProcess.ensureClearanceLayer(gm)
    stale = sorted(tuple(k) for k in gm.clearanceStaleRegions(0.5).tolist())
    assert stale == region_set(gm)  # every region
    assert np.all(snapshot(gm, ["clearance"])[1]["clearance"] == R.CLEAR_WORD["clearance"])
    processed, remaining = gm.clearanceUpdate(0.5)
    assert processed == len(stale) and remaining == 0
    twin = new_map(("occupancy", "clearance"))
    integrate(twin, rays)
    twin.clearanceUpdate(0.5)
    have, expect = snapshot(gm), snapshot(twin)
    assert_same(have, expect)
    assert np.any(have[1]["clearance"] != R.CLEAR_WORD["clearance"])
    assert len(gm.clearanceStaleRegions(0.5)) == 0
    gm.removeLayer("clearance")
    assert status_of(lambda: gm.clearanceUpdate(0.5)) == L.ERR_UNSUPPORTED
    assert status_of(lambda: gm.clearanceStaleRegions(0.5)) == L.ERR_UNSUPPORTED
    # added again: nothing of the earlier computation is remembered
    gm.addLayer("clearance")
    assert sorted(tuple(k) for k in gm.clearanceStaleRegions(0.5).tolist()) == region_set(gm)
    assert np.all(snapshot(gm, ["clearance"])[1]["clearance"] == R.CLEAR_WORD["clearance"])


# -- 10 ------------------------------------------------------------------------------------------------------------------
def test_retained_layers_do_not_move(gpu):
    gm = new_map(("occupancy", "mean"))
    integrate(gm, synth.random_rays(100, extent=2.0, seed=91))
    retained = {name: layer_ptr(gm, name) for name in ("occupancy", "mean")}
    assert all(status == L.OK and ptr for status, ptr, _ in retained.values())
    assert retained["mean"][2] == RV16 * 8
    content = snapshot(gm)
    gm.updateLayout(["occupancy", "mean", "covariance", "clearance"])
    assert {name: layer_ptr(gm, name) for name in retained} == retained
    added = layer_ptr(gm, "covariance")
    assert added[0] == L.OK and added[2] == RV16 * 24 and added[1] not in [p for _, p, _ in retained.values()]
    gm.updateLayout(["occupancy", "mean", "clearance"])
    assert {name: layer_ptr(gm, name) for name in retained} == retained
    assert layer_ptr(gm, "covariance")[0] == L.ERR_NOT_FOUND
    clearance = layer_ptr(gm, "clearance")
    # the mask the map has already: nothing happens
    stats = L.LayerChangeStats()
    mask = R.layer_mask(["occupancy", "mean", "clearance"])
    assert L.lib.ohmhip_map_update_layers(gm._handle, mask, 0, C.byref(stats)) == L.OK
    assert (stats.layers_before, stats.layers_after, stats.regions_evicted) == (mask, mask, 0)
    assert stats.regions_resident == len(content[0])
    assert {name: layer_ptr(gm, name) for name in retained} == retained and layer_ptr(gm, "clearance") == clearance
    gm.updateLayout(["occupancy", "mean"])
    assert_same(snapshot(gm), content)


# -- 11 ------------------------------------------------------------------------------------------------------------------
def state_of(gm):
    return (snapshot(gm), sorted(tuple(k) for k in gm.regionKeys(dirty_only=True).tolist()), device_layers(gm),
            gm.cacheStats(), list(gm.map().layers), {name: layer_ptr(gm, name) for name in gm.map().layers})


def assert_refused(gm, layers, status, reference=None):
    before = state_of(gm)
    stats = L.LayerChangeStats(1, 2, 3, 4, 5, 6, 7)
    assert L.lib.ohmhip_map_update_layers(gm._handle, R.layer_mask(layers), 0, C.byref(stats)) == status
    assert bytes(stats) == bytes(C.sizeof(stats))
    assert status_of(lambda: gm.updateLayout(layers)) == status  # the mirror raises and keeps its own view
    after = state_of(gm)
    assert_same(after[0], before[0])
    assert after[1:] == before[1:]
    if reference is not None:
        assert_same(after[0], snapshot(reference))
        for name in gm.map().layers:
            assert compareVoxels(gm, reference, name), name


@pytest.mark.parametrize("cls,kwargs,layers,without", [
    (GpuMap, {}, ("occupancy", "mean"), "occupancy"),
    (GpuNdtMap, {}, ("occupancy",), "covariance"),
    (GpuNdtMap, {}, ("occupancy",), "mean"),
    (GpuNdtMap, {"ndt_mode": NdtMode.kTraversability}, ("occupancy",), "hit_miss_count"),
    (GpuNdtMap, {"ndt_mode": NdtMode.kTraversability}, ("occupancy",), "intensity"),
    (GpuTsdfMap, {}, ("tsdf", "traversal"), "tsdf"),
])
def test_required_layers_stay(gpu, cls, kwargs, layers, without):
    gm = new_map(layers, cls=cls, **kwargs)
    rays = synth.random_rays(80, extent=1.5, seed=111)
    intensities = np.ones(80, dtype=np.float32) if kwargs else None
    assert gm.integrateRays(rays, intensities=intensities) == rays.shape[0]
    reference = gm.clone()
    assert_refused(gm, [n for n in gm.map().layers if n != without], L.ERR_UNSUPPORTED, reference)
    # (an optional layer of the same map may go and come)
    gm.addLayer("touch_time")
    gm.removeLayer("touch_time")
    assert_same(snapshot(gm), snapshot(reference))


def test_partitioned_and_merging_maps_are_refused(gpu):
    rays = synth.random_rays(80, extent=1.5, seed=112)
    owner = new_map()
    owner.setRegionOwnership(2, 0)
    owner.integrateRays(rays)
    assert_refused(owner, ["occupancy", "mean"], L.ERR_UNSUPPORTED)
    merging = new_map()
    integrate(merging, rays)
    L.check(L.lib.ohmhip_map_enable_merge(merging._handle), "enable_merge")
    assert_refused(merging, ["occupancy", "mean"], L.ERR_UNSUPPORTED)


def test_a_set_that_does_not_fit_the_limit_without_spill(gpu):
    gm = new_map()
    sweep(gm, 900, range(4))
    reference = gm.clone()
    per_region = gm.cacheStats()["bytes_per_region"]
    gm.setMemoryLimit(4 * per_region)
    assert_refused(gm, ["occupancy", "mean"], L.ERR_CAPACITY, reference)
    gm.setMemoryLimit(4 * R.bytes_per_region(("occupancy", "mean"), RV16))
    gm.addLayer("mean")  # (fits now)
    assert gm.lastLayerChangeStats()["regions_evicted"] == 0 and gm.hasLayer("mean")


def test_invalid_arguments_on_a_live_map(gpu):
    gm = new_map()
    integrate(gm, synth.random_rays(50, extent=1.5, seed=113))
    before = state_of(gm)
    update = L.lib.ohmhip_map_update_layers
    assert update(gm._handle, 0, 0, None) == L.ERR_INVALID_ARG
    assert update(gm._handle, 1 | (1 << L.LID_COUNT), 0, None) == L.ERR_INVALID_ARG
    assert update(gm._handle, 3, 2, None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_layers(gm._handle, None) == L.ERR_INVALID_ARG
    after = state_of(gm)
    assert_same(after[0], before[0])
    assert after[1:] == before[1:]


# -- 12 ------------------------------------------------------------------------------------------------------------------
def test_discard_map(gpu):
    gm, _ = spilling_map(("occupancy", "mean"), 5)
    sweep(gm, 1000, range(STOPS))
    assert gm.cacheStats()["regions_spilled"] > 0
    gm.syncVoxels()
    assert gm.map().chunks
    final = ["occupancy", "traversal", "touch_time"]
    gm.updateLayout(final, preserve_map=False)
    assert len(gm.regionKeys()) == 0 and not gm.map().chunks
    st = gm.cacheStats()
    assert st["regions_resident"] == 0 and st["regions_spilled"] == 0
    assert device_layers(gm) == R.layer_mask(final) and gm.map().layers == final
    assert gm.lastLayerChangeStats()["regions_resident"] == 0
    gm.setMemoryLimit(0)
    rays = synth.random_rays(150, extent=2.0, seed=121)
    integrate(gm, rays, 10.0)
    fresh = new_map(tuple(final))
    integrate(fresh, rays, 10.0)
    assert_same(snapshot(gm), snapshot(fresh))


# -- 13 ------------------------------------------------------------------------------------------------------------------
def test_host_map_follows(gpu):
    gm = new_map()
    map_ = gm.map()
    integrate(gm, synth.random_rays(100, extent=1.5, seed=131))
    gm.syncVoxels()
    synced = set(map_.chunks)
    gm.addLayer("mean")
    rv = map_.regionVoxelVolume()
    assert all(chunk["mean"].shape == (2 * rv,) and not chunk["mean"].any() for chunk in map_.chunks.values())
    integrate(gm, synth.random_rays(100, extent=3.0, seed=132))
    gm.syncVoxels()
    keys, blocks = snapshot(gm)
    assert set(keys) == set(map_.chunks) and set(keys) - synced
    for row, key in enumerate(keys):
        for name in ("occupancy", "mean"):
            assert np.array_equal(map_.chunks[key][name].view(np.uint32), blocks[name][row]), (key, name)
    assert blocks["mean"].any()
    region = np.repeat(np.array(keys, dtype=np.int16), 2, axis=0)
    local = np.tile(np.array([[1, 2, 3], [15, 0, 7]], dtype=np.uint8), (len(keys), 1))
    values, present = gm.readVoxels((region, local), "mean")
    index = local[:, 0].astype(int) + 16 * local[:, 1].astype(int) + 256 * local[:, 2].astype(int)
    expect = np.stack([blocks["mean"][np.arange(len(region)) // 2, 2 * index],
                       blocks["mean"][np.arange(len(region)) // 2, 2 * index + 1]], axis=1)
    assert present.all() and np.array_equal(values, expect)
    gm.removeLayer("mean")
    assert all(sorted(chunk) == ["occupancy"] for chunk in map_.chunks.values()) and "mean" not in gm._block_addr
