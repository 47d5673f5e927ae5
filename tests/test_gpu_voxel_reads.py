"""-m gpu: voxels read by key (ohmhip_map_read_voxels / _device, GpuMap.readVoxels / occupancyTypes) against the bytes
ohmhip_map_read_regions delivers for the same voxels, and ohmhip_map_voxel_keys against the oracle's voxelKey -- exact
equality throughout.  An NDT-TM map with every secondary layer plus clearance and a TSDF map; absent regions, null keys,
a tiled region with an empty tile, regions in the host store, duplicates, an empty request, the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (GPU_KEY_DTYPE, LAYERS, ClearanceProcess, GpuMap, GpuNdtMap, GpuTsdfMap, MappingProcessResult, NdtMode,
                     OccupancyMap, OccupancyType, OhmHipError)
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbours_ref as NR  # noqa: E402
from heightmap_cases import two_level_scene  # noqa: E402
from parity import make_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
CLEAR = {"occupancy": np.float32(np.inf), "clearance": np.float32(-1.0)}


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def make_keys(regions, locals_):
    keys = np.zeros(len(regions), dtype=GPU_KEY_DTYPE)
    keys["region"] = np.asarray(regions, dtype=np.int16).reshape(-1, 3)
    keys["voxel"][:, :3] = np.asarray(locals_, dtype=np.uint8).reshape(-1, 3)
    return keys


def null_key():
    return make_keys([(-32768, -32768, -32768)], [(0, 0, 0)])


def expected(map_, keys, name):
    """The bytes of the host chunks (as ohmhip_map_read_regions synced them) at the keys; clear values elsewhere."""
    _, dtype, comps = LAYERS[name]
    dx, dy, _ = map_.region_voxel_dimensions
    values = np.zeros((len(keys), comps), dtype=dtype)
    values[:] = CLEAR.get(name, 0)
    present = np.zeros(len(keys), dtype=np.uint8)
    for i, k in enumerate(keys):
        region = tuple(int(v) for v in k["region"])
        chunk = map_.chunks.get(region)
        if chunk is None or region == (-32768, -32768, -32768):
            continue
        index = int(k["voxel"][0]) + dx * int(k["voxel"][1]) + dx * dy * int(k["voxel"][2])
        values[i] = np.asarray(chunk[name], dtype=dtype).reshape(-1, comps)[index]
        present[i] = 1
    return (values if comps > 1 else values.reshape(-1)), present


def seeded_keys(map_, rng, n=200):
    """~n keys: voxels of present regions (duplicates included), of absent regions, and null keys."""
    regions = sorted(map_.chunks)
    dims = map_.region_voxel_dimensions
    pick = rng.integers(0, len(regions), size=n)
    locals_ = np.stack([rng.integers(0, dims[a], size=n) for a in range(3)], axis=1)
    keys = make_keys([regions[i] for i in pick], locals_)
    absent = make_keys([(40, 40, 40), (-300, 2, 1), (32767, -32768, 0)], [(0, 0, 0), (5, 6, 2), (dims[0] - 1, 0, 1)])
    keys = np.concatenate([keys, keys[:20], absent, null_key(), keys[5:6], null_key()])
    return keys[rng.permutation(len(keys))]


def check_layers(gm, map_, keys, names):
    for name in names:
        want_values, want_present = expected(map_, keys, name)
        values, present = gm.readVoxels(keys, name)
        assert values.dtype == want_values.dtype and values.shape == want_values.shape, name
        assert np.array_equal(raw(values), raw(want_values)), name
        assert np.array_equal(present, want_present), name
    return want_present


@pytest.fixture(scope="module")
def ndt_scene(gpu):
    layers = ("occupancy", "mean", "covariance", "traversal", "touch_time", "incident_normal", "intensity",
              "hit_miss_count")
    map_ = OccupancyMap(0.1, layers=layers)
    ClearanceProcess.ensureClearanceLayer(map_)
    map_.setOrigin((0.35, -1.2, 0.05))
    gm = GpuNdtMap(map_, ndt_mode=NdtMode.kTraversability)
    rays = two_level_scene()
    n = rays.shape[0] // 2
    rng = np.random.default_rng(2)
    intensities = rng.uniform(0.0, 50.0, size=n).astype(np.float32)
    timestamps = np.linspace(10.0, 12.0, n)
    assert gm.integrateRays(rays, intensities, timestamps) == rays.shape[0]
    assert ClearanceProcess(0.5).update(gm) == MappingProcessResult.kMprUpToDate
    gm.syncVoxels()
    return map_, gm


def test_every_layer_of_an_ndt_tm_map(ndt_scene):
    map_, gm = ndt_scene
    assert set(map_.layers) == set(LAYERS) - {"tsdf"}
    keys = seeded_keys(map_, np.random.default_rng(1))
    present = check_layers(gm, map_, keys, map_.layers)
    assert 0 < present.sum() < len(keys)
    values, _ = gm.readVoxels(keys, "covariance")
    assert values.shape == (len(keys), 6) and np.count_nonzero(values) > 0
    values, _ = gm.readVoxels(keys, "clearance")
    assert (values >= 0).any() and (values[present == 0] == -1.0).all()
    values, _ = gm.readVoxels(keys, "occupancy")
    assert (values[present == 0] == INF).all()
    # a (regions, locals) pair and raw 10-byte records name the same voxels
    pair = gm.readVoxels((keys["region"], keys["voxel"][:, :3]), "mean")
    records = gm.readVoxels(keys.view(np.uint8).reshape(-1, 10), "mean")
    assert np.array_equal(pair[0], records[0]) and np.array_equal(pair[1], records[1])


def test_tsdf_map(gpu):
    map_ = OccupancyMap(0.1, layers=())
    gm = GpuTsdfMap(map_, default_truncation_distance=0.2)
    rays = two_level_scene()
    assert gm.integrateRays(rays) == rays.shape[0]
    keys = seeded_keys_after_sync(gm, map_)
    present = check_layers(gm, map_, keys, ["tsdf"])
    values, _ = gm.readVoxels(keys, "tsdf")
    assert values.shape == (len(keys), 2) and (values[present == 1][:, 0] > 0).any()
    with pytest.raises(OhmHipError) as err:
        gm.readVoxels(keys, "occupancy")  # a layer the map lacks
    assert err.value.status == L.ERR_UNSUPPORTED


def seeded_keys_after_sync(gm, map_):
    gm.syncVoxels()
    return seeded_keys(map_, np.random.default_rng(4))


def test_collected_batches_are_seen_and_empty_request(gpu):
    map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
    gm = GpuMap(map_)
    rays = two_level_scene()
    for part in np.array_split(rays.reshape(-1, 2, 3), 6):
        part = part.reshape(-1, 3)
        assert gm.integrateRays(part) == part.shape[0]
    keys = gm.voxelKeys(rays[1::2][::31])
    early = gm.readVoxels(keys, "occupancy"), gm.readVoxels(keys, "mean")
    gm.syncVoxels()
    for (values, present), name in zip(early, ("occupancy", "mean")):
        want_values, want_present = expected(map_, keys, name)
        assert np.array_equal(raw(values), raw(want_values)) and np.array_equal(present, want_present)
        assert present.all()
    assert (early[0][0] >= map_.occupancy_threshold_value).sum() > len(keys) // 2  # samples are mostly occupied
    values, present = gm.readVoxels(np.zeros(0, dtype=GPU_KEY_DTYPE), "mean")
    assert values.shape == (0, 2) and present.shape == (0,)
    assert gm.voxelKeys(np.zeros((0, 3))).shape == (0,)
    assert gm.occupancyTypes(np.zeros(0, dtype=GPU_KEY_DTYPE)).shape == (0,)


def test_tiled_region_with_an_empty_tile(gpu):
    """A region of 40 x 40 x 24 voxels is two tiles of 12 layers; rays that stay below z = 0 create only the lower one:
    the upper one reads the clear value and is present, for the region is."""
    map_ = OccupancyMap(0.1, (40, 40, 24), layers=("occupancy", "mean"))
    gm = GpuMap(map_)
    rng = np.random.default_rng(3)
    starts = rng.uniform((-1.8, -1.8, -1.0), (1.8, 1.8, -0.3), size=(400, 3))
    ends = rng.uniform((-1.8, -1.8, -1.0), (1.8, 1.8, -0.3), size=(400, 3))
    rays = np.stack([starts, ends], axis=1).reshape(-1, 3)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    assert sorted(map_.chunks) == [(0, 0, 0)] and gm.cacheStats()["regions_resident"] == 1
    locals_ = np.stack([rng.integers(0, 40, size=200), rng.integers(0, 40, size=200), rng.integers(0, 24, size=200)], axis=1)
    keys = np.concatenate([make_keys([(0, 0, 0)] * 200, locals_), make_keys([(0, 0, 1), (0, 1, 0)], [(1, 2, 3), (39, 39, 23)])])
    present = check_layers(gm, map_, keys, ["occupancy", "mean"])
    assert present[:200].all() and not present[200:].any()
    upper = keys["voxel"][:200, 2] >= 12
    values, _ = gm.readVoxels(keys, "occupancy")
    assert upper.any() and (values[:200][upper] == INF).all() and (values[:200][~upper] != INF).any()


def _observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


def test_spilled_regions_read_only(gpu):
    layers = ("occupancy", "mean")
    map_ = OccupancyMap(0.1, layers=layers)
    gm = GpuMap(map_, region_capacity=8)
    gm.setMemoryLimit(7 * gm.cacheStats()["bytes_per_region"])  # the scene holds 9 regions
    gm.setSpillToHost(True)
    ref_map = OccupancyMap(0.1, layers=layers)
    ref = GpuMap(ref_map)
    pairs = two_level_scene().reshape(-1, 2, 3)
    pairs = pairs[np.argsort(pairs[:, 1, 0], kind="stable")]
    for part in np.array_split(pairs, 8):
        part = part.reshape(-1, 3)
        for g in (gm, ref):
            assert g.integrateRays(part) == part.shape[0]
    assert gm.cacheStats()["regions_spilled"] > 0
    ref.syncVoxels()
    keys = seeded_keys(ref_map, np.random.default_rng(6), n=400)  # every region of the scene, spilled ones too
    assert len({tuple(r) for r in keys["region"].tolist()} & set(ref_map.chunks)) == len(ref_map.chunks) == 9
    before = _observe(gm)
    check_layers(gm, ref_map, keys, layers)
    assert _observe(gm) == before


def test_voxel_keys_equal_the_oracle(gpu):
    for dims, origin in (((32, 32, 32), (0.35, -1.2, 0.05)), ((5, 7, 3), (0.0, 0.0, 0.0))):
        map_ = OccupancyMap(0.1, dims)
        map_.setOrigin(origin)
        gm = GpuMap(map_)
        om = make_oracle(map_)
        rng = np.random.default_rng(12)
        points = [rng.uniform(-20.0, 20.0, size=(150, 3))]
        # within 1e-6 of voxel and region faces: the epsilon rules of pointToRegionVoxel decide
        for a in range(3):
            region_dim = dims[a] * 0.1
            for face in (-1.5 * region_dim, -0.5 * region_dim, 0.5 * region_dim, 0.5 * region_dim + 0.3, 0.1, -0.2):
                for delta in (-1e-6, -5e-7, -1e-9, 0.0, 1e-9, 5e-7, 1e-6):
                    p = rng.uniform(-1.0, 1.0, size=3)
                    p[a] = face + delta
                    points.append((p + np.asarray(origin))[None, :])
        # beyond the int16 range of region coordinates: Key::kNull
        points.append(np.array([(40000.0 * dims[0] * 0.1, 0.0, 0.0), (0.0, -40000.0 * dims[1] * 0.1, 0.0), (1.0, 2.0, 1e12),
                                (32767.4 * dims[0] * 0.1, 0.0, 0.0), (32768.6 * dims[0] * 0.1, 0.0, 0.0)]))
        points = np.concatenate(points)
        keys = gm.voxelKeys(points)
        want = np.zeros(len(points), dtype=GPU_KEY_DTYPE)
        nulls = 0
        for i, p in enumerate(points):
            k = om.voxel_key(p)
            if k is None:
                want[i] = NR.NULL_KEY[0]
                nulls += 1
            else:
                want[i]["region"] = k[0]
                want[i]["voxel"][:3] = k[1]
        assert nulls == 4  # (region 32767 is still a region)
        assert np.array_equal(raw(keys), raw(want)), dims


def test_occupancy_types(gpu):
    map_ = OccupancyMap(0.25, (8, 8, 8))
    threshold = np.float32(map_.occupancy_threshold_value)
    block = np.full(512, INF, dtype=np.float32)
    block[1:5] = [np.nan, np.nextafter(threshold, np.float32(-1)), threshold, 2.0]
    map_.chunks[(0, 0, 0)] = {"occupancy": block}
    gm = GpuMap(map_)
    gm.uploadRegions([(0, 0, 0)])
    keys = np.concatenate([make_keys([(0, 0, 0)] * 5, [(x, 0, 0) for x in range(5)]), make_keys([(3, 0, 0)], [(0, 0, 0)]),
                           null_key()])
    types = gm.occupancyTypes(keys)
    assert types.dtype == np.int8
    assert types.tolist() == [OccupancyType.kUnobserved, OccupancyType.kUnobserved, OccupancyType.kFree,
                              OccupancyType.kOccupied, OccupancyType.kOccupied, OccupancyType.kNull, OccupancyType.kNull]
    values, present = gm.readVoxels(keys, "occupancy")
    assert np.array_equal(types, NR.occupancy_types(values, present, threshold))


def test_device_variant_and_refusals(ndt_scene):
    map_, gm = ndt_scene
    keys = seeded_keys(map_, np.random.default_rng(9), n=100)
    n = len(keys)
    host_values, host_present = gm.readVoxels(keys, "covariance")
    handles = []
    try:
        ptrs = []
        for nbytes in (10 * n, 24 * n, n):
            handle, ptr = L._vp(), L._vp()
            L.check(L.lib.ohmhip_buffer_create(C.byref(handle), nbytes, 3), "buffer_create")
            handles.append(handle)
            L.check(L.lib.ohmhip_buffer_ptr(handle, C.byref(ptr)), "buffer_ptr")
            ptrs.append(ptr)
        L.check(L.lib.ohmhip_buffer_write(handles[0], keys.ctypes.data, 10 * n, 0, None, None, None), "write")
        L.check(L.lib.ohmhip_map_read_voxels_device(gm._handle, L.LID_COVARIANCE, ptrs[0], n, ptrs[1], ptrs[2]), "device")
        gm.wait()
        values = np.zeros((n, 6), dtype=np.float32)
        present = np.zeros(n, dtype=np.uint8)
        L.check(L.lib.ohmhip_buffer_read(handles[1], values.ctypes.data, values.nbytes, 0, None, None, None), "read")
        L.check(L.lib.ohmhip_buffer_read(handles[2], present.ctypes.data, present.nbytes, 0, None, None, None), "read")
        assert np.array_equal(raw(values), raw(host_values)) and np.array_equal(present, host_present)
    finally:
        for handle in handles:
            L.lib.ohmhip_buffer_destroy(handle)
    # refusals
    values = np.zeros((n, 6), dtype=np.float32)
    present = np.zeros(n, dtype=np.uint8)

    def call(layer, k=keys, count=n, v=values, p=present):
        return L.lib.ohmhip_map_read_voxels(gm._handle, layer, k.ctypes.data if k is not None else None, count,
                                            v.ctypes.data if v is not None else None,
                                            p.ctypes.data if p is not None else None)

    assert call(L.LID_COVARIANCE) == L.OK
    assert call(-1) == L.ERR_INVALID_ARG and call(L.LID_COUNT) == L.ERR_INVALID_ARG
    assert call(L.LID_TSDF) == L.ERR_UNSUPPORTED  # a layer the map lacks
    assert call(0, k=None) == L.ERR_INVALID_ARG and call(0, v=None) == L.ERR_INVALID_ARG
    assert call(0, p=None) == L.ERR_INVALID_ARG
    assert call(0, k=None, count=0, v=None, p=None) == L.OK
    outside = keys.copy()
    outside["voxel"][7, 1] = 32  # beyond the region's 32 voxels
    assert call(0, k=outside) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_voxel_keys(gm._handle, None, 3, outside.ctypes.data) == L.ERR_INVALID_ARG
    owner = GpuMap(OccupancyMap(0.1))
    owner.setRegionOwnership(2, 0)
    with pytest.raises(OhmHipError) as err:
        owner.readVoxels(keys, "occupancy")
    assert err.value.status == L.ERR_UNSUPPORTED
