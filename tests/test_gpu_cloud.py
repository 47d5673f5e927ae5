"""-m gpu: the device point clouds (ohmhip_map_cloud / _count / _device, ohm_amd.extract_cloud) against the CPU
restatement (tests/cloud_ref.py) at EXACT equality: the count, and positions, keys and values with np.array_equal on
the raw bytes -- no tolerance, no excluded point.  Constructed maps whose matching set is known exactly (the edges of
waves, workgroups and chunks; offsets across regions; a scan of more partial counts than one workgroup scans; blocks of
no particular alignment; a region cut into tiles), a map integrated from rays in every mode, spill to host and the
read-only guarantee, capacity and count, the device-array variant, the refusal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (CLOUD_CHUNK_VOXELS, GPU_KEY_DTYPE, ClearanceProcess, CloudMode, GpuMap, GpuTsdfMap,
                     MappingProcessResult, OccupancyMap, OhmHipError, cloud_params, count_cloud, extract_cloud)
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as CR  # noqa: E402
from heightmap_cases import two_level_scene  # noqa: E402

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
WAVES_PER_CHUNK = 4  # one partial count per wave and chunk (ohm_amd/csrc/cloud_kernels.h)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def assert_same(got, want, what=""):
    assert got.count == want.count, (what, got.count, want.count)
    assert len(got) == want.count, what
    assert got.keys.dtype == GPU_KEY_DTYPE and got.positions.dtype == np.float64 and got.values.dtype == np.float32
    assert np.array_equal(raw(got.keys), raw(want.keys)), (what, "keys")
    assert np.array_equal(raw(got.values), raw(want.values)), (what, "values")
    assert np.array_equal(raw(got.positions), raw(want.positions)), (what, "positions")


def check(gm, map_, p, what="", chunks=None, all_pass=False):
    want = CR.extract_map(map_, p, chunks)
    # the expectation is not trivial: neither an empty result nor "everything" can pass
    if all_pass:
        assert want.count == want.considered > 0, what
    else:
        assert 0 < want.count < want.considered, (what, want.count, want.considered)
    got = extract_cloud(gm, **p.kwargs())
    assert_same(got, want, what)
    return got, want


def constructed(dims, chunks, layers=("occupancy",), origin=(0.0, 0.0, 0.0), resolution=0.1):
    """A device map holding exactly `chunks`."""
    map_ = OccupancyMap(resolution, dims, layers=layers)
    map_.setOrigin(origin)
    for key, c in chunks.items():
        map_.chunks[key] = {name: block.copy() for name, block in c.items()}
    gm = GpuMap(map_)
    gm.uploadRegions(sorted(chunks))
    return map_, gm


def occupancy_block(n, occupied, value=1.5):
    block = np.full(n, INF, dtype=np.float32)
    block[np.asarray(occupied, dtype=np.int64)] = np.float32(value)
    return block


# -- constructed maps ----------------------------------------------------------------------------------------------------

_EDGES = {
    "issue": [0, 63, 64, 255, 256, CLOUD_CHUNK_VOXELS - 1, CLOUD_CHUNK_VOXELS, 32767],
    # a wave's share of a chunk is a quarter of it; the last wave of the last chunk
    "waves": [CLOUD_CHUNK_VOXELS // 4 - 1, CLOUD_CHUNK_VOXELS // 4, CLOUD_CHUNK_VOXELS // 2 - 1,
              3 * CLOUD_CHUNK_VOXELS // 4, 32768 - CLOUD_CHUNK_VOXELS // 4 - 1, 32768 - CLOUD_CHUNK_VOXELS // 4, 32766],
}


@pytest.mark.parametrize("which", sorted(_EDGES))
@pytest.mark.parametrize("complement", [False, True])
def test_wave_workgroup_and_chunk_edges(gpu, which, complement):
    n = 32 ** 3
    assert 0 < CLOUD_CHUNK_VOXELS < n
    chosen = np.zeros(n, dtype=bool)
    chosen[_EDGES[which]] = True
    if complement:
        chosen = ~chosen
    map_, gm = constructed((32, 32, 32), {(0, 0, 0): {"occupancy": occupancy_block(n, np.nonzero(chosen)[0])}})
    got, want = check(gm, map_, CR.Params(), "edges")
    assert want.count == int(chosen.sum())
    v = got.keys["voxel"].astype(np.int64)
    assert np.array_equal(v[:, 0] + 32 * v[:, 1] + 1024 * v[:, 2], np.nonzero(chosen)[0])


def test_offsets_across_regions(gpu):
    n = 32 ** 3
    chunks = {(-2, 1, -1): {"occupancy": np.full(n, np.float32(0.25), dtype=np.float32)},
              (3, -4, 0): {"occupancy": np.full(n, INF, dtype=np.float32)},
              (-1, -1, 2): {"occupancy": occupancy_block(n, [12345])}}
    map_, gm = constructed((32, 32, 32), chunks, origin=(0.3, -0.2, 1.0))
    got, want = check(gm, map_, CR.Params(), "three regions")
    assert want.count == n + 1 and want.considered == 3 * n
    assert tuple(got.keys["region"][0]) == (-2, 1, -1) and tuple(got.keys["region"][-1]) == (-1, -1, 2)


def test_scan_longer_than_one_workgroup(gpu):
    rng = np.random.default_rng(11)
    cells = rng.permutation(41 ** 3)[:3200]
    keys = [(int(c % 41) - 20, int((c // 41) % 41) - 20, int(c // 1681) - 20) for c in cells]
    chunks = {}
    for k in keys:
        block = np.full(64, INF, dtype=np.float32)
        mask = rng.random(64) < 0.3
        block[mask] = rng.uniform(-2.0, 3.0, size=int(mask.sum())).astype(np.float32)
        chunks[k] = {"occupancy": block}
    map_, gm = constructed((4, 4, 4), chunks)
    assert len(chunks) >= 3000
    partials = len(chunks) * -(-64 // CLOUD_CHUNK_VOXELS) * WAVES_PER_CHUNK
    assert partials > 2048
    check(gm, map_, CR.Params(), "many regions")
    check(gm, map_, CR.Params(export_free=True), "many regions, free")


def test_unaligned_blocks(gpu):
    """Regions of 105 voxels: a pool slot's block starts on no particular boundary."""
    rng = np.random.default_rng(5)
    dims, n = (5, 7, 3), 105
    chunks = {}
    for k in [(0, 0, 0), (1, 0, 0), (-1, 2, 0), (0, -3, 1), (2, 2, -2), (-4, 0, 0), (1, 1, 1)]:
        block = np.full(n, INF, dtype=np.float32)
        mask = rng.random(n) < 0.5
        block[mask] = rng.uniform(-2.0, 3.0, size=int(mask.sum())).astype(np.float32)
        mean = np.zeros((n, 2), dtype=np.uint32)
        mean[:, 0] = rng.integers(0, 1 << 30, size=n, dtype=np.uint32) | np.uint32(1 << 31)
        mean[:, 1] = rng.integers(1, 100, size=n, dtype=np.uint32)
        chunks[k] = {"occupancy": block, "mean": mean.reshape(-1)}
    map_, gm = constructed(dims, chunks, layers=("occupancy", "mean"), origin=(-0.05, 0.4, 0.0))
    check(gm, map_, CR.Params(), "5x7x3")
    check(gm, map_, CR.Params(export_free=True, ignore_voxel_mean=True), "5x7x3 free")


def test_tiled_region(gpu):
    """A region of 64 000 voxels is cut into tiles: the order is the region's voxel index across them."""
    rng = np.random.default_rng(9)
    n = 40 ** 3
    chunks = {}
    for k in [(0, 0, 0), (-1, 0, 1)]:
        block = np.full(n, INF, dtype=np.float32)
        mask = rng.random(n) < 0.1
        block[mask] = rng.uniform(-2.0, 3.0, size=int(mask.sum())).astype(np.float32)
        chunks[k] = {"occupancy": block}
    map_, gm = constructed((40, 40, 40), chunks)
    got, want = check(gm, map_, CR.Params(export_free=True), "tiled")
    v = got.keys["voxel"].astype(np.int64)
    index = v[:, 0] + 40 * v[:, 1] + 1600 * v[:, 2]
    first = int((got.keys["region"] == (-1, 0, 1)).all(axis=1).argmax())  # (rz, ry, rx): (0, 0, 0) comes first
    assert 0 < first < len(got) and (np.diff(index[:first]) > 0).all() and (np.diff(index[first:]) > 0).all()
    assert index.max() > 32768


# -- a map integrated from rays -------------------------------------------------------------------------------------------

_SCENES = {}


def scene(layers=("occupancy", "mean"), origin=(0.0, 0.0, 0.0), dims=(32, 32, 32), cls=GpuMap, **kw):
    """A device map of the two-level scene, integrated in small batches; the cloud `first` (default parameters of
    `first_params`) is asked for while the batches are still collected, the host chunks are synced after it."""
    key = (layers, origin, dims, cls)
    if key not in _SCENES:
        map_ = OccupancyMap(0.1, dims, layers=layers)
        map_.setOrigin(origin)
        gm = cls(map_, **kw)
        rays = two_level_scene()
        for part in np.array_split(rays.reshape(-1, 2, 3), 6):
            part = part.reshape(-1, 3)
            assert gm.integrateRays(part) == part.shape[0]
        first_params = CR.Params(mode=CR.TSDF, surface_distance=0.05) if cls is GpuTsdfMap else CR.Params()
        first = extract_cloud(gm, **first_params.kwargs())
        gm.syncVoxels()
        _SCENES[key] = (map_, gm, first, first_params)
    return _SCENES[key]


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (0.35, -1.2, 0.05)])
def test_rays_collected_batches_are_seen(gpu, origin):
    map_, gm, first, first_params = scene(origin=origin)
    want = CR.extract_map(map_, first_params)
    assert 0 < want.count < want.considered
    assert_same(first, want, "collected")
    assert (np.asarray(want.keys["region"]) < 0).any()


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (0.35, -1.2, 0.05)])
@pytest.mark.parametrize("export_free,ignore_mean", [(False, False), (True, False), (False, True), (True, True)])
def test_rays_occupancy(gpu, origin, export_free, ignore_mean):
    map_, gm, _, _ = scene(origin=origin)
    got, want = check(gm, map_, CR.Params(export_free=export_free, ignore_voxel_mean=ignore_mean), "rays")
    if export_free:
        assert (want.values < map_.occupancy_threshold_value).any()


def test_rays_extents(gpu):
    map_, gm, _, _ = scene()
    p = CR.Params(export_free=True, extents=((-1.0, -1.0, -0.5), (2.0, 1.0, 0.5)))
    got, want = check(gm, map_, p, "extents")
    assert want.considered < 32 ** 3 * len(map_.chunks)


def test_rays_occupancy_without_mean_layer(gpu):
    map_, gm, _, _ = scene(layers=("occupancy",))
    check(gm, map_, CR.Params(export_free=True), "no mean layer")


def test_rays_tiled_regions(gpu):
    """Regions of 40^3 voxels: tiles no ray has reached are not created and read as a cleared chunk does."""
    layers = ("occupancy", "mean", "traversal")
    map_, gm, first, first_params = scene(layers=layers, dims=(40, 40, 40))
    assert_same(first, CR.extract_map(map_, first_params), "tiled, collected")
    check(gm, map_, CR.Params(export_free=True), "tiled rays")
    check(gm, map_, CR.Params(mode=CR.DENSITY), "tiled density", all_pass=True)


def test_density(gpu):
    layers = ("occupancy", "mean", "traversal")
    map_, gm, _, _ = scene(layers=layers)
    got, want = check(gm, map_, CR.Params(mode=CR.DENSITY), "density 0", all_pass=True)
    finite = want.values[np.isfinite(want.values) & (want.values > 0)]
    assert finite.size > 100
    threshold = float(np.median(finite))
    split, _ = check(gm, map_, CR.Params(mode=CR.DENSITY, density_threshold=threshold), "density split")
    assert (split.values >= np.float32(threshold)).all()
    check(gm, map_, CR.Params(mode=CR.DENSITY, density_threshold=threshold, ignore_voxel_mean=True), "density centre")
    # a map without the traversal layer: nothing, and no error
    plain_map, plain, _, _ = scene()
    assert extract_cloud(plain, mode=CloudMode.DENSITY).count == 0
    assert CR.extract_map(plain_map, CR.Params(mode=CR.DENSITY)).count == 0


def test_tsdf(gpu):
    map_, gm, first, first_params = scene(layers=(), origin=(0.35, -1.2, 0.05), cls=GpuTsdfMap,
                                          default_truncation_distance=0.2)
    want = CR.extract_map(map_, first_params)
    assert 0 < want.count < want.considered and (want.values < 0).any() and (want.values > 0).any()
    assert_same(first, want, "tsdf, collected")
    check(gm, map_, CR.Params(mode=CR.TSDF, surface_distance=0.11), "tsdf")
    assert extract_cloud(gm, mode=CloudMode.OCCUPANCY).count == 0  # no occupancy layer


@pytest.fixture(scope="module")
def clearance_scene(gpu):
    map_ = OccupancyMap(0.1, layers=("occupancy",))
    ClearanceProcess.ensureClearanceLayer(map_)
    map_.setOrigin((0.35, -1.2, 0.05))
    gm = GpuMap(map_)
    rays = two_level_scene()
    assert gm.integrateRays(rays) == rays.shape[0]
    assert ClearanceProcess(0.5).update(gm) == MappingProcessResult.kMprUpToDate
    gm.syncVoxels()
    return map_, gm


@pytest.mark.parametrize("export_type", [-1, 0, 1])
@pytest.mark.parametrize("extents", [None, ((-1.0, -1.0, -0.5), (2.0, 1.0, 0.5))])
def test_clearance(clearance_scene, export_type, extents):
    map_, gm = clearance_scene
    assert (map_.chunks[(0, 0, 0)]["clearance"] >= 0).any()
    # colour_range < 0: voxels without an obstacle in range are dropped, so no export type takes everything
    got, want = check(gm, map_, CR.Params(mode=CR.CLEARANCE, colour_range=-1.0, export_type=export_type,
                                          extents=extents), "clearance")
    assert (want.values >= 0).all()
    replaced, _ = check(gm, map_, CR.Params(mode=CR.CLEARANCE, colour_range=2.5, export_type=export_type,
                                            extents=extents), "clearance, replaced", all_pass=export_type == -1)
    if export_type == -1:
        assert (replaced.values == np.float32(2.5)).any()  # voxels with no obstacle in range


# -- the map as it is used ------------------------------------------------------------------------------------------------

def _observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


def test_spill_to_host_read_only(gpu):
    """Regions in the host store answer from their pinned records: the same bytes as the fully resident map, and the
    call changes nothing of the map."""
    layers = ("occupancy", "mean")
    map_ = OccupancyMap(0.1, layers=layers)
    gm = GpuMap(map_, region_capacity=8)
    gm.setMemoryLimit(7 * gm.cacheStats()["bytes_per_region"])  # the scene holds 9 regions
    gm.setSpillToHost(True)
    ref_map = OccupancyMap(0.1, layers=layers)
    ref = GpuMap(ref_map)
    pairs = two_level_scene().reshape(-1, 2, 3)
    pairs = pairs[np.argsort(pairs[:, 1, 0], kind="stable")]  # by end point x: a part touches few regions
    for part in np.array_split(pairs, 8):
        part = part.reshape(-1, 3)
        for g in (gm, ref):
            assert g.integrateRays(part) == part.shape[0]
    assert gm.cacheStats()["regions_spilled"] > 0
    before = _observe(gm)
    p = CR.Params(export_free=True)
    got = extract_cloud(gm, **p.kwargs())
    assert count_cloud(gm, **p.kwargs()) == got.count
    assert _observe(gm) == before
    full = extract_cloud(ref, **p.kwargs())
    assert_same(got, full, "spill against resident")
    ref.syncVoxels()
    want = CR.extract_map(ref_map, p)
    assert 0 < want.count < want.considered
    assert_same(got, want, "spill")


def test_capacity_and_count(gpu):
    map_, gm, _, _ = scene()
    p = CR.Params(export_free=True)
    want = CR.extract_map(map_, p)
    assert want.count > 1000
    assert count_cloud(gm, **p.kwargs()) == want.count
    # capacity < count: exactly the prefix, and the full count
    short = extract_cloud(gm, capacity=777, **p.kwargs())
    assert short.count == want.count and len(short) == 777
    assert np.array_equal(raw(short.positions), raw(want.positions[:777]))
    assert np.array_equal(raw(short.keys), raw(want.keys[:777]))
    assert np.array_equal(raw(short.values), raw(want.values[:777]))
    # capacity > count: nothing beyond the points is touched
    cp = cloud_params(**p.kwargs())
    n = C.c_uint64(0)
    positions = np.full((want.count + 5, 3), -7.0)
    values = np.full(want.count + 5, -7.0, dtype=np.float32)
    L.check(L.lib.ohmhip_map_cloud(gm._handle, C.byref(cp), want.count + 5, positions.ctypes.data, None,
                                   values.ctypes.data, C.byref(n)), "cloud")
    assert n.value == want.count
    assert np.array_equal(raw(positions[:want.count]), raw(want.positions)) and (positions[want.count:] == -7.0).all()
    assert np.array_equal(raw(values[:want.count]), raw(want.values)) and (values[want.count:] == -7.0).all()
    # the count-only call of ohmhip_map_cloud
    n = C.c_uint64(0)
    L.check(L.lib.ohmhip_map_cloud(gm._handle, C.byref(cp), 0, None, None, None, C.byref(n)), "count only")
    assert n.value == want.count
    # two calls: identical bytes
    one, two = extract_cloud(gm, **p.kwargs()), extract_cloud(gm, **p.kwargs())
    assert_same(one, want, "first call")
    assert_same(two, want, "second call")


def test_empty_map_and_further_batch(gpu):
    map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
    gm = GpuMap(map_)
    assert count_cloud(gm) == 0
    empty = extract_cloud(gm)
    assert empty.count == 0 and empty.positions.shape == (0, 3)
    rays = two_level_scene()
    half = rays.shape[0] // 4 * 2
    assert gm.integrateRays(rays[:half]) == half
    p = CR.Params()
    before = extract_cloud(gm, **p.kwargs())
    gm.syncVoxels()
    assert_same(before, CR.extract_map(map_, p), "first half")
    assert gm.integrateRays(rays[half:]) == rays.shape[0] - half
    after = extract_cloud(gm, **p.kwargs())
    gm.syncVoxels()
    want = CR.extract_map(map_, p)
    assert want.count != before.count and 0 < want.count < want.considered
    assert_same(after, want, "both halves")


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


@pytest.mark.parametrize("short", [False, True])
def test_device_variant_equals_host_variant(gpu, short):
    map_, gm, _, _ = scene()
    p = CR.Params(export_free=True)
    host = extract_cloud(gm, **p.kwargs())
    assert host.count > 1000
    capacity = 500 if short else host.count
    bufs = [DeviceBuffer(24 * capacity), DeviceBuffer(10 * capacity), DeviceBuffer(4 * capacity), DeviceBuffer(8)]
    try:
        cp = cloud_params(**p.kwargs())
        L.check(L.lib.ohmhip_map_cloud_device(gm._handle, C.byref(cp), capacity, *[b.ptr for b in bufs]), "device")
        gm.wait()
        assert int(bufs[3].read(np.uint64, (1,))[0]) == host.count
        assert np.array_equal(raw(bufs[0].read(np.float64, (capacity, 3))), raw(host.positions[:capacity]))
        assert np.array_equal(raw(bufs[1].read(GPU_KEY_DTYPE, (capacity,))), raw(host.keys[:capacity]))
        assert np.array_equal(raw(bufs[2].read(np.float32, (capacity,))), raw(host.values[:capacity]))
    finally:
        for b in bufs:
            b.close()


def test_refusal_for_region_ownership(gpu):
    owner = GpuMap(OccupancyMap(0.1))
    owner.setRegionOwnership(2, 0)
    with pytest.raises(OhmHipError) as err:
        extract_cloud(owner)
    assert err.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(OhmHipError) as err:
        count_cloud(owner)
    assert err.value.status == L.ERR_UNSUPPORTED
