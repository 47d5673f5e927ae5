"""-m gpu: the device NearestNeighbours query (ohmhip_map_nearest_neighbours / _device, GpuMap.nearestNeighbours,
ohm_amd.NearestNeighbours) against the CPU restatement (tests/neighbours_ref.py) at EXACT equality: counts, keys, the
bits of every range and the order, with np.array_equal on the raw bytes -- no tolerance, no excluded case.  Constructed
maps whose answers are known (the exact lattice of tests/test_neighbours_ref.py; run, wave and chunk edges; a non-cubic
region; a tiled region with an empty tile; an absent region in the box), a 0.1 m map with a shifted origin and seeded
points, maps integrated from rays (collected batches, spill to host), capacity and count, the device-array variant,
the pruned against the unpruned work list, the read-only guarantee and the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (CLOUD_CHUNK_VOXELS, GPU_KEY_DTYPE, GpuMap, GpuTsdfMap, NearestNeighbours, OccupancyMap, OhmHipError,
                     QueryFlag)
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbours_ref as NR  # noqa: E402
from heightmap_cases import two_level_scene  # noqa: E402

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
UAO, NEAREST = int(QueryFlag.kQfUnknownAsOccupied), int(QueryFlag.kQfNearestResult)
ALL_FLAGS = (0, UAO, NEAREST, UAO | NEAREST)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def blocks_of(map_):
    return {k: c["occupancy"] for k, c in map_.chunks.items()}


def reference(map_, points, radius, flags):
    return NR.nearest_neighbours(blocks_of(map_), map_.resolution, map_.region_voxel_dimensions, map_.origin,
                                 map_.occupancy_threshold_value, points, radius, flags)


def assert_same(got, want, what=""):
    assert got[0].dtype == np.uint64 and got[1].dtype == GPU_KEY_DTYPE and got[2].dtype == np.float32
    assert np.array_equal(got[0], want[0]), (what, "counts", got[0], want[0])
    assert np.array_equal(raw(got[1]), raw(want[1])), (what, "keys")
    assert np.array_equal(raw(got[2]), raw(want[2])), (what, "ranges")


def check(gm, map_, points, radius, flags, what="", some=True):
    want = reference(map_, points, radius, flags)
    if some:
        assert want[0].sum() > 0, (what, "the expectation is empty")
    got = gm.nearestNeighbours(points, radius, flags)
    assert_same(got, want, (what, flags))
    return got, want


def constructed(dims, blocks, origin=(0.0, 0.0, 0.0), resolution=0.1):
    """A device map holding exactly `blocks` ({region: occupancy block})."""
    map_ = OccupancyMap(resolution, dims, layers=("occupancy",))
    map_.setOrigin(origin)
    for key, block in blocks.items():
        map_.chunks[key] = {"occupancy": np.asarray(block, dtype=np.float32).copy()}
    gm = GpuMap(map_)
    gm.uploadRegions(sorted(blocks))
    return map_, gm


def lattice_block(occupied, value=1.0, fill=INF):
    b = np.full(512, fill, dtype=np.float32)
    for (x, y, z) in occupied:
        b[x + 8 * y + 64 * z] = np.float32(value)
    return b


def as_tuples(keys):
    return [(tuple(int(v) for v in k["region"]), tuple(int(v) for v in k["voxel"][:3])) for k in keys]


# -- the exact lattice: resolution 0.25, 8^3 regions ----------------------------------------------------------------------

def test_lattice_voxel_on_the_sphere(gpu):
    centre = (-0.375, -0.375, -0.375)
    for target, radius in (((5, 2, 2), 0.75), ((5, 6, 2), 1.25)):
        map_, gm = constructed((8, 8, 8), {(0, 0, 0): lattice_block([target])}, resolution=0.25)
        got, _ = check(gm, map_, [centre], radius, 0, "on the sphere")
        assert got[0].tolist() == [1] and as_tuples(got[1]) == [((0, 0, 0), target)] and got[2][0] == np.float32(radius)
        inside = float(np.nextafter(np.float32(radius), np.float32(0)))
        got, _ = check(gm, map_, [centre], inside, 0, "inside the sphere", some=False)
        assert got[0].tolist() == [0] and got[1].size == 0


def test_lattice_corner_of_eight_and_three_queries(gpu):
    blocks = {(0, 0, 0): lattice_block([(7, y, z) for y in (3, 4) for z in (3, 4)]),
              (1, 0, 0): lattice_block([(0, y, z) for y in (3, 4) for z in (3, 4)])}
    map_, gm = constructed((8, 8, 8), blocks, resolution=0.25)
    got, _ = check(gm, map_, [(1.0, 0.0, 0.0)], 0.25, 0, "corner")
    assert got[0].tolist() == [8] and as_tuples(got[1])[0] == ((0, 0, 0), (7, 3, 3))
    got, _ = check(gm, map_, [(1.0, 0.0, 0.0)], 0.25, NEAREST, "corner, nearest")
    assert got[0].tolist() == [1] and as_tuples(got[1]) == [((0, 0, 0), (7, 3, 3))]
    got, _ = check(gm, map_, [(1.0625, 0.0, 0.0)], 0.5, NEAREST, "a later voxel is strictly closer")
    assert as_tuples(got[1]) == [((1, 0, 0), (0, 3, 3))]
    # three queries in one call; the middle one has no result
    points = [(1.0, 0.0, 0.0), (1.0, 0.0, 0.75), (0.875, -0.125, -0.125)]
    for flags in (0, NEAREST):
        got, _ = check(gm, map_, points, 0.25, flags, "three queries")
        assert got[0][1] == 0 and got[0][0] > 0 and got[0][2] > 0
    # radius 0: only a voxel whose centre is the near point
    got, _ = check(gm, map_, [(0.875, -0.125, -0.125), (0.875, -0.125, -0.126)], 0.0, 0, "radius 0")
    assert got[0].tolist() == [1, 0] and got[2].tolist() == [0.0]


def test_lattice_obstruction_rule(gpu):
    centre = (-0.375, -0.375, -0.375)
    threshold = OccupancyMap(0.25).occupancy_threshold_value
    values = {"threshold": threshold, "below": np.nextafter(np.float32(threshold), np.float32(-1)), "nan": np.nan,
              "inf": np.inf}
    expect = {"threshold": (1, 1), "below": (0, 0), "nan": (0, 0), "inf": (0, 1)}
    for name, value in values.items():
        block = lattice_block([(3, 2, 2)], value=value, fill=np.float32(-1.0))
        map_, gm = constructed((8, 8, 8), {(0, 0, 0): block}, resolution=0.25)
        for flags, n in zip((0, UAO), expect[name]):
            got, _ = check(gm, map_, [centre], 0.3, flags, name, some=False)
            assert got[0].tolist() == [n], (name, flags)


# -- shapes ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seeded(gpu):
    """0.1 m, 32^3 regions, a shifted origin, regions with negative coordinates; one region of the cluster missing."""
    rng = np.random.default_rng(17)
    n = 32 ** 3
    blocks = {}
    for key in [(-1, -1, -1), (0, -1, -1), (-1, 0, -1), (0, 0, -1), (-1, -1, 0), (0, -1, 0), (0, 0, 0), (-2, 0, 0)]:
        block = rng.uniform(-2.0, 3.0, size=n).astype(np.float32)
        block[rng.random(n) < 0.4] = INF
        block[rng.random(n) < 0.01] = np.nan
        blocks[key] = block
    origin = (0.35, -1.2, 0.05)
    map_, gm = constructed((32, 32, 32), blocks, origin=origin)
    points = rng.uniform(-2.5, 1.5, size=(50, 3)) + np.asarray(origin)
    return map_, gm, points


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_seeded_points_inexact_floats(seeded, flags):
    map_, gm, points = seeded
    got, want = check(gm, map_, points, 0.45, flags, "seeded")
    assert (np.asarray(want[1]["region"]) < 0).any() and (want[0] > 0).sum() > 25
    if flags & UAO:
        assert (np.asarray(want[1]["region"]) == (-1, 0, 0)).all(axis=1).any()  # the missing region answers


def test_run_wave_and_chunk_edges(gpu):
    n = 32 ** 3
    edges = [63, 64, 1023, 1024, CLOUD_CHUNK_VOXELS - 1, CLOUD_CHUNK_VOXELS, 0, n - 1]
    block = np.full(n, np.float32(-1.0), dtype=np.float32)
    block[edges] = np.float32(2.0)
    map_, gm = constructed((32, 32, 32), {(0, 0, 0): block})
    got, _ = check(gm, map_, [(0.0, 0.0, 0.0)], 3.0, 0, "edges")  # the whole region lies within 2.8 m of its centre
    v = got[1]["voxel"].astype(np.int64)
    assert np.array_equal(v[:, 0] + 32 * v[:, 1] + 1024 * v[:, 2], sorted(edges))
    check(gm, map_, [(0.0, 0.0, 0.0)], 3.0, NEAREST, "edges, nearest")
    complement = np.full(n, np.float32(2.0), dtype=np.float32)
    complement[edges] = INF
    map_, gm = constructed((32, 32, 32), {(0, 0, 0): complement})
    got, _ = check(gm, map_, [(0.05, -0.05, 0.05), (1.6, 1.6, 1.6)], 1.0, 0, "complement")
    assert got[0][0] > 3000


def test_non_cubic_region(gpu):
    rng = np.random.default_rng(5)
    dims, n = (5, 7, 3), 105
    blocks = {}
    for k in [(0, 0, 0), (1, 0, 0), (-1, 2, 0), (0, -3, 1), (2, 2, -2), (-4, 0, 0), (1, 1, 1), (0, 1, 0), (0, 0, 1)]:
        block = np.full(n, INF, dtype=np.float32)
        mask = rng.random(n) < 0.5
        block[mask] = rng.uniform(-2.0, 3.0, size=int(mask.sum())).astype(np.float32)
        blocks[k] = block
    map_, gm = constructed(dims, blocks, origin=(-0.05, 0.4, 0.0))
    points = rng.uniform(-0.6, 0.9, size=(12, 3))
    for flags in ALL_FLAGS:
        check(gm, map_, points, 0.35, flags, "5x7x3")


def test_tiled_region_with_an_empty_tile(gpu):
    """A region of 40 x 40 x 24 voxels is two tiles of 12 layers; rays that stay below z = 0 create only the lower one."""
    map_ = OccupancyMap(0.1, (40, 40, 24), layers=("occupancy",))
    gm = GpuMap(map_)
    rng = np.random.default_rng(3)
    starts = rng.uniform((-1.8, -1.8, -1.0), (1.8, 1.8, -0.3), size=(400, 3))
    ends = rng.uniform((-1.8, -1.8, -1.0), (1.8, 1.8, -0.3), size=(400, 3))
    rays = np.stack([starts, ends], axis=1).reshape(-1, 3)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    assert sorted(map_.chunks) == [(0, 0, 0)] and gm.cacheStats()["regions_resident"] == 1  # one tile of two
    upper = map_.chunks[(0, 0, 0)]["occupancy"].reshape(24, 40, 40)[12:]
    assert (upper == INF).all()
    points = [(0.02, 0.03, -0.04), (1.0, -1.0, -0.6), (0.3, 0.3, 0.5)]
    got, _ = check(gm, map_, points, 0.35, 0, "tiled")
    assert got[0][2] == 0
    got, want = check(gm, map_, points, 0.35, UAO, "tiled, unknown as occupied")
    assert (want[1]["voxel"][:, 2] >= 12).any() and got[0][2] > 0
    check(gm, map_, points, 0.35, UAO | NEAREST, "tiled, nearest")


def test_absent_region_inside_the_box(gpu):
    n = 16 ** 3
    rng = np.random.default_rng(8)
    blocks = {}
    for key in [(0, 0, 0), (2, 0, 0)]:
        block = rng.uniform(-2.0, 3.0, size=n).astype(np.float32)
        block[rng.random(n) < 0.5] = INF
        blocks[key] = block
    map_, gm = constructed((16, 16, 16), blocks)
    point = [(2.4, 0.1, -0.1)]  # region (1, 0, 0) spans x in [0.8, 2.4)
    got, want = check(gm, map_, point, 1.7, 0, "absent region")
    regions = {tuple(r) for r in want[1]["region"].tolist()}
    assert regions == {(0, 0, 0), (2, 0, 0)}
    got, want = check(gm, map_, point, 1.7, UAO, "absent region, unknown as occupied")
    regions = {tuple(r) for r in want[1]["region"].tolist()}
    assert (1, 0, 0) in regions and len(regions) > 3
    check(gm, map_, point, 1.7, UAO | NEAREST, "absent region, nearest")


# -- maps integrated from rays ---------------------------------------------------------------------------------------------

def _observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


@pytest.fixture(scope="module")
def scene(gpu):
    """The two-level scene integrated in small batches; a query is asked while the batches are still collected."""
    map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
    map_.setOrigin((0.35, -1.2, 0.05))
    gm = GpuMap(map_)
    rays = two_level_scene()
    for part in np.array_split(rays.reshape(-1, 2, 3), 6):
        part = part.reshape(-1, 3)
        assert gm.integrateRays(part) == part.shape[0]
    points = rays[1::2][::173][:24].copy()
    first = gm.nearestNeighbours(points, 0.3, 0)
    gm.syncVoxels()
    return map_, gm, points, first


def test_collected_batches_are_seen(scene):
    map_, gm, points, first = scene
    want = reference(map_, points, 0.3, 0)
    assert want[0].sum() > 100
    assert_same(first, want, "collected")


def test_read_only_repeatable_capacity_and_count(scene):
    map_, gm, points, _ = scene
    before = _observe(gm)
    got, want = check(gm, map_, points, 0.3, UAO, "scene")
    again = gm.nearestNeighbours(points, 0.3, UAO)
    assert_same(again, got, "second call")
    total = int(want[0].sum())
    assert total > 1000
    # capacity below the total: the full counts and the prefix of the results
    short = gm.nearestNeighbours(points, 0.3, UAO, capacity=777)
    assert np.array_equal(short[0], want[0]) and len(short[1]) == 777
    assert np.array_equal(raw(short[1]), raw(want[1][:777])) and np.array_equal(raw(short[2]), raw(want[2][:777]))
    # a count-only call
    counted = gm.nearestNeighbours(points, 0.3, UAO, capacity=0)
    assert np.array_equal(counted[0], want[0]) and counted[1].size == 0
    # capacity above the total: nothing beyond the results is touched; null ranges are fine
    p = L.NeighboursParams(0.3, UAO)
    counts = np.zeros(len(points), dtype=np.uint64)
    keys = np.full((total + 5, 10), 0x5a, dtype=np.uint8)
    n = C.c_uint64(0)
    pts = np.ascontiguousarray(points, dtype=np.float64)
    L.check(L.lib.ohmhip_map_nearest_neighbours(gm._handle, pts.ctypes.data, len(points), C.byref(p), total + 5,
                                                counts.ctypes.data, keys.ctypes.data, None, C.byref(n)), "nn")
    assert n.value == total and np.array_equal(raw(keys[:total]), raw(want[1])) and (keys[total:] == 0x5a).all()
    assert _observe(gm) == before


def test_pruned_list_gives_identical_bytes(scene):
    map_, gm, points, _ = scene
    results = {}
    for prune in ("1", "0"):
        os.environ["OHMHIP_NN_PRUNE"] = prune
        try:
            results[prune] = [gm.nearestNeighbours(points, 0.45, flags) for flags in ALL_FLAGS]
        finally:
            del os.environ["OHMHIP_NN_PRUNE"]
    for one, two in zip(results["1"], results["0"]):
        assert one[0].sum() > 0
        assert_same(one, two, "pruned against unpruned")


def test_query_object(scene):
    map_, gm, points, _ = scene
    for flags in (0, NEAREST, UAO | NEAREST | int(QueryFlag.kQfGpuEvaluate)):
        query = NearestNeighbours(gm, points[3], 0.3, flags)
        assert query.execute()
        want = reference(map_, [points[3]], 0.3, flags & (UAO | NEAREST))
        assert query.numberOfResults() == int(want[0][0]) > 0
        assert np.array_equal(raw(query.intersectedVoxels()), raw(want[1]))
        assert query.ranges().dtype == np.float64 and np.array_equal(query.ranges(), want[2].astype(np.float64))
    query.setNearPoint((50.0, 50.0, 50.0))
    query.setQueryFlags(0)
    assert query.execute() and query.numberOfResults() == 0
    query.reset()
    assert query.ranges().size == 0


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


@pytest.mark.parametrize("flags,short", [(0, False), (0, True), (NEAREST, False), (UAO | NEAREST, True)])
def test_device_variant_equals_host_variant(scene, flags, short):
    map_, gm, points, _ = scene
    host = gm.nearestNeighbours(points, 0.3, flags)
    total = int(host[0].sum())
    assert total > 8
    capacity = total // 2 if short else total
    nq = len(points)
    bufs = [DeviceBuffer(8 * nq), DeviceBuffer(10 * capacity), DeviceBuffer(4 * capacity), DeviceBuffer(8)]
    try:
        p = L.NeighboursParams(0.3, flags)
        pts = np.ascontiguousarray(points, dtype=np.float64)
        L.check(L.lib.ohmhip_map_nearest_neighbours_device(gm._handle, pts.ctypes.data, nq, C.byref(p), capacity,
                                                           *[b.ptr for b in bufs]), "device")
        gm.wait()
        assert int(bufs[3].read(np.uint64, (1,))[0]) == total
        assert np.array_equal(bufs[0].read(np.uint64, (nq,)), host[0])
        assert np.array_equal(raw(bufs[1].read(GPU_KEY_DTYPE, (capacity,))), raw(host[1][:capacity]))
        assert np.array_equal(raw(bufs[2].read(np.float32, (capacity,))), raw(host[2][:capacity]))
    finally:
        for b in bufs:
            b.close()


def test_spill_to_host_read_only(gpu):
    """Regions in the host store answer from their pinned records: the same bytes as the reference of the fully resident
    map, and the call changes nothing of the map."""
    map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
    gm = GpuMap(map_, region_capacity=8)
    gm.setMemoryLimit(7 * gm.cacheStats()["bytes_per_region"])  # the scene holds 9 regions
    gm.setSpillToHost(True)
    ref_map = OccupancyMap(0.1, layers=("occupancy", "mean"))
    ref = GpuMap(ref_map)
    pairs = two_level_scene().reshape(-1, 2, 3)
    pairs = pairs[np.argsort(pairs[:, 1, 0], kind="stable")]  # by end point x: a part touches few regions
    for part in np.array_split(pairs, 8):
        part = part.reshape(-1, 3)
        for g in (gm, ref):
            assert g.integrateRays(part) == part.shape[0]
    assert gm.cacheStats()["regions_spilled"] > 0
    ref.syncVoxels()
    points = pairs[::211, 1][:24]
    before = _observe(gm)
    for flags in (0, UAO | NEAREST):
        want = reference(ref_map, points, 0.4, flags)
        assert want[0].sum() > 20
        assert_same(gm.nearestNeighbours(points, 0.4, flags), want, "spill")
    assert _observe(gm) == before


# -- refusals --------------------------------------------------------------------------------------------------------------

def _call(gm, points=((0.0, 0.0, 0.0),), radius=0.5, flags=0, capacity=0, keys=None, counts=True, total=True,
          params=True, nq=None, fn=None):
    fn = fn or L.lib.ohmhip_map_nearest_neighbours
    p = L.NeighboursParams(radius, flags)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3) if points is not None else None
    nq = (pts.shape[0] if pts is not None else 1) if nq is None else nq
    cnt = np.zeros(max(nq, 1), dtype=np.uint64)
    tot = C.c_uint64(99)
    status = fn(gm._handle, pts.ctypes.data if pts is not None else None, nq, C.byref(p) if params else None, capacity,
                cnt.ctypes.data if counts else None, keys, None, C.byref(tot) if total else None)
    return status, tot.value


def test_refusals_against_a_live_map(gpu):
    map_, gm = constructed((8, 8, 8), {(0, 0, 0): lattice_block([(3, 2, 2)])}, resolution=0.25)
    invalid = L.ERR_INVALID_ARG
    assert _call(gm)[0] == L.OK
    assert _call(gm, params=False)[0] == invalid
    assert _call(gm, points=None)[0] == invalid
    assert _call(gm, counts=False)[0] == invalid
    assert _call(gm, total=False)[0] == invalid
    assert _call(gm, points=[(0.0, np.nan, 0.0)])[0] == invalid
    assert _call(gm, points=[(0.0, 0.0, 0.0), (0.0, 0.0, -np.inf)])[0] == invalid
    for radius in (-0.5, np.inf, np.nan):
        assert _call(gm, radius=radius)[0] == invalid
    assert _call(gm, flags=4)[0] == invalid and _call(gm, flags=1 << 16)[0] == invalid
    assert _call(gm, capacity=3)[0] == invalid
    assert _call(gm, points=None, nq=0) == (L.OK, 0)  # no query: nothing to do
    # the work list of this call cannot stay under 2^24 entries
    assert _call(gm, radius=3.0e4, flags=UAO)[0] == L.ERR_CAPACITY  # (30 001^3 regions of 2 m)
    assert _call(gm, radius=3.0e4)[0] == L.OK  # (without the flag only the map's one region is listed)
    owner = GpuMap(OccupancyMap(0.1))
    owner.setRegionOwnership(2, 0)
    assert _call(owner)[0] == L.ERR_UNSUPPORTED
    with pytest.raises(OhmHipError) as err:
        owner.nearestNeighbours([(0.0, 0.0, 0.0)], 1.0)
    assert err.value.status == L.ERR_UNSUPPORTED
    tsdf = GpuTsdfMap(OccupancyMap(0.1, layers=()))
    assert _call(tsdf)[0] == L.ERR_UNSUPPORTED  # no occupancy layer


def test_empty_map(gpu):
    gm = GpuMap(OccupancyMap(0.1))
    counts, keys, ranges = gm.nearestNeighbours([(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)], 0.5)
    assert counts.tolist() == [0, 0] and keys.size == 0 and ranges.size == 0
    counts, keys, ranges = gm.nearestNeighbours([(0.05, 0.05, 0.05)], 0.1, UAO)
    want = NR.nearest_neighbours({}, 0.1, (32, 32, 32), (0.0, 0.0, 0.0), 0.0, [(0.05, 0.05, 0.05)], 0.1, UAO)
    assert_same((counts, keys, ranges), want, "empty map, unknown as occupied")
    assert counts[0] >= 1
