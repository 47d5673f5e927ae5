"""-m gpu: the read-side features on a TILED map whose tiles live in BOTH places, the pool and the host store.  Every
feature is tested on a tiled map and, separately, on a map with regions in the host store; the host code that finds a
tile's data (ohm_amd/csrc/read_side.h: tileHome) serves both, so the combination is its seam.

Regions of 40 x 40 x 24 voxels are two tiles of 12 layers.  Nine regions (3 x 3 in x and y) are integrated in two
batches, first the lower tile of all nine, then the upper tile of eight: region (1, 1, 0) keeps an absent tile.  The
results are recorded with all 17 tiles resident.  Then the pool, which holds exactly those 17, is limited to 11, spill to
host is enabled, and a small batch ten regions away evicts tiles.  The far region lies outside every extent and radius
asked for, so the answers must be the recorded ones, byte for byte, and the Python models' (cloud_ref, neighbours_ref,
point_filter_ref) evaluated on the nine regions as synced before the eviction.

The Python surface counts resident and spilled tiles but does not say which tile is where: eviction order decides.  The
lower tiles were used one batch earlier than the upper ones, so a least-recently-used eviction of fewer than nine tiles
leaves regions with one tile in each place; the test asserts the counts (both kinds present, fewer spilled than there
are lower tiles) and no more."""
import os
import sys

import numpy as np
import pytest

from ohm_amd import GPU_KEY_DTYPE, GpuMap, OccupancyMap, QueryFlag, count_cloud, extract_cloud

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as CR  # noqa: E402
import neighbours_ref as NR  # noqa: E402
import point_filter_ref as PF  # noqa: E402

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)
UAO, NEAREST = int(QueryFlag.kQfUnknownAsOccupied), int(QueryFlag.kQfNearestResult)
DIMS = (40, 40, 24)
REGIONS = [(rx, ry, 0) for ry in (-1, 0, 1) for rx in (-1, 0, 1)]
LOWER_ONLY = (1, 1, 0)
TILES = 2 * len(REGIONS) - 1
LIMIT_TILES = 11  # about two thirds of the 17
NN_RADIUS = 0.35
NN_FLAGS = (0, UAO, NEAREST)
#: the nine regions and nothing else: x, y in [-6, 6), z in [-1.2, 1.2); the far batch is at x = 40
CLOUD = CR.Params(export_free=True, extents=((-5.9, -5.9, -1.1), (5.9, 5.9, 1.1)))


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def rays_in(rng, region, z_lo, z_hi, n):
    """n rays that stay inside `region` (4 m x 4 m x 2.4 m around its centre) between heights z_lo and z_hi."""
    cx, cy = 4.0 * region[0], 4.0 * region[1]
    lo, hi = (cx - 1.7, cy - 1.7, z_lo), (cx + 1.7, cy + 1.7, z_hi)
    return np.stack([rng.uniform(lo, hi, size=(n, 3)), rng.uniform(lo, hi, size=(n, 3))], axis=1).reshape(-1, 3)


def observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


def ask(gm, points, keys):
    """Every read the test makes, in one record."""
    cloud = extract_cloud(gm, **CLOUD.kwargs())
    return {"cloud_count": count_cloud(gm, **CLOUD.kwargs()), "cloud": cloud,
            "nn": {flags: gm.nearestNeighbours(points, NN_RADIUS, flags) for flags in NN_FLAGS},
            "voxels": gm.readVoxels(keys, "occupancy"),
            "filter": gm.filterPoints(points, occupancy_only=True)}


@pytest.fixture(scope="module")
def mixed(gpu):
    rng = np.random.default_rng(29)
    map_ = OccupancyMap(0.1, DIMS, layers=("occupancy",))
    gm = GpuMap(map_, region_capacity=TILES)
    lower = np.concatenate([rays_in(rng, r, -1.0, -0.15, 60) for r in REGIONS])
    upper = np.concatenate([rays_in(rng, r, 0.15, 1.0, 60) for r in REGIONS if r != LOWER_ONLY])
    assert gm.integrateRays(lower) == lower.shape[0]
    gm.syncVoxels()
    assert gm.cacheStats()["regions_resident"] == len(REGIONS)  # the lower tiles alone
    assert gm.integrateRays(upper) == upper.shape[0]
    gm.syncVoxels()
    assert sorted(map_.chunks) == sorted(REGIONS) and gm.cacheStats()["regions_resident"] == TILES
    chunks = {r: {"occupancy": map_.chunks[r]["occupancy"].copy()} for r in REGIONS}

    # sample ends in both tiles, a point in the absent tile and one in an absent region above it
    points = np.concatenate([lower[1::2][::23], upper[1::2][::23], [(4.3, 3.6, 0.5), (4.3, 3.6, 2.0)]])
    keys = gm.voxelKeys(points)
    resident = ask(gm, points, keys)

    gm.setMemoryLimit(LIMIT_TILES * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    far = rays_in(rng, (10, 0, 0), -1.0, 1.0, 40)
    assert gm.integrateRays(far) == far.shape[0]
    gm.wait()
    before = observe(gm)
    spilled = ask(gm, points, keys)
    return {"map": map_, "gm": gm, "chunks": chunks, "points": points, "keys": keys, "resident": resident,
            "spilled": spilled, "before": before, "after": observe(gm)}


def test_tiles_live_in_both_places_and_reads_move_none(mixed):
    stats = mixed["before"][2]
    assert stats["regions_resident"] > 0 and 0 < stats["regions_spilled"] < len(REGIONS)
    assert stats["regions_resident"] + stats["regions_spilled"] == TILES + 2
    assert stats["regions_resident"] <= LIMIT_TILES
    assert (10, 0, 0) in mixed["before"][0] and len(mixed["before"][0]) == len(REGIONS) + 1
    assert mixed["after"] == mixed["before"]


def test_cloud(mixed):
    want = CR.extract_map(mixed["map"], CLOUD, mixed["chunks"])
    assert 0 < want.count < want.considered == len(REGIONS) * 40 * 40 * 24
    assert (want.keys["voxel"][:, 2] >= 12).any() and (want.keys["voxel"][:, 2] < 12).any()
    for state in ("resident", "spilled"):
        got = mixed[state]["cloud"]
        assert mixed[state]["cloud_count"] == want.count == got.count == len(got), state
        assert got.keys.dtype == GPU_KEY_DTYPE
        assert np.array_equal(raw(got.keys), raw(want.keys)), state
        assert np.array_equal(raw(got.values), raw(want.values)), state
        assert np.array_equal(raw(got.positions), raw(want.positions)), state


@pytest.mark.parametrize("flags", NN_FLAGS)
def test_nearest_neighbours(mixed, flags):
    map_ = mixed["map"]
    blocks = {r: c["occupancy"] for r, c in mixed["chunks"].items()}
    want = NR.nearest_neighbours(blocks, map_.resolution, map_.region_voxel_dimensions, map_.origin,
                                 map_.occupancy_threshold_value, mixed["points"], NN_RADIUS, flags)
    assert want[0].sum() > 20
    if flags & UAO:
        absent = (np.asarray(want[1]["region"]) == LOWER_ONLY).all(axis=1) & (want[1]["voxel"][:, 2] >= 12)
        assert absent.any()  # the absent tile answers as unknown space
    for state in ("resident", "spilled"):
        got = mixed[state]["nn"][flags]
        assert np.array_equal(got[0], want[0]), (state, "counts")
        assert np.array_equal(raw(got[1]), raw(want[1])), (state, "keys")
        assert np.array_equal(raw(got[2]), raw(want[2])), (state, "ranges")


def test_read_voxels(mixed):
    keys, chunks = mixed["keys"], mixed["chunks"]
    want_values = np.full(len(keys), INF, dtype=np.float32)
    want_present = np.zeros(len(keys), dtype=np.uint8)
    for i, k in enumerate(keys):
        region, v = tuple(int(c) for c in k["region"]), k["voxel"].astype(np.int64)
        if region in chunks:
            want_values[i] = chunks[region]["occupancy"][v[0] + 40 * v[1] + 1600 * v[2]]
            want_present[i] = 1
    in_absent_tile = (np.asarray(keys["region"]) == LOWER_ONLY).all(axis=1) & (keys["voxel"][:, 2] >= 12)
    assert in_absent_tile.sum() == 1 and want_present[in_absent_tile][0] == 1 and want_values[in_absent_tile][0] == INF
    assert want_present[-1] == 0 and want_present[:-1].all()
    held = want_values != INF
    assert (held & (keys["voxel"][:, 2] < 12)).any() and (held & (keys["voxel"][:, 2] >= 12)).any()
    for state in ("resident", "spilled"):
        values, present = mixed[state]["voxels"]
        assert values.dtype == np.float32 and np.array_equal(raw(values), raw(want_values)), state
        assert np.array_equal(present, want_present), state


def test_filter_points(mixed):
    map_, points, keys = mixed["map"], mixed["points"], mixed["keys"]
    want_status, _ = PF.filter_points(points, keys, mixed["chunks"], map_.resolution, map_.region_voxel_dimensions,
                                      map_.origin, map_.occupancy_threshold_value, -1.0, True, map_.layers)
    assert (want_status == 1).sum() > 10 and (want_status == 0).any()
    for state in ("resident", "spilled"):
        status, kept, values, got_keys = mixed[state]["filter"]
        assert np.array_equal(status, want_status), state
        assert np.array_equal(kept, np.nonzero(status == 1)[0]), state
        assert np.array_equal(raw(got_keys), raw(keys)), state
        assert (values.view(np.uint64) == 0x7ff8000000000000).all(), state
