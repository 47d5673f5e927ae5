"""-m gpu: the three routes that write voxels into the resident pool from outside the ray pipeline leave the same map
(DESIGN.md 5c): (a) region uploads (GpuMap.uploadRegions: ohmhip_map_write_regions), (b) copyMap from a map filled by
(a), (c) writeVoxels of every voxel of every region, one call per layer.

Three fresh maps of one configuration receive the planted scenes of tests/copy_cases.py by one route each.  Their
blocks must be equal word for word, the dirty-region lists of (b) and (c) must name the same regions (an upload leaves
no dirty mark; the two lists are compared sorted: slots are handed out in each route's own order), and after the
follow-up batch the three maps must be equal again -- which is where a replay mask derived by another rule on one of
the routes shows -- and meet the bar of tests/test_gpu_copy.py for the mode: bit-exact against the oracle for TSDF; for
NDT planted voxels of both classes change in occupancy, the same number per class as in the oracle's map (a mask of all
ones or all zeros on all three routes alike fails one of these).  Shapes: `odd` (5 x 3 x 7: a partial last mask word,
blocks 16-byte aligned in every other slot only) and `tiled` (40 x 40 x 24: two tiles per region).

The clearance case does the same for the marks the incremental clearance update goes by."""
import functools

import numpy as np
import pytest

import copy_cases as cases
from ohm_amd import LAYERS, OccupancyMap, copyMap
from test_gpu_copy import integrate, keys_of, make, read_all

pytestmark = pytest.mark.gpu

SHAPES = ("odd", "tiled")


@functools.lru_cache(maxsize=None)
def planted(kind, shape):
    """The oracle's scene, built once per (kind, shape) and never changed."""
    if kind == "tsdf":
        return cases.planted_tsdf(shape)
    return cases.planted_ndt(shape, float(OccupancyMap().missProbability()))


def by_upload(gm, chunks):
    """(a): the chunks become the host map's, GpuMap.uploadRegions pushes them."""
    gm.map().chunks.update({k: {name: np.array(block) for name, block in c.items()} for k, c in chunks.items()})
    assert gm.uploadRegions(sorted(chunks)) == len(chunks)


def by_voxel_writes(gm, chunks, layers):
    """(c): every voxel of every region by key, one writeVoxels per layer."""
    dim = gm.map().region_voxel_dimensions
    z, y, x = np.meshgrid(np.arange(dim[2]), np.arange(dim[1]), np.arange(dim[0]), indexing="ij")
    local = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)  # block order: x fastest
    keys = sorted(chunks)
    regions = np.repeat(np.asarray(keys, dtype=np.int16), len(local), axis=0)
    locals_ = np.tile(local, (len(keys), 1))
    for name in layers:
        comps = LAYERS[name][2]
        values = np.concatenate([np.asarray(chunks[k][name]).reshape(len(local), comps) for k in keys])
        assert gm.writeVoxels((regions, locals_), name, values) == len(regions)
        assert gm.lastEditStats()["distinct_voxels"] == len(regions)


def assert_same_words(maps, layers=None):
    """Every map's blocks equal the first one's, as uint32 views; returns the first map's blocks."""
    first = read_all(maps[0], layers)
    for gm in maps[1:]:
        other = read_all(gm, layers)
        assert sorted(other) == sorted(first)
        for k in first:
            for name in first[k]:
                assert np.array_equal(first[k][name].view(np.uint32), other[k][name].view(np.uint32)), (k, name)
    return first


def deliver(kind, p, **kwargs):
    """The maps of (a), (b) and (c), holding p.chunks."""
    a, b, c, source = (make(kind, p.shape, layers=p.layers, **kwargs) for _ in range(4))
    by_upload(a, p.chunks)
    by_upload(source, p.chunks)
    assert copyMap(b, source)
    by_voxel_writes(c, p.chunks, p.layers)
    maps = [a, b, c]
    held = assert_same_words(maps)
    for k in p.chunks:
        for name in p.layers:
            assert np.array_equal(held[k][name].view(np.uint32), np.asarray(p.chunks[k][name]).view(np.uint32)), (k, name)
    assert keys_of(a, dirty_only=True) == []
    assert sorted(keys_of(b, dirty_only=True)) == sorted(keys_of(c, dirty_only=True)) == sorted(p.chunks)
    return maps


@pytest.mark.parametrize("shape", SHAPES)
def test_tsdf_three_deliveries_replay_alike(gpu, shape):
    p = planted("tsdf", shape)
    maps = deliver("tsdf", p, default_truncation_distance=p.options["dst_trunc"])
    for gm in maps:
        integrate(gm, p.rays)
    got = assert_same_words(maps)
    changed = p.changed(got, "tsdf")
    print("tsdf", shape, "changed", changed)
    assert all(changed[name] >= 1 for name in cases.TSDF_CLASSES), changed
    assert changed == p.changed(p.after, "tsdf")
    assert sorted(got) == sorted(p.after)
    for k in got:
        assert np.array_equal(got[k]["tsdf"].view(np.uint32), np.asarray(p.after[k]["tsdf"]).view(np.uint32)), k


@pytest.mark.parametrize("shape", SHAPES)
def test_ndt_three_deliveries_replay_alike(gpu, shape):
    p = planted("ndt", shape)
    maps = deliver("ndt", p)
    for name, value in p.options.items():
        assert getattr(maps[0], {"reinit_count": "reinitialise_covariance_point_count"}.get(name, name)) == value, name
    for gm in maps:
        integrate(gm, p.rays)
    got = assert_same_words(maps)
    changed = p.changed(got, "occupancy")
    print("ndt", shape, "changed", changed, "oracle", p.changed(p.after, "occupancy"))
    assert all(changed[name] >= 1 for name in cases.NDT_CLASSES), changed
    assert changed == p.changed(p.after, "occupancy")


def test_clearance_marks_of_three_deliveries(gpu):
    """Occupancy delivered into maps whose clearance layer is up to date: the incremental update finds the same regions
    stale, and leaves the same layer, whichever route delivered."""
    shape, radius = "odd", 0.25
    layers = ("occupancy", "clearance")
    filled = make("occ", shape, layers=("occupancy",))
    integrate(filled, cases.fan(shape))
    data = read_all(filled)
    listed = {k: data[k] for k in sorted(data)[::2]}
    maps = [make("occ", shape, layers=layers) for _ in range(3)]
    own = cases.fan(shape, scale=0.5, shift=(0.0, 0.0, 1.1))
    for gm in maps:
        integrate(gm, own)
        gm.clearanceUpdate(radius)
        assert len(gm.clearanceStaleRegions(radius)) == 0
        gm.syncVoxels()
        assert keys_of(gm, dirty_only=True) == []
    held_before = len(keys_of(maps[0]))
    source = make("occ", shape, layers=("occupancy",))
    by_upload(maps[0], listed)
    by_upload(source, listed)
    assert copyMap(maps[1], source)
    by_voxel_writes(maps[2], listed, ("occupancy",))
    assert_same_words(maps, ["occupancy"])
    assert sorted(keys_of(maps[1], dirty_only=True)) == sorted(keys_of(maps[2], dirty_only=True)) == sorted(listed)
    stale = [[tuple(int(v) for v in k) for k in gm.clearanceStaleRegions(radius)] for gm in maps]
    print("clearance stale", len(stale[0]), "of", len(keys_of(maps[0])), "held before", held_before)
    assert stale[0] and stale[0] == stale[1] == stale[2]
    assert set(listed) <= set(stale[0])
    done = [gm.clearanceUpdate(radius) for gm in maps]
    assert done[0][1] == 0 and done[0] == done[1] == done[2]
    assert_same_words(maps)
