"""-m gpu: voxels edited by key on the device (ohmhip_map_write_voxels / ohmhip_map_integrate_voxels and their _device
forms; GpuMap.writeVoxels / integrateVoxels / integrateHits / integrateMisses) against the sequential model of tests/
voxel_edit_ref.py applied to the blocks read before the edit.  Every comparison is on uint32 views of whole region
blocks read from the device into fresh buffers (test_gpu_mean_states.read_device); there is no tolerance except in the
NDT case, which keeps the bar of tests/test_gpu_ndt_states.py.  Regions are 8 x 8 x 8 unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import mean_cases
import occupancy_cases as OC
import voxel_edit_ref as V
from ohm_amd import (LAYERS, ClearanceProcess, GpuMap, GpuNdtMap, GpuTsdfMap, OccupancyMap, OhmHipError, VoxelEdit,
                     compareVoxels, synth)
from ohm_amd import _lib as L
from parity import assert_parity, compare_maps, make_oracle
from test_gpu_mean_states import read_device
from test_gpu_occupancy_states import set_config

pytestmark = pytest.mark.gpu

F = np.float32
NULL_KEY = (V.NULL_REGION, (0, 0, 0))
ALL_LAYERS = ("occupancy", "mean", "covariance", "traversal", "touch_time", "clearance")


def new_map(layers=("occupancy",), dim=8, cls=GpuMap, res=0.1, cfg=None, origin=None, coalesce=0, **kw):
    dim = (dim,) * 3 if np.isscalar(dim) else tuple(dim)
    map_ = OccupancyMap(res, dim, layers=tuple(n for n in layers if n != "clearance"))
    if "clearance" in layers:
        ClearanceProcess.ensureClearanceLayer(map_)
    if origin is not None:
        map_.setOrigin(origin)
    if cfg is not None:
        set_config(map_, cfg)
    gm = cls(map_, **kw)
    if coalesce is not None:
        gm.setBatchCoalescing(coalesce)
    return map_, gm, V.geometry(res, dim, tuple(map_.layers), map_.origin)


def blocks_of(map_, gm):
    return {r: {n: b.copy() for n, b in layers.items()} for r, layers in read_device(map_, gm).items()}


def key_pair(keys):
    """[(region, local)] -> the (regions, locals) pair the mirror takes."""
    return (np.array([k[0] for k in keys], dtype=np.int16).reshape(-1, 3),
            np.array([k[1] for k in keys], dtype=np.uint8).reshape(-1, 3))


def assert_blocks(device, model, what=""):
    assert set(device) == set(model), (what, sorted(set(device) ^ set(model)))
    for region in model:
        for name, want in model[region].items():
            got = device[region][name]
            bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
            assert bad.size == 0, (what, region, name, bad.size, bad[:6], got.view(np.uint32)[bad[:6]],
                                   want.view(np.uint32)[bad[:6]])


def interleave(runs):
    """{key: [element, ...]} -> one list in which every key's elements keep their order and no run is contiguous."""
    out = []
    for k in range(max(len(r) for r in runs.values())):
        out += [r[k] for r in runs.values() if len(r) > k]
    return out


def integrate_elements(gm, elements):
    """HIT / MISS / HIT_SAMPLE elements through one integrateVoxels call (keys, or points when any element has one)."""
    ops = np.array([e.op for e in elements], dtype=np.uint8)
    if any(e.point is not None for e in elements):
        return gm.integrateVoxels(ops, points=np.array([e.point for e in elements], dtype=np.float64))
    return gm.integrateVoxels(ops, keys=key_pair([e.key for e in elements]))


def set_elements(gm, layer, keys, values):
    gm.writeVoxels(key_pair(keys), layer, values)
    return [V.Element(V.SET, k, None, layer, v) for k, v in zip(keys, values)]


# -- 1. SET round trip -----------------------------------------------------------------------------------------------

def layer_values(name, n, seed):
    dtype, comps = LAYERS[name][1:]
    raw = np.random.default_rng(seed).integers(0, 1 << 32, size=n * comps, dtype=np.uint64).astype(np.uint32)
    raw[:comps] = 0x7fc01234 if dtype == np.float32 else 0xffffffff                      # a NaN payload / all ones
    raw[comps:2 * comps] = 0x80000000                                                    # -0.0
    return raw.view(dtype).reshape((n, comps) if comps > 1 else n)


@pytest.mark.parametrize("kind", ["occupancy", "tsdf"])
def test_set_round_trip(gpu, kind):
    if kind == "tsdf":
        map_, gm, geo = new_map((), cls=GpuTsdfMap, default_truncation_distance=0.2)
    else:
        map_, gm, geo = new_map(ALL_LAYERS)
    rays = synth.random_rays(300, extent=1.5, seed=5)
    assert gm.integrateRays(rays) == rays.shape[0]
    before = blocks_of(map_, gm)
    absent = (9, -7, 3)
    assert absent not in before
    keys = [((0, 0, 0), (1, 2, 3)), NULL_KEY, ((0, 0, 0), (7, 7, 7)), (absent, (0, 0, 0)), ((0, 0, 0), (1, 2, 3)),
            (absent, (7, 0, 5)), ((-1, 0, 0), (4, 4, 4)), NULL_KEY, ((0, 0, 0), (7, 7, 7))]
    model = {r: {n: b.copy() for n, b in layers.items()} for r, layers in before.items()}
    for i, name in enumerate(map_.layers):
        values = layer_values(name, len(keys), 100 + i)
        elements = set_elements(gm, name, keys, values)
        want = V.apply(model, geo, None, elements)
        assert gm.lastEditStats() == want, (name, gm.lastEditStats(), want)
        assert want["null_keys"] == 2 and want["distinct_voxels"] == 5
        # the last of the duplicates won; a null key reads as absent
        got, present = gm.readVoxels(key_pair(keys), name)
        last = {k: values[j] for j, k in enumerate(keys)}
        for j, k in enumerate(keys):
            if k == NULL_KEY:
                assert present[j] == 0
            else:
                assert present[j] == 1
                assert np.array_equal(np.asarray(got[j]).view(np.uint32), np.asarray(last[k]).view(np.uint32)), (name, j)
    after = blocks_of(map_, gm)
    assert_blocks(after, model, kind)
    # untouched voxels of the created region read the clear value; untouched regions are byte-identical
    for name in map_.layers:
        clear = V.clear_block(geo, name)
        comps = LAYERS[name][2]
        untouched = np.ones(V.volume(geo), dtype=bool)
        untouched[[V.voxel_index(geo, (0, 0, 0)), V.voxel_index(geo, (7, 0, 5))]] = False
        assert np.array_equal(after[absent][name].view(np.uint32).reshape(-1, comps)[untouched],
                              clear.view(np.uint32).reshape(-1, comps)[untouched]), name
    for region in set(before) - {(0, 0, 0), (-1, 0, 0)}:
        for name in map_.layers:
            assert before[region][name].tobytes() == after[region][name].tobytes(), (region, name)
    assert len(set(before) - {(0, 0, 0), (-1, 0, 0)}) > 3
    gm.close()


# -- 2. HIT / MISS states, 3. run lengths ------------------------------------------------------------------------------

def voxel_keys(n, geo, first_region=0):
    """n distinct keys filling regions (first_region + i, 0, 0) voxel by voxel."""
    vol = V.volume(geo)
    d = geo.dim
    return [((first_region + i // vol, 0, 0), ((i % vol) % d[0], ((i % vol) // d[0]) % d[1], (i % vol) // (d[0] * d[1])))
            for i in range(n)]


def test_hit_miss_states(gpu):
    map_, gm, geo = new_map()
    for name, cfg in OC.configs().items():
        set_config(map_, cfg)
        states = OC.edge_states(cfg)
        cells = [(value, pattern) for value in states.values() for pattern in OC.PATTERNS]
        keys = voxel_keys(len(cells), geo)
        model = blocks_of(map_, gm)
        V.apply(model, geo, cfg, set_elements(gm, "occupancy", keys, np.array([c[0] for c in cells], dtype=F)))
        assert_blocks(blocks_of(map_, gm), model, name + ": planted")
        runs = {k: [V.Element(V.MISS if c == "m" else V.HIT, k) for c in cell[1]] for k, cell in zip(keys, cells)}
        elements = interleave(runs)
        for call in range(2):
            assert integrate_elements(gm, elements) == len(elements)
            want = V.apply(model, geo, cfg, elements)
            assert gm.lastEditStats() == want
            assert_blocks(blocks_of(map_, gm), model, "%s: call %d" % (name, call))
    gm.close()


@pytest.mark.parametrize("cfg_name", ["tight_11", "tiny"])
def test_run_lengths(gpu, cfg_name):
    cfg = OC.configs()[cfg_name]
    map_, gm, geo = new_map(cfg=cfg)
    lengths = (1, 2, 63, 64, 65, 257)
    keys = voxel_keys(len(lengths), geo)
    runs = {k: [V.Element(V.HIT if i % 3 == 0 else V.MISS, k) for i in range(n)] for k, n in zip(keys, lengths)}
    elements = interleave(runs)
    model = {}
    for call in range(3):                                      # (the later calls start at the clamps)
        assert integrate_elements(gm, elements) == sum(lengths)
        V.apply(model, geo, cfg, elements)
        assert_blocks(blocks_of(map_, gm), model, "%s: call %d" % (cfg_name, call))
    assert gm.lastEditStats()["distinct_voxels"] == len(lengths)
    gm.close()


# -- 4. HIT_SAMPLE ----------------------------------------------------------------------------------------------------

PLANTED_COUNTS = (0, 1, 0xfffffffe, 0xffffffff)


def sample_cases(config, limit=48):
    """Cases of one sheet of mean_cases (voxel faces, grid cell edges, near-ties of the 10-bit cell), every fourth
    with one of the planted counts in the place of its own."""
    sheet = [s for s in mean_cases.build() if s.config == config][0]
    return mean_cases.geometry(config), sheet.cases[:limit]


@pytest.mark.parametrize("config", ["near10", "far25"])
def test_hit_sample(gpu, config):
    mgeo, cases = sample_cases(config)
    map_, gm, geo = new_map(("occupancy", "mean"), dim=mgeo.dim, res=mgeo.res, origin=mgeo.origin)
    region = tuple(mgeo.region)
    keys = [(region, tuple(c.local)) for c in cases]
    counts = [PLANTED_COUNTS[(i // 4) % 4] if i % 4 == 0 else c.count for i, c in enumerate(cases)]
    assert set(PLANTED_COUNTS) <= set(counts)
    model = {}
    V.apply(model, geo, None, set_elements(gm, "occupancy", keys, np.array([c.occupancy for c in cases], dtype=F)))
    V.apply(model, geo, None, set_elements(gm, "mean", keys, np.array([(c.coord, n) for c, n in zip(cases, counts)],
                                                                          dtype=np.uint32)))
    runs = {}
    for k, c in zip(keys, cases):
        ends = list(c.ends) + [c.ends[0]] * 2                 # several samples per voxel
        assert all(V.voxel_key(geo, e) == k for e in ends)
        runs[k] = [V.Element(V.HIT_SAMPLE, point=tuple(e)) for e in ends]
    elements = interleave(runs)
    cfg = OC.configs()["default"]
    assert integrate_elements(gm, elements) == len(elements)
    V.apply(model, geo, cfg, elements)
    after = blocks_of(map_, gm)
    assert_blocks(after, model, config)
    vi = [V.voxel_index(geo, k[1]) for k, n in zip(keys, counts) if n == 0xffffffff][0]
    assert after[region]["mean"][2 * vi + 1] == 0xffffffff
    gm.close()


def test_hit_sample_touches_no_other_layer(gpu):
    map_, gm, geo = new_map(("occupancy", "mean", "covariance", "traversal", "touch_time", "incident_normal"),
                            cls=GpuNdtMap)
    rays = synth.random_rays(400, extent=1.2, seed=9)
    assert gm.integrateRays(rays, None, np.arange(400, dtype=np.float64) * 0.01) == rays.shape[0]
    before = blocks_of(map_, gm)
    points = np.concatenate([rays[1::2][:200], rays[1::2][:50] + 0.01, [[5.03, 5.02, 5.01]]])
    elements = [V.Element(V.HIT_SAMPLE, point=tuple(p)) for p in points]
    cfg = OC.configs()["default"]
    assert gm.integrateHits(points=points, update_mean=True) == len(points)
    model = {r: {n: b.copy() for n, b in layers.items()} for r, layers in before.items()}
    want = V.apply(model, geo, cfg, elements)
    assert gm.lastEditStats() == want and want["regions_created"] >= 1
    after = blocks_of(map_, gm)
    assert_blocks(after, model, "ndt map")
    for region in before:
        for name in ("covariance", "traversal", "touch_time", "incident_normal"):
            assert before[region][name].tobytes() == after[region][name].tobytes(), (region, name)
    assert any(before[r]["touch_time"].any() for r in before) and any(before[r]["covariance"].any() for r in before)
    # without the mean layer only the occupancy changes (updatePositionSafe)
    map2, gm2, geo2 = new_map()
    assert gm2.integrateHits(points=points, update_mean=True) == len(points)
    model2 = {}
    V.apply(model2, geo2, cfg, elements)
    assert_blocks(blocks_of(map2, gm2), model2, "no mean layer")
    gm.close()
    gm2.close()


# -- 5. order against rays -----------------------------------------------------------------------------------------------

def oracle_blocks(om, names):
    return {r: {n: b.copy() for n, b in layers.items()} for r, layers in om.chunks(names).items()}


def put_blocks(om, blocks):
    for region, layers in blocks.items():
        for name, block in layers.items():
            om.region_layer_view(region, name)[:] = block


@pytest.mark.parametrize("mode", ["coalesced", "async"])
def test_order_against_rays(gpu, mode):
    n = 500 if mode == "coalesced" else 66000
    map_, gm, geo = new_map(("occupancy", "mean"), coalesce=None)      # the default coalescing threshold
    if mode == "async":
        gm.setAsyncLaunch(True)
    first = synth.random_rays(n, extent=1.4, seed=21)
    second = synth.random_rays(n, extent=1.4, seed=22)
    # thirty misses drive a sampled voxel from the hit side onto the min clamp, a hit and a sample follow: applied
    # ahead of the first rays, or behind the second, the clamp lands elsewhere
    targets = first[1::2][:40]
    elements = interleave({i: [V.Element(V.MISS, point=tuple(p))] * 30 + [V.Element(V.HIT, point=tuple(p)),
                                                                          V.Element(V.HIT_SAMPLE, point=tuple(p))]
                           for i, p in enumerate(targets)})
    assert gm.integrateRays(first) == first.shape[0]
    assert integrate_elements(gm, elements) == len(elements)
    assert gm.lastEditStats()["regions_created"] == 0         # every target's region came with the first rays
    assert gm.integrateRays(second) == second.shape[0]
    om = make_oracle(map_)
    om.integrate_occupancy(first)
    blocks = oracle_blocks(om, map_.layers)
    V.apply(blocks, geo, OC.configs()["default"], elements)
    put_blocks(om, blocks)
    om.integrate_occupancy(second)
    assert_blocks(blocks_of(map_, gm), oracle_blocks(om, map_.layers), mode)
    gm.close()


# -- 6. regions and bookkeeping ------------------------------------------------------------------------------------------

def keyset(keys):
    return sorted(tuple(int(v) for v in k) for k in np.asarray(keys).reshape(-1, 3))


def test_regions_and_bookkeeping(gpu):
    map_, gm, geo = new_map(("occupancy", "mean"))
    rays = synth.random_rays(300, extent=1.5, seed=31)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()                                           # (clears the dirty marks)
    assert len(gm.regionKeys(dirty_only=True)) == 0
    held = keyset(gm.regionKeys())
    points = np.array([[4.01, 4.02, 4.03], [-3.3, 2.2, 0.1], [0.051, 0.052, 0.053], [4.015, 4.02, 4.03],
                       [1e9, 0.0, 0.0]])
    elements = [V.Element(V.HIT_SAMPLE, point=tuple(p)) for p in points]
    model = blocks_of(map_, gm)
    assert gm.integrateHits(points=points, update_mean=True) == 4
    want = V.apply(model, geo, OC.configs()["default"], elements)
    assert gm.lastEditStats() == want
    assert want["regions_created"] == 2 and want["regions_touched"] == 3 and want["null_keys"] == 1
    touched = sorted({V.voxel_key(geo, p)[0] for p in points[:4]})
    assert keyset(gm.regionKeys()) == sorted(set(held) | set(touched))
    assert keyset(gm.regionKeys(dirty_only=True)) == touched
    # syncVoxels brings the edit into the host chunks
    gm.syncVoxels()
    for region in touched:
        for name in map_.layers:
            assert np.array_equal(map_.chunks[region][name].view(np.uint32), model[region][name].view(np.uint32))
    # a second map that received the same voxels through uploadRegions compares equal
    map2 = OccupancyMap(0.1, (8, 8, 8), layers=("occupancy", "mean"))
    for region, layers in model.items():
        map2.chunks[region] = {n: b.copy() for n, b in layers.items()}
    gm2 = GpuMap(map2)
    for name in map_.layers:
        for eval_, ref in ((gm, gm2), (gm2, gm)):
            result = compareVoxels(eval_, ref, name, flags=1)
            assert result.voxels_failed == 0 and result.voxels_passed == len(model) * V.volume(geo), (name, result)
    gm.close()
    gm2.close()


def test_free_a_box_with_key_range(gpu):
    map_, gm, geo = new_map()
    lo, hi = (-0.55, 0.31, -0.45), (-0.32, 0.48, -0.33)         # crosses a region corner
    keys = gm.keyRange(lo, hi)
    want_keys = V.key_range(geo, V.voxel_key(geo, lo), V.voxel_key(geo, hi))
    assert [(tuple(int(v) for v in k["region"]), tuple(int(v) for v in k["voxel"][:3])) for k in keys] == want_keys
    assert len({k[0] for k in want_keys}) == 8
    assert gm.integrateMisses(gm.keyRange(lo, hi)) == len(want_keys)
    assert gm.integrateVoxels(VoxelEdit.kHit, keys=keys[:5]) == 5
    model = {}
    cfg = OC.configs()["default"]
    V.apply(model, geo, cfg, [V.Element(V.MISS, k) for k in want_keys] + [V.Element(V.HIT, k) for k in want_keys[:5]])
    assert_blocks(blocks_of(map_, gm), model, "box")
    gm.close()


# -- 7. spill and limit ------------------------------------------------------------------------------------------------

def test_spilled_regions_come_back(gpu):
    map_, gm, geo = new_map(region_capacity=16)
    gm.setMemoryLimit(16 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    model = {}
    cfg = OC.configs()["default"]
    for base in range(0, 40, 8):
        elements = [V.Element(V.HIT, ((r, 1, -2), (r % 8, 3, 5))) for r in range(base, base + 8)]
        assert integrate_elements(gm, elements) == 8
        V.apply(model, geo, cfg, elements)
    st = gm.cacheStats()
    assert st["regions_spilled"] > 0 and st["regions_resident"] <= 16 and len(gm.regionKeys()) == 40
    assert_blocks(blocks_of(map_, gm), model, "40 regions")
    back = gm.cacheStats()["readmissions"]
    for base in (0, 16):                                      # (16 regions are resident: one of the calls names stored ones)
        elements = [V.Element(V.MISS, ((r, 1, -2), (r % 8, 3, 5))) for r in range(base, base + 16)]
        elements.append(V.Element(V.HIT, ((base, 1, -2), (7, 7, 7))))
        assert integrate_elements(gm, elements) == 17
        want = V.apply(model, geo, cfg, elements)
        assert gm.lastEditStats() == want and want["regions_created"] == 0
    assert gm.cacheStats()["readmissions"] > back
    assert_blocks(blocks_of(map_, gm), model, "after the edit of a stored region")
    gm.close()


def test_capacity_changes_nothing(gpu):
    map_, gm, geo = new_map(region_capacity=4)
    gm.setMemoryLimit(4 * gm.cacheStats()["bytes_per_region"])
    elements = [V.Element(V.HIT, ((r, 0, 0), (1, 1, 1))) for r in range(4)]
    assert integrate_elements(gm, elements) == 4
    before = blocks_of(map_, gm)
    regions = keyset(gm.regionKeys())
    more = [V.Element(V.MISS, ((0, 0, 0), (1, 1, 1)))] + [V.Element(V.HIT, ((r, 5, 0), (2, 2, 2))) for r in range(3)]
    with pytest.raises(OhmHipError) as err:
        integrate_elements(gm, more)
    assert err.value.status == L.ERR_CAPACITY
    assert gm.lastEditStats() == dict.fromkeys(gm.lastEditStats(), 0)
    with pytest.raises(OhmHipError) as err:
        gm.writeVoxels(key_pair([e.key for e in more]), "occupancy", np.zeros(4, dtype=F))
    assert err.value.status == L.ERR_CAPACITY
    assert keyset(gm.regionKeys()) == regions
    assert_blocks(blocks_of(map_, gm), before, "after the refused edits")
    gm.close()


# -- 8. tiled regions ----------------------------------------------------------------------------------------------------

def test_tiled_regions(gpu):
    dim = (40, 36, 37)                                        # cut into 37 tiles of one z layer each
    map_, gm, geo = new_map(("occupancy", "mean"), dim=dim)
    rays = synth.random_rays(200, extent=1.0, seed=41)        # reaches a few tiles of the regions around the origin
    assert gm.integrateRays(rays) == rays.shape[0]
    model = blocks_of(map_, gm)
    cfg = OC.configs()["default"]
    keys = [(region, (x, y, z)) for region in ((0, 0, 0), (-1, 2, 0)) for z in range(dim[2])
            for x, y in ((0, 0), (39, 35), (z % 40, (5 * z) % 36))]
    runs = {k: [V.Element(V.HIT if (i + j) % 2 else V.MISS, k) for j in range(1 + i % 3)] for i, k in enumerate(keys)}
    elements = interleave(runs)
    assert integrate_elements(gm, elements) == len(elements)
    want = V.apply(model, geo, cfg, elements)
    assert gm.lastEditStats() == want and want["regions_created"] == 1 and want["regions_touched"] == 2
    assert_blocks(blocks_of(map_, gm), model, "tiled, keys")
    points = np.array([V.voxel_centre(geo, k) for k in keys[::3]]) + 0.01
    elements = [V.Element(V.HIT_SAMPLE, point=tuple(p)) for p in points]
    assert gm.integrateHits(points=points, update_mean=True) == len(points)
    V.apply(model, geo, cfg, elements)
    assert_blocks(blocks_of(map_, gm), model, "tiled, points")
    values, present = gm.readVoxels(key_pair(keys), "occupancy")
    assert present.all()
    want_values = np.array([model[k[0]]["occupancy"][V.voxel_index(geo, k[1])] for k in keys], dtype=F)
    assert np.array_equal(values.view(np.uint32), want_values.view(np.uint32))
    gm.close()


# -- 9. replay masks -----------------------------------------------------------------------------------------------------

def plant_oracle(om, geo, blocks, integrate):
    """The regions of `blocks` created in the oracle and every layer of them overwritten."""
    for region in blocks:
        c = np.array(V.voxel_centre(geo, (region, (0, 0, 0))))
        integrate(np.array([c, c]))
    put_blocks(om, blocks)


def test_ndt_replay_mask(gpu):
    map_, gm, geo = new_map((), dim=32, cls=GpuNdtMap)
    key = ((0, 0, 0), (20, 21, 22))
    centre = np.array(V.voxel_centre(geo, key))
    sample = tuple(centre + (0.011, -0.023, 0.017))
    elements = [V.Element(V.HIT_SAMPLE, point=sample)] * 2
    assert integrate_elements(gm, elements) == 2
    model = {}
    V.apply(model, geo, OC.configs()["default"], elements)
    assert_blocks(blocks_of(map_, gm), model, "the edit alone")
    # 2 000 NDT rays from one sensor: half end in the voxel, half pass through it
    rng = np.random.default_rng(3)
    sensor = centre + (-1.1, -0.9, 0.7)
    ends = centre + rng.uniform(-0.045, 0.045, size=(2000, 3))
    ends[1::2] = sensor + (ends[1::2] - sensor) * 1.5
    rays = np.empty((4000, 3))
    rays[0::2], rays[1::2] = sensor, ends
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    om = make_oracle(map_)
    om.set_ndt(sensor_noise=gm.sensor_noise, sample_threshold=gm.sample_threshold, adaptation_rate=gm.adaptation_rate,
               reinit_threshold=gm.reinitialise_covariance_threshold, reinit_count=gm.reinitialise_covariance_point_count)
    plant_oracle(om, geo, model, om.integrate_ndt)
    om.integrate_ndt(rays)
    layers = ["occupancy", "mean", "covariance"]
    assert_parity(compare_maps(om.chunks(), map_.chunks, layers, rel=1e-5))
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["mean"]))
    gm.close()


def test_tsdf_replay_mask(gpu):
    trunc = 0.2
    map_, gm, geo = new_map((), cls=GpuTsdfMap, default_truncation_distance=trunc)
    rays = synth.random_rays(300, extent=1.2, seed=51)
    assert gm.integrateRays(rays) == rays.shape[0]
    model = blocks_of(map_, gm)
    ends = rays[1::2]
    # voxels the next rays cross: midpoints of rays, in free space
    mids = 0.5 * (rays[0::2] + ends)
    keys = [V.voxel_key(geo, mids[0]), V.voxel_key(geo, mids[1])]
    assert keys[0] != keys[1]
    values = np.array([[2.5, 0.01], [0.0, 0.0]], dtype=F)     # not countable; never observed
    V.apply(model, geo, None, set_elements(gm, "tsdf", keys, values))
    assert gm.integrateRays(rays) == rays.shape[0]
    om = make_oracle(map_)
    om.set_tsdf(trunc=trunc)
    om.integrate_tsdf(rays)
    put_blocks(om, {r: {"tsdf": layers["tsdf"]} for r, layers in model.items()})
    om.integrate_tsdf(rays)
    assert_blocks(blocks_of(map_, gm), oracle_blocks(om, ["tsdf"]), "tsdf")
    gm.close()


# -- 10. clearance -------------------------------------------------------------------------------------------------------

def test_clearance_marks(gpu):
    from clearance_ref import Geometry, clearance_regions
    from rays_query_ref import ChunkBlocks
    radius = float(F(1.5 * 0.1))
    maps = [new_map(("occupancy", "clearance")) for _ in range(2)]
    rays = synth.random_rays(600, extent=1.6, seed=61)
    for map_, gm, geo in maps:
        assert gm.integrateRays(rays) == rays.shape[0]
        gm.clearanceUpdate(radius)
        assert len(gm.clearanceStaleRegions(radius)) == 0
    (map_a, gm_a, geo), (map_b, gm_b, _) = maps
    # a free voxel: the start voxel of the rays
    key = V.voxel_key(geo, rays[0])
    before = blocks_of(map_a, gm_a)
    vi = V.voxel_index(geo, key[1])
    assert before[key[0]]["occupancy"][vi] < 0
    elements = [V.Element(V.HIT, key)] * 12
    assert integrate_elements(gm_a, elements) == 12
    model = {r: {n: b.copy() for n, b in layers.items()} for r, layers in before.items()}
    V.apply(model, geo, OC.configs()["default"], elements)
    assert model[key[0]]["occupancy"][vi] > 0
    # the twin receives the same block by ohmhip_map_write_regions
    block = model[key[0]]["occupancy"]
    k = np.array([key[0]], dtype=np.int16)
    ptrs = (C.c_void_p * 1)(block.ctypes.data)
    L.check(L.lib.ohmhip_map_write_regions(gm_b._handle, L.LID_OCCUPANCY, k.ctypes.data, 1, ptrs), "write")
    stale = keyset(gm_a.clearanceStaleRegions(radius))
    assert stale == keyset(gm_b.clearanceStaleRegions(radius)) and key[0] in stale and len(stale) > 1
    gm_a.clearanceUpdate(radius)
    assert len(gm_a.clearanceStaleRegions(radius)) == 0
    gm_a.syncVoxels()
    regions = np.array(stale, dtype=np.int16)
    ref = clearance_regions(Geometry(0.1, (8, 8, 8), map_a.occupancy_threshold_value), ChunkBlocks(map_a.chunks), regions,
                            radius)
    got = np.stack([map_a.chunks[r]["clearance"] for r in stale]).reshape(np.asarray(ref).shape)
    assert np.array_equal(got.view(np.uint32), np.asarray(ref, dtype=F).view(np.uint32))
    # a SET on the clearance layer: the marks of ohmhip_map_write_regions + ohmhip_map_mark_dirty on the twin
    gm_b.clearanceUpdate(radius)
    gm_a.writeVoxels(key_pair([key]), "clearance", np.array([0.5], dtype=F))
    block = blocks_of(map_b, gm_b)[key[0]]["clearance"]
    block[vi] = 0.5
    ptrs = (C.c_void_p * 1)(block.ctypes.data)
    L.check(L.lib.ohmhip_map_write_regions(gm_b._handle, L.LID_CLEARANCE, k.ctypes.data, 1, ptrs), "write")
    slot = C.c_uint32(0)
    L.check(L.lib.ohmhip_map_region_slot(gm_b._handle, k.ctypes.data, C.byref(slot)), "slot")
    L.check(L.lib.ohmhip_map_mark_dirty(gm_b._handle, C.byref(slot), 1), "mark_dirty")
    stale = keyset(gm_a.clearanceStaleRegions(radius))
    assert stale == keyset(gm_b.clearanceStaleRegions(radius)) and key[0] in stale
    assert_blocks(blocks_of(map_a, gm_a), blocks_of(map_b, gm_b), "twins")
    for _, gm, _ in maps:
        gm.close()


# -- 11. device forms ----------------------------------------------------------------------------------------------------

class DeviceArray:
    """A numpy array's bytes in device memory (an ohmhip_buffer; torch cannot open the device once the library has)."""

    def __init__(self, array):
        array = np.ascontiguousarray(array)
        self.handle = L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(self.handle), max(array.nbytes, 16), 3), "buffer_create")
        L.check(L.lib.ohmhip_buffer_write(self.handle, array.ctypes.data, array.nbytes, 0, None, None, None), "write")
        self.ptr = L._vp()
        L.check(L.lib.ohmhip_buffer_ptr(self.handle, C.byref(self.ptr)), "buffer_ptr")

    def close(self):
        L.lib.ohmhip_buffer_destroy(self.handle)


def test_device_forms(gpu):
    cfg = OC.configs()["tight_11"]
    mgeo, cases = sample_cases("near10", limit=16)
    region = tuple(mgeo.region)
    keys = [(region, tuple(c.local)) for c in cases] + [NULL_KEY, ((5, 5, 5), (200, 0, 0))]
    rec = np.zeros((len(keys), 10), dtype=np.uint8)
    rec[:, :6] = key_pair(keys)[0].view(np.uint8).reshape(-1, 6)
    rec[:, 6:9] = key_pair(keys)[1]
    mean_values = np.array([(c.coord, PLANTED_COUNTS[i % 4]) for i, c in enumerate(cases)] + [(1, 1)] * 2, dtype=np.uint32)
    patterns = [OC.PATTERNS[i % len(OC.PATTERNS)] or "h" for i in range(len(cases))]
    key_elements = interleave({k: [V.Element(V.MISS if ch == "m" else V.HIT, k) for ch in p]
                               for k, p in zip(keys, patterns)})
    key_rec = np.zeros((len(key_elements), 10), dtype=np.uint8)
    pair = key_pair([e.key for e in key_elements])
    key_rec[:, :6], key_rec[:, 6:9] = pair[0].view(np.uint8).reshape(-1, 6), pair[1]
    key_ops = np.array([e.op for e in key_elements] , dtype=np.uint8)
    points = np.array([e for c in cases for e in c.ends] + [[np.nan, 0.0, 0.0], [1e9, 0.0, 0.0]])
    point_ops = np.array([1 + i % 3 for i in range(len(points))], dtype=np.uint8)
    results = []
    for device in (False, True):
        map_, gm, geo = new_map(("occupancy", "mean"), dim=mgeo.dim, res=mgeo.res, origin=mgeo.origin, cfg=cfg)
        gm._push_config_if_changed()
        stats = []

        def call(fn, *args):
            st = L.VoxelEditStats()
            L.check(fn(*args, C.byref(st)), fn.__name__)
            stats.append({name: int(getattr(st, name)) for name, _ in L.VoxelEditStats._fields_})

        if device:
            buffers = {n: DeviceArray(a) for n, a in (("rec", rec), ("mean", mean_values), ("key_rec", key_rec),
                                                      ("key_ops", key_ops), ("points", points[:-2]),
                                                      ("all_points", points), ("point_ops", point_ops))}
            p = {n: b.ptr for n, b in buffers.items()}
            call(L.lib.ohmhip_map_write_voxels_device, gm._handle, L.LID_MEAN, p["rec"], len(keys), p["mean"])
            call(L.lib.ohmhip_map_integrate_voxels_device, gm._handle, p["key_ops"], 0, p["key_rec"], None, len(key_ops))
            call(L.lib.ohmhip_map_integrate_voxels_device, gm._handle, p["point_ops"], 0, None, p["all_points"],
                 len(points))
            call(L.lib.ohmhip_map_integrate_voxels_device, gm._handle, None, L.EDIT_HIT_SAMPLE, None, p["points"],
                 len(points) - 2)
        else:
            # (the host forms refuse what the device forms skip: the out-of-region key and the NaN go as null keys)
            host_rec = rec.copy()
            host_rec[-1] = host_rec[-2]
            host_points = points.copy()
            host_points[-2] = host_points[-1]
            call(L.lib.ohmhip_map_write_voxels, gm._handle, L.LID_MEAN, host_rec.ctypes.data, len(keys),
                 mean_values.ctypes.data)
            call(L.lib.ohmhip_map_integrate_voxels, gm._handle, key_ops.ctypes.data, 0, key_rec.ctypes.data, None,
                 len(key_ops))
            call(L.lib.ohmhip_map_integrate_voxels, gm._handle, point_ops.ctypes.data, 0, None, host_points.ctypes.data,
                 len(points))
            call(L.lib.ohmhip_map_integrate_voxels, gm._handle, None, L.EDIT_HIT_SAMPLE, None, points.ctypes.data,
                 len(points) - 2)
            # ... and refuse them before any device work
            st = L.VoxelEditStats()
            assert L.lib.ohmhip_map_write_voxels(gm._handle, L.LID_MEAN, rec.ctypes.data, len(keys),
                                                 mean_values.ctypes.data, C.byref(st)) == L.ERR_INVALID_ARG
            assert L.lib.ohmhip_map_integrate_voxels(gm._handle, point_ops.ctypes.data, 0, None, points.ctypes.data,
                                                     len(points), C.byref(st)) == L.ERR_INVALID_ARG
            assert L.lib.ohmhip_map_write_voxels(gm._handle, L.LID_TSDF, host_rec.ctypes.data, len(keys),
                                                 mean_values.ctypes.data, C.byref(st)) == L.ERR_UNSUPPORTED
        gm.wait()
        results.append((blocks_of(map_, gm), stats))
        gm.close()
        if device:
            for b in buffers.values():
                b.close()
    (host_blocks, host_stats), (device_blocks, device_stats) = results
    assert host_stats == device_stats and host_stats[0]["null_keys"] == 2 and host_stats[2]["null_keys"] == 2
    assert_blocks(device_blocks, host_blocks, "device forms against host forms")
    # and both are the model's
    geo = V.geometry(mgeo.res, mgeo.dim, ("occupancy", "mean"), mgeo.origin)
    model = {}
    V.apply(model, geo, cfg, [V.Element(V.SET, k, None, "mean", v) for k, v in zip(keys[:-1], mean_values)])
    V.apply(model, geo, cfg, key_elements)
    V.apply(model, geo, cfg, [V.Element(int(o), point=tuple(p)) for o, p in zip(point_ops[:-2], points[:-2])])
    V.apply(model, geo, cfg, [V.Element(V.HIT_SAMPLE, point=tuple(p)) for p in points[:-2]])
    assert_blocks(host_blocks, model, "host forms against the model")
