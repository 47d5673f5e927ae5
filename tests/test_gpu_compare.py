"""-m gpu: ohmhip_map_compare / ohm_amd.compareVoxels between device maps (include/ohmhip.h, MAP COMPARE: K1 - K7).

The yardstick throughout is the CPU restatement (tests/compare_ref.py) on the blocks the two maps hold -- the planted
blocks, or what ohmhip_map_read_regions downloads -- and the device must equal it on every result field, on both lists'
bytes and on the member_max_diff bits.  Each case asserts on the restatement the precondition it exists for.  Shapes and
bit patterns: tests/compare_cases.py."""
import ctypes as C

import numpy as np
import pytest

import compare_cases as cases
import compare_ref as R
from ohm_amd import (LAYERS, GpuMap, GpuNdtMap, OccupancyMap, Severity, Tolerance, compare_maps, compareLayoutLayer,
                     compareVoxels, configureTolerance, kContinue, occupancy_stats)
from ohm_amd import _lib as L
from ohm_amd import compare as M
from ohm_amd.distributed import RegionPartition

pytestmark = pytest.mark.gpu

BIG = 1 << 20
ODD = (5, 3, 7)  # 105 voxels: every other pool slot of a 4-byte layer is only 4-byte aligned


def make(dims, layers, res=0.1, cls=GpuMap, **kwargs):
    return cls(OccupancyMap(res, dims, layers=layers), **kwargs)


def layers_for(layer):
    return ("occupancy",) if layer == "occupancy" else ("occupancy", layer)


def upload(gm, layer, chunks):
    """ohmhip_map_write_regions of {region: (voxels, members) uint32 block} into `layer`."""
    keys = sorted(chunks)
    if not keys:
        return
    karr = np.ascontiguousarray(keys, dtype=np.int16)
    blocks = [np.ascontiguousarray(chunks[k], dtype=np.uint32) for k in keys]
    ptrs = (C.c_void_p * len(keys))(*[b.ctypes.data for b in blocks])
    L.check(L.lib.ohmhip_map_write_regions(gm._handle, LAYERS[layer][0], karr.ctypes.data, len(keys), ptrs), "write")


def keys_of(gm, dirty_only=False):
    return [tuple(int(v) for v in k) for k in gm.regionKeys(dirty_only=dirty_only)]


def download(gm, layer):
    """{region: (voxels, members) uint32 block} through ohmhip_map_read_regions."""
    keys = sorted(keys_of(gm))
    if not keys:
        return {}
    karr = np.ascontiguousarray(keys, dtype=np.int16)
    members = LAYERS[layer][2]
    blocks = np.empty((len(keys), gm.map().regionVoxelVolume(), members), dtype=np.uint32)
    ptrs = (C.c_void_p * len(keys))(*[blocks[i].ctypes.data for i in range(len(keys))])
    L.check(L.lib.ohmhip_map_read_regions(gm._handle, LAYERS[layer][0], karr.ctypes.data, len(keys), ptrs), "read")
    return {k: blocks[i] for i, k in enumerate(keys)}


def pair_of_maps(layer, dims, ev, ref, **kwargs):
    ge, gr = make(dims, layers_for(layer), **kwargs), make(dims, layers_for(layer), **kwargs)
    upload(ge, layer, ev)
    upload(gr, layer, ref)
    return ge, gr


def run(ge, gr, layer, tol_members=0, tol_bits=(0,) * 6, flags=kContinue, keys=None, mismatch_capacity=BIG,
        missing_capacity=64):
    p = L.CompareParams()
    p.flags, p.layer_id, p.tolerance_members = flags, LAYERS[layer][0], tol_members
    for i in range(6):
        p.tolerance_bits[i] = tol_bits[i]
    held = None
    if keys is not None:
        held = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        p.keys_xyz, p.key_count = held.ctypes.data, len(held)
    status, detail, listed, missing = M.compare_raw(ge, gr, p, mismatch_capacity, missing_capacity)
    assert status == L.OK
    return detail, listed, missing


def assert_equals_restatement(got, want):
    """Every result field, both lists' bytes."""
    (g_res, g_keys, g_missing), (w_res, w_keys, w_missing) = got, want
    for name in w_res:
        assert g_res[name] == w_res[name], (name, g_res[name], w_res[name])
    assert set(g_res) == set(w_res)
    assert g_keys.tobytes() == w_keys.tobytes()
    assert np.array_equal(g_missing, w_missing)


def check(ge, gr, ev, ref, layer, dims, **kw):
    """Device against restatement for one call; returns the restatement's answer."""
    want = R.compare_voxels(ev, ref, layer, dims, tol_members=kw.get("tol_members", 0), tol_bits=kw.get("tol_bits", (0,) * 6),
                            flags=kw.get("flags", kContinue), keys=kw.get("keys"),
                            mismatch_capacity=kw.get("mismatch_capacity", BIG), missing_capacity=kw.get("missing_capacity", 64))
    assert_equals_restatement(run(ge, gr, layer, **kw), want)
    return want


# ---- 1. planted pairs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,regions", [(cases.SMALL, cases.SMALL_REGIONS), (cases.TWO_CHUNKS, [(0, 0, 0), (1, 0, 0)]),
                                          (ODD, cases.SMALL_REGIONS)], ids=["8x8x8", "32x16x16", "5x3x7"])
@pytest.mark.parametrize("layer", ["occupancy", "mean", "covariance", "hit_miss_count", "tsdf"])
def test_planted_mismatches(gpu, layer, dims, regions):
    plants = cases.edge_plants(layer, dims, regions)
    ev, ref = cases.planted_pair(layer, dims, regions, plants)
    ge, gr = pair_of_maps(layer, dims, ev, ref)
    res, listed, _ = check(ge, gr, ev, ref, layer, dims)
    # the preconditions: every plant is a failure of exactly its member, the edges are among them
    assert res["mismatch_count"] == len(plants) == len(listed) and res["voxels_failed"] == len(plants)
    order = R.region_order(regions)
    want_keys = sorted(((order.index(r), i, 1 << m) for r, i, m in plants))
    got_keys = [(order.index(tuple(int(v) for v in k["region"])),
                 int(k["voxel"][0]) + dims[0] * (int(k["voxel"][1]) + dims[1] * int(k["voxel"][2])), int(k["voxel"][3]))
                for k in listed]
    assert got_keys == want_keys
    indices = set(i for _, i, _ in plants)
    assert {0, cases.voxels_of(dims) - 1, 63, 64} <= indices and ((4095 in indices) == (cases.voxels_of(dims) > 4096))
    members = len(R.LAYOUT[layer][0])
    assert sum(res["member_failed"]) == len(plants) and (members == 1 or res["member_failed"][members - 1] > 0)
    assert all(d > 0 for d in res["member_max_diff"][:members] if members == 1)
    # two calls return identical bytes; stop-at-first returns the walk's answer
    assert_equals_restatement(run(ge, gr, layer), (res, listed, np.zeros((0, 3), dtype=np.int16)))
    first = check(ge, gr, ev, ref, layer, dims, flags=0)
    assert first[0]["voxels_failed"] == 1 and first[0]["voxels_passed"] == 0  # (voxel 0 of the first region is planted)
    # eval == ref is allowed and passes
    same, none, _ = run(gr, gr, layer)
    assert same["voxels_failed"] == 0 and same["voxels_passed"] == cases.voxels_of(dims) * len(regions) and len(none) == 0


# ---- 2. the K4 truth table, in voxels --------------------------------------------------------------------------------
def test_truth_table_f32_planted(gpu):
    layer, dims = "occupancy", cases.SMALL
    ev, ref, placed = cases.truth_pair(layer, dims)
    ge, gr = pair_of_maps(layer, dims, ev, ref)
    for eps in sorted(set(row[3] for _, row in placed if row[3] is not None)) + [None]:
        kw = dict(tol_members=0 if eps is None else 1, tol_bits=(eps or 0, 0, 0, 0, 0, 0))
        res, listed, _ = check(ge, gr, ev, ref, layer, dims, **kw)
        failing = set(int(k["voxel"][0]) + 8 * (int(k["voxel"][1]) + 8 * int(k["voxel"][2])) for k in listed)
        for index, row in placed:
            if row[3] == eps:
                assert (index not in failing) is row[4], row[0]
        # stop-at-first on the same pair
        check(ge, gr, ev, ref, layer, dims, flags=0, **kw)
    # member_max_diff may be inf (+inf against FLT_MAX), never a NaN's bits
    assert res["member_max_diff"][0] == cases.INF


def test_truth_table_u32_planted(gpu):
    layer, dims = "mean", cases.SMALL
    ev = {(0, 0, 0): cases.base_block(layer, dims, 5)}
    ref = {(0, 0, 0): ev[(0, 0, 0)].copy()}
    for i, row in enumerate(cases.TRUTH_U32):
        ev[(0, 0, 0)][60 + i, 1], ref[(0, 0, 0)][60 + i, 1] = row[1], row[2]
    ge, gr = pair_of_maps(layer, dims, ev, ref)
    for eps in sorted(set(row[3] for row in cases.TRUTH_U32 if row[3] is not None)) + [None]:
        kw = dict(tol_members=0 if eps is None else 0b10, tol_bits=(0, eps or 0, 0, 0, 0, 0))
        res, listed, _ = check(ge, gr, ev, ref, layer, dims, **kw)
        failing = set(int(k["voxel"][0]) + 8 * (int(k["voxel"][1]) + 8 * int(k["voxel"][2])) for k in listed)
        for i, row in enumerate(cases.TRUTH_U32):
            if row[3] == eps:
                assert ((60 + i) not in failing) is row[4], row[0]
        assert res["member_max_diff"][1] == 0xffffffff and res["member_failed"][0] == 0


def test_separate_tolerances_per_covariance_member(gpu):
    """Members 0, 2 and 5 carry a tolerance each (0, +inf, the smallest subnormal), members 1, 3 and 4 none: every truth
    row lands in the member whose rule is its own."""
    layer, dims = "covariance", cases.SMALL
    member_of = {cases.PZ: 0, cases.INF: 2, cases.SUB1: 5, None: 1}
    ev = {(0, 0, 0): cases.base_block(layer, dims, 11)}
    ref = {(0, 0, 0): ev[(0, 0, 0)].copy()}
    placed = []
    for i, row in enumerate(r for r in cases.TRUTH_F32 if r[3] in member_of):
        m = member_of[row[3]]
        ev[(0, 0, 0)][100 + i, m], ref[(0, 0, 0)][100 + i, m] = row[1], row[2]
        placed.append((100 + i, m, row))
    assert len(placed) >= 20 and set(m for _, m, _ in placed) == {0, 1, 2, 5}
    ge, gr = pair_of_maps(layer, dims, ev, ref)
    kw = dict(tol_members=0b100101, tol_bits=(cases.PZ, 0, cases.INF, 0, 0, cases.SUB1))
    res, listed, _ = check(ge, gr, ev, ref, layer, dims, **kw)
    masks = {int(k["voxel"][0]) + 8 * (int(k["voxel"][1]) + 8 * int(k["voxel"][2])): int(k["voxel"][3]) for k in listed}
    for index, m, row in placed:
        assert (masks.get(index, 0) == 0) is row[4], row[0]
        assert masks.get(index, 0) in (0, 1 << m)
    assert res["member_failed"][3] == 0 and res["member_failed"][4] == 0
    check(ge, gr, ev, ref, layer, dims, flags=0, **kw)


# ---- 3. regions one side lacks, key lists ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lacking(gpu):
    """ref: the 3 x 3 grid; eval lacks the first, a middle and the last region in order, differs in two voxels of regions
    it holds, and holds one region of its own."""
    layer, dims = "occupancy", cases.SMALL
    order = R.region_order(cases.SMALL_REGIONS)
    gone = [order[0], order[4], order[-1]]
    ev, ref = cases.planted_pair(layer, dims, cases.SMALL_REGIONS, [(order[1], 7, 0), (order[5], 300, 0)])
    for region in gone:
        del ev[region]
    ev[(5, 5, 5)] = cases.base_block(layer, dims, 77)
    ge, gr = pair_of_maps(layer, dims, ev, ref)
    return ge, gr, ev, ref, order, gone


def test_regions_eval_lacks_and_regions_only_eval_holds(lacking):
    ge, gr, ev, ref, order, gone = lacking
    res, listed, missing = check(ge, gr, ev, ref, "occupancy", cases.SMALL)
    assert [tuple(m) for m in missing.tolist()] == gone and res["regions_missing"] == 3 and res["regions_compared"] == 6
    assert res["voxels_failed"] == 3 * 512 + 2 and res["mismatch_count"] == 2 and res["member_failed"][0] == 2
    assert (5, 5, 5) in keys_of(ge) and (5, 5, 5) not in keys_of(gr)
    # the other way round: ref's own region is missing in the old ref, and nothing else
    back = check(gr, ge, ref, ev, "occupancy", cases.SMALL)
    assert back[0]["regions_missing"] == 1 and back[0]["regions_compared"] == 6


def test_key_list_with_an_absent_and_a_repeated_key(lacking):
    ge, gr, ev, ref, order, gone = lacking
    keys = [order[1], (40, 0, 0), gone[1], order[1], order[2], (5, 5, 5), order[1]]
    res, listed, missing = check(ge, gr, ev, ref, "occupancy", cases.SMALL, keys=keys)
    assert (res["keys_absent"], res["regions_compared"], res["regions_missing"]) == (2, 2, 1)
    assert res["voxels_passed"] == 2 * 512 - 1 and len(listed) == 1 and len(missing) == 1
    # a list of absent keys alone compares nothing
    res, _, _ = check(ge, gr, ev, ref, "occupancy", cases.SMALL, keys=[(40, 0, 0)])
    assert res["keys_absent"] == 1 and res["voxels_passed"] == res["voxels_failed"] == 0 and res["layout_match"] == 1


# ---- 4. stop at first -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", ["value first", "missing first", "missing last", "none"])
def test_stop_at_first(gpu, scenario):
    layer, dims = "mean", cases.SMALL
    order = R.region_order(cases.SMALL_REGIONS)
    plants, gone = {"value first": ([(order[2], 77, 1), (order[2], 400, 0), (order[6], 0, 0)], [order[4]]),
                    "missing first": ([(order[5], 3, 0)], [order[2]]),
                    "missing last": ([], [order[-1]]),
                    "none": ([], [])}[scenario]
    ev, ref = cases.planted_pair(layer, dims, cases.SMALL_REGIONS, plants)
    for region in gone:
        del ev[region]
    ge, gr = pair_of_maps(layer, dims, ev, ref)
    res, listed, missing = check(ge, gr, ev, ref, layer, dims, flags=0, mismatch_capacity=8, missing_capacity=8)
    walk = R.walk_stop_at_first(ev, ref, layer, dims)
    assert (res["voxels_passed"], res["voxels_failed"]) == walk[:2]
    assert len(listed) + len(missing) == res["voxels_failed"] == (0 if scenario == "none" else 1)
    if scenario == "value first":
        assert res["voxels_passed"] == 2 * 512 + 77 and res["member_failed"][:2] == [0, 1] and len(listed) == 1
    elif scenario == "missing first":
        assert res["voxels_passed"] == 2 * 512 and [tuple(m) for m in missing.tolist()] == [order[2]]
    elif scenario == "missing last":
        assert res["voxels_passed"] == 8 * 512 and len(missing) == 1
    else:
        assert res["voxels_passed"] == 9 * 512
    # ... and with no room in the lists the counts are the same
    check(ge, gr, ev, ref, layer, dims, flags=0, mismatch_capacity=0, missing_capacity=0)


# ---- 5. capacities ----------------------------------------------------------------------------------------------------
def test_capacities_do_not_change_the_totals(lacking):
    ge, gr, ev, ref, order, gone = lacking
    full = check(ge, gr, ev, ref, "occupancy", cases.SMALL)
    assert full[0]["mismatch_count"] == 2 and full[0]["missing_count"] == 3
    for mismatch_capacity, missing_capacity in ((0, 0), (1, 2), (2, 3), (1, 0), (0, 1), (1 << 16, 1 << 16)):
        want = R.compare_voxels(ev, ref, "occupancy", cases.SMALL, flags=kContinue, mismatch_capacity=mismatch_capacity,
                                missing_capacity=missing_capacity)
        got = run(ge, gr, "occupancy", mismatch_capacity=mismatch_capacity, missing_capacity=missing_capacity)
        assert_equals_restatement(got, want)
        assert got[0] == full[0]
        assert len(got[1]) == min(2, mismatch_capacity) and len(got[2]) == min(3, missing_capacity)
        assert got[1].tobytes() == full[1][:len(got[1])].tobytes()


# ---- 6. tiled regions -------------------------------------------------------------------------------------------------
def slab_rays(z_lo, z_hi):
    """Rays along x inside region (0, 0, 0) of the 64 x 32 x 32 shape, z within one of its two slabs."""
    g = np.arange(0.15, 1.4, 0.2)
    zz = np.linspace(z_lo, z_hi, 5)
    yy, zg = np.meshgrid(g, zz, indexing="ij")
    rays = np.empty((2 * yy.size, 3))
    rays[0::2] = np.stack([np.full(yy.size, 0.05), yy.ravel(), zg.ravel()], axis=1)
    rays[1::2] = np.stack([np.full(yy.size, 2.7), yy.ravel(), zg.ravel()], axis=1)
    return rays


def test_a_tile_one_map_lacks_reads_cleared(gpu):
    """64 x 32 x 32: two tiles (z slabs) a region.  eval holds the upper tile of region (0, 0, 0) only.  Against a ref
    whose lower tile is present but cleared everything passes; against a ref with data there exactly those voxels fail;
    and the same with the roles exchanged."""
    dims, layers = cases.TILED, ("occupancy", "mean")
    half = 64 * 32 * 16
    ge = make(dims, layers)
    assert ge.integrateRays(slab_rays(0.15, 1.05)) > 0
    assert keys_of(ge) == [(0, 0, 0)]
    ev = {name: download(ge, name) for name in layers}
    occ = ev["occupancy"][(0, 0, 0)][:, 0]
    assert np.all(occ[:half] == cases.INF) and np.any(occ[half:] != cases.INF)
    # ref 1: every tile written (ohmhip_map_write_regions names them all), the lower one with cleared values
    g1 = make(dims, layers)
    for name in layers:
        upload(g1, name, ev[name])
    # ref 2: both slabs integrated
    g2 = make(dims, layers)
    assert g2.integrateRays(np.concatenate([slab_rays(0.15, 1.05), slab_rays(-1.05, -0.15)])) > 0
    assert keys_of(g2) == [(0, 0, 0)]
    for name in layers:
        r1, r2 = download(g1, name), download(g2, name)
        res, _, _ = check(ge, g1, ev[name], r1, name, dims)
        assert res["voxels_failed"] == 0 and res["voxels_passed"] == 2 * half
        res, listed, _ = check(ge, g2, ev[name], r2, name, dims)
        assert res["voxels_failed"] > 0 and all(int(k["voxel"][2]) < 16 for k in listed)
        assert np.array_equal(r2[(0, 0, 0)][half:], ev[name][(0, 0, 0)][half:])
        back, back_listed, _ = check(g2, ge, r2, ev[name], name, dims)  # the lacking tile on the ref side
        assert back["voxels_failed"] == res["voxels_failed"] and back_listed.tobytes() == listed.tobytes()
        check(ge, g2, ev[name], r2, name, dims, flags=0)


# ---- 7. layout --------------------------------------------------------------------------------------------------------
def test_layout(gpu):
    dims = cases.SMALL
    with_mean, without = make(dims, ("occupancy", "mean")), make(dims, ("occupancy",))
    other = make(dims, ("occupancy",))
    block = {(0, 0, 0): cases.base_block("occupancy", dims, 1)}
    for gm in (with_mean, without, other):
        upload(gm, "occupancy", block)
    for ge, gr in ((with_mean, without), (without, with_mean), (without, other)):
        res, listed, missing = run(ge, gr, "mean")
        assert res == R.empty_result("mean", False) and len(listed) == 0 and len(missing) == 0
        logged = []
        assert not compareLayoutLayer(ge, gr, "mean", log=lambda sev, msg: logged.append(sev))
        assert logged == [Severity.kError] * (2 if ge is without and gr is other else 1)
        out = compareVoxels(ge, gr, "mean", flags=kContinue)
        assert not out and not out.layout_match and out.voxels_passed == 0
    assert compareLayoutLayer(with_mean, without, "occupancy") and compareVoxels(with_mean, without, "occupancy")


def test_an_ndt_maps_occupancy_against_a_plain_maps(gpu):
    """K1: the mode is not looked at."""
    dims = (16, 16, 16)
    rays = cases.fan_rays(300, 2)
    ndt = make(dims, ("occupancy",), cls=GpuNdtMap)
    plain = make(dims, ("occupancy", "mean"))
    for gm in (ndt, plain):
        assert gm.integrateRays(rays) == len(rays)
    ev, ref = download(ndt, "occupancy"), download(plain, "occupancy")
    res, _, _ = check(ndt, plain, ev, ref, "occupancy", dims)
    assert res["layout_match"] == 1 and res["regions_compared"] == len(ref) and res["regions_missing"] == 0
    res, _, _ = check(ndt, plain, download(ndt, "mean"), download(plain, "mean"), "mean", dims)
    assert res["voxels_passed"] + res["voxels_failed"] == len(ref) * 4096
    assert run(ndt, plain, "covariance")[0]["layout_match"] == 0


# ---- 8. integration level, the mirrors --------------------------------------------------------------------------------
INTEGRATION_LAYERS = ("occupancy", "mean")  # bit-identical whatever the batch split: every voxel's events in ray order


def one_and_four(layers):
    """About 2 000 rays at 0.1 m into two maps: one call, and four calls."""
    rays = cases.fan_rays(2000, 4, reach=2.5)
    one, four = make((32, 32, 32), layers), make((32, 32, 32), layers)
    assert one.integrateRays(rays) == len(rays)
    for i in range(0, len(rays), 1000):
        assert four.integrateRays(rays[i:i + 1000]) == 1000
    return one, four


@pytest.fixture(scope="module")
def integrated(gpu):
    return one_and_four(INTEGRATION_LAYERS)


def test_traversal_differs_by_batch_split_within_a_tolerance(gpu):
    """The traversal layer folds a batch's fixed-point sums into the float once per batch (traversal_kernels.h), so one
    call and four calls differ in the last bits -- what a tolerance is for.  Without one the device fails exactly the
    voxels the host diff finds.  The bound: 2 000 rays of at most 0.1 * sqrt(3) m a voxel keep every sum below 512 m,
    where an ulp is 2^-15 m; four roundings on one side and one on the other are within 5 * 2^-16 < 1e-3 m."""
    one, four = one_and_four(("occupancy", "traversal"))
    ev, ref = download(four, "traversal"), download(one, "traversal")
    res, _, _ = check(four, one, ev, ref, "traversal", (32, 32, 32))
    assert res["voxels_failed"] == sum(int(np.count_nonzero(ev[k] != ref[k])) for k in ref)
    assert float(np.concatenate(list(ref.values())).view(np.float32).max()) < 512.0
    loose = Tolerance("traversal")
    configureTolerance(loose, "traversal", 1e-3)
    assert compareVoxels(four, one, "traversal", loose, kContinue)
    assert res["member_max_diff"][0] <= R.bits_of(1e-3)
    assert compare_maps(four, one, tolerances={"traversal": loose}).ok
    assert compare_maps(four, one, tolerances=False).ok == (res["voxels_failed"] == 0)


def test_one_call_equals_four_calls_on_every_layer(integrated):
    one, four = integrated
    regions = len(keys_of(one))
    assert regions >= 7
    for name in INTEGRATION_LAYERS:
        out = compareVoxels(four, one, name, flags=kContinue)
        assert out and out.voxels_passed == regions * 32768 and out.detail["regions_missing"] == 0, name
    verdict = compare_maps(four, one, tolerances=False)
    assert verdict.ok and sorted(verdict.voxels) == sorted(INTEGRATION_LAYERS) and all(verdict.layout.values())
    assert not verdict.layers_differ and verdict.eval_stats == verdict.ref_stats == occupancy_stats(one)
    occ = np.concatenate([b[:, 0] for b in download(one, "occupancy").values()]).view(np.float32)
    threshold = np.float32(one.map().occupancy_threshold_value)
    observed = occ != np.float32(np.inf)
    assert occupancy_stats(one) == (int(np.count_nonzero(observed & (occ >= threshold))),
                                    int(np.count_nonzero(observed & (occ < threshold))))
    assert occupancy_stats(one)[0] > 100 and occupancy_stats(one)[1] > 1000


def test_one_more_ray_fails_exactly_the_voxels_the_host_diff_finds(integrated):
    one, _ = integrated
    more = one.clone()
    assert more.integrateRays(np.array([[0.01, 0.02, 0.03], [1.93, -1.21, 0.77]])) == 2
    for name in INTEGRATION_LAYERS:
        ev, ref = download(more, name), download(one, name)
        res, listed, _ = check(more, one, ev, ref, name, (32, 32, 32))
        host = sum(int(np.count_nonzero(np.any(ev[k] != ref[k], axis=1))) for k in ref)
        # (the ray's end voxel in the mean layer; the voxels it crosses as well in occupancy)
        assert res["voxels_failed"] == host == len(listed) and host >= (1 if name == "mean" else 10), name
    # the mirrors: one message per failing member of the listed voxels, carrying what both maps hold
    for name, limit in (("occupancy", 5), ("mean", 1024)):
        logged = []
        out = compareVoxels(more, one, name, flags=kContinue, log=lambda sev, msg: logged.append((sev, msg)), max_logged=limit)
        assert not out and len(out.mismatches) == min(limit, out.detail["mismatch_count"]) > 0
        assert (name == "mean") or out.detail["mismatch_count"] > limit
        assert len(logged) == sum(bin(int(k["voxel"][3])).count("1") for k in out.mismatches)
        ev, ref = download(more, name), download(one, name)
        for sev, msg in logged:
            assert sev == Severity.kError and isinstance(msg, str) and int(msg.key["voxel"][3]) == 0
            region = tuple(int(v) for v in msg.key["region"])
            index = int(msg.key["voxel"][0]) + 32 * (int(msg.key["voxel"][1]) + 32 * int(msg.key["voxel"][2]))
            member = [n for n, _ in M.MEMBERS[name]].index(msg.member)
            have, expect = (int(np.asarray(v).reshape(1).view(np.uint32)[0]) for v in (msg.have, msg.expect))
            assert have == int(ev[region][index, member]) != expect == int(ref[region][index, member])
    # ohmcmp's run: the verdict per layer, with the tool's tolerances.  1e2 on occupancy forgives one more ray where both
    # maps had observed the voxel; a voxel the ray observed first is +inf against a number, which no finite eps forgives
    verdict = compare_maps(more, one)
    ev, ref = download(more, "occupancy"), download(one, "occupancy")
    first_seen = sum(int(np.count_nonzero((ref[k] == cases.INF) & (ev[k] != cases.INF))) for k in ref)
    changed = sum(int(np.count_nonzero(ev[k] != ref[k])) for k in ref)
    assert 0 < first_seen < changed
    assert not verdict.ok and not verdict.voxels["mean"] and verdict.voxels["occupancy"].voxels_failed == first_seen
    assert verdict.voxels["occupancy"].detail["member_max_diff"][0] == cases.INF
    strict = compare_maps(more, one, tolerances=False, stop_on_error=True)
    assert not strict.voxels["occupancy"] and strict.voxels["occupancy"].voxels_failed == 1
    tol = Tolerance("mean")
    configureTolerance(tol, "count", np.uint32(1))
    configureTolerance(tol, "coord", np.uint32(0xffffffff))
    assert compareVoxels(more, one, "mean", tol, kContinue)


# ---- 9. K6: both maps are only read ----------------------------------------------------------------------------------
def observe(gm, layers):
    stats = gm.cacheStats()
    listed = keys_of(gm)  # (the resident regions first, then the host store's)
    return dict(stats=stats, listed=listed, dirty=keys_of(gm, dirty_only=True), launched=gm.batchesLaunched(),
                data={name: {k: b.tobytes() for k, b in download(gm, name).items()} for name in layers})


def test_both_maps_are_only_read_and_a_host_store_is_read_in_place(gpu):
    dims, layers = cases.SMALL, ("occupancy", "mean")
    rays = cases.fan_rays(60, 9)
    ref = make(dims, layers)
    resident = make(dims, layers)
    spilling = make(dims, layers, region_capacity=16)
    spilling.setMemoryLimit(16 * spilling.cacheStats()["bytes_per_region"])
    spilling.setSpillToHost(True)
    extra = np.array([[0.0, 0.0, 0.0], [0.9, 1.1, -0.4]])
    assert ref.integrateRays(rays) == len(rays)
    for gm in (resident, spilling):
        for i in range(0, len(rays), 4):  # (two rays a batch: fewer regions than the limit)
            assert gm.integrateRays(rays[i:i + 4]) == 4
        assert gm.integrateRays(extra) == 2
        gm.wait()
    assert spilling.cacheStats()["regions_spilled"] > 0 and resident.cacheStats()["regions_spilled"] == 0
    before = {gm: observe(gm, layers) for gm in (ref, resident, spilling)}
    assert before[ref]["dirty"] and before[spilling]["dirty"]
    for name in layers:
        ev, rf = download(resident, name), download(ref, name)
        want = check(resident, ref, ev, rf, name, dims)
        assert want[0]["voxels_failed"] > 0
        got = run(spilling, ref, name)
        assert_equals_restatement(got, want)  # identical to the resident run
        assert_equals_restatement(run(ref, spilling, name), run(ref, resident, name))  # the store on the ref side
        assert_equals_restatement(run(spilling, ref, name, flags=0), run(resident, ref, name, flags=0))
    for gm in (ref, resident, spilling):
        assert observe(gm, layers) == before[gm]


# ---- 10. the device variant -------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("flags,capacity", [(kContinue, 64), (kContinue, 1), (kContinue, 0), (0, 4)])
def test_device_variant_equals_host_variant(lacking, flags, capacity):
    ge, gr, ev, ref, order, gone = lacking
    host = run(ge, gr, "occupancy", flags=flags, mismatch_capacity=capacity, missing_capacity=capacity)
    p = L.CompareParams()
    p.flags, p.layer_id = flags, L.LID_OCCUPANCY
    d_keys, d_missing, d_res = DeviceBuffer(10 * capacity), DeviceBuffer(6 * capacity), DeviceBuffer(C.sizeof(L.CompareResult))
    L.check(L.lib.ohmhip_map_compare_device(ge._handle, gr._handle, C.byref(p), capacity, d_keys.ptr if capacity else None,
                                            capacity, d_missing.ptr if capacity else None, d_res.ptr), "compare_device")
    L.check(L.lib.ohmhip_map_sync(gr._handle), "sync")
    raw = d_res.read(np.uint8, C.sizeof(L.CompareResult))
    res = L.CompareResult.from_buffer_copy(raw.tobytes())
    for name, _ in L.CompareResult._fields_:
        value = getattr(res, name)
        assert ([int(v) for v in value] if hasattr(value, "__len__") else int(value)) == host[0][name], name
    n_keys, n_missing = len(host[1]), len(host[2])
    assert d_keys.read(np.uint8, 10 * capacity)[:10 * n_keys].tobytes() == host[1].tobytes()
    assert np.array_equal(d_missing.read(np.int16, 3 * capacity)[:3 * n_missing].reshape(-1, 3), host[2])
    for buf in (d_keys, d_missing, d_res):
        buf.close()


# ---- 11. refusals with live maps --------------------------------------------------------------------------------------
def test_refusals(lacking):
    ge, gr, *_ = lacking

    def status(eval_=ge, ref=gr, flags=kContinue, layer_id=0, tol=0, mismatch=(0, None), missing=(0, None), keys=(None, 0)):
        p = L.CompareParams()
        p.flags, p.layer_id, p.tolerance_members = flags, layer_id, tol
        p.keys_xyz, p.key_count = keys
        res = L.CompareResult()
        return L.lib.ohmhip_map_compare(eval_._handle, ref._handle, C.byref(p), mismatch[0], mismatch[1], missing[0],
                                        missing[1], C.byref(res))

    assert status() == L.OK
    some = np.zeros((2, 3), dtype=np.int16)
    for kw in (dict(flags=2), dict(flags=0x80000001), dict(layer_id=-1), dict(layer_id=10), dict(tol=0b10),
               dict(layer_id=L.LID_MEAN, tol=0b100), dict(layer_id=L.LID_COVARIANCE, tol=1 << 6), dict(mismatch=(1, None)),
               dict(missing=(1, None)), dict(keys=(some.ctypes.data, 0)), dict(keys=(None, 2))):
        assert status(**kw) == L.ERR_INVALID_ARG, kw
    assert status(layer_id=L.LID_COVARIANCE, tol=0x3f) == L.OK  # (a layer neither map holds: layout_match 0)
    # K1: region voxel dimensions; resolution and origin are not looked at
    other_dims = make((8, 8, 4), ("occupancy",))
    assert status(eval_=other_dims) == L.ERR_INVALID_ARG and status(ref=other_dims) == L.ERR_INVALID_ARG
    moved = OccupancyMap(0.25, cases.SMALL, layers=("occupancy",))
    moved.setOrigin((0.5, -1.0, 2.0))
    assert status(eval_=GpuMap(moved)) == L.OK
    owner, part = make(cases.SMALL, ("occupancy",)), make(cases.SMALL, ("occupancy",))
    owner.setRegionOwnership(2, 0)
    part.setRegionPartition(RegionPartition(2, 1))
    for gm in (owner, part):
        assert status(eval_=gm) == L.ERR_UNSUPPORTED and status(ref=gm) == L.ERR_UNSUPPORTED
