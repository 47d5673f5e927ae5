"""-m gpu: the device's traversal layer on the constructed sheets of tests/traversal_cases.py, held bit for bit to the
exact fixed-point model (tests/traversal_ref.py) -- every touched region's whole block after every call, on uint32
views.  There is no tolerance.

A sheet plants traversal (and, for `stop`, occupancy) tiles by uploading a host map, and every state is read back from
the device itself (ohmhip_map_read_regions into fresh 0xa5-filled buffers: syncVoxels copies only regions marked as
modified).  Coalescing is off, so a call is a device batch.  Every sheet is fed call by call with a read after every
call (each state judged) and call by call without reads; both end on the model's final state.  In the same run
occupancy and, where present, the mean stay bit exact against the CPU oracle fed the same calls (the NDT sites: the mean
only -- NDT's log-odds go through exp() and are held to their own model by test_gpu_ndt_states.py).

The sites (traversal_cases.SITES) are the places the layer is written:
  direct  occupancy + traversal, one chunk per region: k_region_traversal's tile flush, folded by k_apply_counts for a
          region whose counts the walk applied itself
  chunks  the same with several chunks per region: carries and flushes of several tiles into one accumulator
  mean    occupancy + mean + traversal: shares from k_apply_hits, then the fold
  stop    kRfStopOnFirstOccupied: shares from k_stop_replay<true>, the fold by the skip_masked k_apply_counts
  ndt     GpuNdtMap with a traversal layer: shares from k_replay_ndt, then the fold
  rewalk  ndt with an event list of 64 entries: the repeated walk must not add the visits twice
  tiled   48^3 regions cut into z slabs: one region's voxels in several tiles
  spill   a pool of 4 regions with spill to host: the float layer survives eviction and re-admission, the per-batch
          accumulator does not leak
test_traversal_ref.py (CPU) asserts which edges the sheets reach, the model's and the oracle's bounds against the exact
sum, and that each mutant of the model is caught on every site it applies to.

Each test also prints, as a record and not an assertion, the site's largest |device - oracle| over the sum of the two
derived bounds (the model's and the oracle's, traversal_ref), with the ulp taken at the largest of the two final
values and the model's intermediate ones."""
import numpy as np
import pytest

import traversal_cases as TC
import traversal_ref as T
from ohm_amd import GpuMap, GpuNdtMap, OccupancyMap
from test_gpu_mean_states import read_device
from traversal_ref import F

pytestmark = pytest.mark.gpu

SPILL_POOL = 4                                                  # regions the `spill` site's pool may hold
NDT_SITES = ("ndt", "rewalk")
LAYERS = {"direct": ("occupancy", "traversal"), "chunks": ("occupancy", "traversal"),
          "mean": ("occupancy", "mean", "traversal"), "stop": ("occupancy", "traversal"),
          "ndt": ("occupancy", "traversal"), "rewalk": ("occupancy", "traversal"),
          "tiled": ("occupancy", "traversal"), "spill": ("occupancy", "traversal")}


def far_rays(mp):
    """One short ray in each of the regions (5, 0, 0) ... (8, 0, 0): together they fill the spill site's pool."""
    out = []
    for r in range(5, 5 + SPILL_POOL):
        g = [r * mp.dim[0] + 3, 3, 3]
        out.append((TC.point(g, (0.5, 0.5, 0.5), mp), TC.point([g[0] + 2, 3, 3], (0.5, 0.5, 0.5), mp)))
    return TC.rays_array(out)


def device_map(sheet, site):
    mp = sheet.mp
    map_ = OccupancyMap(mp.res, mp.dim, layers=LAYERS[site])
    for region, tile in sheet.planted.items():
        map_.chunks[region] = {"occupancy": TC.occupancy_tile(sheet, region).copy(), "traversal": tile.copy()}
    capacity = SPILL_POOL if site == "spill" else 0
    gm = GpuNdtMap(map_, region_capacity=capacity) if site in NDT_SITES else GpuMap(map_, region_capacity=capacity)
    gm.setBatchCoalescing(0)
    if site == "spill":
        gm.setMemoryLimit(SPILL_POOL * gm.cacheStats()["bytes_per_region"])   # (bites when the pool would grow)
        gm.setSpillToHost(True)
    ndt = dict(adaptation_rate=gm.adaptation_rate) if site in NDT_SITES else None
    om = TC.make_oracle(sheet, list(map_.layers), ndt)
    return map_, gm, om


def integrate(gm, om, site, rays, flags):
    assert gm.integrateRays(rays, None, None, flags) == rays.shape[0]
    if site in NDT_SITES:
        om.integrate_ndt(rays, flags=flags)
    else:
        om.integrate_occupancy(rays, flags=flags)


def differing(sheet, state, device):
    """[(region, voxel, device value, model value)] over every region either side knows (an unknown one is cleared)."""
    out = []
    zero = np.zeros(sheet.mp.volume, dtype=F)
    for region in sorted(set(state) | set(device)):
        got = device[region]["traversal"] if region in device else zero
        want = state.get(region, zero)
        for vi in np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)):
            out.append((region, sheet.mp.local(int(vi)), float(got[vi]), float(want[vi])))
    return out


def report(sheet, what, bad):
    if not bad:
        return ""
    region, local, got, want = bad[0]
    return "%s, %s: %d voxels differ from the model; first %s %s holds %r (%s), model %r (%s)\n" % (
        sheet.name, what, len(bad), region, local, got, np.float32(got).view(np.uint32), want,
        np.float32(want).view(np.uint32))


def oracle_exact_layers(site):
    return ["mean"] if site in NDT_SITES else [n for n in LAYERS[site] if n != "traversal"]


def check_oracle(sheet, site, device, om, what):
    theirs = om.chunks()
    for region, layers in theirs.items():
        for name in oracle_exact_layers(site):
            assert region in device, (sheet.name, what, region, "missing on the device")
            assert np.array_equal(device[region][name].view(np.uint32), layers[name].view(np.uint32)), (
                sheet.name, what, region, name, "differs from the oracle")
    return theirs


def feed(sheet, site, judge=None):
    """The sheet through a device map and an oracle map side by side; judge(k, device regions) after call k where
    given.  Returns the final device regions and the oracle's."""
    map_, gm, om = device_map(sheet, site)
    before = read_device(map_, gm)                                # the upload round trip keeps every planted bit
    assert set(before) == set(sheet.planted)
    for region, tile in sheet.planted.items():
        assert np.array_equal(before[region]["traversal"].view(np.uint32), tile.view(np.uint32)), sheet.name
        assert np.array_equal(before[region]["occupancy"].view(np.uint32),
                              TC.occupancy_tile(sheet, region).view(np.uint32)), sheet.name
    far = far_rays(sheet.mp) if site == "spill" else None
    for k, call in enumerate(sheet.calls):
        if site == "spill":
            # other regions fill the pool: the sheet's regions wait in the host store between its calls
            integrate(gm, om, site, far, 0)
            assert gm.cacheStats()["regions_spilled"] >= 1 or not (k or sheet.planted)   # (nothing to evict yet)
        integrate(gm, om, site, call.rays, call.flags)
        if judge:
            judge(k, read_device(map_, gm))
    final = read_device(map_, gm)
    if site == "spill":
        st = gm.cacheStats()
        assert st["evictions"] > 0 and st["readmissions"] > 0, st
    gm.close()
    theirs = check_oracle(sheet, site, final, om, "at the end")
    return final, theirs


def model_states(sheet, site):
    """The sheet's states; the spill site's far rays add their own (constant) regions, which the model gets too."""
    if site != "spill":
        return sheet.states
    far = T.Call(far_rays(sheet.mp), 0)
    calls = []
    for call in sheet.calls:
        calls += [far, call]
    return T.replay(sheet.planted, calls, sheet.mp)[1::2]


def oracle_gap(sheet, device, theirs):
    """Largest |device - oracle| over the sum of the two derived bounds (a record, not a check)."""
    visits, shares, occupancy = {}, {}, sheet.occupancy()
    for call in sheet.calls:
        for a in T.cpu_adds(call, sheet.mp, occupancy)[0]:
            into = shares if a.share else visits
            into[(a.region, a.vi)] = into.get((a.region, a.vi), 0) + 1
    unit_bits, b, worst = T.traversal_unit_bits(sheet.mp.res), len(sheet.calls), 0.0
    for region, vi in set(visits) | set(shares):
        if region in device and region in theirs:
            n, s = visits.get((region, vi), 0), shares.get((region, vi), 0)
            ours, ref = float(device[region]["traversal"][vi]), float(theirs[region]["traversal"][vi])
            peak = max(d.get((region, vi), {}).get("peak", 0.0) for d in sheet.details)
            ulp = T.ulp32(max(abs(ours), abs(ref), peak))
            bound = n * 2.0 ** -(unit_bits + 1) + (b + s) * ulp / 2 + (n + s) * ulp / 2
            worst = max(worst, abs(ours - ref) / bound)
    return worst


@pytest.mark.parametrize("site", TC.SITES)
def test_device_traversal_holds_to_the_model(gpu, site, monkeypatch, capsys):
    """Call by call, every region judged after every call."""
    if site == "rewalk":
        monkeypatch.setenv("OHMHIP_EVENT_LIMIT", "64")           # read at map creation: every batch overflows the list
    failures, worst = "", 0.0
    for sheet in TC.build(site):
        states = model_states(sheet, site)

        def judge(k, device, sheet=sheet, states=states):
            nonlocal failures
            failures += report(sheet, "after call %d" % k, differing(sheet, states[k], device))
        final, theirs = feed(sheet, site, judge)
        worst = max(worst, oracle_gap(sheet, final, theirs))
    with capsys.disabled():
        print("\n%-7s largest |device - oracle| / bound: %.3f" % (site, worst))
    assert not failures, "\n" + failures


@pytest.mark.parametrize("site", TC.SITES)
def test_reads_between_the_calls_do_not_change_a_bit(gpu, site, monkeypatch):
    """Call by call without reads in between: the same final state."""
    if site == "rewalk":
        monkeypatch.setenv("OHMHIP_EVENT_LIMIT", "64")
    failures = ""
    for sheet in TC.build(site):
        unread, _ = feed(sheet, site)
        failures += report(sheet, "call by call, no reads", differing(sheet, model_states(sheet, site)[-1], unread))
    assert not failures, "\n" + failures
