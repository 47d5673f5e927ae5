"""-m gpu: the device's occupancy log-odds on the constructed sheets of tests/occupancy_cases.py, held bit for bit to
the exact model (tests/occupancy_ref.py) -- the whole occupancy block of every region either side knows, after every
call, on uint32 views.  There is no tolerance; a region one side does not know counts as never observed.

A sheet plants its states by uploading a host map, and every state is read back from the device itself
(ohmhip_map_read_regions into fresh 0xa5-filled buffers).  Coalescing is off, so a call is a device batch, and the map
is created under the sheet's pinned chunk size (OHMHIP_CHUNK_SEGMENTS = OHMHIP_MIN_CHUNK_SEGMENTS).  The configuration
of every call is set on the host map before the call, as an application would.  Every sheet is fed twice: with a read
after every call (each state judged) and with none; both end on the model's final state.  The CPU oracle is fed the
same calls in the same run: occupancy and, where the map has one, the mean layer must equal it bit for bit after
every judged call.

The sites (occupancy_cases.SITES) are the places the log-odds are written; test_occupancy_ref.py (CPU) asserts from the
model's own segment and sample counts that each site's sheets meet the conditions that select its path:
  walk      occupancy only, every region in one chunk: k_region_walk's epilogue counts and its inline sample replay
  lists     occupancy only, every region in several chunks: k_apply_lists, sample part and count part
  dense     occupancy only, more samples in a region than the walk stages in LDS: k_flagged_events
  mean      occupancy + mean: k_apply_hits and k_apply_counts, regions in one chunk (counts applied by the walk) and in
            several
  odd       17^3, 18 x 17 x 17 and 15 x 9 x 7 regions: the scalar branches, with and without a mean layer
  half      16^3 regions: the half-size walk shape
  stop      kRfStopOnFirstOccupied: k_stop_replay, with and without a mean layer
  tiled     48^3 regions cut into z slabs
  spill     a pool of 4 regions with spill to host: planted values survive eviction and re-admission, NaN payload
            included
  maxchunk  the library's largest chunk: 8192 and 8193 rays of one call through one voxel, counts past 2^15 and 2^16;
            first under kRfExcludeSample (counts alone), then with more samples than the walk stages in LDS"""
import numpy as np
import pytest

import occupancy_cases as OC
import occupancy_ref as O
from ohm_amd import GpuMap, OccupancyMap
from test_gpu_mean_states import read_device
from traversal_cases import point, rays_array

pytestmark = pytest.mark.gpu

SPILL_POOL = 4                                                  # regions the `spill` site's pool may hold
F = np.float32


def far_rays(mp):
    """One short ray in each of the regions (5, 0, 0) ... (8, 0, 0): together they fill the spill site's pool."""
    out = []
    for r in range(5, 5 + SPILL_POOL):
        g = [r * mp.dim[0] + 3, 3, 3]
        out.append((point(g, (0.5, 0.5, 0.5), mp), point([g[0] + 1, 3, 3], (0.5, 0.5, 0.5), mp)))
    return rays_array(out)


def calls_of(sheet, site):
    """The sheet's calls; the spill site's far rays go before each of them (the model gets them too)."""
    if site != "spill":
        return list(sheet.calls), list(range(len(sheet.calls)))
    far, calls = far_rays(sheet.mp), []
    for call in sheet.calls:
        calls += [O.Call(far, 0, call.cfg), call]
    return calls, list(range(1, len(calls), 2))


def model_states(sheet, site):
    if site != "spill":
        return sheet.states
    calls, own = calls_of(sheet, site)
    states = O.replay(sheet.planted, calls, sheet.mp)
    return [states[k] for k in own]


def set_config(map_, cfg):
    map_.hit_value, map_.miss_value = float(cfg.hit), float(cfg.miss)
    map_.occupancy_threshold_value = F(cfg.threshold)
    map_.min_voxel_value, map_.max_voxel_value = F(cfg.min_value), F(cfg.max_value)
    map_.saturate_at_min_value, map_.saturate_at_max_value = cfg.sat_min, cfg.sat_max


def device_map(sheet, site, monkeypatch):
    mp = sheet.mp
    monkeypatch.setenv("OHMHIP_CHUNK_SEGMENTS", str(sheet.chunk))          # both are read at map creation
    monkeypatch.setenv("OHMHIP_MIN_CHUNK_SEGMENTS", str(sheet.chunk))
    map_ = OccupancyMap(mp.res, mp.dim, layers=sheet.layers)
    for region, tile in sheet.planted.items():
        map_.chunks[region] = {"occupancy": tile.copy()}
        if "mean" in sheet.layers:
            map_.chunks[region]["mean"] = np.zeros(2 * mp.volume, dtype=np.uint32)
    set_config(map_, sheet.calls[0].cfg)
    gm = GpuMap(map_, region_capacity=SPILL_POOL if site == "spill" else 64)
    gm.setBatchCoalescing(0)
    if site == "spill":
        gm.setMemoryLimit(SPILL_POOL * gm.cacheStats()["bytes_per_region"])   # (bites when the pool would grow)
        gm.setSpillToHost(True)
    return map_, gm, OC.make_oracle(sheet)


def differing(sheet, state, device, name="occupancy"):
    """[(region, voxel index, device bits, model bits)] over every region either side knows."""
    out = []
    unknown = np.full(sheet.mp.volume, np.inf, dtype=F)
    for region in sorted(set(state) | set(device)):
        got = device[region][name] if region in device else unknown
        want = state.get(region, unknown)
        for vi in np.flatnonzero(got.view(np.uint32) != want.view(np.uint32)):
            out.append((region, int(vi), int(got.view(np.uint32)[vi]), int(want.view(np.uint32)[vi])))
    return out


def report(sheet, k, what, bad, events=None):
    if not bad:
        return ""
    region, vi, got, want = bad[0]
    pattern = "?" if events is None else O.patterns_of(events).get((region, vi), "")
    as_float = lambda b: float(np.array([b], dtype=np.uint32).view(F)[0])  # noqa: E731
    return ("%s, call %d (%s): %d voxels differ from the model; first: region %s voxel %s holds 0x%08x (%r), model "
            "0x%08x (%r); its events in this call: %r\n" % (sheet.name, k, what, len(bad), region, sheet.mp.local(vi),
                                                            got, as_float(got), want, as_float(want), pattern))


def check_oracle(sheet, k, device, om):
    theirs = om.chunks()
    for region, layers in theirs.items():
        for name in sheet.layers:
            assert region in device, (sheet.name, k, region, "missing on the device")
            assert np.array_equal(device[region][name].view(np.uint32), layers[name].view(np.uint32)), (
                sheet.name, k, region, name, "differs from the oracle")


def feed(sheet, site, monkeypatch, judged):
    """The sheet through a device map and an oracle map side by side.  Returns the failure text."""
    map_, gm, om = device_map(sheet, site, monkeypatch)
    before = read_device(map_, gm)                                # the upload round trip keeps every planted bit
    assert set(before) == set(sheet.planted)
    for region, tile in sheet.planted.items():
        assert np.array_equal(before[region]["occupancy"].view(np.uint32), tile.view(np.uint32)), sheet.name
    calls, own = calls_of(sheet, site)
    states = model_states(sheet, site)
    failures = ""
    for k, call in enumerate(calls):
        set_config(map_, call.cfg)
        OC.set_oracle_config(om, call.cfg)
        assert gm.integrateRays(call.rays, None, None, call.flags) == call.rays.shape[0]
        om.integrate_occupancy(call.rays, flags=call.flags)
        if site == "spill" and k not in own:
            assert gm.cacheStats()["regions_spilled"] >= 1 or not (k or sheet.planted)
        last = k == len(calls) - 1
        if k in own and (judged or last):
            i = own.index(k)
            device = read_device(map_, gm)
            what = "read after every call" if judged else "no reads before the last"
            failures += report(sheet, i, what, differing(sheet, states[i], device), sheet.events[i])
            if not failures:
                check_oracle(sheet, i, device, om)
    if site == "spill":
        st = gm.cacheStats()
        assert st["evictions"] > 0 and st["readmissions"] > 0, st
    gm.close()
    return failures


@pytest.mark.parametrize("site", OC.SITES)
def test_device_occupancy_holds_to_the_model(gpu, site, monkeypatch):
    """Call by call, every region judged after every call."""
    failures = "".join(feed(sheet, site, monkeypatch, True) for sheet in OC.build(site))
    assert not failures, "\n" + failures


@pytest.mark.parametrize("site", OC.SITES)
def test_reads_between_the_calls_do_not_change_a_bit(gpu, site, monkeypatch):
    """Call by call without reads in between: the same final state."""
    failures = "".join(feed(sheet, site, monkeypatch, False) for sheet in OC.build(site))
    assert not failures, "\n" + failures
