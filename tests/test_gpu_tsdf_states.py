"""-m gpu: the device's TSDF voxel update on the constructed sheets of tests/tsdf_cases.py, held bit for bit to the exact
model (tests/tsdf_ref.py) and to the CPU oracle -- the whole region after every call, on the uint32 views of weight and
distance.  There is no tolerance.  One exception: where the model's value is NaN the device's must be a NaN, of any
payload (the reference does not define it); such values come from the planted NaN and infinite rows only.

A sheet plants (weight, distance) states by uploading a host map, and every state is read back from the device itself
(ohmhip_map_read_regions into fresh 0xa5-filled buffers: syncVoxels copies only regions marked as modified).  Coalescing
is off, so a call is a device batch.  Every sheet is fed three ways, and all three must give the model's answer: call
by call with a read after every call (each state judged), one call per option segment, and call by call without reads.
Options change between calls through GpuTsdfMap's own setters; the oracle gets the same change between the same calls.

The sites (tsdf_cases.SITES) are the places the device applies a free-space count, or must not: the device may apply a
voxel's free-space visits of a batch as one addition only where that is what the reference's n updates give
(tsdf_ref.counted), and which voxels those are is decided by a persistent mask that uploads, re-admissions from the host
store and option changes all have to keep true to the stored state.  test_tsdf_ref.py (CPU) asserts that every sheet
holds voxels on both sides of that line, which edges the sheets reach, and that each mutant of the model -- `count_once`
is the device's shortcut with no mask at all -- is caught on every site."""
import numpy as np
import pytest

import tsdf_cases
from ohm_amd import GpuTsdfMap, OccupancyMap
from test_gpu_mean_states import read_device
from tsdf_cases import REGION, RES, batches, differing, refusals, set_options, state_of

pytestmark = pytest.mark.gpu

_SHEETS = {}
SPILL_POOL = 4                                                  # regions the `spill` site's pool may hold
# one short ray in each of the regions (5, 0, 0) ... (8, 0, 0): together they fill the pool
FAR = np.array([[3.2 * r + dx, 0.05, 0.05] for r in range(5, 5 + SPILL_POOL) for dx in (0.05, 0.3)])


def sheets_of(site):
    if site not in _SHEETS:
        _SHEETS[site] = tsdf_cases.build(sites=(site,))
    return _SHEETS[site]


def device_map(sheet):
    map_ = OccupancyMap(RES, (sheet.dim,) * 3, layers=("tsdf",))
    map_.chunks[REGION] = {"tsdf": sheet.tile()}
    o = sheet.calls[0].opts
    gm = GpuTsdfMap(map_, max_weight=float(o.max_weight), default_truncation_distance=float(o.trunc),
                    dropoff_epsilon=float(o.dropoff), sparsity_compensation_factor=float(o.sparsity),
                    region_capacity=SPILL_POOL if sheet.site == "spill" else 0)
    gm.setBatchCoalescing(0)
    if sheet.site == "spill":
        gm.setMemoryLimit(SPILL_POOL * gm.cacheStats()["bytes_per_region"])     # (the limit bites when the pool would grow)
        gm.setSpillToHost(True)
    return map_, gm


def apply_options(gm, o, whole):
    if whole:
        gm.tsdf_options = (float(o.max_weight), float(o.trunc), float(o.dropoff), float(o.sparsity))
        return
    gm.setMaxWeight(float(o.max_weight))
    gm.setDropoffEpsilon(float(o.dropoff))
    gm.setSparsityCompensationFactor(float(o.sparsity))


def feed(sheet, merged, judge=None):
    """The sheet through a device map and an oracle map side by side; judge(k, device state, oracle state) after call k
    where given.  Returns the final (device, oracle) states of region (0, 0, 0)."""
    map_, gm = device_map(sheet)
    om = tsdf_cases.make_oracle(sheet)
    before = read_device(map_, gm)                                # the upload round trip keeps every planted bit
    assert set(before) == {REGION}
    assert np.array_equal(before[REGION]["tsdf"].view(np.uint32), sheet.tile().view(np.uint32)), sheet.name
    refuse = refusals(sheet)
    segment = 0
    for k, (o, seg, rays) in enumerate(batches(sheet, merged)):
        if sheet.site == "spill":
            # other regions fill the pool: region (0, 0, 0) waits in the host store while the options change
            assert gm.integrateRays(FAR) == FAR.shape[0]
            om.integrate_tsdf(FAR)
            assert gm.cacheStats()["regions_spilled"] >= 1
        if seg != segment and seg in refuse:
            # a new truncation distance on a populated map is refused, not approximated; the map goes on as it was
            gm.setDefaultTruncationDistance(refuse[seg])
            with pytest.raises(Exception):
                gm.integrateRays(rays)
            gm.setDefaultTruncationDistance(float(o.trunc))
        segment = seg
        apply_options(gm, o, whole=sheet.variant == "trunc_refused")
        set_options(om, o)
        assert gm.integrateRays(rays) == rays.shape[0]
        om.integrate_tsdf(rays)
        if judge:
            judge(k, state_of(read_device(map_, gm)[REGION]["tsdf"]), state_of(om.region_layer(REGION, "tsdf")))
    final = state_of(read_device(map_, gm)[REGION]["tsdf"])
    if sheet.site == "spill":
        st = gm.cacheStats()
        assert st["evictions"] > 0 and st["readmissions"] > 0, st
    gm.close()
    return final, state_of(om.region_layer(REGION, "tsdf"))


def report(sheet, what, model, got):
    bad = differing(model, got)
    if len(bad) == 0:
        return ""
    v = int(bad[0])
    return "%s, %s: %d voxels differ from the model; first %s holds (%r, %r), model (%r, %r), planted (%r, %r)\n" % (
        sheet.name, what, len(bad), sheet.geo.local(v), got[0][v], got[1][v], model[0][v], model[1][v], sheet.w0[v],
        sheet.d0[v])


@pytest.mark.parametrize("site", tsdf_cases.SITES)
def test_device_tsdf_holds_to_the_model_and_the_oracle(gpu, site):
    """Call by call, the whole region judged after every call."""
    failures = ""
    for sheet in sheets_of(site):
        def judge(k, device, oracle, sheet=sheet):
            nonlocal failures
            assert len(differing(sheet.states[k], oracle)) == 0, (sheet.name, k, "oracle differs from the model")
            failures += report(sheet, "after call %d" % k, sheet.states[k], device)
        feed(sheet, merged=False, judge=judge)
    assert not failures, "\n" + failures


@pytest.mark.parametrize("site", tsdf_cases.SITES)
def test_batching_does_not_change_a_bit(gpu, site):
    """One call per option segment, and call by call without reads in between: both end where the model ends."""
    failures = ""
    for sheet in sheets_of(site):
        for merged in (True, False):
            device, oracle = feed(sheet, merged)
            assert len(differing(sheet.states[-1], oracle)) == 0, (sheet.name, merged, "oracle differs from the model")
            failures += report(sheet, "one call per segment" if merged else "call by call, no reads", sheet.states[-1],
                               device)
    assert not failures, "\n" + failures
