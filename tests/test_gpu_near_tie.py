"""-m gpu: the device walkers on rays with one comparison inside the decision band of a shortcut (tests/near_tie_cases.py).

The integration walk replaces the reference's step-by-step fp64 walk with a fixed-point predictor (trusted when the
smallest candidate leads by more than fix_margin units) and a closed-form resume state at tile entries (stepsBefore:
trusted when x keeps 1e-5 from every integer).  Family A puts the critical gap at 0.02 ... 4 margins, early and late in a
tile, in the first and in a third or later segment; family B puts a tile entry 2e-8 ... 1e-4 step deltas from another
axis' step; family C holds exact ties at the same places.  tests/test_near_tie_ref.py shows that the CPU oracle walks
every one of these rays as exact rational arithmetic does, so bit-identity with the oracle is correctness here.

Besides the comparison with the oracle's maps, the voxels each batch should touch are rebuilt from the exact walker's
sequences: a wrong step shows as a missing and an extra voxel, and the message names the rays and gap cells behind it."""
import collections

import numpy as np
import pytest

import near_tie_cases as N
from ohm_amd import GpuMap, GpuTsdfMap, OccupancyMap, RayFlag
from parity import assert_parity, compare_maps, make_oracle
from rays_query_ref import rays_query

pytestmark = pytest.mark.gpu

CONFIG_NAMES = tuple(N.CONFIGS)
END_AS_FREE = int(RayFlag.kRfEndPointAsFree)


def _map(cfg, layers):
    config = N.CONFIGS[cfg]
    map_ = OccupancyMap(N.RES, config["region"], layers=layers)
    map_.setOrigin(N.to_metres(config["origin"]))
    return map_


def _describe(case, i):
    return "ray %d: family %s gap cell %s first %s positions %s entry %s gap %.3f margins = %.3g steps, %s -> %s" % (
        i, case["family"], case["gap_cell"], case["first_cell"], sorted(case["positions"]), case["entry"],
        float(case["gap_margins"]), float(case["gap_steps_b"]), case["start"], case["end"])


def _expected_counts(cases, flags):
    """{region: {local: [misses, hits, [ray indices]]}} from the exact walker's sequences: every voxel before the end
    voxel gets a miss; the end voxel a hit, or a miss with kRfEndPointAsFree (ohm/RayMapperOccupancy.cpp:209-239)."""
    out = collections.defaultdict(dict)
    for i, case in enumerate(cases):
        keys = case["keys"]
        for j, (region, local) in enumerate(keys):
            slot = out[region].setdefault(local, [0, 0, []])
            slot[1 if (j == len(keys) - 1 and not flags & END_AS_FREE) else 0] += 1
            slot[2].append(i)
    return out


def _assert_touched_voxels(cases, flags, map_, dims):
    expected = _expected_counts(cases, flags)
    assert sum(v[0] + v[1] for region in expected.values() for v in region.values()) == sum(len(c["keys"]) for c in cases)
    problems = []
    for region in sorted(set(expected) | set(map_.chunks)):
        block = map_.chunks.get(region)
        finite = set()
        if block is not None:
            for index in np.nonzero(np.isfinite(block["occupancy"]))[0]:
                index = int(index)
                finite.add((index % dims[0], index // dims[0] % dims[1], index // (dims[0] * dims[1])))
        want = expected.get(region, {})
        for local in sorted(set(want) - finite):
            problems.append("voxel %s %s untouched on the device, expected %d misses %d hits; %s" % (
                region, local, want[local][0], want[local][1], "; ".join(_describe(cases[i], i) for i in want[local][2][:3])))
        for local in sorted(finite - set(want)):
            near = [i for other, slot in want.items() if sum(abs(p - q) for p, q in zip(other, local)) == 1
                    for i in slot[2]]
            problems.append("voxel %s %s touched on the device, on no exact sequence; rays through its neighbours: %s" % (
                region, local, "; ".join(_describe(cases[i], i) for i in sorted(set(near))[:4])))
    assert not problems, "%d voxels differ from the exact walker:\n%s" % (len(problems), "\n".join(problems[:12]))


def _integrate_and_check(cfg, family, layers, flags, batch=None):
    cases, _ = N.generate(family, cfg)
    rays = N.rays_of(cases)
    map_ = _map(cfg, layers)
    gm = GpuMap(map_)
    om = make_oracle(map_)
    step = 2 * (batch or len(cases))
    for first in range(0, rays.shape[0], step):
        part = rays[first:first + step]
        assert gm.integrateRays(part, ray_update_flags=flags) == part.shape[0]
        om.integrate_occupancy(part, flags=flags)
    gm.syncVoxels()
    visits = gm.stats()["voxel_visits"]
    # the exact sequences first: their message says which rays and gap cells are behind a difference
    _assert_touched_voxels(cases, flags, map_, N.CONFIGS[cfg]["region"])
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
    assert visits == om.visit_count(), (visits, om.visit_count())
    walked = sum(len(c["keys"]) for c in cases)      # a miss per voxel before the end voxel; a hit or a miss there
    assert visits == walked, (visits, walked)
    gm.close()


@pytest.mark.parametrize("flags", [0, END_AS_FREE])
@pytest.mark.parametrize("layers", [("occupancy",), ("occupancy", "mean")])
@pytest.mark.parametrize("cfg", CONFIG_NAMES)
def test_occupancy_integration_on_near_ties(gpu, cfg, layers, flags):
    for family in "ABC":
        _integrate_and_check(cfg, family, layers, flags)


@pytest.mark.parametrize("cfg", CONFIG_NAMES)
def test_occupancy_integration_on_near_ties_in_batches_of_64(gpu, cfg):
    """The same rays land in other chunks and lanes of the walk kernel."""
    _integrate_and_check(cfg, "A", ("occupancy", "mean"), 0, batch=64)


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("cfg", ["r32", "r64"])
def test_tsdf_integration_on_near_ties(gpu, cfg, family):
    """dropoff_epsilon > 0: every visited voxel changes, so every visit goes through the event list and the ordered
    replay, whose resume state is stepsBefore() again (replay_kernels.h)."""
    cases, _ = N.generate(family, cfg)
    rays = N.rays_of(cases)
    map_ = _map(cfg, ("tsdf",))
    gm = GpuTsdfMap(map_, default_truncation_distance=0.25, dropoff_epsilon=0.05)
    om = make_oracle(map_)
    opts = gm.tsdf_options
    om.set_tsdf(max_weight=opts[0], trunc=opts[1], dropoff=opts[2], sparsity=opts[3])
    assert gm.integrateRays(rays) == rays.shape[0]
    om.integrate_tsdf(rays)
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["tsdf"], exact_float=True))
    assert gm.stats()["voxel_visits"] == om.visit_count()
    gm.close()


@pytest.mark.parametrize("family", ["A", "B"])
def test_traversal_layer_on_near_ties(gpu, family):
    """Occupancy bit exact; traversal at the tolerance tests/test_gpu_secondary.py holds that layer to."""
    from test_gpu_secondary import _check as check_secondary
    cases, _ = N.generate(family, "r32")
    rays = N.rays_of(cases)
    layers = ("occupancy", "traversal")
    map_ = _map("r32", layers)
    gm = GpuMap(map_)
    om = make_oracle(map_)
    assert gm.integrateRays(rays) == rays.shape[0]
    om.integrate_occupancy(rays)
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy"], exact_float=True))
    check_secondary(om, map_, layers)
    gm.close()


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("cfg", ["r32", "r64"])
def test_line_keys_equal_the_exact_walker_on_near_ties(gpu, cfg, family):
    cases, _ = N.generate(family, cfg)
    lines = N.rays_of(cases).reshape(-1, 6)
    gm = GpuMap(_map(cfg, ("occupancy",)))
    longest = max(len(c["keys"]) for c in cases)
    regions, voxels, counts = gm.lineKeys(lines, max_keys_per_line=longest + 2)
    for i, case in enumerate(cases):
        keys = case["keys"]
        assert counts[i] == len(keys), _describe(case, i)
        got = [(tuple(int(v) for v in regions[i, j]), tuple(int(v) for v in voxels[i, j])) for j in range(len(keys))]
        assert got == keys, _describe(case, i)
    gm.close()


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("cfg", ["r32", "r64"])
def test_rays_query_on_near_ties(gpu, cfg, family):
    """One occupied voxel per ray, the one the critical step leads into: a query that takes the other axis there walks
    past it.  Held to tests/rays_query_ref.py, which walks with the oracle."""
    cases, _ = N.generate(family, cfg)
    map_ = _map(cfg, ("occupancy",))
    gm = GpuMap(map_)
    om = make_oracle(map_)
    targets = sorted({case["keys"][case["decision"] + 1] for case in cases})
    centres = np.array([om.voxel_centre(region, local) for region, local in targets], dtype=np.float64)
    hits = np.repeat(centres, 2, axis=0)      # zero-length rays: a sample in the voxel and nothing else
    assert gm.integrateRays(hits) == hits.shape[0]
    om.integrate_occupancy(hits)
    query = N.rays_of(cases)
    got = gm.raysQuery(query)
    want, _ = rays_query(om, query, map_.occupancy_threshold_value, 1.0, map_.ray_filter)
    for name, g, w in zip(("ranges", "volumes", "types", "regions", "locals"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (name, bad.size, [_describe(cases[i], i) for i in bad[:3]], g[bad[:3]], w[bad[:3]])
    occupied = int((np.asarray(got[2]) == 1).sum())
    assert occupied == len(cases), occupied     # every ray ends at an occupied voxel: its own or an earlier one
    gm.close()
