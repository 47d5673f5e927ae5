"""-m gpu: the per-region ordering of a plain occupancy batch's sample keys (k_sort_region_hits: placement by bucket
voxel >> 5 and a rank inside the bucket; the bitonic network where buckets are crowded; the device-wide sort above 8192
samples in a region).

Every case feeds the same calls to a device map and to the CPU oracle (oracle.oracle.OracleMap) and compares every
region either side knows bit for bit (uint32 views).  Coalescing is off (a call is a device batch), the maps are 32^3 at
0.1 m, the rays are a few voxels long and start inside the region they end in unless a case says otherwise.
GpuMap.orderCounts() tells the two orderings apart, so that the network cannot pass for the ranked path or the other
way round.

Every case is ORDER-SENSITIVE, and says so itself: in its setup the oracle is fed the same calls with the rays of every
call in reversed order and must end with at least one voxel that differs from the forward order (order_sensitive()).
A sample order that is wrong therefore shows.  What makes the order matter: several rays end in voxels that other rays
of the same call cross (hit and miss adjustments do not commute in float32 once the voxel holds a value, and not at all
at the clamps), and every case makes two or three calls, so that values sit between the clamps.

A region's voxel index is x + 32 * (y + 32 * z): a bucket of the ranked ordering is one x-row."""
import numpy as np
import pytest

from ohm_amd import GpuMap, OccupancyMap
from parity import make_oracle
from test_gpu_mean_states import read_device

pytestmark = pytest.mark.gpu

EDGE = 3.2                                    # a 32^3 region at 0.1 m
LOW = np.array([-1.6, -1.6, -1.6])            # low corner of region (0, 0, 0): the map's origin is the region's centre
RES = 0.1


def pairs(starts, ends):
    ends = np.asarray(ends, dtype=np.float64)
    out = np.empty((2 * ends.shape[0], 3), dtype=np.float64)
    out[0::2] = starts
    out[1::2] = ends
    return out


def reverse_rays(rays):
    return np.ascontiguousarray(rays.reshape(-1, 2, 3)[::-1]).reshape(-1, 3)


def samples_per_region(rays):
    regions, counts = np.unique(np.floor((rays[1::2] - LOW) / EDGE).astype(int), axis=0, return_counts=True)
    return {tuple(int(v) for v in r): int(c) for r, c in zip(regions, counts)}


def new_map():
    return OccupancyMap(RES, (32, 32, 32), layers=("occupancy",))


def run_oracle(calls, reverse=False):
    om = make_oracle(new_map())
    for rays in calls:
        om.integrate_occupancy(reverse_rays(rays) if reverse else rays)
    return om.chunks(["occupancy"])


def order_sensitive(calls):
    """The oracle fed `calls` with every call's rays reversed ends with a voxel that differs from the forward order."""
    forward, backward = run_oracle(calls), run_oracle(calls, reverse=True)
    assert set(forward) == set(backward)
    return any(np.any(forward[r]["occupancy"].view(np.uint32) != backward[r]["occupancy"].view(np.uint32))
               for r in forward)


def run_case(monkeypatch, calls, early=0, region_capacity=64, back_to_back=False, env=()):
    """`calls` through a device map and the oracle; every region either side knows bit for bit.  Returns orderCounts()
    and pipelineCounts() after every call."""
    assert order_sensitive(calls), "the case tests nothing: the reversed oracle agrees with the forward one"
    monkeypatch.setenv("OHMHIP_EARLY_BIN", str(early))
    for name, value in env:
        monkeypatch.setenv(name, str(value))
    map_ = new_map()
    gm = GpuMap(map_, region_capacity=region_capacity)
    gm.setBatchCoalescing(0)
    om = make_oracle(map_)
    order, pipeline = [], []
    for rays in calls:
        gm.integrateRays(rays)
        pipeline.append(gm.pipelineCounts())
        if not back_to_back:
            order.append(gm.orderCounts())
    order.append(gm.orderCounts())
    for rays in calls:
        om.integrate_occupancy(rays)
    device = read_device(map_, gm)
    oracle = om.chunks(["occupancy"])
    gm.close()
    unknown = np.full(map_.regionVoxelVolume(), np.inf, dtype=np.float32)
    bad = []
    for region in sorted(set(device) | set(oracle)):
        got = device[region]["occupancy"] if region in device else unknown
        want = oracle[region]["occupancy"] if region in oracle else unknown
        n = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
        if n:
            bad.append((region, n))
    assert not bad, "regions that differ from the oracle (region, voxels): %r" % bad[:8]
    return order, pipeline


def voxel_points(rng, voxels, region=(0, 0, 0)):
    """A point inside each voxel (index x + 32 * (y + 32 * z)) of `region`, off the voxel's faces."""
    voxels = np.asarray(voxels, dtype=np.int64)
    cell = np.column_stack([voxels & 31, (voxels >> 5) & 31, voxels >> 10]).astype(np.float64)
    return LOW + np.asarray(region) * EDGE + (cell + rng.uniform(0.15, 0.85, size=cell.shape)) * RES


def rays_to(rng, ends, region=(0, 0, 0), reach=0.25):
    """Rays of at most `reach` per axis to `ends`, started inside `region`."""
    low = LOW + np.asarray(region) * EDGE
    starts = np.clip(ends + rng.uniform(-reach, reach, size=ends.shape), low + 0.02, low + EDGE - 0.02)
    return pairs(starts, ends)


def crossed_batch(rng, n, crossers=3, marked=32):
    """n rays that end in region (0, 0, 0), end points uniform in it -- but the first min(n, marked) of them within three
    voxels of the +x face, where `crossers` rays each, six voxels long and AHEAD of the n rays in the call, pass through
    the end point on their way to an end in region (1, 0, 0): misses of earlier rays in sampled voxels, whatever n."""
    ends = LOW + rng.uniform(0.02, EDGE - 0.02, size=(n, 3))
    m = min(n, marked)
    ends[:m, 0] = LOW[0] + rng.uniform(2.92, 3.18, size=m)
    through = np.repeat(ends[:m], crossers, axis=0)
    starts = through - [0.12, 0.0, 0.0]
    beyond = through.copy()
    beyond[:, 0] = LOW[0] + EDGE + rng.uniform(0.05, 0.25, size=beyond.shape[0])
    rays = np.vstack([pairs(starts, beyond), rays_to(rng, ends)])
    assert samples_per_region(rays) == {(0, 0, 0): n, (1, 0, 0): m * crossers}
    return rays


# ---- 1: sizes around every boundary of the two instantiations ----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 8191, 8192])
def test_sizes_at_the_instantiations_edges(gpu, monkeypatch, n):
    """Exactly n samples in region (0, 0, 0) (2048 is the last size of the 256-thread instantiation, 8192 of the
    1024-thread one; 64 the smallest padded network), three calls of the same rays.  Uniform end points: ranked."""
    rays = crossed_batch(np.random.default_rng(100 + n), n)
    order, _ = run_case(monkeypatch, [rays] * 3)
    ranked, network = order[-1]
    assert (ranked, network) == (6, 0), order      # two regions (the crossing rays end in (1, 0, 0)), three calls


# ---- 2: bucket edges ---------------------------------------------------------------------------------------------------
def bucket_edge_calls(seed, per_edge_voxel, per_full_voxel):
    """Samples in the first and last voxel of consecutive buckets (voxels 31, 32, 63, 64, ...: 448 of them) and in all
    32 voxels of one bucket, twice."""
    rng = np.random.default_rng(seed)
    edges = np.sort(np.concatenate([np.arange(31, 32 * 225, 32), np.arange(32, 32 * 225, 32)]))[:448]
    assert edges[0] == 31 and edges[1] == 32 and edges[2] == 63
    full = 32 * 700 + np.arange(32)
    voxels = rng.permutation(np.concatenate([np.repeat(edges, per_edge_voxel), np.repeat(full, per_full_voxel)]))
    calls = [rays_to(np.random.default_rng(seed + 1 + k), voxel_points(rng, voxels)) for k in range(2)]
    assert all(samples_per_region(c) == {(0, 0, 0): voxels.shape[0]} for c in calls)
    return calls, voxels


def test_bucket_edges(gpu, monkeypatch):
    """2048 samples: 4 in each of the 448 edge voxels, 8 in each voxel of the full bucket.  sum(c^2)/n = 39 -- the full
    bucket alone makes 32 -- so the route is the threshold's choice and only the result is held."""
    calls, voxels = bucket_edge_calls(200, 4, 8)
    assert voxels.shape[0] == 2048
    order, _ = run_case(monkeypatch, calls)
    assert sum(order[-1]) == 2, order


def test_bucket_edges_ranked(gpu, monkeypatch):
    """The same voxels with 2 samples each (960 samples, sum(c^2)/n = 8: as crowded as a uniform region of 8192), which
    no threshold worth having sends to the network: an offset[b + 1] or a rank range off by one shows here."""
    calls, voxels = bucket_edge_calls(210, 2, 2)
    assert voxels.shape[0] == 960 and np.sum(np.bincount(voxels >> 5) ** 2) <= 8 * 960
    order, _ = run_case(monkeypatch, calls)
    assert order[-1] == (2, 0), order


# ---- 3: across the fallback threshold ------------------------------------------------------------------------------------
def rows_batch(seed, n, rows):
    """n samples in `rows` x-rows (buckets) of region (0, 0, 0), n / rows in each, x uniform."""
    rng = np.random.default_rng(seed)
    buckets = rng.choice(1024, size=rows, replace=False)
    voxels = np.repeat(buckets, n // rows) * 32 + rng.integers(0, 32, size=n)
    return rays_to(rng, voxel_points(rng, rng.permutation(voxels)))


@pytest.mark.parametrize("n", [2048, 8192])
def test_across_the_fallback_threshold(gpu, monkeypatch, n):
    """All n samples in k x-rows, k = n/2, n/4, .., 1: sum(c^2)/n = n/k sweeps 2 .. n.  Every step bit exact; ranked at
    the low end, the network at k = 1, and one change of route in between -- wherever the threshold lies.  (A region has
    1024 x-rows: the sweep of 8192 samples starts at k = 1024, sum(c^2)/n = 8.)"""
    routes = []
    k = n // 2
    while k >= 1:
        if k <= 1024:     # (a region has 1024 x-rows)
            calls = [rows_batch(300 + k, n, k), rows_batch(301 + k, n, k)]
            assert all(samples_per_region(c) == {(0, 0, 0): n} for c in calls)
            order, _ = run_case(monkeypatch, calls)
            ranked, network = order[-1]
            assert (ranked, network) in ((2, 0), (0, 2)), (k, order)
            routes.append("ranked" if ranked else "network")
        k //= 2
    assert routes[0] == "ranked" and routes[-1] == "network", routes
    assert sum(a != b for a, b in zip(routes, routes[1:])) == 1, routes


def one_voxel_batch(seed, n, crossers=64):
    """n rays that end in voxel (30, 16, 16) of region (0, 0, 0), from all around it, and -- anywhere among them in the
    call -- `crossers` rays along x through that voxel to an end in region (1, 0, 0): the voxel sits at a clamp, where a
    miss before a hit and a hit before a miss leave different values."""
    rng = np.random.default_rng(seed)
    hot = voxel_points(rng, np.full(n, 30 + 32 * (16 + 32 * 16)))
    through = voxel_points(rng, np.full(crossers, 30 + 32 * (16 + 32 * 16)))
    beyond = through.copy()
    beyond[:, 0] = LOW[0] + EDGE + rng.uniform(0.05, 0.25, size=crossers)
    rays = np.vstack([rays_to(rng, hot), pairs(through - [0.25, 0.0, 0.0], beyond)]).reshape(-1, 2, 3)
    rays = np.ascontiguousarray(rays[rng.permutation(rays.shape[0])]).reshape(-1, 3)
    assert samples_per_region(rays) == {(0, 0, 0): n, (1, 0, 0): crossers}
    return rays


@pytest.mark.parametrize("n", [2048, 8192])
def test_all_samples_in_one_voxel(gpu, monkeypatch, n):
    """sum(c^2) = n^2 in region (0, 0, 0): the network.  (The 64 samples of region (1, 0, 0) lie in one x-row too:
    sum(c^2)/n = 64, either route.)"""
    order, _ = run_case(monkeypatch, [one_voxel_batch(350, n), one_voxel_batch(351, n)])
    ranked, network = order[-1]
    assert ranked + network == 4 and network >= 2, order


# ---- 4: several regions in one launch ------------------------------------------------------------------------------------
def mixed_regions_batch(seed, sizes):
    """Region (r, 0, 0) gets sizes[r] samples: uniform for even r, in ONE x-row for odd r (the network)."""
    rng = np.random.default_rng(seed)
    rays = []
    for r, n in enumerate(sizes):
        voxels = rng.integers(0, 32768, size=n) if r % 2 == 0 else 32 * 500 + rng.integers(0, 32, size=n)
        rays.append(rays_to(rng, voxel_points(rng, voxels, (r, 0, 0)), (r, 0, 0)))
    rays = np.vstack(rays)
    assert samples_per_region(rays) == {(r, 0, 0): n for r, n in enumerate(sizes)}
    return rays


def test_mixed_regions_share_workgroups(gpu, monkeypatch):
    """40 regions of 1 .. 6000 samples ordered by launches of three workgroups each (OHMHIP_SORT_WORKGROUPS=3): a
    workgroup orders region after region in the same LDS, ranked after network and network after ranked (every other
    region has its samples in one x-row).  Both instantiations see both: the list is densest first, so the 1024-thread
    workgroups take 6000 (ranked), 5000 (one row: network), 3000 and 2049 (ranked) in turn, the 256-thread ones 2048,
    2047 (network), 700 (network), 65, 30, 1."""
    sizes = [30, 700, 2048, 5000, 6000, 1, 2049, 65, 3000, 2047] * 4
    calls = [mixed_regions_batch(400 + k, sizes) for k in range(2)]
    order, _ = run_case(monkeypatch, calls, env=(("OHMHIP_SORT_WORKGROUPS", 3),))
    ranked, network = order[-1]
    # (an odd region with a few dozen samples in its row may stay below the threshold; sum(c^2)/n = n for the others)
    assert ranked + network == 2 * len(sizes) and ranked >= len(sizes) and network >= 2 * 12, order


# ---- 5: the device-wide sort above 8192 samples ----------------------------------------------------------------------------
def test_dense_region_keeps_the_radix_path(gpu, monkeypatch):
    """9000 samples in one region: device-wide sort + k_hit_bounds, exact, and counted neither way."""
    rng = np.random.default_rng(500)
    calls = [rays_to(rng, LOW + rng.uniform(0.02, EDGE - 0.02, size=(9000, 3))) for _ in range(2)]
    assert all(samples_per_region(c) == {(0, 0, 0): 9000} for c in calls)
    order, _ = run_case(monkeypatch, calls)
    assert order[-1] == (0, 0), order


# ---- 6: speculated and repeated passes ---------------------------------------------------------------------------------
def spread_batch(seed, n, regions_x, reach=0.25):
    """n short rays, end points uniform over regions (0 .. regions_x - 1, 0 .. 1, 0 .. 1)."""
    rng = np.random.default_rng(seed)
    ends = LOW + rng.uniform([0.3, 0.3, 0.3], [regions_x * EDGE - 0.3, 2 * EDGE - 0.3, 2 * EDGE - 0.3], size=(n, 3))
    return pairs(ends + rng.uniform(-reach, reach, size=ends.shape), ends)


@pytest.mark.parametrize("early", [1, 0])
def test_three_calls_back_to_back(gpu, monkeypatch, early):
    """65536 rays over 16 regions (about 4096 samples each: both instantiations), three calls without a read in between:
    the second and third call's binning pass and ordering are launched on the previous call's guess."""
    calls = [spread_batch(600, 65536, 4), spread_batch(601, 65536, 4), spread_batch(600, 65536, 4)]
    assert max(samples_per_region(calls[0]).values()) <= 8192
    order, pipeline = run_case(monkeypatch, calls, early=early, back_to_back=True)
    ranked, network = order[-1]
    assert network == 0 and ranked >= 3 * 16, order
    assert pipeline[-1][0] == 3 and (pipeline[-1][1] == 2 if early else pipeline[-1][1] == 0), pipeline


@pytest.mark.parametrize("early", [1, 0])
def test_densest_region_jumps_over_2048(gpu, monkeypatch, early):
    """1500 + 1500 samples in two regions, then 3000 in one: the speculated launch counted on the 256-thread
    instantiation alone, the 1024-thread one is launched late, once the batch's own summary asks for it."""
    def batch(seed, split):
        rng = np.random.default_rng(seed)
        ends = LOW + rng.uniform(0.02, EDGE - 0.02, size=(3000, 3))
        return np.vstack([rays_to(rng, ends[:split] + [2 * EDGE, 0, 0], (2, 0, 0)), rays_to(rng, ends[split:])])
    calls = [batch(610, 1500), batch(611, 0), batch(612, 1500), batch(613, 0)]
    assert samples_per_region(calls[0]) == {(0, 0, 0): 1500, (2, 0, 0): 1500}
    assert samples_per_region(calls[1]) == {(0, 0, 0): 3000}
    order, _ = run_case(monkeypatch, calls, early=early)
    ranked, network = order[-1]
    assert network == 0 and ranked >= 6, order


@pytest.mark.parametrize("early", [1, 0])
def test_after_a_batch_of_another_size(gpu, monkeypatch, early):
    """512 rays size the segment buffer; 16384 rays then need more segments than the speculated pass was given: its
    results are dropped, the cursors reset (k_reset_cursors) and the pass and the ordering repeated."""
    small = [spread_batch(620 + k, 512, 1) for k in range(2)]
    big = spread_batch(622, 16384, 2)
    calls = [small[0], small[1], big, small[0], small[1]]
    order, pipeline = run_case(monkeypatch, calls, early=early)
    assert order[-1][1] == 0 and order[-1][0] >= 5, order
    if early:
        assert pipeline[2][1] == pipeline[1][1], pipeline      # the big call's early pass did not stand


# ---- 7: the sample mask and the first-sample table ---------------------------------------------------------------------
def test_rays_that_only_cross_sampled_voxels(gpu, monkeypatch):
    """2048 samples within six voxels of region (0, 0, 0)'s +x face, twice; then 2048 rays that start two voxels ahead
    of a sampled point, pass through it and end in region (1, 0, 0): no sample of theirs in the region, and every one
    crosses sampled voxels -- a mask bit or a first-sample entry left over from the calls before shows; then the
    samples again."""
    rng = np.random.default_rng(700)
    ends = LOW + rng.uniform([2.6, 0.02, 0.02], [3.18, EDGE - 0.02, EDGE - 0.02], size=(2048, 3))
    samples = rays_to(rng, ends)
    beyond = ends.copy()
    beyond[:, 0] = LOW[0] + EDGE + rng.uniform(0.05, 0.25, size=2048)
    crossing = pairs(ends - [0.2, 0.0, 0.0], beyond)
    assert samples_per_region(samples) == {(0, 0, 0): 2048} and samples_per_region(crossing) == {(1, 0, 0): 2048}
    order, _ = run_case(monkeypatch, [samples, samples, crossing, samples])
    assert order[-1][1] == 0, order
