"""-m gpu: the early binning pass (BatchRun::frontHalf; OHMHIP_EARLY_BIN) and the sample mask set by the ordering step.

A plain occupancy batch that follows another one launches its k_ray_bin on the front stream, behind the previous batch's
walk and BESIDE that batch's apply kernels; its sample mask bits are set by k_sort_region_hits / k_hit_bounds on the
compute stream.  Every case runs the same calls through a device map and the CPU oracle (oracle.oracle.OracleMap) and
compares every region either side knows bit for bit (uint32 views) after the last call, once with OHMHIP_EARLY_BIN=1 and
once with 0.  GpuMap.pipelineCounts() tells the routes apart, so a fallback to the compute stream cannot pass for the
early route: with 1 every call the case marks as `early` must have been binned early, with 0 none may be.

Coalescing is off (a call is a device batch) and, unless a case says otherwise, the maps are created under
OHMHIP_CHUNK_SEGMENTS = OHMHIP_MIN_CHUNK_SEGMENTS = 256, so a region with a few thousand segments is cut into several
chunks and its counts and samples go through k_apply_lists -- the kernels the early pass runs beside.

The mask cases were also run against a build in which the early k_ray_bin still set the mask bits and the sort did not
(not committed).  test_mask_hand_over passes there: the device has finished a 2048-ray call before the host presents
the next one, so the pass never meets the apply kernels.  test_mask_hand_over_with_batches_in_flight, added for that
reason, fails there with OHMHIP_EARLY_BIN=1 -- 57 voxels of region (0, 0, 0) and 501 of (1, 0, 0) differ from the
oracle -- and passes with 0 (profiles/r08_notes.md)."""
import ctypes as C

import numpy as np
import pytest

import ray_pattern_ref as R
from ohm_amd import ClearingPattern, GpuMap, OccupancyMap, RayFlag, RayPattern
from ohm_amd import _lib as L
from parity import make_oracle
from test_gpu_mean_states import read_device

pytestmark = pytest.mark.gpu

EDGE = 3.2                                    # a 32^3 region at 0.1 m
LOW = np.array([-1.6, -1.6, -1.6])            # low corner of region (0, 0, 0): the map's origin is the region's centre
ORIGIN = LOW + [1.63, 1.66, 1.61]             # inside voxel (16, 16, 16) of region (0, 0, 0), off its centre
STOP = int(RayFlag.kRfStopOnFirstOccupied)
EXCLUDE_RAY = int(RayFlag.kRfExcludeRay)
EARLY = pytest.mark.parametrize("early", [1, 0])


def pairs(starts, ends):
    ends = np.asarray(ends, dtype=np.float64)
    out = np.empty((2 * ends.shape[0], 3), dtype=np.float64)
    out[0::2] = starts
    out[1::2] = ends
    return out


def fan(seed, n=3000, reach=6.0, origin=ORIGIN):
    """n rays from (nearly) one origin to points within `reach` of it on every axis: a few dozen regions of 32^3."""
    rng = np.random.default_rng(seed)
    return pairs(origin + rng.uniform(-0.02, 0.02, size=(n, 3)), origin + rng.uniform(-reach, reach, size=(n, 3)))


def short_rays(seed, n, lo, hi, length=0.25):
    """n rays of at most `length` per axis that start in [lo, hi) on every axis, measured from region (0, 0, 0)'s low
    corner (with lo / hi a `length` inside a region they end in it too)."""
    rng = np.random.default_rng(seed)
    starts = LOW + rng.uniform(lo, hi, size=(n, 3))
    return pairs(starts, starts + rng.uniform(-length, length, size=(n, 3)))


def samples_per_region(rays):
    """{region: end points in it} of a 32^3 map (checked against the oracle's keys in Maps.__init__)."""
    regions, counts = np.unique(np.floor((rays[1::2] - LOW) / EDGE).astype(int), axis=0, return_counts=True)
    return {tuple(int(v) for v in r): int(c) for r, c in zip(regions, counts)}


class Maps:
    """A device map and the oracle fed the same calls; `marks` holds pipelineCounts() after every integrate call."""

    def __init__(self, monkeypatch, early, dims=(32, 32, 32), chunk=256, region_capacity=64, ray_filter=None):
        monkeypatch.setenv("OHMHIP_EARLY_BIN", str(early))           # all three are read at map creation
        monkeypatch.setenv("OHMHIP_CHUNK_SEGMENTS", str(chunk))
        monkeypatch.setenv("OHMHIP_MIN_CHUNK_SEGMENTS", str(chunk))
        self.early = early
        self.map = OccupancyMap(0.1, dims, layers=("occupancy",))
        if ray_filter:
            self.map.ray_filter = ray_filter
        self.gm = GpuMap(self.map, region_capacity=region_capacity)
        self.gm.setBatchCoalescing(0)
        self.om = make_oracle(self.map)
        self.marks = []
        if tuple(dims) == (32, 32, 32):       # the geometry the cases are built on
            for point in (LOW + 0.01, LOW + EDGE - 0.01, LOW + [EDGE + 0.01, 0.01, 2 * EDGE + 0.01]):
                assert self.om.voxel_key(point)[0] == tuple(np.floor((point - LOW) / EDGE).astype(int))

    def integrate(self, rays, flags=0, read=False):
        self.gm.integrateRays(rays, None, None, flags)
        self.om.integrate_occupancy(rays, flags=flags)
        self.marks.append(self.gm.pipelineCounts())
        if read:
            read_device(self.map, self.gm)

    def integrate_back_to_back(self, calls):
        """The device calls one behind the other, nothing in between that lets the device run dry; the oracle afterwards."""
        for rays in calls:
            self.gm.integrateRays(rays)
            self.marks.append(self.gm.pipelineCounts())
        for rays in calls:
            self.om.integrate_occupancy(rays)

    def binned_early(self, call):
        """Whether integrate call `call` (0-based) was binned early."""
        before = self.marks[call - 1][1] if call else 0
        return self.marks[call][1] - before == 1

    def check_routes(self, early_calls, compute_calls=()):
        """OHMHIP_EARLY_BIN=1: `early_calls` were binned early, `compute_calls` were not.  0: no call was."""
        assert [m[0] for m in self.marks] == list(range(1, len(self.marks) + 1)), self.marks
        if not self.early:
            assert self.marks[-1][1] == 0, self.marks
            return
        assert all(self.binned_early(k) for k in early_calls), (early_calls, self.marks)
        assert not any(self.binned_early(k) for k in compute_calls), (compute_calls, self.marks)

    def finish(self):
        """Every region either side knows, bit for bit; a region one side does not know counts as never observed."""
        device = read_device(self.map, self.gm)
        oracle = self.om.chunks(["occupancy"])
        unknown = np.full(self.map.regionVoxelVolume(), np.inf, dtype=np.float32)
        bad = []
        for region in sorted(set(device) | set(oracle)):
            got = device[region]["occupancy"] if region in device else unknown
            want = oracle[region]["occupancy"] if region in oracle else unknown
            n = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
            if n:
                bad.append((region, n))
        self.gm.close()
        assert not bad, "regions that differ from the oracle (region, voxels): %r" % bad[:8]


# ---- the mask hand-over ---------------------------------------------------------------------------------------------------
def handover_batches(n=2048, seed=5, n_a=None, end_regions=1):
    """A: n_a (n) rays from ORIGIN through region (1, 0, 0) to end points in the regions (2, 0, 0) .. (1 + end_regions,
    0, 0).  B: n rays from ORIGIN to points ON A's first n rays, half of them in region (0, 0, 0), half in (1, 0, 0): B's
    end voxels are voxels A's rays cross."""
    rng = np.random.default_rng(seed)
    n_a = n_a or n
    ends_a = LOW + np.column_stack([rng.uniform(6.6, 7.4 + EDGE * (end_regions - 1), size=n_a), rng.uniform(0.4, 2.8, size=n_a),
                                    rng.uniform(0.4, 2.8, size=n_a)])
    # (the points ON the rays: at these x, in region (0, 0, 0) for the first half, in (1, 0, 0) for the second)
    x_b = LOW[0] + np.where(np.arange(n) < n // 2, rng.uniform(1.9, 3.0, size=n), rng.uniform(3.4, 6.2, size=n))
    t = (x_b - ORIGIN[0]) / (ends_a[:n, 0] - ORIGIN[0])
    ends_b = ORIGIN + (ends_a[:n] - ORIGIN) * t[:, None]
    a, b = pairs(ORIGIN, ends_a), pairs(ORIGIN, ends_b)
    per_region = samples_per_region(a)
    assert set(per_region) == {(2 + k, 0, 0) for k in range(end_regions)} and sum(per_region.values()) == n_a
    assert max(per_region.values()) <= 8192           # (more in one region, and the call after A is not speculated)
    assert samples_per_region(b) == {(0, 0, 0): n // 2, (1, 0, 0): n - n // 2}
    return a, b


@EARLY
@pytest.mark.parametrize("read", [False, True], ids=["no reads", "read after every call"])
def test_mask_hand_over(gpu, monkeypatch, early, read):
    """A, B, A, B ... eight calls.  Regions (0, 0, 0) and (1, 0, 0) hold 2048 and 1024 .. 2048 segments per call -- four to
    eight 256-segment chunks, the apply_counts route -- and B's samples lie in voxels whose miss counts A's k_apply_lists
    applies while B's binning pass runs: a mask bit B set there early would be read by A's apply kernels and cleared by
    A's k_batch_cleanup before B's walk looks for it."""
    a, b = handover_batches()
    maps = Maps(monkeypatch, early)
    for k in range(8):
        maps.integrate(b if k % 2 else a, read=read)
    maps.check_routes(early_calls=range(2, 8))
    maps.finish()


@EARLY
def test_mask_hand_over_with_batches_in_flight(gpu, monkeypatch, early):
    """The same geometry with 65536 rays in A, their end points spread over ten regions (at most 8192 samples in each, so
    that B is still speculated), and the eight calls issued back to back (the oracle is fed afterwards): A's walk and
    apply kernels are still on the device when the host launches B's front half, so B's binning pass really does run
    beside A's k_apply_lists / k_batch_cleanup.  With the 2048-ray A above the device has finished a call before the host
    presents the next one, and the order on the streams is never put to the test."""
    a, b = handover_batches(n_a=65536, seed=6, end_regions=10)
    maps = Maps(monkeypatch, early)
    maps.integrate_back_to_back([a, b] * 4)
    maps.check_routes(early_calls=range(2, 8))
    maps.finish()


# ---- samples the walk does not replay ---------------------------------------------------------------------------------
@EARLY
@pytest.mark.parametrize("chunk", [256, 8192], ids=["chunks of 256", "one chunk"])
def test_dense_samples_then_samples_in_the_same_region(gpu, monkeypatch, early, chunk):
    """7000 rays inside region (0, 0, 0): more samples than the walk stages in LDS (6144), so they are replayed by
    k_apply_lists and their deferred misses by k_flagged_events -- after the walk, beside the next call's binning pass.
    With 256-segment chunks the region is cut into 28 chunks; with 8192-segment chunks (and more than 16384 rays in the
    call, which keeps the batch's chunk size there) its 7000 segments are ONE chunk and only the samples are listed.  The
    next call ends in voxels of that region."""
    dense = np.vstack([short_rays(21, 7000, 0.4, 2.8), short_rays(22, 10000, 3.6, 12.4)])
    into = pairs(LOW + [4.0, 1.7, 1.5], LOW + np.random.default_rng(23).uniform(0.3, 2.9, size=(2048, 3)))
    assert samples_per_region(dense)[(0, 0, 0)] == 7000 and samples_per_region(into) == {(0, 0, 0): 2048}
    maps = Maps(monkeypatch, early, chunk=chunk)
    maps.integrate(fan(20))
    maps.integrate(dense)
    maps.integrate(into)
    maps.integrate(dense)
    maps.integrate(into)
    maps.check_routes(early_calls=range(2, 5))
    maps.finish()


# ---- wrong guesses ----------------------------------------------------------------------------------------------------
@EARLY
def test_wrong_guess_segment_buffer(gpu, monkeypatch, early):
    """512 short rays size the segment buffer; 8192 rays of up to 30 m then need more segments than the speculated pass
    was given: its results are dropped and the pass is repeated on the compute stream (not counted as early)."""
    short = short_rays(31, 512, 0.4, 2.8)
    rng = np.random.default_rng(32)
    direction = rng.normal(size=(8192, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    far = pairs(ORIGIN, ORIGIN + direction * rng.uniform(20.0, 30.0, size=(8192, 1)))
    maps = Maps(monkeypatch, early)
    for rays in (short, short, far, short, short):
        maps.integrate(rays)
    maps.check_routes(early_calls=(1, 3, 4), compute_calls=(0, 2))
    maps.finish()


@EARLY
def test_wrong_guess_dense_region(gpu, monkeypatch, early):
    """9000 samples in one region are more than k_sort_region_hits orders (8192): the speculated pass is dropped, the keys
    go through the device-wide sort and k_hit_bounds sets the mask.  The call after it is not speculated at all."""
    sparse = fan(41)
    dense = short_rays(42, 9000, 0.4, 2.8)
    assert samples_per_region(dense) == {(0, 0, 0): 9000}
    maps = Maps(monkeypatch, early)
    for rays in (sparse, sparse, dense, sparse, sparse, dense, sparse):
        maps.integrate(rays)
    maps.check_routes(early_calls=(1, 4), compute_calls=(0, 2, 3, 5, 6))
    maps.finish()


# ---- no walk before ---------------------------------------------------------------------------------------------------
@EARLY
def test_after_a_call_without_chunks(gpu, monkeypatch, early):
    """kRfExcludeRay: samples only, no segments, no walk kernel -- tev[3] is a plain record.  A normal call follows."""
    maps = Maps(monkeypatch, early)
    maps.integrate(fan(51))
    maps.integrate(fan(52), flags=EXCLUDE_RAY)
    maps.integrate(fan(53))
    maps.integrate(fan(54), flags=EXCLUDE_RAY)
    maps.integrate(fan(55))
    maps.check_routes(early_calls=())
    maps.finish()


@EARLY
def test_after_a_call_the_filter_rejects(gpu, monkeypatch, early):
    """Every ray of the second and fourth call is longer than the filter's 5 m: nothing to bin, walk or apply."""
    rng = np.random.default_rng(56)
    direction = rng.normal(size=(2048, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    rejected = pairs(ORIGIN, ORIGIN + direction * rng.uniform(6.0, 9.0, size=(2048, 1)))
    maps = Maps(monkeypatch, early, ray_filter=("good", 5.0))
    for rays in (fan(57, reach=2.5), rejected, fan(58, reach=2.5), rejected, fan(59, reach=2.5), fan(60, reach=2.5)):
        maps.integrate(rays)
    maps.check_routes(early_calls=())
    maps.finish()


# ---- other work in between --------------------------------------------------------------------------------------------
@EARLY
def test_other_work_between_speculated_calls(gpu, monkeypatch, early):
    """A read, a query, a stop-flag batch, a clearing pattern and an upload, each between two speculated calls."""
    maps = Maps(monkeypatch, early)
    gm, om = maps.gm, maps.om
    for seed in (61, 62):
        maps.integrate(fan(seed))
    gm.syncVoxels()
    maps.integrate(fan(63))
    gm.raysQuery(fan(64, n=500))
    maps.integrate(fan(65))
    maps.integrate(fan(66), flags=STOP)                                    # call 4: not an occupancy_mode batch
    maps.integrate(fan(67))                                                # call 5: follows one, not speculated
    maps.integrate(fan(68))
    pattern = RayPattern()
    pattern.addRays(pairs(np.zeros(3), np.random.default_rng(69).uniform(-3.0, 3.0, size=(400, 3))))
    clearing = ClearingPattern(pattern, False)
    pose = list(ORIGIN) + [0.0, 0.0, 0.0, 1.0]
    assert clearing.apply(gm, pose[:3], pose[3:]) == 2 * pattern.rayCount()
    om.integrate_occupancy(R.build_rays(pattern.rayPoints(), [pose]), flags=int(ClearingPattern.kDefaultRayFlags))
    maps.integrate(fan(70))
    maps.integrate(fan(71))
    block = np.random.default_rng(72).uniform(-1.5, 1.5, size=maps.map.regionVoxelVolume()).astype(np.float32)
    block[::7] = np.inf
    key = np.array([[0, 0, 0]], dtype=np.int16)
    src = (C.c_void_p * 1)(block.ctypes.data)
    L.check(L.lib.ohmhip_map_write_regions(gm._handle, L.LID_OCCUPANCY, key.ctypes.data, 1, src), "write_regions")
    om.region_layer_view((0, 0, 0), "occupancy")[:] = block
    maps.integrate(fan(73))
    maps.integrate(fan(74))
    if early:
        assert all(maps.binned_early(k) for k in (2, 3, 6, len(maps.marks) - 1)), maps.marks
    else:
        assert maps.marks[-1][1] == 0
    maps.finish()


# ---- pool growth, two maps, another region size -----------------------------------------------------------------------
@EARLY
def test_pool_growth_on_a_speculated_call(gpu, monkeypatch, early):
    """A pool of 4 regions; the third call -- speculated -- touches a few dozen: its set-up overflows the pool, the early
    pass returns at once, the pool grows and the call is repeated on the compute stream."""
    maps = Maps(monkeypatch, early, region_capacity=4)
    inside = [short_rays(80 + k, 2048, 0.4, 2.8) for k in range(2)]
    for rays in (inside[0], inside[1], fan(82), fan(83), fan(84)):
        maps.integrate(rays)
    assert maps.gm.cacheStats()["region_capacity"] > 4
    maps.check_routes(early_calls=(1, 4), compute_calls=(0, 2))
    maps.finish()


@EARLY
def test_two_maps_alternating(gpu, monkeypatch, early):
    first, second = Maps(monkeypatch, early), Maps(monkeypatch, early)
    a, b = handover_batches(seed=91)
    for k in range(6):
        first.integrate(b if k % 2 else a)
        second.integrate(fan(92 + k))
    for maps in (first, second):
        maps.check_routes(early_calls=range(2, 6))
        maps.finish()


@EARLY
def test_region_size_20_12_24(gpu, monkeypatch, early):
    """Region edges that are no powers of two: the general k_ray_bin instantiation."""
    maps = Maps(monkeypatch, early, dims=(20, 12, 24))
    a, b = handover_batches(seed=95)
    for rays in (fan(96), a, b, a, b, fan(97)):
        maps.integrate(rays)
    maps.check_routes(early_calls=range(2, 6))
    maps.finish()
