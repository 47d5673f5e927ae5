"""-m gpu: GpuTransformSamples equivalent (ohmhip_transform_samples) vs the oracle's fp64 restatement of the reference
kernel, and the reference test's own property (tests/ohmtestgpu/GpuTests.cpp:32-228: samples pushed into a moving sensor
frame and transformed back must land on the original points).  Positions are bit exact (plain fp64 lerp); the rotated
sample goes through acos / sin, where the device maths library and glibc may differ in the last place: 1e-12 relative."""
import functools

import numpy as np
import pytest

import transform_cases as TC
import transform_ref as R
from ohm_amd import GpuMap, GpuTransformSamples, OccupancyMap, synth
from oracle import oracle as O
from parity import assert_parity, compare_maps, make_oracle

pytestmark = pytest.mark.gpu


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def quat_rotate(q, v):
    x, y, z, w = q
    m = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return m @ v


def trajectory(count, base_time, end_time):
    times = base_time + (end_time - base_time) * np.arange(count) / (count - 1)
    translations = np.array([-0.42, -0.42, -0.42]) + (np.arange(count) / (count - 1))[:, None] * 10.42
    angles = np.pi * np.arange(count) / (count - 1)
    # rotation about z by `angle`, as (x, y, z, w)
    rotations = np.stack([np.zeros(count), np.zeros(count), np.sin(angles / 2), np.cos(angles / 2)], axis=1)
    return times, translations, rotations


def test_transform_matches_oracle_and_round_trips(gpu):
    n = 20000
    idx = np.arange(n)
    global_pts = np.stack([(synth.uniform01(5, idx, s) - 0.5) * 40.0 for s in range(3)], axis=1)
    base = 1.7e9
    dt = 1e-3
    times, translations, rotations = trajectory(10, base, base + n * dt + 1.5 * dt)
    sample_times = base + 0.67 * dt + dt * idx
    # global -> local with the reference's pose rule (its test does the same on the CPU)
    local = np.zeros_like(global_pts)
    tidx = 0
    for i in range(n):
        while times[tidx + 1] < sample_times[i]:
            tidx += 1
        f = (sample_times[i] - times[tidx]) / (times[tidx + 1] - times[tidx])
        pos = translations[tidx] + f * (translations[tidx + 1] - translations[tidx])
        # pose rotation = rot[from] * slerp(rot[from], rot[to], f); both are rotations about z, so compose angles
        a0 = 2 * np.arctan2(rotations[tidx][2], rotations[tidx][3])
        a1 = 2 * np.arctan2(rotations[tidx + 1][2], rotations[tidx + 1][3])
        ang = a0 + (a0 + f * (a1 - a0))
        q = np.array([0.0, 0.0, np.sin(ang / 2), np.cos(ang / 2)])
        q_inv = q * np.array([-1, -1, -1, 1])
        local[i] = quat_rotate(q_inv, global_pts[i] - pos)
    # a few rejects: NaN component, beyond max_range (dot > max_range, as the reference compares)
    local[17, 1] = np.nan
    local[123] = [80.0, 0.0, 0.0]
    max_range = 60.0 * 60.0
    expect = O.transform_samples(times, translations, rotations, sample_times, local, max_range)
    ts = GpuTransformSamples()
    ptr, count = ts.transform(times, translations, rotations, sample_times, local, max_range)
    assert count == expect.shape[0] == 2 * (n - 2)
    got = ts.read(count)
    assert np.array_equal(got[0::2], expect[0::2])  # sensor positions: bit exact
    scale = np.maximum(np.abs(expect[1::2]), 1.0)
    assert np.max(np.abs(got[1::2] - expect[1::2]) / scale) < 1e-12
    # round trip (GpuTests.cpp:206-222 uses 1e-4 for its fp32 kernel; fp64 gets 1e-7 like the reference's CPU check)
    keep = np.ones(n, dtype=bool)
    keep[[17, 123]] = False
    assert np.max(np.linalg.norm(got[1::2] - global_pts[keep], axis=1)) < 1e-7
    # the device buffer feeds the integration path directly
    map_ = OccupancyMap(0.25)
    gm = GpuMap(map_)
    assert gm.integrateRaysDevice(ptr, count) == count
    gm.syncVoxels()
    assert len(map_.chunks) > 0
    ts.close()


def test_transform_edge_cases(gpu):
    ts = GpuTransformSamples()
    times, translations, rotations = trajectory(4, 100.0, 103.0)
    pts = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 3.0]])
    # sample times before, inside (exactly on a transform stamp) and after the trajectory
    st = np.array([99.0, 101.0, 200.0])
    expect = O.transform_samples(times, translations, rotations, st, pts)
    ptr, count = ts.transform(times, translations, rotations, st, pts)
    got = ts.read(count)
    assert count == 6
    assert np.all(np.isfinite(got))
    assert np.allclose(got, expect, rtol=1e-12, atol=1e-12)
    # two transforms: no search; one transform: that pose
    for k in (2, 1):
        expect = O.transform_samples(times[:k], translations[:k], rotations[:k], st, pts)
        ptr, count = ts.transform(times[:k], translations[:k], rotations[:k], st, pts)
        assert np.allclose(ts.read(count), expect, rtol=1e-12, atol=1e-12)
    # nothing in -> nothing out
    ptr, count = ts.transform(times, translations, rotations, np.zeros(0), np.zeros((0, 3)))
    assert count == 0
    ts.close()


# ---------------------------------------------------------------------------------------------------------------------
# The device against the arbitrary-precision reference (tests/transform_ref.py) on the families of
# tests/transform_cases.py.  Discrete results are exact; sensor positions are bit-identical to the C oracle (no
# transcendental function, no contraction, IEEE divide); for the samples the allowance is MEASURED, not chosen: four
# times the C oracle's own worst scaled deviation from the reference on the same inputs in the same run -- the device's
# acos / sin are specified to a few ulp where glibc's are within one, those errors pass linearly into the result, and
# nothing else in the chain may differ.
# ---------------------------------------------------------------------------------------------------------------------
FAMILIES = TC.families()
DEVICE_FACTOR = 4.0


def oracle_rows(case):
    return O.transform_samples(case["times"], case["translations"], case["rotations"], case["sample_times"],
                               case["local"], case["max_range"]).reshape(-1, 6)


def device_rows(ts, case, local=None, sample_times=None, max_range=None):
    """-> ((valid, 6) rows read back, ray_elements, device pointer)"""
    ptr, count = ts.transform(case["times"], case["translations"], case["rotations"],
                              case["sample_times"] if sample_times is None else sample_times,
                              case["local"] if local is None else local,
                              case["max_range"] if max_range is None else max_range)
    assert count % 2 == 0
    return ts.read(count).reshape(-1, 6), count, ptr


def bit_identical(a, b):
    """Same bit patterns, any NaN standing for any other (its payload is not part of the result)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan]))


def scaled_difference(got, expect, local_kept):
    """Worst |device sample - oracle sample| over max(1, |local sample|, |position|), finite rows only."""
    if got.shape[0] == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        scale = np.maximum(1.0, np.maximum(np.linalg.norm(local_kept, axis=1), np.linalg.norm(expect[:, :3], axis=1)))
        err = np.max(np.abs(got[:, 3:] - expect[:, 3:]), axis=1) / scale
    finite = np.all(np.isfinite(expect), axis=1) & np.all(np.isfinite(local_kept), axis=1)
    assert np.array_equal(np.isnan(got[~finite]), np.isnan(expect[~finite]))
    return float(np.max(err[finite])) if finite.any() else 0.0


@functools.lru_cache(maxsize=None)
def general_allowance():
    """DEVICE_FACTOR x the oracle's worst scaled sample deviation from the reference on the general family (the stamps
    near 1.7e9): the bound for device rows compared with oracle rows where the reference is not evaluated per sample.
    It bounds another quantity than test_device_matches_reference does -- device against ORACLE, on inputs of another
    family -- and stands in for it by the triangle inequality: device and oracle each lie within a few ulp-sized errors
    of the exact value, so their difference is of the same size as either one's deviation from the reference."""
    worst = None
    for case in dict(FAMILIES)["general_big_stamps"]:
        kept, rows = R.reference(case)
        worst = R.merge(worst, R.deviation(rows, oracle_rows(case), case["local"][kept]))
    assert worst["mismatched"] == 0 and 0.0 < worst["sample"] < 64.0 * 2.0 ** -52, worst
    return DEVICE_FACTOR * worst["sample"]


@pytest.mark.parametrize("name,cases", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_device_matches_reference(gpu, name, cases, capsys):
    ts = GpuTransformSamples()
    oracle_worst = device_worst = None
    for case in cases:
        kept, rows = R.reference(case)
        expect = oracle_rows(case)
        got, count, _ = device_rows(ts, case)
        assert count == 2 * len(rows) and got.shape[0] == expect.shape[0] == len(rows)
        # order: every sample is transformed on its own, so the reference's kept samples alone, unfiltered, give the
        # same rows
        if len(rows):
            alone, _, _ = device_rows(ts, case, case["local"][kept], case["sample_times"][kept], float("inf"))
            assert bit_identical(got, alone)
        assert bit_identical(got[:, :3], expect[:, :3])  # sensor positions
        oracle_worst = R.merge(oracle_worst, R.deviation(rows, expect, case["local"][kept]))
        device_worst = R.merge(device_worst, R.deviation(rows, got, case["local"][kept]))
    ts.close()
    with capsys.disabled():
        print("\n[transform vs reference] %-22s sample: oracle %.3e device %.3e (allowed %.3e)  position: %.3e (%.3e m)"
              % (name, oracle_worst["sample"], device_worst["sample"], DEVICE_FACTOR * oracle_worst["sample"],
                 device_worst["position"], device_worst["position_abs"]))
    assert oracle_worst["mismatched"] == 0 and device_worst["mismatched"] == 0, (oracle_worst, device_worst)
    assert device_worst["sample"] <= DEVICE_FACTOR * oracle_worst["sample"], (device_worst, oracle_worst)


@pytest.mark.parametrize("pattern", TC.COMPACTION_PATTERNS)
@pytest.mark.parametrize("n", TC.COMPACTION_SIZES)
def test_device_compaction(gpu, n, pattern):
    """rocprim::exclusive_scan over the keep flags + scatter: ray_elements, and rows equal to the oracle's rows in the
    oracle's order (which tests/test_transform_ref.py holds to the reference's kept indices) -- positions bit exact,
    samples within the measured allowance."""
    case, rejected = TC.compaction_case(n, pattern)
    expect = oracle_rows(case)
    kept = np.flatnonzero(~rejected)
    assert expect.shape[0] == kept.shape[0]
    ts = GpuTransformSamples()
    got, count, _ = device_rows(ts, case)
    ts.close()
    assert count == 2 * kept.shape[0]
    if pattern == "all":
        assert count == 0
    # row identity and order rest on the bit-exact positions: the sample times are random, so no two rows share one
    assert bit_identical(got[:, :3], expect[:, :3])
    assert scaled_difference(got, expect, case["local"][kept]) <= general_allowance()  # device vs oracle, see there


def test_device_buffer_reuse(gpu):
    """One GpuTransformSamples object, a large call, a tiny one, a middling one: the grow-only buffer keeps rows of the
    earlier calls behind the new ones, and none of them may be counted or read as a result."""
    ts = GpuTransformSamples()
    for n in (2 ** 20 + 77, 3, 65537):
        case, rejected = TC.compaction_case(n, "scattered", seed=11)
        expect = oracle_rows(case)
        got, count, _ = device_rows(ts, case)
        assert count == 2 * expect.shape[0] == 2 * int((~rejected).sum())
        assert bit_identical(got[:, :3], expect[:, :3])
        assert scaled_difference(got, expect, case["local"][~rejected]) <= general_allowance()
    ts.close()


def raw_layers(chunks):
    return {key: {name: np.asarray(data).tobytes() for name, data in layers.items()} for key, layers in chunks.items()}


def test_device_rays_integrate_like_host_rays(gpu):
    """The hand-off: the device buffer integrated in place (map A) gives the very map that the same rays give when they
    are read back and passed in from the host (map B), and that map is the CPU oracle's for those rays."""
    rng = np.random.default_rng(301)
    times, translations, rotations = TC.random_trajectory(rng, 120, TC.BIG_STAMP, extent=4.0)
    n = 50000
    st = rng.uniform(times[0] - 0.2, times[-1] + 0.2, n)
    local = TC.random_local(rng, n, reach=14.0)
    max_range = 12.0 * 12.0
    ts = GpuTransformSamples()
    ptr, count = ts.transform(times, translations, rotations, st, local, max_range)
    rays = ts.read(count)
    assert count == 2 * int(R.keep_mask(local, max_range).sum()) and 0.9 * n < count // 2 < n
    assert np.all(np.isfinite(rays))
    layers = ("occupancy", "mean")
    map_a, map_b = OccupancyMap(0.1, (32, 32, 32), layers=layers), OccupancyMap(0.1, (32, 32, 32), layers=layers)
    gm_a, gm_b = GpuMap(map_a), GpuMap(map_b)
    assert gm_a.integrateRaysDevice(ptr, count) == count
    assert gm_b.integrateRays(rays) == count
    gm_a.syncVoxels()
    gm_b.syncVoxels()
    ts.close()
    assert len(map_a.chunks) > 50
    assert set(map_a.chunks.keys()) == set(map_b.chunks.keys())
    assert raw_layers(map_a.chunks) == raw_layers(map_b.chunks)
    om = make_oracle(map_a)
    om.integrate_occupancy(rays)
    assert_parity(compare_maps(om.chunks(), map_a.chunks, list(layers), exact_float=True))
