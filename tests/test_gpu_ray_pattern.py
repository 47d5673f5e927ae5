"""GPU: RayPattern / RayPatternConical / ClearingPattern on the device (include/ohmhip.h, RAY PATTERNS).  The rays the
device builds equal the model (tests/ray_pattern_ref.py) bit for bit; the maps they are integrated into equal the CPU
oracle fed the model's rays, bit for bit on occupancy and mean."""
import ctypes as C
import math

import numpy as np
import pytest

from ohm_amd import (ClearingPattern, GpuMap, GpuNdtMap, OccupancyMap, RayFlag, RayPattern, RayPatternConical, synth)
from ohm_amd import _lib as L
from ohm_amd.raypattern import POSE_MAT4, POSE_QUAT
from oracle.oracle import lib as oracle_lib

import ray_pattern_ref as R
from parity import assert_parity, compare_maps, make_oracle

pytestmark = pytest.mark.gpu

CLEARING_FLAGS = int(ClearingPattern.kDefaultRayFlags)


def voxel_centre_000():
    """map.voxelCentreGlobal(Key(0, 0, 0, 0, 0, 0)) of the reference test's map (resolution 0.1)."""
    return np.array(make_oracle(OccupancyMap(0.1, (32, 32, 32))).voxel_centre((0, 0, 0), (0, 0, 0)))


def pose_matrix(pose):
    """The column-major 4 x 4 matrix of a (translation, quaternion xyzw) pose: any matrix serves, the model takes it as
    given; built in numpy, it is an input like the quaternion is."""
    t, (x, y, z, w) = pose[:3], pose[3:]
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = t
    return m.T.reshape(16)


def three_poses():
    """Identity; the reference test's angleAxis(-pi/2, z) at the voxel centre; a general non-unit quaternion ~1e3 away."""
    quarter = R.angle_axis(-0.5 * math.pi, (0.0, 0.0, 1.0))
    return np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0],
                     list(voxel_centre_000()) + list(quarter),
                     [1013.25, -987.5, 1001.125, 0.31, -0.52, 0.23, 0.83]])


# ---- 1. the transform, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [1.0, 0.37])
@pytest.mark.parametrize("pose_kind", [POSE_QUAT, POSE_MAT4])
def test_transform_bit_for_bit(gpu, pose_kind, scaling):
    """67 rays (the last wave has idle lanes) with non-zero starts, three poses in one call: ohmhip_pattern_build_rays
    and ohmhip_pattern_last_rays give the model's doubles."""
    rng = np.random.default_rng(67)
    pairs = rng.uniform(-3.0, 3.0, size=(2 * 67, 3))
    pattern = RayPattern()
    pattern.addRays(pairs)
    assert pattern.rayCount() == 67
    poses = three_poses()
    if pose_kind == POSE_MAT4:
        poses = np.array([pose_matrix(p) for p in poses])
    expected = R.build_rays(pairs, poses, pose_kind, scaling)
    got = pattern.buildRaysMany(poses, pose_kind, scaling)
    assert got.shape == (3 * 2 * 67, 3)
    assert np.array_equal(got, expected)
    n = C.c_size_t(0)
    L.check(L.lib.ohmhip_pattern_last_rays(pattern._device_pattern(), None, C.byref(n)))
    assert n.value == 3 * 2 * 67
    last = np.full((n.value, 3), -1.0)
    L.check(L.lib.ohmhip_pattern_last_rays(pattern._device_pattern(), last.ctypes.data, C.byref(n)))
    assert np.array_equal(last, expected)
    # the reference's overloads, one pose each
    if scaling == 1.0:
        for i, pose in enumerate(poses):
            single = pattern.buildRays(pose) if pose_kind == POSE_MAT4 else pattern.buildRays(pose[:3], pose[3:])
            assert np.array_equal(single, expected[i * 134:(i + 1) * 134])
        if pose_kind == POSE_MAT4:    # a (4, 4) array in row, column indexing is the same matrix
            assert np.array_equal(pattern.buildRays(poses[2].reshape(4, 4).T), expected[2 * 134:])
    pattern.close()


# ---- 2. RayPattern.Clearing as the reference writes it ------------------------------------------------------------------
def seed_region(map_, om, values):
    """CPU-side voxel writes (Voxel<float>::write in the reference's tests): region (0, 0, 0) of the host map and of the
    oracle holds `values` {local (x, y, z): log-odds}, everything else unobserved."""
    tile = np.full(32 * 32 * 32, np.inf, dtype=np.float32)
    for (x, y, z), v in values.items():
        tile[x + 32 * (y + 32 * z)] = np.float32(v)
    map_.chunks[(0, 0, 0)] = {"occupancy": tile.copy()}
    c = np.array(om.voxel_centre((0, 0, 0), (16, 16, 16)))
    om.integrate_occupancy(np.array([c, c]))      # makes the region exist in the oracle
    om.region_layer_view((0, 0, 0), "occupancy")[:] = tile


def test_ray_pattern_clearing_as_the_reference_writes_it(gpu):
    """RayPattern.Clearing (tests/ohmtestgpu/GpuRayPatternTests.cpp:28-85): a line of 20 occupied voxels along x, hit
    probability 0.51, miss probability 0; RayPattern.addPoint((0, 20 * resolution, 0)) in a ClearingPattern, applied 20
    times with angleAxis(-pi/2, z) at the centre of voxel 0.  Every application frees exactly the first occupied voxel."""
    map_ = OccupancyMap(0.1, (32, 32, 32))
    map_.setHitProbability(0.51)
    map_.setMissProbability(0.0)
    om = make_oracle(map_)
    hit = np.float32(map_.hit_value)
    seed_region(map_, om, {(x, 0, 0): hit for x in range(20)})
    gm = GpuMap(map_, True, 2)
    line = RayPattern()
    line.addPoint((0.0, map_.resolution * 20, 0.0))
    clearing = ClearingPattern(line, False)
    translate = voxel_centre_000()
    rotation = R.angle_axis(-0.5 * math.pi, (0.0, 0.0, 1.0))
    rays = R.build_rays(line.rayPoints(), [list(translate) + list(rotation)])
    miss = map_.missValue()
    for i in range(20):
        occ = map_.chunks[(0, 0, 0)]["occupancy"]
        assert occ[i] >= map_.occupancy_threshold_value
        assert clearing.apply(gm, translate, rotation) == 2
        gm.syncVoxels()
        assert np.array_equal(clearing.lastRaySet(), rays)
        om.integrate_occupancy(rays, flags=CLEARING_FLAGS)
        occ = map_.chunks[(0, 0, 0)]["occupancy"]
        assert np.isfinite(occ[i]) and occ[i] < map_.occupancy_threshold_value   # voxel i is no longer occupied
        assert np.all(occ[i + 1:20] == hit)                                      # the ray stopped there
        assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy"], exact_float=True))
        assert gm.missValue() == miss and map_.missValue() == miss
    gm.close()


# ---- 3. the scaled miss value and the rays that were waiting -------------------------------------------------------------
def wall_rays(n, seed, x=2.0):
    """n rays from near the origin to points of the plane at `x`, within +-0.8 m of the axis."""
    rng = np.random.default_rng(seed)
    rays = np.empty((2 * n, 3))
    rays[0::2] = (0.05, 0.05, 0.05)
    rays[1::2, 0] = x + rng.uniform(0.0, 0.09, size=n)
    rays[1::2, 1:] = rng.uniform(-0.8, 0.8, size=(n, 2))
    return rays


def test_miss_value_scaling_against_waiting_rays(gpu):
    """Coalescing at its default: a 100-ray host batch is still waiting when apply(probability_scaling=0.5) is called, and
    another follows.  The map equals the oracle integrating the three ray sets in order with the miss values
    (m, fp32(m * 0.5), m).  Setting the miss value, integrating and setting it back around the coalescing buffer would
    integrate the first batch's rays with the scaled value."""
    map_ = OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean"))
    gm = GpuMap(map_)
    om = make_oracle(map_)
    first, second = wall_rays(100, 1), wall_rays(100, 2)
    cone = RayPatternConical((1.0, 0.0, 0.0), math.radians(60.0), 3.0, math.radians(15.0))
    assert 30 <= cone.rayCount() <= 60
    clearing = ClearingPattern(cone)
    position, rotation = (0.05, 0.05, 0.05), (0.0, 0.0, 0.0, 1.0)
    m = np.float32(map_.missValue())
    launched = gm.batchesLaunched()
    assert gm.integrateRays(first) == 200
    assert gm.batchesLaunched() == launched                    # collected, not launched
    assert clearing.apply(gm, position, rotation, probability_scaling=0.5) == 2 * cone.rayCount()
    assert gm.batchesLaunched() == launched + 2                # the waiting rays, then the pattern
    assert gm.integrateRays(second) == 200
    assert gm.batchesLaunched() == launched + 2                # never merged with the pattern's batch: waiting again
    gm.syncVoxels()
    assert gm.missValue() == float(m) and map_.missValue() == float(m)
    cone_rays = R.build_rays(cone.rayPoints(), [list(position) + list(rotation)])
    om.integrate_occupancy(first)
    before = om.chunks(["occupancy"])
    oracle_lib.oracle_map_set_miss_value(om.handle, float(np.float32(m * np.float32(0.5))))
    om.integrate_occupancy(cone_rays, flags=CLEARING_FLAGS)
    lowered = sum(int(np.count_nonzero(b["occupancy"] != before[k]["occupancy"]))
                  for k, b in om.chunks(["occupancy"]).items() if k in before)
    assert lowered > 0                                         # the pattern met occupied voxels
    oracle_lib.oracle_map_set_miss_value(om.handle, float(m))
    om.integrate_occupancy(second)
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy", "mean"], exact_float=True))
    gm.close()


# ---- 4. / 5. many poses in one batch ------------------------------------------------------------------------------------
def room_rays(n=3000, half=(2.0, 1.5, 1.0)):
    """A small room seen from near its middle: n rays in uniform directions ending on the walls, so that a cone meets
    occupied voxels at different depths."""
    d = synth.rays_c0(n=n, origin=(0.0, 0.0, 0.0), length=1.0, seed=77)[1::2]
    with np.errstate(divide="ignore"):
        t = np.min(np.where(np.abs(d) > 1e-9, np.array(half) / np.abs(d), np.inf), axis=1)
    rays = np.empty((2 * n, 3))
    rays[0::2] = (0.05, 0.05, 0.05)
    rays[1::2] = rays[0::2] + d * t[:, None]
    return rays


def four_poses():
    """Four sensor poses in the room; the third repeats the first, so its rays meet what the first left."""
    poses = np.empty((4, 7))
    for i, (angle, axis) in enumerate([(0.0, (0, 0, 1)), (0.4, (0, 0, 1)), (0.0, (0, 0, 1)), (-0.7, (0.6, 0.0, 0.8))]):
        poses[i, :3] = (0.05 + 0.03 * (i % 2), 0.05 - 0.02 * (i % 2), 0.05)
        poses[i, 3:] = R.angle_axis(angle, axis)
    return poses


def many_poses_case(gpu_map_type, flags):
    """-> (map after apply_many, map after four apply calls, oracle, occupied voxels the pattern freed)."""
    cone = RayPatternConical((1.0, 0.0, 0.0), math.radians(60.0), 5.0, math.radians(15.0))
    poses = four_poses()
    room = room_rays()
    maps = []
    for many in (True, False):
        map_ = OccupancyMap(0.1, (32, 32, 32))
        map_.setMissProbability(0.1)     # two applications free a voxel that was hit once
        gm = gpu_map_type(map_)
        clearing = ClearingPattern(cone)
        clearing.setRayFlags(flags)
        assert gm.integrateRays(room) == room.shape[0]
        if many:
            assert clearing.apply_many(gm, poses) == 4 * 2 * cone.rayCount()
            assert np.array_equal(clearing.lastRaySet(), R.build_rays(cone.rayPoints(), poses))
        else:
            for pose in poses:
                assert clearing.apply(gm, pose[:3], pose[3:]) == 2 * cone.rayCount()
            assert np.array_equal(clearing.lastRaySet(), R.build_rays(cone.rayPoints(), poses[3:]))
        gm.syncVoxels()
        maps.append((map_, gm))
    map_, gm = maps[0]
    om = make_oracle(map_)
    ndt = isinstance(gm, GpuNdtMap)
    if ndt:
        om.set_ndt(sensor_noise=gm.sensor_noise, sample_threshold=gm.sample_threshold, adaptation_rate=gm.adaptation_rate,
                   reinit_threshold=gm.reinitialise_covariance_threshold,
                   reinit_count=gm.reinitialise_covariance_point_count)
    integrate = om.integrate_ndt if ndt else om.integrate_occupancy
    integrate(room)
    before = {k: b["occupancy"].copy() for k, b in om.chunks(["occupancy"]).items()}
    for pose in poses:
        integrate(R.build_rays(cone.rayPoints(), [pose]), flags=int(flags) & ~int(RayFlag.kRfReverseWalk))
    threshold = np.float32(map_.occupancy_threshold_value)
    freed = 0
    for key, block in om.chunks(["occupancy"]).items():
        if key in before:
            was = np.isfinite(before[key]) & (before[key] >= threshold)
            freed += int(np.count_nonzero(was & (block["occupancy"] < threshold)))
    for _, g in maps:
        g.close()
    return maps[0][0], maps[1][0], om, freed


@pytest.mark.parametrize("flags", [CLEARING_FLAGS, int(RayFlag.kRfEndPointAsFree)], ids=["clearing", "end-point-as-free"])
def test_many_poses_in_one_batch(gpu, flags):
    """apply_many with 4 poses == four apply calls == the oracle fed the four ray sets in order, exactly.  The third pose
    repeats the first: its rays meet voxels the first lowered, and free them."""
    many, single, om, freed = many_poses_case(GpuMap, flags)
    assert_parity(compare_maps(om.chunks(), many.chunks, ["occupancy"], exact_float=True))
    assert_parity(compare_maps(om.chunks(), single.chunks, ["occupancy"], exact_float=True))
    assert_parity(compare_maps(single.chunks, many.chunks, ["occupancy"], exact_float=True))
    assert freed > 0


def test_many_poses_ndt(gpu):
    """The same on an NDT map: occupancy exact, the NDT layers at the project's 1e-5."""
    many, single, om, freed = many_poses_case(GpuNdtMap, CLEARING_FLAGS)
    others = [n for n in many.layers if n != "occupancy"]
    for got in (many, single):
        assert_parity(compare_maps(om.chunks(), got.chunks, ["occupancy"], exact_float=True))
        assert_parity(compare_maps(om.chunks(), got.chunks, others, rel=1e-5))
    assert freed > 0


# ---- 6. edges -------------------------------------------------------------------------------------------------------------
def test_edges(gpu):
    map_ = OccupancyMap(0.1, (32, 32, 32))
    map_.setMissProbability(0.1)
    gm = GpuMap(map_)
    om = make_oracle(map_)
    room = room_rays(1500)
    assert gm.integrateRays(room) == room.shape[0]
    om.integrate_occupancy(room)
    gm.wait()
    cone = RayPatternConical((1.0, 0.0, 0.0), math.radians(60.0), 5.0, math.radians(15.0))
    clearing = ClearingPattern(cone)
    poses = four_poses()
    # no pose, and a pattern without rays: nothing integrated, nothing launched
    launched = gm.batchesLaunched()
    assert clearing.apply_many(gm, np.empty((0, 7))) == 0
    assert clearing.lastRaySet().shape == (0, 3)
    empty = ClearingPattern(RayPattern())
    assert empty.apply(gm, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)) == 0
    assert empty.pattern().buildRays((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)).shape == (0, 3)
    assert gm.batchesLaunched() == launched
    # errors
    handle = cone._device_pattern()
    done = C.c_size_t(7)
    assert L.lib.ohmhip_map_apply_pattern(gm._handle, handle, poses.ctypes.data, 1, 2, 1.0, 1.0, 0,
                                          C.byref(done)) == L.ERR_INVALID_ARG and done.value == 0
    assert L.lib.ohmhip_map_apply_pattern(gm._handle, handle, None, 1, 0, 1.0, 1.0, 0, None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_apply_pattern(gm._handle, None, poses.ctypes.data, 1, 0, 1.0, 1.0, 0, None) == L.ERR_INVALID_ARG
    too_many = (1 << 28) // cone.rayCount() + 1     # poses x rays overflows what one batch takes: checked before any read
    assert L.lib.ohmhip_map_apply_pattern(gm._handle, handle, poses.ctypes.data, too_many, 0, 1.0, 1.0, 0,
                                          C.byref(done)) == L.ERR_CAPACITY and done.value == 0
    assert L.lib.ohmhip_pattern_build_rays(handle, poses.ctypes.data, too_many, 0, 1.0, None) == L.ERR_CAPACITY
    assert gm.batchesLaunched() == launched
    # a NaN pose yields NaN rays: the map's ray filter drops them, and `integrated` says so
    with_nan = poses[:2].copy()
    with_nan[1, 4] = np.nan
    nan_rays = R.build_rays(cone.rayPoints(), with_nan)
    assert np.isnan(nan_rays[2 * cone.rayCount():]).any()
    assert clearing.apply_many(gm, with_nan) == 2 * R.filter_good_count(nan_rays) == 2 * cone.rayCount()
    assert np.array_equal(clearing.lastRaySet(), nan_rays, equal_nan=True)
    om.integrate_occupancy(nan_rays, flags=CLEARING_FLAGS)
    # applications straight after one another, no sync in between: the three output buffers are used in turn and the
    # fourth application takes the first buffer again
    for i in range(4):
        launched = gm.batchesLaunched()
        assert clearing.apply(gm, poses[i, :3], poses[i, 3:]) == 2 * cone.rayCount()
        assert gm.batchesLaunched() == launched + 1
        om.integrate_occupancy(R.build_rays(cone.rayPoints(), poses[i:i + 1]), flags=CLEARING_FLAGS)
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy"], exact_float=True))
    # the pattern goes after a sync; the map carries on
    cone.close()
    extra = wall_rays(50, 9)
    assert gm.integrateRays(extra) == 100
    om.integrate_occupancy(extra)
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy"], exact_float=True))
    gm.close()
