"""-m gpu: LineQueryGpu (line walk on the device + ohmhip_map_clearance_keys) restated from LineQuery.Gpu,
CpuVsGpuSimple and CpuVsGpu (tests/ohmtestgpu/GpuLineQueryTests.cpp:86-239) at EXACT equality of keys and ranges --
against the oracle's walk (calculateSegmentKeys) and the clearance restatement (tests/clearance_ref.py) with
LineQueryGpu::onExecute's post-processing -- plus kQfNearestResult and defaultRange."""
import math
import os
import sys

import numpy as np
import pytest

from ohm_amd import GpuMap, LineQueryGpu, OccupancyMap, QueryFlag

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clearance_ref import QF_UNKNOWN_AS_OCCUPIED, Geometry, clearance_keys  # noqa: E402
from parity import make_oracle  # noqa: E402
from rays_query_ref import ChunkBlocks  # noqa: E402

pytestmark = pytest.mark.gpu


def hit_map(points, resolution=0.1):
    """A map whose only observations are hits at `points` (zero-length rays: integrateHit)."""
    map_ = OccupancyMap(resolution)
    gm = GpuMap(map_)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    assert gm.integrateRays(np.repeat(pts, 2, axis=0)) == 2 * pts.shape[0]
    gm.syncVoxels()
    return map_, gm


def sparse_map():
    """sparseMap (GpuLineQueryTests.cpp): a handful of isolated obstacles around the origin."""
    rng = np.random.default_rng(11)
    pts = rng.uniform(-3.0, 3.0, size=(40, 3))
    pts = np.concatenate([pts, [[0.0, 0.45, 0.0], [1.05, -0.2, 0.1], [-2.0, 0.0, 0.35]]])
    return hit_map(pts)


def box_room(half=5.0, thickness=3, resolution=0.1):
    """ohmgen::boxRoom: the walls of a cube +-half, `thickness` voxels thick."""
    n = int(round(half / resolution))
    c = (np.arange(-n, n) + 0.5) * resolution
    pts = []
    for t in range(thickness):
        for axis in range(3):
            for side in (-1, 1):
                w = side * (half - (t + 0.5) * resolution)
                a, b = np.meshgrid(c, c, indexing="ij")
                p = np.zeros((a.size, 3))
                p[:, axis] = w
                p[:, (axis + 1) % 3] = a.reshape(-1)
                p[:, (axis + 2) % 3] = b.reshape(-1)
                pts.append(p)
    return hit_map(np.concatenate(pts), resolution)


def expected(map_, start, end, radius, flags=0, default_range=-1.0):
    om = make_oracle(map_)
    length = math.dist(start, end)
    keys, _, _ = om.walk(tuple(start), tuple(end), 0, cap=int(length / map_.resolution * 1.8) + 16)
    regions = np.array([k[0] for k in keys], dtype=np.int16).reshape(-1, 3)
    locals_ = np.array([k[1] for k in keys], dtype=np.uint8).reshape(-1, 3)
    geom = Geometry(map_.resolution, map_.region_voxel_dimensions, map_.occupancy_threshold_value)
    uao = QF_UNKNOWN_AS_OCCUPIED if flags & QueryFlag.kQfUnknownAsOccupied else 0
    ranges = clearance_keys(geom, ChunkBlocks(map_.chunks), regions, locals_, radius, uao)
    present = np.array([tuple(int(v) for v in r) in map_.chunks for r in regions], dtype=bool)
    ranges = np.where(present & (ranges >= 0), ranges, np.float32(default_range)).astype(np.float32)
    return regions, locals_, ranges


def run(gm, start, end, radius, flags=0, default_range=None):
    q = LineQueryGpu(gm, start, end, radius, flags)
    if default_range is not None:
        q.setDefaultRange(default_range)
    assert q.execute() and q.wait()
    regions, locals_ = q.intersectedVoxels()
    return q, regions, locals_, q.ranges()


def assert_same(got, want):
    for g, w in zip(got, want):
        assert np.asarray(g).shape == np.asarray(w).shape
        assert np.array_equal(np.asarray(g), np.asarray(w)), (g, w)


def test_line_query_gpu_sparse(gpu):
    """LineQuery.Gpu: lines through the sparse map, with and without unknown-as-occupied."""
    map_, gm = sparse_map()
    for start, end in [((-5.0, 0.0, 0.0), (5.0, 0.0, 0.0)), ((-2.0, -2.0, -2.0), (2.5, 1.5, 2.0)),
                       ((0.0, 3.0, -1.0), (0.2, -3.0, 1.0))]:
        for flags in (0, QueryFlag.kQfUnknownAsOccupied):
            q, regions, locals_, ranges = run(gm, start, end, 2.0, flags)
            want = expected(map_, start, end, 2.0, flags)
            assert_same((regions, locals_, ranges), want)
            assert q.numberOfResults() == len(want[2])
            assert (ranges >= 0).any()


def test_cpu_vs_gpu_simple(gpu):
    """LineQuery.CpuVsGpuSimple: (-5, 0, 0) -> (5, 0, 0), radius 2, exact."""
    map_, gm = sparse_map()
    _, regions, locals_, ranges = run(gm, (-5.0, 0.0, 0.0), (5.0, 0.0, 0.0), 2.0)
    assert_same((regions, locals_, ranges), expected(map_, (-5.0, 0.0, 0.0), (5.0, 0.0, 0.0), 2.0))


def test_cpu_vs_gpu_box_room(gpu):
    """LineQuery.CpuVsGpu: 50 lines (the reference's first, then random within 1.1 x the room) in a box room."""
    map_, gm = box_room()
    rng = np.random.default_rng(0)
    pts = [(-2.5, -1.25, 1.25), (6.0, 6.0, 6.0)] + [tuple(rng.uniform(-5.5, 5.5, 3)) for _ in range(22)]
    for i in range(0, len(pts), 2):
        got = run(gm, pts[i], pts[i + 1], 2.0)[1:]
        assert_same(got, expected(map_, pts[i], pts[i + 1], 2.0))


def test_nearest_result_and_default_range(gpu):
    map_, gm = sparse_map()
    start, end = (-5.0, 0.0, 0.0), (5.0, 0.0, 0.0)
    regions, locals_, ranges = expected(map_, start, end, 0.5, 0, default_range=7.5)
    q, r, l, got = run(gm, start, end, 0.5, 0, default_range=7.5)
    assert_same((r, l, got), (regions, locals_, ranges))
    assert (got == np.float32(7.5)).any() and q.defaultRange() == 7.5
    # kQfNearestResult: the first voxel, then any later one with range >= 0 and (range < closest or closest < 0)
    closest_index, closest = 0, np.float32(-1)
    for i, v in enumerate(ranges):
        if i == 0 or (v >= 0 and (v < closest or closest < 0)):
            closest_index, closest = i, v
    q, r, l, got = run(gm, start, end, 0.5, QueryFlag.kQfNearestResult, default_range=7.5)
    assert q.numberOfResults() == 1
    assert_same((r, l, got), (regions[closest_index:closest_index + 1], locals_[closest_index:closest_index + 1],
                              ranges[closest_index:closest_index + 1]))
    assert got[0] < 7.5
    # default range -1: unobstructed voxels stay -1, the first voxel holds until a non-negative range appears
    regions, locals_, ranges = expected(map_, start, end, 0.5)
    q, r, l, got = run(gm, start, end, 0.5, QueryFlag.kQfNearestResult)
    i = int(np.nonzero(ranges >= 0)[0][np.argmin(ranges[ranges >= 0])]) if (ranges >= 0).any() else 0
    assert got[0] == ranges[i] and tuple(l[0]) == tuple(locals_[i])


def test_line_outside_the_map(gpu):
    """A line through regions the map does not hold: every voxel reports the default range, even with unknown as
    occupied (the clearance of a voxel outside the map is not valid, LineQueryGpu.cpp:139-153)."""
    map_, gm = sparse_map()
    _, _, _, got = run(gm, (40.0, 40.0, 40.0), (42.0, 40.0, 40.0), 1.0, QueryFlag.kQfUnknownAsOccupied, 3.0)
    assert (got == np.float32(3.0)).all() and got.size > 10
