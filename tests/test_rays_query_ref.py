"""RaysQuery.Cpu (tests/ohmtest/RaysQueryTests.cpp) restated against the CPU query helper (tests/rays_query_ref.py),
which the device query is held to: terminal types, ranges to the analytic lengths, unobserved volume before and after
integration.  Plus the two reference behaviours the helper carries over: a filtered ray, and the terminal type / key that
a ray visiting no voxel inherits from the last ray that visited one (ohm/RaysQuery.cpp:116-117)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle.oracle import OracleMap  # noqa: E402
from rays_query_ref import K_FREE, K_NULL, K_OCCUPIED, K_UNOBSERVED, NULL_KEY, filter_ray, rays_query  # noqa: E402

BASE_SCALE = 10.0
QUERY_SCALE = (1.2, 1.2, 0.6)
THRESHOLD = 0.0  # probability_to_value(0.5)
_DIRS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 1, 0), (0, 1, 1), (1, 0, 1),
         (-1, -1, 0), (0, -1, -1), (-1, 0, -1), (1, 1, 1), (-1, -1, -1)]


def reference_rays():
    """RaysQueryTests.cpp:25-41: 14 axis / diagonal rays from the origin, 10 m per axis."""
    rays = np.zeros((2 * len(_DIRS), 3))
    rays[1::2] = np.array(_DIRS, dtype=np.float64) * BASE_SCALE
    return rays


def scaled(rays, scale):
    out = rays.copy()
    out[1::2] *= scale
    return out


def hits_only(rays):
    """integrateHit(map, voxelKey(sample)) for every sample: zero-length rays, which apply the sample update only."""
    out = np.repeat(rays[1::2], 2, axis=0)
    return out


def aabb_entry(origin, end, centre, half):
    """ohm::Aabb::rayIntersect entry time of the ray origin -> end against the voxel box (slab method)."""
    d = np.asarray(end, float) - np.asarray(origin, float)
    d = d / np.linalg.norm(d)
    t_near = -math.inf
    for a in range(3):
        if d[a] == 0:
            continue
        t1 = (centre[a] - half - origin[a]) / d[a]
        t2 = (centre[a] + half - origin[a]) / d[a]
        t_near = max(t_near, min(t1, t2))
    return t_near


def test_rays_query_cpu_restated():
    om = OracleMap(0.1)
    rays = reference_rays()
    om.integrate_occupancy(hits_only(rays))
    expected_type = (K_OCCUPIED, K_OCCUPIED, K_FREE)
    for iteration, scale in enumerate(QUERY_SCALE):
        q = scaled(rays, scale)
        (ranges, volumes, types, regions, locals_), _ = rays_query(om, q, THRESHOLD)
        assert ranges.shape[0] == len(_DIRS)
        for i in range(len(_DIRS)):
            if iteration > 0:
                assert volumes[i] == 0.0, (iteration, i)
            else:
                assert volumes[i] > 0.0, (iteration, i)
            if iteration < 2:
                length = float(np.linalg.norm(rays[2 * i + 1] - rays[2 * i]))
                if types[i] == K_OCCUPIED:
                    key = om.voxel_key(rays[2 * i + 1])
                    centre = om.voxel_centre(*key)
                    length = aabb_entry(rays[2 * i], rays[2 * i + 1], centre, 0.05)
                    assert (tuple(regions[i]), tuple(locals_[i])) == key
            else:
                length = float(np.linalg.norm(q[2 * i + 1] - q[2 * i]))
            assert abs(ranges[i] - length) <= 1e-5, (iteration, i, ranges[i], length)
            assert types[i] == expected_type[iteration], (iteration, i, types[i])
        if iteration == 0:
            om.integrate_occupancy(rays)


def test_unobserved_volume_is_the_cone_sum():
    """An empty map: every voxel is unobserved, the volume telescopes to coef * length^3 (up to rounding)."""
    om = OracleMap(0.1)
    rays = np.array([[0.01, 0.02, 0.03], [3.0, 1.0, -2.0]])
    (ranges, volumes, types, _, _), visits = rays_query(om, rays, THRESHOLD, volume_coefficient=0.5)
    length = float(np.linalg.norm(rays[1] - rays[0]))
    assert visits > 10
    assert types[0] == K_UNOBSERVED
    assert ranges[0] == float(np.float32(length))
    assert abs(volumes[0] - 0.5 * length ** 3) <= 1e-9 * length ** 3


def test_filtered_ray_and_terminal_carry():
    """A filtered ray reports (0, 0, kNull, Key::kNull) and leaves the carried terminal state alone; a ray that passes
    the filter but visits no voxel (its end key is null: beyond +-32767 regions) repeats the terminal type and key of
    the last ray that visited one -- kNull / Key::kNull before any."""
    om = OracleMap(0.1)
    far = 32768 * 3.2 + 10.0  # region coordinate beyond the int16 range: Key::kNull
    rays = np.array([
        [0.0, 0.0, 0.0], [far, 0.0, 0.0],          # 0: passes, visits nothing, nothing to carry yet
        [0.05, 0.05, 0.05], [1.0, 0.5, 0.25],       # 1: walked, unobserved end
        [np.nan, 0.0, 0.0], [1.0, 1.0, 1.0],        # 2: filtered
        [0.0, 0.0, 0.0], [far, 0.0, 0.0],          # 3: carries ray 1's terminal state
        [0.0, 0.0, 0.0], [0.0, -far, 0.0],         # 4: again
    ])
    (ranges, volumes, types, regions, locals_), _ = rays_query(om, rays, THRESHOLD)
    assert (types[0], ranges[0], volumes[0]) == (K_NULL, 0.0, 0.0)
    assert (tuple(regions[0]), tuple(locals_[0])) == NULL_KEY
    assert types[1] == K_UNOBSERVED and volumes[1] > 0
    key1 = (tuple(regions[1]), tuple(locals_[1]))
    assert key1 == om.voxel_key(rays[3])
    assert (types[2], ranges[2], volumes[2]) == (K_NULL, 0.0, 0.0)
    assert (tuple(regions[2]), tuple(locals_[2])) == NULL_KEY
    for i in (3, 4):
        assert (types[i], ranges[i], volumes[i]) == (K_UNOBSERVED, 0.0, 0.0)
        assert (tuple(regions[i]), tuple(locals_[i])) == key1


def test_clip_filter_walks_the_clipped_ray():
    om = OracleMap(0.1)
    rays = np.array([[0.0, 0.0, 0.0], [30.0, 40.0, 0.0]])
    (ranges, _, types, regions, locals_), _ = rays_query(om, rays, THRESHOLD, ray_filter=("clip", 5.0))
    ok, _, end = filter_ray(("clip", 5.0), tuple(rays[0]), tuple(rays[1]))
    assert ok and end == pytest.approx((3.0, 4.0, 0.0))
    assert types[0] == K_UNOBSERVED
    assert (tuple(regions[0]), tuple(locals_[0])) == om.voxel_key(end)
    assert ranges[0] == float(np.float32(5.0)) or abs(ranges[0] - 5.0) < 1e-6
    (_, _, types_good, _, _), _ = rays_query(om, rays, THRESHOLD, ray_filter=("good", 5.0))
    assert types_good[0] == K_NULL


def test_strict_threshold():
    """A voxel whose value equals the threshold is free (`>`, not the reference GPU kernel's `>=`)."""
    om = OracleMap(0.1)
    rays = np.array([[0.05, 0.05, 0.05], [0.95, 0.05, 0.05]])
    om.integrate_occupancy(rays)
    key = om.voxel_key(rays[1])
    block = om.region_layer_view(key[0], "occupancy")
    lx, ly, lz = key[1]
    idx = lx + ly * 32 + lz * 32 * 32
    thr = np.float32(0.25)
    block[idx] = thr
    (_, _, types, _, _), _ = rays_query(om, rays, thr)
    assert types[0] == K_FREE
    block[idx] = np.nextafter(thr, np.float32(np.inf))
    (_, _, types, _, _), _ = rays_query(om, rays, thr)
    assert types[0] == K_OCCUPIED
