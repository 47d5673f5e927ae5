"""-m gpu: ohm::RayPattern / ClearingPattern of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver clearing`:
RayPattern.Clearing as the reference writes it (tests/ohmtestgpu/GpuRayPatternTests.cpp:28-85).  After each of the 20
applications the occupancy words equal the CPU oracle's, fed the model's rays; lastRaySet() returns the model's rays."""
import math

import numpy as np
import pytest

import cpp_driver
import ray_pattern_ref as R
from ohm_amd import ClearingPattern, OccupancyMap
from parity import make_oracle

pytestmark = pytest.mark.gpu


def test_cpp_ray_pattern_clearing(gpu):
    map_ = OccupancyMap(0.1, (32, 32, 32))
    map_.setHitProbability(0.51)
    map_.setMissProbability(0.0)
    om = make_oracle(map_)
    hit = np.float32(map_.hit_value)
    translate = om.voxel_centre((0, 0, 0), (0, 0, 0))
    data = cpp_driver.run("clearing", 0.1, 0, None, *[repr(float(v)) for v in translate])
    rec = np.dtype([("rays", "<f8", (2, 3)), ("integrated", "<u8"), ("row", "<f4", 32)])
    assert len(data) == 20 * rec.itemsize + 4 * 32768 + 4
    got = np.frombuffer(data, dtype=rec, count=20)
    final = np.frombuffer(data, dtype=np.float32, count=32768, offset=20 * rec.itemsize)
    miss_after = np.frombuffer(data, dtype=np.float32, count=1, offset=20 * rec.itemsize + 4 * 32768)[0]
    # the oracle: the line written directly, then the model's ray 20 times under the clearing flags
    c = np.array(om.voxel_centre((0, 0, 0), (16, 16, 16)))
    om.integrate_occupancy(np.array([c, c]))
    tile = np.full(32768, np.inf, dtype=np.float32)
    tile[:20] = hit
    om.region_layer_view((0, 0, 0), "occupancy")[:] = tile
    pose = list(translate) + list(R.angle_axis(-0.5 * math.pi, (0.0, 0.0, 1.0)))
    rays = R.build_rays([(0.0, 0.0, 0.0), (0.0, map_.resolution * 20, 0.0)], [pose])
    threshold = np.float32(map_.occupancy_threshold_value)
    for i in range(20):
        om.integrate_occupancy(rays, flags=int(ClearingPattern.kDefaultRayFlags))
        row = om.region_layer((0, 0, 0), "occupancy")[:32]
        assert np.array_equal(got["rays"][i], rays), i
        assert got["integrated"][i] == 2
        assert np.array_equal(got["row"][i].view(np.uint32), row.view(np.uint32)), i
        assert np.isfinite(got["row"][i][i]) and got["row"][i][i] < threshold      # voxel i is no longer occupied
        assert np.all(got["row"][i][i + 1:20] == hit)                              # the ray stopped there
    assert np.array_equal(final.view(np.uint32), om.region_layer((0, 0, 0), "occupancy").view(np.uint32))
    assert miss_after == np.float32(map_.miss_value)                               # GpuMap::missValue() is unchanged
