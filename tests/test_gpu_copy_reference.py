"""-m gpu: the reference's Copy.* group (tests/ohmtestgpu/GpuCopyTests.cpp:34-247) restated with its inputs: 131 072 rays
from a default-constructed std::mt19937 (tests/stdrandom.py) from (0.05, 0.05, 0.05) to a shell of radius 9 .. 10,
resolution 0.2, the submap box 0 .. 4.5.  The reference copies from the GPU cache into a host map and compares after a
sync; here both maps are on the device and are compared through ohmhip_map_read_regions."""
import numpy as np
import pytest

import copy_ref as R
from ohm_amd import GpuMap, OccupancyMap, copyFilterDirty, copyFilterExtents, copyMap
from ohm_amd import _lib as L
from oracle.oracle import OracleMap
from stdrandom import Mt19937
from test_gpu_copy import assert_same, keys_of, read_all, spatial_of

pytestmark = pytest.mark.gpu

RAY_COUNT = 1024 * 128
RESOLUTION = 0.2
COPY_MIN, COPY_MAX = (0.0, 0.0, 0.0), (4.5, 4.5, 4.5)


def shell_rays(ray_count=RAY_COUNT, map_extents=10.0, noise=1.0):
    """GpuCopyTests.cpp:45-59: per ray three draws of unit_rand(-1, 1) and one of length_rand(extents - noise, extents)
    from the same engine; glm::normalize is v * (1 / sqrt(dot(v, v)))."""
    u = Mt19937().uniform(0.0, 1.0, 4 * ray_count).reshape(-1, 4)
    v = u[:, :3] * (1.0 - -1.0) + -1.0
    length = u[:, 3] * (map_extents - (map_extents - noise)) + (map_extents - noise)
    dot = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    ends = v * (1.0 / np.sqrt(dot))[:, None] * length[:, None]
    rays = np.empty((2 * ray_count, 3))
    rays[0::2] = 0.05
    rays[1::2] = ends
    return rays


@pytest.fixture(scope="module")
def source(gpu):
    """The populated source map, shared and never changed by a copy (C6)."""
    src = GpuMap(OccupancyMap(RESOLUTION))
    rays = shell_rays()
    assert src.integrateRays(rays) == len(rays)
    return src, read_all(src)


def test_copy_from_gpu(source):
    src, data = source
    dst = GpuMap(OccupancyMap(RESOLUTION))
    assert copyMap(dst, src)
    assert len(data) >= 27
    assert_same(read_all(dst), data)
    assert any(np.any(~np.isinf(b["occupancy"])) for b in data.values())  # (GpuCopyTests.cpp:102-103: something observed)


def test_copy_submap_from_gpu(source):
    src, data = source
    dst = GpuMap(OccupancyMap(RESOLUTION))
    assert copyMap(dst, src, copyFilterExtents(COPY_MIN, COPY_MAX))
    want, _ = R.select_regions(list(data), spatial_of(src), extents=(COPY_MIN, COPY_MAX))
    assert 0 < len(want) < len(data)
    assert sorted(keys_of(dst)) == sorted(want)
    assert_same(read_all(dst), {k: data[k] for k in want})


def test_copy_updated(gpu):
    src = GpuMap(OccupancyMap(RESOLUTION))
    dst = GpuMap(OccupancyMap(RESOLUTION))
    rays = shell_rays()
    assert src.integrateRays(rays) == len(rays)
    # "Get the map stamp now" (:184): the device map keeps dirty bits, the stamp is clear_dirty
    L.check(L.lib.ohmhip_map_clear_dirty(src._handle), "clear_dirty")
    assert copyMap(dst, src, copyFilterDirty())
    assert keys_of(dst) == []
    # a ray that goes nowhere for every voxel of region (0, 0, 0) (:191-210)
    om = OracleMap(RESOLUTION)
    centres = np.array([om.voxel_centre((0, 0, 0), (x, y, z)) for z in range(32) for y in range(32) for x in range(32)])
    blat = np.repeat(centres, 2, axis=0)
    assert src.integrateRays(blat) == len(blat)
    assert copyMap(dst, src, copyFilterDirty())
    assert keys_of(dst) == [(0, 0, 0)]
    assert_same(read_all(dst), read_all(src, keys=[(0, 0, 0)]))
