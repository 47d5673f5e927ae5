"""-m gpu: the C++ mirror's DeviceRayFilter through the driver (ohm_amd/host/gpumap_driver.cpp, mode occchain): one box
chain -- goodRay(6) then clipBounded on (-1, -1, -0.5)-(2, 1.5, 1) -- set on the device; maps and counts equal the Python
mirror's, and both equal the model's."""
import struct

import numpy as np
import pytest

import cpp_driver
import rayfilter_chain_cases as cases
from ohm_amd import GpuMap, OccupancyMap
from parity import assert_parity, compare_maps

pytestmark = pytest.mark.gpu


def test_cpp_mirror_equals_python_mirror(gpu):
    stages = cases.CHAINS["good_then_clip_bounded"]
    rays = cases.random_rays(1500, seed=31)
    batch = 700
    data = cpp_driver.run("occchain", 0.25, batch, rays)
    total, kept = struct.unpack_from("<QQ", data, 0)
    n = rays.shape[0] // 2
    flags = np.frombuffer(data, dtype=np.uint8, count=n, offset=16)
    cpp_chunks = cpp_driver.read_region_dump(data[16 + n:], 2)

    layers = ("occupancy", "mean")
    map_ = OccupancyMap(0.25, (16, 16, 16), layers=layers)
    gm = GpuMap(map_)
    gm.setRayFilter(cases.device_filter(stages))
    py_keep, _, py_flags = gm.applyRayFilter(rays)
    py_total = sum(gm.integrateRays(rays[at:at + 2 * batch]) for at in range(0, rays.shape[0], 2 * batch))
    gm.syncVoxels()
    m_keep, _, m_flags = cases.run_model(stages, rays)
    assert total == py_total == 2 * int(m_keep.sum()) and kept == int(py_keep.sum()) == int(m_keep.sum())
    assert 0 < kept < n
    assert np.array_equal(flags, py_flags) and np.array_equal(flags, m_flags)
    assert_parity(compare_maps(cpp_chunks, map_.chunks, list(layers), exact_float=True))
    assert_parity(compare_maps(map_.chunks, cpp_chunks, list(layers), exact_float=True))
    gm.close()
