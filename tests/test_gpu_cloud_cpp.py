"""-m gpu: ohm::extractCloud of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver cloud`: the map
(occupancy + mean) is built by ohm::GpuMap::integrateRays in small batches -- still collected by batch coalescing when
the cloud is asked for -- and the three arrays it writes equal the CPU restatement's (tests/cloud_ref.py)."""
import struct

import numpy as np
import pytest

import cloud_ref as CR
import cpp_driver
from heightmap_cases import two_level_scene
from ohm_amd import OccupancyMap
from parity import make_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("export_free", [False, True])
def test_cpp_cloud(gpu, export_free):
    rays = two_level_scene()
    data = cpp_driver.run("cloud", 0.1, 4096, rays, int(export_free))
    count, n = struct.unpack_from("<QQ", data, 0)
    assert count == n and len(data) == 16 + n * (24 + 10 + 4)
    positions = np.frombuffer(data, dtype=np.float64, count=3 * n, offset=16).reshape(n, 3)
    keys = np.frombuffer(data, dtype=CR.GPU_KEY, count=n, offset=16 + 24 * n)
    values = np.frombuffer(data, dtype=np.float32, count=n, offset=16 + 34 * n)
    layers = ("occupancy", "mean")
    map_ = OccupancyMap(0.1, layers=layers)
    om = make_oracle(map_)
    om.integrate_occupancy(rays)
    want = CR.extract(om.chunks(), 0.1, (32, 32, 32), (0.0, 0.0, 0.0), map_.occupancy_threshold_value, layers,
                      CR.Params(export_free=export_free))
    assert 0 < want.count < want.considered
    assert count == want.count
    assert np.array_equal(keys.view(np.uint8), want.keys.view(np.uint8))
    assert np.array_equal(values.view(np.uint32), want.values.view(np.uint32))
    assert np.array_equal(positions.view(np.uint64), want.positions.view(np.uint64))
