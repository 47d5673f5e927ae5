"""-m gpu: ohm::Heightmap of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver heightmap`: the map
(occupancy + mean) is built by ohm::GpuMap::integrateRays in small batches -- still collected by batch coalescing when
the heightmap is asked for -- and the three arrays it writes equal the CPU restatement's (tests/heightmap_ref.py)."""
import struct

import numpy as np
import pytest

import cpp_driver
import heightmap_ref as R
from heightmap_cases import two_level_scene
from ohm_amd import OccupancyMap
from parity import make_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("min_clearance,virtual", [(0.0, False), (1.5, True)])
def test_cpp_heightmap(gpu, min_clearance, virtual):
    rays = two_level_scene()
    data = cpp_driver.run("heightmap", 0.1, 4096, rays, min_clearance, int(virtual))
    ma, mb, populated, cells, has_mean = struct.unpack_from("<IIQQB", data, 0)
    n = ma * mb
    assert has_mean == 1 and len(data) == 25 + n * (4 + 24 + 8)
    occupancy = np.frombuffer(data, dtype=np.float32, count=n, offset=25).reshape(mb, ma)
    voxels = np.frombuffer(data, dtype=R.HEIGHTMAP_VOXEL, count=n, offset=25 + 4 * n).reshape(mb, ma)
    mean = np.frombuffer(data, dtype=np.uint32, count=2 * n, offset=25 + 28 * n).reshape(mb, ma, 2)
    layers = ("occupancy", "mean")
    map_ = OccupancyMap(0.1, layers=layers)
    om = make_oracle(map_)
    om.integrate_occupancy(rays)
    src = R.Source(0.1, (32, 32, 32), om.chunks(), map_.occupancy_threshold_value, has_mean=True)
    want = R.build_heightmap(src, R.Params(0.1, min_clearance, virtual_surface=virtual))
    assert (want.occupancy == 1.0).any() and (not virtual or (want.occupancy == -1.0).any())
    assert (ma, mb) == (want.ma, want.mb)
    assert np.array_equal(occupancy.view(np.uint32), want.occupancy.view(np.uint32))
    assert np.array_equal(voxels.view(np.uint8), want.voxels.view(np.uint8))
    assert np.array_equal(mean, want.mean)
    assert populated == want.populated and cells == int((want.source_column != R.NO_COLUMN).sum())
