"""-m gpu: ohm::RaysQueryGpu of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver raysquery`: the map is
built by ohm::GpuMap::integrateRays from the first half of the rays (collected by batch coalescing when the query
comes), the second half queries it through addRay / executeAsync / wait.  Every result equals the CPU query's."""
import struct

import numpy as np
import pytest

import cpp_driver
from ohm_amd import OccupancyMap, synth
from parity import make_oracle
from rays_query_ref import rays_query

pytestmark = pytest.mark.gpu


def test_cpp_rays_query_gpu(gpu):
    build = synth.random_rays(2000, extent=6.0, seed=81)
    query = build.copy()
    query[1::2] *= 1.2
    rays = np.concatenate([build, query])
    data = cpp_driver.run("raysquery", 0.1, 0, rays)
    (n,) = struct.unpack_from("<Q", data, 0)
    assert n == 2000
    rec = np.dtype([("range", "<f8"), ("volume", "<f8"), ("type", "<i4"), ("region", "<i2", 3), ("local", "u1", 3)])
    assert len(data) == 8 + n * rec.itemsize
    got = np.frombuffer(data, dtype=rec, count=n, offset=8)
    map_ = OccupancyMap(0.1)
    om = make_oracle(map_)
    om.integrate_occupancy(build)
    (ranges, volumes, types, regions, locals_), _ = rays_query(om, query, map_.occupancy_threshold_value)
    assert np.array_equal(got["range"], ranges)
    assert np.array_equal(got["volume"], volumes)
    assert np.array_equal(got["type"], types.astype(np.int32))
    assert np.array_equal(got["region"], regions)
    assert np.array_equal(got["local"], locals_)
    assert (types == 1).sum() > 100
