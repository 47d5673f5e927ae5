"""-m gpu: ohm::RaysQueryGpu of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver raysquery`: the map is
built by ohm::GpuMap::integrateRays from the first half of the rays (collected by batch coalescing when the query
comes), the second half queries it through addRay / executeAsync / wait.  Every result equals the CPU query's."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from ohm_amd import OccupancyMap, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from parity import make_oracle  # noqa: E402
from rays_query_ref import rays_query  # noqa: E402

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ohm_amd", "lib", "gpumap_driver")


def test_cpp_rays_query_gpu(gpu):
    build = synth.random_rays(2000, extent=6.0, seed=81)
    query = build.copy()
    query[1::2] *= 1.2
    rays = np.concatenate([build, query])
    assert os.path.exists(DRIVER), "gpumap_driver missing: run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as tmp:
        rp, op = os.path.join(tmp, "rays.bin"), os.path.join(tmp, "out.bin")
        with open(rp, "wb") as f:
            f.write(struct.pack("<Q", rays.shape[0]))
            f.write(np.ascontiguousarray(rays, dtype=np.float64).tobytes())
        res = subprocess.run([DRIVER, "raysquery", "0.1", "0", rp, op], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
        data = open(op, "rb").read()
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
