"""-m gpu: ohm::Mapper + ohm::ClearanceProcess::update of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by
`gpumap_driver clearanceupdate`, give the clearance layer the Python path gives, bit for bit."""
import struct

import numpy as np
import pytest

import cpp_driver
from ohm_amd import ClearanceProcess, GpuMap, Mapper, MappingProcessResult, OccupancyMap, QueryFlag, synth

pytestmark = pytest.mark.gpu


def drive(rays, batch_rays, radius, flags, budget, dim):
    data = cpp_driver.run("clearanceupdate", 0.1, batch_rays, rays, radius, flags, budget, dim, timeout=600)
    (n,) = struct.unpack_from("<Q", data, 0)
    rec = np.dtype([("key", "<i2", 3), ("block", "<f4", dim ** 3)])
    assert len(data) == 8 + n * rec.itemsize
    return np.frombuffer(data, dtype=rec, count=n, offset=8)


@pytest.mark.parametrize("flags,dim", [(0, 32), (int(QueryFlag.kQfUnknownAsOccupied), 16)])
def test_cpp_clearance_update_matches_python(gpu, flags, dim):
    rays = synth.random_rays(6000, extent=4.0, seed=1201 + dim)
    radius, batch = 0.45, 1000
    got = drive(rays, batch, radius, flags, 2, dim)
    map_ = OccupancyMap(0.1, (dim, dim, dim))
    ClearanceProcess.ensureClearanceLayer(map_)
    gm = GpuMap(map_)
    mapper = Mapper(gm)
    mapper.addProcess(ClearanceProcess(radius, flags | int(QueryFlag.kQfGpuEvaluate)))
    for i in range(0, rays.shape[0], 2 * batch):
        assert gm.integrateRays(rays[i:i + 2 * batch]) == min(2 * batch, rays.shape[0] - i)
        mapper.update(1e-9, max_regions=2)
    assert mapper.update(0.0) == MappingProcessResult.kMprUpToDate
    gm.syncVoxels()
    keys = sorted(map_.chunks)
    assert [tuple(int(v) for v in k) for k in got["key"]] == keys
    want = np.stack([map_.chunks[k]["clearance"] for k in keys])
    assert np.array_equal(got["block"].view(np.uint32), want.view(np.uint32))
    assert (want == 0).any() and (want > 0).any()
