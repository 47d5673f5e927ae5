"""-m gpu: the ohm::Query surface of the C++ mirror's four query classes (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver
queryapi` on the smallest map that still answers -- 8 rays inside one 32^3 region at resolution 0.1 -- and held to
constants: which queries force kQfGpuEvaluate, what execute / executeAsync / wait return, what a soft and a hard reset
leave, and that a query without a map refuses to run."""
import numpy as np
import pytest

import cpp_driver

pytestmark = pytest.mark.gpu

QF_GPU_EVALUATE = 1 << 2
#                 flags after construction with 0, after setQueryFlags(0); execute(), executeAsync(), wait();
#                 numberOfResults() after execute(), after reset(false), after another execute(), after reset(true)
SURFACE = {
    "LineKeysQueryGpu": (0, 0, 1, 1, 1, 8, 0, 8, 0),                              # one result per ray
    "RaysQueryGpu": (QF_GPU_EVALUATE, QF_GPU_EVALUATE, 1, 1, 1, 8, 0, 8, 0),      # one result per ray
    "LineQueryGpu": (QF_GPU_EVALUATE, QF_GPU_EVALUATE, 1, 1, 1, 5, 0, 5, 0),      # 5 voxels from centre to centre, +4 in x
    "NearestNeighbours": (0, 0, 1, 0, 1, 1, 0, 1, 0),                             # no async form; one voxel in reach
}
# RaysQueryGpu::numberOfRays() after reset(false) and after reset(true); LineKeysQueryGpu::rayPointCount() after
# reset(true); LineKeysQueryGpu::ranges() == nullptr; execute() without a map: LineKeysQueryGpu, RaysQueryGpu
EXTRAS = (8, 0, 16, 1, 0, 0)


def test_cpp_query_surface(gpu):
    # every ray from the centre of one voxel to the centre of another, all in region (0, 0, 0); the end points are more
    # than the neighbour search radius (0.25) apart and no ray passes through another ray's end voxel
    start = (0.05, 0.05, 0.05)
    rays = np.array([p for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)
                     for p in (start, (0.85 * sx, 0.35 * sy, 0.15 * sz))])
    assert rays.shape == (16, 3) and np.abs(rays).max() < 1.6
    got = np.frombuffer(cpp_driver.run("queryapi", 0.1, 0, rays, timeout=120), dtype="<u4")
    assert len(got) == 9 * len(SURFACE) + len(EXTRAS)
    for i, (name, want) in enumerate(SURFACE.items()):
        assert tuple(int(v) for v in got[9 * i:9 * i + 9]) == want, name
    assert tuple(int(v) for v in got[9 * len(SURFACE):]) == EXTRAS
