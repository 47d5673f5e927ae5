"""-m gpu: the C++14 host mirror's point filter (ohm_amd/host/OhmGpuMap.h: GpuMap::filterPoints), driven by gpumap_driver
on an occupancy + mean map of ~2 000 rays -- integrated by ohm::GpuMap::integrateRays in batches that batch coalescing
still holds when the filter is asked -- against the Python mirror on the same rays and points: the same bytes."""
import struct

import numpy as np
import pytest

import cpp_driver
from ohm_amd import GPU_KEY_DTYPE, GpuMap, OccupancyMap

pytestmark = pytest.mark.gpu


def run_driver(rays, *args):
    return cpp_driver.run("filter", 0.1, 512, rays, *args)


@pytest.mark.parametrize("args", [(), (0.5, 0), (-1.0, 1)])
def test_cpp_filter_points(gpu, args):
    rng = np.random.default_rng(21)
    ends = np.zeros((2000, 3))
    ends[:, :2] = rng.uniform(-3.0, 3.0, size=(2000, 2))
    ends[:, 2] = rng.uniform(-0.3, 0.1, size=2000)
    rays = np.empty((4000, 3))
    rays[0::2] = (0.1, -0.2, 1.4)
    rays[1::2] = ends
    data = run_driver(rays, *args)
    n, n_kept = struct.unpack_from("<QQ", data, 0)
    assert n == 4000 and len(data) == 16 + n + 8 * n_kept + 8 * n + 10 * n
    status = np.frombuffer(data, dtype=np.uint8, count=n, offset=16)
    kept = np.frombuffer(data, dtype=np.uint64, count=n_kept, offset=16 + n)
    values = np.frombuffer(data, dtype=np.float64, count=n, offset=16 + n + 8 * n_kept)
    keys = np.frombuffer(data, dtype=GPU_KEY_DTYPE, count=n, offset=16 + 9 * n + 8 * n_kept)

    gm = GpuMap(OccupancyMap(0.1, layers=("occupancy", "mean")))
    assert gm.integrateRays(rays) == rays.shape[0]
    shifted = ends.copy()
    shifted[:, 0] += 0.35
    tolerance, occupancy_only = (args + (-1.0, 0))[:2] if args else (-1.0, 0)
    want = gm.filterPoints(np.concatenate([ends, shifted]), tolerance, bool(occupancy_only))
    assert np.array_equal(status, want[0]) and np.array_equal(kept, want[1])
    assert np.array_equal(values.view(np.uint64), want[2].view(np.uint64))
    assert np.array_equal(keys.view(np.uint8), want[3].view(np.uint8))
    assert 0 < n_kept < n and (status[:2000] == 1).sum() > (status[2000:] == 1).sum()
