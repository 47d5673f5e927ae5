"""-m gpu: the C++14 host mirror's point queries (ohm_amd/host/OhmGpuMap.h: GpuMap::nearestNeighbours / voxelKeys /
readVoxels / occupancyTypes and the ohm::NearestNeighbours query class), driven by gpumap_driver on the two-level scene
-- integrated by ohm::GpuMap::integrateRays in batches that batch coalescing still holds when the first query is asked --
against the CPU restatement (tests/neighbours_ref.py) over the oracle's map, at exact equality."""
import struct

import numpy as np
import pytest

import cpp_driver
import neighbours_ref as NR
from heightmap_cases import two_level_scene
from ohm_amd import OccupancyMap
from parity import make_oracle

pytestmark = pytest.mark.gpu
LAYERS = ("occupancy", "mean")


@pytest.fixture(scope="module")
def scene(gpu):
    rays = two_level_scene()
    map_ = OccupancyMap(0.1, layers=LAYERS)
    om = make_oracle(map_)
    om.integrate_occupancy(rays)
    return rays, map_, om, om.chunks()


def run_driver(mode, rays, *args):
    return cpp_driver.run(mode, 0.1, 4096, rays, *args)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_cpp_neighbours(scene, flags):
    rays, map_, om, chunks = scene
    points = rays[1::2][::97]
    data = run_driver("neighbours", rays, 0.25, flags)
    nq, n = struct.unpack_from("<QQ", data, 0)
    assert nq == len(points)
    counts = np.frombuffer(data, dtype=np.uint64, count=nq, offset=16)
    keys = np.frombuffer(data, dtype=NR.GPU_KEY, count=n, offset=16 + 8 * nq)
    ranges = np.frombuffer(data, dtype=np.float32, count=n, offset=16 + 8 * nq + 10 * n)
    blocks = {k: c["occupancy"] for k, c in chunks.items()}
    want = NR.nearest_neighbours(blocks, 0.1, (32, 32, 32), (0.0, 0.0, 0.0), map_.occupancy_threshold_value, points,
                                 np.float32(0.25), flags)
    assert want[0].sum() > nq // 2
    assert np.array_equal(counts, want[0])
    assert np.array_equal(keys.view(np.uint8), want[1].view(np.uint8))
    assert np.array_equal(ranges.view(np.uint32), want[2].view(np.uint32))
    # the query object, for the first point
    at = 16 + 8 * nq + 14 * n
    (n_query,) = struct.unpack_from("<Q", data, at)
    record = np.dtype([("region", "<i2", (3,)), ("local", "u1", (3,)), ("range", "<f8")])
    assert record.itemsize == 17 and len(data) == at + 8 + 17 * n_query
    results = np.frombuffer(data, dtype=record, count=n_query, offset=at + 8)
    first = int(want[0][0])
    assert n_query == first > 0
    assert np.array_equal(results["region"], want[1]["region"][:first])
    assert np.array_equal(results["local"], want[1]["voxel"][:first, :3])
    assert np.array_equal(results["range"], want[2][:first].astype(np.float64))


def test_cpp_voxels(scene):
    rays, map_, om, chunks = scene
    points = rays[1::2][::97]
    data = run_driver("voxels", rays)
    (n,) = struct.unpack_from("<Q", data, 0)
    assert n == len(points) and len(data) == 8 + n * (10 + 4 + 8 + 1 + 1)
    keys = np.frombuffer(data, dtype=NR.GPU_KEY, count=n, offset=8)
    occupancy = np.frombuffer(data, dtype=np.float32, count=n, offset=8 + 10 * n)
    mean = np.frombuffer(data, dtype=np.uint32, count=2 * n, offset=8 + 14 * n).reshape(n, 2)
    present = np.frombuffer(data, dtype=np.uint8, count=n, offset=8 + 22 * n)
    types = np.frombuffer(data, dtype=np.int8, count=n, offset=8 + 23 * n)
    want_occupancy = np.zeros(n, dtype=np.float32)
    want_mean = np.zeros((n, 2), dtype=np.uint32)
    for i, p in enumerate(points):
        region, local = om.voxel_key(p)
        assert tuple(keys[i]["region"]) == region and tuple(keys[i]["voxel"][:3]) == local and keys[i]["voxel"][3] == 0
        index = local[0] + 32 * local[1] + 1024 * local[2]
        want_occupancy[i] = chunks[region]["occupancy"][index]
        want_mean[i] = np.asarray(chunks[region]["mean"], dtype=np.uint32).reshape(-1, 2)[index]
    assert present.all()
    assert np.array_equal(occupancy.view(np.uint32), want_occupancy.view(np.uint32))
    assert np.array_equal(mean, want_mean) and (mean[:, 1] > 0).all()
    assert np.array_equal(types, NR.occupancy_types(occupancy, present, map_.occupancy_threshold_value))
    assert (types == 1).sum() > n // 2
