"""-m gpu: ohm::ClearanceProcess and ohm::LineQueryGpu of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by
`gpumap_driver clearance` and `gpumap_driver linequery`, against the clearance restatement (tests/clearance_ref.py) at
exact equality."""
import struct

import numpy as np
import pytest

import cpp_driver
from clearance_ref import QF_UNKNOWN_AS_OCCUPIED, Geometry, clearance_keys, clearance_regions
from ohm_amd import OccupancyMap, synth
from parity import make_oracle
from rays_query_ref import OracleBlocks

pytestmark = pytest.mark.gpu


def drive(mode, rays, radius, flags, query_lines=0):
    return cpp_driver.run(mode, 0.1, query_lines, rays, radius, flags, timeout=600)


def oracle_map(rays):
    map_ = OccupancyMap(0.1)
    om = make_oracle(map_)
    om.integrate_occupancy(rays)
    return map_, om


@pytest.mark.parametrize("flags", [0, QF_UNKNOWN_AS_OCCUPIED])
def test_cpp_clearance_process(gpu, flags):
    rays = synth.random_rays(1500, extent=3.0, seed=131 + flags)
    data = drive("clearance", rays, 0.35, flags)
    (n,) = struct.unpack_from("<Q", data, 0)
    rec = np.dtype([("key", "<i2", 3), ("block", "<f4", 32 ** 3)])
    assert n > 0 and len(data) == 8 + n * rec.itemsize
    got = np.frombuffer(data, dtype=rec, count=n, offset=8)
    map_, om = oracle_map(rays)
    geom = Geometry(0.1, (32, 32, 32), map_.occupancy_threshold_value)
    keys = got["key"]
    sample = list(range(0, n, max(1, n // 4)))[:4]
    want = clearance_regions(geom, OracleBlocks(om), keys[sample], 0.35, flags)
    assert np.array_equal(got["block"][sample].reshape(want.shape), want)
    assert (got["block"] == 0).any() and (got["block"] > 0).any()


def test_cpp_line_query(gpu):
    build = synth.random_rays(1500, extent=3.0, seed=141)
    rng = np.random.default_rng(3)
    lines = rng.uniform(-3.0, 3.0, size=(20, 3))
    rays = np.concatenate([build, lines])
    data = drive("linequery", rays, 0.5, QF_UNKNOWN_AS_OCCUPIED, query_lines=10)
    (n_lines,) = struct.unpack_from("<Q", data, 0)
    assert n_lines == 10
    map_, om = oracle_map(build)
    geom = Geometry(0.1, (32, 32, 32), map_.occupancy_threshold_value)
    blocks = OracleBlocks(om)
    off = 8
    rec = np.dtype([("region", "<i2", 3), ("local", "u1", 3), ("range", "<f4")])
    for i in range(n_lines):
        (count,) = struct.unpack_from("<I", data, off)
        off += 4
        got = np.frombuffer(data, dtype=rec, count=count, offset=off)
        off += count * rec.itemsize
        start, end = tuple(lines[2 * i]), tuple(lines[2 * i + 1])
        keys, _, _ = om.walk(start, end, 0, cap=4096)
        regions = np.array([k[0] for k in keys], dtype=np.int16).reshape(-1, 3)
        locals_ = np.array([k[1] for k in keys], dtype=np.uint8).reshape(-1, 3)
        ranges = clearance_keys(geom, blocks, regions, locals_, 0.5, QF_UNKNOWN_AS_OCCUPIED)
        present = np.array([blocks(tuple(int(v) for v in r)) is not None for r in regions], dtype=bool)
        ranges = np.where(present & (ranges >= 0), ranges, np.float32(-1.0))
        assert np.array_equal(got["region"], regions) and np.array_equal(got["local"], locals_)
        assert np.array_equal(got["range"], ranges.astype(np.float32)), i
    assert off == len(data)
