"""-m gpu: ohm::compare::compareVoxels of the C++14 host mirror (ohm_amd/host/OhmGpuMap.h), driven by the `compare` mode of
ohm_amd/lib/gpumap_driver: every ray but the last into the reference map, every ray into the evaluated one.  What the
driver writes -- the result, both lists, the number of messages; with kContinue, with stop-at-first and with ohmcmp's
occupancy tolerance -- must equal what the Python mirror gives for the same rays."""
import ctypes as C
import struct

import numpy as np
import pytest

import compare_cases as cases
import cpp_driver
from ohm_amd import GpuMap, OccupancyMap, Tolerance, compareVoxels, configureTolerance, kContinue
from ohm_amd import _lib as L

pytestmark = pytest.mark.gpu

RESOLUTION = 0.1


def _results(data, count):
    off, out = 0, []
    size = C.sizeof(L.CompareResult)
    for _ in range(count):
        res = L.CompareResult.from_buffer_copy(data[off:off + size])
        off += size
        (n_keys,) = struct.unpack_from("<Q", data, off)
        keys = data[off + 8:off + 8 + 10 * n_keys]
        off += 8 + 10 * n_keys
        (n_missing,) = struct.unpack_from("<Q", data, off)
        missing = np.frombuffer(data, dtype=np.int16, count=3 * n_missing, offset=off + 8).reshape(-1, 3)
        off += 8 + 6 * n_missing
        (logged,) = struct.unpack_from("<Q", data, off)
        off += 8
        out.append((res, keys, missing, logged))
    assert off == len(data)
    return out


def test_cpp_compare_equals_the_python_mirror(gpu):
    rays = np.concatenate([cases.fan_rays(1500, 12, reach=2.5), [[0.01, 0.02, 0.03], [1.93, -1.21, 0.77]]])
    cpp = _results(cpp_driver.run("compare", RESOLUTION, 0, rays, timeout=120), 3)
    ref, ev = GpuMap(OccupancyMap(RESOLUTION)), GpuMap(OccupancyMap(RESOLUTION))
    assert ref.integrateRays(rays[:-2]) == len(rays) - 2 and ev.integrateRays(rays) == len(rays)
    loose = Tolerance("occupancy")
    configureTolerance(loose, "occupancy", np.float32(1e2))
    configureTolerance(loose, "count", np.uint32(1))
    failed = []
    for (got, keys, missing, logged), (flags, tolerance) in zip(cpp, ((kContinue, None), (0, None), (kContinue, loose))):
        messages = []
        want = compareVoxels(ev, ref, "occupancy", tolerance, flags, log=lambda sev, msg: messages.append(msg))
        failed.append(want.voxels_failed)
        for name, _ in L.CompareResult._fields_:
            value = getattr(got, name)
            assert ([int(v) for v in value] if hasattr(value, "__len__") else int(value)) == want.detail[name], name
        assert keys == want.mismatches.tobytes() and np.array_equal(missing, want.missing_regions)
        assert logged == len(messages) == len(want.mismatches)
    # the last ray changed voxels; it stops the walk at one; the tolerance forgives those both maps had observed
    assert failed[0] >= 10 and failed[1] == 1 and failed[2] < failed[0]
