"""-m gpu: ohm::copyMap, the filter helpers and GpuMap::clone of the C++14 host mirror (ohm_amd/host/OhmGpuMap.h), driven
by the `copy` mode of ohm_amd/lib/gpumap_driver: Copy.CopySubmapFromGpu (tests/ohmtestgpu/GpuCopyTests.cpp:112-150).  The
driver dumps the source's, the copy's and the clone's chunks; they are compared with what the Python mirror gives for
the same rays."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import ohm_amd
from ohm_amd import GpuMap, OccupancyMap, copyFilterExtents, copyMap
from test_gpu_copy import assert_same, read_all
from test_gpu_copy_reference import COPY_MAX, COPY_MIN, RESOLUTION, shell_rays

pytestmark = pytest.mark.gpu

DRIVER = os.path.join(os.path.dirname(ohm_amd.LIB_PATH), "gpumap_driver")


def _dumps(data, count):
    """`count` maps, each u64 regions, then per region i16[3] key, u32 layer id, u64 bytes, the occupancy block."""
    off, maps = 0, []
    for _ in range(count):
        (n_regions,) = struct.unpack_from("<Q", data, off)
        off += 8
        chunks = {}
        for _r in range(n_regions):
            key = struct.unpack_from("<3h", data, off)
            lid, nbytes = struct.unpack_from("<IQ", data, off + 6)
            assert lid == 0
            off += 18
            chunks[tuple(key)] = {"occupancy": np.frombuffer(data, dtype=np.float32, count=nbytes // 4, offset=off).copy()}
            off += nbytes
        maps.append(chunks)
    assert off == len(data)
    return maps


def test_cpp_copy_submap_from_gpu(gpu):
    assert os.path.exists(DRIVER), "gpumap_driver missing: run __graft_entry__.build()"
    rays = shell_rays(ray_count=1024 * 16)
    with tempfile.TemporaryDirectory() as tmp:
        rp, op = os.path.join(tmp, "rays.bin"), os.path.join(tmp, "out.bin")
        with open(rp, "wb") as f:
            f.write(struct.pack("<Q", rays.shape[0]))
            f.write(np.ascontiguousarray(rays, dtype=np.float64).tobytes())
        res = subprocess.run([DRIVER, "copy", repr(RESOLUTION), "0", rp, op, repr(COPY_MIN[0]), repr(COPY_MAX[0])],
                             capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
        with open(op, "rb") as f:
            cpp_src, cpp_dst, cpp_clone = _dumps(f.read(), 3)
    src, dst = GpuMap(OccupancyMap(RESOLUTION)), GpuMap(OccupancyMap(RESOLUTION))
    assert src.integrateRays(rays) == len(rays)
    assert copyMap(dst, src, copyFilterExtents(COPY_MIN, COPY_MAX))
    want = read_all(dst)
    assert 0 < len(want) < len(cpp_src)
    assert_same(cpp_src, read_all(src))
    assert_same(cpp_dst, want)
    assert_same(cpp_clone, want)
