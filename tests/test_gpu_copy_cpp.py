"""-m gpu: ohm::copyMap, the filter helpers and GpuMap::clone of the C++14 host mirror (ohm_amd/host/OhmGpuMap.h), driven
by the `copy` mode of ohm_amd/lib/gpumap_driver: Copy.CopySubmapFromGpu (tests/ohmtestgpu/GpuCopyTests.cpp:112-150).  The
driver dumps the source's, the copy's and the clone's chunks; they are compared with what the Python mirror gives for
the same rays."""
import pytest

import cpp_driver
from ohm_amd import GpuMap, OccupancyMap, copyFilterExtents, copyMap
from test_gpu_copy import assert_same, read_all
from test_gpu_copy_reference import COPY_MAX, COPY_MIN, RESOLUTION, shell_rays

pytestmark = pytest.mark.gpu


def test_cpp_copy_submap_from_gpu(gpu):
    rays = shell_rays(ray_count=1024 * 16)
    data = cpp_driver.run("copy", RESOLUTION, 0, rays, repr(COPY_MIN[0]), repr(COPY_MAX[0]), timeout=120)
    cpp_src, cpp_dst, cpp_clone = cpp_driver.read_region_dump(data, 1, maps=3)  # one layer each: occupancy
    assert all(set(layers) == {"occupancy"} for chunks in (cpp_src, cpp_dst, cpp_clone) for layers in chunks.values())
    src, dst = GpuMap(OccupancyMap(RESOLUTION)), GpuMap(OccupancyMap(RESOLUTION))
    assert src.integrateRays(rays) == len(rays)
    assert copyMap(dst, src, copyFilterExtents(COPY_MIN, COPY_MAX))
    want = read_all(dst)
    assert 0 < len(want) < len(cpp_src)
    assert_same(cpp_src, read_all(src))
    assert_same(cpp_dst, want)
    assert_same(cpp_clone, want)
