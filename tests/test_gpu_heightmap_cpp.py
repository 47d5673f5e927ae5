"""-m gpu: ohm::Heightmap of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver heightmap`: the map
(occupancy + mean) is built by ohm::GpuMap::integrateRays in small batches -- still collected by batch coalescing when
the heightmap is asked for -- and the three arrays it writes equal the CPU restatement's (tests/heightmap_ref.py)."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from ohm_amd import OccupancyMap

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
from heightmap_cases import two_level_scene  # noqa: E402
from parity import make_oracle  # noqa: E402

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ohm_amd", "lib", "gpumap_driver")


@pytest.mark.parametrize("min_clearance,virtual", [(0.0, False), (1.5, True)])
def test_cpp_heightmap(gpu, min_clearance, virtual):
    rays = two_level_scene()
    assert os.path.exists(DRIVER), "gpumap_driver missing: run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as tmp:
        rp, op = os.path.join(tmp, "rays.bin"), os.path.join(tmp, "out.bin")
        with open(rp, "wb") as f:
            f.write(struct.pack("<Q", rays.shape[0]))
            f.write(np.ascontiguousarray(rays, dtype=np.float64).tobytes())
        res = subprocess.run([DRIVER, "heightmap", "0.1", "4096", rp, op, repr(min_clearance), str(int(virtual))],
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
        data = open(op, "rb").read()
    ma, mb, populated, cells, has_mean = struct.unpack_from("<IIQQB", data, 0)
    n = ma * mb
    assert has_mean == 1 and len(data) == 25 + n * (4 + 24 + 8)
    occupancy = np.frombuffer(data, dtype=np.float32, count=n, offset=25).reshape(mb, ma)
    voxels = np.frombuffer(data, dtype=R.HEIGHTMAP_VOXEL, count=n, offset=25 + 4 * n).reshape(mb, ma)
    mean = np.frombuffer(data, dtype=np.uint32, count=2 * n, offset=25 + 28 * n).reshape(mb, ma, 2)
    layers = ("occupancy", "mean")
    map_ = OccupancyMap(0.1, layers=layers)
    om = make_oracle(map_)
    om.integrate_occupancy(rays)
    src = R.Source(0.1, (32, 32, 32), om.chunks(), map_.occupancy_threshold_value, has_mean=True)
    want = R.build_heightmap(src, R.Params(0.1, min_clearance, virtual_surface=virtual))
    assert (want.occupancy == 1.0).any() and (not virtual or (want.occupancy == -1.0).any())
    assert (ma, mb) == (want.ma, want.mb)
    assert np.array_equal(occupancy.view(np.uint32), want.occupancy.view(np.uint32))
    assert np.array_equal(voxels.view(np.uint8), want.voxels.view(np.uint8))
    assert np.array_equal(mean, want.mean)
    assert populated == want.populated and cells == int((want.source_column != R.NO_COLUMN).sum())
