"""-m gpu: ohm::Heightmap of the C++ mirror (ohm_amd/host/OhmGpuMap.h) in HeightmapMode::kSimpleFill, run by
`gpumap_driver heightmapfill`: the scaled multi-level scene is written into the host map voxel by voxel and uploaded,
kLayeredFill is still refused, and the arrays, the visit log and the stats the fill writes equal the CPU restatement's
(tests/heightmap_fill_ref.py)."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
import heightmap_fill_ref as F  # noqa: E402
from heightmap_fill_cases import scaled_multi_level  # noqa: E402

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ohm_amd", "lib", "gpumap_driver")


def test_cpp_heightmap_fill(gpu):
    scene, p = scaled_multi_level()
    assert os.path.exists(DRIVER), "gpumap_driver missing: run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as tmp:
        sp, op = os.path.join(tmp, "scene.bin"), os.path.join(tmp, "out.bin")
        with open(sp, "wb") as f:
            f.write(struct.pack("<3i", *scene.dim))
            f.write(struct.pack("<6d", *p.reference_pos, p.floor, p.ceiling, p.min_clearance))
            f.write(struct.pack("<iI", p.up_axis, (1 if p.virtual_surface else 0) | (2 if p.promote_virtual_below else 0)))
            f.write(struct.pack("<Q", len(scene.chunks)))
            for key in sorted(scene.chunks):
                f.write(struct.pack("<3h", *key))
                f.write(np.ascontiguousarray(scene.chunks[key]["occupancy"], dtype=np.float32).tobytes())
        res = subprocess.run([DRIVER, "heightmapfill", repr(scene.resolution), "0", sp, op], capture_output=True,
                             text=True, timeout=300)
        assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
        data = open(op, "rb").read()
    want = F.build_fill(scene.source(), p)
    assert want.revisits > 0 and want.raising_pops > 0 and (want.occupancy == -1.0).any()
    ma, mb = struct.unpack_from("<II", data, 0)
    visits, populated, cells, revisits, generations, largest = struct.unpack_from("<4Q2I", data, 8)
    surface, virtual = struct.unpack_from("<2Q", data, 48)
    n = ma * mb
    assert (ma, mb) == (want.ma, want.mb) and len(data) == 64 + n * (4 + 24 + 4) + 12 * visits
    occupancy = np.frombuffer(data, dtype=np.float32, count=n, offset=64).reshape(mb, ma)
    voxels = np.frombuffer(data, dtype=R.HEIGHTMAP_VOXEL, count=n, offset=64 + 4 * n).reshape(mb, ma)
    source_visit = np.frombuffer(data, dtype=np.uint32, count=n, offset=64 + 28 * n).reshape(mb, ma)
    log = np.frombuffer(data, dtype=np.uint32, count=3 * visits, offset=64 + 32 * n).reshape(-1, 3)
    assert np.array_equal(occupancy.view(np.uint32), want.occupancy.view(np.uint32))
    assert np.array_equal(voxels.view(np.uint8), want.voxels.view(np.uint8))
    assert np.array_equal(source_visit, want.source_visit)
    assert np.array_equal(log, want.log)
    assert (visits, populated, cells, revisits, generations, largest) == \
        (want.visits, want.populated, want.cells, want.revisits, want.generations, want.largest_generation)
    # getHeightmapVoxelInfo on the result
    assert (surface, virtual) == (int((want.occupancy == 1.0).sum()), int((want.occupancy == -1.0).sum()))
