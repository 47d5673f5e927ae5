"""-m gpu: ohm::Heightmap of the C++ mirror (ohm_amd/host/OhmGpuMap.h) in HeightmapMode::kSimpleFill, run by
`gpumap_driver heightmapfill`: the scaled multi-level scene is written into the host map voxel by voxel and uploaded,
kLayeredFill is still refused, and the arrays, the visit log and the stats the fill writes equal the CPU restatement's
(tests/heightmap_fill_ref.py)."""
import struct

import numpy as np
import pytest

import cpp_driver
import heightmap_fill_ref as F
import heightmap_ref as R
from heightmap_fill_cases import scaled_multi_level

pytestmark = pytest.mark.gpu


def test_cpp_heightmap_fill(gpu):
    scene, p = scaled_multi_level()
    blob = struct.pack("<3i", *scene.dim)
    blob += struct.pack("<6d", *p.reference_pos, p.floor, p.ceiling, p.min_clearance)
    blob += struct.pack("<iI", p.up_axis, (1 if p.virtual_surface else 0) | (2 if p.promote_virtual_below else 0))
    blob += struct.pack("<Q", len(scene.chunks))
    for key in sorted(scene.chunks):
        blob += struct.pack("<3h", *key)
        blob += np.ascontiguousarray(scene.chunks[key]["occupancy"], dtype=np.float32).tobytes()
    data = cpp_driver.run("heightmapfill", scene.resolution, 0, blob)
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
