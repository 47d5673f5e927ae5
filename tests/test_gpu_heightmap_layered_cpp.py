"""-m gpu: ohm::LayeredHeightmap of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver heightmaplayered`
through a reference to its base class: the scaled multi-level scene is written into the host map voxel by voxel and
uploaded, and the planes, the layer counts, the visit log and the stats the build writes equal the CPU restatement's
(tests/heightmap_layered_ref.py), in both modes, the filter off and on."""
import struct

import numpy as np
import pytest

import cpp_driver
import heightmap_layered_cases as LC
import heightmap_layered_ref as LR
import heightmap_ref as R
from heightmap_fill_cases import scaled_multi_level

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode,threshold", [(LC.MODE_UNORDERED, 0), (LC.MODE_ORDERED, 0), (LC.MODE_ORDERED, 8)])
def test_cpp_heightmap_layered(gpu, mode, threshold):
    scene, p = scaled_multi_level()
    blob = struct.pack("<3i", *scene.dim)
    blob += struct.pack("<6d", *p.reference_pos, p.floor, p.ceiling, p.min_clearance)
    blob += struct.pack("<iI", p.up_axis, (1 if p.virtual_surface else 0) | (2 if p.promote_virtual_below else 0))
    blob += struct.pack("<II", mode, threshold)
    blob += struct.pack("<Q", len(scene.chunks))
    for key in sorted(scene.chunks):
        blob += struct.pack("<3h", *key)
        blob += np.ascontiguousarray(scene.chunks[key]["occupancy"], dtype=np.float32).tobytes()
    data = cpp_driver.run("heightmaplayered", scene.resolution, 0, blob)
    want = LR.build_layered(scene.source(), p, mode, threshold)
    counts = LC.quirk_counts(want)
    assert counts["repeats"] > 0 and counts["virtual_kept"] > 0 and want.layers == 2
    if mode == LC.MODE_ORDERED:
        assert counts["multi_layer_columns"] > 0 and counts["permuted_columns"] > 0
        assert (counts["filtered"] > 0) == (threshold != 0)
    ma, mb, slots, zero = struct.unpack_from("<4I", data, 0)
    stats = struct.unpack_from("<8Q3I", data, 16)  # 80 bytes with the tail padding
    surface, virtual = struct.unpack_from("<2Q", data, 96)
    n, cells = slots * ma * mb, ma * mb
    assert (ma, mb, slots, zero) == (want.ma, want.mb, want.slots, 0)
    assert stats == LR.stats_of(want)
    visits = stats[0]
    assert len(data) == 112 + n * (4 + 24 + 4) + cells + 12 * visits
    shape = (slots, mb, ma)
    occupancy = np.frombuffer(data, dtype=np.float32, count=n, offset=112).reshape(shape)
    voxels = np.frombuffer(data, dtype=R.HEIGHTMAP_VOXEL, count=n, offset=112 + 4 * n).reshape(shape)
    source_visit = np.frombuffer(data, dtype=np.uint32, count=n, offset=112 + 28 * n).reshape(shape)
    layer_count = np.frombuffer(data, dtype=np.uint8, count=cells, offset=112 + 32 * n).reshape(mb, ma)
    log = np.frombuffer(data, dtype=np.uint32, count=3 * visits, offset=112 + 32 * n + cells).reshape(-1, 3)
    assert np.array_equal(occupancy.view(np.uint32), want.occupancy.view(np.uint32))
    assert np.array_equal(voxels.view(np.uint8), want.voxels.view(np.uint8))
    assert np.array_equal(source_visit, want.source_visit)
    assert np.array_equal(layer_count, want.layer_count)
    assert np.array_equal(log, want.log)
    # getHeightmapVoxelInfo with the key's up coordinate as the slot
    assert (surface, virtual) == (int((want.occupancy == 1.0).sum()), int((want.occupancy == -1.0).sum()))
