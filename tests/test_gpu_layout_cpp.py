"""-m gpu: layer changes through the C++14 host mirror (ohm_amd/host/OhmGpuMap.h: GpuMap::updateLayout, add*Layer) -- the
`layout` mode of ohm_amd/lib/gpumap_driver, run as a child process: VoxelMean.LayoutToggle restated
(tests/ohmtestgpu/GpuVoxelMeanTests.cpp:143-244), and layers added between two batches against a twin map that had them
from the start (tests/test_gpu_layout.py has the cases in full)."""
import struct

import numpy as np
import pytest

import cpp_driver
import layout_ref as R
import mean_ref
from ohm_amd import _lib as L, synth
from test_gpu_layout import ALL_SECONDARY, integrate, new_map, reset_layers

pytestmark = pytest.mark.gpu


def test_voxel_mean_layout_toggle(gpu):
    resolution = 0.5
    sample, centre = (1.1, 1.1, 1.1), (1.25, 1.25, 1.25)
    coord = mean_ref.coord_ref(tuple(s - c for s, c in zip(sample, centre)), resolution)
    data = cpp_driver.run("layout", resolution, 0, None, "toggle", coord)
    stage = struct.Struct("<IIfQ3d")
    stages = [stage.unpack_from(data, i * stage.size) for i in range(4)]
    mean_added = struct.unpack_from("<II", data, 4 * stage.size)
    (gone,) = struct.unpack_from("<i", data, 4 * stage.size + 8)
    assert len(data) == 4 * stage.size + 12
    one, two = R.layer_mask(["occupancy"]), R.layer_mask(["occupancy", "mean"])
    assert [s[0] for s in stages] == [s[1] for s in stages] == [one, two, two, one]  # host and device layers
    threshold = np.float32(np.log(np.float32(0.5) / np.float32(0.5)))
    assert all(s[2] == stages[0][2] and s[2] >= threshold for s in stages)  # occupancy unchanged and occupied
    assert all(s[3] == 1 for s in stages)
    positions = [np.array(s[4:7]) for s in stages]
    assert np.array_equal(positions[0], centre) and np.array_equal(positions[3], centre)
    assert np.all(np.abs(positions[2] - sample) <= resolution / 1000.0) and np.all(positions[2] != centre)
    assert mean_added == (0, 0)
    assert gone == L.ERR_UNSUPPORTED


def test_added_layers_start_now(gpu):
    rays1 = synth.random_rays(150, extent=1.5, seed=11)
    rays2 = synth.random_rays(200, extent=4.0, seed=12)
    final = ("occupancy",) + ALL_SECONDARY
    data = cpp_driver.run("layout", 0.1, rays1.shape[0] // 2, np.concatenate([rays1, rays2]), "added")
    chunks = cpp_driver.read_region_dump(data, len(final))
    twin = new_map(final)
    integrate(twin, rays1, 100.0)
    first_regions = {tuple(k) for k in twin.regionKeys().tolist()}
    reset_layers(twin, ALL_SECONDARY)
    integrate(twin, rays2, 200.0)
    twin.syncVoxels()
    expect = twin.map().chunks
    assert set(chunks) == set(expect) and set(chunks) - first_regions
    for key, layers in chunks.items():
        assert sorted(layers) == sorted(final)
        for name in final:
            assert layers[name].tobytes() == expect[key][name].tobytes(), (key, name)
    assert all(any(layers[name].any() for layers in chunks.values()) for name in ALL_SECONDARY)
