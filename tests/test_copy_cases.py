"""CPU: the conditions the scenes of tests/copy_cases.py meet, confirmed by the oracle alone.  The device tests
(tests/test_gpu_copy.py) rely on them: a replay mask that is wrong cannot pass unseen only if the follow-up batch visits
and changes planted voxels of every class."""
import numpy as np
import pytest

import copy_cases as cases


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_fans_touch_enough_regions_and_the_follow_up_leaves_some_alone(shape):
    rays = cases.fan(shape)
    assert 100 <= len(rays) // 2 <= 400
    wide = cases.regions_touched(shape, rays)
    narrow = cases.regions_touched(shape, cases.follow_up(shape))
    assert len(wide) >= 8
    assert narrow and narrow < wide


def test_shapes_are_the_ones_the_kernel_branches_on():
    voxels = {name: int(np.prod(s["dim"])) for name, s in cases.SHAPES.items()}
    assert voxels["odd"] == 105 and voxels["odd"] % 32 and (voxels["odd"] * 4) % 16 and (voxels["odd"] * 8) % 16
    assert voxels["unit"] == 1 and voxels["default"] == 32768
    assert voxels["tiled"] == 38400 > 32768  # (more than one tile: ohm_amd/csrc/tiling_impl.h)


@pytest.mark.parametrize("shape,dst_trunc", [("odd", None), ("odd", 0.2), ("default", None), ("tiled", None)])
def test_tsdf_follow_up_changes_a_planted_voxel_of_every_class(shape, dst_trunc):
    p = cases.planted_tsdf(shape, 0.1, dst_trunc)
    assert all(len(p.voxels[name]) >= 4 for name in cases.TSDF_CLASSES), {k: len(v) for k, v in p.voxels.items()}
    assert len(set(region for where in p.voxels.values() for region, _ in where)) >= 2
    changed = p.changed(p.after, "tsdf")
    assert all(changed[name] >= 1 for name in cases.TSDF_CLASSES), changed
    # what was planted is what tsdfCountable (ohm_amd/csrc/replay_kernels.h) tells apart
    t = np.float32(0.1)
    for name, states in cases.tsdf_states(0.1).items():
        for w, d in states:
            countable = (d == 0) if w == 0 else bool(d == t and 1.0 <= w <= 1e4 and w == np.trunc(w))
            assert countable == (name in ("countable", "unobserved")), (name, w, d)


@pytest.mark.parametrize("shape", ["odd", "default"])
def test_ndt_follow_up_changes_planted_voxels_with_and_without_samples(shape):
    p = cases.planted_ndt(shape, 0.45)
    assert all(len(p.voxels[name]) >= 4 for name in cases.NDT_CLASSES)
    for region, vi in p.voxels["samples"]:
        assert p.chunks[region]["mean"].reshape(-1, 2)[vi, 1] > 0
    for region, vi in p.voxels["no_samples"]:
        assert p.chunks[region]["mean"].reshape(-1, 2)[vi, 1] == 0
    changed = p.changed(p.after, "occupancy")
    assert all(changed[name] >= 1 for name in cases.NDT_CLASSES), changed
