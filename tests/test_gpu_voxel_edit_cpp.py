"""-m gpu: the C++14 host mirror's voxel edits (ohm_amd/host/OhmGpuMap.h: GpuMap::integrateVoxels, the single-voxel
conveniences integrateHit / integrateMiss with the reference's names, keyRange and integrateMisses over it), driven by
gpumap_driver's `voxeledit` mode on an edit script, against the model of tests/voxel_edit_ref.py at exact equality."""
import struct

import numpy as np
import pytest

import cpp_driver
import mean_cases
import occupancy_cases as OC
import voxel_edit_ref as V

pytestmark = pytest.mark.gpu
GPU_KEY = np.dtype([("region", "<i2", (3,)), ("voxel", "u1", (4,))])


def run_driver(points, ops):
    return cpp_driver.run("voxeledit", 0.1, 0, points, np.ascontiguousarray(ops, dtype=np.uint8).tobytes(), timeout=120)


def parse(data, layers):
    blocks, rest = cpp_driver.read_region_dump(data, len(layers), tail=True)
    assert all(set(region) == set(layers) for region in blocks.values())
    counters = struct.unpack_from("<6Q", rest, 0)
    keys = np.frombuffer(rest, dtype=GPU_KEY, count=counters[5], offset=48)
    assert 48 + 10 * counters[5] == len(rest)
    return blocks, counters, keys


def test_cpp_voxel_edits(gpu):
    layers = ("occupancy", "mean")
    geo = V.geometry(0.1, 32, layers)
    cfg = OC.configs()["default"]
    # the sample points of a sheet of mean_cases (cases 2 and 4 at reduced size: every pattern of ops on them), a point
    # without a key, and the two corners of a box that crosses a region corner
    sheet = [s for s in mean_cases.build() if s.config == "near10"][0]
    points, ops = [], []
    for i, case in enumerate(sheet.cases[:24]):
        pattern = OC.PATTERNS[1 + i % (len(OC.PATTERNS) - 1)]
        for j, ch in enumerate(pattern):
            points.append(case.ends[j % len(case.ends)])
            ops.append(V.MISS if ch == "m" else (V.HIT_SAMPLE if (i + j) % 2 else V.HIT))
    order = np.random.default_rng(5).permutation(len(points))  # (no run is contiguous; the model sees the same order)
    points = [points[k] for k in order] + [(1e9, 0.0, 0.0), (-1.65, 1.52, -1.63), (-1.52, 1.68, -1.55)]
    ops = [ops[k] for k in order] + [V.HIT, V.MISS, V.MISS]
    points = np.array(points, dtype=np.float64)
    blocks, counters, range_keys = parse(run_driver(points, ops), layers)
    model = {}
    st = V.apply(model, geo, cfg, [V.Element(o, point=tuple(p)) for o, p in zip(ops, points)])
    assert counters[:5] == (st["applied"], st["null_keys"], st["distinct_voxels"], st["regions_touched"],
                            st["regions_created"]) and st["null_keys"] == 1
    first = V.voxel_key(geo, points[0])
    V.apply(model, geo, cfg, [V.Element(V.HIT_SAMPLE, point=tuple(points[0])), V.Element(V.MISS, first),
                              V.Element(V.HIT, first)])
    want_range = V.key_range(geo, V.voxel_key(geo, points[-2]), V.voxel_key(geo, points[-1]))
    assert len({k[0] for k in want_range}) == 8
    got_range = [(tuple(int(v) for v in k["region"]), tuple(int(v) for v in k["voxel"][:3])) for k in range_keys]
    assert got_range == want_range
    V.apply(model, geo, cfg, [V.Element(V.MISS, k) for k in want_range])
    assert set(blocks) == set(model)
    for region in model:
        for name in layers:
            assert np.array_equal(blocks[region][name].view(np.uint32), model[region][name].view(np.uint32)), (region, name)
