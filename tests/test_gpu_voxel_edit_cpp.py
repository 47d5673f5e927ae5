"""-m gpu: the C++14 host mirror's voxel edits (ohm_amd/host/OhmGpuMap.h: GpuMap::integrateVoxels, the single-voxel
conveniences integrateHit / integrateMiss with the reference's names, keyRange and integrateMisses over it), driven by
gpumap_driver's `voxeledit` mode on an edit script, against the model of tests/voxel_edit_ref.py at exact equality."""
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import mean_cases
import occupancy_cases as OC
import voxel_edit_ref as V
from ohm_amd import LAYERS

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ohm_amd", "lib", "gpumap_driver")
GPU_KEY = np.dtype([("region", "<i2", (3,)), ("voxel", "u1", (4,))])


def run_driver(points, ops):
    assert os.path.exists(DRIVER), "gpumap_driver missing: run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as tmp:
        pp, qp, op = (os.path.join(tmp, n) for n in ("points.bin", "ops.bin", "out.bin"))
        with open(pp, "wb") as f:
            f.write(struct.pack("<Q", points.shape[0]))
            f.write(np.ascontiguousarray(points, dtype=np.float64).tobytes())
        with open(qp, "wb") as f:
            f.write(np.ascontiguousarray(ops, dtype=np.uint8).tobytes())
        res = subprocess.run([DRIVER, "voxeledit", "0.1", "0", pp, op, qp], capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, (res.returncode, res.stdout, res.stderr)
        return open(op, "rb").read()


def parse(data, layers):
    (n_regions,) = struct.unpack_from("<Q", data, 0)
    at = 8
    blocks = {}
    by_id = {LAYERS[n][0]: n for n in layers}
    for _ in range(n_regions):
        region = struct.unpack_from("<3h", data, at)
        at += 6
        blocks[region] = {}
        for _ in layers:
            lid, nbytes = struct.unpack_from("<IQ", data, at)
            at += 12
            blocks[region][by_id[lid]] = np.frombuffer(data, dtype=LAYERS[by_id[lid]][1], count=nbytes // 4, offset=at)
            at += nbytes
    counters = struct.unpack_from("<6Q", data, at)
    at += 48
    keys = np.frombuffer(data, dtype=GPU_KEY, count=counters[5], offset=at)
    assert at + 10 * counters[5] == len(data)
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
