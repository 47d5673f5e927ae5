"""CPU: the clearance restatement (tests/clearance_ref.py) pinned to known answers -- Ranges.Scaling's four queries
(tests/ohmtestgpu/GpuRangesTests.cpp:505-568) at their exact values, a single obstacle, the target itself, radius 0,
the `>=` threshold, the int16 wrap of moveKey and the scan-order tie -- and its two evaluations against each other."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clearance_ref import (QF_REPORT_UNSCALED, QF_UNKNOWN_AS_OCCUPIED, DictBlocks, Geometry,  # noqa: E402
                           clearance_keys, clearance_regions, half_extent)

INF = np.float32(np.inf)


def empty(kd, value=np.float32(-1.0)):
    return np.full(kd[0] * kd[1] * kd[2], value, dtype=np.float32)


def put(block, kd, local, value=np.float32(1.0)):
    block[local[0] + local[1] * kd[0] + local[2] * kd[0] * kd[1]] = value


def one(geom, blocks, region, local, radius, flags=0, scaling=(1.0, 1.0, 1.0)):
    return clearance_keys(geom, blocks, [region], [local], radius, flags, scaling)[0]


def scaling_map():
    """Ranges.Scaling: res 0.25, 8^3 regions, origin -0.125 (0, 0, 0 is the centre of voxel (0,0,0 : 4,4,4)); hits at
    (0.5, 0, 0), (0, 0.75, 0), (0, 0, 1) -- voxels (0,0,0 : 6,4,4), (0,0,0 : 4,7,4) and (0,0,1 : 4,4,0)."""
    kd = (8, 8, 8)
    a = empty(kd, INF)
    b = empty(kd, INF)
    hit = np.float32(np.log(np.float32(0.9) / np.float32(0.1)))
    put(a, kd, (6, 4, 4), hit)
    put(a, kd, (4, 7, 4), hit)
    put(b, kd, (4, 4, 0), hit)
    return Geometry(0.25, kd, 0.0), DictBlocks({(0, 0, 0): a, (0, 0, 1): b})


@pytest.mark.parametrize("scaling,expected,report_scaled", [
    ((1.0, 1.0, 1.0), np.float32(2 * 0.25), False),
    ((4.0, 1.0, 1.0), np.float32(3 * 0.25), False),
    ((1.0, 1.0, np.float32(1.0) / np.float32(3.0)), np.float32(4 * 0.25), False),
    ((np.float32(1.1), np.float32(1.1), np.float32(1.0) / np.float32(4.0)), np.float32(4 * 0.25 / 4.0), True),
])
def test_ranges_scaling(scaling, expected, report_scaled):
    geom, blocks = scaling_map()
    flags = 0 if report_scaled else QF_REPORT_UNSCALED
    assert one(geom, blocks, (0, 0, 0), (4, 4, 4), 2.0, flags, scaling) == expected
    got = clearance_regions(geom, blocks, [(0, 0, 0)], 2.0, flags, scaling)
    assert got[0, 4, 4, 4] == expected


@pytest.mark.parametrize("offset", [(1, 0, 0), (0, -2, 0), (1, 2, -3), (-4, 4, 4), (5, 0, -5)])
def test_single_obstacle(offset):
    kd = (32, 32, 32)
    block = empty(kd)
    put(block, kd, (16 + offset[0], 16 + offset[1], 16 + offset[2]))
    geom = Geometry(1.0, kd, 0.0)
    d2 = np.float32(offset[0] ** 2 + offset[1] ** 2 + offset[2] ** 2)
    assert one(geom, DictBlocks({(0, 0, 0): block}), (0, 0, 0), (16, 16, 16), 9.0) == np.sqrt(d2)
    # beyond the radius: none
    assert one(geom, DictBlocks({(0, 0, 0): block}), (0, 0, 0), (16, 16, 16), float(np.sqrt(d2)) * 0.99) == -1


def test_self_and_radius_zero():
    kd = (8, 8, 8)
    block = empty(kd)
    put(block, kd, (3, 3, 3))
    put(block, kd, (4, 3, 3))
    geom = Geometry(0.1, kd, 0.0)
    blocks = DictBlocks({(0, 0, 0): block})
    assert half_extent(0.0, 0.1) == 0
    assert one(geom, blocks, (0, 0, 0), (3, 3, 3), 0.5) == 0.0
    assert one(geom, blocks, (0, 0, 0), (3, 3, 3), 0.0) == 0.0
    assert one(geom, blocks, (0, 0, 0), (2, 3, 3), 0.0) == -1.0  # radius 0: the window is the voxel itself
    # the float separation of neighbouring centres is not exactly the resolution: 0.1 itself is beyond a 0.1 radius
    assert one(geom, blocks, (0, 0, 0), (2, 3, 3), 0.1) == -1.0
    assert abs(one(geom, blocks, (0, 0, 0), (2, 3, 3), 0.15) - 0.1) < 1e-6
    # unknown as occupied: a missing region obstructs, so does an unobserved voxel
    assert one(geom, blocks, (0, 0, 0), (0, 0, 0), 0.1, QF_UNKNOWN_AS_OCCUPIED) > 0
    assert one(geom, blocks, (1, 0, 0), (0, 0, 0), 0.1, QF_UNKNOWN_AS_OCCUPIED) == 0.0
    put(block, kd, (6, 6, 6), INF)
    assert one(geom, DictBlocks({(0, 0, 0): block}), (0, 0, 0), (6, 6, 6), 0.1, QF_UNKNOWN_AS_OCCUPIED) == 0.0
    assert one(geom, DictBlocks({(0, 0, 0): block}), (0, 0, 0), (6, 6, 6), 0.1) == -1.0


def test_threshold_is_inclusive():
    kd = (8, 8, 8)
    thr = np.float32(0.4054651)
    block = empty(kd)
    put(block, kd, (2, 2, 2), thr)
    put(block, kd, (5, 5, 5), np.nextafter(thr, np.float32(-np.inf)))
    geom = Geometry(1.0, kd, thr)
    blocks = DictBlocks({(0, 0, 0): block})
    assert one(geom, blocks, (0, 0, 0), (2, 2, 2), 1.0) == 0.0   # value == threshold: occupied (`>=`)
    assert one(geom, blocks, (0, 0, 0), (5, 5, 5), 1.0) == -1.0  # one ulp below: not


def test_int16_wrap():
    """moveKey adds into an i16vec3: the neighbour +1 in x of region 32767's last voxel is region -32768's first.  Its
    centre lies 2 * 32768 regions away, so only a tiny x scaling lets it count."""
    kd = (32, 32, 32)
    block = empty(kd)
    put(block, kd, (0, 5, 5))
    geom = Geometry(0.1, kd, 0.0)
    blocks = DictBlocks({(-32768, 0, 0): block, (32767, 0, 0): empty(kd)})
    rsd = 32 * 0.1
    cv = np.float32(((float(np.float32(32767)) * rsd - 0.5 * rsd) + 31 * 0.1) + 0.05)
    cn = np.float32(((float(np.float32(-32768)) * rsd - 0.5 * rsd) + 0 * 0.1) + 0.05)
    sx = (cn - cv) * np.float32(1e-6)
    expected = np.sqrt(sx * sx)
    assert 0.1 < expected < 0.3
    assert one(geom, blocks, (32767, 0, 0), (31, 5, 5), 1.0, 0, (np.float32(1e-6), 1.0, 1.0)) == expected
    assert one(geom, blocks, (32767, 0, 0), (31, 5, 5), 1.0) == -1.0  # (too far unscaled)
    got = clearance_regions(geom, blocks, [(32767, 0, 0)], 1.0, 0, (np.float32(1e-6), 1.0, 1.0))
    assert got[0, 5, 5, 31] == expected


@pytest.mark.parametrize("dy,expected", [(1, np.float32(2.0)), (-1, np.float32(1.0))])
def test_scan_order_tie(dy, expected):
    """Two obstacles of equal scaled range 4 -- (+2, 0, 0) at scale 1, (0, dy, 0) at y scale 2 -- differ in unscaled
    range; the earlier in z, y, x scan order wins."""
    kd = (32, 32, 32)
    block = empty(kd)
    put(block, kd, (12, 10, 10))
    put(block, kd, (10, 10 + dy, 10))
    geom = Geometry(1.0, kd, 0.0)
    blocks = DictBlocks({(0, 0, 0): block})
    scale = (1.0, 2.0, 1.0)
    assert one(geom, blocks, (0, 0, 0), (10, 10, 10), 3.0, QF_REPORT_UNSCALED, scale) == expected
    got = clearance_regions(geom, blocks, [(0, 0, 0)], 3.0, QF_REPORT_UNSCALED, scale)
    assert got[0, 10, 10, 10] == expected


@pytest.mark.parametrize("flags", [0, QF_UNKNOWN_AS_OCCUPIED, QF_REPORT_UNSCALED])
def test_two_evaluations_agree(flags):
    rng = np.random.default_rng(5 + flags)
    kd = (10, 6, 7)
    blocks = {}
    for key in [(0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1)]:
        v = rng.choice(np.array([-1.0, 1.0, np.inf], dtype=np.float32), size=kd[0] * kd[1] * kd[2], p=[0.9, 0.05, 0.05])
        blocks[key] = v.astype(np.float32)
    geom = Geometry(0.3, kd, 0.0)
    args = (geom, DictBlocks(blocks), [(0, 0, 0), (1, 0, 0)], 0.95, flags, (1.0, np.float32(0.7), 1.3))
    a = clearance_regions(*args, method="offsets")
    b = clearance_regions(*args, method="targets")
    assert np.array_equal(a, b)
    assert (a > 0).any() and (a == 0).any()
