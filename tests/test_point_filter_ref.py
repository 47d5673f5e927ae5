"""CPU: the numpy restatement of the point filter's covariance test (tests/point_filter_ref.py, the order include/ohmhip.h
states under "POINT FILTER") held to exact rational arithmetic.

The bound.  The formula makes about 20 roundings, each relative to a sum of absolute terms that s = sum_i (sum_j
|inverse(S)_ij d_j|)^2 bounds; against exact rationals the worst error on the 3 000 random cases below is 6.0 * 2^-53 * s.
Values must agree within 2^-40 * s -- three orders of magnitude of margin -- and decisions must agree for every case with
|a - T| outside that band, T = fl(3.0 + tolerance).  The band is a condition, not a hiding place: at most 1 % of the
random set may fall inside it (200 000 random cases found none).  Cases built to sit inside it are a list of their own, and
only their value is asserted."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_filter_ref as PF  # noqa: E402


@pytest.mark.parametrize("tolerance", [0.0, 0.75])
def test_random_cases_agree_with_exact_arithmetic(tolerance):
    c, d = PF.random_cases(3000, 11)
    values = PF.covariance_value(c, d)
    status = PF.decide(values, tolerance)
    kept, removed = (status == PF.KEPT).mean(), (status == PF.REMOVED).mean()
    assert kept >= 0.2 and removed >= 0.2, (kept, removed)
    in_band = PF.check_against_exact(c, d, tolerance, values, status)
    assert in_band <= len(values) // 100, in_band


def test_cases_inside_the_band_assert_the_value_only():
    c, d = [], []
    for scale in (0.03125, 0.05, 0.1, 0.07):
        c0 = np.float32(scale)
        for axis in range(3):
            offset = [0.0, 0.0, 0.0]
            offset[axis] = float(c0) * np.sqrt(3.0)  # a = 3 to within a rounding
            c.append([c0, 0, c0, 0, 0, c0])
            d.append(offset)
    c, d = np.array(c, dtype=np.float32), np.array(d)
    values = PF.covariance_value(c, d)
    assert PF.check_against_exact(c, d, 0.0, values, PF.decide(values, 0.0)) == len(values)


def test_constructed_states():
    d = np.array([0.01, -0.02, 0.015])
    good = np.array([0.05, 0.01, 0.04, -0.02, 0.005, 0.03], dtype=np.float32)
    # a zero on each diagonal position, a NaN or infinite entry: removed
    broken = []
    for position in (0, 2, 5):
        state = good.copy()
        state[position] = 0.0
        broken.append(state)
    for position in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            state = good.copy()
            state[position] = bad
            broken.append(state)
    broken = np.array(broken, dtype=np.float32)
    values = PF.covariance_value(broken, np.tile(d, (len(broken), 1)))
    assert (PF.decide(values, 0.0) == PF.REMOVED).all() and (PF.decide(values, 1e300) == PF.REMOVED).all()
    assert not np.isfinite(values).any()
    assert PF.check_against_exact(broken[:3], np.tile(d, (3, 1)), 0.0, values[:3], PF.decide(values[:3], 0.0)) == 0
    # a negative diagonal is a matrix like any other; a far above and far below T; tolerance 0
    c = np.array([[-0.05, 0.01, 0.04, -0.02, 0.005, 0.03], [0.05, 0.01, -0.04, -0.02, 0.005, -0.03], good, good],
                 dtype=np.float32)
    offsets = np.array([d, d, 100.0 * d, 1e-3 * d])
    values = PF.covariance_value(c, offsets)
    status = PF.decide(values, 0.0)
    assert PF.check_against_exact(c, offsets, 0.0, values, status) == 0
    assert status[2] == PF.REMOVED and values[2] > 1e3 and status[3] == PF.KEPT and values[3] < 1e-3
    assert float(PF.exact_limit(0.0)) == 3.0 and PF.exact_limit(0.1) == Fraction(3.0 + 0.1)
    # the test is |a| < T, strictly
    assert PF.decide(np.array([3.0, np.nextafter(3.0, 0.0), np.nan, np.inf]), 0.0).tolist() == [2, 1, 2, 2]


def test_selection_and_occupancy():
    """Which filter runs (ohmfilter.cpp:187-221) and isOccupied, on a hand-made chunk."""
    dim, res, origin, threshold = (4, 4, 4), 0.5, (0.25, 0.0, -0.5), np.float32(0.0)
    occupancy = np.full(64, np.inf, dtype=np.float32)
    occupancy[:5] = [np.nan, np.nextafter(threshold, np.float32(-1)), threshold, 2.0, -1.0]
    mean = np.zeros((64, 2), dtype=np.uint32)
    mean[:, 0] = 511 | (511 << 10) | (511 << 20)
    covariance = np.tile(np.array([0.1, 0, 0.1, 0, 0, 0.1], dtype=np.float32), (64, 1))
    chunks = {(0, 0, 0): {"occupancy": occupancy, "mean": mean, "covariance": covariance}}
    keys = np.zeros(8, dtype=PF.GPU_KEY)
    keys["voxel"][:6, 0] = [0, 1, 2, 3, 0, 1]
    keys["voxel"][4:6, 1] = 1  # (0, 1, 0): index 4 (-1.0); (1, 1, 0): +inf
    keys["region"][6] = (3, 0, 0)  # a region the map does not hold
    keys["region"][7] = (-32768, -32768, -32768)
    centre = PF.mean_positions(keys, np.full(8, mean[0, 0]), res, dim, origin)
    points = centre + np.array([0.3, 0.0, 0.0])  # a = 9: removed when the test runs
    status, values = PF.filter_points(points, keys, chunks, res, dim, origin, threshold, tolerance=0.0)
    assert status.tolist() == [0, 0, 2, 2, 0, 0, 0, 0]
    assert np.isnan(values[[0, 1, 4, 5, 6, 7]]).all() and np.allclose(values[2:4], 9.0, rtol=1e-2)
    for kw in ({"tolerance": -1.0}, {"tolerance": 0.0, "occupancy_only": True},
               {"tolerance": 0.0, "layers": ("occupancy", "mean")}):
        status, values = PF.filter_points(points, keys, chunks, res, dim, origin, threshold, **kw)
        assert status.tolist() == [0, 0, 1, 1, 0, 0, 0, 0] and np.isnan(values).all()
    status, _ = PF.filter_points(points, keys, chunks, res, dim, origin, threshold, tolerance=7.0)
    assert status.tolist() == [0, 0, 1, 1, 0, 0, 0, 0]


def test_filtered_ply_bytes(tmp_path):
    from ohm_amd.cloud import write_filtered_ply
    points = np.array([[1.0, -2.5, 3.25], [0.1, 0.2, 0.3]])
    times = np.array([10.5, 11.0])
    path = tmp_path / "filtered.ply"
    assert write_filtered_ply(str(path), points, times) == 2
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty double x\nproperty double y\n"
              b"property double z\nproperty double time\nend_header\n")
    body = np.array([1.0, -2.5, 3.25, 10.5, 0.1, 0.2, 0.3, 11.0], dtype="<f8").tobytes()
    assert path.read_bytes() == header + body
    assert write_filtered_ply(str(path), np.zeros((0, 3)), np.zeros(0)) == 0
    assert path.read_bytes() == header.replace(b"vertex 2", b"vertex 0")
