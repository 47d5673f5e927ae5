"""CPU: the ray pattern model (tests/ray_pattern_ref.py) pinned to the reference's recorded conical image and to exact
arithmetic.  The device kernel and both host mirrors are then held to the model (tests/test_gpu_ray_pattern*.py)."""
import math
import os

import mpmath as mp
import numpy as np
import pytest

import ray_pattern_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53   # unit roundoff of binary64


def gamma(k):
    return k * U / (1.0 - k * U)


def test_conical_pattern_equals_the_recorded_image():
    """RayPattern.Conical (tests/ohmtest/RayPatternTests.cpp:105-160): axis (0.7, 0.7, 0), cone angle 65 deg, range 5,
    resolution 5 deg; the ray ends rasterised into the 72 x 36 spherical image equal the reference's recorded
    conical_ray_image (tests/golden/conical_ray_image.npy: its 2592 byte values), pixel for pixel."""
    resolution = math.radians(5.0)
    points = R.conical_ray_points((0.7, 0.7, 0.0), math.radians(65.0), 5.0, resolution)
    assert points.shape == (2 * 439, 3)            # 1 + 73 x 6 rays
    image, width, height = R.spherical_image(points, resolution)
    assert (width, height) == (72, 36)
    golden = np.load(os.path.join(GOLDEN, "conical_ray_image.npy"))
    assert golden.dtype == np.uint8 and golden.shape == (2592,)
    assert int((image == 255).sum()) == 112
    assert int(np.count_nonzero(image != golden)) == 0
    assert np.all(points[0::2] == 0.0)             # min_range 0: every ray starts at the sensor
    assert np.allclose(np.linalg.norm(points[1::2], axis=1), 5.0, rtol=1e-12)


def test_python_mirror_builds_the_model_pattern():
    """ohm_amd.RayPatternConical assembles its points on the host: the same points as the model, bit for bit (no device
    needed until the pattern is used)."""
    from ohm_amd import ClearingPattern, RayFlag, RayPattern, RayPatternConical
    for args in (((0.7, 0.7, 0.0), math.radians(65.0), 5.0, math.radians(5.0)),
                 ((0.1, -0.3, 2.0), math.radians(60.0), 3.5, math.radians(15.0), 0.25)):
        pattern = RayPatternConical(*args)
        model = R.conical_ray_points(*args)
        assert pattern.rayCount() == model.shape[0] // 2
        assert np.array_equal(pattern.rayPoints(), model)
    line = RayPattern()
    line.addPoint((0.0, 2.0, 0.0))
    line.addPoints([(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)])
    line.addRay((0.5, 0.5, 0.5), (1.0, 1.0, 1.0))
    line.addRays([(0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (9.0, 9.0, 9.0)])   # the odd trailing point is dropped
    assert line.rayCount() == 5
    assert np.array_equal(line.rayPoints()[0], (0.0, 0.0, 0.0)) and np.array_equal(line.rayPoints()[7], (1.0, 1.0, 1.0))
    clearing = ClearingPattern(line)
    default = (RayFlag.kRfEndPointAsFree | RayFlag.kRfStopOnFirstOccupied | RayFlag.kRfExcludeFree |
               RayFlag.kRfExcludeUnobserved)
    assert ClearingPattern.kDefaultRayFlags == default and clearing.rayFlags() == int(default) == 0x63
    clearing.setRayFlags(RayFlag.kRfEndPointAsFree | RayFlag.kRfReverseWalk)
    assert clearing.rayFlags() == int(RayFlag.kRfEndPointAsFree)        # ClearingPattern.cpp:40-44
    assert clearing.lastRaySet().shape == (0, 3)


def _poses(rng, count):
    """Unit, non-unit and near-180-degree quaternions (w close to 0), translations up to 1e4."""
    poses = np.empty((count, 7))
    for i in range(count):
        kind = i % 4
        q = rng.normal(size=4)
        if kind in (0, 1):
            q /= np.linalg.norm(q)                      # unit to rounding
        elif kind == 2:
            q *= rng.uniform(0.2, 3.0)                  # non-unit: used as given
        else:
            q[3] = rng.uniform(-1.0, 1.0) * 1e-9        # a half turn, almost
            q /= np.linalg.norm(q)
        t = rng.uniform(-1.0, 1.0, size=3) * 10.0 ** rng.uniform(-2, 4)
        poses[i, :3] = t
        poses[i, 3:] = q
    return poses


def _mp_cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def _mp_cross_abs(a, b):
    return (a[1] * b[2] + b[1] * a[2], a[2] * b[0] + b[2] * a[0], a[0] * b[1] + b[0] * a[1])


@pytest.mark.parametrize("scaling", [1.0, 0.37])
def test_quaternion_transform_against_mpmath(scaling):
    """rotation * (scaling * sample) + position against 200-bit arithmetic on the same binary64 inputs, 300 poses x 8
    points.  Bound per component: gamma_k * S, S the same expression with every term replaced by its absolute value
    (differences become sums), gamma_k = k u / (1 - k u), u = 2^-53.  k = 8, the roundings on the longest path of the
    expression as written: scaling * sample (1), the product and the difference of uv = cross(u, s) (3), those of
    uuv = cross(u, uv) (5), (uv * w) + uuv (6; uv * w alone ends at 4), * 2 (exact), s + ... (7), + position (8)."""
    mp.mp.prec = 200
    rng = np.random.default_rng(20261019)
    poses = _poses(rng, 300)
    points = rng.uniform(-1.0, 1.0, size=(8, 3)) * 10.0 ** rng.uniform(-1, 2, size=(8, 1))
    model = R.build_rays(points, poses, R.POSE_QUAT, scaling).reshape(300, 8, 3)
    k, worst = 8, 0.0
    for pi, pose in enumerate(poses):
        t = [mp.mpf(float(v)) for v in pose[:3]]
        u = [mp.mpf(float(v)) for v in pose[3:6]]
        w = mp.mpf(float(pose[6]))
        ua, wa = [abs(v) for v in u], abs(w)
        for si, sample in enumerate(points):
            s = [mp.mpf(scaling) * mp.mpf(float(v)) for v in sample]
            uv = _mp_cross(u, s)
            uuv = _mp_cross(u, uv)
            sa = [abs(v) for v in s]
            uva = _mp_cross_abs(ua, sa)
            uuva = _mp_cross_abs(ua, uva)
            for a in range(3):
                exact = s[a] + ((uv[a] * w) + uuv[a]) * 2 + t[a]
                bound = gamma(k) * (sa[a] + ((uva[a] * wa) + uuva[a]) * 2 + abs(t[a]))
                err = abs(mp.mpf(float(model[pi, si, a])) - exact)
                assert err <= bound, (pi, si, a, float(err), float(bound))
                if bound > 0:
                    worst = max(worst, float(err / bound))
    print("quaternion transform: worst error / bound = %.3f" % worst)


@pytest.mark.parametrize("scaling", [1.0, 0.37])
def test_matrix_transform_against_mpmath(scaling):
    """(m[0][r]*x + m[1][r]*y) + (m[2][r]*z + m[3][r]) with (x, y, z) = scaling * sample against 200-bit arithmetic, 300
    matrices x 8 points; bound gamma_k * S as above.  k = 4: scaling * sample (1), a product (2), the inner sum (3), the
    outer sum (4)."""
    mp.mp.prec = 200
    rng = np.random.default_rng(19102026)
    poses = _poses(rng, 300)
    mats = np.empty((300, 16))
    for i, pose in enumerate(poses):
        # the rotation matrix of the pose's quaternion (any matrix would do: the model takes it as given), times a shear
        x, y, z, w = pose[3:]
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        m = np.eye(4)
        m[:3, :3] = rot @ (np.eye(3) + 0.1 * rng.normal(size=(3, 3)))
        m[:3, 3] = pose[:3]
        mats[i] = m.T.reshape(16)                    # column major
    points = rng.uniform(-1.0, 1.0, size=(8, 3)) * 10.0 ** rng.uniform(-1, 2, size=(8, 1))
    model = R.build_rays(points, mats, R.POSE_MAT4, scaling).reshape(300, 8, 3)
    k, worst = 4, 0.0
    for mi, m in enumerate(mats):
        mm = [mp.mpf(float(v)) for v in m]
        for si, sample in enumerate(points):
            x, y, z = (mp.mpf(scaling) * mp.mpf(float(v)) for v in sample)
            for r in range(3):
                exact = (mm[r] * x + mm[4 + r] * y) + (mm[8 + r] * z + mm[12 + r])
                bound = gamma(k) * ((abs(mm[r] * x) + abs(mm[4 + r] * y)) + (abs(mm[8 + r] * z) + abs(mm[12 + r])))
                err = abs(mp.mpf(float(model[mi, si, r])) - exact)
                assert err <= bound, (mi, si, r, float(err), float(bound))
                if bound > 0:
                    worst = max(worst, float(err / bound))
    print("matrix transform: worst error / bound = %.3f" % worst)


def test_batch_is_the_sequential_sets_concatenated():
    """Pose major in pattern order: K poses in one call are the K single-pose ray sets one behind the other."""
    rng = np.random.default_rng(5)
    poses = _poses(rng, 3)
    points = rng.normal(size=(10, 3))
    whole = R.build_rays(points, poses)
    parts = np.concatenate([R.build_rays(points, poses[i:i + 1]) for i in range(3)])
    assert np.array_equal(whole, parts)
    ident = np.array([[0, 0, 0, 0, 0, 0, 1.0]])
    assert np.array_equal(R.build_rays(points, ident), points)
    assert np.array_equal(R.build_rays(points, np.eye(4).reshape(1, 16), R.POSE_MAT4), points)
