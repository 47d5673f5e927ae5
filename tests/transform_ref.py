"""Arbitrary-precision reference for the sample transform (GpuTransformSamples::transform), independent of the C oracle.

Written from the documented semantics (include/ohmhip.h, "GpuTransformSamples::transform"; the reference's
ohmgpu/GpuTransformSamples.cpp:47-60, 131-142 and ohmgpu/gpu/TransformSamples.cl), in two halves:

* everything DISCRETE is reproduced exactly, on the fp64 inputs: which samples are kept (NaN component, or squared length
  above max_range -- evaluated in fp64, as the inputs are compared in fp64), stable compaction, the bracketing search with
  the reference's own probe sequence, the clamps outside the trajectory, the "no search" rule for one and two poses, f = 0
  on a zero time span, the from == to shortcut, the !(cos >= 0) flip and the 1 - cos > 1e-12 branch;
* everything CONTINUOUS is evaluated with mpmath at 60 digits on the exact values of the fp64 inputs: f, the lerp of the
  translation, the dot product, acos, sin, the slerp coefficients, the quaternion product, the rotation matrix.

Two branches of slerp are decided in fp64 by the code under test and exactly here, so a pose pair whose exact value lies
within rounding of the threshold has no defined answer.  Such a pair is an error of the INPUTS (BranchBandError), never
skipped: |(1 - cos) - 1e-12| < 1e-13 (the two branches differ by ~angle^2/6, 3e-13 relative there), and |cos| < 1e-13
for the hemisphere flip (the two sides are different rotations)."""
import math

import mpmath
import numpy as np

CTX = mpmath.MPContext()
CTX.dps = 60

LERP_THRESHOLD = 1e-12  # the fp64 literal of the slerp branch
BRANCH_BAND = 1e-13
FLIP_BAND = 1e-13


class BranchBandError(ValueError):
    """A pose pair sits on a slerp branch threshold: the generator has to move it, the check may not drop it."""


def keep_mask(local, max_range):
    """goodSample on the fp64 inputs: no NaN component, and (x*x + y*y) + z*z <= max_range (equality is kept)."""
    local = np.asarray(local, dtype=np.float64).reshape(-1, 3)
    x, y, z = local[:, 0], local[:, 1], local[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        far = ((x * x + y * y) + z * z) > np.float64(max_range)
    return ~(np.isnan(x) | np.isnan(y) | np.isnan(z)) & ~far


def bracket(times, t):
    """(from, to, sample time after clamping) as the reference's search finds them."""
    n = len(times)
    frm, to = 0, n - 1
    if n > 2:
        if times[0] <= t <= times[n - 1]:
            iterations = 0
            while frm <= to and iterations < 100000:
                iterations += 1
                mid_low = (frm + to) // 2
                mid_high = min(mid_low + 1, n - 1)
                if t >= times[mid_low] and t <= times[mid_high]:
                    frm, to = mid_low, mid_high
                    break
                elif t <= times[mid_low]:
                    to = mid_low - 1
                else:
                    frm = mid_low + 1
            else:
                raise AssertionError("bracketing search left its loop without a bracket")
        elif t < times[0]:
            t, frm, to = times[0], 0, 0
        else:  # after the trajectory, or a NaN stamp: every comparison above is false
            t, frm, to = times[n - 1], n - 1, n - 1
    return frm, to, t


class _Slerp:
    """slerp(rot[from], rot[to], .) for one pose pair: the discrete decisions and the angle, made once."""

    def __init__(self, qf, qt):
        m = CTX.mpf
        self.qf = [m(float(v)) for v in qf]
        self.identical = all(float(a) == float(b) for a, b in zip(qf, qt))
        if self.identical:
            return
        to = [m(float(v)) for v in qt]
        cos_angle = sum((a * b for a, b in zip(self.qf, to)), m(0))
        if abs(cos_angle) < FLIP_BAND:
            raise BranchBandError("pose pair within %g of the hemisphere flip (cos = %s)" % (FLIP_BAND, cos_angle))
        if not (cos_angle >= 0):
            to = [-v for v in to]
            cos_angle = -cos_angle
        self.to = to
        gap = 1 - cos_angle
        if abs(gap - m(LERP_THRESHOLD)) < BRANCH_BAND:
            raise BranchBandError("pose pair within %g of the lerp threshold (1 - cos = %s)" % (BRANCH_BAND, gap))
        self.spherical = gap > m(LERP_THRESHOLD)
        if self.spherical:
            self.angle = CTX.acos(cos_angle)
            self.inv_sin = 1 / CTX.sin(self.angle)

    def at(self, f):
        if self.identical:
            return self.qf
        if self.spherical:
            c0 = CTX.sin((1 - f) * self.angle) * self.inv_sin
            c1 = CTX.sin(f * self.angle) * self.inv_sin
        else:
            c0, c1 = 1 - f, f
        return [c0 * a + c1 * b for a, b in zip(self.qf, self.to)]


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz]


def _rotate(q, v):
    x, y, z, w = q
    return [(1 - 2 * (y * y + z * z)) * v[0] + 2 * (x * y - z * w) * v[1] + 2 * (x * z + y * w) * v[2],
            2 * (x * y + z * w) * v[0] + (1 - 2 * (x * x + z * z)) * v[1] + 2 * (y * z - x * w) * v[2],
            2 * (x * z - y * w) * v[0] + 2 * (y * z + x * w) * v[1] + (1 - 2 * (x * x + y * y)) * v[2]]


class Trajectory:
    """A trajectory held at full precision; pose(t) is the reference's pose rule rot[from] * slerp(rot[from], rot[to], f)
    with the translation lerp, for the bracket the reference's search picks."""

    def __init__(self, times, translations, rotations_xyzw):
        self.times = [float(t) for t in np.asarray(times, dtype=np.float64)]
        self.translations = np.asarray(translations, dtype=np.float64).reshape(-1, 3)
        self.rotations = np.asarray(rotations_xyzw, dtype=np.float64).reshape(-1, 4)
        self._pairs = {}
        self.pairs_used = set()

    def pose(self, sample_time):
        """-> (position [3], rotation [4] x, y, z, w) in mpmath, or None when f is NaN (a NaN stamp on two poses)."""
        m = CTX.mpf
        frm, to, t = bracket(self.times, float(sample_time))
        span = m(self.times[to]) - m(self.times[frm])
        if span != 0:
            if math.isnan(t):
                return None
            f = (m(t) - m(self.times[frm])) / span
        else:
            f = m(0)
        key = (frm, to)
        pair = self._pairs.get(key)
        if pair is None:
            pair = self._pairs[key] = _Slerp(self.rotations[frm], self.rotations[to])
        self.pairs_used.add(key)
        pf = [m(float(v)) for v in self.translations[frm]]
        pt = [m(float(v)) for v in self.translations[to]]
        position = [a + f * (b - a) for a, b in zip(pf, pt)]
        return position, _quat_mul(pair.qf, pair.at(f))


def transform(times, translations, rotations_xyzw, sample_times, local_samples, max_range=float("inf"), values=True):
    """-> (kept input indices in output order, rows).  rows[k] = 6 mpmath numbers (sensor position, world sample) for
    input kept[k]; None with values=False (count and order only)."""
    local = np.asarray(local_samples, dtype=np.float64).reshape(-1, 3)
    sample_times = np.asarray(sample_times, dtype=np.float64)
    if local.shape[0] == 0 or len(times) == 0:
        return np.zeros(0, dtype=np.int64), ([] if values else None)
    kept = np.flatnonzero(keep_mask(local, max_range))
    if not values:
        return kept, None
    trajectory = Trajectory(times, translations, rotations_xyzw)
    nan = CTX.mpf("nan")
    rows = []
    for i in kept:
        pose = trajectory.pose(sample_times[i])
        if pose is None:
            rows.append([nan] * 6)
            continue
        position, q = pose
        r = _rotate(q, [CTX.mpf(float(v)) for v in local[i]])
        rows.append(position + [p + d for p, d in zip(position, r)])
    return kept, rows


def reference(case, values=True):
    """transform() of a case of tests/transform_cases.py."""
    return transform(case["times"], case["translations"], case["rotations"], case["sample_times"], case["local"],
                     case["max_range"], values=values)


def merge(worst, other):
    """Fold one deviation() result into a running worst (None to start)."""
    if worst is None:
        return dict(other)
    return {k: (worst[k] + other[k]) if k == "mismatched" else max(worst[k], other[k]) for k in worst}


def to_local(trajectory, sample_time, world_point):
    """The inverse of the pose at sample_time applied to a world point, rounded to fp64: conj(q) * (p - position).  q is a
    product of fp64-normalised quaternions, unit to a few 1e-16, so the conjugate inverts it to the same order."""
    position, q = trajectory.pose(sample_time)
    d = [CTX.mpf(float(w)) - p for w, p in zip(world_point, position)]
    x, y, z, w = q
    return np.array([float(v) for v in _rotate([-x, -y, -z, w], d)])


def deviation(rows, got, local_kept):
    """Worst deviation of fp64 output `got` ((2k, 3): position, sample per kept input) from the reference rows, scaled
    by max(1, |local sample|, |position|).  Non-finite reference values (inf / NaN components let through by an infinite
    max_range, NaN stamps) must be matched in kind.  -> dict(sample, position, position_abs, mismatched)."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 6)
    assert got.shape[0] == len(rows), (got.shape, len(rows))
    worst = {"sample": 0.0, "position": 0.0, "position_abs": 0.0, "mismatched": 0}
    m = CTX.mpf
    for k, row in enumerate(rows):
        finite_pos = [v for v in row[:3] if CTX.isfinite(v)]
        scale = max([m(1), CTX.sqrt(sum((v * v for v in finite_pos), m(0)))] +
                    ([m(float(np.linalg.norm(local_kept[k])))] if np.all(np.isfinite(local_kept[k])) else []))
        for c in range(6):
            ref, value = row[c], float(got[k, c])
            if not CTX.isfinite(ref):
                same = (math.isnan(value) if CTX.isnan(ref) else (math.isinf(value) and (value > 0) == (ref > 0)))
                worst["mismatched"] += 0 if same else 1
                continue
            if not math.isfinite(value):
                worst["mismatched"] += 1
                continue
            err = abs(m(value) - ref)
            if c < 3:
                worst["position_abs"] = max(worst["position_abs"], float(err))
                worst["position"] = max(worst["position"], float(err / scale))
            else:
                worst["sample"] = max(worst["sample"], float(err / scale))
    return worst
