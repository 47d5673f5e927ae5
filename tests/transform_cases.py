"""Seeded input families for the sample transform, shared by tests/test_transform_ref.py (CPU: C oracle against the
arbitrary-precision reference) and tests/test_gpu_transform_samples.py (device against both).

A case is a dict: times, translations, rotations (x, y, z, w; unit, normalised in fp64), sample_times, local, max_range.
A family is (name, [cases]); deviations are reported per family.  Pose pairs are either near-identical (perturbation
<= 1e-7: 1 - cos ~ 1e-14, the lerp branch) or well apart (perturbation >= 1e-5: 1 - cos >= ~5e-11), so none lies in the
reference's branch band around 1 - cos = 1e-12 (tests/transform_ref.py)."""
import numpy as np

BIG_STAMP = 1.7e9  # seconds since the epoch: what a sensor log carries

COMPACTION_SIZES = (1, 255, 256, 257, 65537, 2 ** 20 + 77)
COMPACTION_PATTERNS = ("scattered", "block_runs", "first_rejected", "last_rejected", "all_but_last", "all", "none")
REJECT_FRACTION = 0.35
COMPACTION_MAX_RANGE = 60.0 * 60.0


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))


def random_rotations(rng, count):
    """Uniform on the 3-sphere: neighbouring pairs need the hemisphere flip half of the time, angles run up to pi."""
    return _unit(rng.standard_normal((count, 4)))


def perturbed(rng, q, eps):
    """q moved by eps along a unit direction orthogonal to it, renormalised: 1 - cos = eps^2 / 2 to first order."""
    d = rng.standard_normal(4)
    d -= np.dot(d, q) * q
    d /= np.sqrt(np.dot(d, d))
    return _unit(q + eps * d)


def random_trajectory(rng, count, base_time, step=(0.02, 0.3), extent=25.0):
    times = base_time + np.cumsum(rng.uniform(step[0], step[1], count))  # unequal spacing
    translations = np.cumsum(rng.uniform(-0.5, 0.5, (count, 3)), axis=0) + rng.uniform(-extent, extent, 3)
    return times, translations, random_rotations(rng, count)


def random_local(rng, count, reach=30.0):
    """Sensor-frame points from a few centimetres to `reach` metres, every direction."""
    direction = rng.standard_normal((count, 3))
    direction /= np.sqrt(np.sum(direction * direction, axis=1, keepdims=True))
    return direction * (reach * 10.0 ** rng.uniform(-3.0, 0.0, count))[:, None]


def _case(times, translations, rotations, sample_times, local, max_range=float("inf")):
    sample_times = np.ascontiguousarray(sample_times, dtype=np.float64)
    local = np.ascontiguousarray(local, dtype=np.float64).reshape(-1, 3)
    assert sample_times.shape[0] == local.shape[0]
    return dict(times=np.ascontiguousarray(times, dtype=np.float64),
                translations=np.ascontiguousarray(translations, dtype=np.float64),
                rotations=np.ascontiguousarray(rotations, dtype=np.float64), sample_times=sample_times, local=local,
                max_range=float(max_range))


def _sample_times(rng, times, uniform, on_stamps=True, outside=True, nan=True):
    """Uniform inside the trajectory; exactly on every stamp (first and last too); before and after it; a NaN."""
    parts = [rng.uniform(times[0], times[-1], uniform)]
    if on_stamps:
        parts.append(times)
    if outside:
        span = max(times[-1] - times[0], 1.0)
        parts.append(np.array([times[0] - 0.37 * span, np.nextafter(times[0], -np.inf), np.nextafter(times[-1], np.inf),
                               times[-1] + 2.5 * span]))
    if nan:
        parts.append(np.array([np.nan]))
    out = np.concatenate(parts)
    rng.shuffle(out)
    return out


def general_case(seed, poses, base_time, uniform):
    rng = np.random.default_rng(seed)
    times, translations, rotations = random_trajectory(rng, poses, base_time)
    st = _sample_times(rng, times, uniform)
    return _case(times, translations, rotations, st, random_local(rng, st.shape[0]))


def near_degenerate_case(seed, base_time):
    """A general trajectory with special neighbours planted every sixth pose, sampled densely inside and on the ends of
    exactly those brackets."""
    rng = np.random.default_rng(seed)
    poses = 60
    times, translations, rotations = random_trajectory(rng, poses, base_time)
    kinds = ("identical", "lerp_1e-7", "acos_1e-5", "negated", "negated_1e-7", "negated_1e-5", "lerp_1e-8", "acos_1e-4")
    special = []
    for j, kind in enumerate(kinds):
        k = 3 + 6 * j
        q = rotations[k]
        if kind == "identical":
            nxt = q.copy()
        elif kind == "negated":
            nxt = -q
        else:
            nxt = perturbed(rng, q, float(kind.split("_")[-1]))
            if kind.startswith("negated"):
                nxt = -nxt
        rotations[k + 1] = nxt
        special.append(k)
    parts = [_sample_times(rng, times, 300)]
    for k in special:
        parts.append(rng.uniform(times[k], times[k + 1], 90))
        parts.append(np.array([times[k], times[k + 1], np.nextafter(times[k], np.inf),
                               np.nextafter(times[k + 1], -np.inf)]))
    st = np.concatenate(parts)
    rng.shuffle(st)
    return _case(times, translations, rotations, st, random_local(rng, st.shape[0]))


def duplicate_stamp_case(seed, base_time):
    """Zero time spans inside the trajectory (pairs and one triple of equal stamps, with different poses on them), sampled
    on the duplicated stamps, one ulp either side of them, and in between."""
    rng = np.random.default_rng(seed)
    poses = 48
    times, translations, rotations = random_trajectory(rng, poses, base_time)
    for k in (0, 5, 11, 12, 20, 33, poses - 2):  # 11, 12: three equal stamps; both ends of the trajectory too
        times[k + 1] = times[k]
    assert np.all(np.diff(times) >= 0)
    doubled = times[np.flatnonzero(np.diff(times) == 0)]
    st = np.concatenate([_sample_times(rng, times, 700), np.repeat(doubled, 8), np.nextafter(doubled, np.inf),
                         np.nextafter(doubled, -np.inf)])
    rng.shuffle(st)
    return _case(times, translations, rotations, st, random_local(rng, st.shape[0]))


def few_pose_case(seed, poses, base_time):
    """Two poses: no search, and the reference extrapolates (f < 0, f > 1) outside them.  One pose: that pose."""
    rng = np.random.default_rng(seed)
    times, translations, rotations = random_trajectory(rng, poses, base_time)
    span = (times[-1] - times[0]) if poses > 1 else 1.0
    st = np.concatenate([rng.uniform(times[0] - 2.0 * span, times[-1] + 2.0 * span, 900), times,
                         np.array([times[0] - span, times[-1] + span, np.nan, np.nan])])
    rng.shuffle(st)
    return _case(times, translations, rotations, st, random_local(rng, st.shape[0]))


def filter_cases(seed):
    """The sample filter: one trajectory and one sample set under every max_range of interest.  (3, 4, 12) and its kin have
    a squared length of exactly 169 in fp64, so max_range = 169 keeps them, one ulp below rejects them."""
    rng = np.random.default_rng(seed)
    times, translations, rotations = random_trajectory(rng, 40, BIG_STAMP)
    local = random_local(rng, 600, reach=40.0)  # squared lengths on both sides of 169
    exact = np.array([[3.0, 4.0, 12.0], [12.0, -4.0, 3.0], [0.0, 0.0, 13.0], [-13.0, 0.0, 0.0], [5.0, 12.0, 0.0],
                      [0.0, 0.0, 0.0], [-0.0, 0.0, -0.0]])
    odd = []
    for axis in range(3):
        for value in (np.nan, np.inf, -np.inf):
            row = rng.uniform(-3.0, 3.0, 3)
            row[axis] = value
            odd.append(row)
    odd.append([np.inf, -np.inf, 1.0])
    odd.append([np.nan, np.inf, np.nan])
    local = np.concatenate([local, exact, np.array(odd), exact])
    order = rng.permutation(local.shape[0])
    local = local[order]
    st = rng.uniform(times[0], times[-1], local.shape[0])
    ranges = (169.0, np.nextafter(169.0, np.inf), np.nextafter(169.0, -np.inf), float("inf"), 0.0, -1.0, 1.0e4)
    return [_case(times, translations, rotations, st, local, r) for r in ranges]


def families():
    """Every family small enough for the arbitrary-precision reference to evaluate per sample."""
    return [
        ("general_small_stamps", [general_case(101, 40, 12.5, 1500)]),
        ("general_big_stamps", [general_case(102, 200, BIG_STAMP, 2500)]),
        ("near_degenerate", [near_degenerate_case(103, BIG_STAMP), near_degenerate_case(104, 3.0)]),
        ("duplicate_stamps", [duplicate_stamp_case(105, BIG_STAMP), duplicate_stamp_case(106, 0.0)]),
        ("two_poses", [few_pose_case(107, 2, BIG_STAMP), few_pose_case(108, 2, -4.0)]),
        ("one_pose", [few_pose_case(109, 1, BIG_STAMP)]),
        ("filter", filter_cases(110)),
    ]


def reject_mask(n, pattern, rng):
    if pattern == "none":
        return np.zeros(n, dtype=bool)
    if pattern == "all":
        return np.ones(n, dtype=bool)
    if pattern == "all_but_last":
        mask = np.ones(n, dtype=bool)
        mask[-1] = False
        return mask
    if pattern == "block_runs":
        # runs that cover whole 256-sample blocks (one, two or three in a row), and a ragged run across a block edge
        mask = np.zeros(n, dtype=bool)
        blocks = (n + 255) // 256
        b = 0
        while b < blocks:
            run = int(rng.integers(1, 4))
            if rng.random() < REJECT_FRACTION:
                mask[256 * b:256 * (b + run)] = True
            b += run
        mask[:256] = True  # the first block always, so the sizes of one or two blocks have a whole block rejected too
        if n > 1024:
            mask[760:780] = True
        return mask
    mask = rng.random(n) < REJECT_FRACTION
    if pattern == "first_rejected":
        mask[0] = True
    elif pattern == "last_rejected":
        mask[-1] = True
    else:
        assert pattern == "scattered", pattern
    return mask


def compaction_case(n, pattern="scattered", seed=7):
    """n samples on a general trajectory, the rejected ones by `pattern`: half of them through a NaN component, half
    through their range.  Every kept sample is a distinct local point, so an output row identifies its input index.
    -> (case, reject mask)."""
    rng = np.random.default_rng([seed, n, COMPACTION_PATTERNS.index(pattern)])
    times, translations, rotations = random_trajectory(rng, 64, BIG_STAMP)
    st = rng.uniform(times[0] - 0.5, times[-1] + 0.5, n)
    local = rng.uniform(-20.0, 20.0, (n, 3))  # squared length <= 1200 < max_range
    mask = reject_mask(n, pattern, rng)
    rejected = np.flatnonzero(mask)
    by_nan = rejected[rng.random(rejected.shape[0]) < 0.5]
    local[by_nan, rng.integers(0, 3, by_nan.shape[0])] = np.nan
    by_range = np.setdiff1d(rejected, by_nan)
    local[by_range] = local[by_range] / np.sqrt(np.sum(local[by_range] ** 2, axis=1, keepdims=True)) * \
        rng.uniform(61.0, 500.0, (by_range.shape[0], 1))
    kept_rows = local[~mask]
    assert np.unique(kept_rows[:, 0]).shape[0] == kept_rows.shape[0], "kept samples must be distinct (in x already)"
    return _case(times, translations, rotations, st, local, COMPACTION_MAX_RANGE), mask
