"""CPU: the C oracle's sample transform (oracle_transform_samples) pinned to the independent arbitrary-precision reference
of tests/transform_ref.py over every input family of tests/transform_cases.py.

Discrete results -- which samples are kept, their order, the bracket chosen on a stamp, f on a zero span -- must be the
reference's exactly.  For the values no bound is chosen from the oracle's behaviour: its worst deviation is measured and
printed per family (DESIGN.md section 6 records the figures), and the assertion is only a ceiling of 64 x 2^-52 on the
error scaled by max(1, |local sample|, |position|).  The chain is some two dozen fp64 operations and three libm calls
good to an ulp, so it cannot legitimately come near that; a wrong formula or bracket shows up at 1e-3 and more."""
import numpy as np
import pytest

import transform_cases as TC
import transform_ref as R
from oracle import oracle as O

CEILING = 64.0 * 2.0 ** -52
FAMILIES = TC.families()


def oracle_rows(case, local=None, sample_times=None, max_range=None):
    out = O.transform_samples(case["times"], case["translations"], case["rotations"],
                              case["sample_times"] if sample_times is None else sample_times,
                              case["local"] if local is None else local,
                              case["max_range"] if max_range is None else max_range)
    return out.reshape(-1, 6)


def assert_kept_in_order(case, got, kept):
    """Count and order against the reference's kept indices without a value reference: every sample is transformed on its
    own, so the oracle run on the reference's kept samples alone, unfiltered, must give the very same rows."""
    assert got.shape[0] == kept.shape[0]
    if kept.shape[0]:
        alone = oracle_rows(case, case["local"][kept], case["sample_times"][kept], float("inf"))
        assert np.array_equal(got, alone, equal_nan=True)


def family_deviation(cases, rows_of):
    """Worst deviation of rows_of(case) from the reference over the cases of one family, count and order asserted."""
    worst = None
    for case in cases:
        kept, rows = R.reference(case)
        got = rows_of(case)
        assert got.shape[0] == len(rows), "valid count: %d, reference %d" % (got.shape[0], len(rows))
        worst = R.merge(worst, R.deviation(rows, got, case["local"][kept]))
    return worst


@pytest.mark.parametrize("name,cases", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_oracle_matches_reference(name, cases, capsys):
    for case in cases:
        kept, _ = R.reference(case, values=False)
        assert_kept_in_order(case, oracle_rows(case), kept)
    worst = family_deviation(cases, oracle_rows)
    with capsys.disabled():
        print("\n[transform oracle vs reference] %-22s samples %6d  sample %.2e  position %.2e  position_abs %.2e m"
              % (name, sum(c["local"].shape[0] for c in cases), worst["sample"], worst["position"],
                 worst["position_abs"]))
    assert worst["mismatched"] == 0, worst
    assert worst["sample"] <= CEILING and worst["position"] <= CEILING, worst


def test_families_hold_what_they_promise():
    """The generators reach every discrete branch they are there for (and no pose pair trips the branch band: the
    reference raises on one instead of dropping it)."""
    general = FAMILIES[0][1][0]
    cosines = np.sum(general["rotations"][:-1] * general["rotations"][1:], axis=1)
    assert 0.3 < np.mean(cosines < 0) < 0.7  # about half the neighbours need the hemisphere flip
    assert np.unique(np.round(np.diff(general["times"]), 6)).shape[0] > 10  # unequal spacing
    assert set(general["times"]) <= set(general["sample_times"])  # a sample on every stamp
    kinds = set()
    case = dict(FAMILIES)["near_degenerate"][0]
    for k in range(case["rotations"].shape[0] - 1):
        pair = R._Slerp(case["rotations"][k], case["rotations"][k + 1])
        flipped = float(np.dot(case["rotations"][k], case["rotations"][k + 1])) < 0
        kinds.add("identical" if pair.identical else (("flip+" if flipped else "") +
                                                      ("spherical" if pair.spherical else "lerp")))
    assert kinds == {"identical", "spherical", "lerp", "flip+spherical", "flip+lerp"}
    dup = dict(FAMILIES)["duplicate_stamps"][0]
    doubled = dup["times"][np.flatnonzero(np.diff(dup["times"]) == 0)]
    assert doubled.shape[0] >= 6 and set(doubled) <= set(dup["sample_times"])
    brackets = [R.bracket(list(dup["times"]), t)[:2] for t in doubled]
    assert any(dup["times"][a] == dup["times"][b] and a != b for a, b in brackets)  # a zero span is really chosen
    filt = dict(FAMILIES)["filter"]
    counts = [int(R.keep_mask(c["local"], c["max_range"]).sum()) for c in filt]
    assert counts[1] == counts[0] and counts[0] - counts[2] == 10  # 169 exactly: kept at 169 and above, not one ulp below
    assert counts[4] == 4 and counts[5] == 0  # max_range 0 keeps the zero vectors only; negative keeps nothing
    with np.errstate(invalid="ignore"):
        assert np.isinf(filt[3]["local"][R.keep_mask(filt[3]["local"], np.inf)]).any()  # inf passes an infinite range


@pytest.mark.parametrize("pattern", TC.COMPACTION_PATTERNS)
@pytest.mark.parametrize("n", TC.COMPACTION_SIZES)
def test_oracle_compaction(n, pattern):
    case, rejected = TC.compaction_case(n, pattern)
    kept, _ = R.reference(case, values=False)
    assert np.array_equal(kept, np.flatnonzero(~rejected))  # the generator rejects exactly what it means to
    if pattern in ("scattered", "block_runs") and n >= 65537:
        assert 0.25 < rejected.mean() < 0.45
    got = oracle_rows(case)
    assert_kept_in_order(case, got, kept)
    if n <= 257 and kept.shape[0]:
        worst = family_deviation([case], oracle_rows)
        assert worst["mismatched"] == 0 and worst["sample"] <= CEILING and worst["position"] <= CEILING, worst


def test_oracle_round_trip_general_rotations(capsys):
    """World points moved into the sensor frame with the reference's pose (arbitrary precision, rounded to fp64 once) and
    transformed back by the oracle land on the original points.  The rounding of the local point to fp64 is an input
    error of half an ulp of |local|, inside the scale of the bound."""
    case = TC.general_case(201, 80, TC.BIG_STAMP, 600)
    rng = np.random.default_rng(202)
    inside = np.isfinite(case["sample_times"])
    st = case["sample_times"][inside]
    trajectory = R.Trajectory(case["times"], case["translations"], case["rotations"])
    world = rng.uniform(-40.0, 40.0, (st.shape[0], 3))
    local = np.array([R.to_local(trajectory, t, p) for t, p in zip(st, world)])
    got = oracle_rows(case, local, st, float("inf"))
    assert got.shape[0] == st.shape[0]
    scale = np.maximum(1.0, np.maximum(np.linalg.norm(local, axis=1), np.linalg.norm(got[:, :3], axis=1)))
    worst = float(np.max(np.max(np.abs(got[:, 3:] - world), axis=1) / scale))
    with capsys.disabled():
        print("\n[transform oracle round trip] samples %d  worst scaled error %.2e" % (st.shape[0], worst))
    assert worst <= CEILING
