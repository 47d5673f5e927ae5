"""The constructed set of tests/secondary_cases.py and its numpy model, on the CPU.

- The model's leaf equals the reference header, bit for bit, on the golden rows and on every update of the set (with and
  without a mean layer); the golden is tests/golden/ref_incident.npz, the outputs of ohm/VoxelIncidentCompute.h and
  ohm/VoxelTouchTimeCompute.h compiled in place.
- The set holds what it was built to hold: each condition is counted from the set's inputs and the reference's recorded
  outputs (the model is used only where the same test has just held it to them), printed, and asserted.
- Each wrong variant of the update changes at least one voxel of the expected layers.

Two variants cannot be told apart by chained updates of a fresh map, by arithmetic and not for want of cases:
`nan_dropping_clamps` -- the only NaN a chain produces is the decoded z, x and y stay finite and z is never clamped, so
no clamp ever sees a NaN operand; it is told apart on the golden's direct encodeNormal rows with NaN components.
`ignore_zero_normal_rule` -- a decoded normal is zero only while the voxel's word is 0, and then a fresh map's count is
0 too; it is told apart on the set replayed over `prior_counts` (a map that had a mean layer before an incident layer)."""
import os

import numpy as np
import pytest

import secondary_cases as S

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_incident.npz"))
F = np.float32


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cs():
    c = S.cases()
    assert S.digest(c) == bytes(G["case_digest"]).hex(), "the set changed: regenerate tests/golden/ref_incident.npz"
    return c


@pytest.fixture(scope="module")
def truth(cs):
    """The model's replays, each with its trace, computed once."""
    out = {}
    for with_mean in (True, False):
        for size in (None, 97):
            trace = []
            normals, times = S.replay(cs, S.NumpyLeaf(), with_mean=with_mean, call_size=size, trace=trace)
            out[(with_mean, size)] = (normals, times, trace)
    return out


def test_set_size(cs):
    assert cs.n_rays <= 3000
    assert 200 <= np.count_nonzero(cs.target < 0) <= 400  # through-going rays
    regions = {tuple(v) for v in (cs.voxel_ids()[cs.target >= 0] // S.REGION_DIM).tolist()}
    assert regions == set(S.REGIONS)  # global voxel index // 32 is the region key with the origin at 0
    near = (cs.target >= 0) & (cs.target < S.TARGETS_PER_REGION)
    assert np.abs(cs.rays[1::2][near]).max() < 5.0 and np.abs(cs.rays[1::2][cs.target >= 16][:, :2]).min() > 1990.0


def test_model_leaf_equals_reference_on_golden_rows():
    leaf = S.NumpyLeaf()
    # (IEEE 754 leaves the sign of the NaN a square root of a negative number returns open, and x86 and numpy differ in
    # it: a NaN is compared as a NaN, everything else as bits)
    got = np.array([_bits(leaf.decode(w)) for w in G["dec_in"]], dtype=np.uint32)
    want = G["dec_out"].copy()
    for a in (got, want):
        a[np.isnan(a.view(F))] = 0x7FC00000
    assert np.array_equal(got, want)
    assert np.array_equal(np.array([leaf.encode(r) for r in G["enc_in"].view(F)], dtype=np.uint32), G["enc_out"])
    got = [leaf.update_normal(p, r, c) for p, r, c in zip(G["upd_packed"], G["upd_ray"].view(F), G["upd_count"])]
    assert np.array_equal(np.array(got, dtype=np.uint32), G["upd_out"])
    got = [leaf.encode_time(b, t) for b, t in G["touch_in"]]
    assert np.array_equal(np.array(got, dtype=np.uint32), G["touch_out"])


def test_model_equals_reference_on_every_update(cs, truth):
    for name, with_mean in (("mean", True), ("nomean", False)):
        trace = truth[(with_mean, None)][2]
        assert [t[0] for t in trace] == list(range(cs.n_rays))  # default flags, no filter: every ray has a sample
        assert np.array_equal(np.array([t[3] for t in trace], dtype=np.uint32), G["case_inc_" + name])
        assert np.array_equal(np.array([t[4] for t in trace], dtype=np.uint32), G["case_touch"])
        # cutting the set into calls changes neither layer's per-update values (the time base is the map's, not a call's)
        cut = truth[(with_mean, 97)][2]
        assert [t[3:] for t in cut] == [t[3:] for t in trace]


def test_conditions_on_the_set(cs, truth):
    counts = {}
    leaf = S.NumpyLeaf()  # held to the reference on these very updates by the test above
    trace = truth[(True, None)][2]
    counts["prev_normal_nan_z"] = int(G["case_prev_z_nan_mean"].sum())
    counts["prev_normal_nan_z_without_mean"] = int(G["case_prev_z_nan_nomean"].sum())
    d = (cs.rays[0::2] - cs.rays[1::2]).astype(F)
    len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert len2.dtype == F
    counts["incident_len2_le_1e-6"] = int(np.count_nonzero(len2 <= F(1e-6)))
    counts["incident_len2_in_1e-6_4e-6"] = int(np.count_nonzero((len2 > F(1e-6)) & (len2 <= F(4e-6))))
    counts["start_equals_end"] = int(np.count_nonzero(np.all(cs.rays[0::2] == cs.rays[1::2], axis=1)))
    fails = 0
    for ray, prev, count, _new, _touch in trace:
        lengths = []
        leaf.update_v3(leaf.decode(prev), d[ray], count, lengths)
        fails += not lengths[1] > F(1e-6)
    counts["second_length_test_fails"] = int(fails)
    inc = G["case_inc_mean"]
    fx, fy = inc & 0x3FFF, (inc >> 15) & 0x3FFF
    for name, field in (("x", fx), ("y", fy)):
        counts["field_%s_0" % name] = int(np.count_nonzero(field == 0))
        counts["field_%s_16383" % name] = int(np.count_nonzero(field == 16383))
    far = cs.target >= S.TARGETS_PER_REGION
    cast_first = cs.rays[0::2].astype(F) - cs.rays[1::2].astype(F)
    counts["far_cast_order_matters"] = int(np.count_nonzero(far & np.any(_bits(cast_first) != _bits(d), axis=1)))
    # (voxel, call) groups in calls of 97 rays
    vox = [tuple(v) for v in cs.voxel_ids().tolist()]
    not_max = not_min = 0
    for sl in cs.calls(97):
        groups = {}
        for ray in range(sl.start, sl.stop):
            groups.setdefault(vox[ray], []).append(cs.stamps[ray])
        not_max += sum(1 for g in groups.values() if g[-1] != max(g))
        not_min += sum(1 for g in groups.values() if g[-1] != min(g))
    counts["groups_last_not_max"], counts["groups_last_not_min"] = not_max, not_min
    k = cs.stamp_rank - S.FIRST_STAMP_RANK
    plain = cs.stamps == 100.0 + S.TIME_BASE_STEP * cs.stamp_rank.astype(np.float64)
    counts["exact_ms_truncates_to_k_minus_1"] = int(np.count_nonzero(
        plain & (k >= 1) & (G["case_touch"].astype(np.int64) == k - 1)))
    q = (cs.stamps - cs.stamps[0]) / 0.001
    counts["stamps_before_base"] = int(np.count_nonzero(q < 0))
    counts["stamps_beyond_2^32_ms"] = int(np.count_nonzero(q >= 2.0**32))
    equal = 0
    for t in (2, 19):
        for rnd in range(S.ROUNDS):
            sel = (cs.target == t) & (cs.round_of == rnd)
            equal += int(sel.sum() > 1 and len(set(cs.stamps[sel].tolist())) == 1)
    counts["voxel_rounds_with_equal_stamps"] = equal
    for name, value in counts.items():
        print("%-36s %d" % (name, value))
    assert counts["prev_normal_nan_z"] >= 200
    assert counts["incident_len2_le_1e-6"] >= 50 and counts["incident_len2_in_1e-6_4e-6"] >= 50
    assert counts["start_equals_end"] >= 1
    assert counts["second_length_test_fails"] >= 50
    assert min(counts["field_x_0"], counts["field_x_16383"], counts["field_y_0"], counts["field_y_16383"]) >= 1
    assert counts["far_cast_order_matters"] >= 50
    assert counts["groups_last_not_max"] >= 100 and counts["groups_last_not_min"] >= 100
    assert counts["exact_ms_truncates_to_k_minus_1"] >= 100
    assert counts["stamps_before_base"] >= 20 and counts["stamps_beyond_2^32_ms"] >= 5
    assert counts["voxel_rounds_with_equal_stamps"] >= 10


def _differs(a, b):
    return sum(a[0][k] != b[0][k] for k in a[0]) + sum(a[1][k] != b[1][k] for k in a[1])


@pytest.mark.parametrize("name", sorted(S.VARIANTS))
def test_wrong_variant_is_detected(cs, truth, name):
    leaf_sw, replay_sw = S.VARIANTS[name]
    if name == "nan_dropping_clamps":
        rows = G["enc_in"].view(F)
        wrong = np.array([S.NumpyLeaf(**leaf_sw).encode(r) for r in rows], dtype=np.uint32)
        assert np.count_nonzero(wrong != G["enc_out"]) >= 1
        return
    if name == "ignore_zero_normal_rule":
        prior = S.prior_counts(cs)
        right = S.replay(cs, S.NumpyLeaf(), prior_counts=prior)
        wrong = S.replay(cs, S.NumpyLeaf(**leaf_sw), prior_counts=prior, **replay_sw)
        assert _differs(right, wrong) >= 1
        return
    # one call and calls of 97 rays, each with a mean layer (the weight variants need one)
    for size in (None, 97):
        wrong = S.replay(cs, S.NumpyLeaf(**leaf_sw), with_mean=True, call_size=size, **replay_sw)
        assert _differs(truth[(True, size)], wrong) >= 1, size
