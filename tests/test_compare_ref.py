"""CPU: the restatement of ohm::compare (tests/compare_ref.py) against what CompareMaps.cpp:58-75 says by hand (the K4
truth table), against exact rational arithmetic for the one fp32 subtraction, and its stop-at-first closed form against
the sequential walk."""
from fractions import Fraction

import numpy as np
import pytest

import compare_cases as cases
import compare_ref as R


@pytest.mark.parametrize("row", cases.TRUTH_F32, ids=[r[0] for r in cases.TRUTH_F32])
def test_truth_table_f32(row):
    _, val, ref, eps, want = row
    got = R.compare_voxel([val], [ref], 0x1, 0 if eps is None else 1, [eps or 0])
    assert (got == 0) is want
    mask, _ = R.member_masks(np.array([[val]], dtype=np.uint32), np.array([[ref]], dtype=np.uint32), 0x1,
                             0 if eps is None else 1, [eps or 0])
    assert (int(mask[0]) == 0) is want


@pytest.mark.parametrize("row", cases.TRUTH_U32, ids=[r[0] for r in cases.TRUTH_U32])
def test_truth_table_u32(row):
    _, val, ref, eps, want = row
    got = R.compare_voxel([val], [ref], 0x0, 0 if eps is None else 1, [eps or 0])
    assert (got == 0) is want
    mask, diffs = R.member_masks(np.array([[val]], dtype=np.uint32), np.array([[ref]], dtype=np.uint32), 0x0,
                                 0 if eps is None else 1, [eps or 0])
    assert (int(mask[0]) == 0) is want
    assert int(diffs[0, 0]) == abs(val - ref)


def exact(bits):
    return Fraction(float(R.f32(bits)))


def round_to_f32_bits(x):
    """A non-negative rational rounded to the nearest float32, ties to even, subnormals kept, overflow to +inf."""
    if x == 0:
        return 0
    e = -126
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    quantum = Fraction(2) ** (e - 23)
    q = x / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    value = n * quantum
    if value >= Fraction(2) ** 128:
        return cases.INF
    return R.bits_of(np.float32(float(value)))


def _ulps(bits, k):
    return bits + k  # (positive finite floats: the next pattern is the next value)


def near_eps_pairs():
    """(val, ref, eps): pairs whose exact difference lies within one ulp of eps on either side, subnormal differences and
    overflow."""
    out = []
    for a, eps in ((0x3f8ccccd, 0x3dcccccd), (0x40490fdb, 0x3a83126f), (0x42c80000, 0x3f800000), (0x3f800000, 0x33d6bf95),
                   (0x00c00000, 0x00000003), (0x7f000000, 0x7e800000)):
        target = exact(a) + exact(eps)
        b = round_to_f32_bits(target)
        if b == cases.INF:
            continue
        for k in (-2, -1, 0, 1, 2):
            out.append((_ulps(b, k), a, eps))
            out.append((a, _ulps(b, k), eps))
            out.append((_ulps(b, k) | 0x80000000, a | 0x80000000, eps))  # both negative: the swap goes the other way
    quarter = 0xbe800000  # -0.25: hi = eps' - 0.25 is representable, so hi - lo is eps' exactly, eps' = eps +- k ulps
    for eps in (0x3f8ccccd, 0x3fc00001):
        for k in (-2, -1, 0, 1, 2):
            hi = round_to_f32_bits(exact(eps + k) - Fraction(1, 4))
            assert exact(hi) + Fraction(1, 4) == exact(eps + k)
            out.append((hi, quarter, eps))
            out.append((quarter, hi, eps))
    out.append((0x4b800001, 0xbf800000, 0x4b800001))  # 2^24 + 2 + 1: a tie, rounds to even 2^24 + 4 > eps = 2^24 + 2
    out.append((0xbf800000, 0x4b800001, 0x4b800002))  # ... and == eps = 2^24 + 4
    for k in (1, 2, 3, 5):
        out.append((cases.MIN_NORMAL + k, cases.MIN_NORMAL, k))      # subnormal difference == eps
        out.append((cases.MIN_NORMAL + k, cases.MIN_NORMAL, k - 1))  # ... one subnormal more than eps
        out.append((k, 0x80000000 | k, 2 * k))                       # +-subnormals
    out.append((cases.FMAX, cases.NFMAX, cases.FMAX))                # overflow
    out.append((cases.FMAX, 0xff000000, cases.FMAX))                 # FLT_MAX + 2^127: overflow as well
    out.append((0x7f000000, 0xff000000, cases.FMAX))                 # 2^127 + 2^127 = 2^128: inf
    out.append((0x7f000000, 0xfeffffff, cases.FMAX))                 # just below: finite
    return out


@pytest.mark.parametrize("val,ref,eps", near_eps_pairs())
def test_fp32_difference_is_the_correctly_rounded_one(val, ref, eps):
    hi, lo = max(exact(val), exact(ref)), min(exact(val), exact(ref))
    want_bits = round_to_f32_bits(hi - lo)
    want_pass = hi == lo or (want_bits != cases.INF and exact(want_bits) <= exact(eps))
    ok, diff = R.compare_datum(val, ref, 1, eps)
    assert diff == want_bits and ok is want_pass
    mask, diffs = R.member_masks(np.array([[val]], dtype=np.uint32), np.array([[ref]], dtype=np.uint32), 0x1, 1, [eps])
    assert int(diffs[0, 0]) == want_bits and (int(mask[0]) == 0) is want_pass


def test_the_pairs_straddle_eps():
    """The condition the test above exists for: passes and failures both occur, among them pairs that differ from eps by
    exactly one ulp of the difference."""
    verdicts = [R.compare_datum(v, r, 1, e)[0] for v, r, e in near_eps_pairs()]
    assert verdicts.count(True) >= 20 and verdicts.count(False) >= 20
    diffs = [R.compare_datum(v, r, 1, e)[1] - e for v, r, e in near_eps_pairs()]
    assert {-1, 0, 1} <= set(diffs)


def _small_maps(layer, missing=(), plants=()):
    dims = (4, 3, 2)
    regions = [(0, 0, 0), (1, 0, 0), (-1, 1, 0), (0, 0, -1), (2, -1, 1)]
    ev, ref = cases.planted_pair(layer, dims, regions, plants)
    for region in missing:
        del ev[region]
    ev[(9, 9, 9)] = cases.base_block(layer, dims, 99)  # a region only eval holds: ignored
    return dims, ev, ref


@pytest.mark.parametrize("layer", ["occupancy", "mean", "covariance"])
@pytest.mark.parametrize("missing,plants", [
    ((), ()),
    ((), [((1, 0, 0), 17, 0), ((0, 0, 0), 5, 0)]),
    ([(-1, 1, 0)], [((2, -1, 1), 3, 0)]),                    # a missing region ahead of a value mismatch
    ([(2, -1, 1)], [((-1, 1, 0), 23, 0), ((-1, 1, 0), 0, 0)]),  # a value mismatch ahead of a missing region
    ([(0, 0, -1)], ()),                                       # the first region in order is missing
])
def test_stop_at_first_closed_form_equals_the_walk(layer, missing, plants):
    dims, ev, ref = _small_maps(layer, missing, plants)
    assert R.region_order(ref)[0] == (0, 0, -1) and R.region_order(ref)[-1] == (2, -1, 1)
    passed, failed, where = R.walk_stop_at_first(ev, ref, layer, dims)
    res, keys, gone = R.compare_voxels(ev, ref, layer, dims, flags=0, mismatch_capacity=4, missing_capacity=4)
    assert (res["voxels_passed"], res["voxels_failed"]) == (passed, failed)
    assert res["mismatch_count"] + res["missing_count"] == failed == len(keys) + len(gone)
    assert res["member_max_diff"] == [0] * R.MAX_MEMBERS
    if where is None:
        assert passed == 24 * (5 - len(missing)) and not missing
    elif where[2] is None:
        assert [tuple(g) for g in gone.tolist()] == [where[0]] and res["member_failed"] == [0] * R.MAX_MEMBERS
    else:
        region, index, mask = where
        assert tuple(keys[0]["region"]) == region and int(keys[0]["voxel"][3]) == mask
        assert tuple(int(v) for v in keys[0]["voxel"][:3]) == (index % 4, (index // 4) % 3, index // 12)
        assert res["member_failed"] == [(mask >> i) & 1 for i in range(R.MAX_MEMBERS)]
    # the ordinal of the first failure, from the full comparison
    full, all_keys, all_gone = R.compare_voxels(ev, ref, layer, dims, flags=R.CONTINUE, mismatch_capacity=1 << 20,
                                                missing_capacity=16)
    assert full["voxels_passed"] + full["voxels_failed"] == 24 * 5
    assert full["voxels_failed"] == len(all_keys) + 24 * len(all_gone) and len(all_gone) == len(missing)
    assert (failed == 0) == (full["voxels_failed"] == 0)


def test_key_list_absent_and_repeated():
    dims, ev, ref = _small_maps("occupancy", missing=[(1, 0, 0)], plants=[((0, 0, 0), 2, 0)])
    keys = [(1, 0, 0), (0, 0, 0), (7, 7, 7), (0, 0, 0), (9, 9, 9)]
    res, listed, gone = R.compare_voxels(ev, ref, "occupancy", dims, flags=R.CONTINUE, keys=keys, mismatch_capacity=8,
                                         missing_capacity=8)
    assert (res["keys_absent"], res["regions_compared"], res["regions_missing"]) == (2, 1, 1)
    assert (res["voxels_passed"], res["voxels_failed"]) == (23, 25)
    assert len(listed) == 1 and gone.tolist() == [[1, 0, 0]]


def test_configure_tolerance_reads_as_the_members_type():
    """A float 1.0 configured on a u32 member is eps = 0x3f800000 words, as in the reference."""
    assert R.compare_voxel([0, 0x3f800000], [0, 0], 0x0, 0x2, [0, R.bits_of(1.0)]) == 0
    assert R.compare_voxel([0, 0x3f800001], [0, 0], 0x0, 0x2, [0, R.bits_of(1.0)]) == 0x2
