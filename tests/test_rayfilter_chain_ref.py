"""CPU: the host form of ohm_amd.rayfilter.DeviceRayFilter against the independent model of the device ray-filter chain
(tests/rayfilter_chain_ref.py) over the edge list and 2 000 random rays (tests/rayfilter_chain_cases.py): keep, both
points and flags, bit for bit (a NaN equals a NaN).  Where no NaN meets a box stage it also equals the existing
single-stage factories of rayfilter.py; the NaN-end clipToBounds ray gets the reference's answer."""
import math

import numpy as np
import pytest

import rayfilter_chain_cases as cases
import rayfilter_chain_ref as ref
from ohm_amd import rayfilter as RF


@pytest.mark.parametrize("chain_name", sorted(cases.CHAINS))
def test_host_form_equals_model(chain_name):
    rays = cases.all_rays()
    f = cases.device_filter(cases.CHAINS[chain_name])
    keep, starts, ends, flags = f(rays[0::2], rays[1::2])
    out = np.empty_like(rays)
    out[0::2], out[1::2] = starts, ends
    cases.assert_equals_model(chain_name, keep, out, flags, "DeviceRayFilter host form")


def test_host_form_leaves_its_input_alone():
    rays = cases.all_rays().copy()
    before = rays.copy()
    cases.device_filter(cases.CHAINS["four_stages"])(rays[0::2], rays[1::2])
    assert cases.same_bits(rays, before).all()


@pytest.mark.parametrize("chain_name", cases.SINGLE_STAGE)
def test_equals_existing_single_stage_filters_without_nan(chain_name):
    stage = cases.CHAINS[chain_name][0]
    existing = {"clip": lambda: RF.clip_ray_filter(stage[1]),
                "clip_bounded": lambda: RF.clip_bounded(RF.Aabb(stage[1], stage[2])),
                "clip_to_bounds": lambda: RF.clip_to_bounds(RF.Aabb(stage[1], stage[2]))}[stage[0]]()
    rays = cases.all_rays()
    clean = ~np.isnan(rays[0::2]).any(axis=1) & ~np.isnan(rays[1::2]).any(axis=1)
    clean &= ~(np.abs(rays[0::2]) == 1e200).any(axis=1)  # (the existing factories warn about the overflowing square)
    starts, ends = rays[0::2][clean], rays[1::2][clean]
    keep_a, starts_a, ends_a, flags_a = existing(starts.copy(), ends.copy())
    keep_b, starts_b, ends_b, flags_b = cases.device_filter([stage])(starts, ends)
    assert np.array_equal(keep_a, keep_b)
    kept = keep_a
    # (the per-ray reference form flags a rejected ray invalid; the existing factories report flags of kept rays only)
    assert np.array_equal(np.asarray(flags_a)[kept], flags_b[kept])
    assert cases.same_bits(np.asarray(starts_a)[kept], starts_b[kept]).all()
    assert cases.same_bits(np.asarray(ends_a)[kept], ends_b[kept]).all()
    assert (flags_b[~kept] & RF.kRffInvalid).all()


def test_nan_end_clip_to_bounds_is_the_references():
    """Aabb::contains is !any(max < p) && !any(min > p): a NaN coordinate fails both comparisons, the end counts as
    contained and the sample is suppressed (kRffClippedEnd).  rayfilter.Aabb.contains says outside: existing behaviour."""
    box = RF.Aabb(*cases.BOX)
    start = np.array([[0.0, 0.0, 0.0]])
    end = np.array([[math.nan, 0.5, 0.5]])
    keep, _, ends, flags = RF.on_device(RF.clip_to_bounds_stage(box))(start, end)
    assert keep[0] and flags[0] == RF.kRffClippedEnd and math.isnan(ends[0, 0])
    k, _, _, f = ref.chain([("clip_to_bounds",) + cases.BOX], start[0], end[0])
    assert k and f == ref.kRffClippedEnd
    _, _, _, old_flags = RF.clip_to_bounds(box)(start, end)
    assert old_flags[0] == 0
    # a NaN ray passes clipBounded unflagged: the box filters have no validity test of their own
    keep, _, _, flags = RF.on_device(RF.clip_bounded_stage(box))(start, end)
    assert keep[0] and flags[0] == 0


def test_chain_semantics_on_named_rays():
    """A few results spelled out, so that model and implementation cannot agree on a wrong reading."""
    names, rays = cases.edge_rays()
    at = names.index

    def one(chain_name, ray):
        keep, out, flags = cases.model(chain_name)
        i = at(ray)
        return bool(keep[i]), out[2 * i].tolist(), out[2 * i + 1].tolist(), int(flags[i])

    assert one("clip_bounded", "inside") == (True, [0, 0, 0], [1, 1, 0.5], 0)
    keep, start, end, flags = one("clip_bounded", "crossing")
    assert keep and flags == (ref.kRffClippedStart | ref.kRffClippedEnd)
    assert abs(start[0] + 1.0) < 1e-12 and abs(end[0] - 2.0) < 1e-12  # origin + dir * t: not clamped to the face
    assert one("clip_bounded", "outside_stops_short") == (True, [-5, 0, 0], [-2, 0, 0], 0)  # the reference keeps it
    assert one("clip_bounded", "outside_line_misses")[0] and one("clip_bounded", "outside_line_misses")[3] == 0
    assert one("clip_bounded", "end_on_face_from_inside") == (True, [0, 0, 0], [2, 0, 0], 0)  # t == length: not clipped
    assert one("clip_bounded", "d2_under_1e-9")[3] == 0
    assert one("clip_to_bounds", "end_on_box_min")[3] == ref.kRffClippedEnd
    assert one("clip_to_bounds", "end_on_box_max")[3] == ref.kRffClippedEnd
    assert not one("good_6", "start_nan_x")[0] and one("good_6", "start_nan_x")[3] == ref.kRffInvalid
    assert one("clip_just_under_5", "length_5")[3] == ref.kRffClippedEnd
    assert one("clip_exactly_5", "length_5")[3] == 0
    assert one("clip_just_over_5", "length_5")[3] == 0
    assert not one("good_just_under_5", "length_5")[0] and one("good_just_over_5", "length_5")[0]
    # a stage sees the ray as the one before left it: the 3.5 m entering ray is cut to 3 m (its end stays in the box),
    # then its start is moved to the face x = -1; the flags of both stages are OR-ed
    keep, start, end, flags = one("clip_then_clip_bounded", "entering")
    assert keep and flags == (ref.kRffClippedStart | ref.kRffClippedEnd)
    assert abs(start[0] + 1.0) < 1e-12 and abs(math.dist([-3, 0, 0], end) - 3.0) < 1e-12
    # the first stage that rejects ends the chain: the 7 m crossing ray never reaches clipBounded
    assert one("good_then_clip_bounded", "crossing") == (False, [-3, 0, 0.2], [4, 0.3, 0.3], ref.kRffInvalid)


def test_stage_limit_and_types():
    box = RF.Aabb(*cases.BOX)
    with pytest.raises(ValueError):
        RF.on_device(*([RF.good_ray(1.0)] * (RF.kMaxStages + 1)))
    with pytest.raises(ValueError):
        RF.on_device(RF.clip_bounded(box))  # a host callable is not a stage
    assert len(RF.on_device().stages) == 0
