"""The edge list of the device ray-filter chain: not a test.

Rays are listed against the box (-1, -1, -0.5)-(2, 1.5, 1); every chain of CHAINS is run over every ray of edge_rays()
and over 2 000 seeded random rays around the box.  Stages are the tuples of tests/rayfilter_chain_ref.py.
"""
import functools
import math

import numpy as np

import rayfilter_chain_ref

BOX = ((-1.0, -1.0, -0.5), (2.0, 1.5, 1.0))
BODY = ((-0.3, -0.3, -0.2), (0.3, 0.3, 0.2))        # a robot body inside BOX, for clipToBounds
FLAT = ((-1.0, -1.0, 0.25), (2.0, 1.5, 0.25))       # min == max on z
INVERTED = ((2.0, -1.0, -0.5), (-1.0, 1.5, 1.0))    # min > max on x
NAN_BOX = ((-1.0, math.nan, -0.5), (2.0, 1.5, 1.0))

nan, inf = math.nan, math.inf

EDGE_RAYS = [
    ("inside", (0, 0, 0), (1, 1, 0.5)),
    ("crossing", (-3, 0, 0.2), (4, 0.3, 0.3)),
    ("entering", (-3, 0, 0), (0.5, 0.2, 0.1)),
    ("leaving", (0.5, 0.2, 0.1), (4, 0, 0)),
    ("outside_line_misses", (-3, 5, 0), (4, 6, 0)),
    ("outside_stops_short", (-5, 0, 0), (-2, 0, 0)),
    ("outside_points_away", (-2, 0, 0), (-5, 0, 0)),
    ("in_face_y_max", (-3, 1.5, 0), (4, 1.5, 0)),            # zero y component, origin on the plane: 0 x inf
    ("in_face_z_min", (-3, 0.25, -0.5), (4, 0.5, -0.5)),
    ("in_face_inside", (0, 1.5, 0), (1, 1.5, 0.5)),
    ("parallel_outside", (-3, 1.75, 0), (4, 1.75, 0)),       # zero y component off the box: +-inf times
    ("axis_aligned_through", (0.5, -4, 0.25), (0.5, 4, 0.25)),
    ("start_on_face", (-1, 0, 0), (1, 0.5, 0.5)),
    ("start_on_face_leaving", (-1, 0, 0), (4, 0.5, 0.5)),
    ("end_on_face_from_inside", (0, 0, 0), (2, 0, 0)),       # t_exit == length
    ("end_on_face_from_outside", (-3, 0, 0), (-1, 0, 0)),    # t_entry == length
    ("through_edge", (-2, -2, 0), (0, 0, 0)),
    ("through_edge_outside", (-2, 0, 0), (0, -2, 0)),        # touches the edge x = -1, y = -1 only
    ("through_corner", (-2, -2, -1.5), (0, 0, 0.5)),
    ("through_corner_outside", (-3, -1, -0.5), (-1, -3, -0.5)),
    ("d2_under_1e-9", (-1.00001, 0, 0), (-1.00001 + 3.1e-5, 0, 0)),
    ("d2_over_1e-9", (-1.00001, 0, 0), (-1.00001 + 3.2e-5, 0, 0)),
    ("zero_length_inside", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    ("zero_length_outside", (5, 5, 5), (5, 5, 5)),
    ("end_on_box_min", (-3, -3, -3), (-1, -1, -0.5)),
    ("end_on_box_max", (4, 4, 4), (2, 1.5, 1)),
    ("end_on_box_min_from_inside", (0, 0, 0), (-1, -1, -0.5)),
    ("end_on_box_max_from_inside", (0, 0, 0), (2, 1.5, 1)),
    ("end_in_body", (1.5, 1, 0.5), (0.1, 0.1, 0.1)),
    ("end_on_body_face", (1.5, 0, 0), (0.3, 0, 0)),
    ("length_5", (0, 0, 0), (3, 4, 0)),
    ("length_5_outside", (-4, -4, 0.25), (-1, 0, 0.25)),
    ("start_nan_x", (nan, 0, 0), (1, 1, 0.5)),
    ("start_nan_z", (0, 0, nan), (4, 0, 0)),
    ("start_pinf_y", (0, inf, 0), (1, 1, 0.5)),
    ("start_ninf_x", (-inf, 0, 0), (1, 1, 0.5)),
    ("end_nan_x", (0, 0, 0), (nan, 1, 0.5)),
    ("end_nan_z_outside", (-3, 0, 0), (0.5, 0.2, nan)),
    ("end_pinf_x", (0, 0, 0), (inf, 0, 0)),
    ("end_ninf_z", (0, 0, 0), (1, 1, -inf)),
    ("all_nan", (nan, nan, nan), (nan, nan, nan)),
    ("huge", (-1e200, 0, 0), (1e200, 0.5, 0.5)),             # d2 overflows to inf
]

CHAINS = {
    "good_6": [("good", 6.0)],
    "good_0": [("good", 0.0)],
    "clip_3": [("clip", 3.0)],
    "clip_just_under_5": [("clip", 4.999999999)],
    "clip_exactly_5": [("clip", 5.0)],
    "clip_just_over_5": [("clip", 5.000000001)],
    "good_just_under_5": [("good", 4.999999999)],
    "good_just_over_5": [("good", 5.000000001)],
    "clip_bounded": [("clip_bounded",) + BOX],
    "clip_to_bounds": [("clip_to_bounds",) + BOX],
    "clip_to_bounds_body": [("clip_to_bounds",) + BODY],
    "clip_bounded_flat": [("clip_bounded",) + FLAT],
    "clip_to_bounds_flat": [("clip_to_bounds",) + FLAT],
    "clip_bounded_inverted": [("clip_bounded",) + INVERTED],
    "clip_to_bounds_inverted": [("clip_to_bounds",) + INVERTED],
    "clip_bounded_nan_box": [("clip_bounded",) + NAN_BOX],
    "good_nan_range": [("good", nan)],
    "good_then_clip_bounded": [("good", 6.0), ("clip_bounded",) + BOX],
    "clip_then_clip_bounded": [("clip", 3.0), ("clip_bounded",) + BOX],
    "clip_bounded_then_clip_to_bounds": [("clip_bounded",) + BOX, ("clip_to_bounds",) + BODY],
    "clip_bounded_then_clip": [("clip_bounded",) + BOX, ("clip", 1.25)],
    "four_stages": [("good", 50.0), ("clip_bounded",) + BOX, ("clip_to_bounds",) + BODY, ("clip", 2.5)],
}

# chains whose every stage treats NaN like rayfilter.py's own filters (no box stage sees a NaN ray): the existing
# single-stage factories give the same result
SINGLE_STAGE = ("clip_3", "clip_bounded", "clip_to_bounds", "clip_to_bounds_body", "clip_bounded_flat")


def edge_rays():
    """(names, (2N, 3) float64 array of origin / sample pairs)."""
    names = [name for name, _, _ in EDGE_RAYS]
    rays = np.empty((2 * len(EDGE_RAYS), 3), dtype=np.float64)
    for i, (_, start, end) in enumerate(EDGE_RAYS):
        rays[2 * i] = start
        rays[2 * i + 1] = end
    return names, rays


def random_rays(n=2000, seed=20250117, spread=3.0):
    """Seeded rays around BOX: starts and ends uniform in the box grown by `spread` metres, a third of the starts pulled
    inside the box (a sensor in it), coordinates rounded to 1/4 m for a tenth (rays that land exactly on faces)."""
    rng = np.random.default_rng(seed)
    lo = np.array(BOX[0]) - spread
    hi = np.array(BOX[1]) + spread
    starts = rng.uniform(lo, hi, size=(n, 3))
    ends = rng.uniform(lo, hi, size=(n, 3))
    inside = rng.random(n) < (1.0 / 3.0)
    starts[inside] = rng.uniform(np.array(BOX[0]), np.array(BOX[1]), size=(int(inside.sum()), 3))
    coarse = rng.random(n) < 0.1
    starts[coarse] = np.round(starts[coarse] * 4.0) / 4.0
    ends[coarse] = np.round(ends[coarse] * 4.0) / 4.0
    rays = np.empty((2 * n, 3), dtype=np.float64)
    rays[0::2] = starts
    rays[1::2] = ends
    return rays


@functools.lru_cache(maxsize=None)
def all_rays():
    """Edge rays followed by the random rays (shared: do not write to it)."""
    rays = np.concatenate([edge_rays()[1], random_rays()])
    rays.setflags(write=False)
    return rays


def ray_name(index):
    names = edge_rays()[0]
    return names[index] if index < len(names) else "random_%d" % (index - len(names))


def run_model(stages, rays):
    """The model over a ray array: (keep bool array, (2N, 3) moved rays, uint8 flags)."""
    keep, out, flags = rayfilter_chain_ref.run(stages, np.asarray(rays).tolist())
    return (np.array(keep, dtype=bool), np.array(out, dtype=np.float64).reshape(-1, 3),
            np.array(flags, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def model(chain_name):
    """The model's result for one of CHAINS over all_rays(), computed once per session."""
    result = run_model(CHAINS[chain_name], all_rays())
    for part in result:
        part.setflags(write=False)
    return result


def same_bits(a, b):
    """Element-wise: identical bit patterns, or both NaN (IEEE 754 leaves the sign and payload of a generated NaN to the
    implementation: the host's, the device's and Python's differ in the sign bit)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def assert_equals_model(chain_name, keep, rays_out, flags, what):
    """keep / moved rays / flags of an implementation over all_rays() against the model, bit for bit."""
    m_keep, m_rays, m_flags = model(chain_name)
    keep = np.asarray(keep, dtype=bool)
    flags = np.asarray(flags, dtype=np.uint8)
    rays_out = np.asarray(rays_out, dtype=np.float64).reshape(-1, 3)
    bad = (keep != m_keep) | (flags != m_flags) | \
        ~same_bits(rays_out[0::2], m_rays[0::2]).all(axis=1) | ~same_bits(rays_out[1::2], m_rays[1::2]).all(axis=1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s, chain %s: %d rays differ from the model; first %s: keep %s / %s, flags %d / %d, "
                             "start %r / %r, end %r / %r" % (what, chain_name, int(bad.sum()), ray_name(i), keep[i],
                                                             m_keep[i], flags[i], m_flags[i], rays_out[2 * i].tolist(),
                                                             m_rays[2 * i].tolist(), rays_out[2 * i + 1].tolist(),
                                                             m_rays[2 * i + 1].tolist()))


def device_filter(stages):
    """The ohm_amd DeviceRayFilter of a model chain."""
    from ohm_amd import rayfilter as RF
    made = []
    for st in stages:
        if st[0] == "good":
            made.append(RF.good_ray(st[1]))
        elif st[0] == "clip":
            made.append(RF.clip_ray(st[1]))
        elif st[0] == "clip_bounded":
            made.append(RF.clip_bounded_stage(RF.Aabb(st[1], st[2])))
        else:
            made.append(RF.clip_to_bounds_stage(RF.Aabb(st[1], st[2])))
    return RF.on_device(*made)
