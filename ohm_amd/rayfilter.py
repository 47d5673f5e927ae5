"""Ray filters for GpuMap.setRayFilter -- the reference's `RayFilterFunction`s (ohm/RayFilter.h:45-100,
ohm/RayFilter.cpp:12-93), vectorised over a batch.

A filter here is a callable `f(starts, ends) -> (keep, starts, ends, flags)`: `starts` / `ends` are (N, 3) float64
arrays, `keep` a bool mask of the rays that survive, `flags` the per-ray `RayFilterFlag` bits (uint8).  The reference
calls its filter once per ray with pointers (`bool(dvec3 *start, dvec3 *end, unsigned *filter_flags)`); the arithmetic
below follows the same statements ray by ray, so results are those of the per-ray form.
"""
import numpy as np

kRffInvalid = 1  # ohm/RayFilter.h:21-29
kRffClippedStart = 2
kRffClippedEnd = 4


def _finite(v):
    return np.all(np.isfinite(v), axis=1)


def good_ray_filter(max_range=0.0):
    """ohm::goodRayFilter (ohm/RayFilter.cpp:12-34): reject NaN / inf rays and rays longer than max_range (> 0)."""
    def f(starts, ends):
        ray = ends - starts
        len2 = (ray[:, 0] * ray[:, 0] + ray[:, 1] * ray[:, 1]) + ray[:, 2] * ray[:, 2]
        keep = _finite(starts) & _finite(ends)
        if max_range > 0:
            with np.errstate(invalid="ignore"):
                keep &= len2 <= max_range * max_range
        return keep, starts, ends, np.zeros(len(starts), dtype=np.uint8)
    return f


def clip_ray_filter(max_length):
    """ohm::clipRayFilter (ohm/RayFilter.cpp:37-58): shorten rays longer than max_length, flagging the clipped end."""
    def f(starts, ends):
        keep = _finite(starts) & _finite(ends)
        ray = ends - starts
        len2 = (ray[:, 0] * ray[:, 0] + ray[:, 1] * ray[:, 1]) + ray[:, 2] * ray[:, 2]
        with np.errstate(invalid="ignore"):
            clip = keep & (max_length > 0) & (len2 > max_length * max_length)
        ends = ends.copy()
        flags = np.zeros(len(starts), dtype=np.uint8)
        if clip.any():
            unit = ray[clip] / np.sqrt(len2[clip])[:, None]
            ends[clip] = starts[clip] + unit * max_length
            flags[clip] |= kRffClippedEnd
        return keep, starts, ends, flags
    return f


class Aabb:
    """The parts of ohm::Aabb (ohm/Aabb.h) the ray filters use."""

    def __init__(self, min_ext, max_ext):
        self.min = np.asarray(min_ext, dtype=np.float64).reshape(3)
        self.max = np.asarray(max_ext, dtype=np.float64).reshape(3)

    def contains(self, points):
        """Aabb::contains (ohm/Aabb.h:301-312, epsilon 0): closed box."""
        return np.all((points >= self.min) & (points <= self.max), axis=1)

    def _ray_intersect(self, origin, direction):
        """Aabb::rayIntersect (ohm/Aabb.h:330-383): slab test; returns (hit, t_entry, t_exit)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / direction
            sign = (direction < 0.0).astype(np.int64)
            corners = np.stack([self.min, self.max])  # [2, 3]
            near = corners[sign, np.arange(3)]        # (N, 3): corners_[sign[a]][a]
            far = corners[1 - sign, np.arange(3)]
            t0 = (near[:, 0] - origin[:, 0]) * inv[:, 0]
            t1 = (far[:, 0] - origin[:, 0]) * inv[:, 0]
            miss = np.zeros(len(origin), dtype=bool)
            for a in (1, 2):
                tmin = (near[:, a] - origin[:, a]) * inv[:, a]
                tmax = (far[:, a] - origin[:, a]) * inv[:, a]
                miss |= (t0 > tmax) | (tmin > t1)
                t0 = np.where((tmin > t0) | np.isnan(t0), tmin, t0)
                t1 = np.where((tmax < t1) | np.isnan(t1), tmax, t1)
        return ~miss, t0, t1

    def clip_line(self, starts, ends):
        """Aabb::clipLine (ohm/Aabb.h:386-446, allow_clamp false): returns (clipped_any, starts, ends, clip_flags) with
        clip flag 1 = start moved, 2 = end moved."""
        origin = starts
        direction = ends - starts
        d2 = (direction[:, 0] * direction[:, 0] + direction[:, 1] * direction[:, 1]) + direction[:, 2] * direction[:, 2]
        live = ~(d2 < 1e-9)  # degenerate rays are returned untouched
        with np.errstate(divide="ignore", invalid="ignore"):
            length = np.sqrt(d2)
            unit = direction / length[:, None]
        hit, t0, t1 = self._ray_intersect(origin, unit)
        hit &= live
        with np.errstate(invalid="ignore"):
            move_start = hit & (t0 > 0) & (t0 < length)
            move_end = hit & (t1 > 0) & (t1 < length)
        with np.errstate(invalid="ignore"):  # (degenerate rays carry NaN here and are not selected)
            new_starts = np.where(move_start[:, None], origin + unit * t0[:, None], starts)
            new_ends = np.where(move_end[:, None], origin + unit * t1[:, None], ends)
        flags = move_start.astype(np.uint8) * 1 + move_end.astype(np.uint8) * 2
        return move_start | move_end, new_starts, new_ends, flags


def clip_bounded(box):
    """ohm::clipBounded (ohm/RayFilter.cpp:61-78): clip each ray to `box`; a ray that was clipped and still has neither
    end inside the box is rejected."""
    def f(starts, ends):
        clipped, new_starts, new_ends, clip_flags = box.clip_line(starts, ends)
        reject = clipped & ~box.contains(new_starts) & ~box.contains(new_ends)
        flags = ((clip_flags & 1) != 0).astype(np.uint8) * kRffClippedStart + \
            ((clip_flags & 2) != 0).astype(np.uint8) * kRffClippedEnd
        return ~reject, new_starts, new_ends, flags
    return f


def clip_to_bounds(box):
    """ohm::clipToBounds (ohm/RayFilter.cpp:81-93): samples inside `box` are marked as clipped ends (no hit)."""
    def f(starts, ends):
        flags = box.contains(ends).astype(np.uint8) * kRffClippedEnd
        return np.ones(len(starts), dtype=bool), starts, ends, flags
    return f


# ----------------------------------------------------------------------------------------------------------------------
# The device filter chain (GpuMap.setRayFilter(DeviceRayFilter); include/ohmhip.h: ohmhip_map_set_ray_filter_stages).
#
# A chain is a tuple of stage descriptors -- the four stock filters above -- that the map evaluates on the device for
# every batch, in place of its built-in filter.  DeviceRayFilter is also a host callable of the form described at the top
# of this file, with the device's semantics: stage i sees the ray as stage i - 1 left it, flags are OR-ed, the first
# stage that rejects ends the chain and the ray carries kRffInvalid.  Its Aabb::contains is the reference's own form,
# `!any(max < p) && !any(min > p)` (ohm/Aabb.h:301-312): a NaN coordinate counts as contained -- unlike Aabb.contains
# above, which keeps its earlier behaviour.
# ----------------------------------------------------------------------------------------------------------------------
kStageGood, kStageClip, kStageClipBounded, kStageClipToBounds = 1, 2, 3, 4  # OHMHIP_RFS_*
kMaxStages = 4  # OHMHIP_MAX_RAY_FILTER_STAGES


class RayFilterStage:
    """One stage of a device chain: `kind` (kStage*), `range` for the two range filters, `box` (an Aabb) for the two box
    filters."""

    def __init__(self, kind, range_=0.0, box=None):
        self.kind = int(kind)
        self.range = float(range_)
        self.box = box if box is not None else Aabb((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))

    def __repr__(self):
        return "RayFilterStage(%d, range=%r, box=(%r, %r))" % (self.kind, self.range, self.box.min.tolist(),
                                                               self.box.max.tolist())


def good_ray(max_range=0.0):
    """Stage form of goodRayFilter."""
    return RayFilterStage(kStageGood, max_range)


def clip_ray(max_length):
    """Stage form of clipRayFilter."""
    return RayFilterStage(kStageClip, max_length)


def clip_bounded_stage(box):
    """Stage form of clipBounded."""
    return RayFilterStage(kStageClipBounded, box=box)


def clip_to_bounds_stage(box):
    """Stage form of clipToBounds."""
    return RayFilterStage(kStageClipToBounds, box=box)


def _dot3(v):
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def _contains_reference(box, points):
    return ~np.any(box.max < points, axis=1) & ~np.any(box.min > points, axis=1)


def _stage_host(stage, starts, ends):
    """One stage over a batch: (verdict, starts, ends, flags) as the per-ray reference function gives them (the flags
    of a rejected ray are what the function had OR-ed in when it returned)."""
    n = len(starts)
    flags = np.zeros(n, dtype=np.uint8)
    with np.errstate(all="ignore"):
        if stage.kind in (kStageGood, kStageClip):
            good = _finite(starts) & _finite(ends)
            ray = ends - starts
            len2 = _dot3(ray)
            rng = stage.range
            if stage.kind == kStageGood:
                if not rng <= 0:
                    good = good & (len2 <= rng * rng)
            else:
                clip = good & (rng > 0) & (len2 > rng * rng)
                unit = ray / np.sqrt(len2)[:, None]
                ends = np.where(clip[:, None], starts + unit * rng, ends)
                flags[clip] |= kRffClippedEnd
            flags[~good] |= kRffInvalid
            return good, starts, ends, flags
        box = stage.box
        if stage.kind == kStageClipToBounds:
            flags[_contains_reference(box, ends)] |= kRffClippedEnd
            return np.ones(n, dtype=bool), starts, ends, flags
        # clipBounded over Aabb::clipLine (allow_clamp false) and Aabb::rayIntersect
        origin = starts
        direction = ends - starts
        d2 = _dot3(direction)
        live = ~(d2 < 1e-9)
        length = np.sqrt(d2)
        unit = direction / length[:, None]
        inv = 1.0 / unit
        negative = unit < 0.0
        near = np.where(negative, box.max, box.min)
        far = np.where(negative, box.min, box.max)
        t0 = (near[:, 0] - origin[:, 0]) * inv[:, 0]
        t1 = (far[:, 0] - origin[:, 0]) * inv[:, 0]
        miss = np.zeros(n, dtype=bool)
        for a in (1, 2):
            tmin = (near[:, a] - origin[:, a]) * inv[:, a]
            tmax = (far[:, a] - origin[:, a]) * inv[:, a]
            miss = (t0 > tmax) | (tmin > t1) | miss
            t0 = np.where((tmin > t0) | np.isnan(t0), tmin, t0)
            t1 = np.where((tmax < t1) | np.isnan(t1), tmax, t1)
        hit = live & ~miss
        move_start = hit & (t0 > 0) & (t0 < length)
        move_end = hit & (t1 > 0) & (t1 < length)
        starts = np.where(move_start[:, None], origin + unit * t0[:, None], starts)
        ends = np.where(move_end[:, None], origin + unit * t1[:, None], ends)
        reject = (move_start | move_end) & ~_contains_reference(box, starts) & ~_contains_reference(box, ends)
        flags[move_start & ~reject] |= kRffClippedStart
        flags[move_end & ~reject] |= kRffClippedEnd
        return ~reject, starts, ends, flags


class DeviceRayFilter:
    """A chain of up to kMaxStages stock filters for GpuMap.setRayFilter: evaluated on the device for every batch.
    Calling it runs the same chain on the host: f(starts, ends) -> (keep, starts, ends, flags), every ray reported,
    rejected ones with kRffInvalid and the points as the rejecting stage left them."""

    def __init__(self, *stages):
        if len(stages) > kMaxStages:
            raise ValueError("a device ray filter has at most %d stages" % kMaxStages)
        for stage in stages:
            if not isinstance(stage, RayFilterStage) or not kStageGood <= stage.kind <= kStageClipToBounds:
                raise ValueError("not a ray filter stage: %r" % (stage,))
        self.stages = tuple(stages)

    def __call__(self, starts, ends):
        starts = np.array(starts, dtype=np.float64).reshape(-1, 3)
        ends = np.array(ends, dtype=np.float64).reshape(-1, 3)
        alive = np.ones(len(starts), dtype=bool)
        flags = np.zeros(len(starts), dtype=np.uint8)
        for stage in self.stages:
            verdict, new_starts, new_ends, stage_flags = _stage_host(stage, starts, ends)
            starts = np.where(alive[:, None], new_starts, starts)
            ends = np.where(alive[:, None], new_ends, ends)
            flags[alive] |= stage_flags[alive]
            alive = alive & verdict
        flags[~alive] |= kRffInvalid
        return alive, starts, ends, flags


def on_device(*stages):
    """RF.on_device(RF.good_ray(r), RF.clip_bounded_stage(box), ...): the chain for GpuMap.setRayFilter."""
    return DeviceRayFilter(*stages)
