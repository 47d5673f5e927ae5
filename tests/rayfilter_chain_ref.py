"""An independent model of the device ray-filter chain: not a test.

One ray at a time on Python floats (IEEE binary64, every operation rounded once), written from the reference's
ohm/RayFilter.cpp:12-86 and ohm/Aabb.h:301-446 statement by statement.  It shares no code with ohm_amd/rayfilter.py.

A stage is a tuple: ("good", range), ("clip", range), ("clip_bounded", box_min, box_max) or
("clip_to_bounds", box_min, box_max).  chain(stages, start, end) -> (keep, start, end, flags): the ray as the chain
leaves it; flags are the OR-ed RayFilterFlag bits with kRffInvalid added when a stage rejected the ray.
"""
import math

kRffInvalid, kRffClippedStart, kRffClippedEnd = 1, 2, 4
KINDS = {"good": 1, "clip": 2, "clip_bounded": 3, "clip_to_bounds": 4}


def _div(a, b):
    """IEEE a / b (Python raises on a zero divisor)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _finite(v):
    return not any(math.isnan(x) for x in v) and not any(math.isinf(x) for x in v)


def _dot(v):
    return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def contains(box_min, box_max, p):
    """Aabb::contains, epsilon 0, through overlaps(): !any(max < p) && !any(min > p)."""
    max_less = any(box_max[a] < p[a] for a in range(3))
    min_greater = any(box_min[a] > p[a] for a in range(3))
    return not max_less and not min_greater


def ray_intersect(box_min, box_max, origin, direction):
    """Aabb::rayIntersect: (hit, t_entry, t_exit)."""
    inv = [_div(1.0, d) for d in direction]
    corners = (box_min, box_max)
    sign = [1 if d < 0.0 else 0 for d in direction]
    t0 = (corners[sign[0]][0] - origin[0]) * inv[0]
    t1 = (corners[1 - sign[0]][0] - origin[0]) * inv[0]
    tmin = (corners[sign[1]][1] - origin[1]) * inv[1]
    tmax = (corners[1 - sign[1]][1] - origin[1]) * inv[1]
    miss = (t0 > tmax) or (tmin > t1)
    t0 = tmin if (tmin > t0 or math.isnan(t0)) else t0
    t1 = tmax if (tmax < t1 or math.isnan(t1)) else t1
    tmin = (corners[sign[2]][2] - origin[2]) * inv[2]
    tmax = (corners[1 - sign[2]][2] - origin[2]) * inv[2]
    miss = (t0 > tmax) or (tmin > t1) or miss
    t0 = tmin if (tmin > t0 or math.isnan(t0)) else t0
    t1 = tmax if (tmax < t1 or math.isnan(t1)) else t1
    return (not miss), t0, t1


def clip_line(box_min, box_max, start, end):
    """Aabb::clipLine with allow_clamp false: (clipped, start, end, clip_flags); clip flag 1 start, 2 end."""
    origin = list(start)
    direction = _sub(end, start)
    d2 = _dot(direction)
    if d2 < 1e-9:
        return False, start, end, 0
    length = math.sqrt(d2)
    direction = [_div(d, length) for d in direction]
    hit, t0, t1 = ray_intersect(box_min, box_max, origin, direction)
    if not hit:
        return False, start, end, 0
    clip_flags = 0
    if t0 > 0 and t0 < length:
        start = [origin[a] + direction[a] * t0 for a in range(3)]
        clip_flags |= 1
    if t1 > 0 and t1 < length:
        end = [origin[a] + direction[a] * t1 for a in range(3)]
        clip_flags |= 2
    return clip_flags != 0, start, end, clip_flags


def stage(st, start, end, flags):
    """One reference filter function: (verdict, start, end, flags)."""
    kind = st[0]
    if kind == "good":
        max_range = st[1]
        good = _finite(start) and _finite(end)
        ray = _sub(end, start)
        good = good and (max_range <= 0 or _dot(ray) <= max_range * max_range)
        if not good:
            flags |= kRffInvalid
        return good, start, end, flags
    if kind == "clip":
        max_length = st[1]
        good = _finite(start) and _finite(end)
        ray = _sub(end, start)
        len2 = _dot(ray)
        if good and max_length > 0 and len2 > max_length * max_length:
            root = math.sqrt(len2)
            ray = [_div(r, root) for r in ray]
            end = [start[a] + ray[a] * max_length for a in range(3)]
            flags |= kRffClippedEnd
        if not good:
            flags |= kRffInvalid
        return good, start, end, flags
    box_min, box_max = st[1], st[2]
    if kind == "clip_bounded":
        clipped, start, end, clip_flags = clip_line(box_min, box_max, start, end)
        if clipped:
            if not contains(box_min, box_max, start) and not contains(box_min, box_max, end):
                return False, start, end, flags
        if clip_flags & 1:
            flags |= kRffClippedStart
        if clip_flags & 2:
            flags |= kRffClippedEnd
        return True, start, end, flags
    if kind == "clip_to_bounds":
        if contains(box_min, box_max, end):
            flags |= kRffClippedEnd
        return True, start, end, flags
    raise ValueError(kind)


def chain(stages, start, end):
    start = [float(x) for x in start]
    end = [float(x) for x in end]
    flags = 0
    for st in stages:
        keep, start, end, flags = stage(st, start, end, flags)
        if not keep:
            return False, start, end, flags | kRffInvalid
    return True, start, end, flags


def run(stages, rays):
    """rays: (2N, 3) array-like of origin / sample pairs.  Returns (keep list, moved rays as a list of 2N points,
    flags list)."""
    keep, out, flags = [], [], []
    for i in range(len(rays) // 2):
        k, s, e, f = chain(stages, rays[2 * i], rays[2 * i + 1])
        keep.append(k)
        out.append(s)
        out.append(e)
        flags.append(f)
    return keep, out, flags
