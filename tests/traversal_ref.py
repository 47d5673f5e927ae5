"""The traversal layer's exact fixed-point model (test infrastructure): tests/test_traversal_ref.py (CPU) ties it to the
CPU oracle and to its bounds, tests/test_gpu_traversal_states.py (-m gpu) holds the device to it bit for bit.

The layer holds, per voxel, the sum of the lengths of all rays inside it.  The CPU mapper adds one float32 per visit,
float32(t_exit - t_enter), and one per sample, float32(length - last_exit_range), to a float32 in ray order
(ohm/RayMapperOccupancy.cpp:166-173, :299-305).  The device follows a rule of its own:

  * the sample-side kernels add the samples' shares first, float32 adds in ray order;
  * every visit add a becomes rn_even(a * 2^unit_bits) units -- a 32-bit word per voxel and walk chunk; a word that
    wraps sends one carry of 2^32 units to a 64-bit accumulator, and the word is flushed there when the chunk ends;
  * once per batch, where the accumulator is not zero, layer = float32(float64(layer) + units * 2^-unit_bits).

visits() is the reference's line walk (ohm/LineWalkCompute.h:188-413, CPU instantiation: doubles) in Python floats:
one IEEE operation per step, no contraction.  cpu_adds() lists what the CPU mapper adds for one integrateRays call,
device_layer() applies the device's rule to them, exact_sum() is the exact sum both are measured against.

The bounds.  Let a voxel receive n visit adds and s share adds a_i (float32, exact_sum E = sum a_i over all calls) and
call u(x) = ulp32(x), the spacing of float32 at |x|.

  oracle:  the CPU adds them one at a time, each add rounding to nearest: the i-th add errs by at most u(p_i) / 2 with
           p_i the rounded partial sum it produced, so |oracle - E| <= (n + s) * u(max |p_i|) / 2, the maximum taken
           over the oracle's own partial sums (its planted start included).
  model:   a visit's units differ from a * 2^unit_bits by at most 1/2: round to nearest, and nothing is clamped by
           more -- a visit is at most a voxel diagonal, which unit_bits keeps below 2^31 units, and the only negative
           visit adds are those of an end point that the key maths rounded onto a wall (length - t_enter = -1 ulp of
           float64): above -2^-(unit_bits + 1) m, so 0 units is within half a unit of them too (the CPU test asserts
           both for every visit add of every sheet).  The integer sum therefore errs by at most n * 2^-(unit_bits + 1)
           metres and is otherwise exact.
           Each share add rounds once (u / 2) and each of the b batches that fold rounds once: float64(layer) + units *
           2^-unit_bits is exact in float64 for every sheet here (asserted: the two terms span fewer than 53 bits), so
           the fold is ONE rounding to float32.  |model - E| <= n * 2^-(unit_bits + 1) + (b + s) * u(max |p|) / 2,
           the maximum taken over the model's own intermediate values.

__float2uint_rn, the conversion the kernel uses, is defined by HIP's device header as (unsigned)rint(x): round to the
nearest integer, ties to even, then the conversion, which gfx950 does with v_cvt_u32_f32 -- the ISA defines that to
saturate, negative inputs and NaN giving 0, inputs of 2^32 and more 0xffffffff.  Within C's own rules only the
in-range part is defined, and that is all the sheets use: the negative products above round to -0.0, which converts
to 0 in C as well.  units_of() restates the instruction; the device meeting the model on the `flags` sheets, which
hold such adds, confirms the 0."""
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

F = np.float32

RF_END_POINT_AS_FREE = 1 << 0
RF_STOP_ON_FIRST_OCCUPIED = 1 << 1
RF_EXCLUDE_ORIGIN = 1 << 2
RF_EXCLUDE_SAMPLE = 1 << 3
RF_EXCLUDE_RAY = 1 << 4

INF = float("inf")
CHUNK_RAYS = 512                 # rays through one region in a batch of at most 16384 that still fit one walk chunk

MUTANTS = ("truncate", "unit_27_always", "carry_lost_on_exact_wrap", "fold_per_chunk", "fold_before_samples",
           "end_exits_at_step_time", "origin_range_not_passed", "entry_time_min_axis", "last_exit_across_calls",
           "pass_twice_on_rewalk")
WALK_MUTANTS = ("end_exits_at_step_time", "origin_range_not_passed", "entry_time_min_axis")


class MapParams:
    """Resolution, region dimensions (voxels) and origin of a map; the occupancy constants decide only which voxels
    count as occupied for kRfStopOnFirstOccupied (ohm/OccupancyMap.cpp:205-213)."""

    def __init__(self, res, dim, origin=(0.0, 0.0, 0.0)):
        self.res = float(res)
        self.dim = (dim,) * 3 if isinstance(dim, int) else tuple(int(d) for d in dim)
        self.origin = tuple(float(v) for v in origin)
        self.region_dim = tuple(d * self.res for d in self.dim)
        self.volume = self.dim[0] * self.dim[1] * self.dim[2]
        self.hit = F(math.log(0.9 / 0.1))
        self.miss = F(math.log(0.45 / 0.55))
        self.threshold = F(0.0)
        self.min_value, self.max_value = F(-2.0), F(3.511)

    def index(self, local):
        return local[0] + self.dim[0] * (local[1] + self.dim[1] * local[2])

    def local(self, vi):
        return vi % self.dim[0], (vi // self.dim[0]) % self.dim[1], vi // (self.dim[0] * self.dim[1])


def traversal_unit_bits(res):
    """traversalUnitBits (traversal_kernels.h): the largest exponent <= 28 at which a voxel diagonal, taken as
    res * 1.7320508075688772 in float64, stays below 2^31 units."""
    bits = 28
    while bits > 0 and res * 1.7320508075688772 * float(1 << bits) >= 2147483648.0:
        bits -= 1
    return bits


# ---------------------------------------------------------------------------------------------------------------------
# key maths (ohm/MapCoord.h:45-93, ohm/MapRegion.cpp:32-69, ohm/OccupancyMap.h:757-778)
# ---------------------------------------------------------------------------------------------------------------------
_EPS = float(F(1e-6))


def _region_voxel(coord, res, region_res):
    if -_EPS <= coord < 0:
        coord = 0.0
    elif coord >= region_res and coord - _EPS < region_res:
        coord -= _EPS
    return math.floor(coord / res)


def global_voxel(p, mp):
    """Global voxel coordinate (region * dim + local per axis) of a point, or None where the key is null."""
    g = []
    for a in range(3):
        coord = math.floor((p[a] - mp.origin[a]) / mp.region_dim[a] + 0.5)
        centre = coord * mp.region_dim[a]
        region_min = centre - 0.5 * mp.region_dim[a]
        q = _region_voxel(p[a] - mp.origin[a] - region_min, mp.res, mp.region_dim[a])
        if not 0 <= q < mp.dim[a]:
            return None
        g.append(coord * mp.dim[a] + q)
    return tuple(g)


def key_of(g, mp):
    region = tuple(g[a] // mp.dim[a] for a in range(3))
    return region, mp.index(tuple(g[a] - region[a] * mp.dim[a] for a in range(3)))


def voxel_centre_axis(g, a, mp):
    region, local = g // mp.dim[a], g % mp.dim[a]
    v = float(region)
    v *= mp.region_dim[a]
    v -= 0.5 * mp.region_dim[a]
    v += mp.origin[a]
    v += float(local) * mp.res
    v += 0.5 * mp.res
    return v


# ---------------------------------------------------------------------------------------------------------------------
# the walk
# ---------------------------------------------------------------------------------------------------------------------
def _div(a, b):
    """IEEE a / b (Python raises where IEEE gives an infinity or a NaN)."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return float("nan")
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def ray_length(start, end):
    """sqrt of the ray's dotted difference, as the sample's share takes it (ohm/RayMapperOccupancy.cpp:299-305)."""
    d = [end[a] - start[a] for a in range(3)]
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


Visits = namedtuple("Visits", "keys enter exit last_exit_range reported length")


def visits(start, end, flags, mp, mutant=None):
    """The voxels one ray reports, in order, as (region, voxel index), with t_enter and t_exit in float64 exactly as
    the reference computes them; the ray's last_exit_range (None where it reported no voxel), whether it reported any
    and the length its sample's share is taken from."""
    start, end = [float(v) for v in start], [float(v) for v in end]
    length_share = ray_length(start, end)
    keys, enter, exit_ = [], [], []
    gs, ge = global_voxel(start, mp), global_voxel(end, mp)
    if flags & RF_EXCLUDE_RAY or gs is None or ge is None:
        return Visits(keys, enter, exit_, None, False, length_share)
    include_end = bool(flags & RF_END_POINT_AS_FREE)
    exclude_start = bool(flags & RF_EXCLUDE_ORIGIN)
    # walkInitRay + walkCalculateSteps (ohm/LineWalkCompute.h:188-280)
    d = [end[a] - start[a] for a in range(3)]
    length = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    length = math.sqrt(length) if length > 1e-6 else 0.0
    sign = [1 if d[a] < 0 else 0 for a in range(3)]
    d = [_div(d[a], length) for a in range(3)]
    inv = [_div(1.0, d[a]) if length > 0 else 0.0 for a in range(3)]
    init, delta = [0.0] * 3, [0.0] * 3
    for a in range(3):
        centre = voxel_centre_axis(gs[a], a, mp)
        vmin, vmax = centre - 0.5 * mp.res, centre + 0.5 * mp.res
        init[a] = ((vmin if sign[a] else vmax) - start[a]) * inv[a]
        shift = (-2 * sign[a] + 1) * mp.res
        vmin += shift
        vmax += shift
        e1 = ((vmin if sign[a] else vmax) - start[a]) * inv[a]
        if e1 != INF:
            e1 -= init[a]
        delta[a] = e1
    remaining = [ge[a] - gs[a] for a in range(3)]
    stepped = [0, 0, 0]
    cur = list(gs)
    time_next = [init[a] if remaining[a] else INF for a in range(3)]

    def select():
        axis = 0
        axis = axis if time_next[axis] < time_next[1] else 1
        axis = axis if time_next[axis] < time_next[2] else 2
        return axis

    def step(axis):
        sd = -2 * sign[axis] + 1
        cur[axis] += sd
        remaining[axis] -= sd
        stepped[axis] += sd
        time_next[axis] = init[axis] + delta[axis] * abs(stepped[axis]) if remaining[axis] else INF

    def report(g, t_in, t_out):
        key = key_of(g, mp)
        if mutant == "entry_time_min_axis" and keys and keys[-1][0] != key[0]:
            # a region's first voxel enters at the EARLIEST of the axes' last steps, not the latest
            t_in = min(init[a] if abs(stepped[a]) <= 1 else init[a] + delta[a] * (abs(stepped[a]) - 1)
                       for a in range(3) if stepped[a])
        keys.append(key)
        enter.append(t_in)
        exit_.append(t_out)

    axis = select()
    last_time = 0.0
    done = lambda: all(r == 0 for r in remaining)  # noqa: E731  (limit_flags == 7)
    if exclude_start:
        if mutant != "origin_range_not_passed":
            last_time = time_next[axis]
        step(axis)
        axis = select()
    # (a step along an axis with nothing remaining happens only under kRfExcludeOrigin in the end voxel; the reference
    # then walks on while the keys differ: no sheet does that, asserted by the CPU test through the oracle)
    guard = 0
    while not done() and tuple(cur) != ge:
        report(tuple(cur), last_time, time_next[axis])
        last_time = time_next[axis]
        step(axis)
        axis = select()
        guard += 1
        assert guard < 100000
    if include_end:
        t_out = length
        if mutant == "end_exits_at_step_time":
            t_out = min(init[a] + delta[a] * abs(stepped[a]) if stepped[a] else init[a] for a in range(3))
        report(ge, last_time, t_out)
    last = exit_[-1] if keys else None
    if keys and mutant == "end_exits_at_step_time" and include_end:
        last = length                     # (the deviation is the tile's; the share's exit range is computed elsewhere)
    return Visits(keys, enter, exit_, last, bool(keys), length_share)


# ---------------------------------------------------------------------------------------------------------------------
# what the CPU mapper adds
# ---------------------------------------------------------------------------------------------------------------------
Add = namedtuple("Add", "region vi value share ray")
Call = namedtuple("Call", "rays flags")


class Occupancy:
    """Log-odds of the voxels a sheet has touched or planted: only `occupied` is used (kRfStopOnFirstOccupied).
    The rule itself is occupancy_ref's; this is that model under the map's default configuration."""

    def __init__(self, mp, planted=None):
        import occupancy_ref                        # (it imports this module for the walk)
        self.mp, self.rule = mp, occupancy_ref
        self.cfg = occupancy_ref.config(mp.hit, mp.miss, mp.threshold, mp.min_value, mp.max_value)
        self.values = dict(planted or {})          # (region, vi) -> float32

    def occupied(self, key):
        return self.rule.occupied(self.cfg, self.values.get(key, F(np.inf)))

    def miss(self, key, null_update):
        self.values[key] = self.rule.adjust_miss(self.cfg, self.values.get(key, F(np.inf)), 0, null_update)

    def hit(self, key):
        self.values[key] = self.rule.adjust_hit(self.cfg, self.values.get(key, F(np.inf)))


def cpu_adds(call, mp, occupancy=None, mutant=None, last_exit_in=0.0):
    """([Add] in the order the CPU mapper makes them, last_exit_range at the end of the call).  `occupancy` is updated
    where given and decides which rays kRfStopOnFirstOccupied stops; `last_exit_in` is 0 at the start of every call
    (the mapper's variable is local to integrateRays) -- the `last_exit_across_calls` mutant passes the previous
    call's value."""
    rays, flags = np.asarray(call.rays, dtype=np.float64), int(call.flags)
    walk_mutant = mutant if mutant in WALK_MUTANTS else None
    out = []
    last_exit = float(last_exit_in)
    include_sample_in_ray = bool(flags & RF_END_POINT_AS_FREE)
    for r in range(rays.shape[0] // 2):
        start, end = rays[2 * r], rays[2 * r + 1]
        v = visits(start, end, flags, mp, walk_mutant)
        stopped = False
        for key, t_in, t_out in zip(v.keys, v.enter, v.exit):
            out.append(Add(key[0], key[1], F(t_out - t_in), False, r))
            if occupancy is not None:
                was = occupancy.occupied(key)
                occupancy.miss(key, stopped)
                stopped = stopped or (bool(flags & RF_STOP_ON_FIRST_OCCUPIED) and was)
        if v.reported:
            last_exit = v.last_exit_range
        if not stopped and not include_sample_in_ray and not flags & RF_EXCLUDE_SAMPLE:
            g = global_voxel(end, mp)
            key = key_of(g, mp)
            out.append(Add(key[0], key[1], F(v.length - last_exit), True, r))
            if occupancy is not None:
                occupancy.hit(key)
    return out, last_exit


def exact_sum(values):
    """The exact sum of float32 (or any binary floating point) values."""
    return sum((Fraction(float(v)) for v in values), Fraction(0))


def ulp32(x):
    """Spacing of float32 at |x| (that of the smallest normal below it)."""
    x = abs(float(x))
    if x < 2.0 ** -126:
        return 2.0 ** -149
    return 2.0 ** (math.frexp(x)[1] - 24)


# ---------------------------------------------------------------------------------------------------------------------
# the device's rule
# ---------------------------------------------------------------------------------------------------------------------
def units_of(add, unit_bits, mutant=None):
    """__float2uint_rn(add * 2^unit_bits): the product is formed in float32 (exact: a power of two, far from the
    format's ends), rounded to the nearest integer, ties to even, saturated to [0, 2^32 - 1]; NaN gives 0."""
    p = F(add) * F(2.0 ** unit_bits)
    if p != p or p <= 0:
        return 0
    q = Fraction(float(p))
    n = math.floor(q) if mutant == "truncate" else round(q)     # Python rounds a Fraction half to even
    return min(n, 0xffffffff)


Words = namedtuple("Words", "word carries")


def word_view(units, mutant=None):
    """One walk chunk's 32-bit tile word of a voxel after the given visits: (final word, carries sent)."""
    word = carries = 0
    for n in units:
        total = word + n
        wrapped = total > 0xffffffff
        if mutant == "carry_lost_on_exact_wrap" and total == 1 << 32:
            wrapped = False
        carries += int(wrapped)
        word = total & 0xffffffff
    return Words(word, carries)


def chunk_of(ray_rank):
    """The walk chunk a region's segment falls into, by the rank of its ray among the call's rays through that region.
    A stand-in: the device cuts a region's segments into equal chunks in an order of its own, and the model's answer
    does not depend on the cut at all -- only the `fold_per_chunk` mutant and the word view look at it."""
    return ray_rank // CHUNK_RAYS


def device_layer(state, call, mp, occupancy=None, mutant=None, last_exit_in=0.0, rewalk=False, detail=None):
    """The layer ({region: float32[volume]}, updated in place and returned) after one device batch, and the call's
    final last_exit_range.  `detail`, a dict, receives per voxel the visit units, the word view per chunk and the
    model's largest intermediate magnitude."""
    unit_bits = traversal_unit_bits(mp.res)
    model_bits = 27 if mutant == "unit_27_always" else unit_bits
    adds, last_exit = cpu_adds(call, mp, occupancy, mutant, last_exit_in)
    shares, vis, rank, seen = {}, {}, {}, {}
    for a in adds:
        key = (a.region, a.vi)
        if a.share:
            shares.setdefault(key, []).append(a.value)
        else:
            through = seen.setdefault(a.region, {})
            through.setdefault(a.ray, len(through))
            vis.setdefault(key, []).append((units_of(a.value, model_bits, mutant), chunk_of(through[a.ray])))
    for region in {k[0] for k in list(shares) + list(vis)}:
        state.setdefault(region, np.zeros(mp.volume, dtype=F))

    def fold(key, units):
        if units == 0:
            return
        tile = state[key[0]]
        wide = float(tile[key[1]]) + float(units) * 2.0 ** -model_bits
        if detail is not None:
            detail.setdefault(key, {})["fold_exact"] = (Fraction(float(tile[key[1]])) + Fraction(units, 1 << model_bits)
                                                        == Fraction(wide)) and detail[key].get("fold_exact", True)
            peak(key, wide)
        tile[key[1]] = F(wide)

    def peak(key, value):
        if detail is not None:
            d = detail.setdefault(key, {})
            d["peak"] = max(d.get("peak", 0.0), abs(float(value)))

    def add_shares():
        for key, values in shares.items():
            tile = state[key[0]]
            peak(key, tile[key[1]])
            for v in values:
                tile[key[1]] = F(tile[key[1]] + v)
                peak(key, tile[key[1]])

    def add_visits():
        for key, entries in vis.items():
            peak(key, state[key[0]][key[1]])
            chunks = {}
            for n, c in entries:
                chunks.setdefault(c, []).append(n)
            total, words = 0, {}
            for c, units in sorted(chunks.items()):
                w = word_view(units, mutant)
                words[c] = w
                part = w.word + (w.carries << 32)
                if mutant == "pass_twice_on_rewalk" and rewalk:
                    part *= 2
                if mutant == "fold_per_chunk":
                    fold(key, part)
                total += part
            if mutant != "fold_per_chunk":
                fold(key, total)
            if detail is not None:
                detail.setdefault(key, {}).update(units=[n for n, _ in entries], words=words, n=len(entries),
                                                  s=len(shares.get(key, ())))

    if mutant == "fold_before_samples":
        add_visits()
        add_shares()
    else:
        add_shares()
        add_visits()
    if detail is not None:
        for key, values in shares.items():
            detail.setdefault(key, {}).setdefault("s", len(values))
    return state, last_exit


def replay(planted, calls, mp, occupancy=None, mutant=None, rewalk=False, details=None):
    """The states after every call: [{region: float32[volume]}].  `planted` maps regions to float32 tiles."""
    state = {r: np.array(t, dtype=F, copy=True) for r, t in planted.items()}
    states, last_exit = [], 0.0
    for call in calls:
        detail = None if details is None else {}
        carried = last_exit if mutant == "last_exit_across_calls" else 0.0
        state, last_exit = device_layer(state, call, mp, occupancy, mutant, carried, rewalk, detail)
        states.append({r: t.copy() for r, t in state.items()})
        if details is not None:
            details.append(detail)
    return states
