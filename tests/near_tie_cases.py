"""Rays with ONE comparison of a chosen size, for the integration walk's two shortcuts (test infrastructure).

The integration walk trusts two estimates instead of evaluating the reference's fp64 comparison every time:
  * the fixed-point predictor of k_region_walk takes its own axis when the smallest candidate leads the second smallest
    by more than MARGIN units, and decides exactly (exactNextAxis) otherwise;
  * stepsBefore() (walk_device.h) returns floor(x) + 1 for the number of steps axis b has taken when axis a enters a
    tile, x = (ta - init_b) / delta_b, without the exact predicate when x keeps 1e-5 from every integer.
The rays of the random tests almost never put a comparison next to either threshold.  These rays do, by construction:
a straight line through a lattice point on a voxel edge (both axes of a pair cross a wall there: an exact tie) whose
end point is then moved by m lattice units along one of the two axes.  The two exit times then differ by
u* m / (d + m) of ray parameter (u* the parameter of the edge point, d the moved component), so m is SOLVED for the
wanted gap, not searched.  Everything that decides the right voxel sequence is Python integers and Fractions in
tests/exact_walk.py; no float takes part.

Units.  The lattice is resolution / 2^30 with resolution = 0.125 m: one unit is 2^-33 m, every coordinate is below 2^40
units and exact in fp64, and so is the lattice-aligned origin (0.0625 m = 2^29 units).  A predictor unit is
1.01 * (tile diagonal) / 2^30 metres of ray parameter and MARGIN = 2 * max(tile dim) + 8 (ohmhip_map.hip:136-141,
restated in predictor_unit() / margin()); a region of more than 2^15 voxels is cut into tiles by chooseTileDims
(tiling_impl.h:16-45, restated in tile_dims()): 64^3 becomes 64 x 64 x 8 slabs, so that configuration's margin is 136.
Times are metres of ray parameter, t = L u: L = |end - start| and the tile diagonal are square roots, taken here as
floor(sqrt(n) 2^40) / 2^40 -- a rational within 2^-40 relative of the irrational value, nine orders below any gap used.

Isolation.  A ray is kept only if every OTHER comparison along it (consecutive exit times, which bound all pairs) is a
structural tie or separated by at least 8 MARGIN units and by 8e-5 step deltas of both axes involved: exactly one
comparison per ray sits inside a decision band.  Rays that miss this, miss their position class or gap cell, exceed 6
regions, or leave the exact walker's contract (relative gap 1e-9) are discarded and counted by reason.

init / delta.  stepsBefore() also asks for |init| <= 4 delta before it trusts its estimate.  init is the time to the first
wall and delta the time between walls of the same axis, so 0 < init <= delta for every start inside its voxel: that
condition cannot fail for a finite ray, and no start point lies on its far side.  Covered instead: starts next to the
wall the ray leaves through (init ~ 0) and next to the opposite wall (init ~ delta)."""
import functools
import random
from fractions import Fraction
from math import isqrt

from exact_walk import Undecidable, smallest_gap, walk

SUB = 1 << 30                       # lattice units per voxel
RES = 0.125                         # metres per voxel (dyadic)
UNIT_M = Fraction(1, 8 * SUB)       # metres per lattice unit
G = 1 << 18                         # constructed offsets are multiples of this, so that P + (A, B) j / 256 is on the lattice
HIT_VOXEL_BITS = 15                 # kHitVoxelBits: a tile holds at most 2^15 voxels
MAX_REGIONS = 6
ISOLATION = 8                       # other gaps: >= 8 margins and >= 8e-5 step deltas
BAND_STEPS = Fraction(1, 100000)    # the 1e-5 of stepsBefore()

GAPS_A = [Fraction(s) for s in ("0.02", "0.25", "0.5", "0.9", "0.98", "1.02", "1.1", "1.5", "2", "4")]   # margins
GAPS_B = [Fraction(s) for s in ("2e-8", "1e-6", "0.5e-5", "0.9e-5", "1.1e-5", "2e-5", "1e-4")]          # step deltas of b
POSITIONS_A = ("early", "late", "first", "third+")
ENTRIES_B = ("1", "2", "5+")


def tile_dims(region):
    """chooseTileDims (tiling_impl.h:16-45) for regions whose x-y layer fits a tile: whole z slabs."""
    x, y, z = region
    limit = 1 << HIT_VOXEL_BITS
    if x * y * z <= limit:
        return (x, y, z)
    assert x * y <= limit
    return (x, y, max(d for d in range(1, z + 1) if z % d == 0 and x * y * d <= limit))


def rsqrt(n):
    """sqrt of a non-negative integer as a rational, within 2^-40 of it."""
    return Fraction(isqrt(n << 80), 1 << 40)


def margin(tile):
    return 2 * max(tile) + 8            # ohmhip_map.hip:141


def predictor_unit(tile):
    """Metres of ray parameter per predictor unit: 1.01 * tile diagonal / 2^30 (ohmhip_map.hip:138-140)."""
    return Fraction(101, 100) * Fraction(1, 8) * rsqrt(sum(t * t for t in tile)) / (1 << 30)


CONFIGS = {
    "r32": dict(region=(32, 32, 32), origin=(0, 0, 0)),
    "r32_origin": dict(region=(32, 32, 32), origin=(SUB // 2, SUB // 2, SUB // 2)),   # (0.0625, 0.0625, 0.0625) m
    "r24x40x20": dict(region=(24, 40, 20), origin=(0, 0, 0)),
    "r64": dict(region=(64, 64, 64), origin=(0, 0, 0)),
}
for _c in CONFIGS.values():
    _c["tile"] = tile_dims(_c["region"])
PAIRS = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]
SIGNS = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]


def to_metres(units):
    return tuple(float(c) * 2.0 ** -33 for c in units)


def _mult(rng, lo, hi):
    """A multiple of G in [lo, hi], never 0."""
    lo, hi = max(1, -(-int(lo) // G)), max(1, int(hi) // G)
    return G * rng.randint(min(lo, hi), hi)


def _third_axis(rng, cfg, c, mode, seg_entry_u, u_star, d_ab):
    """Canonical start coordinate (voxels from the tile's lower wall are chosen so that c crosses no tile wall) and
    component of the third axis.  u values are Fractions."""
    tc, rc = cfg["tile"][c], cfg["region"][c]
    lower = (rng.choice((-1, 0)) * tc - rc // 2) * SUB
    if mode == "idle":
        return lower + rng.randrange(tc) * SUB + rng.randrange(1, SUB), 0
    if mode == "exhausted":
        u_c = seg_entry_u + (u_star - seg_entry_u) * Fraction(rng.randint(15, 85), 100)
        dc = rng.randint(3 * SUB // 10, SUB - 1)
        xc = max(1, int(u_c * dc))
        return lower + rng.randrange(0, tc - 1) * SUB + (SUB - xc), dc
    travel = min(rng.randint(2, 10) * min(d_ab) // 10, (tc - 3) * SUB)      # active, no tile wall crossed
    travel = max(travel, SUB // 3) + rng.randrange(1, 1 << 20)
    first = rng.randint(0, max(0, tc - 2 - travel // SUB - 1))
    return lower + first * SUB + rng.randrange(1, SUB), travel


def _build_a(rng, cfg, a, b, position, tie):
    """Family A geometry in canonical coordinates (from the map origin, every component positive): the edge point P, the
    vector (A, B) from the start to P, and the parameter at which the critical tile is entered, as a fraction of (A, B).
    position = (early | late, first | third+)."""
    tile, region = cfg["tile"], cfg["region"]
    ta, tb = tile[a], tile[b]
    when, segment = position
    if when == "late":
        ie_a, ie_b = rng.randint(0, 1), rng.randint(0, 1)
        ic_a, ic_b = rng.randint(ta - 2 + ie_a, ta - 1), rng.randint(tb - 2 + ie_b, tb - 1)
        off_a = _mult(rng, G, SUB - G)
        off_b = off_a if tie else _mult(rng, G, SUB - G)
        if tie:
            if ta != tb:
                return None
            ie_b, ic_b = ie_a, ic_a
        A0, B0 = (ic_a + 1 - ie_a) * SUB - off_a, (ic_b + 1 - ie_b) * SUB - off_b
        if segment == "first":
            A, B, entered = A0, B0, Fraction(0)
        else:
            # start a few voxels back, in the diagonal neighbour: (A, B) = (A0, B0) (1 + k / 256)
            back = (max(ie_a, ie_b) + 2) * SUB
            k = -(-256 * back // min(A0, B0)) + rng.randint(0, 8)
            A, B = A0 + A0 * k // 256, B0 + B0 * k // 256
            entered = max(Fraction(A - (ic_a + 1) * SUB, A), Fraction(B - (ic_b + 1) * SUB, B))
    elif segment == "first":
        ic_a, ic_b = rng.randrange(ta), rng.randrange(tb)
        A = SUB - _mult(rng, G, SUB - G)
        B = A if tie else SUB - _mult(rng, G, SUB - G)
        entered = Fraction(0)
    else:
        # through the corner region of three tiles: the b wall of the tile, then its a wall, then the edge point at the
        # next a wall -- the first decision of the ray's third segment
        ic_a, ic_b = 0, (0 if tie else rng.randint(0, 1))
        for _ in range(50):
            alpha = _mult(rng, 12 * SUB // 10, 35 * SUB // 10)
            beta = alpha if tie else _mult(rng, SUB // 20, 9 * SUB // 10)
            A, B = SUB + alpha, (ic_b + 1) * SUB + beta
            if tie or (Fraction(beta, B) < Fraction(9, 10) * Fraction(alpha, A) and 20 * B <= 19 * A):
                break
        else:
            return None
        entered = Fraction(alpha, A)
    n_a, n_b = rng.choice((-1, 0)), rng.choice((-1, 0))
    P = {a: (n_a * ta - region[a] // 2 + ic_a + 1) * SUB, b: (n_b * tb - region[b] // 2 + ic_b + 1) * SUB}
    return P, A, B, entered


def _build_b(rng, cfg, a, b, entry, xclass, first_axis, wall, gap, tie):
    """Family B geometry: axis a leaves a tile at P, axis b takes its kb-th step there."""
    tile, region = cfg["tile"], cfg["region"]
    ta, tb = tile[a], tile[b]
    kb_max = max(1, int(gap / Fraction(13, 10 ** 10))) if gap else 1 << 20   # relative gap gap / kb stays above 1.3e-9
    if xclass == "neg":
        kb = 1
    elif xclass == "unit":
        kb = 2 if first_axis == "a" else 1
    elif xclass == "large":
        kb = rng.randint(64, 70)
    else:
        kb = rng.randint(3, 12)
    if kb > kb_max:
        return None
    want = {"1": 1, "2": 2, "5+": 5}[entry]
    for _ in range(50):
        i0 = rng.randrange(tb)
        if (i0 + kb) % tb == 0:
            continue
        b_cross = (i0 + kb - 1) // tb
        a_cross = want - b_cross
        if a_cross >= 1:
            break
    else:
        return None
    ia0 = rng.randrange(ta)
    ka = (ta - ia0) + (a_cross - 1) * ta
    if tie:
        kb = ka
    x_a = _mult(rng, G, SUB - G)
    x_b = {"exit": G * rng.randint(1, 4), "opposite": SUB - G * rng.randint(1, 4)}.get(wall) or _mult(rng, G, SUB - G)
    if tie:
        x_b = x_a
    A, B = (ka - 1) * SUB + x_a, (kb - 1) * SUB + x_b
    n_a, n_b = rng.choice((0, 1)), rng.choice((-1, 0))
    P = {a: (n_a * ta - region[a] // 2 + ta) * SUB, b: (n_b * tb - region[b] // 2 + i0 + kb) * SUB}
    entered = max(Fraction(0), Fraction(A - ta * SUB, A))
    return P, A, B, entered


def _classify(trace, index, cfg, a, b, c, total_c):
    """Where the comparison trace[index] falls: segment number (1-based), steps taken inside the tile before it per
    axis, and what the third axis is doing."""
    tile, region = cfg["tile"], cfg["region"]

    def tile_of(voxel):
        return tuple((v + r // 2) // t for v, r, t in zip(voxel, region, tile))

    segment, entry_steps, current = 1, trace[0][5], tile_of(trace[0][4])
    for rec in trace[1:index + 1]:
        t = tile_of(rec[4])
        if t != current:
            segment, entry_steps, current = segment + 1, rec[5], t
    stepped = trace[index][5]
    inside = tuple(s - e for s, e in zip(stepped, entry_steps))
    if total_c == 0:
        third = "idle"
    elif stepped[c] < total_c:
        third = "active"
    else:
        third = "exhausted_in_segment" if entry_steps[c] < total_c else "exhausted_before"
    return segment, inside, third


def make_case(rng, cfg_name, family, cell, a, b, signs, third_mode, tie=False):
    """One constructed ray, or the reason it was discarded (a string)."""
    cfg = CONFIGS[cfg_name]
    tile, region, origin = cfg["tile"], cfg["region"], cfg["origin"]
    c = 3 - a - b
    kind = cell["kind"]
    if kind == "A":
        built = _build_a(rng, cfg, a, b, cell["position"], tie)
    else:
        built = _build_b(rng, cfg, a, b, cell["entry"], cell["xclass"], cell["first"], cell["wall"], cell["gap"], tie)
    if built is None:
        return "not constructible"
    P, A, B, entered = built
    # the tail beyond P: 1.2 to 2.5 voxels of the faster axis, as j / 256 of (A, B)
    j = max(1, -(-256 * rng.randint(12, 25) * SUB // (10 * max(A, B))))
    d = {a: A + A * j // 256, b: B + B * j // 256}
    u_star = Fraction(256, 256 + j)
    start = {a: P[a] - A, b: P[b] - B}
    start[c], d[c] = _third_axis(rng, cfg, c, third_mode, entered * u_star, u_star, (d[a], d[b]))
    unit_p, mrg = predictor_unit(tile), margin(tile)
    if not tie:
        length = UNIT_M * rsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        if kind == "A":
            gap_u = cell["gap"] * mrg * unit_p / length
        else:
            gap_u = cell["gap"] * Fraction(SUB, d[b])
        moved = a if d[a] >= d[b] else b
        m = max(1, round(gap_u * d[moved] / u_star))
        # a longer component brings that axis' steps forward
        d[moved] += m if (moved == a) == (cell["first"] == "a") else -m
    s_canon = [start[0], start[1], start[2]]
    e_canon = [start[k] + d[k] for k in range(3)]
    s_units = tuple(origin[k] + signs[k] * s_canon[k] for k in range(3))
    e_units = tuple(origin[k] + signs[k] * e_canon[k] for k in range(3))
    trace = []
    try:
        keys = walk(s_units, e_units, sub=SUB, region=region, origin_units=origin, trace=trace)
    except Undecidable:
        return "outside the exact walker's contract"
    if len({k[0] for k in keys}) > MAX_REGIONS:
        return "more than 6 regions"
    # the critical comparison: axes a and b, after ka - 1 and kb - 1 steps
    ka = P[a] // SUB - s_canon[a] // SUB
    kb = P[b] // SUB - s_canon[b] // SUB
    index = next((i for i, r in enumerate(trace) if {r[0], r[1]} == {a, b} and r[5][a] == ka - 1 and r[5][b] == kb - 1),
                 None)
    if index is None:
        return "critical comparison not adjacent"
    first, other, num, den, _, _ = trace[index]
    d_abs = [abs(e_units[k] - s_units[k]) for k in range(3)]
    length = UNIT_M * rsqrt(sum(v * v for v in d_abs))
    gap_m = Fraction(num, den) * length
    gap_units = gap_m / unit_p
    delta_b_m = Fraction(SUB, d_abs[b]) * length
    if tie:
        if num != 0:
            return "no tie"
    else:
        if (first == a) != (cell["first"] == "a"):
            return "wrong order"
        if kind == "A" and abs(gap_units / mrg - cell["gap"]) > Fraction(1, 100):
            return "gap off its cell"
        if kind == "B" and abs(gap_m / (cell["gap"] * delta_b_m) - 1) > Fraction(1, 20):
            return "gap off its cell"
    # isolation of every other comparison
    thr_margin = ISOLATION * mrg * unit_p / length                 # in u
    for i, (x, y, n2, d2, _, _) in enumerate(trace):
        if i == index or n2 == 0:
            continue
        thr = max(thr_margin, ISOLATION * BAND_STEPS * Fraction(SUB, min(d_abs[x], d_abs[y])))
        if n2 * thr.denominator < thr.numerator * d2:
            return "another comparison inside a band"
    total_c = abs((e_units[c] - origin[c]) // SUB - (s_units[c] - origin[c]) // SUB)
    segment, inside, third = _classify(trace, index, cfg, a, b, c, total_c)
    positions = set()
    if inside[0] + inside[1] + inside[2] <= 1:
        positions.add("early")
    if inside[a] >= tile[a] - 2 and inside[b] >= tile[b] - 2:
        positions.add("late")
    if segment == 1:
        positions.add("first")
    if segment >= 3:
        positions.add("third+")
    if kind == "A" and not set(cell["position"]) <= positions:
        return "position missed"
    entry = None
    if kind == "B":
        # the a step of the critical comparison leaves segment `segment`: it is the ray's segment-th tile entry
        entry = "1" if segment == 1 else ("2" if segment == 2 else ("5+" if segment >= 5 else None))
        if not tie and entry != cell["entry"]:
            return "entry missed"
        local_a = (trace[index][4][a] + region[a] // 2) % tile[a]
        if local_a != (tile[a] - 1 if signs[a] > 0 else 0):
            return "not a tile entry"
    other_gap = smallest_gap(trace, skip=index)
    return dict(
        family=family, config=cfg_name, kind=kind, start_units=s_units, end_units=e_units,
        start=to_metres(s_units), end=to_metres(e_units), keys=keys,
        gap_cell=None if tie else cell["gap"], first_cell=None if tie else cell["first"],
        axes=(a, b), first_axis=first, other_axis=other, step_index=(ka, kb), segment=segment, steps_in_tile=inside,
        positions=positions, entry=entry, xclass=cell.get("xclass"), wall=cell.get("wall"), third=third, signs=signs,
        gap_u=Fraction(num, den), gap_m=gap_m, gap_units=gap_units, gap_margins=gap_units / mrg,
        gap_steps_b=gap_m / delta_b_m, decision=index,
        other_gap_m=None if other_gap is None else Fraction(other_gap[0], other_gap[1]) * length,
        tie=tie)


def _cells(family):
    if family == "A":
        return [dict(kind="A", gap=g, first=f, position=(w, s)) for g in GAPS_A for f in ("a", "b")
                for w in ("early", "late") for s in ("first", "third+")]
    if family == "B":
        cells = []
        for g in GAPS_B:
            for f in ("a", "b"):
                for e in ENTRIES_B:
                    cells.append(dict(kind="B", gap=g, first=f, entry=e))
        return cells
    cells = [dict(kind="A", gap=None, first=None, position=(w, s)) for w in ("early", "late") for s in ("first", "third+")]
    cells += [dict(kind="B", gap=None, first=None, entry=e) for e in ENTRIES_B]
    return cells


PER_CELL = {"A": 10, "B": 19, "C": 110}
_THIRD = ("idle", "active", "exhausted")
_WALLS = ("exit", "opposite", "generic")


@functools.lru_cache(maxsize=None)
def generate(family, cfg_name, seed=20261017):
    """Deterministic list of kept cases of one family in one configuration, and {reason: count} of the discarded.
    Computed once per process and shared: callers leave the cases unchanged."""
    index = "ABC".index(family) * 16 + list(CONFIGS).index(cfg_name)
    rng = random.Random(seed * 64 + index)
    kept, discarded, n = [], {}, 0
    for cell in _cells(family):
        for k in range(PER_CELL[family]):
            n += 1
            a, b = PAIRS[n % 6]
            signs = SIGNS[(n // 6 + k) % 8]
            third = _THIRD[(n // 2 + k) % 3]
            full = dict(cell)
            if cell["kind"] == "B":
                classes = ("neg", "unit", "mid", "large") if cell["first"] != "b" else ("unit", "mid", "large")
                full["xclass"] = classes[k % len(classes)]
                if full["xclass"] == "large" and cell["entry"] != "5+":
                    full["xclass"] = "mid"
                full["wall"] = _WALLS[(n // 3) % 3]
                full.setdefault("gap", None)
            case = make_case(rng, cfg_name, family, full, a, b, signs, third, tie=(family == "C"))
            if isinstance(case, str):
                discarded[case] = discarded.get(case, 0) + 1
            else:
                kept.append(case)
    return kept, discarded


def rays_of(cases):
    """(2 n, 3) float64 origin / end pairs, the layout integrateRays takes."""
    import numpy as np
    return np.array([p for case in cases for p in (case["start"], case["end"])], dtype=np.float64)
