"""Seeded, constructed cases for the voxel mean update (test infrastructure) -- judged by tests/mean_ref.py.

A case is one voxel with a planted (coord, count), one to six rays that end in it (in ray order) and the model's state
after each.  Cases are dealt onto SHEETS: one sheet is one region of one map (16 x 16 x 16 voxels, or 48 x 48 x 48 for
the `tiled` site, which the library cuts into z slabs), with targets on a lattice three voxels apart.  A ray is 1.1 to
1.7 voxels long and points from the region's interior to its sample, so it stays inside the region and at least 0.3
voxels short of every other target; placement walks every ray with the oracle's line walk and checks that, and that
the sample's key is the target's.

Families (three axes of a voxel are independent chains, so a case carries one constructed point per axis):

  tie       per axis a planted cell k and a cell boundary B within reach for the case's count n; the end point with
            t_exact = B is solved in rationals and +-40 ulp of the END-POINT COORDINATE are scanned.  The scan keeps
            (a) the two points either side of every flip of the model, (b) every point where a mutant's cell differs
            from the model's, (c) every point where the model differs from floor(t_exact); one kept point becomes the
            axis' sample -- the one that kills the mutant the site has killed least so far, else a near-tie, else a
            flip neighbour.  Up to TRIES boundaries are solved per axis while that mutant is still short of its count.
  count     the count edges (COUNTS) on planted patterns that are never produced by integration (coord 0, the used
            bit clear, bit 30 set) and cells 0, 1, 511, 512, 1022, 1023, every count on every pattern, with samples
            at the voxel centre, exactly on the decoded mean (`on_mean`: d == 0; `near_mean` where no double of the
            voxel gives that), on the lower face, one ulp inside it and one ulp inside the upper face (faces as the key
            maths draws them).  Several of these are ties by arithmetic, e.g. n + 1 = 2046 from cell 1023 to the lower
            face, or n + 1 = 1023 from cell 0 / 1023 to the centre: t_exact is an integer and rounding decides.
  sequence  2 to 6 samples into one voxel: the first is a tie point as above (a near-tie, or next to a flip), the rest
            are drawn until the reversed order ends on another pattern.

Against the plan these cases were asked for: a scan contributes ONE kept point per axis (a voxel takes one sample per
axis chain; using every kept point would need a sheet per scan); and a sheet's batch is 150 to 210 rays, not several
hundred, because targets three voxels apart leave 125 to a 16^3 region.  Half of the tie cases on 16^3 sheets sit in
region (0, 0, 0) at origin 0, 40 of 280 at a region coordinate of +-32767.

Redraws happen while a case is being built; every case that build() returns is judged by the tests, none is dropped."""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import mean_ref
from mean_ref import POSITIONS, USED_BIT, Exact, axis_ref, cells_of
from oracle.oracle import OracleMap
from stdrandom import MinStdRand0

SEED = 20240917
SCAN = 40
TRIES = 10
TARGET = 24                      # kills per steered mutant and group of sites before the scans stop looking for more
TIE_COUNTS = (1, 2, 3, 5, 6, 7, 9, 10, 11, 13, 30, 100, 333, 700, 1000, 1500)
COUNTS = (0, 1, 2, 1022, 1023, 1024, 2045, 2046, 2047, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 31) - 2,
          (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1)
COUNT_CELLS = (0, 1, 511, 512, 1022, 1023)
COUNT_STYLES = ("zero", "clear", "bit30", "plain")
SAMPLES = ("centre", "on_mean", "lower", "lower_in", "upper_in")         # + "near_mean" where on_mean has no double
TILE_VOXELS = 1 << 15                # the library cuts larger regions into equal z slabs (ohm_amd/csrc/tiling_impl.h)
COUNT_MUTANTS = ("f32_inv", "signed_count", "wide_count", "sat_int", "used_bit")
# count -> (cell, sample) with t_exact an integer: (k - 511.5) / (n + 1) = k - B + 1 / 2 from the centre, k / (n + 1) from
# the lower face
NATURAL_TIES = {1: ((1, "lower"), (511, "lower"), (1023, "lower")), 2: ((0, "centre"), (1023, "centre")),
                1022: ((0, "centre"), (1023, "centre")), 1023: ((512, "lower"),),
                2045: ((1023, "lower"), (0, "upper_in"))}
FAR_ORIGIN = (0.35, -1.7, 12.0625)
RF_STOP_ON_FIRST_OCCUPIED = 1 << 1
SITES = ("occupancy", "stop", "ndt", "tiled")

# name -> (resolution, region voxels, origin, region key, (tie, count, sequence) cases)
CONFIGS = {
    # of the tie cases on 16^3 sheets half sit in region (0, 0, 0) at origin 0, a few at region coordinate +-32767
    "near10": (0.1, 16, (0.0, 0.0, 0.0), (0, 0, 0), (70, 30, 25)),
    "near25": (0.25, 16, (0.0, 0.0, 0.0), (0, 0, 0), (70, 30, 25)),
    "far10": (0.1, 16, FAR_ORIGIN, (-300, 411, 7), (50, 45, 25)),
    "far25": (0.25, 16, FAR_ORIGIN, (411, 7, -300), (50, 45, 25)),
    "edge10": (0.1, 16, FAR_ORIGIN, (32767, 5, -3), (20, 45, 25)),
    "edge25": (0.25, 16, FAR_ORIGIN, (-4, -32767, 9), (20, 45, 25)),
    "tiled10": (0.1, 48, FAR_ORIGIN, (-300, 411, 7), (150, 0, 0)),
    "tiled25": (0.25, 48, (0.0, 0.0, 0.0), (0, 0, 0), (150, 0, 0)),
}


def slab_layers(dim):
    """z layers per tile of a dim^3 region: the largest divisor of dim whose slab holds at most TILE_VOXELS voxels."""
    return max(t for t in range(1, dim + 1) if dim % t == 0 and dim * dim * t <= TILE_VOXELS)


def sites_of(config):
    return ("tiled",) if config.startswith("tiled") else ("occupancy", "stop", "ndt")


class Rng:
    """Integer and real draws from the reference tests' own engine (tests/stdrandom.py)."""

    def __init__(self, seed):
        self.engine = MinStdRand0(seed)

    def uniform(self, a, b):
        return self.engine.uniform(a, b)

    def below(self, n):
        return min(int(self.engine.canonical() * n), n - 1)

    def choice(self, seq):
        return seq[self.below(len(seq))]


@dataclass
class Case:
    family: str
    config: str
    local: tuple
    coord: int
    count: int
    occupancy: float
    sensors: list                     # fp64[3] per ray
    ends: list                        # fp64[3] per ray
    states: list = None               # the model's (coord, count) after each ray
    exact: list = None                # per ray, per axis: floor(t_exact) where forced, None on a near-tie or the wrap
    near_tie: bool = False            # some axis of some step has margin <= E
    near_flip: bool = False           # some axis sits within 2 ulp of a flip of the model
    wrap: bool = False                # some step divides by zero (count 0xffffffff)
    kills: frozenset = frozenset()    # the mutants whose final (coord, count) differs from the model's
    bound: float = 0.0                # the largest E of its axes and steps
    margin: float = math.inf          # the smallest margin of its forced axes and steps
    tags: tuple = ()

    @property
    def forced(self):
        return all(cell is not None for step in self.exact for cell in step)


@dataclass
class Sheet:
    config: str
    cases: list = field(default_factory=list)


class Geometry:
    def __init__(self, name):
        self.name = name
        self.res, self.dim, self.origin, self.region, self.quota = CONFIGS[name]
        self.region_dim = self.dim * self.res                 # ohm/OccupancyMap.cpp:200-202
        self.om = OracleMap(self.res, (self.dim,) * 3, ["occupancy"])
        self.om.set_origin(self.origin)
        line = range(1, self.dim, 3)
        self.targets = [(x, y, z) for z in line for y in line for x in line]
        self.target_set = set(self.targets)

    def centre(self, local):
        c = tuple(mean_ref.centre_ref(self.origin[a], self.region_dim, self.res, self.region[a], local[a])
                  for a in range(3))
        assert c == self.om.voxel_centre(self.region, local), (self.name, local)
        return c

    def closed(self, local):
        return tuple(mean_ref.centre_closed(self.origin[a], self.dim, self.res, self.region[a], local[a])
                     for a in range(3))

    def index(self, local):
        return local[0] + self.dim * (local[1] + self.dim * local[2])

    def inside(self, local, point):
        return self.om.voxel_key(point) == (tuple(self.region), tuple(local))

    def accepts(self, local, sensor, end):
        """The sample's key is the target's, and the ray walks no other target and leaves the region nowhere."""
        if not self.inside(local, end):
            return False
        keys, _, _ = self.om.walk(sensor, end, cap=64)
        return all(k[0] == tuple(self.region) and (k[1] == tuple(local) or k[1] not in self.target_set) for k in keys)

    def faces(self, local, axis):
        """(smallest, largest) double of the axis that the key maths puts in the voxel (the other axes at the centre)."""
        c = list(self.centre(local))
        out = []
        for sign in (-1.0, 1.0):
            p = list(c)
            inner, outer = c[axis], c[axis] + sign * 0.75 * self.res
            p[axis] = outer
            assert not self.inside(local, p), (self.name, local, axis)
            while True:                                # bisect down to two neighbouring doubles
                mid = inner + (outer - inner) * 0.5
                if mid == inner or mid == outer:
                    break
                p[axis] = mid
                if self.inside(local, p):
                    inner = mid
                else:
                    outer = mid
            assert math.nextafter(inner, outer) == outer
            out.append(inner)
        return tuple(out)


@functools.lru_cache(maxsize=None)
def geometry(name):
    return Geometry(name)


def step_ulps(x, j):
    for _ in range(abs(j)):
        x = math.nextafter(x, math.inf if j > 0 else -math.inf)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the scan of one axis around one solved boundary
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Point:
    end: float
    kills: frozenset
    near_tie: bool
    near_flip: bool
    off_exact: bool


def scan_axis(rng, geo, axis, local, centre, closed, cell, count):
    """Solve one reachable boundary and scan it; -> the kept points (possibly none)."""
    res = geo.res
    ex = Exact(cell, count, res)
    lo, hi = ex.t(-0.45 * res), ex.t(0.45 * res)
    first, last = math.ceil(lo), math.floor(hi)
    if first > last:
        return []
    boundary = first + rng.below(last - first + 1)
    end0 = float(Fraction(centre) + ex.solve(boundary))
    ends = [step_ulps(end0, -SCAN)]
    for _ in range(2 * SCAN):
        ends.append(math.nextafter(ends[-1], math.inf))
    ref = [axis_ref(cell, count, e - centre, res) for e in ends]
    flips = [j for j in range(1, len(ends)) if ref[j] != ref[j - 1]]
    near = set()
    for j in flips:
        near.update(range(max(j - 4, 0), min(j + 4, len(ends))))
    kept = {}
    for j, e in enumerate(ends):
        v = e - centre
        kills = set()
        if closed != centre and axis_ref(cell, count, e - closed, res) != ref[j]:
            kills.add("closed_centre")
        near_tie = off_exact = False
        if j in near:                  # the one-rounding mutants and the exact value can only disagree next to a flip
            for mutant in ("fma", "div_count", "recip_grid"):
                if axis_ref(cell, count, v, res, mutant) != ref[j]:
                    kills.add(mutant)
            _, floor_cell, margin, bound = ex.judge(v, mean_ref.E_MAX)
            near_tie = bound is not None and margin <= bound
            off_exact = floor_cell != ref[j]
        near_flip = any(j - 2 <= f <= j + 1 for f in flips)          # one of the two neighbours either side
        if kills or off_exact or near_flip:
            kept[j] = Point(e, frozenset(kills), near_tie, near_flip, off_exact)
    return list(kept.values())


def pick_point(rng, points, wanted):
    """One kept point: kills `wanted` if any does, else a near-tie, else next to a flip, else any."""
    for test in (lambda p: wanted in p.kills, lambda p: p.near_tie, lambda p: p.near_flip, lambda p: True):
        pool = [p for p in points if test(p)]
        if pool:
            return rng.choice(pool)
    return None


def tie_axis(rng, geo, axis, local, centre, closed, count, wanted, tries=TRIES):
    """(cell, Point) for one axis: up to `tries` scanned boundaries while no kept point kills `wanted`."""
    best = None
    for attempt in range(8 * tries + 400):
        if best is not None and attempt >= tries:
            break
        k = rng.below(POSITIONS + 1) if wanted != "recip_grid" else 512 + rng.below(512)
        points = scan_axis(rng, geo, axis, local, centre, closed, k, count)
        if not points:
            continue
        pick = pick_point(rng, points, wanted)
        if wanted in pick.kills:
            return k, pick
        if wanted is None and not (pick.near_tie or pick.near_flip):
            continue
        if best is None or (pick.near_tie and not best[1].near_tie):
            best = (k, pick)
    assert best is not None, (geo.name, local, axis, count)
    return best


# ---------------------------------------------------------------------------------------------------------------------
# rays and judging
# ---------------------------------------------------------------------------------------------------------------------
def sensor_for(rng, geo, local, end):
    """A sensor 1.1 ... 1.7 voxels from the sample, on the side of the region's interior."""
    for _ in range(50):
        d = [rng.uniform(0.15, 1.0) for _ in range(3)]
        norm = math.sqrt(sum(x * x for x in d))
        length = rng.uniform(1.1, 1.7) * geo.res
        sensor = tuple(end[a] + (1.0 if 2 * local[a] < geo.dim else -1.0) * d[a] / norm * length for a in range(3))
        if geo.accepts(local, sensor, end):
            return sensor
    raise AssertionError(("no ray", geo.name, local, end))


def finish(geo, case, near_flip=False):
    """Run the model and the mutants over a built case."""
    centre = geo.centre(case.local)
    res = geo.res
    case.states = mean_ref.run_ref(case.coord, case.count, case.ends, centre, res)
    case.exact, case.near_tie, case.wrap = [], False, False
    coord, count = case.coord, case.count
    for end, state in zip(case.ends, case.states):
        judged = mean_ref.update_exact(coord, count, end, centre, res)
        case.wrap |= judged[0] is None
        case.near_tie |= any(j is not None and not mean_ref.forced(j) for j in judged)
        case.exact.append(tuple(j[1] if mean_ref.forced(j) else None for j in judged))
        for j in judged:
            if j is not None:
                case.bound = max(case.bound, float(j[3]))
                if mean_ref.forced(j):
                    case.margin = min(case.margin, float(j[2]))
        coord, count = state
    case.near_flip = near_flip
    kills = set()
    final = case.states[-1]
    for mutant in mean_ref.AXIS_MUTANTS + ("used_bit",):
        if mean_ref.run_ref(case.coord, case.count, case.ends, centre, res, mutant)[-1] != final:
            kills.add(mutant)
    if mean_ref.run_ref(case.coord, case.count, case.ends, geo.closed(case.local), res)[-1] != final:
        kills.add("closed_centre")
    if len(case.ends) > 1 and mean_ref.run_ref(case.coord, case.count, case.ends[::-1], centre, res)[-1] != final:
        kills.add("order")
    case.kills = frozenset(kills)
    return case


def occupancy_value(rng):
    return float(np.float32(rng.uniform(-1.5, 3.0)))


def most_wanted(needs):
    short = [m for m in needs if needs[m] < TARGET]
    return min(short, key=needs.get) if short else None


def build_tie(rng, geo, local, needs):
    """`needs`: the steered mutants' kills so far.  recip_grid is rare (1 / mr is 4092 or 10230 to within a rounding, so
    multiplying by it and dividing by mr differ in few quotients): it is looked for with small counts, cells in the upper
    half (a quotient's ulp is largest there) and six times the boundaries."""
    centre, closed = geo.centre(local), geo.closed(local)
    count = rng.choice(TIE_COUNTS[:10] if most_wanted(needs) == "recip_grid" else TIE_COUNTS)
    cells, end, flags = [], [], []
    for a in range(3):
        wanted = most_wanted(needs)
        tries = 1 if wanted is None else (6 * TRIES if wanted == "recip_grid" else TRIES)
        k, point = tie_axis(rng, geo, a, local, centre[a], closed[a], count, wanted, tries)
        for m in point.kills & needs.keys():
            needs[m] += 1
        cells.append(k)
        end.append(point.end)
        flags.append(point.near_flip)
    end = tuple(end)
    case = Case("tie", geo.name, local, mean_ref.pack(cells), count, occupancy_value(rng),
                [sensor_for(rng, geo, local, end)], [end])
    return finish(geo, case, any(flags))


def on_mean_point(geo, local, axis, centre, mean):
    """A coordinate x of the voxel with x - centre == mean exactly (d == 0 in the update), or None: the difference of
    two doubles is a multiple of the smaller ulp of the two, so one exists only where the centre is as fine as the mean
    (voxels next to the map origin) or the mean as coarse as the centre (cell 0 at 0.25 m: -0.125)."""
    lower, upper = geo.faces(local, axis)
    guess = float(Fraction(centre) + Fraction(mean))
    for x in (guess, math.nextafter(guess, math.inf), math.nextafter(guess, -math.inf)):
        if x - centre == mean and lower <= x <= upper:
            return x
    return None


def place_sample(geo, local, axis, centre, kind, mean):
    """The coordinate of one axis for a count-family sample."""
    lower, upper = geo.faces(local, axis)
    if kind == "centre":
        return centre
    if kind == "lower":
        return lower
    if kind == "lower_in":
        return math.nextafter(lower, math.inf)
    if kind == "upper_in":
        return upper
    if kind == "on_mean":
        return on_mean_point(geo, local, axis, centre, mean)
    return min(max(float(Fraction(centre) + Fraction(mean)), lower), upper)          # near_mean: the nearest double


def build_count(rng, geo, local, serial):
    """The count and the planted style cycle so that every count meets every style (serial = i + 17 j: count i, style
    j mod 4).  An `on_mean` axis has d == 0 exactly: where no double of the voxel does that for the drawn cell the other
    cells are tried, and an axis that still has none is tagged `near_mean` (the nearest double).  A case at the wrap
    (count 0xffffffff) gets an `on_mean` axis wherever one of its axes allows it: 0 * inf = NaN is the path to hit."""
    centre = geo.centre(local)
    count = COUNTS[serial % len(COUNTS)]
    style = COUNT_STYLES[(serial // len(COUNTS)) % len(COUNT_STYLES)]
    choices = (0,) if style == "zero" else COUNT_CELLS
    cells = [rng.choice(choices) for _ in range(3)]
    kinds = [rng.choice(SAMPLES) for _ in range(3)]
    if count in NATURAL_TIES and style != "zero":            # one axis on a tie that the arithmetic itself makes
        cells[serial % 3], kinds[serial % 3] = rng.choice(NATURAL_TIES[count])

    def exact_cell(a, first):
        for k in (first,) + tuple(c for c in choices if c != first):
            if on_mean_point(geo, local, a, centre[a], mean_ref.decode(k, geo.res)) is not None:
                return k
        return None
    for a in range(3):
        if kinds[a] == "on_mean":
            k = exact_cell(a, cells[a])
            cells[a], kinds[a] = (k, "on_mean") if k is not None else (cells[a], "near_mean")
    if count == 0xffffffff and "on_mean" not in kinds:
        for a in range(3):
            k = exact_cell(a, cells[a])
            if k is not None:
                cells[a], kinds[a] = k, "on_mean"
                break
    if style == "clear" and not any(cells):                  # a NONZERO pattern with bit 31 clear
        free = [a for a in range(3) if kinds[a] != "on_mean"]
        assert free, (geo.name, local)
        cells[free[0]] = 1023
    kinds = tuple(kinds)
    coord = mean_ref.pack(cells)
    if style in ("zero", "clear"):
        coord &= ~USED_BIT
    if style == "bit30":
        coord |= 1 << 30
    end = tuple(place_sample(geo, local, a, centre[a], kinds[a], mean_ref.decode(cells[a], geo.res)) for a in range(3))
    case = Case("count", geo.name, local, coord, count, occupancy_value(rng), [sensor_for(rng, geo, local, end)],
                [end], tags=(style,) + kinds)
    return finish(geo, case)


def build_sequence(rng, geo, local):
    centre, closed = geo.centre(local), geo.closed(local)
    res = geo.res
    count = rng.choice(TIE_COUNTS[:10])
    cells, first, flags = [], [], []
    for a in range(3):
        k, point = tie_axis(rng, geo, a, local, centre[a], closed[a], count, None, tries=1)
        cells.append(k)
        first.append(point.end)
        flags.append(point.near_flip or point.near_tie)
    assert all(flags), (geo.name, local)
    coord = mean_ref.pack(cells)
    length = 2 + rng.below(5)
    for _ in range(200):
        ends = [tuple(first)] + [tuple(centre[a] + rng.uniform(-0.45, 0.45) * res for a in range(3))
                                 for _ in range(length - 1)]
        forward = mean_ref.run_ref(coord, count, ends, centre, res)[-1]
        if mean_ref.run_ref(coord, count, ends[::-1], centre, res)[-1] != forward:
            break
    else:
        raise AssertionError(("order never mattered", geo.name, local))
    case = Case("sequence", geo.name, local, coord, count, occupancy_value(rng),
                [sensor_for(rng, geo, local, e) for e in ends], ends)
    return finish(geo, case, True)


@functools.lru_cache(maxsize=None)
def build(seed=SEED):
    """-> [Sheet]: one per configuration."""
    rng = Rng(seed)
    sheets = []
    serial = 0
    needs = {}                                      # per group of sites: axis kills so far, to steer the tie scans
    for name in CONFIGS:
        geo = geometry(name)
        tally = needs.setdefault(sites_of(name), {})
        # closed_centre equals the reference's centre at 0.25 (every term is exact there); recip_grid was never seen at 0.1
        # fma and div_count need end points fine enough for the chain's own roundings to decide: the sheets at the origin
        fine = geo.origin == (0.0, 0.0, 0.0)
        wanted = (["fma", "div_count"] if fine else []) + ((["recip_grid"] if fine else []) if geo.res == 0.25 else
                                                           ["closed_centre"])
        for m in wanted:
            tally.setdefault(m, 0)
        steer = {m: tally[m] for m in wanted}
        n_tie, n_count, n_seq = geo.quota
        total = n_tie + n_count + n_seq
        assert total <= len(geo.targets)
        stride = len(geo.targets) // total           # spread over the region (and so over the tiles of a cut one)
        slots = [geo.targets[i * stride] for i in range(total)]
        sheet = Sheet(name)
        made = dict(tie=0, count=0, sequence=0)
        quota = dict(tie=n_tie, count=n_count, sequence=n_seq)
        for local in slots:                          # the families interleaved, each in proportion to its share
            family = min((f for f in quota if made[f] < quota[f]), key=lambda f: (made[f] + 0.5) / quota[f])
            made[family] += 1
            if family == "tie":
                case = build_tie(rng, geo, local, steer)
            elif family == "count":
                case = build_count(rng, geo, local, serial)
                serial += 1
            else:
                case = build_sequence(rng, geo, local)
            sheet.cases.append(case)
        for m in wanted:
            tally[m] = steer[m]
        sheets.append(sheet)
    return sheets


# ---------------------------------------------------------------------------------------------------------------------
# planting and feeding: shared by the CPU test (oracle) and the GPU test (device)
# ---------------------------------------------------------------------------------------------------------------------
LAYER_SHAPES = {"occupancy": (np.float32, 1), "mean": (np.uint32, 2), "covariance": (np.float32, 6)}
NDT = dict(sensor_noise=0.05, sample_threshold=3, adaptation_rate=0.7, reinit_threshold=-1.0e30, reinit_count=100)


def layers_of(site):
    return ["occupancy", "mean"] + (["covariance"] if site == "ndt" else [])


def flags_of(site):
    return RF_STOP_ON_FIRST_OCCUPIED if site == "stop" else 0


def planted_tiles(sheet, site):
    """The sheet's region with every case's state in its voxel, the rest never observed.  Every target is planted above
    the occupancy threshold or below it as drawn; the voxels the rays walk are unobserved, so under
    kRfStopOnFirstOccupied no ray meets an occupied voxel before its sample (the tests assert the count increments)."""
    geo = geometry(sheet.config)
    volume = geo.dim ** 3
    tiles = {n: np.zeros(volume * LAYER_SHAPES[n][1], dtype=LAYER_SHAPES[n][0]) for n in layers_of(site)}
    tiles["occupancy"][:] = np.inf
    for case in sheet.cases:
        vi = geo.index(case.local)
        tiles["occupancy"][vi] = case.occupancy
        tiles["mean"][2 * vi:2 * vi + 2] = (case.coord, case.count)
        if site == "ndt":
            s = np.float32(geo.res)
            tiles["covariance"][6 * vi:6 * vi + 6] = np.array([0.11, 0.01, 0.09, -0.02, 0.015, 0.13], np.float32) * s
    return tiles


def make_oracle(sheet, site):
    geo = geometry(sheet.config)
    om = OracleMap(geo.res, (geo.dim,) * 3, layers_of(site))
    om.set_origin(geo.origin)
    om.set_ray_filter("good", 1e10)
    if site == "ndt":
        om.set_ndt(ndt_tm=False, **NDT)
    return om


def plant(om, sheet, site):
    """Create the sheet's region and overwrite every layer of it with the planted tiles."""
    geo = geometry(sheet.config)
    c = np.array(geo.centre((0, 0, 0)))
    if site == "ndt":
        om.integrate_ndt(np.array([c, c]))
    else:
        om.integrate_occupancy(np.array([c, c]))
    tiles = planted_tiles(sheet, site)
    for name, tile in tiles.items():
        om.region_layer_view(geo.region, name)[:] = tile
    return tiles


def oracle_integrate(om, site, rays):
    if site == "ndt":
        om.integrate_ndt(rays)
    else:
        om.integrate_occupancy(rays, flags=flags_of(site))


def calls(sheet, segment_of=None):
    """Every ray of the sheet, each voxel's in order, as a list of calls (2n x 3 arrays): one call, or one per value of
    segment_of(case, k)."""
    out = {}
    depth = max(len(c.ends) for c in sheet.cases)
    for k in range(depth):
        for c in sheet.cases:
            if len(c.ends) > k:
                out.setdefault(segment_of(c, k) if segment_of else 0, []).append((c.sensors[k], c.ends[k]))
    arrays = []
    for seg in sorted(out):
        rays = np.empty((2 * len(out[seg]), 3), dtype=np.float64)
        rays[0::2] = [r[0] for r in out[seg]]
        rays[1::2] = [r[1] for r in out[seg]]
        arrays.append(rays)
    return arrays


def step_cases(sheet, k):
    return [c for c in sheet.cases if len(c.ends) > k]


def read_voxel(tiles, geo, case):
    vi = geo.index(case.local)
    return int(tiles["mean"][2 * vi]), int(tiles["mean"][2 * vi + 1])


def check_case(case, k, got, who):
    """One voxel after its k-th ray against the model and, where forced, the exact value."""
    want = case.states[k]
    assert got == want, (who, "differs from the model", case.family, case.config, case.local, k,
                         "%08x %d" % got, "%08x %d" % want, case.tags)
    if case.wrap and case.count == 0xffffffff and k == 0:
        assert got == (USED_BIT, 0), (who, "wrap", case.local, got)        # x86: inf / NaN -> INT_MIN -> cell 0
    for a, cell in enumerate(case.exact[k]):
        if cell is not None:
            assert cells_of(got[0])[a] == cell, (who, "differs from floor(t_exact)", case.family, case.local, k, a)


def site_table(sheets):
    """site -> dict(cases, near_ties, near_flip, forced, wraps, kills{mutant: cases})."""
    table = {}
    for sheet in sheets:
        for site in sites_of(sheet.config):
            row = table.setdefault(site, dict(cases=0, near_ties=0, near_flip=0, forced=0, wraps=0, kills={}))
            for c in sheet.cases:
                row["cases"] += 1
                row["near_ties"] += int(c.near_tie)
                row["near_flip"] += int(c.near_flip)
                row["forced"] += int(c.forced)
                row["wraps"] += int(c.wrap)
                for m in c.kills:
                    row["kills"][m] = row["kills"].get(m, 0) + 1
    return table


def show_site_table(sheets, only=None):
    print("\n%-10s %6s %9s %7s %6s  mutants this site's cases catch" % ("site", "cases", "near-ties", "forced", "wraps"))
    for site, row in site_table(sheets).items():
        if only is not None and site != only:
            continue
        caught = " ".join("%s=%d" % (m, row["kills"].get(m, 0)) for m in mean_ref.MUTANTS)
        print("%-10s %6d %9d %7d %6d  %s" % (site, row["cases"], row["near_ties"], row["forced"], row["wraps"], caught))
