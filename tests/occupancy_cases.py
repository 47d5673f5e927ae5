"""Constructed sheets for the occupancy log-odds update (test infrastructure): tests/test_occupancy_ref.py (CPU) holds
the conditions they meet, tests/test_gpu_occupancy_states.py (-m gpu) holds the device to them.

A sheet is a map geometry, the layer set and chunk size its map is created with, planted occupancy tiles, a list of
calls (rays, ray flags, configuration) and the model's state of every region after every call (occupancy_ref.replay).

Geometry is kept out of the way.  Every ray is axis aligned, through voxel centres, two voxels long: it gives its start
voxel one miss and its end voxel one sample.  A CELL is three voxels in a row of x, all planted with the same state; the
middle one is the target.  A "miss ray" runs from the target to its right neighbour, a "hit ray" from the left neighbour
to the target, so the order of the cell's rays in the call IS the target's event pattern ("mmhm": two misses, a sample,
a miss), the left voxel receives misses only and the right one samples only -- a voxel with samples, one with plain
counts and one with both in the same 4-voxel group and mask word.  A ray lies in one region: a region's segments in a
call are its rays, which is what the sites' path conditions count.

Families:
  states   every edge state of the configuration x every pattern, no value-exclusion flag, the same rays in two calls
  flags    every pattern x every subset of kRfExcludeUnobserved / Free / Occupied (a call and regions of its own per
           subset) on a few states
  changing the states rays in four calls under four configurations
  count    N and N + 1 rays of one call through one voxel, N the pinned chunk size, under the tiny-miss configuration
  dense    more samples in one region than the walk stages in LDS
  stop     kRfStopOnFirstOccupied: see stop_sheet()"""
from collections import namedtuple

import numpy as np

import occupancy_ref as O
import traversal_ref as T
from occupancy_ref import Call, F, INF, config
from traversal_cases import point, rays_array
from traversal_ref import RF_END_POINT_AS_FREE, RF_EXCLUDE_ORIGIN, RF_STOP_ON_FIRST_OCCUPIED, MapParams

N = 256                          # the chunk size the sites pin (OHMHIP_CHUNK_SEGMENTS = OHMHIP_MIN_CHUNK_SEGMENTS = N)
MAX_CHUNK = 8192                 # the library's largest chunk (kMaxChunkSegments)
LDS_HITS = 6144                  # samples of a region the full walk shape stages in LDS (OHMHIP_LDS_HITS; 16^3: half)
HALF_VOXELS = 4096               # regions up to this volume are walked by the half-size shape (ohmhip_map.hip)
TILE_VOXELS = 1 << 15            # larger regions are cut into z slabs (tiling_impl.h)
PATTERNS = ("", "m", "mm", "mmm", "m" * 12, "h", "hh", "mhh", "hmmh", "hhmmm", "mmhmhmmm", "mhmhm")
NAN = np.array([0x7fc01234], dtype=np.uint32).view(F)[0]       # a quiet NaN with a payload


def _p(p):
    """ohm/MapProbability.h: log(p / (1 - p)) in float32, through the oracle's own entry point."""
    from oracle.oracle import lib
    return F(lib.oracle_probability_to_value(float(p)))


def configs():
    if not _CONFIGS:
        hit, miss = _p(0.9), _p(0.45)
        _CONFIGS.update({
            "default": config(hit, miss, _p(0.5), -2.0, 3.511),
            "clamp0": config(hit, miss, _p(0.5), 0.0, 3.511, True, True),
            "miss_half": config(hit, _p(0.5), _p(0.5), -2.0, 3.511),
            "pos_threshold": config(hit, miss, _p(0.6), -2.0, 3.511),
            "tiny": config(hit, -1e-7, _p(0.5), -1e30, 1e30),
        })
        for sat_min in (False, True):
            for sat_max in (False, True):
                _CONFIGS["tight_%d%d" % (sat_min, sat_max)] = config(_p(0.8), _p(0.35), _p(0.5), -1.1, 2.3, sat_min,
                                                                      sat_max)
    return _CONFIGS


_CONFIGS = {}
FLAG_CONFIGS = ("default", "clamp0", "miss_half", "pos_threshold", "tight_11")
FLAG_STATES = ("inf", "-0", "+0", "thr", "thr-", "min", "max", "mid+", "mid-", "nan")


def landing(cfg, k):
    """A value from which k plain misses land exactly on min (None where float32 has none nearby)."""
    x = cfg.min_value
    for _ in range(k):
        x = F(x - cfg.miss)
    for step in range(8):
        for cand in (x,) if step == 0 else (_next(x, step), _next(x, -step)):
            y = cand
            for _ in range(k):
                y = F(y + cfg.miss)
            if y == cfg.min_value and (cfg.miss == 0 or cand != cfg.min_value):
                return cand
    return None


def _next(x, steps):
    for _ in range(abs(steps)):
        x = np.nextafter(F(x), F(np.inf) if steps > 0 else F(-np.inf))
    return x


def edge_states(cfg):
    """{name: float32} -- the states the issue lists, for one configuration."""
    up, down = F(np.inf), F(-np.inf)
    s = {"inf": INF, "nan": NAN, "-inf": down, "+0": F(0.0), "-0": F(-0.0), "denormal": F(1e-40),
         "min": cfg.min_value, "min-": np.nextafter(cfg.min_value, down), "min+": np.nextafter(cfg.min_value, up),
         "max": cfg.max_value, "max-": np.nextafter(cfg.max_value, down), "max+": np.nextafter(cfg.max_value, up),
         "thr": cfg.threshold, "thr-": np.nextafter(cfg.threshold, down),
         "max-hit": F(cfg.max_value - cfg.hit),
         "below_min": F(cfg.min_value - max(F(5.0), abs(cfg.min_value))),
         "above_max": F(cfg.max_value + max(F(5.0), abs(cfg.max_value))),
         "flt_max": O.FLT_MAX, "lowest": O.LOWEST, "stuck": F(-2.0 ** 26), "mid+": F(0.7), "mid-": F(-0.7)}
    for k in (1, 2, 3):
        land = landing(cfg, k)
        if land is not None:
            s["land%d" % k] = land
        s["over%d" % k] = F(F(cfg.min_value - F(k) * cfg.miss) + F(0.5) * cfg.miss)   # the k-th miss overshoots
    return s


class Sheet:
    def __init__(self, name, mp, calls, planted, cells=(), layers=("occupancy",), chunk=N):
        self.name, self.mp, self.calls, self.planted = name, mp, calls, planted
        self.cells, self.layers, self.chunk = list(cells), tuple(layers), chunk
        self.events = []
        self.states = O.replay(planted, calls, mp, events=self.events)

    def mutant_states(self, mutant):
        return O.replay(self.planted, self.calls, self.mp, mutant)

    def regions(self):
        return sorted(set(self.planted) | set(self.states[-1]))

    def with_layers(self, layers):
        """The same sheet for a map with another layer set (the model's states do not depend on it)."""
        other = object.__new__(Sheet)
        other.__dict__.update(self.__dict__)
        other.layers = tuple(layers)
        other.name = self.name + "+" + "+".join(layers[1:])
        return other

    def segments(self, k):
        """{region: ray segments of call k}, from the model's own walk; every ray of a sheet lies in one region."""
        out = {}
        rays, flags = self.calls[k].rays, self.calls[k].flags
        for r in range(rays.shape[0] // 2):
            keys, sample = O.cached_visits(rays[2 * r], rays[2 * r + 1], flags, self.mp)
            regions = {key[0] for key in keys} | ({sample[0]} if sample else set())
            assert len(regions) == 1, (self.name, k, r)
            for region in regions:
                out[region] = out.get(region, 0) + 1
        return out

    def samples(self, k):
        out = {}
        for e in self.events[k]:
            if e.kind == "h":
                out[e.key[0]] = out.get(e.key[0], 0) + 1
        return out


Cell = namedtuple("Cell", "state pattern flags call target")


class Layout:
    """Hands out cells region by region along x, keeping every (call, region)'s ray count within [lo, hi]."""

    def __init__(self, mp, lo, hi):
        self.mp, self.lo, self.hi = mp, lo, hi
        self.per_row = mp.dim[0] // 3
        self.capacity = self.per_row * mp.dim[1] * mp.dim[2]
        self.region, self.cell, self.count = 0, 0, 0
        self.rays, self.planted, self.cells = [], {}, []

    def _tile(self):
        return self.planted.setdefault((self.region, 0, 0), np.full(self.mp.volume, INF, dtype=F))

    def _voxels(self):
        row, t = divmod(self.cell, self.per_row)
        ly, lz = row // self.mp.dim[2], (row * 13) % self.mp.dim[2]     # (13: the rows spread over every z slab)
        return [(self.region * self.mp.dim[0] + 3 * t + i, ly, lz) for i in range(3)]

    def next_region(self):
        if self.count and self.count < self.lo:
            self.add(INF, "m" * (self.lo - self.count), "filler", pad=True)
        if self.count or self.cell:
            self.region, self.cell, self.count = self.region + 1, 0, 0

    def add(self, value, pattern, state="", flags=0, call=0, pad=False):
        if not pad and (self.count + len(pattern) > self.hi or self.cell >= self.capacity):
            self.next_region()
        assert self.cell < self.capacity and (pad or len(pattern) <= self.hi)
        left, target, right = self._voxels()
        tile = self._tile()
        for g in (left, target, right):
            tile[self.mp.index((g[0] - self.region * self.mp.dim[0], g[1], g[2]))] = value
        centre = (0.5, 0.5, 0.5)
        for c in pattern:
            a, b = (target, right) if c == "m" else (left, target)
            self.rays.append((point(a, centre, self.mp), point(b, centre, self.mp)))
        self.cells.append(Cell(state, pattern, flags, call, T.key_of(target, self.mp)))
        self.cell += 1
        self.count += len(pattern)

    def take_rays(self):
        """The rays added since the last take, the open region closed."""
        self.next_region()
        rays, self.rays = self.rays, []
        return rays_array(rays)


BOUNDS = {"walk": (0, N), "lists": (N + 1, 3 * N), "any": (0, 1 << 20)}


def states_sheet(cfg_name, dim, packing, res=0.1, calls=2, chunk=N):
    cfg = configs()[cfg_name]
    mp = MapParams(res, dim)
    layout = Layout(mp, *BOUNDS[packing])
    for state, value in edge_states(cfg).items():
        for pattern in PATTERNS:
            layout.add(value, pattern, state)
    rays = layout.take_rays()
    name = "states/%s/%s/%s" % (cfg_name, "x".join(map(str, mp.dim)), packing)
    return Sheet(name, mp, [Call(rays, 0, cfg)] * calls, layout.planted, layout.cells, chunk=chunk)


def flags_sheet(cfg_name, dim, packing, res=0.1):
    cfg = configs()[cfg_name]
    mp = MapParams(res, dim)
    layout = Layout(mp, *BOUNDS[packing])
    states = edge_states(cfg)
    calls = []
    for k, subset in enumerate(O.VALUE_FLAG_SUBSETS):
        for state in FLAG_STATES:
            for pattern in PATTERNS:
                layout.add(states[state], pattern, state, subset, k)
        calls.append(Call(layout.take_rays(), subset, cfg))
    name = "flags/%s/%s/%s" % (cfg_name, "x".join(map(str, mp.dim)), packing)
    return Sheet(name, mp, calls, layout.planted, layout.cells)


def changing_sheet(dim, packing):
    """The default configuration's edge states under four configurations in turn."""
    order = ("default", "tight_11", "tiny", "clamp0")
    mp = MapParams(0.1, dim)
    layout = Layout(mp, *BOUNDS[packing])
    for state, value in edge_states(configs()["default"]).items():
        for pattern in PATTERNS:
            layout.add(value, pattern, state)
    rays = layout.take_rays()
    name = "changing/%s/%s" % ("x".join(map(str, mp.dim)), packing)
    return Sheet(name, mp, [Call(rays, 0, configs()[c]) for c in order], layout.planted, layout.cells)


def count_sheet(dim, counts, chunk=N, res=2.0 ** -4, plain=(), flags=(0, 0)):
    """One region per count: that many rays of one call through one voxel planted with 1.0, under the tiny-miss
    configuration (n roundings differ from one product), the voxel's neighbours as in any cell; then the same again
    with a sample first, so the count lands in an interval before a sample as well as behind the last.  One call per
    entry of `flags`; the cells belong to the first call without kRfExcludeSample."""
    cfg = configs()["tiny"]
    mp = MapParams(res, dim)
    layout = Layout(mp, 0, 1 << 20)
    call = [f & T.RF_EXCLUDE_SAMPLE for f in flags].index(0)
    for n in counts:
        layout.add(F(1.0), "m" * n, "count%d" % n, call=call)
        layout.next_region()
        layout.add(F(1.0), "h" + "m" * (n - 1), "count%d" % n, call=call)
        layout.next_region()
    for n in plain:                                          # (counts past the 15- and 16-bit fields: misses only)
        layout.add(F(1.0), "m" * n, "count%d" % n, call=call)
        layout.next_region()
    rays = layout.take_rays()
    name = "count/%s/%s" % ("x".join(map(str, mp.dim)), "_".join(map(str, tuple(counts) + tuple(plain))))
    return Sheet(name, mp, [Call(rays, f, cfg) for f in flags], layout.planted, layout.cells, chunk=chunk)


def dense_sheet(cfg_name, dim=32, lds_hits=LDS_HITS):
    """One configuration's states in ONE region that also receives more samples than the walk stages in LDS:
    its deferred misses go through the global event list."""
    cfg = configs()[cfg_name]
    mp = MapParams(0.1, dim)
    layout = Layout(mp, 0, 1 << 20)
    states = edge_states(cfg)
    per = (lds_hits + 1) // (len(states) * 2) + 1
    for state, value in states.items():
        for pattern in PATTERNS:
            layout.add(value, pattern, state)
        layout.add(value, "mh" * per, state)                 # a voxel whose events alternate, `per` times
    rays = layout.take_rays()
    name = "dense/%s/%s" % (cfg_name, "x".join(map(str, mp.dim)))
    return Sheet(name, mp, [Call(rays, 0, cfg)] * 2, layout.planted, layout.cells)


# ---------------------------------------------------------------------------------------------------------------------
# kRfStopOnFirstOccupied
# ---------------------------------------------------------------------------------------------------------------------
CHAIN = 45


def stop_sheet(extra=0, layers=("occupancy",)):
    """Rows of one 32^3 region at 0.1 m, each ray 12 voxels along x unless said otherwise:
      z = 2   the wall voxel (x = 12) planted at the threshold / one ulp below it / the other edge states, one per row;
              behind the wall the edge states again (x = 13 ... 18), which a stopped ray gives NULL updates
      z = 4   a voxel one hit below the threshold: a short ray's sample makes it occupied, the long ray behind it stops
      z = 6   a voxel less than one miss above the threshold: the first long ray stops there and frees it, the second
              passes and applies its sample
      z = 8   a staircase of CHAIN rays: ray i crosses V_i and ends in V_(i+1), planted one hit below the threshold:
              it stops in V_i exactly if ray i - 1 did not stop, so the stops alternate, each depending on the one before
    `extra` adds kRfEndPointAsFree or kRfExcludeOrigin to every call."""
    cfg = configs()["default"]
    mp = MapParams(0.1, 32)
    states = edge_states(cfg)
    tile = np.full(mp.volume, INF, dtype=F)
    centre = (0.5, 0.5, 0.5)
    rays = []

    def long_ray(ly, lz, x0=6, x1=19):
        return point((x0, ly, lz), centre, mp), point((x1, ly, lz), centre, mp)

    names = list(states)
    for ly, name in enumerate(names):                           # z = 2
        tile[mp.index((12, ly, 2))] = states[name]
        for i in range(6):
            tile[mp.index((13 + i, ly, 2))] = states[names[(ly + 1 + i * 5) % len(names)]]
        rays += [long_ray(ly, 2)] * 2
    below = F(-cfg.hit)                                          # (threshold 0: below + hit == 0.0 exactly)
    for ly in range(4):                                          # z = 4
        tile[mp.index((12, ly, 4))] = below
        rays.append((point((11, ly, 4), centre, mp), point((12, ly, 4), centre, mp)))
        rays += [long_ray(ly, 4)] * (1 + ly)
    above = F(F(-0.5) * cfg.miss)                                # (occupied; one miss makes it free)
    for ly in range(4):                                          # z = 6
        tile[mp.index((12, ly, 6))] = above
        rays += [long_ray(ly, 6)] * (2 + ly)
    chain = []
    for i in range(CHAIN):                                       # z = 8
        k = i // 2
        if i % 2 == 0:
            o, v, w = (k + 1, k + 2), (k + 2, k + 2), (k + 3, k + 2)
        else:
            o, v, w = (k + 3, k + 1), (k + 3, k + 2), (k + 3, k + 3)
        if i > 0:
            tile[mp.index((v[0], v[1], 8))] = below
        chain.append((point((o[0], o[1], 8), centre, mp), point((w[0], w[1], 8), centre, mp)))
    rays += chain
    flags = RF_STOP_ON_FIRST_OCCUPIED | extra
    calls = [Call(rays_array(rays), flags, cfg), Call(rays_array(rays[::-1]), flags, cfg)]
    name = "stop/%d%s" % (extra, "" if len(layers) == 1 else "+mean")
    sheet = Sheet(name, mp, calls, {(0, 0, 0): tile}, layers=layers)
    sheet.chain = (len(rays) - CHAIN, CHAIN)                     # where the staircase sits in call 0
    return sheet


# ---------------------------------------------------------------------------------------------------------------------
# sites
# ---------------------------------------------------------------------------------------------------------------------
SITES = ("walk", "lists", "dense", "mean", "odd", "half", "stop", "tiled", "spill", "maxchunk")
MEAN = ("occupancy", "mean")
ODD_DIMS = ((17, 17, 17), (18, 17, 17), (15, 9, 7))             # odd; even but no multiple of 4; odd and half-size
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _states(cfg, dim, packing, **kw):
    return _cached(("states", cfg, dim, packing), lambda: states_sheet(cfg, dim, packing, **kw))


def build(site):
    """The sheets of one site (cached: sites share sheets)."""
    names = list(configs())
    if site in ("walk", "lists"):
        out = [_states(c, 32, site) for c in names]
        out += [_cached(("flags", c, 32, site), lambda c=c: flags_sheet(c, 32, site)) for c in FLAG_CONFIGS]
        out.append(_cached(("changing", 32, site), lambda: changing_sheet(32, site)))
        counts = (N,) if site == "walk" else (N + 1,)
        out.append(_cached(("count", 32, counts), lambda: count_sheet(32, counts)))
        return out
    if site == "dense":
        return [_cached(("dense", c), lambda c=c: dense_sheet(c)) for c in ("default", "clamp0")]
    if site == "mean":
        out = []
        for packing in ("walk", "lists"):
            out += [_states(c, 32, packing).with_layers(MEAN) for c in ("default", "clamp0", "tight_11", "tiny")]
            out.append(_cached(("flags", "default", 32, packing),
                               lambda p=packing: flags_sheet("default", 32, p)).with_layers(MEAN))
        out.append(_cached(("count", 32, (N, N + 1)), lambda: count_sheet(32, (N, N + 1))).with_layers(MEAN))
        return out
    if site == "odd":
        out = []
        for dim in ODD_DIMS:
            for packing in ("walk", "lists"):
                sheet = _states("clamp0", dim, packing)
                out += [sheet, sheet.with_layers(MEAN)]
                out.append(_cached(("flags", "default", dim, packing),
                                   lambda d=dim, p=packing: flags_sheet("default", d, p)))
        return out
    if site == "half":
        return [_states(c, 16, p) for c in ("default", "clamp0", "tiny") for p in ("walk", "lists")] + [
            _cached(("flags", "default", 16, "walk"), lambda: flags_sheet("default", 16, "walk")),
            _cached(("count", 16, (N, N + 1)), lambda: count_sheet(16, (N, N + 1)))]
    if site == "stop":
        out = []
        for extra in (0, RF_END_POINT_AS_FREE, RF_EXCLUDE_ORIGIN):
            out.append(_cached(("stop", extra), lambda e=extra: stop_sheet(e)))
            out.append(_cached(("stop", extra), lambda e=extra: stop_sheet(e)).with_layers(MEAN))
        return out
    if site == "tiled":
        return [_states(c, 48, p) for c in ("default", "clamp0") for p in ("walk", "lists")] + [
            _cached(("flags", "default", 48, "walk"), lambda: flags_sheet("default", 48, "walk"))]
    if site == "spill":
        return [_cached(("states", c, 32, "any"), lambda c=c: states_sheet(c, 32, "any", calls=3))
                for c in ("default", "clamp0")]
    if site == "maxchunk":
        return [_cached("maxchunk", lambda: count_sheet(32, (MAX_CHUNK, MAX_CHUNK + 1), chunk=MAX_CHUNK,
                                                        plain=((1 << 15) + 1, (1 << 16) + 1),
                                                        flags=(T.RF_EXCLUDE_SAMPLE, 0)))]
    raise KeyError(site)


def all_sheets():
    """Every distinct sheet, with the sites that use it."""
    out = {}
    for site in SITES:
        for sheet in build(site):
            out.setdefault(sheet.name, (sheet, []))[1].append(site)
    return list(out.values())


def make_oracle(sheet):
    """An OracleMap of the sheet's geometry and layers holding its planted regions (every other layer cleared)."""
    from oracle.oracle import LAYER_DTYPES, OracleMap
    mp = sheet.mp
    om = OracleMap(mp.res, mp.dim, sheet.layers)
    for region, tile in sheet.planted.items():
        c = [T.voxel_centre_axis(region[a] * mp.dim[a] + mp.dim[a] // 2, a, mp) for a in range(3)]
        om.integrate_occupancy(np.array([c, c]))                 # creates the region; overwritten next
        for name in sheet.layers:
            om.region_layer_view(region, name)[:] = np.zeros(1, dtype=LAYER_DTYPES[name][0])
        om.region_layer_view(region, "occupancy")[:] = tile
    return om


def set_oracle_config(om, cfg):
    from oracle.oracle import lib
    lib.oracle_map_set_hit_value(om.handle, float(cfg.hit))
    lib.oracle_map_set_miss_value(om.handle, float(cfg.miss))
    p = [p for p in (0.5, 0.6) if _p(p) == cfg.threshold][0]   # (the oracle takes its threshold as a probability)
    lib.oracle_map_set_threshold_probability(om.handle, p)
    lib.oracle_map_set_min_max(om.handle, float(cfg.min_value), float(cfg.max_value))
    lib.oracle_map_set_saturation(om.handle, int(cfg.sat_min), int(cfg.sat_max))
