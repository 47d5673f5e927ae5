"""Constructed sheets for the TSDF voxel update (test infrastructure): tests/test_tsdf_ref.py (CPU) holds the conditions
they meet, tests/test_gpu_tsdf_states.py (-m gpu) holds the device to them.

A sheet is one region of planted (weight, distance) states, a list of calls (ray batches), each under one option set,
and the model's answer: every ray is walked with the oracle's own `walk`, every visit's sdf comes from
tsdf_ref.sdf_ref, and tsdf_ref.update_ref is replayed over them voxel by voxel in ray order -- the whole region, not
only the voxels a ray was aimed at, so nothing a ray does on its way is left unjudged.

Layout.  Voxels are planted in rows along x.  `free` rows hold every planted weight at the truncation distance (what a
free-space voxel looks like) and get groups of n = 1, 2, 37, 146 long rays per call that start in the row's near half
and end near its far end: the voxels before the ends see free-space visits only, 1 to n of them.  `edge` rows hold every
planted weight against every planted distance and get one short ray per voxel and call, cut so that the sdf at the
voxel's centre lands on an edge: within a few ulp of 1.01f * trunc (formed in float32), of trunc, of 0 and of -trunc,
behind the surface, below -trunc.  A short ray keeps sqrt(|sample - sensor|^2) below 0.5 (0.125 for the small
truncation distance), where float32 resolves single ulps of the truncation distance; aim() scans the cut in steps of
2^-29 m for the wanted value and the case is discarded where none of the 513 cuts reaches it within 4 ulp
(Sheet.discarded; the CPU test bounds it).  Where a drop-off can clamp a visit's weight to 0, a `lone` row that no
other ray crosses holds weights on and around 0.00001f, the near-zero threshold of the update.

An option-change script (CHANGES) feeds two calls per option set, few rays per group before the last change and many
after it; the ones that make uncountable states themselves (HOLES) leave most free rows unobserved: what those voxels
hold when the options change, the script made.

Sites (which device code applies a voxel's free-space count):
  direct  32^3, at most 512 rays per call: one walk chunk, k_region_walk applies the counts itself
  apply4  32^3, more than 512 rays per call: k_apply_counts_tsdf, four voxels per lane
  apply1  31^3 (volume not divisible by 4), more than 512 rays: k_apply_counts_tsdf, one voxel per lane
  tiled   48^3, cut into z slabs by the library; rows in every slab
  replay  32^3, every planted distance off the truncation distance: k_replay_tsdf for every planted voxel
  spill   32^3, the region evicted to the host store and re-admitted between the calls"""
import ctypes as C
from collections import namedtuple

import numpy as np

import tsdf_ref
from oracle.oracle import Key, OracleMap
from oracle.oracle import lib as _olib
from tsdf_ref import F, UPDATE_MUTANTS, bits, opts, sdf_ref, update_ref

RES = 0.1
SEED = 7
REGION = (0, 0, 0)
FREE_MARGIN = F(1.01)            # a visit at or past FREE_MARGIN * trunc (float32 product) is what the device may count
SCAN = 256                       # aim(): cuts tried each side of the nominal one
SCAN_STEP = 2.0 ** -29
NEAR_ULPS = 4
COUNTS = (1, 2, 37, 146)
SITES = ("direct", "apply4", "apply1", "tiled", "replay", "spill")
SITE_DIM = {"direct": 32, "apply4": 32, "apply1": 31, "tiled": 48, "replay": 32, "spill": 32}
CHUNK_RAYS = 512                 # rays through one region in a batch of at most 16384 that still fit one walk chunk
SMALL_TRUNC = 0.04

Refuse = namedtuple("Refuse", "trunc")        # a truncation distance the populated map must refuse

_UP = float(np.nextafter(F(1e4), F(np.inf)))
# variant -> the option sets of its segments, in order (a Refuse between two segments is tried and must fail)
VARIANTS = {
    "default": [opts()],
    "reversed": [opts()],                                       # `default` with every call's rays in reverse order
    "dropoff": [opts(dropoff=0.05)],
    "small_trunc": [opts(trunc=SMALL_TRUNC)],
    "small_trunc_dropoff": [opts(trunc=SMALL_TRUNC, dropoff=0.01, sparsity=0.5)],
    "sparsity_half": [opts(sparsity=0.5)],
    "sparsity_03_max_3": [opts(sparsity=0.3, max_weight=3.0)],
    "sparsity_0_max_03": [opts(sparsity=0.0, max_weight=0.3)],
    "sparsity_neg_max_above_1e4": [opts(sparsity=-1.0, max_weight=_UP)],
    "max_2e6": [opts(max_weight=2e6)],
    "drop_on_off": [opts(dropoff=0.05), opts()],
    "drop_off_on_off": [opts(), opts(dropoff=0.05), opts()],
    "max_03_then_1e4": [opts(max_weight=0.3), opts()],
    "max_011_then_1e4": [opts(max_weight=0.11), opts()],
    "max_2e6_then_1e4": [opts(max_weight=2e6), opts()],
    "sparsity_03_then_1": [opts(sparsity=0.3), opts()],
    "trunc_refused": [opts(), Refuse(0.2), opts()],
}
CHANGES = ("drop_on_off", "drop_off_on_off", "max_03_then_1e4", "max_011_then_1e4", "max_2e6_then_1e4",
           "sparsity_03_then_1", "trunc_refused")
# ... of which the script itself makes states that may not be counted.  (A cap of 0.3 is not among them: 0.3f + 1 + ...
# + 1 and 0.3f + float(n) round to the same float32 for every n up to 300, as for most caps below 1; 0.11f parts ways at
# n = 2.)
HOLES = ("drop_on_off", "drop_off_on_off", "max_011_then_1e4")
SITE_VARIANTS = {
    "direct": tuple(VARIANTS),
    "apply4": ("default", "small_trunc_dropoff", "drop_on_off", "max_011_then_1e4"),
    "apply1": ("default", "small_trunc_dropoff", "drop_on_off", "max_011_then_1e4"),
    "tiled": ("default", "small_trunc_dropoff", "drop_on_off", "max_011_then_1e4"),
    "replay": ("default", "dropoff", "small_trunc_dropoff"),
    "spill": ("default", "small_trunc_dropoff", "drop_on_off", "max_011_then_1e4"),
}


def planted_weights(max_weight):
    return [0.0, -0.0, 1.0, 1e4 - 1, 1e4, 1e4 + 1, float(max_weight), 2.0 ** 24 - 1, 2.0 ** 24, 0.3, 2.5, 1e-6, 1e-5,
            -1.0, -2.0, -1.0 + 2.0 ** -20, np.inf, np.nan, 1e-40, 3.0, 17.0]


def planted_distances(trunc):
    t = F(trunc)
    return [t, -t, F(0.0), F(-0.0), np.nextafter(t, F(0)), np.nextafter(t, F(np.inf)), F(2) * t, F(-2) * t, F(np.nan)]


def ordinal(x):
    """float32 -> an integer that grows with the value, one per ulp (-0.0 and 0.0 share 0)."""
    b = bits(x).astype(np.int64)
    return np.where(b & 0x80000000, -(b & 0x7fffffff), b)


class Geo:
    """One region of dim^3 voxels at the default origin: centres and walks from the oracle's own map code."""

    def __init__(self, dim):
        self.dim = dim
        self.om = OracleMap(RES, (dim,) * 3, ("tsdf",))
        self._centres = {}
        cap = 512
        self._cap = cap
        self._keys, self._enter, self._exit = (Key * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
        self._view = np.frombuffer(self._keys, dtype=np.uint8).reshape(cap, C.sizeof(Key))

    def index(self, local):
        return local[0] + self.dim * (local[1] + self.dim * local[2])

    def local(self, vi):
        return vi % self.dim, (vi // self.dim) % self.dim, vi // (self.dim * self.dim)

    def centre(self, vi):
        if vi not in self._centres:
            self._centres[vi] = self.om.voxel_centre(REGION, self.local(vi))
        return self._centres[vi]

    def walk(self, start, end):
        """Voxel indices of region (0, 0, 0) in the order the reference walks them, or None where the ray leaves it."""
        n = _olib.oracle_walk_segment_keys(self.om.handle, (C.c_double * 3)(*start), (C.c_double * 3)(*end), 0,
                                           self._keys, self._enter, self._exit, self._cap)
        if n > self._cap:
            return None
        raw = self._view[:n]
        if raw[:, :6].any():                                     # three int16 region coordinates, all zero
            return None
        loc = raw[:, 6:9].astype(np.int64)
        return loc[:, 0] + self.dim * (loc[:, 1] + self.dim * loc[:, 2])


Call = namedtuple("Call", "opts segment rays vi sdf sdf_late ray")


class Sheet:
    def __init__(self, site, variant):
        self.site, self.variant, self.dim = site, variant, SITE_DIM[site]
        self.name = "%s/%s" % (site, variant)
        self.script = VARIANTS[variant]
        self.calls = []               # Call, in order
        self.drawn = self.discarded = 0
        self.aimed = []               # (call, voxel, edge name) of every short ray kept
        self.free_rows, self.edge_rows = [], []

    @property
    def volume(self):
        return self.dim ** 3

    def tile(self):
        t = np.empty(2 * self.volume, dtype=F)
        t[0::2], t[1::2] = self.w0, self.d0
        return t


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
def edges_of(trunc):
    """(name, target float32 or None, ulps from it) of the short rays' aims."""
    t = F(trunc)
    m = FREE_MARGIN * t
    out = [("free", None, 0), ("inside", None, 0), ("behind", None, 0)]
    out += [("margin", m, k) for k in (-3, -1, 0, 1, 3)]
    out += [("trunc", t, k) for k in (-2, -1, 0, 1, 2)]
    out += [("zero", F(0), k) for k in (-1, 0, 1)]
    if t < F(0.5 * RES):                  # the end voxel's centre lies at most half a voxel past the sample along the ray
        out += [("neg_trunc", -t, k) for k in (-3, -1, 0, 1, 3)]
        out += [("below_neg_trunc", None, 0)]
    return out


def nominal(rng, trunc, name, target):
    t = float(trunc)
    if name == "free":
        return t * rng.uniform(1.5, 3.0)
    if name == "inside":
        return t * rng.uniform(0.2, 0.8)
    if name == "behind":
        return -min(0.45 * RES, t) * rng.uniform(0.2, 0.8)
    if name == "below_neg_trunc":
        return -rng.uniform(t * 1.02, 0.048)
    return float(target)


def aim(rng, geo, centre, trunc, name, target, k):
    """A short ray (sensor, sample) whose sdf at `centre` is the wanted one, or None."""
    tilt = rng.uniform(-0.004, 0.004, 2)
    direction = np.array([1.0, tilt[0], tilt[1]])
    direction /= np.linalg.norm(direction)
    back = rng.uniform(0.07, 0.15) if trunc > F(0.1) else rng.uniform(0.05, 0.058)
    sensor = np.array(centre) - direction * back
    length = back + nominal(rng, trunc, name, target)
    if target is None:
        return sensor, sensor + direction * length
    cuts = length + SCAN_STEP * np.arange(-SCAN, SCAN + 1)
    samples = sensor[None, :] + direction[None, :] * cuts[:, None]
    sdf = sdf_ref(sensor[None, :], samples, np.array(centre)[None, :])
    if float(target) == 0.0:
        ok = (sdf == 0) if k == 0 else ((sdf > 0) & (sdf < F(1e-6)) if k > 0 else (sdf < 0) & (sdf > F(-1e-6)))
        hit = np.flatnonzero(ok)
    else:
        off = ordinal(sdf) - int(ordinal(target))
        hit = np.flatnonzero(off == k)
        if hit.size == 0 and k != 0:
            hit = np.flatnonzero((np.sign(off) == np.sign(k)) & (np.abs(off) <= NEAR_ULPS))
    if hit.size == 0:
        return None
    return sensor, samples[hit[len(hit) // 2]]


def long_ray(rng, geo, row, trunc):
    """From a voxel of the row's near half to a cut just past the free-space margin of a voxel near its far end."""
    ly, lz = row
    tilt = rng.uniform(-0.004, 0.004, 2)
    direction = np.array([1.0, tilt[0], tilt[1]])
    direction /= np.linalg.norm(direction)
    # (the start anywhere in the row's near half: the voxels there see every count up to the group's, the far half all)
    sensor = np.array(geo.centre(geo.index((int(rng.integers(geo.dim // 2)), ly, lz)))) + rng.uniform(-0.02, 0.02, 3)
    target = np.array(geo.centre(geo.index((geo.dim - 5 - int(rng.integers(4)), ly, lz))))
    cut = float(trunc) * (rng.uniform(1.0101, 1.02) if rng.integers(2) else rng.uniform(0.0, 1.0))
    return sensor, sensor + direction * (np.dot(target - sensor, direction) + cut)


# ---------------------------------------------------------------------------------------------------------------------
# building
# ---------------------------------------------------------------------------------------------------------------------
TILE_VOXELS = 1 << 15                # the library cuts larger regions into equal z slabs (ohm_amd/csrc/tiling_impl.h)


def slab_layers(dim):
    """z layers per tile of a dim^3 region: the largest divisor of dim whose slab holds at most TILE_VOXELS voxels."""
    return max(t for t in range(1, dim + 1) if dim % t == 0 and dim * dim * t <= TILE_VOXELS)


def rows_of(site, dim, variant):
    """(free rows, edge rows, the lone row) as (ly, lz): z spread over the region, so over every slab of a tiled one."""
    zs = [2, dim // 3, dim // 2, (2 * dim) // 3, dim - 3]
    ys = list(range(1, dim - 1, 3))
    grid = [(y, z) for z in zs for y in ys]
    rng = np.random.default_rng(5)
    rng.shuffle(grid)
    n_free, n_edge = (4, 8) if site == "direct" else (8, 11)
    if site == "direct" and variant in CHANGES:
        n_free, n_edge = 4, 3                    # (two groups of 146, two of 37 after the last change: one chunk still)
    return grid[:n_free], grid[n_free:n_free + n_edge], grid[n_free + n_edge]


def build_sheet(site, variant, seed=SEED):
    sheet = Sheet(site, variant)
    geo = Geo(sheet.dim)
    sheet.geo = geo
    dim = sheet.dim
    rng = np.random.default_rng([seed, SITES.index(site), list(VARIANTS).index(variant)])
    segments = [s for s in sheet.script if not isinstance(s, Refuse)]
    first = segments[0]
    weights = planted_weights(first.max_weight)
    distances = planted_distances(first.trunc)
    sheet.free_rows, sheet.edge_rows, lone_row = rows_of(site, dim, variant)
    # Where drop-off can clamp a visit's weight to 0 (sdf below -trunc), new_weight IS the stored weight: voxels of a row
    # no other ray crosses hold 0.00001f itself, its neighbours and weights inside the near-zero band, each with a
    # distance beyond the truncation distance -- the update clamps it or, inside the band, must leave it alone.
    lone = []
    if first.dropoff > 0 and first.trunc < F(0.5 * RES):
        band = [F(1e-5), np.nextafter(F(1e-5), F(0)), np.nextafter(F(1e-5), F(1)), F(1e-6), F(-1e-5), F(-1e-6)]
        lone = [(geo.index((lx, lone_row[0], lone_row[1])), band[i % len(band)])
                for i, lx in enumerate(range(3, dim - 3, 3))]
    w0, d0 = np.zeros(sheet.volume, dtype=F), np.zeros(sheet.volume, dtype=F)
    named_zero = np.zeros(sheet.volume, dtype=bool)
    for r, (ly, lz) in enumerate(sheet.free_rows):
        for lx in range(dim):
            vi = geo.index((lx, ly, lz))
            w = F(weights[(lx + 3 * r) % len(weights)])
            # a free-space voxel: the truncation distance -- or, for the replay site, anything but (every voxel flagged)
            d = distances[1 + (lx + r) % (len(distances) - 1)] if site == "replay" else F(first.trunc)
            if w == 0 and site != "replay":
                d = F(0.0) if (lx + r) % 3 else F(-0.0)          # unobserved, and its signed-zero variants
            if variant in HOLES and r >= 1:
                w, d = F(0.0), F(0.0)      # a fresh map: whatever these voxels hold later, the script itself made
            w0[vi], d0[vi], named_zero[vi] = w, d, True
    for r, (ly, lz) in enumerate(sheet.edge_rows):
        for lx in range(dim):
            vi = geo.index((lx, ly, lz))
            w0[vi] = F(weights[(lx + 5 * r) % len(weights)])
            d0[vi] = distances[(1 if site == "replay" else 0) + (lx + r) % (len(distances) - (site == "replay"))]
            named_zero[vi] = True
    for i, (vi, w) in enumerate(lone):
        w0[vi], d0[vi], named_zero[vi] = w, F(2 if i % 2 else -2) * first.trunc, True
    n_calls = 3 if len(segments) == 1 else 2
    for si, o in enumerate(segments):
        edges = edges_of(o.trunc)
        for k in range(n_calls):
            rays = []
            for r, row in enumerate(sheet.free_rows):
                count = COUNTS[(r + k + si) % len(COUNTS)]
                if len(segments) > 1:
                    # an option-change script: few visits first, many after the last change -- a small weight that the
                    # earlier options left crosses several binades then, where n roundings and one part ways
                    count = COUNTS[2 + (r + k) % 2] if si == len(segments) - 1 else COUNTS[(r + k) % 2]
                for _ in range(count):
                    sheet.drawn += 1
                    sensor, sample = long_ray(rng, geo, row, o.trunc)
                    if geo.walk(sensor, sample) is None:
                        sheet.discarded += 1
                        continue
                    rays.append((sensor, sample))
            for r, (ly, lz) in enumerate(sheet.edge_rows):
                for lx in range(2, dim - 6):
                    vi = geo.index((lx, ly, lz))
                    name, target, ulps = edges[(lx + 2 * r + 7 * k + 3 * si) % len(edges)]
                    sheet.drawn += 1
                    ray = None
                    for _ in range(3):                           # redrawn here, never on the GPU
                        ray = aim(rng, geo, geo.centre(vi), o.trunc, name, target, ulps)
                        if ray is not None:
                            visited = geo.walk(*ray)
                            if visited is not None and vi in visited:
                                break
                            ray = None
                    if ray is None:
                        sheet.discarded += 1
                        continue
                    rays.append(ray)
                    sheet.aimed.append((len(sheet.calls), vi, name))
            for vi, _ in lone:
                sheet.drawn += 1
                ray = aim(rng, geo, geo.centre(vi), o.trunc, "below_neg_trunc", None, 0)
                visited = geo.walk(*ray)
                if visited is None or vi not in visited or len(visited) > 2:
                    sheet.discarded += 1
                    continue
                rays.append(ray)
                sheet.aimed.append((len(sheet.calls), vi, "lone"))
            if variant == "reversed":
                rays.reverse()
            sheet.calls.append(make_call(geo, o, si, rays))
    sheet.w0, sheet.d0, sheet.named_zero = w0, d0, named_zero
    sheet.states = replay(sheet)
    return sheet


def make_call(geo, o, segment, rays):
    arr = np.empty((2 * len(rays), 3), dtype=np.float64)
    arr[0::2] = [r[0] for r in rays]
    arr[1::2] = [r[1] for r in rays]
    ray_id, vis = [], []
    for i in range(len(rays)):
        v = geo.walk(arr[2 * i], arr[2 * i + 1])
        vis.append(v)
        ray_id.append(np.full(len(v), i))
    vi, ray_id = np.concatenate(vis), np.concatenate(ray_id)
    centres = np.array([geo.centre(int(v)) for v in vi])
    sensor, sample = arr[0::2][ray_id], arr[1::2][ray_id]
    return Call(o, segment, arr, vi, sdf_ref(sensor, sample, centres), sdf_ref(sensor, sample, centres, "dot_cast_late"),
                ray_id)


def build(sites=SITES, seed=SEED):
    return [build_sheet(site, variant, seed) for site in sites for variant in SITE_VARIANTS[site]]


# ---------------------------------------------------------------------------------------------------------------------
# the model's answer
# ---------------------------------------------------------------------------------------------------------------------
def replay(sheet, mutant=None, record=None, trace=None):
    """(w, d) of the whole region after every call: update_ref over every visit, each voxel's in ray order (voxels are
    independent, so round j applies the j-th visit of every voxel at once).  `record` gets one entry per call with every
    visited voxel's state before and after, its visit count and its smallest sdf."""
    w, d = sheet.w0.copy(), sheet.d0.copy()
    states = []
    update_mutant = mutant if mutant in UPDATE_MUTANTS else None
    for call in sheet.calls:
        o = call.opts
        sdf = call.sdf_late if mutant == "dot_cast_late" else call.sdf
        order = np.argsort(call.vi, kind="stable")
        v, s = call.vi[order], sdf[order]
        starts = np.flatnonzero(np.r_[True, v[1:] != v[:-1]])
        counts = np.diff(np.r_[starts, len(v)])
        rank = np.arange(len(v)) - np.repeat(starts, counts)
        gv = v[starts]
        w_before, d_before = w[gv].copy(), d[gv].copy()
        with np.errstate(all="ignore"):
            low = np.minimum.reduceat(s, starts)
            free = low >= FREE_MARGIN * o.trunc
        skip = np.zeros(len(v), dtype=bool)
        if mutant == "count_once":
            with np.errstate(all="ignore"):
                ok = free & ((d_before == o.trunc) | ((w_before == 0) & (d_before == 0)))
                wn = w_before[ok] + counts[ok].astype(F)
                w[gv[ok]] = np.where(o.max_weight < wn, o.max_weight, wn)
            d[gv[ok]] = o.trunc
            skip = np.repeat(ok, counts)
        for j in range(int(rank.max()) + 1):
            sel = (rank == j) & ~skip
            if sel.any():
                t = v[sel]
                w[t], d[t] = update_ref(o, s[sel], w[t], d[t], update_mutant, trace)
        if record is not None:
            record.append(dict(vi=gv, n=counts, low=low, free=free, w0=w_before, d0=d_before, w1=w[gv].copy(),
                               d1=d[gv].copy(), sdf=s, starts=starts, opts=o))
        states.append((w.copy(), d.copy()))
    return states


def shortcut(entry):
    """What counting gives for every voxel of a record entry: (min(w + float(n), max_weight), trunc)."""
    o = entry["opts"]
    with np.errstate(all="ignore"):
        wn = entry["w0"] + entry["n"].astype(F)
        return np.where(o.max_weight < wn, o.max_weight, wn).astype(F), np.full(len(wn), o.trunc, dtype=F)


def differing(a, b):
    """Voxels at which two (w, d) states differ (any NaN equals any NaN)."""
    return np.flatnonzero(~(tsdf_ref.same(a[0], b[0]) & tsdf_ref.same(a[1], b[1])))


def batches(sheet, merged):
    """The calls as the device and the oracle get them: [(opts, segment, rays)], one per call, or -- merged -- one per
    segment with the calls' rays in order."""
    if not merged:
        return [(c.opts, c.segment, c.rays) for c in sheet.calls]
    out = []
    for c in sheet.calls:
        if out and out[-1][1] == c.segment:
            out[-1] = (c.opts, c.segment, np.concatenate([out[-1][2], c.rays]))
        else:
            out.append((c.opts, c.segment, c.rays))
    return out


def refusals(sheet):
    """segment index -> truncation distance to try (and see refused) before that segment's first call."""
    out, si = {}, 0
    for s in sheet.script:
        if isinstance(s, Refuse):
            out[si] = s.trunc
        else:
            si += 1
    return out


def make_oracle(sheet):
    """An OracleMap holding the sheet's planted region, options of the first segment."""
    om = OracleMap(RES, (sheet.dim,) * 3, ("tsdf",))
    set_options(om, sheet.calls[0].opts)
    c = np.array(sheet.geo.centre(sheet.geo.index((sheet.dim // 2,) * 3)))
    om.integrate_tsdf(np.array([c, c]))                  # creates region (0, 0, 0); overwritten next
    om.region_layer_view(REGION, "tsdf")[:] = sheet.tile()
    return om


def set_options(om, o):
    om.set_tsdf(max_weight=float(o.max_weight), trunc=float(o.trunc), dropoff=float(o.dropoff),
                sparsity=float(o.sparsity))


def state_of(tile):
    tile = np.asarray(tile).view(F)
    return tile[0::2], tile[1::2]
