"""Constructed sheets for the traversal layer (test infrastructure): tests/test_traversal_ref.py (CPU) holds the
conditions they meet, tests/test_gpu_traversal_states.py (-m gpu) holds the device to them.

A sheet is a map geometry, planted traversal (and, for `stop`, occupancy) tiles, a list of calls (rays + ray flags) and
the model's state of every touched region after every call (traversal_ref.replay).  Families:

  tiny_start  rays that start a hair before a voxel wall and end in the next voxel: visits of exactly 2^-29, 3 * 2^-29,
              5 * 2^-29 m (ties: 0, 2, 2 units at 2^-28 m), just below one unit, 1e-7 m and, where the key maths'
              rounding makes one, ~1e-16 m.  Every visit of the sheet is tiny.  Each call opens with a sub-voxel ray
              that reports nothing and closes with a tiny-start ray, so the exit range a call leaves behind is tiny.
  tiny_end    the mirror: rays that end a hair before a wall, under kRfEndPointAsFree.
  wrap        2^-4 m: axis-aligned full-voxel visits of exactly 2^24 units, 255 / 256 / 257 / 512 of them through one
              row per call, the 256-, 257- and 512-rows planted with 2^22 m; then 450 rays of unequal lengths through
              one voxel (> 16 m in one call).  With `filler`, other rays of the region are interleaved so its segments
              fall into several walk chunks.
  fold        the same random rays over two regions as 1, 2, 3 and 6 calls, on tiles planted with 2^21, 2^17 and
              2^10 m in a repeating pattern (sub-ulp batches) -- samples and visits meet in most voxels.
  flags       random, degenerate (zero-length, sub-voxel after a long ray), tiny-start and tiny-end rays under one
              ray-flag combination.
  entry       rays into the neighbouring regions by an x, a y and a z step, through an edge and a corner exactly
              (several axes tie) and a few 1e-8 m beside them (the axes' last step times differ by a few units); the
              eight regions around one corner.
  corner      rays that start within 1e-7 m of that corner and cross it: every region is entered within a few units
              of the other axes' steps, so a wrong entry time stays far inside the old tolerance.
  large       4.5, 4.75 and 10 m voxels (unit_bits 28, 27, 26); at 4.5 m visits within nanometres of the full voxel
              diagonal, just under 2^31 units.
  stop        kRfStopOnFirstOccupied over a planted wall."""
import itertools

import numpy as np

import traversal_ref as T
from traversal_ref import (F, RF_END_POINT_AS_FREE, RF_EXCLUDE_ORIGIN, RF_EXCLUDE_RAY, RF_EXCLUDE_SAMPLE,
                           RF_STOP_ON_FIRST_OCCUPIED, Call, MapParams)

SEED = 11
FINE = 2.0 ** -4
SITES = ("direct", "chunks", "mean", "stop", "ndt", "rewalk", "tiled", "spill")
ULP = "ulp"                      # a tiny that means: the float64 next to the wall
TINIES = (2.0 ** -29, 3 * 2.0 ** -29, 5 * 2.0 ** -29, 2.0 ** -28 - 2.0 ** -52, 0.75 * 2.0 ** -28, 1e-7, 1e-16, ULP)
WRAP_COUNTS = (255, 256, 257, 512)
FLAG_SETS = {"end_as_free": RF_END_POINT_AS_FREE, "exclude_origin": RF_EXCLUDE_ORIGIN,
             "end_as_free_exclude_origin": RF_END_POINT_AS_FREE | RF_EXCLUDE_ORIGIN,
             "exclude_sample": RF_EXCLUDE_SAMPLE, "exclude_ray": RF_EXCLUDE_RAY}


class Sheet:
    def __init__(self, name, mp, calls, planted=None, planted_occupancy=None, rewalk=False):
        self.name, self.mp, self.calls = name, mp, calls
        self.planted = planted or {}
        self.planted_occupancy = planted_occupancy
        self.rewalk = rewalk
        self.details = []
        self.states = T.replay(self.planted, calls, mp, self.occupancy(), rewalk=rewalk, details=self.details)

    def occupancy(self):
        """A fresh occupancy tracker for sheets whose flags need one."""
        if not any(c.flags & RF_STOP_ON_FIRST_OCCUPIED for c in self.calls):
            return None
        planted = {}
        for region, tile in (self.planted_occupancy or {}).items():
            for vi in np.flatnonzero(tile != F(np.inf)):
                planted[(region, int(vi))] = tile[vi]
        return T.Occupancy(self.mp, planted)

    def mutant_states(self, mutant):
        return T.replay(self.planted, self.calls, self.mp, self.occupancy(), mutant=mutant, rewalk=self.rewalk)

    def regions(self):
        return sorted(set(self.planted) | set(self.states[-1]))


# ---------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------
def wall(g, a, mp):
    """Lower wall of global voxel g along axis a, as the walk computes it."""
    return T.voxel_centre_axis(g, a, mp) - 0.5 * mp.res


def point(g, frac, mp):
    return [wall(g[a], a, mp) + frac[a] * mp.res for a in range(3)]


def rays_array(rays):
    arr = np.empty((2 * len(rays), 3), dtype=np.float64)
    arr[0::2] = [r[0] for r in rays]
    arr[1::2] = [r[1] for r in rays]
    return arr


def tiny_start_ray(g, axis, sgn, tiny, mp):
    start = point(g, (0.5, 0.5, 0.5), mp)
    if tiny == ULP:
        start[axis] = float(np.nextafter(wall(g[axis] + 1, axis, mp), -np.inf) if sgn > 0 else
                            np.nextafter(wall(g[axis], axis, mp), np.inf))
        tiny = 0.0
    else:
        start[axis] = wall(g[axis] + 1, axis, mp) - tiny if sgn > 0 else wall(g[axis], axis, mp) + tiny
    end = list(start)
    end[axis] = start[axis] + sgn * (tiny + 0.4 * mp.res)
    if T.global_voxel(start, mp) != tuple(g):
        return None                                  # (the key maths rounded the start into the neighbour)
    return start, end


def tiny_end_ray(g, axis, sgn, tiny, mp):
    """From the middle of voxel g to `tiny` before the far wall of its neighbour (tiny = 0: onto the wall)."""
    start = point(g, (0.5, 0.5, 0.5), mp)
    end = list(start)
    n = g[axis] + sgn
    if tiny == ULP:
        end[axis] = float(np.nextafter(wall(n + 1, axis, mp), -np.inf) if sgn > 0 else
                          np.nextafter(wall(n, axis, mp), np.inf))
    else:
        end[axis] = wall(n + 1, axis, mp) - tiny if sgn > 0 else wall(n, axis, mp) + tiny
    return start, end


def tiny_rays(maker, mp, corner, tinies=TINIES):
    """One ray per (axis, direction, tiny), each in voxels of its own, laid out from global voxel `corner`."""
    out = []
    for i, (axis, sgn, tiny) in enumerate(itertools.product(range(3), (1, -1), tinies)):
        g = [corner[0] + 1 + 3 * (i % 6), corner[1] + 1 + 3 * ((i // 6) % 6), corner[2] + 1 + 3 * (i // 36)]
        ray = maker(g, axis, sgn, tiny, mp)
        if ray is not None:
            out.append(ray)
    return out


def sub_voxel_ray(g, mp):
    return point(g, (0.2, 0.3, 0.4), mp), point(g, (0.7, 0.5, 0.6), mp)


def random_rays(rng, mp, n, centre_g, sensor_share=0.5):
    """n rays around global voxel centre_g, within +-0.35 of a region per axis: half from one sensor voxel."""
    ext = [0.35 * d for d in mp.dim]
    sensor = point([centre_g[a] - int(0.2 * mp.dim[a]) for a in range(3)], rng.uniform(0.1, 0.9, 3), mp)
    out = []
    for _ in range(n):
        end = point([centre_g[a] + int(rng.integers(-int(ext[a]), int(ext[a]) + 1)) for a in range(3)],
                    rng.uniform(0.02, 0.98, 3), mp)
        if rng.uniform() < sensor_share:
            start = [sensor[a] + rng.uniform(-0.05, 0.05) * mp.res for a in range(3)]
        else:
            start = point([centre_g[a] + int(rng.integers(-int(ext[a]), int(ext[a]) + 1)) for a in range(3)],
                          rng.uniform(0.02, 0.98, 3), mp)
        out.append((start, end))
    return out


def boundary_voxel(mp):
    """A global voxel on the x boundary between regions (0, 0, 0) and (1, 0, 0), central in y and z."""
    return [mp.dim[0], mp.dim[1] // 2, mp.dim[2] // 2]


def planted_pattern(mp, regions):
    out = {}
    for region in regions:
        tile = np.zeros(mp.volume, dtype=F)
        vi = np.arange(mp.volume)
        tile[vi % 7 == 0] = F(2.0 ** 21)
        tile[vi % 7 == 1] = F(2.0 ** 10)
        tile[vi % 7 == 2] = F(2.0 ** 17)
        out[region] = tile
    return out


# ---------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------
def tiny_sheet(kind, res, dim, flags=0, rewalk=False, tag=""):
    mp = MapParams(res, dim)
    corner = [2, 2, 2]
    maker = tiny_start_ray if kind == "tiny_start" else tiny_end_ray
    # (an end within an ulp of a wall may round into the voxel behind it: those ends are in the flags sheets)
    tinies = TINIES if kind == "tiny_start" else TINIES[:6]
    rays = tiny_rays(maker, mp, corner, tinies)
    calls = []
    for k in range(3):
        part = rays[k::3]
        first = sub_voxel_ray([corner[0] + 1, corner[1] + 1 + k, corner[2] - 1], mp)
        last = tiny_start_ray([corner[0] + 4, corner[1] + 1 + k, corner[2] - 1], 0, 1, 1e-7, mp)
        if kind == "tiny_end":
            first, last = part[0], part[-1]          # (every end of this sheet lies within 1e-7 m of a wall)
        if flags & RF_EXCLUDE_ORIGIN:
            first = part[0]                          # (an excluded origin that is also the end voxel: not defined)
        calls.append(Call(rays_array([first] + part + [last]), flags))
    return Sheet("%s/%g/%s%s" % (kind, res, "x".join(map(str, mp.dim)), tag), mp, calls, rewalk=rewalk)


def wrap_sheet(dim, filler=False, tag=""):
    mp = MapParams(FINE, dim)
    d = mp.dim
    zs = [2, d[2] // 3 + 1, (2 * d[2]) // 3 + 1, d[2] - 3]          # (one row per z slab of a tiled region)
    rows = {n: (3 + 2 * i, zs[i]) for i, n in enumerate(WRAP_COUNTS)}

    def row_ray(n):
        ly, lz = rows[n]
        return point((3, ly, lz), (0.25, 0.5, 0.5), mp), point((7, ly, lz), (0.5, 0.5, 0.5), mp)

    def fill(rays):
        if not filler:
            return rays
        out = []
        for i, ray in enumerate(rays):
            out.append(ray)
            for j in range(2):                       # two short rays along +y elsewhere in the region per wrap ray
                lx, lz = 12 + (2 * i + j) % 16, 5 + ((2 * i + j) // 16) % 4
                out.append((point((lx, 20, lz), (0.5, 0.25, 0.5), mp), point((lx, 24, lz), (0.5, 0.5, 0.5), mp)))
        return out

    planted = np.zeros(mp.volume, dtype=F)
    for n in (256, 257, 512):                        # (257 visits pass through exactly 2^32 on their way)
        for lx in range(d[0]):
            planted[mp.index((lx, rows[n][0], rows[n][1]))] = F(2.0 ** 22)
    calls = [Call(rays_array(fill([row_ray(255)] * 255 + [row_ray(256)] * 256)), 0),
             Call(rays_array(fill([row_ray(257)] * 257 + [row_ray(255)] * 255)), 0),
             Call(rays_array(fill([row_ray(512)] * 512)), 0)]
    # unequal lengths through one voxel: > 16 m in one call
    rng = np.random.default_rng([SEED, 3])
    g = (d[0] // 2 + 4, d[1] // 2 + 5, d[2] // 2)
    centre = np.array(point(g, (0.5, 0.5, 0.5), mp))
    pile = []
    for _ in range(450):
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        jitter = rng.uniform(-0.2, 0.2, 3) * mp.res
        pile.append((list(centre + jitter - v * 0.3), list(centre + jitter + v * 0.3)))
    calls.append(Call(rays_array(fill(pile)), 0))
    # (global voxel coordinates 0 ... dim - 1 are the local ones of region (0, 0, 0))
    return Sheet("wrap/%s%s" % ("x".join(map(str, d)), tag), mp, calls, {(0, 0, 0): planted})


def fold_sheet(res, dim, k, n=480, flags=0, planted=True, tag="fold", seed=0):
    mp = MapParams(res, dim)
    rng = np.random.default_rng([SEED, 5, seed])
    rays = random_rays(rng, mp, n, boundary_voxel(mp))
    per = (len(rays) + k - 1) // k
    calls = [Call(rays_array(rays[i:i + per]), flags) for i in range(0, len(rays), per)]
    plant = planted_pattern(mp, [(0, 0, 0), (1, 0, 0)]) if planted else None
    return Sheet("%s/%g/%s/%dcalls" % (tag, res, "x".join(map(str, mp.dim)), k), mp, calls, plant)


def flags_sheet(name, flags, res=0.37, dim=(20, 32, 9)):
    mp = MapParams(res, dim)
    rng = np.random.default_rng([SEED, 7, flags])
    centre = boundary_voxel(mp)
    corner = [centre[0] - 8, centre[1] - 12, centre[2] - 2]
    calls = []
    for k in range(3):
        rays = [sub_voxel_ray([corner[0] + 1, corner[1] + k, corner[2]], mp)]       # reports nothing; inherits 0
        body = random_rays(rng, mp, 120, centre)
        # degenerate rays behind long ones: zero length, sub-voxel (their share is negative)
        for j in range(0, 120, 10):
            g = [centre[0] + j // 10 - 6, centre[1] + 7, centre[2] + 1]
            p = point(g, (0.3, 0.6, 0.2), mp)
            body.insert(j + 1, (p, list(p)))
            body.insert(j + 3, sub_voxel_ray([g[0], g[1] + 1, g[2]], mp))
        rays += body
        rays += tiny_rays(tiny_start_ray, mp, corner, (2.0 ** -29, 3 * 2.0 ** -29, 1e-7, 1e-8))[k::3]
        rays += tiny_rays(tiny_end_ray, mp, [corner[0], corner[1] + 12, corner[2]], (1e-8, 3e-8, 0.0, 1e-16, ULP))[k::3]
        rays.append(tiny_start_ray([corner[0], corner[1] + k, corner[2] + 1], 0, 1, 1e-7, mp))
        if flags & RF_EXCLUDE_ORIGIN:
            # (the reference's walk is not defined for an excluded origin that is also the end voxel)
            rays = [r for r in rays if T.global_voxel(r[0], mp) != T.global_voxel(r[1], mp)]
        calls.append(Call(rays_array(rays), flags))
    return Sheet("flags/%s" % name, mp, calls)


def entry_sheet(res, dim, tag=""):
    mp = MapParams(res, dim)
    d = mp.dim
    top = [d[0], d[1], d[2]]                         # global voxel (dim, dim, dim): local (0, 0, 0) of region (1, 1, 1)
    rays = []
    corner = [wall(top[a], a, mp) for a in range(3)]  # the corner shared by regions (0,0,0) ... (1,1,1)
    span = 3.5 * mp.res
    for axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
        for offset in (0.0, 1e-8, 3e-8):
            if offset and len(axes) == 1:
                continue
            # through a point of the boundary: axes in `axes` cross their region wall there, the others stay 2.5 voxels
            # inside region 0; the offset moves the first crossing axis so the crossings come apart by a few units
            through = [corner[a] if a in axes else corner[a] - 2.5 * mp.res for a in range(3)]
            direction = np.array([1.0 if a in axes else 0.0 for a in range(3)])
            s = [through[a] - span * direction[a] for a in range(3)]
            e = [through[a] + span * direction[a] for a in range(3)]
            s[axes[0]] += offset
            e[axes[0]] += offset
            rays.append((s, e))
            rays.append((e, s))                      # and back: negative directions, into region (0, 0, 0)
    calls = [Call(rays_array(rays[0::2]), 0), Call(rays_array(rays[1::2]), 0), Call(rays_array(rays), 0)]
    return Sheet("entry/%g/%s%s" % (res, "x".join(map(str, d)), tag), mp, calls)


def corner_sheet(res, dim):
    """Rays that start within 1e-7 m of the corner shared by regions (0, 0, 0) ... (1, 1, 1) and cross it: every axis
    steps once, all within a few units of one another, so every region is entered just after the other axes' steps."""
    mp = MapParams(res, dim)
    corner = [wall(mp.dim[a], a, mp) for a in range(3)]
    rays = []
    for i, order in enumerate(itertools.permutations((1e-8, 2.5e-8, 6e-8))):
        for sgn in (1, -1):
            s = [corner[a] - sgn * order[a] for a in range(3)]
            e = [corner[a] + sgn * (0.3 + 0.02 * i) * mp.res for a in range(3)]
            rays.append((s, e))
    calls = [Call(rays_array(rays[0::2]), 0), Call(rays_array(rays[1::2]), 0)]
    return Sheet("corner/%g/%s" % (res, "x".join(map(str, mp.dim))), mp, calls)


def large_sheet(res):
    mp = MapParams(res, 16)
    rng = np.random.default_rng([SEED, 9, int(res * 100)])
    rays = random_rays(rng, mp, 200, boundary_voxel(mp))
    if res == 4.5:
        for k in range(1, 7):
            g = [3 + k, 4, 5]
            lo = [wall(g[a], a, mp) for a in range(3)]
            hi = [wall(g[a] + 1, a, mp) for a in range(3)]
            s = [lo[a] + (a + 1) * k * 1e-9 for a in range(3)]
            e = [hi[a] + (3 - a) * k * 1e-9 for a in range(3)]
            rays.append((s, e))
    calls = [Call(rays_array(rays[0::2]), 0), Call(rays_array(rays[1::2]), 0)]
    return Sheet("large/%g" % res, mp, calls, planted_pattern(mp, [(0, 0, 0)]))


def stop_sheet():
    mp = MapParams(0.1, 32)
    rng = np.random.default_rng([SEED, 13])
    occ = np.full(mp.volume, F(np.inf), dtype=F)
    for ly in range(32):
        for lz in range(32):
            occ[mp.index((20, ly, lz))] = F(2.0)
    calls = []
    for k in range(3):
        rays = []
        for _ in range(200):
            s = point((5, 16, 16), rng.uniform(0.1, 0.9, 3), mp)
            e = point((int(rng.integers(10, 30)), int(rng.integers(6, 27)), int(rng.integers(6, 27))),
                      rng.uniform(0.02, 0.98, 3), mp)
            rays.append((s, e))
        calls.append(Call(rays_array(rays), RF_STOP_ON_FIRST_OCCUPIED))
    return Sheet("stop/wall", mp, calls, {(0, 0, 0): np.zeros(mp.volume, dtype=F)}, {(0, 0, 0): occ})


# ---------------------------------------------------------------------------------------------------------------------
# sites
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _common():
    return dict(
        tiny=_cached("tiny", lambda: tiny_sheet("tiny_start", FINE, 32)),
        tiny01=_cached("tiny01", lambda: tiny_sheet("tiny_start", 0.1, 32)),
        tiny_end=_cached("tiny_end", lambda: tiny_sheet("tiny_end", FINE, 32, RF_END_POINT_AS_FREE)),
        tiny_origin=_cached("tiny_origin", lambda: tiny_sheet("tiny_start", FINE, 32, RF_END_POINT_AS_FREE |
                                                              RF_EXCLUDE_ORIGIN, tag="/exclude_origin")),
        wrap=_cached("wrap", lambda: wrap_sheet(32)),
        entry=_cached("entry", lambda: entry_sheet(FINE, 32)),
        entry01=_cached("entry01", lambda: entry_sheet(0.1, 32)),
        corner=_cached("corner", lambda: corner_sheet(FINE, 32)),
        fold={k: _cached(("fold", k), lambda k=k: fold_sheet(0.1, 32, k)) for k in (1, 2, 3, 6)},
    )


def build(site):
    """The sheets of one site (cached: sites share sheets)."""
    c = _common()
    if site == "direct":
        out = [c[n] for n in ("tiny", "tiny01", "tiny_end", "tiny_origin", "corner", "wrap", "entry", "entry01")]
        out += list(c["fold"].values())
        out += [_cached(("flags", n), lambda n=n, f=f: flags_sheet(n, f)) for n, f in FLAG_SETS.items()]
        out += [_cached(("flags037", 0), lambda: flags_sheet("none", 0))]
        out += [_cached(("large", r), lambda r=r: large_sheet(r)) for r in (4.5, 4.75, 10.0)]
        return out
    if site == "chunks":
        return [_cached("wrap_filler", lambda: wrap_sheet(32, filler=True, tag="/filler"))] + [
            _cached(("fold2400", k), lambda k=k: fold_sheet(0.1, 32, k, n=2400, tag="fold2400", seed=1))
            for k in (1, 3)]
    if site == "mean":
        return [c["tiny"], c["tiny_end"], c["tiny_origin"], c["corner"], c["wrap"], c["entry"], c["fold"][3],
                _cached(("flags", "end_as_free_exclude_origin"),
                        lambda: flags_sheet("end_as_free_exclude_origin", FLAG_SETS["end_as_free_exclude_origin"])),
                _cached(("flags037", 0), lambda: flags_sheet("none", 0))]
    if site == "stop":
        return [_cached("stop", stop_sheet)]
    if site == "ndt":
        return [c["tiny"], c["tiny01"], c["corner"], c["wrap"], c["entry"], c["fold"][3],
                _cached(("large", 4.5), lambda: large_sheet(4.5))]
    if site == "rewalk":
        return [_cached("tiny_rewalk", lambda: tiny_sheet("tiny_start", FINE, 32, rewalk=True, tag="/rewalk")),
                _cached("fold_rewalk", lambda: _rewalk(fold_sheet(0.1, 32, 3, tag="fold_rewalk")))]
    if site == "tiled":
        return [_cached("tiny48", lambda: tiny_sheet("tiny_start", FINE, 48)),
                _cached("wrap48", lambda: wrap_sheet(48)),
                _cached("entry48", lambda: entry_sheet(FINE, 48)),
                _cached("corner48", lambda: corner_sheet(FINE, 48)),
                _cached("fold48", lambda: fold_sheet(0.1, 48, 3))]
    if site == "spill":
        return [c["tiny"], c["wrap"], c["fold"][6]]
    raise KeyError(site)


def occupancy_tile(sheet, region):
    """The occupancy a planted region is uploaded with: unobserved, but for a planted wall."""
    if sheet.planted_occupancy and region in sheet.planted_occupancy:
        return sheet.planted_occupancy[region]
    return np.full(sheet.mp.volume, F(np.inf), dtype=F)


def make_oracle(sheet, layers, ndt=None):
    """An OracleMap of the sheet's geometry holding its planted regions (every other layer cleared)."""
    from oracle.oracle import LAYER_DTYPES, OracleMap
    mp = sheet.mp
    om = OracleMap(mp.res, mp.dim, layers)
    if ndt is not None:
        om.set_ndt(**ndt)
    for region, tile in sheet.planted.items():
        c = [T.voxel_centre_axis(region[a] * mp.dim[a] + mp.dim[a] // 2, a, mp) for a in range(3)]
        om.integrate_occupancy(np.array([c, c]))                 # creates the region; overwritten next
        for name in layers:
            view = om.region_layer_view(region, name)
            view[:] = np.zeros(1, dtype=LAYER_DTYPES[name][0])
        om.region_layer_view(region, "occupancy")[:] = occupancy_tile(sheet, region)
        om.region_layer_view(region, "traversal")[:] = tile
    return om


def _rewalk(sheet):
    sheet.rewalk = True
    return sheet


def all_sheets():
    """Every distinct sheet, with the sites that use it."""
    out = {}
    for site in SITES:
        for sheet in build(site):
            out.setdefault(id(sheet), (sheet, []))[1].append(site)
    return list(out.values())
