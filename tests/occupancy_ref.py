"""The occupancy log-odds update's exact model (test infrastructure): tests/test_occupancy_ref.py (CPU) ties it to
exact rational arithmetic, to the CPU oracle and to the reference header; tests/test_gpu_occupancy_states.py (-m gpu)
holds the device to it bit for bit on the sheets of tests/occupancy_cases.py.

The rule (ohm/VoxelOccupancyCompute.h:44-54, 110-120; the flag selects of ohm/RayMapperOccupancy.cpp:143-163, 261-281).
A voxel holds a float32 x; +inf means never observed.  One event -- a miss or a hit -- is, one IEEE float32 operation
at a time:

  unobserved = x == +inf
  free       = not unobserved and x <  threshold          (classified on x BEFORE the operation)
  occupied   = not unobserved and x >= threshold
  adj        = miss (or hit)
  adj        = +inf if unobserved and kRfExcludeUnobserved
  adj        = 0.0  if free       and kRfExcludeFree
  adj        = 0.0  if occupied   and kRfExcludeOccupied
  base       = x    if null_update or not unobserved else 0.0
  adj        = adj  if not null_update and (unobserved or sat_lo < x < sat_hi) else 0.0
  x'         = base if base == +inf else fmax(min, base + adj)        (a hit: fmin(base + adj, max))

with (sat_lo, sat_hi) the OPEN interval (min, max), either end replaced by lowest() / max() of float32 where that
side's saturation is off, and fmax / fmin those of C: where one operand is a NaN the other one wins.  Nothing else
happens to a voxel; in particular x' is stored whether or not it compares equal to x, so a -0.0 that receives a zero
adjustment becomes +0.0 (-0.0 + 0.0 is +0.0), a NaN becomes min (or max), and a null update still clamps.
(Adjustments of -0.0 are outside the model: fmax(+0.0, -0.0) is not defined by C.)

integrate() is the sequential mapper: ray by ray in submission order, voxel by voxel in walk order
(traversal_ref.visits); every visited voxel gets a miss, a null one once the ray has met an occupied voxel under
kRfStopOnFirstOccupied (the stopping voxel itself still gets its miss); then the sample's voxel gets a hit unless the
ray was stopped, the end point was walked (kRfEndPointAsFree) or kRfExcludeSample / kRfExcludeRay say otherwise.  The
configuration (Config) is given per call.

MUTANTS are one-line changes of the model; the CPU test asserts that the sheets tell each of them from the model."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

import traversal_ref as T
from traversal_ref import (F, RF_END_POINT_AS_FREE, RF_EXCLUDE_RAY, RF_EXCLUDE_SAMPLE,  # noqa: F401
                           RF_STOP_ON_FIRST_OCCUPIED)
from tsdf_ref import round_f32

RF_EXCLUDE_UNOBSERVED = 1 << 5
RF_EXCLUDE_FREE = 1 << 6
RF_EXCLUDE_OCCUPIED = 1 << 7
VALUE_FLAGS = (RF_EXCLUDE_UNOBSERVED, RF_EXCLUDE_FREE, RF_EXCLUDE_OCCUPIED)
VALUE_FLAG_SUBSETS = tuple(sum(f for i, f in enumerate(VALUE_FLAGS) if s >> i & 1) for s in range(8))

INF = F(np.inf)
LOWEST, FLT_MAX = F(-3.4028234663852886e38), F(3.4028234663852886e38)

OP_MUTANTS = ("sat_closed", "threshold_strict", "classify_after_update", "unobserved_keeps_inf_base", "clamp_then_add",
              "nan_propagates", "zero_sign_kept", "null_update_adjusts")
RUN_MUTANTS = ("n_misses_as_one_product", "misses_all_before_hits", "trailing_misses_dropped", "count_mod_2_15",
               "count_mod_2_16")
STOP_MUTANTS = ("stop_voxel_skips_its_miss", "stopped_ray_keeps_sample", "stop_judged_after_miss")
MUTANTS = OP_MUTANTS + RUN_MUTANTS + STOP_MUTANTS + ("config_of_previous_call",)

Config = namedtuple("Config", "hit miss threshold min_value max_value sat_min sat_max")


def config(hit, miss, threshold, min_value, max_value, sat_min=False, sat_max=False):
    return Config(F(hit), F(miss), F(threshold), F(min_value), F(max_value), bool(sat_min), bool(sat_max))


def window(cfg):
    """The open saturation interval."""
    return (cfg.min_value if cfg.sat_min else LOWEST), (cfg.max_value if cfg.sat_max else FLT_MAX)


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _add32(a, b):
    with np.errstate(all="ignore"):
        return F(F(a) + F(b))


def _add_exact(a, b):
    """a + b in rational arithmetic, rounded once (tsdf_ref.round_f32); IEEE's rules where they are not arithmetic."""
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)) or Fraction(a) + Fraction(b) == 0:
        with np.errstate(all="ignore"):
            return F(np.float64(a) + np.float64(b))    # inf, NaN, the sign of an exact zero sum: the same at any width
    return F(round_f32(Fraction(a) + Fraction(b)))


def selected(cfg, x, flags, hit):
    """The adjustment the mapper hands to occupancyAdjustHit / Miss: the value-exclusion selects alone."""
    x = F(x)
    adj = cfg.hit if hit else cfg.miss
    unobserved = x == INF
    adj = INF if unobserved and flags & RF_EXCLUDE_UNOBSERVED else adj
    adj = F(0.0) if not unobserved and x < cfg.threshold and flags & RF_EXCLUDE_FREE else adj
    return F(0.0) if not unobserved and x >= cfg.threshold and flags & RF_EXCLUDE_OCCUPIED else adj


def adjust(cfg, x, flags, hit, null_update=False, mutant=None, add=_add32):
    """One event on a voxel that holds x."""
    x = F(x)
    lo, hi = window(cfg)
    adj = cfg.hit if hit else cfg.miss
    clamp = (lambda v: _fmin(v, cfg.max_value)) if hit else (lambda v: _fmax(cfg.min_value, v))
    if mutant == "nan_propagates":
        inner = clamp
        clamp = lambda v: v if v != v else inner(v)  # noqa: E731  (std::min / std::max keep a NaN in this position)
    if mutant == "null_update_adjusts":
        null_update = False
    unobserved = x == INF
    judged = x
    if mutant == "classify_after_update" and not unobserved:
        judged = clamp(add(x, adj))
    free = not unobserved and judged < cfg.threshold
    occupied = not unobserved and (judged > cfg.threshold if mutant == "threshold_strict" else judged >= cfg.threshold)
    adj = INF if unobserved and flags & RF_EXCLUDE_UNOBSERVED else adj
    adj = F(0.0) if free and flags & RF_EXCLUDE_FREE else adj
    adj = F(0.0) if occupied and flags & RF_EXCLUDE_OCCUPIED else adj
    base = x if (null_update or not unobserved or mutant == "unobserved_keeps_inf_base") else F(0.0)
    inside = (lo <= x <= hi) if mutant == "sat_closed" else (lo < x < hi)
    adj = adj if (not null_update and (unobserved or inside)) else F(0.0)
    if base == INF:
        return base
    out = add(clamp(base), adj) if mutant == "clamp_then_add" else clamp(add(base, adj))
    if mutant == "zero_sign_kept" and out == x:
        return x
    return F(out)


def adjust_miss(cfg, x, flags=0, null_update=False, mutant=None):
    return adjust(cfg, x, flags, False, null_update, mutant)


def adjust_hit(cfg, x, flags=0, null_update=False, mutant=None):
    return adjust(cfg, x, flags, True, null_update, mutant)


def adjust_exact(cfg, x, flags, hit, null_update=False):
    """The same expression with its one arithmetic operation evaluated in fractions.Fraction and rounded once."""
    return adjust(cfg, x, flags, hit, null_update, add=_add_exact)


# ---------------------------------------------------------------------------------------------------------------------
# the sequential mapper
# ---------------------------------------------------------------------------------------------------------------------
Call = namedtuple("Call", "rays flags cfg")
Event = namedtuple("Event", "key kind ray")                  # kind: "m" miss, "n" null update, "h" hit

_VISITS = {}


def cached_visits(start, end, flags, mp):
    """traversal_ref.visits, remembered per ray: the sheets send the same few rays many times."""
    walk_flags = flags & (T.RF_END_POINT_AS_FREE | T.RF_EXCLUDE_ORIGIN | T.RF_EXCLUDE_RAY)
    key = (mp.res, mp.dim, mp.origin, tuple(start), tuple(end), walk_flags)
    if key not in _VISITS:
        v = T.visits(start, end, walk_flags, mp)
        sample = T.global_voxel(end, mp)
        _VISITS[key] = (tuple(v.keys), None if sample is None else T.key_of(sample, mp))
    return _VISITS[key]


class State:
    """Occupancy of every region a sheet planted or touched: {region: float32[volume]}, +inf where never observed."""

    def __init__(self, mp, planted=None):
        self.mp = mp
        self.tiles = {r: np.array(t, dtype=F, copy=True) for r, t in (planted or {}).items()}

    def get(self, key):
        tile = self.tiles.get(key[0])
        return INF if tile is None else tile[key[1]]

    def set(self, key, value):
        if key[0] not in self.tiles:
            self.tiles[key[0]] = np.full(self.mp.volume, INF, dtype=F)
        self.tiles[key[0]][key[1]] = value

    def copy(self):
        return {r: t.copy() for r, t in self.tiles.items()}


def occupied(cfg, x, mutant=None):
    return x != INF and (x > cfg.threshold if mutant == "threshold_strict" else x >= cfg.threshold)


def integrate(state, call, mp, mutant=None, events=None):
    """One integrateRays call on `state` (updated in place).  `events`, a list, receives the call's Events in order."""
    cfg, flags = call.cfg, int(call.flags)
    rays = np.asarray(call.rays, dtype=np.float64)
    op_mutant = mutant if mutant in OP_MUTANTS else None
    log = [] if (events is None and mutant in RUN_MUTANTS) else events
    before = State(mp, state.tiles) if mutant in RUN_MUTANTS else None
    stop_flag = bool(flags & RF_STOP_ON_FIRST_OCCUPIED)
    sample_in_ray = bool(flags & RF_END_POINT_AS_FREE)
    for r in range(rays.shape[0] // 2):
        keys, sample = cached_visits(rays[2 * r], rays[2 * r + 1], flags, mp)
        stopped = False
        for key in keys:
            x = state.get(key)
            null = stopped
            was = occupied(cfg, x, mutant)
            if mutant == "stop_voxel_skips_its_miss" and stop_flag and was:
                null = True
            state.set(key, adjust(cfg, x, flags, False, null, op_mutant))
            if mutant == "stop_judged_after_miss":
                was = occupied(cfg, state.get(key), mutant)
            stopped = stopped or (stop_flag and was)
            if log is not None:
                log.append(Event(key, "n" if null else "m", r))
        keeps = not stopped or mutant == "stopped_ray_keeps_sample"
        if keeps and not sample_in_ray and not flags & (RF_EXCLUDE_SAMPLE | RF_EXCLUDE_RAY) and sample is not None:
            state.set(sample, adjust(cfg, state.get(sample), flags, True, False, op_mutant))
            if log is not None:
                log.append(Event(sample, "h", r))
    if mutant in RUN_MUTANTS:
        _rerun(state, before, log, cfg, flags, mutant)
    return state


def patterns_of(events):
    """{voxel key: its events of one call as a string, e.g. "mmhm"}."""
    out = {}
    for e in events:
        out.setdefault(e.key, []).append(e.kind)
    return {k: "".join(v) for k, v in out.items()}


def _rerun(state, before, events, cfg, flags, mutant):
    """The mutants that see a voxel's events as runs of misses between hits, as a counting implementation does: every
    voxel of the call again from its value before the call (the voxels of a call without kRfStopOnFirstOccupied do not
    depend on one another)."""
    for key, pattern in patterns_of(events).items():
        x = before.get(key)
        if mutant == "misses_all_before_hits":
            pattern = "".join(sorted(pattern, key=lambda c: c != "m"))
        runs = pattern.split("h")                          # misses before each hit, then the trailing ones
        for i, run in enumerate(runs):
            n = len(run)
            last = i == len(runs) - 1
            if mutant == "trailing_misses_dropped" and last and len(runs) > 1:
                n = 0
            if mutant == "count_mod_2_15":
                n %= 1 << 15
            if mutant == "count_mod_2_16":
                n %= 1 << 16
            if mutant == "n_misses_as_one_product" and n > 1:
                x = adjust(cfg._replace(miss=F(F(n) * cfg.miss)), x, flags, False)
                n = 0
            for _ in range(n):
                nx = adjust(cfg, x, flags, False)
                if bits(nx) == bits(x):
                    break                                  # a fixed point: the remaining misses are the identity
                x = nx
            if not last:
                x = adjust(cfg, x, flags, True)
        state.set(key, x)


def replay(planted, calls, mp, mutant=None, events=None):
    """The states after every call: [{region: float32[volume]}]."""
    state = State(mp, planted)
    out = []
    for k, call in enumerate(calls):
        if mutant == "config_of_previous_call" and k > 0:
            call = call._replace(cfg=calls[k - 1].cfg)
        log = None if events is None else []
        integrate(state, call, mp, mutant, log)
        out.append(state.copy())
        if events is not None:
            events.append(log)
    return out
