"""Seeded single-voxel NDT states and event scripts (test infrastructure) for tests/ndt_ref.py.

A case is a full voxel state (value, factor, packed mean, count, and for NDT-TM the intensity pair and the hit / miss
counts), a script of events on that voxel in ray order (H: a sample in it, M: a ray through it) and the mapper
parameters of the configuration it belongs to.  States are planted, not integrated; the random room scans of the other
NDT tests do not steer the per-voxel state machine, these do, one edge per family.

Placement.  Targets sit four voxels apart in region (0, 0, 0) of a map with 0.2 m voxels: a 32^3 region at the origin,
and a 24 x 40 x 20 region with the origin at (0.0625)^3.  Most rays are shorter than three voxels; some come from 3 m
and 30 m.  Every ray is walked with OracleMap.walk and kept only if the one target it touches is its own and it touches
it the way its event says (H: the sample lies in it; M: it is walked as a ray voxel).  A region holds 512 (300) targets,
so the cases of a configuration are dealt onto sheets, each sheet one map.

Gaps are SOLVED: for the families that put a decision next to eta = adaptation_rate / 2, one coordinate of the sensor
(misses) or of the sample (NDT-TM hits) is bisected in mpmath until the exact product sits at eta (1 +- g); the fp64
rounding of that coordinate moves the gap by parts in 1e12, so the achieved gap is recomputed and must fall in
[g / 2, 2 g] on the wanted side.  Cases the model finds inside a decision band (ndt_ref.Ambiguous) are regenerated and
counted; the CPU test bounds their share.

A miss needs the voxel walked as a ray voxel, so its sample lies beyond the voxel -- or, where the clip filter cuts the
ray, possibly inside it: a clipped end point is walked as free space (ohm/RayMapperNdt.cpp:269-270).  That is the one
way a miss has its sample inside the voxel without kRfEndPointAsFree; a sample short of the voxel never reaches it."""
import ctypes as C
import functools
from dataclasses import dataclass, field

import numpy as np

import ndt_ref
from ndt_ref import MP, Ambiguous, Params, State, mpf
from oracle.oracle import OracleMap, lib as _olib

RES = 0.2
HALF = 0.1
SEED = 20240611
GAPS = (1e-6, 1e-4, 1e-2)
RF_EXCLUDE_RAY = 1 << 4


def _value(p):
    return float(_olib.oracle_probability_to_value(p))


_BASE = dict(resolution=RES, hit_value=_value(0.9), miss_value=_value(0.45), min_value=-2.0, max_value=3.511,
             reinit_threshold=_value(0.2))

# name -> (Params, region dimensions, origin, (filter mode, range), ray flags)
CONFIGS = {
    # defaults of the NDT map, with a sensor noise wide enough for p_s to matter on short rays
    "A": (Params(**_BASE, sensor_noise=0.1, sample_threshold=3, adaptation_rate=0.2, reinit_count=100, ndt_tm=True),
          (32, 32, 32), (0.0, 0.0, 0.0), ("good", 1e10), 0),
    # full adaptation (p reaches 0), both saturations, the clip filter, a re-initialisation count that an upload reaches
    "B": (Params(**_BASE, sensor_noise=0.05, sample_threshold=4, adaptation_rate=1.0, reinit_count=5,
                 saturate_at_min=True, saturate_at_max=True, initial_intensity_cov=0.25, ndt_tm=True),
          (24, 40, 20), (0.0625, 0.0625, 0.0625), ("clip", 2.5), 0),
    # scripts that re-initialise by integration: no saturation (a saturated voxel never moves again), NDT-OM layers only
    "C": (Params(**_BASE, sensor_noise=0.05, sample_threshold=3, adaptation_rate=1.0, reinit_count=5, ndt_tm=False),
          (32, 32, 32), (0.0, 0.0, 0.0), ("good", 1e10), 0),
    # the sensor noise whose float32 square is rounded the most (0.99 * 2^-24 relative) and no clamp in reach, so that
    # a log-odds adjustment of -15.95 ... -15.3 (full adaptation, ray through the mean) shows a variance formed in fp64
    "E": (Params(**dict(_BASE, min_value=-1000.0), sensor_noise=0.04425, sample_threshold=3, adaptation_rate=1.0,
                 reinit_count=100, ndt_tm=True),
          (32, 32, 32), (0.0, 0.0, 0.0), ("good", 1e10), 0),
    # samples only (kRfExcludeRay)
    "D": (Params(**_BASE, sensor_noise=0.1, sample_threshold=3, adaptation_rate=0.2, reinit_count=100, ndt_tm=True),
          (32, 32, 32), (0.0, 0.0, 0.0), ("good", 1e10), RF_EXCLUDE_RAY),
}


@dataclass
class Case:
    family: str
    cell: tuple
    config: str
    state: State
    events: list                      # (kind, sensor fp64[3], sample fp64[3], intensity) as the mapper receives them
    local: tuple = None               # the target voxel, set at placement
    model_events: list = None         # the same events with the sample the maths sees (after the clip filter)
    wanted_gap: float = None          # signed, relative to eta
    factor_bar: str = "ulp"           # "ulp" | "1e-6"


@dataclass
class Sheet:
    config: str
    cases: list = field(default_factory=list)


class Geometry:
    """The voxel grid of one configuration, asked of the oracle's key maths and line walk."""

    def __init__(self, name):
        self.name = name
        self.prm, self.region, self.origin, self.ray_filter, self.flags = CONFIGS[name]
        self.om = OracleMap(RES, self.region, ["occupancy"])
        self.om.set_origin(self.origin)
        self.targets = [(x, y, z) for z in range(2, self.region[2], 4) for y in range(2, self.region[1], 4)
                        for x in range(2, self.region[0], 4)]
        self.target_set = set(self.targets)

    def centre(self, local):
        return np.array(self.om.voxel_centre((0, 0, 0), local), dtype=np.float64)

    def index(self, local):
        return local[0] + self.region[0] * (local[1] + self.region[1] * local[2])

    def filtered(self, sensor, sample):
        """(sample the maths sees, clipped?) -- clipRayFilter in fp64, operation by operation (ohm/RayFilter.cpp:37-57)."""
        mode, rng = self.ray_filter
        if mode != "clip":
            return sample, False
        ray = sample - sensor
        l2 = (ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2]
        if not l2 > rng * rng:
            return sample, False
        ray = ray / np.sqrt(l2)
        return sensor + ray * rng, True

    def accepts(self, local, kind, sensor, sample):
        """The ray touches no target but `local`, and touches it the way `kind` says."""
        end, clipped = self.filtered(sensor, sample)
        keys, _, _ = self.om.walk(sensor, end)
        touched = {k[1] for k in keys if k[0] == (0, 0, 0)} & self.target_set
        if touched != {tuple(local)}:
            return False
        end_key = self.om.voxel_key(end)
        ends_here = end_key == ((0, 0, 0), tuple(local))
        if kind == "H":
            return ends_here and not clipped
        return clipped or not ends_here


@functools.lru_cache(maxsize=None)
def geometry(name):
    return Geometry(name)


# ---------------------------------------------------------------------------------------------------------------------
# state and ray construction (centre-relative: placement adds the voxel centre, which is why constructed gaps are
# re-solved per target -- the bisection runs on the placed voxel)
# ---------------------------------------------------------------------------------------------------------------------
def f32(x):
    return float(np.float32(x))


def pack_mean(offset):
    return int(_olib.oracle_sub_voxel_coord((C.c_double * 3)(*[float(v) for v in offset]), RES))


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def random_factor(rng, lo=-4.0, hi=-1.0, shape="general"):
    d = 10.0 ** rng.uniform(lo, hi, size=3)
    if shape == "planar":                      # one diagonal 1e-4 of the others
        big = 10.0 ** rng.uniform(-2.0, -1.0)
        d = np.array([big, big * rng.uniform(0.5, 1.0), big * rng.uniform(0.5, 1.0)])
        d[rng.integers(3)] = big * 1e-4
    elif shape == "rod":                       # two diagonals 1e-3 of the third
        big = 10.0 ** rng.uniform(-2.0, -1.0)
        d = np.full(3, big * 1e-3) * rng.uniform(0.5, 1.0, size=3)
        d[rng.integers(3)] = big
    o = rng.uniform(-0.5, 0.5, size=3)
    return (f32(d[0]), f32(o[0] * np.sqrt(d[0] * d[1])), f32(d[1]), f32(o[1] * np.sqrt(d[0] * d[2])),
            f32(o[2] * np.sqrt(d[1] * d[2])), f32(d[2]))


def random_state(rng, prm, shape="general", lo=-4.0, hi=-1.0, **over):
    st = dict(value=np.float32(rng.uniform(-1.9, 3.0)), cov=random_factor(rng, lo, hi, shape),
              coord=pack_mean(rng.uniform(-0.03, 0.03, size=3)), count=int(rng.integers(prm.sample_threshold, 60)),
              intensity=(f32(rng.uniform(0, 50)), f32(rng.uniform(0.01, 4))),
              hit_miss=(int(rng.integers(0, 200)), int(rng.integers(0, 200))))
    st.update(over)
    return State(**st)


def factor_matrix(cov):
    return np.array([[cov[0], 0, 0], [cov[1], cov[2], 0], [cov[3], cov[4], cov[5]]], dtype=np.float64)


def inside(point, centre, margin=0.01):
    return bool(np.all(np.abs(point - centre) < HALF - margin))


def through_point(rng, state, centre, mahal):
    """A point of the voxel at Mahalanobis distance <= mahal from the mean (pulled in until it is inside)."""
    mean = ndt_ref.voxel_mean(state.coord, centre, RES)
    step = factor_matrix(state.cov) @ (unit(rng) * mahal)
    for _ in range(60):
        if inside(mean + step, centre):
            break
        step = step * 0.7
    return mean + step


def exit_distance(q, d, centre):
    """Distance from q (inside the voxel) along d to the voxel's wall."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d > 0, (centre + HALF - q) / d, np.where(d < 0, (centre - HALF - q) / d, np.inf))
    return float(np.min(t))


def miss_ray(rng, state, centre, mahal, near="short", far="short", beyond=None):
    q = through_point(rng, state, centre, mahal)
    d = unit(rng)
    back = exit_distance(q, -d, centre)
    fwd = exit_distance(q, d, centre)
    if beyond is not None:
        return q - d * (back + rng.uniform(0.02, 0.15)), q + d * beyond
    a = {"short": back + rng.uniform(0.02, 0.15), "inside": back * rng.uniform(0.1, 0.9), "3m": 3.0, "30m": 30.0}[near]
    b = {"short": fwd + rng.uniform(0.05, 0.15), "wall": fwd + rng.uniform(1e-3, 0.02), "far": fwd + 2.0,
         "beyond_clip": 4.0}[far]
    return q - d * a, q + d * b


def hit_ray(rng, centre, sample, near="short"):
    d = unit(rng)
    a = {"short": rng.uniform(0.25, 0.5), "3m": 3.0, "30m": 30.0}[near]
    return sample - d * a, sample


def near_mode(i):
    """A few per family from 3 m and 30 m."""
    return {7: "3m", 15: "30m", 23: "3m", 31: "30m"}.get(i % 32, "short")


def _bisect(f, lo, hi):
    """Root of f between lo and hi (mpf), f(lo) > 0 > f(hi)."""
    lo, hi = mpf(lo), mpf(hi)
    for _ in range(90):
        mid = (lo + hi) / 2
        if f(mid) > 0:
            lo = mid
        else:
            hi = mid
    return float((lo + hi) / 2)


# ---------------------------------------------------------------------------------------------------------------------
# families: each yields (cell, builder); builder(rng, geo, centre, i) -> (state, events, extras) or None to redraw
# ---------------------------------------------------------------------------------------------------------------------
def _m(sensor, sample):
    return ("M", sensor, sample, 0.0)


def _h(sensor, sample, intensity=0.0):
    return ("H", sensor, sample, f32(intensity))


def fam_m_general(shape, config):
    def build(rng, geo, centre, i):
        st = random_state(rng, geo.prm, shape)
        return st, [_m(*miss_ray(rng, st, centre, rng.uniform(0, 3), near_mode(i) if config == "A" else "short"))], {}
    return build


def fam_m_gap(side, g):
    def build(rng, geo, centre, i):
        prm = geo.prm
        st = random_state(rng, prm, lo=-2.6, hi=-1.8)
        sensor, sample = miss_ray(rng, st, centre, 0.0)          # through the mean: prod ~ 1 - p_s > eta
        axis = int(np.argmin(np.abs(sample - sensor)))           # move the sensor across the ray
        mean = ndt_ref.voxel_mean(st.coord, centre, RES)
        eta = mpf(f32(prm.adaptation_rate)) / 2
        want = eta * (1 + side * mpf(g))

        def f(s):
            moved = [mpf(float(v)) for v in sensor]
            moved[axis] += s
            p_v, p_s = ndt_ref.likelihoods(prm, st.cov, mean, moved, sample)
            return p_v * (1 - p_s) - want
        if not (f(0) > 0 > f(mpf("0.12"))):
            return None
        sensor = sensor.copy()
        sensor[axis] += _bisect(f, 0, "0.12")
        return st, [_m(sensor, sample)], dict(wanted_gap=side * g)
    return build


def fam_m_prod0(rng, geo, centre, i):
    """The ray's closest approach to the mean is 14 sigma (its direction is orthogonal to the offset in the factor's
    own coordinates): p_v = e^-98, delta underflows to 0 in fp64 and is below 1e-40 exactly."""
    st = random_state(rng, geo.prm, lo=-3.0, hi=-2.5)
    big = factor_matrix(st.cov)
    w = unit(rng)
    v = np.cross(w, unit(rng))
    q = ndt_ref.voxel_mean(st.coord, centre, RES) + big @ (w * 14.0)
    d = big @ v
    d = d / np.linalg.norm(d)
    if not inside(q, centre):
        return None
    return st, [_m(q - d * (exit_distance(q, -d, centre) + rng.uniform(0.02, 0.15)),
                   q + d * (exit_distance(q, d, centre) + rng.uniform(0.05, 0.15)))], {}


def fam_m_through_mean(rng, geo, centre, i):
    st = random_state(rng, geo.prm, value=np.float32(rng.uniform(-1.5, 3.0)))
    return st, [_m(*miss_ray(rng, st, centre, 0.0, far="far"))], {}


def fam_m_variance(rng, geo, centre, i):
    """Ray through the mean (p_v = 1) under full adaptation: p = p_s / 2 and delta = -E - ln 2 with E = d^2 / (2 sigma^2)
    the exponent of p_s.  E in 14.6 ... 15.25 puts |delta| at the top of the binade [8, 16), where a relative error e of
    sigma^2 moves delta by E e: 0.93 float32 ulp for the 5.9e-8 between the float32 product and the fp64 one.  Not
    further out: p = 1/2 - eta p_v (1 - p_s) is formed in fp64 with an absolute error of 2^-53, which is 2^-53 / p of
    delta -- 2e-9 here, but more than an ulp of delta from p ~ 1e-10 on (measured: 78 ulp at p = 1.5e-14).  That is the
    reference's own cancellation; with the default clamps every such voxel ends on min_value."""
    st = random_state(rng, geo.prm, value=np.float32(rng.uniform(-1.5, 3.0)))
    sigma = float(geo.prm.f32("sensor_noise"))
    return st, [_m(*miss_ray(rng, st, centre, 0.0, beyond=sigma * np.sqrt(2.0 * rng.uniform(14.6, 15.25))))], {}


def fam_m_unobserved(rng, geo, centre, i):
    st = random_state(rng, geo.prm, value=np.float32(np.inf))
    return st, [_m(*miss_ray(rng, st, centre, rng.uniform(0, 2)))], {}


def fam_m_count_edge(delta):
    def build(rng, geo, centre, i):
        st = random_state(rng, geo.prm, count=geo.prm.sample_threshold + delta)
        return st, [_m(*miss_ray(rng, st, centre, rng.uniform(0, 2)))], {}
    return build


def fam_m_at_min(which):
    def build(rng, geo, centre, i):
        lo = np.float32(geo.prm.min_value)
        value = {"on": lo, "above": np.nextafter(lo, np.float32(0)), "below": np.nextafter(lo, np.float32(-10)),
                 "far_below": np.float32(lo - 0.75)}[which]
        st = random_state(rng, geo.prm, value=value)
        return st, [_m(*miss_ray(rng, st, centre, rng.uniform(0, 2)))], {}
    return build


def fam_m_at_max(which):
    def build(rng, geo, centre, i):
        hi = np.float32(geo.prm.max_value)
        value = {"on": hi, "above": np.float32(hi + 1.0), "below": np.nextafter(hi, np.float32(0))}[which]
        st = random_state(rng, geo.prm, value=value)
        return st, [_m(*miss_ray(rng, st, centre, rng.uniform(0, 1)))], {}
    return build


def fam_m_zero_diag(position):
    def build(rng, geo, centre, i):
        cov = list(random_factor(rng))
        cov[(0, 2, 5)[position]] = 0.0
        st = random_state(rng, geo.prm, cov=tuple(cov))
        q = centre + rng.uniform(-0.08, 0.08, size=3)
        d = unit(rng)
        return st, [_m(q - d * (exit_distance(q, -d, centre) + 0.05), q + d * (exit_distance(q, d, centre) + 0.1))], {}
    return build


def fam_m_sensor_inside(rng, geo, centre, i):
    st = random_state(rng, geo.prm)
    return st, [_m(*miss_ray(rng, st, centre, rng.uniform(0, 2), near="inside"))], {}


def fam_m_sample_wall(rng, geo, centre, i):
    st = random_state(rng, geo.prm)
    return st, [_m(*miss_ray(rng, st, centre, rng.uniform(0, 2), far="wall"))], {}


def fam_m_clip(where):
    def build(rng, geo, centre, i):
        st = random_state(rng, geo.prm)
        if where == "moved":                       # the clip filter moves a sample that lay beyond the voxel anyway
            sensor, sample = miss_ray(rng, st, centre, rng.uniform(0, 2), far="beyond_clip")
            end, clipped = geo.filtered(sensor, sample)
            return (st, [_m(sensor, sample)], {}) if clipped and not inside(end, centre, -0.005) else None
        # "end_inside": the clipped end point lies inside the voxel, which is still walked as a ray voxel
        q = through_point(rng, st, centre, rng.uniform(0, 2))
        d = unit(rng)
        sensor = q - d * (geo.ray_filter[1] - rng.uniform(0.0, 0.5) * exit_distance(q, d, centre))
        sample = q + d * 3.0
        end, clipped = geo.filtered(sensor, sample)
        return (st, [_m(sensor, sample)], {}) if clipped and inside(end, centre) else None
    return build


def fam_h_general(shape):
    def build(rng, geo, centre, i):
        st = random_state(rng, geo.prm, shape)
        sample = centre + rng.uniform(-0.095, 0.095, size=3)
        return st, [_h(*hit_ray(rng, centre, sample, near_mode(i)), rng.uniform(0, 60))], {}
    return build


def fam_h_count0(which):
    def build(rng, geo, centre, i):
        value = np.float32(np.inf) if which == "unobserved" else np.float32(rng.uniform(-1.9, 0.0))
        st = random_state(rng, geo.prm, value=value, count=0, coord=0 if i % 2 else pack_mean(rng.uniform(-.05, .05, 3)),
                          cov=(0.0,) * 6 if i % 3 else random_factor(rng))
        sample = centre + rng.uniform(-0.095, 0.095, size=3)
        return st, [_h(*hit_ray(rng, centre, sample), rng.uniform(0, 60))], {}
    return build


def fam_h_reinit(count_delta, side):
    def build(rng, geo, centre, i):
        thr = np.float32(geo.prm.reinit_threshold)
        value = {"below": np.nextafter(thr, np.float32(-10)), "on": thr, "above": np.nextafter(thr, np.float32(10)),
                 "far_below": np.float32(thr - 0.5)}[side]
        st = random_state(rng, geo.prm, value=value, count=geo.prm.reinit_count + count_delta)
        sample = centre + rng.uniform(-0.095, 0.095, size=3)
        return st, [_h(*hit_ray(rng, centre, sample), rng.uniform(0, 60))], {}
    return build


def fam_h_unobserved_counted(rng, geo, centre, i):
    st = random_state(rng, geo.prm, value=np.float32(np.inf))
    sample = centre + rng.uniform(-0.095, 0.095, size=3)
    return st, [_h(*hit_ray(rng, centre, sample), rng.uniform(0, 60))], {}


def fam_h_ak0(rng, geo, centre, i):
    st = random_state(rng, geo.prm, cov=(0.0,) * 6)
    sample = ndt_ref.voxel_mean(st.coord, centre, RES)
    return st, [_h(*hit_ray(rng, centre, sample), rng.uniform(0, 60))], {}


def fam_h_zero_diag(position):
    def build(rng, geo, centre, i):
        cov = list(random_factor(rng, -2.5, -1.0))
        cov[(0, 2, 5)[position]] = 0.0
        st = random_state(rng, geo.prm, cov=tuple(cov))
        sample = centre + rng.uniform(-0.095, 0.095, size=3)
        return st, [_h(*hit_ray(rng, centre, sample), rng.uniform(0, 60))], dict(factor_bar="1e-6")
    return build


def fam_h_wall(rng, geo, centre, i):
    st = random_state(rng, geo.prm)
    sample = centre + rng.uniform(-0.095, 0.095, size=3)
    axis = int(rng.integers(3))
    sample[axis] = centre[axis] - HALF          # the lower wall belongs to the voxel where the key maths says so
    return st, [_h(*hit_ray(rng, centre, sample), rng.uniform(0, 60))], {}


def fam_h_at_max(which):
    def build(rng, geo, centre, i):
        hi = np.float32(geo.prm.max_value)
        value = {"on": hi, "below": np.nextafter(hi, np.float32(0)), "above": np.float32(hi + 1.0)}[which]
        st = random_state(rng, geo.prm, value=value)
        sample = centre + rng.uniform(-0.095, 0.095, size=3)
        return st, [_h(*hit_ray(rng, centre, sample), rng.uniform(0, 60))], {}
    return build


def fam_h_tm_gap(which, side, g):
    """NDT-TM on a hit: p_v p_s ("prod") or p_v ("pv", with p_v p_s < eta) at eta (1 +- g); the sample is moved along
    one line from the mean outwards."""
    def build(rng, geo, centre, i):
        prm = geo.prm
        st = random_state(rng, prm, lo=-2.3, hi=-1.9)
        mean = ndt_ref.voxel_mean(st.coord, centre, RES)
        e = unit(rng)
        d = unit(rng)
        reach = 0.9 * exit_distance(mean, e, centre)
        eta = mpf(f32(prm.adaptation_rate)) / 2
        want = eta * (1 + side * mpf(g))
        length = rng.uniform(0.25, 0.5)

        def place(s):
            sample = [mpf(float(m)) + s * mpf(float(x)) for m, x in zip(mean, e)]
            return [z - mpf(float(x)) * mpf(length) for z, x in zip(sample, d)], sample

        def f(s):
            sensor, sample = place(s)
            p_v, p_s = ndt_ref.likelihoods(prm, st.cov, mean, sensor, sample)
            return (p_v * p_s if which == "prod" else p_v) - want
        if not (f(mpf("1e-9")) > 0 > f(reach)):
            return None
        s = _bisect(f, "1e-9", reach)
        sample = mean + s * e
        return st, [_h(sample - d * length, sample, rng.uniform(0, 60))], dict(wanted_gap=side * g, gap_name=(
            "prod_hit" if which == "prod" else "p_v"))
    return build


def script_events(rng, geo, centre, st, pattern):
    """Events of one script on one voxel: hits scatter around a point of the voxel, misses pass near the mean the model
    has reached by then (so that they are NDT misses that matter once the count allows)."""
    events, focus = [], centre + rng.uniform(-0.05, 0.05, size=3)
    for kind in pattern:
        if kind == "H":
            sample = np.clip(focus + rng.normal(scale=0.015, size=3), centre - 0.095, centre + 0.095)
            ev = _h(*hit_ray(rng, centre, sample), rng.uniform(5, 25))
        else:
            mahal = rng.uniform(0, 1.5)
            cov_ok = st.cov[0] != 0 and st.cov[2] != 0 and st.cov[5] != 0
            probe = st if cov_ok else State(cov=(0.01, 0, 0.01, 0, 0, 0.01), coord=st.coord)
            ev = _m(*miss_ray(rng, probe, centre, mahal))
        events.append(ev)
        st = ndt_ref.apply(geo.prm, st, ev, centre).state
    return events


def fam_s_threshold(rng, geo, centre, i):
    """MMHMHHMM...: the count crosses sample_threshold inside the script."""
    body = "".join(rng.choice(list("HM"), size=int(rng.integers(4, 12))))
    pattern = "MMHMH" + "H" * (geo.prm.sample_threshold - 2) + "MM" + body
    st = State()
    return st, script_events(rng, geo, centre, st, pattern), {}


def fam_s_reinit(rng, geo, centre, i):
    """Hits past reinit_count, misses through the mean until the value is under reinit_threshold, then hits: the
    re-initialisation reached by integration.  adaptation_rate = 1 makes a miss through the mean cost several units of
    log-odds, so a few misses suffice."""
    prm = geo.prm
    st0 = State()
    events = script_events(rng, geo, centre, st0, "H" * (prm.reinit_count + int(rng.integers(1, 4))))
    st = st0
    for ev in events:
        st = ndt_ref.apply(prm, st, ev, centre).state
    for _ in range(30):
        if float(st.value) < prm.reinit_threshold - 0.05:
            break
        ev = _m(*miss_ray(rng, st, centre, rng.uniform(0, 0.7)))
        events.append(ev)
        st = ndt_ref.apply(prm, st, ev, centre).state
    else:
        return None
    for kind in "HH" + "M" * int(rng.integers(0, 3)) + "H":
        ev = script_events(rng, geo, centre, st, kind)[0]
        events.append(ev)
        st = ndt_ref.apply(prm, st, ev, centre).state
    return st0, events, {}


def fam_s_hits_only(planted):
    def build(rng, geo, centre, i):
        st = random_state(rng, geo.prm) if planted else State()
        return st, script_events(rng, geo, centre, st, "H" * int(rng.integers(6, 16))), {}
    return build


def _cells(build, cells):
    return [(cell, build(*cell)) for cell in cells]


def _gap_cells():
    return [(side, g) for side in (-1, 1) for g in GAPS]


# family name -> (config, cases per cell, [(cell, builder)])
FAMILIES = {
    "m_general": ("A", 96, [((), fam_m_general("general", "A"))]),
    "m_planar": ("A", 64, [((), fam_m_general("planar", "A"))]),
    "m_rod": ("A", 64, [((), fam_m_general("rod", "A"))]),
    "m_gap": ("A", 16, _cells(fam_m_gap, _gap_cells())),
    "m_prod0": ("A", 32, [((), fam_m_prod0)]),
    "m_unobserved": ("A", 32, [((), fam_m_unobserved)]),
    "m_count_edge": ("A", 32, _cells(fam_m_count_edge, [(-1,), (0,)])),
    "m_below_min": ("A", 16, _cells(fam_m_at_min, [("on",), ("below",), ("far_below",)])),
    "m_zero_diag": ("A", 16, _cells(fam_m_zero_diag, [(0,), (1,), (2,)])),
    "m_sensor_inside": ("A", 48, [((), fam_m_sensor_inside)]),
    "m_sample_wall": ("A", 48, [((), fam_m_sample_wall)]),
    "m_general_full_rate": ("B", 64, [((), fam_m_general("general", "B"))]),
    "m_through_mean": ("B", 32, [((), fam_m_through_mean)]),
    "m_sat_min": ("B", 16, _cells(fam_m_at_min, [("on",), ("above",), ("below",)])),
    "m_sat_max": ("B", 16, _cells(fam_m_at_max, [("on",), ("above",), ("below",)])),
    "m_variance": ("E", 48, [((), fam_m_variance)]),
    "m_clip": ("B", 24, _cells(fam_m_clip, [("moved",), ("end_inside",)])),
    "h_general": ("A", 96, [((), fam_h_general("general"))]),
    "h_planar": ("A", 48, [((), fam_h_general("planar"))]),
    "h_rod": ("A", 48, [((), fam_h_general("rod"))]),
    "h_count0": ("A", 24, _cells(fam_h_count0, [("unobserved",), ("observed",)])),
    "h_reinit": ("A", 12, _cells(fam_h_reinit, [(c, s) for c in (-1, 0) for s in ("below", "on", "above", "far_below")])),
    "h_reinit_small_count": ("B", 12, _cells(fam_h_reinit, [(c, s) for c in (-1, 0, 7)
                                                            for s in ("below", "above")])),
    "h_unobserved_counted": ("A", 24, [((), fam_h_unobserved_counted)]),
    "h_ak0": ("A", 16, [((), fam_h_ak0)]),
    "h_zero_diag": ("A", 12, _cells(fam_h_zero_diag, [(0,), (1,), (2,)])),
    "h_wall": ("A", 32, [((), fam_h_wall)]),
    "h_max": ("A", 16, _cells(fam_h_at_max, [("on",), ("below",), ("above",)])),
    "h_sat_max": ("B", 16, _cells(fam_h_at_max, [("on",), ("below",), ("above",)])),
    "h_tm_gap": ("A", 8, _cells(fam_h_tm_gap, [(w, s, g) for w in ("prod", "pv") for s, g in _gap_cells()])),
    "s_threshold": ("A", 16, [((), fam_s_threshold)]),
    "s_reinit": ("C", 12, [((), fam_s_reinit)]),
    "s_hits_only": ("D", 12, _cells(fam_s_hits_only, [(False,), (True,)])),
}


def _achieved(steps, name):
    for step in steps:
        if name in step.gaps:
            return float(step.gaps[name])
    return None


def run_model(prm, case, centre):
    """The model's steps over a case's events from its planted state (raises ndt_ref.Ambiguous)."""
    st, steps = case.state, []
    for ev in case.model_events:
        step = ndt_ref.apply(prm, st, ev, centre)
        steps.append(step)
        st = step.state
    return steps


@functools.lru_cache(maxsize=None)
def build(seed=SEED):
    """-> (sheets, stats): stats[family] = dict(constructed, band, geometry, redrawn)."""
    rng = np.random.default_rng(seed)
    per_config = {name: [] for name in CONFIGS}
    stats = {}
    for family, (config, per_cell, cells) in FAMILIES.items():
        geo = geometry(config)
        st = stats[family] = dict(constructed=0, band=0, geometry=0, redrawn=0, cells={})
        for cell, builder in cells:
            made = 0
            attempts = 0
            while made < per_cell:
                attempts += 1
                assert attempts < 60 * per_cell, (family, cell, st)
                slot = len(per_config[config])
                local = geo.targets[slot % len(geo.targets)]
                centre = geo.centre(local)
                try:
                    out = builder(rng, geo, centre, made)
                except Ambiguous:
                    st["constructed"] += 1
                    st["band"] += 1
                    continue
                if out is None or out[1] is None:
                    st["redrawn"] += 1
                    continue
                state, events, extras = out
                if not all(geo.accepts(local, ev[0], ev[1], ev[2]) for ev in events):
                    st["geometry"] += 1
                    continue
                st["constructed"] += 1
                gap_name = extras.pop("gap_name", "prod")
                case = Case(family, cell, config, state, events, local=local, **extras)
                case.model_events = [(k, s, geo.filtered(s, z)[0], it) for k, s, z, it in events]
                try:
                    steps = run_model(geo.prm, case, centre)
                except Ambiguous:
                    st["band"] += 1
                    continue
                if case.wanted_gap is not None:
                    got = _achieved(steps, gap_name)
                    g = abs(case.wanted_gap)
                    if got is None or got * case.wanted_gap <= 0 or not g / 2 <= abs(got) <= 2 * g:
                        st["redrawn"] += 1
                        continue
                per_config[config].append(case)
                made += 1
            st["cells"][cell] = made
    sheets = []
    for config, cases in per_config.items():
        n = len(geometry(config).targets)
        for first in range(0, len(cases), n):
            sheets.append(Sheet(config, cases[first:first + n]))
    return sheets, stats


# ---------------------------------------------------------------------------------------------------------------------
# planting, reading back and judging one transition: shared by the CPU test (oracle) and the GPU test (device)
# ---------------------------------------------------------------------------------------------------------------------
LAYER_SHAPES = {"occupancy": (np.float32, 1), "mean": (np.uint32, 2), "covariance": (np.float32, 6),
                "intensity": (np.float32, 2), "hit_miss_count": (np.uint32, 2)}


def layers_of(prm):
    return ["occupancy", "mean", "covariance"] + (["intensity", "hit_miss_count"] if prm.ndt_tm else [])


def planted_tiles(sheet):
    """Region (0, 0, 0) of a sheet's map with every case's state in its target voxel, the rest untouched."""
    geo = geometry(sheet.config)
    volume = geo.region[0] * geo.region[1] * geo.region[2]
    tiles = {name: np.zeros(volume * LAYER_SHAPES[name][1], dtype=LAYER_SHAPES[name][0]) for name in layers_of(geo.prm)}
    tiles["occupancy"][:] = np.inf
    for case in sheet.cases:
        write_state(tiles, geo.index(case.local), case.state)
    return tiles


def write_state(tiles, vi, st):
    tiles["occupancy"][vi] = st.value
    tiles["mean"][2 * vi:2 * vi + 2] = (st.coord, st.count)
    tiles["covariance"][6 * vi:6 * vi + 6] = st.cov
    if "intensity" in tiles:
        tiles["intensity"][2 * vi:2 * vi + 2] = st.intensity
        tiles["hit_miss_count"][2 * vi:2 * vi + 2] = st.hit_miss


def read_state(tiles, vi):
    """The voxel as an implementation holds it: float32 values exactly (float() of a float32 is exact)."""
    tm = "intensity" in tiles
    return State(value=np.float32(tiles["occupancy"][vi]), cov=tuple(float(v) for v in tiles["covariance"][6 * vi:6 * vi + 6]),
                 coord=int(tiles["mean"][2 * vi]), count=int(tiles["mean"][2 * vi + 1]),
                 intensity=tuple(float(v) for v in tiles["intensity"][2 * vi:2 * vi + 2]) if tm else (0.0, 0.0),
                 hit_miss=tuple(int(v) for v in tiles["hit_miss_count"][2 * vi:2 * vi + 2]) if tm else (0, 0), exact=True)


def same_bits(a, b):
    """Two states, bit for bit."""
    fa = np.array((a.value,) + a.cov + a.intensity, dtype=np.float32).view(np.uint32)
    fb = np.array((b.value,) + b.cov + b.intensity, dtype=np.float32).view(np.uint32)
    return bool(np.array_equal(fa, fb)) and (a.coord, a.count, a.hit_miss) == (b.coord, b.count, b.hit_miss)


# The intensity pair is a float32 recursion in the reference, five and nine roundings deep; the model rounds once.  With
# n, the old pair and the sample exact float32 inputs and intensities non-negative (no cancellation in the sums):
#   mean' = inv * (n * mean + i): inv, the product, the sum and the outer product round once each: 4 half-ulps = 2 ulp
#   cov'  = inv * (n * cov + inv * delta * delta): delta (twice) 1, its two products and inv 1.5, the sum of two
#           non-negative terms 0.5 on top of the larger term error, n * cov 0.5, the outer product and inv 1: 4 ulp
# in units of 2^-23 |exact| (no finer than a true ulp).
INTENSITY_BAR = (2.0, 4.0)


def judge(prm, pre, event, centre, post, factor_bar="ulp"):
    """Hold one transition of an implementation (pre -> post, both as it stores them) to the model run on the same pre
    state.  Returns the measured errors in the bars' own units; raises AssertionError on a miss of a bar."""
    step = ndt_ref.apply(prm, pre, event, centre)
    want = step.state
    kind = event[0]
    assert (post.coord, post.count) == (want.coord, want.count), ("mean", kind, step.path, pre, post, want)
    if prm.ndt_tm:
        assert post.hit_miss == want.hit_miss, ("hit_miss", kind, step.path, step.gaps, pre, post, want)
    out = dict(value=0.0, factor=0.0, factor_rel=0.0, intensity=0.0, path=step.path, is_miss=step.is_miss)
    if not (np.float32(post.value) == np.float32(want.value) and not np.isfinite(post.value)):
        err = abs(mpf(float(post.value)) - step.value_exact)
        out["value"] = float(err) / ndt_ref.ulp32(step.scale)
        assert out["value"] <= 1.0, ("value", kind, step.path, out["value"], pre, post, want)
    if kind == "M":
        assert post.cov == pre.cov and post.intensity == pre.intensity, ("a miss moved the factor", pre, post)
        return out
    for got, exact in zip(post.cov, step.cov_exact):
        err = abs(mpf(got) - exact)
        if factor_bar == "1e-6":
            rel = float(err / abs(exact)) if exact != 0 else (0.0 if got == 0 else np.inf)
            out["factor_rel"] = max(out["factor_rel"], rel)
            assert rel <= 1e-6, ("factor (1e-6)", step.path, rel, pre, post, want)
        else:
            ulps = float(err) / ndt_ref.ulp32(exact)
            out["factor"] = max(out["factor"], ulps)
            assert ulps <= 1.0, ("factor", step.path, ulps, got, exact, pre, post, want)
    if prm.ndt_tm:
        for got, exact, bar in zip(post.intensity, step.intensity_exact, INTENSITY_BAR):
            unit = float(abs(exact)) * 2.0 ** -23
            ulps = float(abs(mpf(got) - exact)) / unit if unit else (0.0 if got == 0 else np.inf)
            out["intensity"] = max(out["intensity"], ulps / bar)
            assert ulps <= bar, ("intensity", step.path, ulps, pre, post, want)
    return out


def step_rays(sheet, k):
    """The k-th event of every case of the sheet that has one: (cases, rays (2n, 3), intensities (n,))."""
    cases = [c for c in sheet.cases if len(c.events) > k]
    rays = np.empty((2 * len(cases), 3), dtype=np.float64)
    for i, c in enumerate(cases):
        rays[2 * i], rays[2 * i + 1] = c.events[k][1], c.events[k][2]
    return cases, rays, np.array([c.events[k][3] for c in cases], dtype=np.float32)


def all_rays(sheet, segment_of=None):
    """Every event of the sheet, voxel scripts in order, as a list of calls (rays, intensities): one call, or one per
    value of segment_of(case, k)."""
    calls = {}
    depth = max(len(c.events) for c in sheet.cases)
    for k in range(depth):
        for c in sheet.cases:
            if len(c.events) > k:
                seg = segment_of(c, k) if segment_of else 0
                calls.setdefault(seg, []).append(c.events[k])
    out = []
    for seg in sorted(calls):
        evs = calls[seg]
        rays = np.empty((2 * len(evs), 3), dtype=np.float64)
        rays[0::2] = [e[1] for e in evs]
        rays[1::2] = [e[2] for e in evs]
        out.append((rays, np.array([e[3] for e in evs], dtype=np.float32)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the oracle side of a sheet, and the per-family table both tests print
# ---------------------------------------------------------------------------------------------------------------------
def make_oracle(config):
    geo = geometry(config)
    prm = geo.prm
    om = OracleMap(RES, geo.region, layers_of(prm))
    om.set_origin(geo.origin)
    om.set_ray_filter(*geo.ray_filter)
    _olib.oracle_map_set_hit_value(om.handle, prm.hit_value)
    _olib.oracle_map_set_miss_value(om.handle, prm.miss_value)
    _olib.oracle_map_set_min_max(om.handle, prm.min_value, prm.max_value)
    _olib.oracle_map_set_saturation(om.handle, int(prm.saturate_at_min), int(prm.saturate_at_max))
    om.set_ndt(sensor_noise=prm.sensor_noise, sample_threshold=prm.sample_threshold,
               adaptation_rate=prm.adaptation_rate, reinit_threshold=prm.reinit_threshold,
               reinit_count=prm.reinit_count, initial_intensity_cov=prm.initial_intensity_cov, ndt_tm=prm.ndt_tm)
    return om


def plant(om, sheet):
    """Create region (0, 0, 0) and overwrite every layer of it with the sheet's planted tiles."""
    geo = geometry(sheet.config)
    c = geo.centre(geo.targets[0])
    om.integrate_ndt(np.array([c, c]), intensities=np.zeros(1, dtype=np.float32))
    tiles = planted_tiles(sheet)
    for name, tile in tiles.items():
        om.region_layer_view((0, 0, 0), name)[:] = tile
    return tiles


def oracle_tiles(om, prm):
    return {name: om.region_layer((0, 0, 0), name) for name in layers_of(prm)}


class Worst:
    """Per-family worst figures, printed as a table."""

    def __init__(self):
        self.rows = {}

    def add(self, family, out):
        row = self.rows.setdefault(family, dict(events=0, value=0.0, factor=0.0, factor_rel=0.0, intensity=0.0))
        row["events"] += 1
        for k in ("value", "factor", "factor_rel", "intensity"):
            row[k] = max(row[k], out[k])

    def show(self, title):
        print("\n%s\n%-22s %7s %10s %11s %12s %14s" % (title, "family", "events", "value/ulp", "factor/ulp",
                                                      "factor rel", "intensity/bar"))
        for family, r in self.rows.items():
            print("%-22s %7d %10.3f %11.3f %12.2e %14.3f" % (family, r["events"], r["value"], r["factor"],
                                                            r["factor_rel"], r["intensity"]))
