"""An exact model of ONE NDT voxel (test infrastructure): what a ray through it (M) and a sample in it (H) do to its
state, written from the equations of Saarinen et al. as ohm/CovarianceVoxelCompute.h documents them -- not from
oracle/ohm_oracle.c and not from ohm_amd/csrc/ndt_tsdf_device.h, which were restated from one reading of the code.

Everything continuous is evaluated with mpmath at 60 digits on the exact values of the fp32 / fp64 inputs.  Rounding
happens only where the reference STORES: the float32 occupancy value, the six float32 factor terms, the float32
intensity pair.  Two inputs are formed in floating point by the reference before any of the maths here and are taken as
it forms them: the voxel mean (packed coordinate -> fp64 local offset + fp64 voxel centre; the packed coordinate and its
update come from oracle_sub_voxel_to_local / oracle_sub_voxel_update, which have exact pins of their own) and the sensor
noise variance, which is the FLOAT32 product sensor_noise * sensor_noise.

Miss (one ray through the voxel, sensor s, sample z, mean u, stored lower-triangular factor C, P = C C^T):
    l = (z - s) / |z - s|,  a = C^-1 l,  b = C^-1 (s - u),  t = -a.b / a.a,  x_ML = s + t l
    p_v = exp(-1/2 |C^-1 (x_ML - u)|^2),  p_s = exp(-1/2 |x_ML - z|^2 / sigma^2)
    prod = p_v (1 - p_s),  eta = adaptation_rate / 2,  p = 1/2 - eta prod,  delta = ln(p / (1 - p))
  around it: an unobserved value becomes miss_value; count < sample_threshold adds miss_value; is_miss = prod < eta;
  a zero factor diagonal divides by zero (the reference's NaN guard: value unchanged, is_miss false); then the
  saturation select and the min clamp of occupancyAdjustDown.
Hit (one sample z in the voxel): (re)initialisation when count == 0 or (value < reinit_threshold and count >=
  reinit_count) -- the factor becomes 0.1f * resolution on the diagonal and the count restarts; otherwise
    P' = n/(n+1) P + n/(n+1)^2 (z - u)(z - u)^T
  and the new factor is THE lower-triangular Cholesky factor of P' with non-negative diagonal (unique when P' is
  positive definite), taken in mpmath: the reference's rank-one Gram-Schmidt update is not restated.  Value: hit_value
  for an unobserved voxel, value + hit_value otherwise; then the select and max clamp of occupancyAdjustUp.
NDT-TM on a hit, from the state BEFORE the hit: reset when the value is unobserved or the factor (re)initialises;
  inc_hit = reset or n < sample_threshold or p_v p_s >= eta;  inc_miss = not reset and n >= sample_threshold and
  p_v p_s < eta and p_v >= eta; the intensity pair follows mean' = (n mean + i)/(n+1),
  cov' = (n cov + (mean - i)^2/(n+1))/(n+1), reset to (i, initial_intensity_covariance).

Decision bands.  The model decides prod < eta, p_v p_s >= eta and p_v >= eta exactly; implementations decide in fp64.
A case whose exact gap to eta is below BAND_REL relative is ambiguous and the model RAISES Ambiguous.  A state the model
has propagated itself (State.exact False: its stored value may differ from an implementation's by the roundings the
bars allow) is also ambiguous when its value lies within BAND_ULPS float32 ulp of reinit_threshold, sat_min or sat_max
at the moment that comparison is made; a planted or read-back state (State.exact True) compares float32 against
float32 as the reference does, with nothing to band.  Nothing is ever dropped silently."""
import math
from dataclasses import dataclass, field, replace

import mpmath
import numpy as np
from mpmath import libmp

from oracle.oracle import _d3, lib as _olib

MP = mpmath.mp.clone()
MP.dps = 60
mpf = MP.mpf
INF32 = np.float32(np.inf)
BAND_REL = mpf(10) ** -9
BAND_ULPS = 8


class Ambiguous(Exception):
    """The case sits inside a decision band: fp64 and exact arithmetic may decide differently."""


@dataclass(frozen=True)
class Params:
    resolution: float = 0.2
    hit_value: float = 0.0
    miss_value: float = 0.0
    min_value: float = -2.0
    max_value: float = 3.511
    saturate_at_min: bool = False
    saturate_at_max: bool = False
    sensor_noise: float = 0.05
    sample_threshold: int = 3
    adaptation_rate: float = 0.2
    reinit_threshold: float = -1.3862944
    reinit_count: int = 100
    initial_intensity_cov: float = 1.0
    ndt_tm: bool = True

    def f32(self, name):
        return np.float32(getattr(self, name))

    @property
    def sat_min(self):
        """ohm/RayMapperNdt.cpp:110-111: the saturation bounds the adjust functions select on."""
        return self.f32("min_value") if self.saturate_at_min else np.float32(np.finfo(np.float32).min)

    @property
    def sat_max(self):
        return self.f32("max_value") if self.saturate_at_max else np.float32(np.finfo(np.float32).max)


@dataclass(frozen=True)
class State:
    value: np.float32 = INF32
    cov: tuple = (0.0,) * 6            # float32 values, packed 0 / 1 2 / 3 4 5 (lower triangle by rows)
    coord: int = 0
    count: int = 0
    intensity: tuple = (0.0, 0.0)      # float32 (mean, covariance)
    hit_miss: tuple = (0, 0)
    exact: bool = True                 # planted or read back (True) / propagated by the model (False)


@dataclass
class Step:
    """What one event did, beyond the new state: the unrounded figures the bars are measured against."""
    state: State
    kind: str
    value_exact: object = None         # mpf (or +-inf): the value before its float32 store
    scale: object = None               # max(|delta|, |initial|, |result|): where the value's ulp is taken
    cov_exact: tuple = None            # six mpf, hits only
    intensity_exact: tuple = None      # two mpf, NDT-TM hits only
    is_miss: bool = None
    gaps: dict = field(default_factory=dict)   # name -> relative distance of an exact decision from eta
    path: str = ""


def to_f32(x):
    """mpf -> np.float32, one rounding to nearest even (not through fp64, which would round twice)."""
    x = mpf(x)
    if not MP.isfinite(x):
        return np.float32(float(x))
    return np.float32(float(mpf(libmp.mpf_pos(x._mpf_, 24, libmp.round_nearest))))


def ulp32(x):
    """Spacing of float32 at |x| (normal range; never below the spacing at the smallest normal)."""
    x = abs(float(x))
    if not math.isfinite(x):
        return math.inf
    return 2.0 ** (max(math.frexp(x)[1], -125) - 24)


def vec(v):
    return [mpf(float(x)) for x in v]


def dot(a, b):
    return sum((x * y for x, y in zip(a, b)), mpf(0))


def solve_lower(c, y):
    """x with C x = y, C packed as State.cov."""
    x0 = y[0] / c[0]
    x1 = (y[1] - c[1] * x0) / c[2]
    x2 = (y[2] - c[3] * x0 - c[4] * x1) / c[5]
    return [x0, x1, x2]


def voxel_mean(coord, centre, resolution):
    """The fp64 mean the reference hands to the NDT maths: sub-voxel local offset + voxel centre, both fp64."""
    import ctypes as C
    local = (C.c_double * 3)()
    _olib.oracle_sub_voxel_to_local(int(coord), float(resolution), local)
    return np.array(local, dtype=np.float64) + np.asarray(centre, dtype=np.float64)


def likelihoods(prm, cov, mean, sensor, sample):
    """(p_v, p_s) exactly, or None when a factor diagonal is zero (the reference divides by zero there)."""
    c = vec(cov)
    if c[0] == 0 or c[2] == 0 or c[5] == 0:
        return None
    s, z, u = vec(sensor), vec(sample), vec(mean)
    ray = [zi - si for zi, si in zip(z, s)]
    norm = MP.sqrt(dot(ray, ray))
    ell = [r / norm for r in ray]
    a = solve_lower(c, ell)
    b = solve_lower(c, [si - ui for si, ui in zip(s, u)])
    t = -dot(a, b) / dot(a, a)
    x_ml = [si + t * li for si, li in zip(s, ell)]
    w = solve_lower(c, [xi - ui for xi, ui in zip(x_ml, u)])
    p_v = MP.exp(-dot(w, w) / 2)
    noise = prm.f32("sensor_noise")
    variance = mpf(float(np.float32(noise * noise)))    # the float32 product
    d = [xi - zi for xi, zi in zip(x_ml, z)]
    p_s = MP.exp(-dot(d, d) / (2 * variance))
    return p_v, p_s


def _eta(prm):
    return mpf(float(prm.f32("adaptation_rate"))) / 2


def _gap(x, eta, name, gaps):
    g = (x - eta) / eta
    gaps[name] = g
    if abs(g) < BAND_REL:
        raise Ambiguous("%s within %s of eta" % (name, MP.nstr(abs(g), 3)))
    return g


def _banded(state, bound, name):
    """A float32 comparison of a model-propagated value against `bound`: ambiguous within BAND_ULPS ulp of it."""
    if state.exact or not np.isfinite(state.value) or not np.isfinite(bound):
        return
    if abs(float(state.value) - float(bound)) <= BAND_ULPS * ulp32(bound):
        raise Ambiguous("value within %d ulp of %s" % (BAND_ULPS, name))


def _unsaturated(prm, state):
    _banded(state, prm.sat_min, "sat_min")
    _banded(state, prm.sat_max, "sat_max")
    return state.value == INF32 or (prm.sat_min < state.value < prm.sat_max)


def _reinitialises(prm, state):
    if state.count == 0:
        return True
    if state.count >= prm.reinit_count:
        _banded(state, prm.f32("reinit_threshold"), "reinit_threshold")
        return bool(state.value < prm.f32("reinit_threshold"))
    return False


def miss(prm, state, sensor, sample, centre):
    """One ray through the voxel."""
    initial = state.value
    gaps = {}
    is_miss = True
    delta = None
    if initial == INF32:
        adjusted, path = mpf(float(prm.f32("miss_value"))), "unobserved"
    elif state.count < prm.sample_threshold:
        delta = mpf(float(prm.f32("miss_value")))
        adjusted, path = mpf(float(initial)) + delta, "plain"
    else:
        like = likelihoods(prm, state.cov, voxel_mean(state.coord, centre, prm.resolution), sensor, sample)
        if like is None:
            adjusted, is_miss, path = mpf(float(initial)), False, "nan"
        else:
            p_v, p_s = like
            eta = _eta(prm)
            prod = p_v * (1 - p_s)
            is_miss = _gap(prod, eta, "prod", gaps) < 0
            p = mpf(1) / 2 - eta * prod
            delta = MP.log(p / (1 - p)) if p > 0 else mpf("-inf")
            adjusted, path = mpf(float(initial)) + delta, "ndt"
    # occupancyAdjustDown: saturation select, then the min clamp
    if not _unsaturated(prm, state):
        adjusted, path = mpf(float(initial)), path + "+saturated"
    lo = mpf(float(prm.f32("min_value")))
    exact = adjusted if adjusted > lo else lo
    scale = max(abs(exact), abs(mpf(float(initial))) if np.isfinite(initial) else mpf(0),
                abs(delta) if delta is not None and MP.isfinite(delta) else mpf(0))
    hit_miss = state.hit_miss
    if prm.ndt_tm and is_miss:
        hit_miss = (hit_miss[0], (hit_miss[1] + 1) & 0xffffffff)
    new = replace(state, value=to_f32(exact), hit_miss=hit_miss, exact=False)
    return Step(new, "M", value_exact=exact, scale=scale, is_miss=is_miss, gaps=gaps, path=path)


def cholesky_lower(p):
    """Lower-triangular factor with non-negative diagonal of a symmetric positive semi-definite 3x3 (a zero pivot's
    column is zero, as it must be for such a matrix)."""
    c = [[mpf(0)] * 3 for _ in range(3)]
    for k in range(3):
        d = p[k][k] - sum((c[k][i] * c[k][i] for i in range(k)), mpf(0))
        if d < 0:
            raise ArithmeticError("not positive semi-definite")
        c[k][k] = MP.sqrt(d)
        for j in range(k + 1, 3):
            r = p[j][k] - sum((c[j][i] * c[k][i] for i in range(k)), mpf(0))
            c[j][k] = r / c[k][k] if c[k][k] != 0 else mpf(0)
    return [c[0][0], c[1][0], c[1][1], c[2][0], c[2][1], c[2][2]]


def hit(prm, state, sensor, sample, centre, intensity=0.0):
    """One sample in the voxel."""
    initial = state.value
    n = state.count
    gaps = {}
    reinit = _reinitialises(prm, state)
    mean = voxel_mean(state.coord, centre, prm.resolution)
    path = "init" if n == 0 else ("reinit" if reinit else "update")
    hit_miss, intensity_pair, intensity_exact = state.hit_miss, state.intensity, None
    if prm.ndt_tm:
        reset = bool(initial == INF32) or reinit
        h, m = (0, 0) if reset else state.hit_miss
        inc_hit, inc_miss = True, False
        if not reset and n >= prm.sample_threshold:
            like = likelihoods(prm, state.cov, mean, sensor, sample)
            if like is None:
                inc_hit = False            # NaN compares false both ways
            else:
                p_v, p_s = like
                eta = _eta(prm)
                inc_hit = _gap(p_v * p_s, eta, "prod_hit", gaps) >= 0
                inc_miss = (not inc_hit) and _gap(p_v, eta, "p_v", gaps) >= 0
        hit_miss = ((h + int(inc_hit)) & 0xffffffff, (m + int(inc_miss)) & 0xffffffff)
        i_s = mpf(float(np.float32(intensity)))
        if n == 0 or reinit:
            intensity_exact = (i_s, mpf(float(prm.f32("initial_intensity_cov"))))
        else:
            i_m, i_c = vec(state.intensity)
            intensity_exact = ((n * i_m + i_s) / (n + 1), (n * i_c + (i_m - i_s) ** 2 / (n + 1)) / (n + 1))
        intensity_pair = tuple(float(to_f32(x)) for x in intensity_exact)
    if reinit:
        s = mpf(float(np.float32(np.float32(0.1) * np.float32(prm.resolution))))
        cov_exact = (s, mpf(0), s, mpf(0), mpf(0), s)
        n = 0
    else:
        c = vec(state.cov)
        big = [[c[0], 0, 0], [c[1], c[2], 0], [c[3], c[4], c[5]]]
        d = [zi - ui for zi, ui in zip(vec(sample), vec(mean))]
        w0, w1 = mpf(n) / (n + 1), mpf(n) / (mpf(n + 1) ** 2)
        p = [[w0 * sum((big[i][k] * big[j][k] for k in range(3)), mpf(0)) + w1 * d[i] * d[j] for j in range(3)]
             for i in range(3)]
        cov_exact = tuple(cholesky_lower(p))
    hv = mpf(float(prm.f32("hit_value")))
    adjusted = hv if initial == INF32 else mpf(float(initial)) + hv
    if not _unsaturated(prm, state):
        adjusted, path = mpf(float(initial)), path + "+saturated"
    hi = mpf(float(prm.f32("max_value")))
    exact = adjusted if adjusted < hi else hi
    scale = max(abs(exact), abs(mpf(float(initial))) if np.isfinite(initial) else mpf(0), abs(hv))
    local = np.asarray(sample, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    coord = int(_olib.oracle_sub_voxel_update(int(state.coord), int(n), _d3(local), float(prm.resolution)))
    new = State(value=to_f32(exact), cov=tuple(float(to_f32(x)) for x in cov_exact), coord=coord, count=n + 1,
                intensity=intensity_pair, hit_miss=hit_miss, exact=False)
    return Step(new, "H", value_exact=exact, scale=scale, cov_exact=cov_exact, intensity_exact=intensity_exact,
                gaps=gaps, path=path)


def apply(prm, state, event, centre):
    """event: ("H" | "M", sensor, sample, intensity)."""
    kind, sensor, sample, intensity = event
    if kind == "M":
        return miss(prm, state, sensor, sample, centre)
    return hit(prm, state, sensor, sample, centre, intensity)
