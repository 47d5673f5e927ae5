"""An exact model of the TSDF voxel update (test infrastructure).

ohm/VoxelTsdfCompute.h, instantiated with Vec3 = dvec3 as RayMapperTsdf does:

    computeDistance (:57-68)
        g    = float(sqrt(dot(sample - sensor, sample - sensor)))       fp64 dot, (x + y) + z, ONE cast of the root
        gv   = float(dot(centre - sensor, sample - sensor)) / g         the cast BEFORE the (float) divide
        sdf  = g - gv
    calculateTsdf (:99-135), every operation in float32
        uw   = 1 * (dropoff > 0 ? (trunc + sdf) / (trunc - dropoff) : 1)
        uw   = std::max(uw, 0)                                          (a < b) ? b : a -- a NaN uw stays
        uw  *= (sparsity > 0 && fabs(sdf) < trunc) ? sparsity : 1
        nw   = w + uw
        near = fabs(nw) < 0.00001f
        ns   = near ? 0 : (sdf * uw + d * w) / nw
        d'   = near ? d : (ns > 0 ? std::min(trunc, ns) : std::max(-trunc, ns))
        w'   = near ? w : std::min(nw, max_weight)
    with std::min(a, b) = (b < a) ? b : a and std::max(a, b) = (a < b) ? b : a: a NaN ns fails `ns > 0` and
    `-trunc < ns`, so it is stored as -trunc; a NaN nw is stored as it is.

update_ref() is that chain in numpy float32 arithmetic, one rounding per operation, on scalars or on arrays (element by
element: the voxels of a batch are independent, so a whole batch is replayed one visit per voxel at a time).

The independent check.  update_exact() evaluates each operation's exact rational result with fractions.Fraction from
the float32 inputs and rounds it once with round_f32(), written here (ties to even, subnormals, overflow to infinity):
numpy's float32 arithmetic is not used.  Zeros, infinities and NaN follow the IEEE rules for the operation (a Python
float is an IEEE double and those rules do not depend on the width).

counted(opts, w, d, sdfs) is the statement, from the reference alone, of when a run of visits may be applied as a
count: replaying them from (w, d) gives (min(w + float(n), max_weight), trunc) -- `w + float(n)` one float32 addition.
It knows no device constant.

Mutants: the same chain with one change each (MUTANTS).  `fma` takes the fused sum from float64 (the product is exact
there; the sum is then rounded twice, which only matters to a mutant in that it stays deterministic); `count_once` and
`dot_cast_late` act outside update_ref: the first in tsdf_cases.replay (a voxel's free-space visits of one batch as
one addition -- what the device does where its mask does not stop it), the second in sdf_ref."""
import math
import struct
from collections import namedtuple
from fractions import Fraction

import numpy as np

F = np.float32
NEAR_ZERO = F(0.00001)

UPDATE_MUTANTS = ("fma", "recip", "clamp_sdf_first", "sparsity_le", "near_zero_le", "near_zero_signed", "clamp_swapped",
                  "cap_first", "dropoff_unclamped")
MUTANTS = UPDATE_MUTANTS + ("count_once", "dot_cast_late")

Opts = namedtuple("Opts", "max_weight trunc dropoff sparsity")


def opts(max_weight=1e4, trunc=0.3, dropoff=0.0, sparsity=1.0):
    """The four options as the float32 values the reference holds them as."""
    return Opts(F(max_weight), F(trunc), F(dropoff), F(sparsity))


def bits(x):
    """uint32 view of float32 value(s)."""
    return np.asarray(x, dtype=F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# the signed distance of a visit
# ---------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sdf_ref(sensor, sample, centre, mutant=None):
    """computeDistance on float64 arrays of shape (..., 3) -> float32."""
    sensor, sample, centre = (np.asarray(v, dtype=np.float64) for v in (sensor, sample, centre))
    to_voxel, to_sample = centre - sensor, sample - sensor
    with np.errstate(all="ignore"):
        g = np.sqrt(_dot(to_sample, to_sample)).astype(F)
        if mutant == "dot_cast_late":
            gv = (_dot(to_voxel, to_sample) / g.astype(np.float64)).astype(F)
        else:
            gv = _dot(to_voxel, to_sample).astype(F) / g
        return g - gv


# ---------------------------------------------------------------------------------------------------------------------
# the update, in float32 arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def update_ref(o, sdf, w, d, mutant=None, trace=None):
    """calculateTsdf given the sdf: (w', d').  Scalars or arrays; `trace` (a dict) counts the paths taken."""
    sdf, w, d = (np.asarray(v, dtype=F) for v in (sdf, w, d))
    one = F(1.0)
    with np.errstate(all="ignore"):
        if mutant == "clamp_sdf_first":
            sdf = np.where(sdf > F(0), np.where(sdf < o.trunc, sdf, o.trunc), np.where(-o.trunc < sdf, sdf, -o.trunc))
        uw = np.full(sdf.shape, one, dtype=F)
        if o.dropoff > 0:
            uw = uw * ((o.trunc + sdf) / (o.trunc - o.dropoff))
        else:
            uw = uw * one
        clamped0 = uw < F(0)
        if mutant != "dropoff_unclamped":
            uw = np.where(clamped0, F(0), uw)                       # std::max(uw, 0.0f)
        inside = (np.abs(sdf) <= o.trunc) if mutant == "sparsity_le" else (np.abs(sdf) < o.trunc)
        sparse = inside if o.sparsity > 0 else np.zeros(sdf.shape, dtype=bool)
        uw = uw * np.where(sparse, o.sparsity, one)
        nw = w + uw
        if mutant == "near_zero_le":
            near = np.abs(nw) <= NEAR_ZERO
        elif mutant == "near_zero_signed":
            near = nw < NEAR_ZERO
        else:
            near = np.abs(nw) < NEAR_ZERO
        divisor = np.where(o.max_weight < nw, o.max_weight, nw) if mutant == "cap_first" else nw
        if mutant == "fma":
            num = (sdf.astype(np.float64) * uw.astype(np.float64) + (d * w).astype(np.float64)).astype(F)
        else:
            num = sdf * uw + d * w
        ns = num * (one / divisor) if mutant == "recip" else num / divisor
        ns = np.where(near, F(0), ns)
        if mutant == "clamp_swapped":                               # std::min(ns, trunc) / std::max(ns, -trunc)
            cl = np.where(ns > F(0), np.where(o.trunc < ns, o.trunc, ns), np.where(ns < -o.trunc, -o.trunc, ns))
        else:                                                       # std::min(trunc, ns) / std::max(-trunc, ns)
            cl = np.where(ns > F(0), np.where(ns < o.trunc, ns, o.trunc), np.where(-o.trunc < ns, ns, -o.trunc))
        d1 = np.where(near, d, cl).astype(F)
        w1 = np.where(near, w, np.where(o.max_weight < nw, o.max_weight, nw)).astype(F)
    if trace is not None:
        for name, hit in (("near_zero", near), ("dropoff_clamped_to_0", clamped0), ("sparsity_applied", sparse),
                          ("weight_capped", ~near & (o.max_weight < nw)), ("clamped_hi", ~near & (ns >= o.trunc)),
                          ("clamped_lo", ~near & ~(ns > F(0)) & ~(-o.trunc < ns)), ("nan_sdf_stored_as_-trunc",
                                                                                    ~near & np.isnan(ns))):
            trace[name] = trace.get(name, 0) + int(np.count_nonzero(hit))
    return w1, d1


def run_ref(o, sdfs, w, d, mutant=None):
    """(w, d) after the visits `sdfs` in order (scalars)."""
    for sdf in sdfs:
        w, d = update_ref(o, sdf, w, d, mutant)
    return F(w), F(d)


def counted(o, w, d, sdfs):
    """True where the visits `sdfs`, replayed in order from (w, d), leave (min(w + float(n), max_weight), trunc): the run
    may then be applied as a count.  Stated from the reference: the replay is update_ref."""
    w1, d1 = run_ref(o, sdfs, w, d)
    with np.errstate(all="ignore"):
        wn = F(w) + F(len(sdfs))
        expect = o.max_weight if o.max_weight < wn else wn
    return bool(bits(w1) == bits(expect) and bits(d1) == bits(o.trunc))


# ---------------------------------------------------------------------------------------------------------------------
# the update, exactly
# ---------------------------------------------------------------------------------------------------------------------
def f32(x):
    """A Python float rounded to float32 (as a double), by the C library's conversion: for constants only."""
    return struct.unpack("f", struct.pack("f", x))[0]


def round_f32(q, negative_zero=False):
    """The rational q rounded once to float32, ties to even, as a Python float; +-inf on overflow."""
    if q == 0:
        return -0.0 if negative_zero else 0.0
    sign = -1.0 if q < 0 else 1.0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()          # 2^(e-1) < q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1                                                         # now 2^e <= q < 2^(e+1)
    e = max(e, -126)                                                   # subnormals share the exponent -126
    quantum = Fraction(2) ** (e - 23)
    n = q / quantum
    lo = n.numerator // n.denominator
    rest = n - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo & 1):
        lo += 1
    value = lo * quantum
    if value >= Fraction(2) ** 128:
        return sign * math.inf
    return sign * float(value)                                         # exact: 24 bits, exponent within a double's


def _special(*xs):
    return any(not math.isfinite(x) for x in xs)


def _add(a, b):
    if _special(a, b) or Fraction(a) + Fraction(b) == 0:
        return a + b                         # IEEE: inf, NaN and the sign of an exact zero sum, as in any width
    return round_f32(Fraction(a) + Fraction(b))


def _mul(a, b):
    if _special(a, b) or a == 0.0 or b == 0.0:
        return a * b
    return round_f32(Fraction(a) * Fraction(b), negative_zero=(a < 0) != (b < 0))


def _div(a, b):
    if _special(a, b) or a == 0.0 or b == 0.0:
        if b == 0.0:
            if a != a or a == 0.0:
                return math.nan
            return math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b
    return round_f32(Fraction(a) / Fraction(b), negative_zero=(a < 0) != (b < 0))


def update_exact(o, sdf, w, d):
    """calculateTsdf given the sdf, every operation exact and rounded once by round_f32: (w', d') as Python floats."""
    sdf, w, d = float(sdf), float(w), float(d)
    trunc, max_weight, dropoff, sparsity = float(o.trunc), float(o.max_weight), float(o.dropoff), float(o.sparsity)
    uw = 1.0
    uw = _mul(uw, _div(_add(trunc, sdf), _add(trunc, -dropoff)) if dropoff > 0 else 1.0)
    uw = 0.0 if uw < 0.0 else uw
    uw = _mul(uw, sparsity if (sparsity > 0 and abs(sdf) < trunc) else 1.0)
    nw = _add(w, uw)
    if abs(nw) < float(NEAR_ZERO):
        return w, d
    ns = _div(_add(_mul(sdf, uw), _mul(d, w)), nw)
    if ns > 0.0:
        d1 = ns if ns < trunc else trunc
    else:
        d1 = ns if -trunc < ns else -trunc
    return (max_weight if max_weight < nw else nw), d1


def same(a, b):
    """Bit-for-bit equality of float32 values, any NaN equal to any NaN (the reference does not define the payload)."""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
