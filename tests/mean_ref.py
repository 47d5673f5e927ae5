"""An exact model of the voxel mean update (test infrastructure), one axis at a time.

The packed mean is a running average that is re-quantised to a 10-bit cell per axis after every sample
(ohm/VoxelMeanCompute.h:69-92, 102-122, 134-152, instantiated with Vec3 = dvec3 and coord_real = double):

    mr     = res / 1023.0                    the cell size
    offset = double(0.5f) * res
    m      = cell * mr - offset              decode; the used bit (31) is NOT looked at (the reference tests a constant)
    inv    = 1.0 / double(u32(count + 1))    the sum wraps at 2^32: 1 / 0 = +inf for count = 0xffffffff
    m     += (v - m) * inv
    cell'  = clamp(int(floor((m + offset) / mr + 0.5)), 0, 1023)
    coord' = cells | 1 << 31, count' = u32(count + 1)

with v = end - centre one double subtraction and the centre from ohm/OccupancyMap.h:763-776.  A Python float is an IEEE
double and Python never contracts a * b + c, so axis_ref() below IS that chain, one rounding per operation: the bit-level
statement of what the reference computes on the host it runs on.  The double -> int conversion follows x86 (cvttsd2si):
NaN, the infinities and anything outside the int range give INT_MIN, which the clamp turns into cell 0.

The independent check.  axis_exact() evaluates the same quantity in rationals from the same double inputs (m, v, mr,
offset as the doubles they are, 1 / (n + 1) exact, no intermediate rounding):

    t_exact = (m + (v - m) / (n + 1) + offset) / mr + 1 / 2

and Exact.judge() bounds |t_double - t_exact| for ANY evaluation that rounds each operation once (in any of the forms
the mutants below take: fused or not, divide or multiply by a rounded reciprocal).  With u = 2^-53 (half an ulp of x
is at most u |x|), first order in u, the roundings are

    d  = v - m                  u |d|                    }  relative to p = d / (n + 1):
    inv (or the divide)         u |inv|                  }  3 u |p|
    p  = d * inv                u |p|                    }
    m' = m + p                  u |m'|
    s  = m' + offset            u |s|
    q  = s / mr  (or s * (1 / mr): two roundings)        2 u |q|    -- absolute errors of s are divided by mr first
    t  = q + 0.5                u |t|

    E = ((3 |p| + |m'| + |s|) / mr + 2 |q| + |t|) * u * (1 + 2^-20)

where the magnitudes are the exact ones and the last factor covers every second-order term (each is below 8 u of a
first-order one).  E is at most 7.7e3 u = 8.6e-13 of a cell (E_MAX).  A case whose t_exact is further than E from the
nearest integer is FORCED: every correct evaluation stores floor(t_exact).  Inside E the case is a NEAR-TIE and only the
reference's own chain (axis_ref) decides.  Nothing here is tuned to an implementation.

Mutants: the same chain with one change each (MUTANTS); where the change is "one rounding instead of two" the single
rounding is taken from the exact rational.  `closed_centre` and `order` act outside the axis chain: centre_closed() and
the order of a case's samples."""
import math
import struct
from fractions import Fraction

POSITIONS = 1023
USED_BIT = 1 << 31
INT_MIN = -(1 << 31)
U = Fraction(1, 1 << 53)
SLACK = 1 + Fraction(1, 1 << 20)
E_MAX = Fraction(1, 10 ** 12)        # above every E: (3 * 1023 + 512 + 1023 + 2 * 1023 + 1024) u = 8.6e-13

AXIS_MUTANTS = ("fma", "div_count", "recip_grid", "f32_inv", "signed_count", "wide_count", "sat_int")
MUTANTS = AXIS_MUTANTS + ("used_bit", "closed_centre", "order")


def f32(x):
    """x rounded to float32 (as a double)."""
    return struct.unpack("f", struct.pack("f", x))[0]


HALF = f32(0.5)


def grid(res):
    """(mr, offset) as the reference forms them."""
    return res / float(POSITIONS), HALF * res


def decode(cell, res):
    mr, offset = grid(res)
    return cell * mr - offset


def cells_of(coord):
    return coord & POSITIONS, (coord >> 10) & POSITIONS, (coord >> 20) & POSITIONS


def pack(cells):
    return cells[0] | (cells[1] << 10) | (cells[2] << 20) | USED_BIT


def host_int(x, saturate=False):
    """double -> int as cvttsd2si does it (saturate: as a saturating conversion would, NaN -> 0)."""
    if x != x:
        return 0 if saturate else INT_MIN
    if x >= 2147483648.0:
        return (1 << 31) - 1 if saturate else INT_MIN
    if x < -2147483648.0:
        return INT_MIN
    return int(x)                      # truncation; exact for a finite in-range double


def _floor(x):
    return float(math.floor(x)) if math.isfinite(x) else x


def _divide(a, b):
    """IEEE a / b for b == 0 too (Python raises there)."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def axis_ref(cell, count, v, res, mutant=None, mean=None):
    """One axis of subVoxelUpdate: the new cell.  `mean` overrides the decoded mean (the used_bit mutant)."""
    mr, offset = grid(res)
    m = cell * mr - offset if mean is None else mean
    n1 = (count + 1) & 0xffffffff
    if mutant == "wide_count":
        n1 = count + 1
    elif mutant == "signed_count":
        n1 = n1 - (1 << 32) if n1 >= (1 << 31) else n1
    d = v - m
    if mutant == "div_count":
        step = _divide(d, float(n1))
        m = m + step
    else:
        inv = _divide(1.0, float(n1))
        if mutant == "f32_inv":
            inv = f32(inv)
        if mutant == "fma" and math.isfinite(inv) and math.isfinite(d):
            m = float(Fraction(m) + Fraction(d) * Fraction(inv))           # one rounding
        else:
            m = m + d * inv
    s = m + offset
    q = s * (1.0 / mr) if mutant == "recip_grid" else s / mr
    pos = host_int(_floor(q + 0.5), saturate=mutant == "sat_int")
    return min(max(pos, 0), POSITIONS)


def coord_ref(v, res):
    """subVoxelCoord (ohm/VoxelMeanCompute.h:69-92): the pattern of an offset v[3] from the voxel centre."""
    mr, offset = grid(res)
    return pack([min(max(host_int(_floor((x + offset) / mr + 0.5)), 0), POSITIONS) for x in v])


def update_ref(coord, count, end, centre, res, mutant=None):
    """(coord', count') after one sample at `end` in the voxel centred on `centre` (three axes)."""
    zero = mutant == "used_bit" and not coord & USED_BIT
    axis_mutant = mutant if mutant in AXIS_MUTANTS else None
    cells = [axis_ref(c, count, end[a] - centre[a], res, axis_mutant, 0.0 if zero else None)
             for a, c in enumerate(cells_of(coord))]
    return pack(cells), (count + 1) & 0xffffffff


def run_ref(coord, count, ends, centre, res, mutant=None):
    """States after each sample of `ends` in order: [(coord, count), ...]."""
    out = []
    for end in ends:
        coord, count = update_ref(coord, count, end, centre, res, mutant)
        out.append((coord, count))
    return out


def centre_ref(origin, region_dim, res, region, local):
    """One axis of OccupancyMap::voxelCentreGlobal in the reference's order (region_dim is the region's edge in metres,
    dim * res as the map computes it; the region coordinate goes through a float, exact for an int16)."""
    v = f32(float(region))
    v = v * region_dim
    v = v - 0.5 * region_dim
    v = v + origin
    v = v + float(local) * res
    v = v + 0.5 * res
    return v


def centre_closed(origin, dim, res, region, local):
    """The closed_centre mutant: origin + (g + 0.5) * res with g the voxel's global index (region `region` spans the
    voxels region * dim - dim / 2 ... of an axis; dim is even here)."""
    return origin + (float(region * dim - dim // 2 + local) + 0.5) * res


class Exact:
    """t_exact of one axis as a linear function of the double v, for scanning: t = a + v * b."""

    def __init__(self, cell, count, res):
        mr, offset = grid(res)
        self.mr, self.offset = Fraction(mr), Fraction(offset)
        self.m = Fraction(cell * mr - offset)
        self.n1 = count + 1
        self.wraps = (self.n1 & 0xffffffff) == 0
        n1 = Fraction(max(self.n1, 1))
        self.b = 1 / (n1 * self.mr)
        self.a = (self.m - self.m / n1 + self.offset) / self.mr + Fraction(1, 2)

    def t(self, v):
        return self.a + Fraction(v) * self.b

    def solve(self, t):
        """The rational v with t_exact = t."""
        return (Fraction(t) - self.a) / self.b

    def judge(self, v, far=None):
        """(t_exact, floor cell clamped, margin, E); E is left None where the margin is above `far`."""
        t = self.t(v)
        fl = t.numerator // t.denominator
        frac = t - fl
        margin = min(frac, 1 - frac)
        if far is not None and margin > far:
            return t, min(max(fl, 0), POSITIONS), margin, None
        p = (Fraction(v) - self.m) / self.n1
        m1 = self.m + p
        s = m1 + self.offset
        q = s / self.mr
        bound = ((3 * abs(p) + abs(m1) + abs(s)) / self.mr + 2 * abs(q) + abs(t)) * U * SLACK
        return t, min(max(fl, 0), POSITIONS), margin, bound


def axis_exact(cell, count, v, res):
    """-> (t_exact, floor(t_exact) clamped to a cell, margin, E), or None at the wrap (count = 0xffffffff), where the
    reference divides by zero and no exact value exists."""
    ex = Exact(cell, count, res)
    return None if ex.wraps else ex.judge(v)


def update_exact(coord, count, end, centre, res):
    """Per axis axis_exact() of one sample; None at the wrap."""
    return [axis_exact(c, count, end[a] - centre[a], res) for a, c in enumerate(cells_of(coord))]


def forced(judged):
    return judged is not None and judged[2] > judged[3]
