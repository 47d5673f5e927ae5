"""Shapes, bit patterns and planted map pairs for the map-compare tests (tests/test_compare_ref.py on the CPU,
tests/test_gpu_compare.py on the device).  Plain numpy: nothing here needs a device."""
import numpy as np

import compare_ref as R

NAN, NAN2, INF, NINF = 0x7fc00000, 0x7fc00001, 0x7f800000, 0xff800000
FMAX, NFMAX, PZ, NZ = 0x7f7fffff, 0xff7fffff, 0x00000000, 0x80000000
ONE, ONE_UP, MINUS_ONE = 0x3f800000, 0x3f800001, 0xbf800000
SUB1, MIN_NORMAL, MIN_NORMAL_UP = 0x00000001, 0x00800000, 0x00800001

# K4, derived by hand from compareDatum (CompareMaps.cpp:58-75: swap when ref > val; pass = hi == lo || hi - lo <= eps)
# and the byte comparison (:313-318).  (name, eval bits, ref bits, eps bits or None for "no tolerance", passes)
TRUTH_F32 = [
    ("identical NaN bits pass the byte comparison", NAN, NAN, None, True),
    ("identical NaN bits fail under eps = +inf", NAN, NAN, INF, False),      # NaN == NaN false, NaN - NaN <= inf false
    ("identical NaN bits fail under eps = 0", NAN, NAN, PZ, False),
    ("different NaN payloads fail the byte comparison", NAN, NAN2, None, False),
    ("NaN in eval fails under eps = +inf", NAN, ONE, INF, False),
    ("NaN in ref fails under eps = +inf", ONE, NAN, INF, False),
    ("NaN against a number fails the byte comparison", NAN, ONE, None, False),
    ("+0 against -0 passes with a tolerance", PZ, NZ, PZ, True),             # hi == lo
    ("-0 against +0 passes with a tolerance", NZ, PZ, PZ, True),
    ("+0 against -0 fails the byte comparison", PZ, NZ, None, False),
    ("+inf against itself passes at eps = 0", INF, INF, PZ, True),           # hi == lo, although inf - inf is NaN
    ("-inf against itself passes at eps = 0", NINF, NINF, PZ, True),
    ("+inf against itself passes the byte comparison", INF, INF, None, True),
    ("+inf against FLT_MAX fails at eps = FLT_MAX", INF, FMAX, FMAX, False),  # inf - FLT_MAX = inf
    ("FLT_MAX against +inf fails at eps = 0", FMAX, INF, PZ, False),
    ("+inf against FLT_MAX passes only at eps = +inf", INF, FMAX, INF, True),
    ("+inf against -inf fails at eps = FLT_MAX", INF, NINF, FMAX, False),
    ("a NaN eps passes equal values", ONE, ONE, NAN, True),
    ("a NaN eps fails values one ulp apart", ONE_UP, ONE, NAN, False),
    ("a negative eps passes equal values", ONE, ONE, MINUS_ONE, True),
    ("a negative eps fails values one ulp apart", ONE, ONE_UP, MINUS_ONE, False),
    ("one subnormal apart fails at eps = 0", MIN_NORMAL_UP, MIN_NORMAL, PZ, False),   # the difference is 2^-149, not 0
    ("one subnormal apart passes at eps = that subnormal", MIN_NORMAL, MIN_NORMAL_UP, SUB1, True),
    ("0 against the smallest subnormal fails at eps = 0", PZ, SUB1, PZ, False),
    ("0 against the smallest subnormal passes at eps = it", SUB1, PZ, SUB1, True),
    ("FLT_MAX against -FLT_MAX overflows: fails at eps = FLT_MAX", FMAX, NFMAX, FMAX, False),
    ("FLT_MAX against -FLT_MAX passes at eps = +inf", NFMAX, FMAX, INF, True),
    ("one ulp apart at 1 passes at eps = that ulp", ONE_UP, ONE, 0x34000000, True),   # 2^-23
    ("one ulp apart at 1 fails just below", ONE, ONE_UP, 0x33ffffff, False),
]
TRUTH_U32 = [
    ("0 against 0xffffffff fails at eps = 0", 0, 0xffffffff, 0, False),
    ("0xffffffff against 0 fails at eps = 0xfffffffe", 0xffffffff, 0, 0xfffffffe, False),
    ("0 against 0xffffffff passes at eps = 0xffffffff", 0, 0xffffffff, 0xffffffff, True),   # no wrap: hi - lo
    ("0xffffffff against 0 passes at eps = 0xffffffff", 0xffffffff, 0, 0xffffffff, True),
    ("5 against 7 passes at eps = 2", 5, 7, 2, True),
    ("7 against 5 fails at eps = 1", 7, 5, 1, False),
    ("equal words pass without a tolerance", 0x80000000, 0x80000000, None, True),
    ("a float's 1.0 as a u32 eps", 0x3f800000, 0, 0x3f800000, True),
    ("a float's 1.0 as a u32 eps, one more", 0x3f800001, 0, 0x3f800000, False),
]

SMALL = (8, 8, 8)        # 512 voxels: a chunk shorter than a wave's share
TWO_CHUNKS = (32, 16, 16)  # 8192 voxels: two chunks of 4096
TILED = (64, 32, 32)     # 65536 voxels: two tiles of 32768
SMALL_REGIONS = [(x, y, 0) for y in (-1, 0, 1) for x in (-1, 0, 1)]

LAYER_DTYPE = {name: (np.float32 if R.LAYOUT[name][1] else np.uint32) for name in R.LAYOUT}


def voxels_of(dims):
    return dims[0] * dims[1] * dims[2]


def base_block(layer, dims, seed):
    """A block of plausible, NaN-free values: (voxels, members) uint32."""
    rng = np.random.default_rng(seed)
    members = len(R.LAYOUT[layer][0])
    n = voxels_of(dims)
    if R.LAYOUT[layer][1]:
        return rng.uniform(-2.0, 3.5, size=(n, members)).astype(np.float32).view(np.uint32)
    return rng.integers(0, 1 << 20, size=(n, members), dtype=np.uint32)


def nudge(block, layer, index, member=0):
    """One member of one voxel moved off its value (a finite float by 0.25, a word by 3)."""
    if R.LAYOUT[layer][1]:
        block.view(np.float32)[index, member] += np.float32(0.25)
    else:
        block[index, member] += np.uint32(3)


def planted_pair(layer, dims, regions, plants, seed=7):
    """(eval chunks, ref chunks): equal blocks, then eval nudged at plants = [(region, voxel index, member)]."""
    ref = {r: base_block(layer, dims, seed + i) for i, r in enumerate(regions)}
    ev = {r: b.copy() for r, b in ref.items()}
    for region, index, member in plants:
        nudge(ev[region], layer, index, member)
    return ev, ref


def edge_plants(layer, dims, regions):
    """Voxel 0 and the last voxel of the first and last region in order, the wave edge 63 / 64 and -- where the region has
    one -- the chunk edge 4095 / 4096; in a multi-member layer the last member only."""
    order = R.region_order(regions)
    n = voxels_of(dims)
    member = len(R.LAYOUT[layer][0]) - 1
    plants = [(order[0], 0, member), (order[0], n - 1, member), (order[-1], 0, 0), (order[-1], n - 1, member),
              (order[len(order) // 2], 63, member), (order[len(order) // 2], 64, 0)]
    if n > 4096:
        plants += [(order[0], 4095, member), (order[0], 4096, member)]
    return plants


def truth_pair(layer, dims, region=(0, 0, 0)):
    """The f32 truth table planted in member 0 of consecutive voxels from voxel 60 on (across the wave edge): (eval
    chunks, ref chunks, [(voxel index, row)]).  Rows with a tolerance come first, then those without."""
    ev = {region: base_block(layer, dims, 3)}
    ref = {region: ev[region].copy()}
    rows = [row for row in TRUTH_F32 if row[3] is not None] + [row for row in TRUTH_F32 if row[3] is None]
    placed = []
    for i, row in enumerate(rows):
        ev[region][60 + i, 0], ref[region][60 + i, 0] = row[1], row[2]
        placed.append((60 + i, row))
    return ev, ref, placed


def fan_rays(n, seed, reach=1.4):
    """n rays from near the origin to points on a shell of radius <= reach: (2n, 3) float64, origin / end pairs."""
    rng = np.random.default_rng(seed)
    ends = rng.normal(size=(n, 3))
    ends *= (reach * rng.uniform(0.5, 1.0, size=(n, 1))) / np.linalg.norm(ends, axis=1, keepdims=True)
    rays = np.empty((2 * n, 3))
    rays[0::2] = rng.uniform(-0.02, 0.02, size=(n, 3))
    rays[1::2] = ends
    return rays
