"""-m gpu: the binning pass (k_ray_bin, forEachBinSegment) on the rays that take each of its routes.

The pass builds a ray's segment records with a step count per axis at every region entry: an arithmetic estimate whose
ray-invariant tests are evaluated once per ray, and stepsBefore()'s exact route for everything the estimate cannot vouch
for.  A wrong count, entry time or flag in a record moves voxel visits, so the maps are held bit for bit to the CPU
oracle (oracle.oracle.OracleMap), and the batch statistics to counts made from the oracle: its visit counter and, for
ray_region_segments, the runs of equal regions in its per-ray voxel sequence (oracle_walk_segment_keys).

Ray families (a few thousand rays each, through several regions): one and two axes without steps, axis-parallel rays,
start points on voxel and region faces, 45 degree rays from voxel centres (every region entry is an exact tie with
another axis' step, so the estimate is a whole number and the exact route has to decide), nearly axis-parallel rays
whose one transverse step has a delta 1e8 ... 1e12 times the main axis', zero-length rays and rays below the walk's
1e-3 m length epsilon.  Then every combination of the four ray flags that change the segments, the clip filter moving
end points, regions of 16^3 and 20 x 12 x 7 (the instantiation that is not restricted to power-of-two edges), one batch
large enough for the large LDS-table instantiation, and two consecutive batches (the second is binned speculatively)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from ohm_amd import GpuMap, OccupancyMap, RayFlag
from oracle.oracle import Key, lib as oracle_lib
from parity import assert_parity, compare_maps, make_oracle

pytestmark = pytest.mark.gpu

RES = 0.1
END_AS_FREE = int(RayFlag.kRfEndPointAsFree)
EXCLUDE_ORIGIN = int(RayFlag.kRfExcludeOrigin)
EXCLUDE_SAMPLE = int(RayFlag.kRfExcludeSample)
EXCLUDE_RAY = int(RayFlag.kRfExcludeRay)
WALK_EXCLUDE_END = 2  # ORACLE_WALK_EXCLUDE_END (oracle/ohm_oracle.h)
KEY_DTYPE = np.dtype([("region", "<i2", (3,)), ("local", "u1", (3,)), ("pad", "u1")])
# BatchRun::prepare(): 256-ray binning workgroups -- the large LDS table -- from 2 x 256 workgroups of them on
LARGE_TABLE_RAYS = 131072


def _pairs(starts, ends):
    out = np.empty((2 * starts.shape[0], 3), dtype=np.float64)
    out[0::2] = starts
    out[1::2] = ends
    return out


def _centres(rng, n, span=60):
    """Voxel centres of a default map (origin 0, 32^3 regions: voxel faces at whole multiples of RES)."""
    return (rng.integers(-span, span, size=(n, 3)) + 0.5) * RES


def rays_generic(n=3000, seed=11, reach=7.0):
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-2.0, 2.0, size=(n, 3))
    return _pairs(starts, starts + rng.uniform(-reach, reach, size=(n, 3)))


def rays_zero_step_axes(n=3000, seed=12):
    """Start and end in the same voxel layer on one axis (first half) or on two axes (second half)."""
    rng = np.random.default_rng(seed)
    starts = _centres(rng, n) + rng.uniform(-0.04, 0.04, size=(n, 3))
    ends = starts + rng.uniform(-7.0, 7.0, size=(n, 3))
    for i in range(n):
        axes = rng.permutation(3)[:1 if i < n // 2 else 2]
        ends[i, axes] = starts[i, axes] + rng.uniform(-0.005, 0.005, size=axes.size)
    return _pairs(starts, ends)


def rays_axis_parallel(n=3000, seed=13):
    """The direction is exactly zero on two axes (infinite step deltas there)."""
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-3.0, 3.0, size=(n, 3))
    ends = starts.copy()
    axis = rng.integers(0, 3, size=n)
    ends[np.arange(n), axis] += rng.uniform(-9.0, 9.0, size=n)
    return _pairs(starts, ends)


def rays_from_faces(n=3000, seed=14):
    """Start points exactly on voxel faces and on region faces (-1.6, 1.6, 4.8 ...), on one, two or all three axes."""
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-3.0, 3.0, size=(n, 3))
    voxel_face = rng.integers(-40, 40, size=(n, 3)) / 10.0
    region_face = (rng.integers(-2, 3, size=(n, 3)) * 32 - 16) / 10.0
    which = rng.integers(0, 3, size=(n, 3))  # 0: free, 1: voxel face, 2: region face
    which[np.all(which == 0, axis=1), 0] = 2
    starts = np.where(which == 1, voxel_face, np.where(which == 2, region_face, starts))
    return _pairs(starts, starts + rng.uniform(-6.0, 6.0, size=(n, 3)))


def rays_diagonal(n=3000, seed=15):
    """From a voxel centre along (+-1, +-1, 0), its permutations and (+-1, +-1, +-1), a whole number of voxels."""
    rng = np.random.default_rng(seed)
    starts = _centres(rng, n, span=40)
    signs = rng.choice([-1.0, 1.0], size=(n, 3))
    drop = rng.integers(0, 4, size=n)  # 3: keep all three axes
    signs[np.arange(n)[drop < 3], drop[drop < 3]] = 0.0
    steps = rng.integers(20, 90, size=(n, 1))
    return _pairs(starts, starts + signs * steps * RES)


def rays_nearly_axis_parallel(n=3000, seed=16):
    """Metres along one axis and one voxel-face crossing, 1e-12 ... 1e-8 m wide, on another."""
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-2.0, 2.0, size=(n, 3))
    ends = starts.copy()
    main = rng.integers(0, 3, size=n)
    side = (main + rng.integers(1, 3, size=n)) % 3
    rows = np.arange(n)
    ends[rows, main] += rng.choice([-1.0, 1.0], size=n) * rng.uniform(3.0, 9.0, size=n)
    face = rng.integers(-20, 20, size=n) / 10.0
    half = 10.0 ** rng.uniform(-12.0, -8.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    starts[rows, side] = face - half
    ends[rows, side] = face + half
    return _pairs(starts, ends)


def rays_short(n=3000, seed=17):
    """Zero-length rays, rays below the walk's length epsilon (some across a voxel face), and rays just above it."""
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-2.0, 2.0, size=(n, 3))
    near_face = rng.integers(-20, 20, size=(n, 3)) / 10.0 + rng.uniform(-2e-4, 2e-4, size=(n, 3))
    starts[n // 2:] = near_face[n // 2:]
    length = np.where(np.arange(n) % 3 == 0, 0.0, 10.0 ** rng.uniform(-6.0, -2.7, size=n))
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    return _pairs(starts, starts + direction * length[:, None])


def _clip_ends(rays, clip_range):
    """clipRayFilter (ohm/RayFilter.cpp:36-58) in its operation order: the end points the mapper walks to."""
    pairs = rays.reshape(-1, 2, 3)
    start, end = pairs[:, 0], pairs[:, 1]
    ray = end - start
    len2 = ray[:, 0] * ray[:, 0] + ray[:, 1] * ray[:, 1] + ray[:, 2] * ray[:, 2]
    clipped = len2 > clip_range * clip_range
    length = np.sqrt(len2)
    with np.errstate(invalid="ignore", divide="ignore"):
        moved = start + (ray / length[:, None]) * clip_range
    return _pairs(start, np.where(clipped[:, None], moved, end)), clipped


def oracle_segment_count(om, rays, flags, clip_range=None):
    """Ray-region segments of a batch from the oracle's walk: per ray, the runs of equal regions in the voxels of its ray
    part -- origin voxel included whatever kRfExcludeOrigin says (the walk kernel skips it inside the segment), end voxel
    only when it is part of the ray (kRfEndPointAsFree or a clipped end)."""
    if flags & EXCLUDE_RAY:
        return 0
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    clipped = np.zeros(rays.shape[0] // 2, dtype=bool)
    if clip_range is not None:
        rays, clipped = _clip_ends(rays, clip_range)
    pairs = rays.reshape(-1, 6)
    room = (np.abs(pairs[:, 3:] - pairs[:, :3]).sum(axis=1) / om.resolution).astype(np.int64) + 8
    offsets = np.concatenate([[0], np.cumsum(room)])
    keys = (Key * int(offsets[-1]))()
    base = C.addressof(keys)
    counts = np.zeros(pairs.shape[0], dtype=np.int64)
    dp = C.POINTER(C.c_double)
    address = pairs.ctypes.data
    for i in range(pairs.shape[0]):
        walk_flags = 0 if (flags & END_AS_FREE or clipped[i]) else WALK_EXCLUDE_END
        n = oracle_lib.oracle_walk_segment_keys(om.handle, C.cast(address + 48 * i, dp), C.cast(address + 48 * i + 24, dp),
                                                walk_flags, C.cast(base + C.sizeof(Key) * int(offsets[i]), C.POINTER(Key)), None, None,
                                                int(room[i]))
        assert n <= room[i], (i, n, room[i])
        counts[i] = n
    regions = np.frombuffer(keys, dtype=KEY_DTYPE)["region"]
    walked = np.nonzero(counts)[0]
    edges = np.zeros(len(keys) + 1, dtype=np.int64)  # +1 where a ray's keys begin, -1 behind its last
    np.add.at(edges, offsets[walked], 1)
    np.add.at(edges, offsets[walked] + counts[walked], -1)
    used = np.cumsum(edges[:-1]) > 0
    first = np.zeros(len(keys), dtype=bool)
    first[offsets[walked]] = True
    change = np.ones(len(keys), dtype=bool)
    change[1:] = np.any(regions[1:] != regions[:-1], axis=1)
    return int(np.count_nonzero(used & (first | change)))


def _check(batches, region=(32, 32, 32), flags=0, clip_range=None, origin=None):
    map_ = OccupancyMap(RES, region, layers=("occupancy",))
    if origin is not None:
        map_.setOrigin(origin)
    if clip_range is not None:
        map_.ray_filter = ("clip", clip_range)
    gm = GpuMap(map_)
    gm.setBatchCoalescing(0)  # every call its own device batch
    om = make_oracle(map_)
    for rays in batches:
        n_rays = rays.shape[0] // 2
        visits_before = om.visit_count()
        assert gm.integrateRays(rays, ray_update_flags=flags) == rays.shape[0]  # (points, like the reference)
        om.integrate_occupancy(rays, flags=flags)
        stats = gm.stats()
        want_segments = oracle_segment_count(om, rays, flags, clip_range)
        print("rays %d visits %d / %d segments %d / %d" % (n_rays, stats["voxel_visits"], om.visit_count() - visits_before,
                                                         stats["ray_region_segments"], want_segments))
        assert stats["rays_integrated"] == n_rays
        assert stats["voxel_visits"] == om.visit_count() - visits_before
        assert stats["ray_region_segments"] == want_segments
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy"], exact_float=True))
    gm.close()


FAMILIES = {"zero_step_axes": rays_zero_step_axes, "axis_parallel": rays_axis_parallel, "from_faces": rays_from_faces,
            "diagonal": rays_diagonal, "nearly_axis_parallel": rays_nearly_axis_parallel, "short": rays_short}


@pytest.mark.parametrize("flags", [0, END_AS_FREE])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_ray_families(gpu, family, flags):
    _check([FAMILIES[family]()], flags=flags)


@pytest.mark.parametrize("flags", [sum(c) for c in itertools.product((0, END_AS_FREE), (0, EXCLUDE_ORIGIN),
                                                                     (0, EXCLUDE_SAMPLE), (0, EXCLUDE_RAY))])
def test_every_flag_combination(gpu, flags):
    rays = np.concatenate([rays_generic(1500), rays_from_faces(500), rays_diagonal(500), rays_short(300)])
    _check([rays], flags=flags)


@pytest.mark.parametrize("flags", [0, EXCLUDE_ORIGIN])
def test_clip_filter_moves_end_points(gpu, flags):
    rays = np.concatenate([rays_generic(3000, reach=8.0), rays_axis_parallel(1000), rays_diagonal(500)])
    _check([rays], flags=flags, clip_range=4.0)


@pytest.mark.parametrize("region", [(16, 16, 16), (20, 12, 7)])
def test_other_region_sizes(gpu, region):
    rays = np.concatenate([rays_generic(2000), rays_from_faces(1000), rays_diagonal(1000), rays_zero_step_axes(1000),
                           rays_nearly_axis_parallel(500), rays_short(300)])
    _check([rays], region=region, origin=(0.03, -0.02, 0.01))
    _check([rays], region=region, flags=END_AS_FREE | EXCLUDE_ORIGIN)


def test_large_table_instantiation(gpu):
    """A batch above BatchRun::prepare()'s threshold for 256-ray workgroups; rays of 1-2 m keep the oracle quick."""
    n = LARGE_TABLE_RAYS + 1000
    rng = np.random.default_rng(21)
    starts = rng.uniform(-6.0, 6.0, size=(n, 3))
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    rays = _pairs(starts, starts + direction * rng.uniform(1.0, 2.0, size=(n, 1)))
    rays[2:2002] = rays_diagonal(1000)
    _check([rays])


def test_two_consecutive_batches(gpu):
    """The second batch of a map is binned before its plan summary has reached the host."""
    first = np.concatenate([rays_generic(3000, seed=31), rays_diagonal(500, seed=32)])
    second = np.concatenate([rays_generic(3000, seed=33), rays_from_faces(500, seed=34), rays_short(300, seed=35)])
    third = np.concatenate([rays_zero_step_axes(2000, seed=36), rays_nearly_axis_parallel(500, seed=37)])
    _check([first, second, third])
    _check([first, second, third], flags=END_AS_FREE)
