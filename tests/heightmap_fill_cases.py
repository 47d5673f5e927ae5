"""Scenes of the flood-fill heightmap tests (CPU restatement and device) -- TEST INFRASTRUCTURE.  Source voxels are
written directly (a hit: hit_value, a miss: miss_value, as integrateHit / integrateMiss leave a fresh voxel), so the same
chunks feed tests/heightmap_fill_ref.py and, uploaded, the device map.

multi_level_scene()  populateMultiLevelMap of the reference (tests/ohmtestheightmap/HeightmapTests.cpp:106-295) with the
                     oracle's key maths: a floor, a platform, a ramp on two sides, a virtual ramp on a third and a
                     shallower virtual ramp that hides one real ramp
flat_floor()         a flat floor with holes
fill_cases()         every (id, Scene, Params) the formulations are compared on"""
import numpy as np

from oracle.oracle import OracleMap, lib as _olib
from heightmap_ref import Params, Source

HIT = np.float32(_olib.oracle_probability_to_value(0.9))
MISS = np.float32(_olib.oracle_probability_to_value(0.45))
INF32 = np.float32(np.inf)


class Scene:
    """Occupancy (and mean) by global voxel coordinate g = region * dim + local."""

    def __init__(self, resolution, dim, mean=False):
        self.resolution = float(resolution)
        self.dim = tuple(int(v) for v in dim)
        self.with_mean = bool(mean)
        self.chunks = {}
        self.om = OracleMap(self.resolution, self.dim)

    def region(self, r):
        n = self.dim[0] * self.dim[1] * self.dim[2]
        c = self.chunks.setdefault(tuple(int(v) for v in r), {"occupancy": np.full(n, np.inf, dtype=np.float32)})
        if self.with_mean and "mean" not in c:
            c["mean"] = np.zeros(2 * n, dtype=np.uint32)
        return c

    def _at(self, g):
        r = tuple(g[a] // self.dim[a] for a in range(3))
        l = tuple(g[a] % self.dim[a] for a in range(3))
        return r, l[0] + l[1] * self.dim[0] + l[2] * self.dim[0] * self.dim[1]

    def get(self, g):
        r, vi = self._at(g)
        c = self.chunks.get(r)
        return INF32 if c is None else np.float32(c["occupancy"][vi])

    def put(self, g, value, mean=None):
        """Writing creates the region, as a mutable ohm::Voxel does."""
        r, vi = self._at(g)
        c = self.region(r)
        c["occupancy"][vi] = value
        if mean is not None:
            c["mean"][2 * vi], c["mean"][2 * vi + 1] = mean

    def key(self, point):
        """voxelKey(point) as a global voxel coordinate."""
        region, local = self.om.voxel_key(point)
        return [region[a] * self.dim[a] + local[a] for a in range(3)]

    def centre(self, g):
        return self.om.voxel_centre([g[a] // self.dim[a] for a in range(3)], [g[a] % self.dim[a] for a in range(3)])

    def is_occupied(self, g):
        v = self.get(g)
        return bool(v != INF32 and v >= 0.0)

    def is_free(self, g):
        return bool(self.get(g) < 0.0)

    def source(self):
        return Source(self.resolution, self.dim, self.chunks, 0.0, has_mean=self.with_mean)

    def permuted(self, up_axis):
        """The scene turned so that `up_axis` (ohm::UpAxis, -3 .. 2) is up: z onto the axis (mirrored for a negative
        one), x and y onto the other two in order."""
        idx = up_axis if up_axis >= 0 else -up_axis - 1
        others = [c for c in range(3) if c != idx]
        dim = [0, 0, 0]
        dim[idx], dim[others[0]], dim[others[1]] = self.dim[2], self.dim[0], self.dim[1]
        out = Scene(self.resolution, dim, self.with_mean)
        for region, c in self.chunks.items():
            occupancy = np.asarray(c["occupancy"])
            for vi in np.nonzero(occupancy != INF32)[0]:
                vi = int(vi)
                l = (vi % self.dim[0], (vi // self.dim[0]) % self.dim[1], vi // (self.dim[0] * self.dim[1]))
                g = [region[a] * self.dim[a] + l[a] for a in range(3)]
                to = [0, 0, 0]
                to[idx] = g[2] if up_axis >= 0 else self.dim[2] - 1 - g[2]
                to[others[0]], to[others[1]] = g[0], g[1]
                out.put(to, occupancy[vi])
            # (a region without an observed voxel still exists)
            r = [0, 0, 0]
            r[idx] = region[2] if up_axis >= 0 else -region[2]
            r[others[0]], r[others[1]] = region[0], region[1]
            out.region(r)
        return out

    def point_permuted(self, point, up_axis):
        idx = up_axis if up_axis >= 0 else -up_axis - 1
        others = [c for c in range(3) if c != idx]
        out = [0.0, 0.0, 0.0]
        out[idx] = point[2] if up_axis >= 0 else -point[2]
        out[others[0]], out[others[1]] = point[0], point[1]
        return tuple(out)


def _box(lo, hi):
    """ohm::KeyRange iteration: every key of the closed box."""
    for z in range(lo[2], hi[2] + 1):
        for y in range(lo[1], hi[1] + 1):
            for x in range(lo[0], hi[0] + 1):
                yield (x, y, z)


def multi_level_scene(resolution=0.1, dim=(32, 32, 32), map_half_extents=6.0, platform_half_extents=2.0,
                      platform_height=1.5, virtual_surfaces=True, occlusion=True):
    """(Scene, surface, virtual_surface, seam): populateMultiLevelMap (HeightmapTests.cpp:106-295) and the three key
    sets of its HeightmapGeneratedInfo, keys as global voxel tuples."""
    s = Scene(resolution, dim)
    surface, virtual, seam = set(), set(), set()
    m, p, h = map_half_extents, platform_half_extents, platform_height

    def hit(g):
        s.put(g, HIT)
        surface.add(tuple(g))

    def try_make_virtual(g):
        """tryMakeVirtual (:69-95): integrateMiss, then, where the voxel is free, the occupied voxels below are eaten."""
        v = s.get(g)
        s.put(g, MISS if v == INF32 else np.float32(v + MISS))
        if not s.is_free(g):
            return
        virtual.add(tuple(g))
        if occlusion:
            key = list(g)
            while True:
                key[2] -= 1
                if s.is_occupied(key):
                    s.put(key, INF32)
                    surface.discard(tuple(key))
                else:
                    s.put(key, s.get(key))  # setKey of a mutable voxel creates the region
                if not s.centre(key)[2] > 0:
                    break

    for g in _box(s.key((-m, -m, 0.0)), s.key((m, m, 0.0))):
        hit(g)
    for g in _box(s.key((-p, -p, h)), s.key((p, p, h))):
        hit(g)
    side_min = [s.key((-p, -p, 0.0)), s.key((p, -p, 0.0))]
    side_max = [s.key((-p, -p, h)), s.key((p, -p, h))]
    for k in side_min:
        k[2] += 1
    y_count = int((2 * p) / resolution)
    for i in range(2):
        x_offset = -(side_max[i][2] - side_min[i][2] + 1)  # KeyRange::range(): the closed interval
        first_row = True
        for ref in _box(side_min[i], side_max[i]):
            key = list(ref)
            key[0] += x_offset * (1 if i == 0 else -1)
            for g in _box(key, [key[0], key[1] + y_count, key[2]]):
                hit(g)
                if first_row:
                    seam.add((g[0], g[1], g[2] - 1))
            x_offset += 1
            first_row = False
    if virtual_surfaces:
        ramp_lo, ramp_hi = s.key((-p, -p, 0.0)), s.key((-p, -p, h))
        x_count = int((2 * p) / resolution)
        y_offset = -(ramp_hi[2] - ramp_lo[2] + 1)
        for ref in _box(ramp_lo, ramp_hi):
            key = list(ref)
            key[1] += y_offset
            for g in _box(key, [key[0] + x_count, key[1], key[2]]):
                try_make_virtual(list(g))
            y_offset += 1
        x_offset = -2 * (side_max[0][2] - side_min[0][2] + 1)
        for ref in _box(side_min[0], side_max[0]):
            for _ in range(2):
                key = list(ref)
                key[0] += x_offset
                for g in _box(key, [key[0], key[1] + y_count, key[2]]):
                    try_make_virtual(list(g))
                x_offset += 1
    # :264-292 a virtual surface voxel is free with an unobserved (or no) voxel below
    virtual = {g for g in virtual if s.is_free(g) and s.get((g[0], g[1], g[2] - 1)) == INF32}
    return s, surface, virtual, seam


def scaled_multi_level(up_axis=2):
    """The multi-level scene at a third of its size in 16^3 regions (floor 41 x 41 voxels, platform at 0.5 m), turned to
    `up_axis`, with the Params of testHeightmapVirtualSurface scaled alike."""
    s, _, _, _ = multi_level_scene(0.1, (16, 16, 16), 2.0, 0.65, 0.5)
    reference = (0.0, 0.0, 1.1 * 0.5)
    if up_axis != 2:
        reference = s.point_permuted(reference, up_axis)
        s = s.permuted(up_axis)
    return s, Params(0.1, 0.0, up_axis=up_axis, reference_pos=reference, ceiling=0.7, virtual_surface=True)


def flat_floor(n=24, dim=(8, 8, 8), resolution=0.5, level=6, holes=(), mean=False, first=-8):
    """An n x n floor of occupied voxels at global z `level` with a free voxel above each, from global x = y = `first`;
    `holes`: (x, y) columns that hold only the free voxel (a virtual surface, or nothing)."""
    s = Scene(resolution, dim, mean)
    for y in range(first, first + n):
        for x in range(first, first + n):
            if (x, y) not in holes:
                s.put((x, y, level), HIT)
            s.put((x, y, level + 1), MISS)
    return s


FLAT_HOLES = tuple((x, y) for x in range(2, 6) for y in range(2, 6)) + ((-3, -3), (10, -7))
FLAT_SEEDS = {"middle": (1.3, 0.8, 1.2), "corner": (-3.9, -3.9, 1.2), "outside": (40.0, -25.0, 9.0),
              "hole": (-0.3, -0.3, 1.2)}  # global voxel (3, 3) is a hole: (-0.3 + 2) / 0.5


def flat_cases():
    """The flat 24 x 24 floor at 1 m in 8^3 regions of 0.5 m voxels (regions -1 .. 1 on x and y, region 0 on z, the z
    range opened to the missing regions above and below by the cull box): 4 seeds x 3 virtual-surface settings x 2
    floor / ceiling limits."""
    scene = flat_floor(holes=FLAT_HOLES)
    for seed_name, seed in FLAT_SEEDS.items():
        for virtual_name, virtual, promote in (("real", False, False), ("virtual", True, False), ("promote", True, True)):
            for limit in (0, 2):
                p = Params(0.5, 0.0, reference_pos=seed, cull_min=(0.0, 0.0, -5.9), cull_max=(0.0, 0.0, 5.9),
                           floor=limit * 0.5, ceiling=limit * 0.5, virtual_surface=virtual,
                           promote_virtual_below=promote)
                yield "flat-%s-%s-%d" % (seed_name, virtual_name, limit), scene, p


def mean_scene():
    """A 12 x 12 floor with the mean layer: means pushed towards a cell edge, every third column's across its middle."""
    s = flat_floor(n=12, dim=(8, 8, 8), resolution=0.5, level=3, mean=True, first=-4)
    for y in range(-4, 8):
        for x in range(-4, 8):
            ix = 1000 if (x + y) % 3 == 0 else (20 if (x + y) % 3 == 1 else 511)
            iy = 900 if x % 2 else 100
            s.put((x, y, 3), HIT, mean=(ix | (iy << 10) | (511 << 20) | (1 << 31), 1 + (x * 7 + y) % 5))
    return s


def fill_cases():
    """(id, Scene, Params) of every case."""
    for case in flat_cases():
        yield case
    for up_axis in (-3, -2, -1, 0, 1, 2):
        scene, p = scaled_multi_level(up_axis)
        yield "multi-level-up%d" % up_axis, scene, p
    scene = mean_scene()
    yield "mean-coarse", scene, Params(1.0, 0.0, reference_pos=(0.1, 0.1, 0.0), origin=(0.5, 0.5, 0.0))
    yield "mean-same", scene, Params(0.5, 0.0, reference_pos=(0.1, 0.1, 0.0), origin=(0.25, 0.25, 0.0), region_size=16)
    yield "mean-coarse-cut", scene, Params(1.0, 0.0, reference_pos=(0.1, 0.1, 0.0), origin=(0.25, 0.25, 0.0))
