"""-m gpu: the per-chunk fixed cost of k_region_walk -- the segment ordering with replicated class counters, the direct
apply of single-chunk regions through its lean body (applyFullTile) and the tile flush of multi-chunk regions
(flushFullTile) -- against the CPU oracle.

Every case runs the same calls through a device map and the oracle (parity.make_oracle) and compares every region either
side knows, every layer, through uint32 views.  Coalescing is off: a call is a device batch.  The lean bodies serve a
plain occupancy batch without exclusion flags on a region that fills the walk's tile (32^3; 32 x 32 x 16 where
OHMHIP_WALK_HALF_VOXELS sends such regions to the half shape); everything else must still take the general form and
match too.

Counting is order independent, so a segment that the ordering loses or places twice shows as a voxel whose count -- and
with it its value after ONE batch on a fresh map -- is wrong."""
import numpy as np
import pytest

from ohm_amd import GpuMap, OccupancyMap, RayFlag
from parity import make_oracle
from test_gpu_mean_states import read_device

pytestmark = pytest.mark.gpu

F = np.float32
RES = 0.1


class Maps:
    """A device map whose region (0, 0, 0) is centred on the origin, and the oracle fed the same calls."""

    def __init__(self, monkeypatch, dims=(32, 32, 32), chunk=None, layers=("occupancy",), miss_value=None,
                 saturate=False, half_voxels=None):
        if half_voxels is None:                                                  # (read at map creation too)
            monkeypatch.delenv("OHMHIP_WALK_HALF_VOXELS", raising=False)
        else:
            monkeypatch.setenv("OHMHIP_WALK_HALF_VOXELS", str(half_voxels))
        for name in ("OHMHIP_CHUNK_SEGMENTS", "OHMHIP_MIN_CHUNK_SEGMENTS"):      # both are read at map creation
            if chunk is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(chunk))
        self.dims = tuple(dims)
        self.low = -0.5 * RES * np.array(dims, dtype=np.float64)
        self.map = OccupancyMap(RES, self.dims, layers=layers)
        if miss_value is not None:
            self.map.miss_value = float(miss_value)
        self.map.saturate_at_min_value = self.map.saturate_at_max_value = bool(saturate)
        self.gm = GpuMap(self.map, region_capacity=64)
        self.gm.setBatchCoalescing(0)
        self.om = make_oracle(self.map)

    def centre(self, local, region=(0, 0, 0)):
        """Centre of a voxel, checked against the oracle's key of that point."""
        point = self.low + RES * (np.array(region) * np.array(self.dims) + np.array(local) + 0.5)
        assert self.om.voxel_key(point) == (tuple(region), tuple(local)), (region, local, point)
        return point

    def index(self, local):
        return local[0] + self.dims[0] * (local[1] + self.dims[1] * local[2])

    def integrate(self, rays, flags=0):
        assert self.gm.integrateRays(rays, None, None, flags) == rays.shape[0]
        self.om.integrate_occupancy(rays, flags=flags)

    def seed(self, locals_, values):
        """Voxel<T>::write on both sides: writeVoxels on the device, the live block of the oracle's region."""
        values = np.asarray(values, dtype=F)
        regions = np.zeros((len(locals_), 3), dtype=np.int16)
        assert self.gm.writeVoxels((regions, np.array(locals_, dtype=np.uint8)), "occupancy", values) == len(locals_)
        block = self.om.region_layer_view((0, 0, 0), "occupancy")
        block.view(np.uint32)[[self.index(v) for v in locals_]] = values.view(np.uint32)

    def device_bits(self, local):
        return int(read_device(self.map, self.gm)[(0, 0, 0)]["occupancy"].view(np.uint32)[self.index(local)])

    def finish(self):
        device = read_device(self.map, self.gm)
        oracle = self.om.chunks(list(self.map.layers))
        bad = []
        for region in sorted(set(device) | set(oracle)):
            for name in self.map.layers:
                if region in device and region in oracle:
                    got, want = device[region][name].view(np.uint32), oracle[region][name].view(np.uint32)
                    n = int(np.count_nonzero(got != want))
                elif name == "occupancy":   # a region one side does not know counts as never observed
                    known = (device if region in device else oracle)[region][name]
                    n = int(np.count_nonzero(known.view(np.uint32) != F(np.inf).view(np.uint32)))
                else:
                    n = 0
                if n:
                    bad.append((region, name, n))
        self.gm.close()
        assert not bad, "regions that differ from the oracle (region, layer, elements): %r" % bad[:8]


def pairs(starts, ends):
    ends = np.asarray(ends, dtype=np.float64).reshape(-1, 3)
    out = np.empty((2 * ends.shape[0], 3), dtype=np.float64)
    out[0::2] = starts
    out[1::2] = ends
    return out


def fan(seed, n, reach, origin=(0.03, 0.06, 0.01)):
    """n rays from (nearly) one point near the map's origin to points within `reach` of it on every axis."""
    rng = np.random.default_rng(seed)
    origin = np.array(origin)
    return pairs(origin + rng.uniform(-0.02, 0.02, size=(n, 3)), origin + rng.uniform(-reach, reach, size=(n, 3)))


def x_rays(maps, rows, x0, x1, seed=0):
    """One ray per entry of rows [(y, z)] along +x from voxel x0 to voxel x1 of region (0, 0, 0): misses in x0 .. x1 - 1,
    the sample in x1.  Parallel to the axis, a little off the voxel centres."""
    rng = np.random.default_rng(seed)
    x0 = np.broadcast_to(x0, len(rows))
    x1 = np.broadcast_to(x1, len(rows))
    starts = np.array([maps.centre((int(a), y, z)) for a, (y, z) in zip(x0, rows)])
    ends = np.array([maps.centre((int(b), y, z)) for b, (y, z) in zip(x1, rows)])
    off = rng.uniform(-0.03, 0.03, size=(len(rows), 3))
    off[:, 0] = 0.0
    return pairs(starts + off, ends + off)


# ---- value states under the lean direct apply ---------------------------------------------------------------------------
COUNTS = {4: 1, 6: 2, 8: 3, 10: 40}     # row y -> misses per voxel (40: more than it takes from max to the clamp)
ROW_Z = 5
FIRST_X = 3


def value_states(map_):
    lo, hi, miss = F(map_.min_voxel_value), F(map_.max_voxel_value), F(map_.miss_value)
    nan = np.array([0x7fc01234], dtype=np.uint32).view(F)[0]
    return np.array([np.inf, -0.0, 0.0, lo, lo - miss,                                   # (sat_min == min_value)
                     np.nextafter(lo, F(np.inf)), np.nextafter(lo, F(-np.inf)),          # just inside / outside sat_min
                     hi, np.nextafter(hi, F(-np.inf)), np.nextafter(hi, F(np.inf)),      # at / inside / outside sat_max
                     lo - F(1.0), -np.inf, nan, 0.5], dtype=F)


@pytest.mark.parametrize("miss_value", [None, 0.0], ids=["default miss", "miss probability 0.5"])
def test_value_states(gpu, monkeypatch, miss_value):
    """One 32^3 region held by one chunk.  Every state sits in each of four rows; one batch of repeated rays then gives
    the rows 1, 2, 3 and 40 misses per voxel.  With a miss value of 0 nothing moves except what the update itself
    rewrites: -0.0 comes out as +0.0, values below the clamp and NaN as the clamp."""
    maps = Maps(monkeypatch, miss_value=miss_value, saturate=True)
    maps.integrate(x_rays(maps, [(28, 28)], 27, 29))           # the region exists on both sides
    states = value_states(maps.map)
    locals_ = [(FIRST_X + s, y, ROW_Z) for y in COUNTS for s in range(len(states))]
    maps.seed(locals_, np.tile(states, len(COUNTS)))
    rows = [(y, ROW_Z) for y, count in COUNTS.items() for _ in range(count)]
    assert FIRST_X + len(states) < 24
    maps.integrate(x_rays(maps, rows, 2, 24, seed=1))
    if miss_value == 0.0:
        for y in COUNTS:
            assert maps.device_bits((FIRST_X + 1, y, ROW_Z)) == 0, y                          # -0.0 -> +0.0
            assert maps.device_bits((FIRST_X + 13, y, ROW_Z)) == int(F(0.5).view(np.uint32))  # untouched
    maps.finish()


# ---- flags inside a tile word -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [("occupancy",), ("occupancy", "mean")], ids=["samples replayed by the walk",
                                                                                 "counts handed to k_apply_hits"])
@pytest.mark.parametrize("case", ["low", "high", "both", "no miss"])
def test_flags_inside_a_tile_word(gpu, monkeypatch, layers, case):
    """Voxels 10 and 11 of a row share a tile word; rays along the row leave misses in both.  End points in 10 only, in
    11 only, in both; and a word whose flagged voxel has no miss beside one with misses and no flag."""
    maps = Maps(monkeypatch, layers=layers)
    y0, z0 = 12, 7
    through = x_rays(maps, [(y0, z0)] * 3, 4, 20, seed=2).reshape(3, 2, 3)

    def y_rays(x, y_from, y_to, n, seed):
        off = np.random.default_rng(seed).uniform(-0.03, 0.03, size=(n, 3))
        off[:, 1] = 0.0
        return (pairs(maps.centre((x, y_from, z0)) + off, maps.centre((x, y_to, z0)) + off)).reshape(n, 2, 3)

    ending = []
    if case in ("low", "both"):
        ending += list(y_rays(10, y0 - 6, y0, 2, 3))
    if case in ("high", "both"):
        ending += list(y_rays(11, y0 - 6, y0, 2, 4))
    if case == "no miss":
        ending += list(y_rays(10, y0 + 8, y0 + 3, 2, 5))                               # (10, y0 + 3): samples only
        ending += list(x_rays(maps, [(y0 + 3, z0)] * 2, 11, 20, seed=6).reshape(2, 2, 3))  # (11, y0 + 3): misses only
    order = [through[0]] + ending[:len(ending) // 2] + [through[1]] + ending[len(ending) // 2:] + [through[2]]
    maps.integrate(np.concatenate(order).reshape(-1, 3))
    maps.finish()


# ---- what the lean bodies do not serve ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [RayFlag.kRfExcludeUnobserved, RayFlag.kRfExcludeFree, RayFlag.kRfExcludeOccupied],
                         ids=["exclude unobserved", "exclude free", "exclude occupied"])
def test_exclusion_flags_take_the_general_form(gpu, monkeypatch, flag):
    maps = Maps(monkeypatch)
    maps.integrate(fan(11, 2000, 4.0))
    maps.integrate(fan(12, 2000, 4.0), flags=int(flag))
    maps.integrate(fan(13, 2000, 4.0), flags=int(flag))
    maps.finish()


@pytest.mark.parametrize("dims,reach", [((33, 31, 31), 4.0), ((5, 5, 5), 1.2)],
                         ids=["33x31x31: odd voxel count, short last mask word", "5x5x5: the half shape"])
def test_other_region_sizes_take_the_general_form(gpu, monkeypatch, dims, reach):
    maps = Maps(monkeypatch, dims=dims)
    maps.integrate(fan(21, 2000, reach))
    maps.integrate(fan(22, 2000, reach))
    maps.finish()


# ---- flush path and direct path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,half_voxels", [((32, 32, 32), None), ((32, 32, 16), 16384)],
                         ids=["32^3", "32x32x16 on the half shape, whose tile it fills"])
@pytest.mark.parametrize("chunk", [256, None], ids=["chunks of 256: tile flush", "defaults: direct apply"])
def test_flush_path_and_direct_path(gpu, monkeypatch, chunk, dims, half_voxels):
    """The same 3000 rays, twice: with 256-segment chunks the regions near the origin are cut into several chunks whose
    tiles are flushed and applied by k_apply_lists; with the defaults every region is one chunk, applied from LDS.
    (The half shape serves regions of up to 4096 voxels unless OHMHIP_WALK_HALF_VOXELS says otherwise: only then does a
    region fill its tile.)"""
    maps = Maps(monkeypatch, dims=dims, chunk=chunk, half_voxels=half_voxels)
    rays = fan(31, 3000, 6.0)
    maps.integrate(rays)
    maps.integrate(rays)
    maps.finish()


# ---- the segment ordering -------------------------------------------------------------------------------------------------
def one_region_batch(maps, n, x0=0, x1=31):
    """n parallel rays along x through region (0, 0, 0), spread over its rows -- n segments of ONE length class in that
    region -- and, when n could otherwise not stay one chunk, enough short rays in region (3, 0, 0) for a call of more
    than 16384 rays: smaller calls halve their chunk size down to 512 segments."""
    dy, dz = maps.dims[1], maps.dims[2]
    rows = [(k % dy, (k // dy) % dz) for k in range(n)]
    rays = x_rays(maps, rows, x0, x1, seed=n)
    if n > 512:
        rng = np.random.default_rng(n + 1)
        starts = maps.centre((0, 0, 0), region=(3, 0, 0)) + rng.uniform(0.4, 2.6, size=(16400 - n, 3))
        rays = np.vstack([rays, pairs(starts, starts + rng.uniform(-0.2, 0.2, size=starts.shape))])
    return rays


@pytest.mark.parametrize("n", [1, 63, 64, 65, 8191, 8192, 8193])
def test_chunk_sizes_of_one_length_class(gpu, monkeypatch, n):
    """Chunks of n segments that all fall into one length class, the worst pile-up on the class counters: up to 8192
    parallel rays across one region (8193: the region takes two chunks and the flush path)."""
    maps = Maps(monkeypatch, chunk=8192)
    maps.integrate(one_region_batch(maps, n))
    maps.finish()


def test_segments_longer_than_the_top_class(gpu, monkeypatch):
    """A 255 x 4 x 4 region: segments of 130 .. 250 voxels share the top length class (127) with each other."""
    maps = Maps(monkeypatch, dims=(255, 4, 4))
    rows = [(k % 4, (k // 4) % 4) for k in range(300)]
    lengths = 130 + (np.arange(300) * 7) % 121
    maps.integrate(x_rays(maps, rows, 0, lengths, seed=41))
    maps.finish()


@pytest.mark.parametrize("dims", [(32, 32, 32), (255, 4, 4)], ids=["32^3: lengths 1 .. 31", "255x4x4: lengths 1 .. 254"])
def test_one_segment_in_each_of_many_classes(gpu, monkeypatch, dims):
    maps = Maps(monkeypatch, dims=dims)
    lengths = np.arange(1, dims[0])
    rows = [(k % dims[1], (k // dims[1]) % dims[2]) for k in range(len(lengths))]
    maps.integrate(x_rays(maps, rows, 0, lengths, seed=42))
    maps.finish()
