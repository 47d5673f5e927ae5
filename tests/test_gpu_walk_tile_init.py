"""-m gpu: the start of a chunk in k_region_walk -- the count tile's initialisation through its lean body (initFullTile:
a region that fills the walk's tile, no flag_all) -- and the first-sample table k_sort_region_hits now writes only for
regions whose samples the walk cannot stage in LDS; against the CPU oracle.

Every case runs the same calls through a device map and the oracle (the Maps harness of test_gpu_walk_fixed_cost) and
compares every region either side knows, bit for bit.

A tile entry is a 15-bit miss count with the voxel's "also receives samples" flag on top.  A voxel that loses its flag has
its misses applied without regard to its samples; a voxel with a flag it should not have keeps its misses for a replay
that never comes.  Sampled voxels are therefore seeded a quarter of a hit below the max clamp and receive a miss from an
earlier ray, the sample, and a miss from a later ray: miss, hit (clamped), miss ends at max + miss, any other order or
grouping at another value; their neighbours receive the two misses only."""
import numpy as np
import pytest

from ohm_amd import RayFlag, device_info
from test_gpu_mean_states import read_device
from test_gpu_walk_fixed_cost import RES, F, Maps, fan, pairs

pytestmark = pytest.mark.gpu

SHAPES = [((32, 32, 32), None), ((32, 32, 16), 16384)]
SHAPE_IDS = ["32^3 on the full shape", "32x32x16 on the half shape, whose tile it fills"]


def near_clamp(map_):
    """A quarter of a hit below the max clamp: hit -> the clamp; miss, hit -> the clamp; hit, miss -> below it."""
    value = F(map_.max_voxel_value) - F(0.25) * F(map_.hit_value)
    assert value + F(map_.miss_value) + F(map_.hit_value) > F(map_.max_voxel_value)
    return value


def through_rays(maps, rows, seed):
    """One ray per row (y, z) along +x from the neighbouring region (-1, 0, 0) across all 32 voxels of the row of region
    (0, 0, 0) into region (1, 0, 0): a miss in every voxel of the row."""
    rng = np.random.default_rng(seed)
    starts = np.array([maps.centre((30, y, z), region=(-1, 0, 0)) for y, z in rows])
    ends = np.array([maps.centre((1, y, z), region=(1, 0, 0)) for y, z in rows])
    off = rng.uniform(-0.03, 0.03, size=(len(rows), 3))
    off[:, 0] = 0.0
    return pairs(starts + off, ends + off)


def sample_rays(maps, locals_, seed):
    """One ray per voxel that starts and ends inside it: the sample, and no miss anywhere."""
    rng = np.random.default_rng(seed)
    centres = np.array([maps.centre(v) for v in locals_])
    return pairs(centres + rng.uniform(-0.03, 0.03, size=centres.shape), centres + rng.uniform(-0.03, 0.03, size=centres.shape))


def filler_rays(maps, n, seed):
    """n rays along x in the rows 8 <= y, z < 16 of region (0, 0, 0), which no case below looks at: with 256-segment
    chunks they make the region take more than one chunk."""
    rows = [(8 + k % 8, 8 + (k // 8) % 8) for k in range(n)]
    rng = np.random.default_rng(seed)
    starts = np.array([maps.centre((4, y, z)) for y, z in rows])
    ends = np.array([maps.centre((20, y, z)) for y, z in rows])
    off = rng.uniform(-0.03, 0.03, size=(n, 3))
    off[:, 0] = 0.0
    return pairs(starts + off, ends + off)


# ---- every flag position ------------------------------------------------------------------------------------------------
ROWS = [(0, 0), (1, 0), (2, 0), (3, 0), (6, 0), (5, 1), (6, 2), (14, 6), (22, 3), (16, 17), (31, 31)]


def row_swizzle(dims, y, z):
    """The XOR constant tileWord() applies to the 16 tile words of row (y, z): one mask word per row of 32 voxels."""
    w = y + dims[1] * z
    return ((w >> 1) ^ (w >> 6)) & 31


@pytest.mark.parametrize("dims,half_voxels", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("chunk", [None, 256], ids=["defaults: direct apply", "chunks of 256: tile flush"])
def test_every_flag_position(gpu, monkeypatch, chunk, dims, half_voxels):
    """Rows whose swizzles cover all four values of the low two bits (the order of the words inside a 4-word group) and
    four of the high bits (the order of the groups).  Batch x gives voxel x of every row a miss, a sample and a miss, and
    the other 31 voxels of the row -- the other half of its tile word, its group, the neighbouring groups -- the two
    misses only.  Every batch is compared with the oracle, and all of it once more at the end."""
    assert dims[0] == 32
    rows = [(y, z % dims[2]) for y, z in ROWS]
    swizzles = [row_swizzle(dims, y, z) for y, z in rows]
    assert {s & 3 for s in swizzles} == {0, 1, 2, 3} and len({s >> 2 for s in swizzles}) >= 4, swizzles
    maps = Maps(monkeypatch, dims=dims, chunk=chunk, half_voxels=half_voxels)
    maps.integrate(through_rays(maps, rows, seed=1))               # the regions exist on both sides
    value = near_clamp(maps.map)
    row_voxels = [(x, y, z) for y, z in rows for x in range(32)]
    for x in range(32):
        maps.seed(row_voxels, np.full(len(row_voxels), value, dtype=F))
        maps.integrate(np.vstack([through_rays(maps, rows, seed=100 + x),
                                  filler_rays(maps, 150, seed=200 + x),
                                  sample_rays(maps, [(x, y, z) for y, z in rows], seed=300 + x),
                                  filler_rays(maps, 150, seed=400 + x),
                                  through_rays(maps, rows, seed=500 + x)]))
        # (the rows are seeded again for the next batch: this batch's values are looked at now)
        got = read_device(maps.map, maps.gm)[(0, 0, 0)]["occupancy"].view(np.uint32)
        want = maps.om.region_layer_view((0, 0, 0), "occupancy").view(np.uint32)
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, "batch %d: voxels that differ from the oracle: %r" % (x, wrong[:8].tolist())
    maps.finish()


# ---- stale tile state ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,half_voxels", SHAPES, ids=SHAPE_IDS)
def test_tiles_initialised_many_times(gpu, monkeypatch, dims, half_voxels):
    """10^5 rays in 256-segment chunks: several chunks per walk workgroup, so every workgroup initialises its tile over
    what the previous chunk left there.  70 % of the rays end around the sensor; the others end 8 to 9.5 m out on x and
    cross regions that receive no sample at all.  The same batch twice."""
    maps = Maps(monkeypatch, dims=dims, chunk=256, half_voxels=half_voxels)
    reach = 1.4 * RES * np.array(dims, dtype=np.float64)           # three regions on every axis
    rng = np.random.default_rng(51)
    origin = np.array((0.03, 0.06, 0.01))
    near = origin + rng.uniform(-1.0, 1.0, size=(70000, 3)) * reach
    far = origin + rng.uniform(-1.0, 1.0, size=(30000, 3)) * reach
    far[:, 0] = rng.uniform(8.2, 9.4, size=far.shape[0])
    ends = np.vstack([near, far])[rng.permutation(100000)]
    rays = pairs(origin + rng.uniform(-0.02, 0.02, size=ends.shape), ends)
    maps.integrate(rays)
    segments = maps.gm.stats()["ray_region_segments"]
    assert segments // 256 > 4 * device_info(0)["compute_units"], segments     # (a chunk holds at most 256 segments)
    maps.integrate(rays)
    maps.finish()


# ---- what the lean body must not serve ------------------------------------------------------------------------------------
def test_stop_flag_batch_takes_the_general_form(gpu, monkeypatch):
    """kRfStopOnFirstOccupied: every visit is an event (flag_all), every tile entry starts flagged."""
    maps = Maps(monkeypatch)
    maps.integrate(fan(61, 3000, 1.5))
    maps.integrate(fan(62, 3000, 1.5), flags=int(RayFlag.kRfStopOnFirstOccupied))
    maps.finish()


def test_small_region_takes_the_general_form(gpu, monkeypatch):
    """5 x 5 x 5: four mask words, the last one short; 63 tile words."""
    maps = Maps(monkeypatch, dims=(5, 5, 5))
    maps.integrate(fan(63, 3000, 0.7))
    maps.integrate(fan(64, 3000, 0.7))
    maps.finish()


# ---- the first-sample table at the staging boundary ---------------------------------------------------------------------
def dense_batch(maps, n, first_voxel, seed):
    """n samples into region (0, 0, 0), in voxel order from `first_voxel` on, every tenth voxel twice; every fifth row
    they touch is crossed by a ray ahead of all samples, one between the two halves of them (the two samples of a voxel
    fall into different halves) and one behind them.  Returns the rays and the sampled voxels."""
    k = np.arange(n)
    voxel = first_voxel + k - k // 10
    dx, dy = maps.dims[0], maps.dims[1]
    locals_ = [(int(v % dx), int((v // dx) % dy), int(v // (dx * dy))) for v in voxel]
    samples = sample_rays(maps, locals_, seed).reshape(n, 2, 3)
    rows = sorted({(v[1], v[2]) for v in locals_})[::5]
    rays = np.vstack([through_rays(maps, rows, seed + 1), samples[0::2].reshape(-1, 3),
                      through_rays(maps, rows, seed + 2), samples[1::2].reshape(-1, 3),
                      through_rays(maps, rows, seed + 3)])
    return rays, sorted(set(locals_))


def run_near_clamp(maps, rays, voxels):
    maps.seed(voxels, np.full(len(voxels), near_clamp(maps.map), dtype=F))
    maps.integrate(rays)


@pytest.mark.parametrize("dims,half_voxels,staged", [(d, h, s) for (d, h), s in zip(SHAPES, (6144, 3072))], ids=SHAPE_IDS)
@pytest.mark.parametrize("delta", [-1, 0, 1], ids=["one below the staging capacity", "at it", "one above it"])
def test_first_sample_table_at_the_staging_boundary(gpu, monkeypatch, delta, dims, half_voxels, staged):
    """A region with exactly as many samples as the walk stages in LDS, one fewer and one more: up to the capacity the
    walk orders the region's misses against the staged keys and nobody writes or reads the table, above it the misses
    travel as events that start their search at the table's entry."""
    maps = Maps(monkeypatch, dims=dims, half_voxels=half_voxels)
    maps.integrate(through_rays(maps, [(0, 0)], seed=1))
    rays, voxels = dense_batch(maps, staged + delta, 0, seed=70)
    run_near_clamp(maps, rays, voxels)
    maps.finish()


@pytest.mark.parametrize("dims,half_voxels,staged", [(d, h, s) for (d, h), s in zip(SHAPES, (6144, 3072))], ids=SHAPE_IDS)
def test_first_sample_table_is_never_read_stale(gpu, monkeypatch, dims, half_voxels, staged):
    """A dense batch writes the table; a sparse batch over the same voxels must not read it (its samples lie elsewhere
    in the list); a dense batch over voxels 3000 further on -- half of them the first batch's -- rewrites what it reads."""
    maps = Maps(monkeypatch, dims=dims, half_voxels=half_voxels)
    maps.integrate(through_rays(maps, [(0, 0)], seed=1))
    for n, first_voxel, seed in ((staged + 1, 0, 80), (400, 1000, 84), (staged + 1, 3000, 88)):
        rays, voxels = dense_batch(maps, n, first_voxel, seed)
        run_near_clamp(maps, rays, voxels)
    maps.finish()
