"""-m gpu: the device flood-fill heightmap (ohmhip_map_heightmap_fill / _device / _extents, ohm_amd.Heightmap with
HeightmapMode.kSimpleFill) against the CPU restatement of ohm::Heightmap::buildHeightmap in kSimpleFill (tests/
heightmap_fill_ref.py) at EXACT equality: occupancy, voxels, mean, source_visit, the full visit log and every stats field
with np.array_equal on the raw bits.  Every test asserts on the restatement's run the precondition it exists for, so a
scene that stops exercising its quirk fails."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import GpuMap, Heightmap, HeightmapMode, HeightmapVoxelType, OccupancyMap, OhmHipError, UpAxis
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
import heightmap_fill_ref as F  # noqa: E402
from heightmap_fill_cases import (FLAT_HOLES, HIT, INF32, MISS, flat_cases, flat_floor, mean_scene,  # noqa: E402
                                  scaled_multi_level)

pytestmark = pytest.mark.gpu


def device_map(scene, one_by_one=False, **kw):
    """(host OccupancyMap, GpuMap) holding the scene's chunks."""
    layers = ("occupancy", "mean") if scene.with_mean else ("occupancy",)
    map_ = OccupancyMap(scene.resolution, scene.dim, layers=layers)
    for key, c in scene.chunks.items():
        map_.chunks[key] = {name: np.array(block, copy=True) for name, block in c.items()}
    gm = GpuMap(map_, **kw)
    if not one_by_one:
        gm.uploadRegions(sorted(scene.chunks))
    return map_, gm


def fill_heightmap(gm, p, keep_log=True, mode=HeightmapMode.kSimpleFill):
    hm = Heightmap(p.grid_resolution, p.min_clearance, UpAxis(p.up_axis), p.region_size)
    hm.floor, hm.ceiling = p.floor, p.ceiling
    hm.generate_virtual_surface = p.virtual_surface
    hm.promote_virtual_below = p.promote_virtual_below
    hm.ignore_voxel_mean = p.ignore_voxel_mean
    hm.heightmap_origin = p.origin
    hm.mode = mode
    hm.keep_visit_log = keep_log
    hm.set_occupancy_map(gm)
    built = hm.build_heightmap(p.reference_pos, (p.cull_min, p.cull_max))
    return hm, built


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same(hm, built, want, what=""):
    e, st = hm.extents, hm.fill_stats
    assert (e.na, e.nb, e.ma, e.mb) == (want.na, want.nb, want.ma, want.mb), what
    assert np.array_equal(hm.visit_log, want.log), (what, "log", hm.visit_log.shape, want.log.shape)
    assert np.array_equal(hm.occupancy.view(np.uint32), want.occupancy.view(np.uint32)), (what, "occupancy")
    assert np.array_equal(bits(hm.voxels), bits(want.voxels)), (what, "voxels")
    assert (hm.mean is None) == (want.mean is None), what
    if want.mean is not None:
        assert np.array_equal(hm.mean, want.mean), (what, "mean")
    assert np.array_equal(hm.source_visit, want.source_visit), (what, "source_visit")
    got = (st.visits, st.populated, st.cells, st.revisits, st.generations, st.largest_generation)
    assert got == (want.visits, want.populated, want.cells, want.revisits, want.generations,
                   want.largest_generation), (what, got)
    assert (hm.populated_count, hm.cell_count) == (want.populated, want.cells), what
    assert built == (want.populated != 0), what


def check(scene, p, what="", gm=None):
    want = F.build_fill(scene.source(), p)
    assert want is not None, what
    if gm is None:
        _, gm = device_map(scene)
    hm, built = fill_heightmap(gm, p)
    assert_same(hm, built, want, what)
    return hm, want


# -- flat floor across regions -------------------------------------------------------------------------------------------

_FLAT = {}


@pytest.mark.parametrize("case", list(flat_cases()), ids=lambda c: c[0])
def test_flat_floor_across_regions(gpu, case):
    name, scene, p = case
    if "gm" not in _FLAT:
        _FLAT["gm"] = device_map(scene)[1]
    hm, want = check(scene, p, name, _FLAT["gm"])
    # 3 x 3 x 1 regions of 8^3 voxels and a z range that reaches into the regions missing above and below
    assert (want.na, want.nb) == (25, 25) and len(scene.chunks) == 9
    assert want.min_ext[2] < 0 and want.max_ext[2] >= 8
    assert want.visits >= 625  # the fill reaches every column, across every region border
    if "outside" in name:
        assert want.log[0].tolist() == [24, 0, want.max_ext[2] - want.min_ext[2]]  # clamped on all three axes
    if "hole" in name:
        assert (3, 3) in FLAT_HOLES and want.log[0].tolist()[:2] == [11, 11]
        assert p.virtual_surface or want.occupancy[11, 11] == np.inf  # no ground voxel under the seed
    if p.virtual_surface and not (p.floor and "outside" in name):
        assert (want.occupancy == -1.0).any() and want.revisits > 0


# -- the multi-level scene -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("up_axis", [-3, -2, -1, 0, 1, 2])
def test_multi_level_scene(gpu, up_axis):
    scene, p = scaled_multi_level(up_axis)
    hm, want = check(scene, p, "up %d" % up_axis)
    assert want.revisits > 0 and want.raising_pops > 0 and want.max_cell_multiplicity >= 2
    assert (want.occupancy == 1.0).any() and (want.occupancy == -1.0).any()
    assert want.populated > want.cells
    # "lower" is lower on the raw key axis, also for a negative up axis: an accepted revisit has the smaller h
    first_h = {}
    lowered = 0
    for ia, ib, h in want.log.tolist():
        lowered += (ia, ib) in first_h and h < first_h[(ia, ib)]
        first_h.setdefault((ia, ib), h)
    assert lowered > 0


def test_voxel_info(gpu):
    scene, p = scaled_multi_level()
    src = scene.source()
    want = F.build_fill(src, p)
    hm, built = fill_heightmap(device_map(scene)[1], p, keep_log=False)
    assert built and hm.visit_log is None
    _, dims, first, _, _ = R.heightmap_geometry(src, p, (want.min_ext, want.max_ext))
    seen = set()
    for cb in range(0, want.mb, 3):
        for ca in range(0, want.ma, 3):
            g = [first[0] + ca, first[1] + cb, 0]
            key = ([g[c] // dims[c] for c in range(3)], [g[c] % dims[c] for c in range(3)])
            voxel_type, pos, _ = hm.get_heightmap_voxel_info(key)
            ref_type, ref_pos, _ = R.voxel_info(want, src, p, (ca, cb))
            assert int(voxel_type) == ref_type and list(pos) == list(ref_pos)
            seen.add(int(voxel_type))
    assert {int(HeightmapVoxelType.kUnknown), int(HeightmapVoxelType.kSurface),
            int(HeightmapVoxelType.kVirtualSurface)} <= seen


# -- a generation wider than a workgroup -------------------------------------------------------------------------------------

def test_generation_wider_than_a_workgroup(gpu):
    scene = flat_floor(n=130, dim=(16, 16, 16), resolution=0.5, level=9, first=-65)
    p = R.Params(0.5, 0.0, reference_pos=(0.1, 0.1, 0.7), floor=1.5, ceiling=1.5)
    hm, want = check(scene, p, "130 x 130")
    assert want.largest_generation > 256 and want.cells == 130 * 130
    assert len(want.log) > (1 << 14)  # the queue outgrows its first block mid-walk, with entries to keep


# -- the two builds' flags of the selection ladder ---------------------------------------------------------------------------

def test_ladder_flags_of_the_two_builds(gpu):
    """Both builds run one ladder on the device: the planar one with kIgnoreVirtualAbove, the fill with kBiasAbove on
    every visit but the first.  Two planted columns of one 16^3 region of 1 m voxels tell the flag sets apart, one per
    row that differs, so flags exchanged between the two call sites fail here.  Column A is free with occupied voxels
    at z = 4 and z = 10, column B unobserved at z = 0 .. 4 and z = 9 and free elsewhere; an ordinary floor at z = 8
    around them, the plane and the seed on it, so the fill reaches both from z = 8 and not as its first visit."""
    col_a, col_b, seed_xy, level = (3, 3), (12, 12), (8, 8), 8
    scene = flat_floor(n=16, dim=(16, 16, 16), resolution=1.0, level=level, first=0)
    for z in range(16):
        scene.put(col_a + (z,), HIT if z in (4, 10) else MISS)
        scene.put(col_b + (z,), INF32 if (z <= 4 or z == 9) else MISS)
    assert len(scene.chunks) == 1
    p = R.Params(1.0, 0.0, reference_pos=scene.centre(seed_xy + (level,)), virtual_surface=True)
    src = scene.source()
    min_key, max_key = R.extents(src, p)
    assert max(1, R.point_to_region_coord(p.min_clearance, src.resolution) - 1) == 1  # clearance_permissive

    def candidate_z(column, flags):
        return R.supporting_voxel(src, list(column) + [level], p.up_axis, min_key, max_key, 0, 0, 1, flags)[2]

    planar_flags, fill_flags = R.F_VIRTUAL | R.F_IGNORE_VIRTUAL_ABOVE, R.F_VIRTUAL | R.F_BIAS_ABOVE
    # the precondition: the restatements disagree on both columns, A on the bias row, B on the ignore-virtual-above row
    assert (candidate_z(col_a, planar_flags), candidate_z(col_a, fill_flags)) == (4, 10)
    assert (candidate_z(col_b, planar_flags), candidate_z(col_b, fill_flags)) == (4, 9)
    assert candidate_z(seed_xy, planar_flags) == candidate_z(seed_xy, fill_flags) == level

    _, gm = device_map(scene)
    hm, want = check(scene, p, "ladder, fill", gm)
    assert want.log[0].tolist() == list(seed_xy) + [level - min_key[2]]
    planar_want = R.build_heightmap(src, p)
    planar, built = fill_heightmap(gm, p, keep_log=False, mode=HeightmapMode.kPlanar)
    assert built and (planar_want.na, planar_want.nb, planar_want.ma, planar_want.mb) == (want.na, want.nb, want.ma, want.mb)
    assert np.array_equal(planar.occupancy.view(np.uint32), planar_want.occupancy.view(np.uint32))
    assert np.array_equal(bits(planar.voxels), bits(planar_want.voxels))
    assert np.array_equal(planar.source_column, planar_want.source_column)
    assert planar.populated_count == planar_want.populated
    # ... and what the builds hold in the two cells is what the candidates lead to (the grid is the map's: cell = column)
    def rise(result, column):
        return float(result.voxels["height"][column[1], column[0]]) - float(result.voxels["height"][seed_xy[1], seed_xy[0]])

    assert (rise(planar_want, col_a), rise(want, col_a)) == (4.0 - level, 10.0 - level)
    assert (rise(planar_want, col_b), rise(want, col_b)) == (5.0 - level, 10.0 - level)  # virtual: the free voxel above
    assert planar_want.occupancy[col_b[1], col_b[0]] == want.occupancy[col_b[1], col_b[0]] == -1.0


# -- mean layer and a coarser grid --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid,origin,region_size,crossing", [
    (1.0, (0.5, 0.5, 0.0), 0, False),      # twice the map's resolution, half a cell: the cell edges are voxel edges
    (0.5, (0.25, 0.25, 0.0), 16, True),    # the map's resolution, half a cell: every source voxel is cut in four
    (1.0, (0.25, 0.25, 0.0), 0, True)])    # both
def test_mean_layer_and_coarser_grid(gpu, grid, origin, region_size, crossing):
    scene = mean_scene()
    p = R.Params(grid, 0.0, reference_pos=(0.1, 0.1, 0.0), origin=origin, region_size=region_size)
    hm, want = check(scene, p, "mean")
    assert want.mean is not None and (want.voxels["contributing_samples"] > 1).any()
    # means pushed across a cell edge: some column's cell is not the cell of its voxel centre
    no_mean = F.build_fill(scene.source(), R.Params(grid, 0.0, reference_pos=p.reference_pos, origin=origin,
                                                    region_size=region_size, ignore_voxel_mean=True))
    assert np.array_equal(no_mean.source_visit, want.source_visit) != crossing
    if grid == 1.0:
        assert want.populated >= 2 * want.cells  # several visits write one cell: source_visit names the winner
        winners = want.source_visit[want.source_visit != F.NO_VISIT]
        assert len(set(winners.tolist())) == want.cells


# -- store and tiles ---------------------------------------------------------------------------------------------------------

def _observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


def test_regions_in_the_host_store(gpu):
    _, scene, _ = next(iter(flat_cases()))
    p = R.Params(0.5, 0.0, reference_pos=(1.3, 0.8, 1.2), cull_min=(0.0, 0.0, -5.9), cull_max=(0.0, 0.0, 5.9),
                 virtual_surface=True)
    map_, gm = device_map(scene, one_by_one=True, region_capacity=8)
    gm.setMemoryLimit(5 * gm.cacheStats()["bytes_per_region"])  # the scene holds 9 regions
    gm.setSpillToHost(True)
    for key in sorted(scene.chunks):
        gm.uploadRegions([key])
    assert gm.cacheStats()["regions_spilled"] > 0
    before = _observe(gm)
    hm, want = check(scene, p, "spill", gm)
    assert _observe(gm) == before
    assert (want.occupancy == 1.0).any() and (want.occupancy == -1.0).any()


def test_tiled_regions(gpu):
    """Regions of 40^3 voxels are cut into tiles by the library; the keys stay the caller's."""
    scene = flat_floor(n=30, dim=(40, 40, 40), resolution=0.5, level=21, holes=((0, 0), (1, 0), (-1, -1)), first=-10)
    p = R.Params(0.5, 0.0, reference_pos=(0.2, 0.2, 0.9), virtual_surface=True, floor=4.0, ceiling=4.0)
    hm, want = check(scene, p, "tiled")
    assert (want.na, want.nb) == (81, 81) and want.cells == 900 and (want.occupancy == -1.0).sum() == 3


def _read_layer(gm, keys, voxels):
    """The occupancy blocks of `keys` as the device holds them (ohmhip_map_read_regions: no mark is cleared)."""
    keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
    out = np.empty((len(keys), voxels), dtype=np.float32)
    ptrs = (C.c_void_p * len(keys))(*[out[i].ctypes.data for i in range(len(keys))])
    L.check(L.lib.ohmhip_map_read_regions(gm._handle, L.LID_OCCUPANCY, keys.ctypes.data, len(keys), ptrs), "read")
    return out


def test_read_only(gpu):
    """Dirty set, region list, cache stats and the occupancy layer are the same before and after a build."""
    scene, p = scaled_multi_level()
    map_, gm = device_map(scene)
    # two samples beyond the floor's edge: cells the uploaded scene does not have
    rays = np.array([[2.2, 2.2, 0.35], [2.2, 2.2, 0.05], [-2.2, 2.2, 0.35], [-2.2, 2.2, 0.05]], dtype=np.float64)
    assert gm.integrateRays(rays) == 4  # collected rays and, once launched, dirty regions
    keys = sorted(map(tuple, gm.regionKeys()))
    voxels = scene.dim[0] * scene.dim[1] * scene.dim[2]
    layer = _read_layer(gm, keys, voxels)
    before = _observe(gm)
    assert before[1]  # something is dirty
    hm, built = fill_heightmap(gm, p)
    assert built and _observe(gm) == before
    assert np.array_equal(_read_layer(gm, keys, voxels).view(np.uint32), layer.view(np.uint32))
    # ... and the build saw the rays: it equals the restatement on the map as read back
    chunks = {k: {"occupancy": layer[i]} for i, k in enumerate(keys)}
    want = F.build_fill(R.Source(scene.resolution, scene.dim, chunks, map_.occupancy_threshold_value), p)
    assert_same(hm, built, want, "read only")
    assert want.cells == F.build_fill(scene.source(), p).cells + 2


# -- log capacity, the device variant ------------------------------------------------------------------------------------------

class DeviceBuffer:
    def __init__(self, nbytes):
        self.handle = L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(self.handle), max(nbytes, 16), 3), "buffer_create")
        self.ptr = L._vp()
        L.check(L.lib.ohmhip_buffer_ptr(self.handle, C.byref(self.ptr)), "buffer_ptr")

    def read(self, dtype, shape):
        out = np.zeros(shape, dtype=dtype)
        L.check(L.lib.ohmhip_buffer_read(self.handle, out.ctypes.data, out.nbytes, 0, None, None, None), "read")
        return out

    def close(self):
        L.lib.ohmhip_buffer_destroy(self.handle)


def test_log_capacity_and_device_variant(gpu):
    scene = mean_scene()
    p = R.Params(1.0, 0.0, reference_pos=(0.1, 0.1, 0.0), origin=(0.5, 0.5, 0.0))
    _, gm = device_map(scene)
    hm, built = fill_heightmap(gm, p)
    visits = int(hm.fill_stats.visits)
    assert built and visits > 100 and hm.visit_log.shape == (visits, 3)
    cp = hm.params(p.reference_pos, (p.cull_min, p.cull_max))
    shape = hm.occupancy.shape
    n = hm.occupancy.size
    # a log smaller than the walk: not an error, the first entries, nothing beyond them written
    small = np.full((40, 3), 0xABABABAB, dtype=np.uint32)
    occ, vox = np.empty(shape, np.float32), np.empty(shape, hm.voxels.dtype)
    st = L.HeightmapFillStats()
    L.check(L.lib.ohmhip_map_heightmap_fill(gm._handle, C.byref(cp), occ.ctypes.data, vox.ctypes.data, None, None,
                                            small.ctypes.data, 30, C.byref(st)), "fill")
    assert st.visits == visits and np.array_equal(small[:30], hm.visit_log[:30]) and (small[30:] == 0xABABABAB).all()
    assert np.array_equal(occ.view(np.uint32), hm.occupancy.view(np.uint32)) and np.array_equal(bits(vox), bits(hm.voxels))
    bufs = [DeviceBuffer(4 * n), DeviceBuffer(24 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n),
            DeviceBuffer(12 * visits)]
    try:
        st = L.HeightmapFillStats()
        L.check(L.lib.ohmhip_map_heightmap_fill_device(gm._handle, C.byref(cp), *[b.ptr for b in bufs], visits,
                                                       C.byref(st)), "device")
        gm.wait()
        assert np.array_equal(bufs[0].read(np.uint32, shape), hm.occupancy.view(np.uint32))
        assert np.array_equal(bits(bufs[1].read(hm.voxels.dtype, shape)), bits(hm.voxels))
        assert np.array_equal(bufs[2].read(np.uint32, shape + (2,)), hm.mean)
        assert np.array_equal(bufs[3].read(np.uint32, shape), hm.source_visit)
        assert np.array_equal(bufs[4].read(np.uint32, (visits, 3)), hm.visit_log)
        for name, _ in L.HeightmapFillStats._fields_:
            assert getattr(st, name) == getattr(hm.fill_stats, name), name
    finally:
        for b in bufs:
            b.close()


# -- refusals ------------------------------------------------------------------------------------------------------------------

def test_layered_fill_still_raises_and_empty_map(gpu):
    scene, p = scaled_multi_level()
    _, gm = device_map(scene)
    hm = Heightmap(0.1, 0.0)
    hm.set_occupancy_map(gm)
    for mode in (HeightmapMode.kLayeredFill, HeightmapMode.kLayeredFillUnordered):
        hm.mode = mode
        with pytest.raises(OhmHipError) as err:
            hm.build_heightmap((0, 0, 0))
        assert err.value.status == L.ERR_UNSUPPORTED
    hm.mode = HeightmapMode.kSimpleFill
    hm.set_occupancy_map(GpuMap(OccupancyMap(0.1)))
    assert hm.build_heightmap((0, 0, 0)) is False and hm.occupancy is None  # an empty map: nothing to build
