"""-m gpu: the device layered heightmaps (ohmhip_map_heightmap_layered / _device / _extents, ohm_amd.LayeredHeightmap)
against the CPU restatement of ohm::Heightmap::buildHeightmap in kLayeredFill / kLayeredFillUnordered (tests/
heightmap_layered_ref.py) at EXACT equality: occupancy, voxels, mean, source_visit, layer_count, the full visit log and
every stats field with np.array_equal on the raw bits.  Every case asserts on the restatement's run that the quirk it
exists for occurs, so a scene that stops exercising it fails."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (GpuMap, Heightmap, HeightmapMode, HeightmapVoxelType, LayeredHeightmap, OccupancyMap, OhmHipError,
                     UpAxis)
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
import heightmap_layered_ref as LR  # noqa: E402
import heightmap_layered_cases as LC  # noqa: E402
from heightmap_fill_cases import flat_cases, flat_floor, scaled_multi_level  # noqa: E402

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


def layered_heightmap(gm, p, mode, threshold, keep_log=True):
    hm = LayeredHeightmap(p.grid_resolution, p.min_clearance, UpAxis(p.up_axis), p.region_size)
    hm.floor, hm.ceiling = p.floor, p.ceiling
    hm.generate_virtual_surface = p.virtual_surface
    hm.promote_virtual_below = p.promote_virtual_below
    hm.ignore_voxel_mean = p.ignore_voxel_mean
    hm.heightmap_origin = p.origin
    hm.mode = HeightmapMode(mode)
    hm.virtual_surface_filter_threshold = threshold
    hm.keep_visit_log = keep_log
    hm.set_occupancy_map(gm)
    built = hm.build_heightmap(p.reference_pos, (p.cull_min, p.cull_max))
    return hm, built


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same(hm, built, want, what=""):
    e, st = hm.extents, hm.layered_stats
    assert (e.na, e.nb, e.ma, e.mb) == (want.na, want.nb, want.ma, want.mb), what
    got = tuple(int(getattr(st, name)) for name in LR.STATS)
    assert got == LR.stats_of(want), (what, got, LR.stats_of(want))
    assert np.array_equal(hm.visit_log, want.log), (what, "log", hm.visit_log.shape, want.log.shape)
    assert hm.occupancy.shape == want.occupancy.shape, (what, hm.occupancy.shape, want.occupancy.shape)
    assert np.array_equal(hm.layer_count, want.layer_count), (what, "layer_count")
    assert np.array_equal(hm.occupancy.view(np.uint32), want.occupancy.view(np.uint32)), (what, "occupancy")
    assert np.array_equal(bits(hm.voxels), bits(want.voxels)), (what, "voxels")
    assert (hm.mean is None) == (want.mean is None), what
    if want.mean is not None:
        assert np.array_equal(hm.mean, want.mean), (what, "mean")
    assert np.array_equal(hm.source_visit, want.source_visit), (what, "source_visit")
    assert (hm.populated_count, hm.cell_count) == (want.populated, want.cells), what
    assert built == (want.populated != 0), what


def check(scene, p, mode, threshold, quirks=(), what="", gm=None):
    want = LR.build_layered(scene.source(), p, mode, threshold)
    assert want is not None, what
    counts = LC.quirk_counts(want)
    for quirk in quirks:
        assert counts[quirk] > 0, (what, quirk)  # the case shows what it is about
    if gm is None:
        _, gm = device_map(scene)
    hm, built = layered_heightmap(gm, p, mode, threshold)
    assert_same(hm, built, want, what)
    return hm, want


# -- the multi-level scene: six up axes, both modes, the filter off and on ------------------------------------------------

_MULTI = {}


@pytest.mark.parametrize("threshold", [0, 8])
@pytest.mark.parametrize("mode", [LC.MODE_UNORDERED, LC.MODE_ORDERED])
@pytest.mark.parametrize("up_axis", [-3, -2, -1, 0, 1, 2])
def test_multi_level_scene(gpu, up_axis, mode, threshold):
    scene, p = scaled_multi_level(up_axis)
    if up_axis not in _MULTI:
        _MULTI.clear()  # one device map at a time
        _MULTI[up_axis] = device_map(scene)[1]
    quirks = ["repeats"]
    if mode == LC.MODE_ORDERED:
        quirks += ["multi_layer_columns", "permuted_columns"]
        if threshold:
            quirks += ["filtered", "virtual_kept"]  # the filter removes at least one voxel and keeps at least one
    hm, want = check(scene, p, mode, threshold, quirks, "up %d mode %d threshold %d" % (up_axis, mode, threshold),
                     _MULTI[up_axis])
    assert (want.occupancy == 1.0).any() and (want.occupancy == -1.0).any() and want.layers >= 2
    if mode == LC.MODE_UNORDERED or not threshold:
        assert want.filtered == 0


# -- the hand-made columns, laid across a region boundary ----------------------------------------------------------------

@pytest.mark.parametrize("case", list(LC.hand_made_cases()), ids=lambda c: c[0])
def test_hand_made_columns(gpu, case):
    name, scene, p, mode, threshold, quirks = case
    assert len(scene.chunks) >= 4  # the storeys span the region boundaries at x = 0 and y = 0 (or their turned images)
    hm, want = check(scene, p, mode, threshold, quirks, name)
    if name == "mean-coarse":
        assert want.layers > 2  # a column outgrows the walk's initial planes


def test_voxel_info_honours_the_slot(gpu):
    name, scene, p, mode, threshold, _ = next(c for c in LC.hand_made_cases() if c[0] == "base-by-distance")
    src = scene.source()
    want = LR.build_layered(src, p, mode, threshold)
    hm, built = layered_heightmap(device_map(scene)[1], p, mode, threshold, keep_log=False)
    assert built and hm.visit_log is None
    hmap, dims, first, _, _ = R.heightmap_geometry(src, p, (want.min_ext, want.max_ext))
    seen = set()
    for cb in range(want.mb):
        for ca in range(want.ma):
            for slot in range(want.slots + 1):
                g = [first[0] + ca, first[1] + cb, slot]
                key = ([g[c] // dims[c] for c in range(3)], [g[c] % dims[c] for c in range(3)])
                voxel_type, pos, voxel = hm.get_heightmap_voxel_info(key)
                if slot >= want.slots or want.occupancy[slot, cb, ca] == np.inf:
                    assert voxel_type == HeightmapVoxelType.kUnknown and voxel is None
                    continue
                centre = hmap.voxel_centre(key[0], key[1])
                assert voxel_type == HeightmapVoxelType.kSurface
                assert list(pos) == [centre[0], centre[1], centre[2] + float(want.voxels["height"][slot, cb, ca])]
                assert bits(np.array(voxel)).tolist() == bits(want.voxels[slot, cb, ca]).tolist()
                seen.add((slot, int(voxel["layer"])))
    assert {(0, LR.HVL_EXTENDED), (1, LR.HVL_BASE), (0, LR.HVL_BASE)} <= seen


# -- a generation wider than a workgroup -----------------------------------------------------------------------------------

def test_generation_wider_than_a_workgroup(gpu):
    scene = flat_floor(n=130, dim=(16, 16, 16), resolution=0.5, level=9, first=-65)
    p = R.Params(0.5, 0.0, reference_pos=(0.1, 0.1, 0.7), floor=1.5, ceiling=1.5)
    hm, want = check(scene, p, LC.MODE_ORDERED, 0, ("repeats",), "130 x 130")
    assert want.largest_generation > 256 and want.cells == 130 * 130 and want.layers == 1
    assert len(want.log) > (1 << 14)  # the queue and the node pool outgrow their first blocks mid-walk, with entries to keep


# -- mean layer and a coarser grid --------------------------------------------------------------------------------------------

def test_mean_layer_same_grid(gpu):
    name, scene, p, mode, threshold, quirks = list(LC.layered_cases())[-1]
    assert name == "mean-same"
    hm, want = check(scene, p, mode, threshold, quirks, name)
    assert want.mean is not None and (want.voxels["contributing_samples"] > 1).any()


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
    hm, want = check(scene, p, LC.MODE_ORDERED, 3, ("repeats", "virtual_kept"), "spill", gm)
    assert _observe(gm) == before
    assert (want.occupancy == 1.0).any()


def test_tiled_regions(gpu):
    """Regions of 40^3 voxels are cut into tiles by the library; the keys stay the caller's."""
    scene = flat_floor(n=30, dim=(40, 40, 40), resolution=0.5, level=21, holes=((0, 0), (1, 0), (-1, -1)), first=-10)
    p = R.Params(0.5, 0.0, reference_pos=(0.2, 0.2, 0.9), virtual_surface=True, floor=4.0, ceiling=4.0)
    hm, want = check(scene, p, LC.MODE_ORDERED, 0, ("repeats",), "tiled")
    assert (want.na, want.nb) == (81, 81) and want.cells == 900 and (want.occupancy == -1.0).sum() == 3


def _read_layer(gm, layer, keys, dtype, shape):
    """The blocks of `keys` of one layer as the device holds them (ohmhip_map_read_regions: no mark is cleared)."""
    keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
    out = np.empty((len(keys),) + shape, dtype=dtype)
    ptrs = (C.c_void_p * len(keys))(*[out[i].ctypes.data for i in range(len(keys))])
    L.check(L.lib.ohmhip_map_read_regions(gm._handle, layer, keys.ctypes.data, len(keys), ptrs), "read")
    return out


def test_read_only(gpu):
    """Dirty set, region list, cache stats and every layer of the map are the same before and after a build."""
    _, _, p, mode, threshold, _ = next(c for c in LC.hand_made_cases() if c[0] == "filter-single-and-multi")
    scene = LC.two_storey(mean=True)
    map_, gm = device_map(scene)
    # a sample beyond the floor's edge, in a region the scene has: a column the uploaded scene does not have
    rays = np.array([[-8.5, 2.5, 0.5], [-8.5, 2.5, -2.5]], dtype=np.float64)
    assert gm.integrateRays(rays) == rays.shape[0]  # collected rays and, once launched, dirty regions
    keys = sorted(map(tuple, gm.regionKeys()))
    voxels = scene.dim[0] * scene.dim[1] * scene.dim[2]

    def layers():
        return (_read_layer(gm, L.LID_OCCUPANCY, keys, np.float32, (voxels,)),
                _read_layer(gm, L.LID_MEAN, keys, np.uint32, (2 * voxels,)))

    occupancy, mean = layers()
    before = _observe(gm)
    assert before[1]  # something is dirty
    hm, built = layered_heightmap(gm, p, mode, threshold)
    assert built and _observe(gm) == before
    after = layers()
    assert np.array_equal(after[0].view(np.uint32), occupancy.view(np.uint32)) and np.array_equal(after[1], mean)
    # ... and the build saw the ray: it equals the restatement on the map as read back
    chunks = {k: {"occupancy": occupancy[i], "mean": mean[i]} for i, k in enumerate(keys)}
    want = LR.build_layered(R.Source(scene.resolution, scene.dim, chunks, map_.occupancy_threshold_value), p, mode,
                            threshold)
    assert_same(hm, built, want, "read only")
    assert want.cells == LR.build_layered(scene.source(), p, mode, threshold).cells + 1


# -- layer capacity, log capacity, the device variant ---------------------------------------------------------------------

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


def test_capacities_and_device_variant(gpu):
    name, scene, p, mode, threshold, _ = next(c for c in LC.hand_made_cases() if c[0] == "mean-coarse")
    _, gm = device_map(scene)
    hm, built = layered_heightmap(gm, p, mode, threshold)
    stats = hm.layered_stats
    visits, slots = int(stats.visits), int(stats.layers)
    assert built and slots == 3 and hm.occupancy.shape[0] == 3 and hm.visit_log.shape == (visits, 3)
    cp = hm.layered_params(p.reference_pos, (p.cull_min, p.cull_max))
    plane = hm.occupancy.shape[1:]
    cells = plane[0] * plane[1]
    # fewer planes and a shorter log than the walk needs: not an error, the first of each, nothing beyond them written
    small = np.full((40, 3), 0xABABABAB, dtype=np.uint32)
    occ = np.full((slots,) + plane, 7.0, dtype=np.float32)
    vox = np.zeros((slots,) + plane, dtype=hm.voxels.dtype)
    bits(vox)[...] = 0xAB
    vox_before = vox.copy()
    st = L.HeightmapLayeredStats()
    L.check(L.lib.ohmhip_map_heightmap_layered(gm._handle, C.byref(cp), 2, occ.ctypes.data, vox.ctypes.data, None, None,
                                               None, small.ctypes.data, 30, C.byref(st)), "layered")
    assert st.visits == visits and st.layers == slots
    assert np.array_equal(small[:30], hm.visit_log[:30]) and (small[30:] == 0xABABABAB).all()
    assert np.array_equal(occ[:2].view(np.uint32), hm.occupancy[:2].view(np.uint32)) and (occ[2] == 7.0).all()
    assert np.array_equal(bits(vox[:2]), bits(hm.voxels[:2])) and np.array_equal(bits(vox[2]), bits(vox_before[2]))
    for field, _ in L.HeightmapLayeredStats._fields_:
        assert getattr(st, field) == getattr(stats, field), field
    n = slots * cells
    bufs = [DeviceBuffer(4 * n), DeviceBuffer(24 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n), DeviceBuffer(cells),
            DeviceBuffer(12 * visits)]
    try:
        st = L.HeightmapLayeredStats()
        L.check(L.lib.ohmhip_map_heightmap_layered_device(gm._handle, C.byref(cp), slots, *[b.ptr for b in bufs], visits,
                                                          C.byref(st)), "device")
        gm.wait()
        shape = (slots,) + plane
        assert np.array_equal(bufs[0].read(np.uint32, shape), hm.occupancy.view(np.uint32))
        assert np.array_equal(bits(bufs[1].read(hm.voxels.dtype, shape)), bits(hm.voxels))
        assert np.array_equal(bufs[2].read(np.uint32, shape + (2,)), hm.mean)
        assert np.array_equal(bufs[3].read(np.uint32, shape), hm.source_visit)
        assert np.array_equal(bufs[4].read(np.uint8, plane), hm.layer_count)
        assert np.array_equal(bufs[5].read(np.uint32, (visits, 3)), hm.visit_log)
        for field, _ in L.HeightmapLayeredStats._fields_:
            assert getattr(st, field) == getattr(stats, field), field
    finally:
        for b in bufs:
            b.close()


# -- refusals ------------------------------------------------------------------------------------------------------------------

def test_parent_class_still_raises_and_empty_map(gpu):
    scene, p = scaled_multi_level()
    _, gm = device_map(scene)
    hm = Heightmap(0.1, 0.0)
    hm.set_occupancy_map(gm)
    for mode in (HeightmapMode.kLayeredFill, HeightmapMode.kLayeredFillUnordered):
        hm.mode = mode
        with pytest.raises(OhmHipError) as err:
            hm.build_heightmap((0, 0, 0))
        assert err.value.status == L.ERR_UNSUPPORTED
    layered = LayeredHeightmap(0.1, 0.0)
    assert layered.mode == HeightmapMode.kLayeredFill
    layered.set_occupancy_map(GpuMap(OccupancyMap(0.1)))
    assert layered.build_heightmap((0, 0, 0)) is False and layered.occupancy is None  # an empty map: nothing to build
    # the parent's modes through the subclass are the parent's builds
    layered.set_occupancy_map(gm)
    layered.mode = HeightmapMode.kPlanar
    planar = Heightmap(0.1, 0.0)
    planar.set_occupancy_map(gm)
    assert layered.build_heightmap(p.reference_pos) == planar.build_heightmap(p.reference_pos)
    assert layered.occupancy.ndim == 2 and np.array_equal(layered.occupancy.view(np.uint32),
                                                          planar.occupancy.view(np.uint32))
