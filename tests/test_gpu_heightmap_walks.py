"""-m gpu: what one generation walk and one set of scratch buffers under the flood-fill and the layered heightmaps
(heightmap_walk_impl.h) can get wrong, against the CPU restatements at EXACT equality.

Interleaved builds   planar, fill and layered builds in turn on one map: each leaves the walk's queue, event, accept and
                     log buffers, the per-key records and the pinned words as the next one finds them
Plane growth         the layered builds' slot planes grow more than once in a walk, by doubling and by what a generation
                     asks for, with the planes so far kept (the queue growing mid-walk: the two
                     test_generation_wider_than_a_workgroup)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import HeightmapMode
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
import heightmap_fill_ref as F  # noqa: E402
import heightmap_layered_ref as LR  # noqa: E402
import heightmap_layered_cases as LC  # noqa: E402
import test_gpu_heightmap_fill as TF  # noqa: E402
import test_gpu_heightmap_layered as TL  # noqa: E402
from heightmap_fill_cases import scaled_multi_level  # noqa: E402

pytestmark = pytest.mark.gpu

#: (build, layered mode, filter threshold)
SEQUENCE = (("planar", 0, 0), ("fill", 0, 0), ("layered", LC.MODE_ORDERED, 8), ("fill", 0, 0),
            ("layered", LC.MODE_UNORDERED, 0), ("planar", 0, 0), ("layered", LC.MODE_ORDERED, 0))
_WANT = {}


def want_of(step):
    """The restatement's result of one step of SEQUENCE on scaled_multi_level(2): computed once, left unchanged."""
    if step not in _WANT:
        scene, p = scaled_multi_level(2)
        build, mode, threshold = step
        _WANT[step] = (R.build_heightmap(scene.source(), p) if build == "planar" else
                       F.build_fill(scene.source(), p) if build == "fill" else
                       LR.build_layered(scene.source(), p, mode, threshold))
        assert _WANT[step] is not None and _WANT[step].populated > 0
    return _WANT[step]


def test_interleaved_builds_host_arrays(gpu):
    scene, p = scaled_multi_level(2)
    _, gm = TF.device_map(scene)
    for at, step in enumerate(SEQUENCE):
        build, mode, threshold = step
        want, what = want_of(step), "step %d %s" % (at, step)
        if build == "layered":
            TL.assert_same(*TL.layered_heightmap(gm, p, mode, threshold), want, what)
            continue
        hm, built = TF.fill_heightmap(gm, p, mode=HeightmapMode.kPlanar if build == "planar" else HeightmapMode.kSimpleFill)
        if build == "fill":
            TF.assert_same(hm, built, want, what)
            continue
        assert built and np.array_equal(hm.occupancy.view(np.uint32), want.occupancy.view(np.uint32)), what
        assert np.array_equal(TF.bits(hm.voxels), TF.bits(want.voxels)), what
        assert (hm.mean is None) == (want.mean is None) and (want.mean is None or np.array_equal(hm.mean, want.mean)), what
        assert np.array_equal(hm.source_column, want.source_column) and hm.populated_count == want.populated, what
        assert hm.cell_count == int((want.source_column != R.NO_COLUMN).sum()), what


def test_interleaved_builds_device_arrays(gpu):
    scene, p = scaled_multi_level(2)
    _, gm = TF.device_map(scene)
    first = want_of(SEQUENCE[0])
    plane, with_mean = first.occupancy.shape, first.mean is not None
    cells = plane[0] * plane[1]
    most_slots = max(want_of(s).slots for s in SEQUENCE if s[0] == "layered")
    most_visits = max(want_of(s).visits for s in SEQUENCE if s[0] != "planar")
    n = most_slots * cells
    # one set of device arrays for every step, filled with a pattern no result holds
    sizes = (4 * n, 24 * n, 8 * n, 4 * n, cells, 12 * most_visits, 16)
    bufs = [TF.DeviceBuffer(size) for size in sizes]
    occ, vox, mean, source, count, log, counts = bufs
    try:
        for at, step in enumerate(SEQUENCE):
            build, mode, threshold = step
            want, what = want_of(step), "step %d %s" % (at, step)
            for b, size in zip(bufs, sizes):
                pattern = np.full(max(size, 16), 0xA5, dtype=np.uint8)
                L.check(L.lib.ohmhip_buffer_write(b.handle, pattern.ctypes.data, pattern.nbytes, 0, None, None, None), what)
            hm = TL.LayeredHeightmap(p.grid_resolution, p.min_clearance, TL.UpAxis(p.up_axis), p.region_size)
            hm.floor, hm.ceiling, hm.heightmap_origin = p.floor, p.ceiling, p.origin
            hm.generate_virtual_surface, hm.promote_virtual_below = p.virtual_surface, p.promote_virtual_below
            hm.ignore_voxel_mean = p.ignore_voxel_mean
            hm.mode = HeightmapMode({"planar": 0, "fill": 1}.get(build, mode))
            hm.virtual_surface_filter_threshold = threshold
            cp = hm.layered_params(p.reference_pos, (p.cull_min, p.cull_max))
            mean_ptr = mean.ptr if with_mean else None
            shape = plane
            if build == "planar":
                L.check(L.lib.ohmhip_map_heightmap_device(gm._handle, C.byref(cp.base), occ.ptr, vox.ptr, mean_ptr,
                                                          source.ptr, counts.ptr), what)
                gm.wait()
                got = counts.read(np.uint64, (2,)).tolist()
                assert got == [want.populated, int((want.source_column != R.NO_COLUMN).sum())], (what, got)
                want_source = want.source_column
            elif build == "fill":
                st = L.HeightmapFillStats()
                L.check(L.lib.ohmhip_map_heightmap_fill_device(gm._handle, C.byref(cp.base), occ.ptr, vox.ptr, mean_ptr,
                                                               source.ptr, log.ptr, want.visits, C.byref(st)), what)
                got = (st.visits, st.populated, st.cells, st.revisits, st.generations, st.largest_generation)
                assert got == (want.visits, want.populated, want.cells, want.revisits, want.generations,
                               want.largest_generation), (what, got)
                want_source = want.source_visit
            else:
                st = L.HeightmapLayeredStats()
                shape = (want.slots,) + plane
                L.check(L.lib.ohmhip_map_heightmap_layered_device(gm._handle, C.byref(cp), want.slots, occ.ptr, vox.ptr,
                                                                  mean_ptr, source.ptr, count.ptr, log.ptr, want.visits,
                                                                  C.byref(st)), what)
                got = tuple(int(getattr(st, name)) for name in LR.STATS)
                assert got == LR.stats_of(want), (what, got, LR.stats_of(want))
                assert np.array_equal(count.read(np.uint8, plane), want.layer_count), (what, "layer_count")
                want_source = want.source_visit
            gm.wait()
            assert np.array_equal(occ.read(np.uint32, shape), want.occupancy.view(np.uint32)), (what, "occupancy")
            assert np.array_equal(TF.bits(vox.read(want.voxels.dtype, shape)), TF.bits(want.voxels)), (what, "voxels")
            if with_mean:
                assert np.array_equal(mean.read(np.uint32, shape + (2,)), want.mean), (what, "mean")
            assert np.array_equal(source.read(np.uint32, shape), want_source), (what, "source")
            if build != "planar":
                assert np.array_equal(log.read(np.uint32, (want.visits, 3)), want.log), (what, "log")
    finally:
        for b in bufs:
            b.close()


# -- the slot planes grow more than once -------------------------------------------------------------------------------------

def _case(name):
    return next(c for c in LC.hand_made_cases() if c[0] == name)


def test_planes_grow_twice_by_doubling(gpu):
    """Six voxels in one column, a step of the staircase per generation: the planes grow three times, twice by doubling."""
    name, scene, p, mode, threshold, quirks = _case("six-storeys")
    want = LR.build_layered(scene.source(), p, mode, threshold)
    grown = LC.plane_growth(want)
    assert want.layers == 6 and int(want.layer_count.max()) == 6 and len(grown) == 3, grown
    assert grown[0] == (2, 6)  # generation 1: the seed's voxel and five adds to its cell
    assert all(asked <= 2 * capacity for capacity, asked in grown[1:]), grown  # max(asked, 2 * capacity): the doubling
    TL.check(scene, p, mode, threshold, quirks, name)


@pytest.mark.parametrize("name", ["six-storeys", "too-close-real"])
def test_planes_grow_by_what_one_generation_asks(gpu, name):
    """One generation makes so many adds to one cell that it asks for more than twice the planes there are."""
    name, scene, p, mode, threshold, quirks = _case(name)
    want = LR.build_layered(scene.source(), p, mode, threshold)
    grown = LC.plane_growth(want)
    assert any(asked > 2 * capacity for capacity, asked in grown), grown  # max(asked, 2 * capacity): what was asked
    assert len(grown) >= 2, grown  # ... and the planes kept across another growth
    TL.check(scene, p, mode, threshold, quirks, name)
