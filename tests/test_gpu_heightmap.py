"""-m gpu: the device heightmap (ohmhip_map_heightmap / _device / _extents, ohm_amd.Heightmap) against the CPU
restatement of the planar ohm::Heightmap::buildHeightmap (tests/heightmap_ref.py) at EXACT equality: every array with
np.array_equal on the raw bits, no tolerance, no excluded cells.  Restates Heightmap.SurfaceSelection (tests/
ohmtestheightmap/HeightmapTests.cpp:686-878, 39 cases) on a device map; a map integrated from rays with every
setting; heightmap geometries other than the source's; region sizes other than 32^3 (a tiled one included), NDT, TSDF;
spill to host and the read-only guarantee; collected rays; the device-array variant."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ohm_amd import (GpuMap, GpuNdtMap, GpuTsdfMap, Heightmap, HeightmapMode, HeightmapVoxelType, OccupancyMap,
                     OhmHipError, UpAxis)
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
from heightmap_cases import (SS_DIM, SS_ORIGIN, rotate_scene, surface_selection_cases,  # noqa: E402
                             two_level_scene)

pytestmark = pytest.mark.gpu


def device_heightmap(gm, p):
    """ohm_amd.Heightmap configured from a heightmap_ref.Params, built on gm."""
    hm = Heightmap(p.grid_resolution, p.min_clearance, UpAxis(p.up_axis), p.region_size)
    hm.floor, hm.ceiling = p.floor, p.ceiling
    hm.generate_virtual_surface = p.virtual_surface
    hm.promote_virtual_below = p.promote_virtual_below
    hm.ignore_voxel_mean = p.ignore_voxel_mean
    hm.heightmap_origin = p.origin
    hm.set_occupancy_map(gm)
    cull = (p.cull_min, p.cull_max)
    built = hm.build_heightmap(p.reference_pos, cull)
    return hm, built


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same(hm, built, want, what=""):
    """Every array of the device result equals the restatement's, bit for bit."""
    if want is None:
        assert not built and hm.occupancy is None, what
        return
    e = hm.extents
    assert (e.na, e.nb, e.ma, e.mb) == (want.na, want.nb, want.ma, want.mb), what
    assert hm.occupancy.shape == want.occupancy.shape, what
    bad = np.nonzero(hm.occupancy.view(np.uint32) != want.occupancy.view(np.uint32))
    assert bad[0].size == 0, (what, "occupancy", bad[0].size, bad[0][:5], bad[1][:5])
    same = bits(hm.voxels).reshape(hm.voxels.shape + (24,)) == bits(want.voxels).reshape(want.voxels.shape + (24,))
    bad = np.nonzero(~same.all(axis=2))
    assert bad[0].size == 0, (what, "voxels", bad[0].size, bad[0][:5], bad[1][:5], hm.voxels[bad][:5],
                              want.voxels[bad][:5])
    assert (hm.mean is None) == (want.mean is None), what
    if want.mean is not None:
        assert np.array_equal(hm.mean, want.mean), (what, "mean")
    assert np.array_equal(hm.source_column, want.source_column), (what, "source_column")
    assert hm.populated_count == want.populated, what
    assert hm.cell_count == int((want.source_column != R.NO_COLUMN).sum()), what
    assert built == (want.populated != 0), what


def source_of(map_, chunks=None):
    return R.Source(map_.resolution, map_.region_voxel_dimensions, chunks if chunks is not None else map_.chunks,
                    map_.occupancy_threshold_value, map_.origin, has_mean="mean" in map_.layers)


def check(gm, map_, p, what="", surface=True, virtual=False, collide=False, chunks=None):
    src = source_of(map_, chunks)
    want = R.build_heightmap(src, p)
    # the expectation is not trivial: an all-empty result cannot pass
    if surface:
        assert want is not None and (want.occupancy == 1.0).any(), what
    if virtual:
        assert (want.occupancy == -1.0).any(), what
    if collide:
        assert want.populated > int((want.source_column != R.NO_COLUMN).sum()), what
    hm, built = device_heightmap(gm, p)
    assert_same(hm, built, want, what)
    return hm, want


# -- Heightmap.SurfaceSelection ----------------------------------------------------------------------------------------

def _ss_cases():
    m = OccupancyMap(1.0, SS_DIM)
    return list(surface_selection_cases(np.float32(m.hit_value), np.float32(m.miss_value)))


@pytest.mark.parametrize("case", _ss_cases(), ids=lambda c: c[0])
def test_surface_selection(gpu, case):
    _, chunks, p, expected_type, expected_height = case
    map_ = OccupancyMap(1.0, SS_DIM)
    map_.setOrigin(SS_ORIGIN)
    for key, c in chunks.items():
        map_.chunks[key] = {"occupancy": c["occupancy"].copy()}
    gm = GpuMap(map_)
    gm.uploadRegions(list(chunks))
    hm, built = device_heightmap(gm, p)
    want = R.build_heightmap(source_of(map_), p)
    assert_same(hm, built, want)
    # the reference's own expectation: the voxel at voxelKey((0, 0, 0)) of the heightmap
    if want is None:
        voxel_type = HeightmapVoxelType.kUnknown
    else:
        geometry = R.heightmap_geometry(source_of(map_), p, (want.min_ext, want.max_ext))[0]
        voxel_type, pos, _ = hm.get_heightmap_voxel_info(geometry.voxel_key((0.0, 0.0, 0.0)))
    assert int(voxel_type) == expected_type
    if expected_type != R.HM_UNKNOWN:
        assert pos[2] == expected_height


# -- a map integrated from rays ----------------------------------------------------------------------------------------

_SCENES = {}


def scene(up_axis=2, layers=("occupancy", "mean"), dims=(32, 32, 32), cls=GpuMap):
    """A device map of the two-level scene (synced host chunks for the restatement), cached per configuration."""
    key = (up_axis, layers, dims, cls)
    if key not in _SCENES:
        map_ = OccupancyMap(0.1, dims, layers=layers)
        gm = cls(map_)
        rays = rotate_scene(two_level_scene(), up_axis) if up_axis != 2 else two_level_scene()
        assert gm.integrateRays(rays) == rays.shape[0]
        gm.syncVoxels()
        _SCENES[key] = (map_, gm)
    return _SCENES[key]


def params(**kw):
    kw.setdefault("reference_pos", (0.0, 0.0, 0.0))
    return R.Params(kw.pop("grid_resolution", 0.1), kw.pop("min_clearance", 0.0), **kw)


def test_default_settings(gpu):
    map_, gm = scene()
    hm, want = check(gm, map_, params(), "default")
    assert (want.voxels["clearance"] > 0).any()  # floor cells under the platform
    assert (want.voxels["contributing_samples"] > 0).any()
    assert (want.voxels["flags"] == 1).any()


@pytest.mark.parametrize("promote", [False, True])
def test_virtual_surfaces(gpu, promote):
    map_, gm = scene()
    check(gm, map_, params(virtual_surface=True, promote_virtual_below=promote), "virtual", virtual=True)


def test_ignore_voxel_mean(gpu):
    map_, gm = scene()
    hm, want = check(gm, map_, params(ignore_voxel_mean=True), "ignore mean")
    assert hm.mean is None and not (want.voxels["contributing_samples"] > 0).any()


@pytest.mark.parametrize("min_clearance", [0.0, 0.5, 1.5])
def test_min_clearance(gpu, min_clearance):
    map_, gm = scene()
    check(gm, map_, params(min_clearance=min_clearance, virtual_surface=min_clearance == 0.5), "clearance")


@pytest.mark.parametrize("floor,ceiling", [(0.35, 0.0), (0.0, 0.45), (0.25, 0.75)])
def test_floor_and_ceiling(gpu, floor, ceiling):
    map_, gm = scene()
    check(gm, map_, params(floor=floor, ceiling=ceiling, reference_pos=(0.0, 0.0, 0.5), virtual_surface=True),
          "floor / ceiling", virtual=True)


@pytest.mark.parametrize("up_axis", [-3, -2, -1, 0, 1, 2])
def test_up_axes(gpu, up_axis):
    map_, gm = scene(up_axis)
    check(gm, map_, params(up_axis=up_axis, virtual_surface=True), "up %d" % up_axis, virtual=True)
    check(gm, map_, params(up_axis=up_axis, min_clearance=1.5), "up %d clearance" % up_axis)


def test_cull_box(gpu):
    map_, gm = scene()
    check(gm, map_, params(cull_min=(-1.05, -2.0, 0.0), cull_max=(2.55, 1.33, 0.0)), "cull xy")
    check(gm, map_, params(cull_min=(0.0, -2.0, -0.3), cull_max=(0.0, 1.33, 0.6), virtual_surface=True), "cull yz")
    # A cull box far from the origin of a map whose regions are cut into tiles (64^3: 8 tiles along z; no rays, one
    # uploaded region).  Region 20000 along z is addressable by the caller's int16 key while its tile coordinates,
    # 160000..160007, are beyond the packed tile key: the extents are the caller's keys and must not notice.
    far = OccupancyMap(0.1, (64, 64, 64), layers=("occupancy",))
    block = np.full(64 ** 3, np.inf, dtype=np.float32)
    block[0] = np.float32(far.hit_value)
    far.chunks[(0, 0, 0)] = {"occupancy": block}
    far_gm = GpuMap(far)
    far_gm.uploadRegions([(0, 0, 0)])
    z = 20000 * 6.4
    p = params(up_axis=1, reference_pos=(1.15, 0.0, z), cull_min=(1.0, -0.2, z - 0.15), cull_max=(1.3, 0.2, z + 0.15))
    hm, want = check(far_gm, far, p, "far tiled", surface=False)
    src, e = source_of(far), hm.extents
    assert want is not None and src.split(want.min_ext)[0][2] == 20000 and want.na > 1 and want.nb > 1
    assert e.populated == 1
    assert (tuple(e.min_region), tuple(e.min_local)[:3]) == src.split(want.min_ext)
    assert (tuple(e.max_region), tuple(e.max_local)[:3]) == src.split(want.max_ext)
    first = [divmod(c, p.region_size) for c in want.first_cell]
    assert tuple(e.first_region) == (first[0][0], first[1][0])
    assert tuple(e.first_local) == (first[0][1], first[1][1])


@pytest.mark.parametrize("reference_pos", [(0.0, 0.0, 2.5), (0.0, 0.0, 1.2), (0.0, 0.0, -0.7), (0.0, 0.0, -30.0),
                                           (100.0, -50.0, 0.45)])
def test_reference_positions(gpu, reference_pos):
    map_, gm = scene()
    check(gm, map_, params(reference_pos=reference_pos, virtual_surface=True), "reference %r" % (reference_pos,))


# -- heightmap geometry other than the source's -------------------------------------------------------------------------

@pytest.mark.parametrize("grid,origin,region_size,collide", [
    (0.2, (0.0, 0.0, 0.0), 0, True), (0.05, (0.0, 0.0, 0.0), 0, False), (0.1, (0.05, 0.05, 0.0), 0, False),
    (0.2, (0.03, -0.07, 0.4), 16, True), (0.1, (0.0, 0.0, 0.0), 16, False)])
def test_heightmap_geometry(gpu, grid, origin, region_size, collide):
    map_, gm = scene()
    check(gm, map_, params(grid_resolution=grid, origin=origin, region_size=region_size, virtual_surface=True),
          "geometry", virtual=True, collide=collide)


# -- other maps -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(16, 16, 16), (64, 64, 16), (24, 40, 48)])
def test_region_dimensions(gpu, dims):
    """16^3, and regions of more than 32 768 voxels, which the library cuts into tiles."""
    map_, gm = scene(dims=dims)
    check(gm, map_, params(virtual_surface=True), "dims %r" % (dims,), virtual=True)
    check(gm, map_, params(min_clearance=1.5, grid_resolution=0.2), "dims %r coarse" % (dims,), collide=True)


def test_ndt_map_normals_stay_zero(gpu):
    map_, gm = scene(layers=("occupancy",), cls=GpuNdtMap)
    hm, want = check(gm, map_, params(), "ndt")
    for name in ("normal_x", "normal_y", "normal_z"):
        assert not hm.voxels[name].any()


def _status(fn):
    with pytest.raises(OhmHipError) as err:
        fn()
    return err.value.status


def test_refusals(gpu):
    gt = GpuTsdfMap(OccupancyMap(0.1, layers=()), default_truncation_distance=0.2)
    hm = Heightmap(0.1, 0.0)
    hm.set_occupancy_map(gt)
    assert _status(lambda: hm.build_heightmap((0, 0, 0))) == L.ERR_UNSUPPORTED  # no occupancy layer
    map_, gm = scene()
    hm.set_occupancy_map(gm)
    hm.mode = HeightmapMode.kLayeredFill
    assert _status(lambda: hm.build_heightmap((0, 0, 0))) == L.ERR_UNSUPPORTED
    hm.mode = HeightmapMode.kPlanar
    for name, value in (("grid_resolution", 0.0), ("grid_resolution", float("nan")), ("floor", -1.0),
                        ("ceiling", float("inf")), ("min_clearance", -0.1)):
        bad = Heightmap(0.1, 0.0)
        bad.set_occupancy_map(gm)
        setattr(bad, name, value)
        assert _status(lambda: bad.build_heightmap((0, 0, 0))) == L.ERR_INVALID_ARG, name
    owner = GpuMap(OccupancyMap(0.1))
    owner.setRegionOwnership(2, 0)
    hm.set_occupancy_map(owner)
    assert _status(lambda: hm.build_heightmap((0, 0, 0))) == L.ERR_UNSUPPORTED
    empty = GpuMap(OccupancyMap(0.1))
    hm.set_occupancy_map(empty)
    assert hm.build_heightmap((0, 0, 0)) is False and hm.occupancy is None  # an empty map: not populated


# -- the map as it is used ------------------------------------------------------------------------------------------------

def _observe(gm):
    return (sorted(map(tuple, gm.regionKeys())), sorted(map(tuple, gm.regionKeys(dirty_only=True))), gm.cacheStats())


def test_spill_to_host_read_only(gpu):
    """Regions in the host store answer from their pinned records: the same arrays as the fully resident map, and the
    call changes nothing of the map."""
    layers = ("occupancy", "mean")
    map_ = OccupancyMap(0.1, layers=layers)
    gm = GpuMap(map_, region_capacity=8)
    gm.setMemoryLimit(7 * gm.cacheStats()["bytes_per_region"])  # the scene holds 9 regions
    gm.setSpillToHost(True)
    ref_map = OccupancyMap(0.1, layers=layers)
    ref = GpuMap(ref_map)
    pairs = two_level_scene().reshape(-1, 2, 3)
    pairs = pairs[np.argsort(pairs[:, 1, 0], kind="stable")]  # by end point x: a part touches few regions
    for part in np.array_split(pairs, 8):
        part = part.reshape(-1, 3)
        for g in (gm, ref):
            assert g.integrateRays(part) == part.shape[0]
    assert gm.cacheStats()["regions_spilled"] > 0
    before = _observe(gm)
    p = params(virtual_surface=True)
    hm, built = device_heightmap(gm, p)
    assert _observe(gm) == before
    full, full_built = device_heightmap(ref, p)
    assert built and full_built
    assert np.array_equal(hm.occupancy.view(np.uint32), full.occupancy.view(np.uint32))
    assert np.array_equal(bits(hm.voxels), bits(full.voxels))
    assert np.array_equal(hm.mean, full.mean) and np.array_equal(hm.source_column, full.source_column)
    assert (hm.populated_count, hm.cell_count) == (full.populated_count, full.cell_count)
    ref.syncVoxels()
    want = R.build_heightmap(source_of(ref_map), p)
    assert (want.occupancy == 1.0).any() and (want.occupancy == -1.0).any()
    assert_same(hm, built, want, "spill")


def test_collected_rays_are_seen(gpu):
    """Host batches below the coalescing threshold are still collected when the heightmap is asked for."""
    map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
    gm = GpuMap(map_)
    rays = two_level_scene()
    for part in np.array_split(rays.reshape(-1, 2, 3), 6):
        part = part.reshape(-1, 3)
        assert gm.integrateRays(part) == part.shape[0]
    p = params(virtual_surface=True)
    hm, built = device_heightmap(gm, p)
    gm.syncVoxels()
    want = R.build_heightmap(source_of(map_), p)
    assert (want.occupancy == 1.0).any()
    assert_same(hm, built, want, "collected")


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


def test_device_variant_equals_host_variant(gpu):
    map_, gm = scene()
    p = params(virtual_surface=True, grid_resolution=0.2)
    hm, built = device_heightmap(gm, p)
    assert built
    n = hm.occupancy.size
    bufs = [DeviceBuffer(4 * n), DeviceBuffer(24 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n), DeviceBuffer(16)]
    try:
        cp = hm.params(p.reference_pos, (p.cull_min, p.cull_max))
        L.check(L.lib.ohmhip_map_heightmap_device(gm._handle, C.byref(cp), *[b.ptr for b in bufs]), "device")
        gm.wait()
        shape = hm.occupancy.shape
        assert np.array_equal(bufs[0].read(np.uint32, shape), hm.occupancy.view(np.uint32))
        assert np.array_equal(bits(bufs[1].read(hm.voxels.dtype, shape)), bits(hm.voxels))
        assert np.array_equal(bufs[2].read(np.uint32, shape + (2,)), hm.mean)
        assert np.array_equal(bufs[3].read(np.uint32, shape), hm.source_column)
        counts = bufs[4].read(np.uint64, (2,))
        assert (int(counts[0]), int(counts[1])) == (hm.populated_count, hm.cell_count)
        assert hm.populated_count > hm.cell_count > 0
    finally:
        for b in bufs:
            b.close()
