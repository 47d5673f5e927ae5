"""-m gpu: ohmhip_map_copy / ohm_amd.copyMap between device maps (include/ohmhip.h, MAP COPY: C1 - C9).

The yardstick throughout is the host route on the same build: a third map `via_host` receives the source's regions by
ohmhip_map_read_regions + ohmhip_map_write_regions, and the copy's destination must equal it -- byte for byte after the
copy, and byte for byte again after both have integrated the same follow-up batch, which is where a replay mask that
was derived wrongly shows (tests/test_copy_cases.py confirms on the CPU that the follow-up batch visits and changes
planted voxels of every class).  Shapes and scenes: tests/copy_cases.py."""
import ctypes as C

import numpy as np
import pytest

import copy_cases as cases
import copy_ref as R
from ohm_amd import (LAYERS, GpuMap, GpuNdtMap, GpuTsdfMap, NdtMode, OccupancyMap, OhmHipError, canCopy, copyFilterDirty,
                     copyFilterExtents, copyLayersFilter, copyMap)
from ohm_amd import _lib as L
from ohm_amd.distributed import RegionPartition

pytestmark = pytest.mark.gpu

INF = float("inf")
OCC_LAYERS = ("occupancy", "mean", "traversal", "touch_time", "incident_normal")


def make(kind, shape, layers=None, origin=None, **kwargs):
    s = cases.SHAPES[shape]
    if kind == "occ":
        map_ = OccupancyMap(s["res"], s["dim"], layers=layers or OCC_LAYERS)
        cls = GpuMap
    elif kind == "ndt_tm":
        map_ = OccupancyMap(s["res"], s["dim"], layers=layers or ("occupancy",))
        cls, kwargs = GpuNdtMap, dict(kwargs, ndt_mode=NdtMode.kTraversability)
    elif kind == "ndt":
        map_ = OccupancyMap(s["res"], s["dim"], layers=layers or ("occupancy",))
        cls = GpuNdtMap
    else:
        map_ = OccupancyMap(s["res"], s["dim"], layers=layers or ("tsdf",))
        cls = GpuTsdfMap
    if origin is not None:
        map_.setOrigin(origin)
    return cls(map_, **kwargs)


def integrate(gm, rays, chunk=0):
    """The rays with time stamps and intensities where the map has a layer for them, in pieces of `chunk` rays."""
    n = len(rays) // 2
    ts = np.linspace(10.0, 11.0, n) if gm.hasLayer("touch_time") else None
    ints = np.linspace(1.0, 40.0, n).astype(np.float32) if gm.hasLayer("intensity") else None
    step = chunk or n
    for i in range(0, n, step):
        part = rays[2 * i:2 * (i + step)]
        assert gm.integrateRays(part, None if ints is None else ints[i:i + step],
                                None if ts is None else ts[i:i + step]) == len(part)


def keys_of(gm, dirty_only=False):
    return [tuple(int(v) for v in k) for k in gm.regionKeys(dirty_only=dirty_only)]


def read_all(gm, layers=None, keys=None):
    """{region: {layer: block}} through ohmhip_map_read_regions."""
    keys = sorted(keys_of(gm)) if keys is None else list(keys)
    out = {k: {} for k in keys}
    if not keys:
        return out
    karr = np.ascontiguousarray(keys, dtype=np.int16)
    rv = gm.map().regionVoxelVolume()
    for name in (layers or gm.map().layers):
        _, dtype, comps = LAYERS[name]
        blocks = np.empty((len(keys), rv * comps), dtype=dtype)
        ptrs = (C.c_void_p * len(keys))(*[blocks[i].ctypes.data for i in range(len(keys))])
        L.check(L.lib.ohmhip_map_read_regions(gm._handle, LAYERS[name][0], karr.ctypes.data, len(keys), ptrs), "read")
        for i, k in enumerate(keys):
            out[k][name] = blocks[i]
    return out


def write_all(gm, data, layers=None):
    """ohmhip_map_write_regions of every region of `data`, layer after layer; the first status that is not OK."""
    keys = sorted(data)
    if not keys:
        return L.OK
    karr = np.ascontiguousarray(keys, dtype=np.int16)
    for name in (layers or gm.map().layers):
        if name not in data[keys[0]]:
            continue
        blocks = [np.ascontiguousarray(data[k][name]) for k in keys]
        ptrs = (C.c_void_p * len(keys))(*[b.ctypes.data for b in blocks])
        status = L.lib.ohmhip_map_write_regions(gm._handle, LAYERS[name][0], karr.ctypes.data, len(keys), ptrs)
        if status != L.OK:
            return status
    return L.OK


def assert_same(a, b, layers=None):
    """Two {region: {layer: block}} hold the same regions and the same bytes."""
    assert sorted(a) == sorted(b)
    for k in a:
        for name in (layers or a[k]):
            assert np.array_equal(np.asarray(a[k][name]).view(np.uint8), np.asarray(b[k][name]).view(np.uint8)), (k, name)


def raw_copy(dst, src, flags=0, layers=0, keys=None, extents=None, params=True):
    p = L.CopyParams()
    p.flags, p.layers = flags, layers
    if extents is not None:
        for a in range(3):
            p.min_extents[a], p.max_extents[a] = extents[0][a], extents[1][a]
    if keys is not None:
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        p.keys_xyz, p.key_count = keys.ctypes.data, len(keys)
    st = L.CopyStats()
    status = L.lib.ohmhip_map_copy(dst._handle, src._handle, C.byref(p) if params else None, C.byref(st))
    return status, {name: int(getattr(st, name)) for name, _ in L.CopyStats._fields_}


def spatial_of(gm):
    return R.spatial_dimensions(gm.map().resolution, gm.map().region_voxel_dimensions)


def tiles_held(shape, data, layer):
    """{region: tiles of it that hold data} for the tiled shape (two z slabs: ohm_amd/csrc/tiling_impl.h): a tile a ray
    crossed has a voxel off the layer's clear value."""
    if shape != "tiled":
        return None, 1
    out = {}
    for k, blocks in data.items():
        words = np.asarray(blocks[layer]).view(np.uint32).reshape(2, -1)
        clear = 0x7f800000 if layer == "occupancy" else 0
        out[k] = int(np.any(words[0] != clear)) + int(np.any(words[1] != clear))
    return out, 2


# ---- 1. bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["odd", "unit", "default", "tiled"])
@pytest.mark.parametrize("kind", ["occ", "ndt_tm", "tsdf"])
def test_copy_equals_the_source_byte_for_byte(gpu, kind, shape):
    src, dst = make(kind, shape), make(kind, shape)
    integrate(src, cases.fan(shape))
    assert canCopy(dst, src) and not canCopy(src, src)
    before = read_all(src)
    assert len(before) >= 8
    assert copyMap(dst, src)
    assert sorted(keys_of(dst)) == sorted(keys_of(src))
    assert_same(read_all(dst), before)
    layers = src.map().layers
    if kind == "ndt_tm":
        assert set(layers) == {"occupancy", "mean", "covariance", "intensity", "hit_miss_count"}
    held, tiles = tiles_held(shape, before, "tsdf" if kind == "tsdf" else "occupancy")
    want = R.predict_stats(list(before), [], spatial_of(src), layers, layers, src.map().regionVoxelVolume(),
                           src_tiles_per_region=held, tiles_per_region=tiles)
    assert dst.lastCopyStats() == want
    # a second copy creates nothing and lands the same bytes
    assert copyMap(dst, src)
    assert dst.lastCopyStats() == dict(want, regions_created=0)
    assert_same(read_all(dst), before)


def test_clone_and_submap(gpu):
    src = make("tsdf", "odd", default_truncation_distance=0.15)
    integrate(src, cases.fan("odd"))
    whole = src.clone()
    assert type(whole) is GpuTsdfMap and whole.tsdf_options == src.tsdf_options
    assert_same(read_all(whole), read_all(src))
    box = ((0.0, 0.0, 0.0), (0.6, 0.4, 0.3))
    part = src.clone(*box)
    want, _ = R.select_regions(keys_of(src), spatial_of(src), extents=box)
    assert 0 < len(want) < len(keys_of(src)) and sorted(keys_of(part)) == sorted(want)
    assert_same(read_all(part), read_all(src, keys=sorted(want)))


# ---- 2. behaviour: the replay mask -----------------------------------------------------------------------------------
def _source_from(planted, kind, **kwargs):
    """A map that holds the planted chunks, given to it through ohmhip_map_write_regions."""
    src = make(kind, planted.shape, layers=planted.layers, **kwargs)
    assert write_all(src, planted.chunks) == L.OK
    return src


@pytest.mark.parametrize("shape,dst_trunc", [("odd", None), ("odd", 0.2), ("default", None), ("tiled", None)])
def test_tsdf_replay_mask_follows_the_copied_layer(gpu, shape, dst_trunc):
    p = cases.planted_tsdf(shape, 0.1, dst_trunc)
    src = _source_from(p, "tsdf", default_truncation_distance=0.1)
    trunc = p.options["dst_trunc"]
    dst = make("tsdf", shape, default_truncation_distance=trunc)
    via_host = make("tsdf", shape, default_truncation_distance=trunc)
    assert copyMap(dst, src)
    assert write_all(via_host, read_all(src)) == L.OK
    assert_same(read_all(dst), read_all(via_host))
    for gm in (dst, via_host):
        integrate(gm, p.rays)
    got, want = read_all(dst), read_all(via_host)
    assert_same(got, want)
    # the condition: the follow-up batch visited and changed planted voxels of every class (and the CPU agrees on which)
    changed = p.changed(want, "tsdf")
    assert all(changed[name] >= 1 for name in cases.TSDF_CLASSES), changed
    assert changed == p.changed(p.after, "tsdf")
    assert_same(got, p.after)


@pytest.mark.parametrize("shape", ["odd", "default"])
def test_ndt_replay_mask_follows_the_copied_mean(gpu, shape):
    probe = OccupancyMap()
    p = cases.planted_ndt(shape, float(probe.missProbability()))
    src = _source_from(p, "ndt")
    for name, value in p.options.items():
        assert getattr(src, {"reinit_count": "reinitialise_covariance_point_count"}.get(name, name)) == value, name
    dst, via_host = make("ndt", shape), make("ndt", shape)
    assert copyMap(dst, src)
    assert write_all(via_host, read_all(src)) == L.OK
    assert_same(read_all(dst), read_all(via_host))
    for gm in (dst, via_host):
        integrate(gm, p.rays)
    got, want = read_all(dst), read_all(via_host)
    assert_same(got, want)
    changed = p.changed(want, "occupancy")
    assert all(changed[name] >= 1 for name in cases.NDT_CLASSES), changed


def test_ndt_occupancy_into_a_plain_map(gpu):
    """C1: the modes may differ.  Only the common layers land; the plain map's mask is not the mean's business."""
    src = make("ndt", "odd")
    integrate(src, cases.fan("odd"))
    dst = make("occ", "odd", layers=("occupancy", "traversal"))
    via_host = make("occ", "odd", layers=("occupancy", "traversal"))
    assert copyMap(dst, src)
    assert dst.lastCopyStats()["layers_copied"] == 1
    assert write_all(via_host, read_all(src, layers=["occupancy"])) == L.OK
    for gm in (dst, via_host):
        integrate(gm, cases.follow_up("odd"))
    assert_same(read_all(dst), read_all(via_host))


# ---- 3. what dst already held ----------------------------------------------------------------------------------------
def test_layers_only_the_destination_has_keep_what_they_held(gpu):
    shape = "odd"
    src = make("occ", shape, layers=("occupancy", "mean"))
    dst = make("occ", shape, layers=("occupancy", "mean", "traversal"))
    integrate(src, cases.fan(shape, scale=0.6))
    integrate(dst, cases.fan(shape, shift=(0.0, 0.31, -0.23)))
    src_data, held = read_all(src), read_all(dst)
    both = sorted(set(src_data) & set(held))
    created = sorted(set(src_data) - set(held))
    kept = sorted(set(held) - set(src_data))
    assert both and created and kept
    # somewhere dst has observed a voxel the source never saw: the copy must make it unobserved
    assert any(np.any(np.isinf(src_data[k]["occupancy"]) & ~np.isinf(held[k]["occupancy"])) for k in both)
    assert copyMap(dst, src)
    assert dst.lastCopyStats()["regions_created"] == len(created)
    after = read_all(dst)
    assert sorted(after) == sorted(set(src_data) | set(held))
    for k in src_data:
        for name in ("occupancy", "mean"):
            assert np.array_equal(after[k][name].view(np.uint8), src_data[k][name].view(np.uint8)), (k, name)
    for k in both:
        assert np.array_equal(after[k]["traversal"].view(np.uint32), held[k]["traversal"].view(np.uint32))
    assert any(np.any(held[k]["traversal"] != 0) for k in both)
    for k in created:
        assert not np.any(after[k]["traversal"].view(np.uint32))
    for k in kept:
        for name in ("occupancy", "mean", "traversal"):
            assert np.array_equal(after[k][name].view(np.uint8), held[k][name].view(np.uint8)), (k, name)


def test_a_tile_the_source_lacks_reads_as_cleared(gpu):
    """Tiled regions (40 x 40 x 24: two z slabs).  The source holds the upper slab of region (0, 0, 0) only, the
    destination the lower one: after the copy the lower slab of the destination reads as cleared too."""
    def slab_rays(z_lo, z_hi):
        g = np.arange(0.2, 1.6, 0.15)
        zz = np.linspace(z_lo, z_hi, len(g))
        rays = np.empty((2 * len(g) * len(zz), 3))
        yy, zg = np.meshgrid(g, zz, indexing="ij")
        rays[0::2] = np.stack([np.full(yy.size, 0.05), yy.ravel(), zg.ravel()], axis=1)
        rays[1::2] = np.stack([np.full(yy.size, 1.7), yy.ravel(), zg.ravel()], axis=1)
        return rays
    src = make("occ", "tiled", layers=("occupancy", "mean"))
    dst = make("occ", "tiled", layers=("occupancy", "mean"))
    integrate(src, slab_rays(0.15, 1.05))
    integrate(dst, slab_rays(-1.05, -0.15))
    assert keys_of(src) == [(0, 0, 0)] and keys_of(dst) == [(0, 0, 0)]
    s, d = read_all(src)[(0, 0, 0)], read_all(dst)[(0, 0, 0)]
    lower = slice(0, 40 * 40 * 12)
    assert np.all(np.isinf(s["occupancy"][lower])) and not np.all(np.isinf(s["occupancy"][40 * 40 * 12:]))
    assert not np.all(np.isinf(d["occupancy"][lower])) and np.any(d["mean"].reshape(-1, 2)[lower])
    assert copyMap(dst, src)
    assert dst.lastCopyStats()["bytes_copied"] == 40 * 40 * 12 * 12  # one tile had a source
    assert_same(read_all(dst), read_all(src))


# ---- 4. filters ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_source(gpu):
    """One source map for the filter tests, with its bytes.  Nothing changes it: C6."""
    src = make("occ", "odd", layers=("occupancy", "mean"))
    integrate(src, cases.fan("odd"))
    return src, read_all(src)


def _fresh(shape="odd", layers=("occupancy", "mean"), **kwargs):
    return make("occ", shape, layers=layers, **kwargs)


def test_key_list_with_absent_keys(gpu, odd_source):
    src, data = odd_source
    listed = sorted(data)[1:6:2]
    keys = [listed[0], (900, 0, 0), listed[1], listed[0], listed[2], (0, -900, 7)]
    dst = _fresh()
    status, st = raw_copy(dst, src, keys=keys)
    assert status == L.OK
    assert st == R.predict_stats(list(data), [], spatial_of(src), ("occupancy", "mean"), ("occupancy", "mean"), 105, keys=keys)
    assert st["keys_absent"] == 2 and st["regions_passed"] == 3
    assert_same(read_all(dst), {k: data[k] for k in listed})


def test_extents_with_a_face_on_a_region_boundary_and_a_map_origin(gpu):
    """The box is judged against coord * region dimension, without the map origin (C3 b): the expected set comes from
    the restatement, which never sees the origin."""
    origin = (1.3, -2.7, 0.05)
    src = make("occ", "odd", layers=("occupancy",), origin=origin)
    dst = make("occ", "odd", layers=("occupancy",), origin=origin)
    integrate(src, cases.fan("odd", origin=origin))
    data = read_all(src)
    spatial = spatial_of(src)
    xs = sorted(set(k[0] for k in data))
    assert len(xs) >= 3
    cx = xs[1]
    face = float(cx) * spatial[0] + 0.5 * spatial[0]         # the upper x face of the regions at cx, as the rule forms it
    box = ((face, -INF, -INF), (INF, INF, 0.3))
    want, _ = R.select_regions(list(data), spatial, extents=box)
    assert any(k[0] == cx for k in want) and not any(k[0] < cx for k in want) and len(want) < len(data)
    assert copyMap(dst, src, copyFilterExtents(*box))
    assert sorted(keys_of(dst)) == sorted(want)
    assert_same(read_all(dst), {k: data[k] for k in want})
    # one ulp further the regions at cx are out
    dst2 = make("occ", "odd", layers=("occupancy",), origin=origin)
    box2 = ((float(np.nextafter(face, INF)), -INF, -INF), (INF, INF, 0.3))
    assert copyMap(dst2, src, copyFilterExtents(*box2))
    assert sorted(keys_of(dst2)) == sorted(k for k in want if k[0] != cx)
    # in world coordinates the two boxes would have cut elsewhere
    assert origin[0] != 0.0 and canCopy(dst, src)


def test_dirty_only(gpu):
    src = make("occ", "odd", layers=("occupancy", "mean"))
    integrate(src, cases.fan("odd"))
    L.check(L.lib.ohmhip_map_clear_dirty(src._handle), "clear_dirty")
    dst = _fresh()
    assert copyMap(dst, src, copyFilterDirty())
    assert keys_of(dst) == [] and dst.lastCopyStats()["regions_passed"] == 0
    integrate(src, cases.fan("odd", scale=0.2))
    dirty = sorted(keys_of(src, dirty_only=True))
    assert 0 < len(dirty) < len(keys_of(src))
    assert copyMap(dst, src, copyFilterDirty())
    assert sorted(keys_of(dst)) == dirty
    assert sorted(keys_of(src, dirty_only=True)) == dirty  # the copy never clears the bit
    assert_same(read_all(dst), read_all(src, keys=dirty))


def test_host_lambda(gpu, odd_source):
    src, data = odd_source
    dst = _fresh()
    seen = []

    def keep(chunk):
        seen.append(chunk.region.coord)
        assert chunk.map.region_spatial_dimensions == spatial_of(src) and chunk.dirty
        assert chunk.region.centre == R.region_centre(chunk.region.coord, spatial_of(src))
        return chunk.region.coord[0] >= 1 and chunk.region.coord[2] != 0

    want = sorted(k for k in data if k[0] >= 1 and k[2] != 0)
    assert want and len(want) < len(data)
    assert copyMap(dst, src, keep)
    assert sorted(seen) == sorted(data)
    assert_same(read_all(dst), {k: data[k] for k in want})
    # a lambda that passes nothing: true, and nothing happens
    assert copyMap(_fresh(), src, lambda chunk: False)


def test_layer_mask_that_leaves_only_mean(gpu, odd_source):
    src, data = odd_source
    dst = _fresh()
    assert copyMap(dst, src, None, copyLayersFilter(["mean", "covariance"]))
    assert dst.lastCopyStats()["layers_copied"] == 1 << LAYERS["mean"][0]
    after = read_all(dst)
    assert sorted(after) == sorted(data)
    for k in data:
        assert np.array_equal(after[k]["mean"], data[k]["mean"])
        assert np.all(np.isposinf(after[k]["occupancy"]))


def test_layer_mask_that_leaves_nothing(gpu, odd_source):
    src, data = odd_source
    dst = _fresh()
    assert copyMap(dst, src, None, lambda name: False) is True
    st = dst.lastCopyStats()
    assert st == R.predict_stats(list(data), [], spatial_of(src), ("occupancy", "mean"), ("occupancy", "mean"), 105,
                                 layer_filter=lambda name: False)
    assert st["regions_created"] == len(data) and st["bytes_copied"] == 0
    after = read_all(dst)
    assert sorted(after) == sorted(data)
    for k in after:
        assert np.all(np.isposinf(after[k]["occupancy"])) and not np.any(after[k]["mean"])


def test_no_layer_in_common(gpu, odd_source):
    src, _ = odd_source
    dst = make("tsdf", "odd")
    integrate(dst, cases.fan("odd", scale=0.4))
    before = read_all(dst)
    assert before
    assert raw_copy(dst, src)[0] == L.ERR_NOT_FOUND
    assert raw_copy(dst, src, layers=1)[0] == L.ERR_NOT_FOUND  # (before the mask is applied)
    assert copyMap(dst, src) is False
    assert_same(read_all(dst), before)


# ---- 5. src untouched ------------------------------------------------------------------------------------------------
def _limited(kind, shape, regions, spill, layers=None):
    # (a batch meets the limit when its pool is full and may not grow: the pool starts no larger than the limit)
    gm = make(kind, shape, layers=layers, region_capacity=min(64, regions))
    gm.setMemoryLimit(regions * gm.cacheStats()["bytes_per_region"])
    if spill:
        gm.setSpillToHost(True)
    return gm


def _observe(gm):
    stats = gm.cacheStats()
    listed = keys_of(gm)  # (the resident regions first, then the host store's)
    return dict(stats=stats, stored=sorted(listed[stats["regions_resident"]:]), dirty=keys_of(gm, dirty_only=True),
                count=len(listed), launched=gm.batchesLaunched())


def test_source_is_untouched_and_its_host_store_is_read_in_place(gpu):
    shape = "odd"
    src = _limited("occ", shape, 16, spill=True, layers=("occupancy", "mean"))
    integrate(src, cases.fan(shape), chunk=18)  # (a row of the fan: at most 12 regions)
    src.wait()
    before = _observe(src)
    assert before["stats"]["regions_spilled"] > 0 and before["stats"]["regions_resident"] <= 16
    data = read_all(src)
    assert _observe(src) == before  # (looking is free)
    dst = _fresh()
    assert copyMap(dst, src)
    assert _observe(src) == before
    assert_same(read_all(src), data)
    assert_same(read_all(dst), data)  # 6: the copy is complete, stored regions included
    assert dst.lastCopyStats()["regions_passed"] == before["count"] == len(data)
    # filters see the stored regions as well
    dst2 = _fresh()
    stored = before["stored"][:3]
    assert raw_copy(dst2, src, keys=stored)[0] == L.OK
    assert sorted(keys_of(dst2)) == sorted(stored) and _observe(src) == before


# ---- 6. spill on the destination -------------------------------------------------------------------------------------
def test_destination_under_a_limit_with_spill_equals_the_host_route(gpu, odd_source):
    src, data = odd_source
    dst = _limited("occ", "odd", 40, spill=True, layers=("occupancy", "mean"))
    via_host = _limited("occ", "odd", 40, spill=True, layers=("occupancy", "mean"))
    extra = cases.fan("odd", scale=0.5, shift=(0.0, 0.0, 1.1))
    for gm in (dst, via_host):
        integrate(gm, extra, chunk=27)
    assert len(data) <= 40 < len(set(data) | set(keys_of(dst)))
    assert copyMap(dst, src)
    assert write_all(via_host, data) == L.OK
    assert dst.cacheStats()["regions_spilled"] > 0
    for name in ("regions_resident", "regions_spilled"):
        assert dst.cacheStats()[name] == via_host.cacheStats()[name]
    assert_same(read_all(dst), read_all(via_host))
    for gm in (dst, via_host):
        integrate(gm, cases.follow_up("odd"), chunk=27)
    assert_same(read_all(dst), read_all(via_host))


def test_destination_under_a_limit_without_spill_fails_like_the_host_route(gpu, odd_source):
    src, data = odd_source
    assert len(data) > 12
    dst = _limited("occ", "odd", 12, spill=False, layers=("occupancy", "mean"))
    via_host = _limited("occ", "odd", 12, spill=False, layers=("occupancy", "mean"))
    want = write_all(via_host, data)
    assert want == L.ERR_CAPACITY
    status, st = raw_copy(dst, src)
    assert status == want
    assert st["regions_passed"] == len(data) and st["regions_created"] == 0 and st["bytes_copied"] == 0
    assert keys_of(dst) == keys_of(via_host) == []
    with pytest.raises(OhmHipError):
        copyMap(dst, src)
    # what fits is copied
    some = sorted(data)[:12]
    assert raw_copy(dst, src, keys=some)[0] == L.OK
    assert_same(read_all(dst), {k: data[k] for k in some})


# ---- 7. the marks of C5 ----------------------------------------------------------------------------------------------
def test_copied_regions_are_dirty_and_clearance_is_stale_as_after_an_upload(gpu, odd_source):
    src, data = odd_source
    layers = ("occupancy", "clearance")
    dst, via_host = _fresh(layers=layers), _fresh(layers=layers)
    own = cases.fan("odd", scale=0.5, shift=(0.0, 0.0, 1.1))
    radius = 0.25
    for gm in (dst, via_host):
        integrate(gm, own)
        gm.clearanceUpdate(radius)
        assert len(gm.clearanceStaleRegions(radius)) == 0
        gm.syncVoxels()
        assert keys_of(gm, dirty_only=True) == []
    listed = sorted(data)[::2]
    assert raw_copy(dst, src, keys=listed)[0] == L.OK
    assert write_all(via_host, {k: data[k] for k in listed}, layers=["occupancy"]) == L.OK
    assert sorted(keys_of(dst, dirty_only=True)) == listed
    stale = [tuple(int(v) for v in k) for k in dst.clearanceStaleRegions(radius)]
    assert stale and stale == [tuple(int(v) for v in k) for k in via_host.clearanceStaleRegions(radius)]
    for gm in (dst, via_host):
        gm.clearanceUpdate(radius)
    assert_same(read_all(dst), read_all(via_host))


# ---- 8. refusals with live maps --------------------------------------------------------------------------------------
def test_refusals(gpu, odd_source):
    src, data = odd_source
    s = cases.SHAPES["odd"]
    assert not canCopy(src, src) and raw_copy(src, src)[0] == L.ERR_INVALID_ARG
    others = [OccupancyMap(float(np.nextafter(s["res"], 1.0)), s["dim"], layers=("occupancy", "mean")),
              OccupancyMap(s["res"], (5, 3, 8), layers=("occupancy", "mean")),
              OccupancyMap(s["res"], (6, 3, 7), layers=("occupancy", "mean"))]
    moved = OccupancyMap(s["res"], s["dim"], layers=("occupancy", "mean"))
    moved.setOrigin((0.0, float(np.nextafter(0.0, 1.0)), 0.0))
    for map_ in others + [moved]:
        gm = GpuMap(map_)
        assert not canCopy(gm, src) and not canCopy(src, gm)
        assert raw_copy(gm, src)[0] == L.ERR_INVALID_ARG and raw_copy(src, gm)[0] == L.ERR_INVALID_ARG
        assert copyMap(gm, src) is False and keys_of(gm) == []
    owner = _fresh()
    owner.setRegionOwnership(2, 0)
    part = _fresh()
    part.setRegionPartition(RegionPartition(2, 1))
    plain = _fresh()
    for gm in (owner, part):
        assert canCopy(gm, src)  # (C1 is about geometry alone)
        assert raw_copy(gm, src)[0] == L.ERR_UNSUPPORTED and raw_copy(plain, gm)[0] == L.ERR_UNSUPPORTED
    merging = _fresh()
    L.check(L.lib.ohmhip_map_enable_merge(merging._handle), "enable_merge")
    assert raw_copy(merging, src)[0] == L.ERR_UNSUPPORTED
    assert raw_copy(plain, merging)[0] == L.OK  # a merging map may be read
    # live maps, bad arguments: still refused, and nothing happened
    assert raw_copy(plain, src, flags=4)[0] == L.ERR_INVALID_ARG
    assert raw_copy(plain, src, layers=1 << 10)[0] == L.ERR_INVALID_ARG
    assert raw_copy(plain, src, flags=L.COPY_USE_EXTENTS, extents=((float("nan"), 0, 0), (1, 1, 1)))[0] == L.ERR_INVALID_ARG
    assert keys_of(plain) == []
    # NULL params: everything
    assert raw_copy(plain, src, params=False)[0] == L.OK
    assert_same(read_all(plain), data)
    assert_same(read_all(src), data)
