"""-m gpu: the device ray-filter chain (GpuMap.setRayFilter(DeviceRayFilter); include/ohmhip.h:
ohmhip_map_set_ray_filter_stages) against the independent model of tests/rayfilter_chain_ref.py.

applyRayFilter equals the model bit for bit (a NaN equals a NaN) over the whole case list, for host and for device
pointers.  Maps equal the CPU oracle fed the model's output -- kept rays, moved points, flag bytes -- with the
tolerances of tests/test_gpu_rayfilter.py: occupancy, mean and TSDF exact, NDT at rel 1e-5; every call's count is the
model's kept count.  Maps are small: 0.25 m voxels, 16^3 regions, a few hundred to a few thousand rays."""
import ctypes as C
import math

import numpy as np
import pytest

from ohm_amd import (ClearingPattern, GpuMap, GpuNdtMap, GpuTsdfMap, OccupancyMap, OhmHipError, RayFlag,
                     RayPatternConical)
from ohm_amd import _lib as L
from ohm_amd import rayfilter as RF
from ohm_amd.distributed import RegionPartition

import ray_pattern_ref as R
import rayfilter_chain_cases as cases
from parity import assert_parity, compare_maps, make_oracle

pytestmark = pytest.mark.gpu

RESOLUTION = 0.25
REGION = (16, 16, 16)
MAP_CHAINS = ("good_6", "clip_3", "clip_bounded", "clip_to_bounds_body", "good_then_clip_bounded",
              "clip_then_clip_bounded", "clip_bounded_then_clip_to_bounds", "clip_bounded_then_clip")


class DeviceArray:
    """A device buffer of the library's holding a copy of a numpy array."""

    def __init__(self, array=None, nbytes=0):
        self.handle = L._vp()
        nbytes = array.nbytes if array is not None else nbytes
        L.check(L.lib.ohmhip_buffer_create(C.byref(self.handle), max(nbytes, 1), 3))
        if array is not None and array.nbytes:
            array = np.ascontiguousarray(array)
            L.check(L.lib.ohmhip_buffer_write(self.handle, array.ctypes.data, array.nbytes, 0, None, None, None))
        self.ptr = L._vp()
        L.check(L.lib.ohmhip_buffer_ptr(self.handle, C.byref(self.ptr)))

    def read(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            L.check(L.lib.ohmhip_buffer_read(self.handle, out.ctypes.data, out.nbytes, 0, None, None, None))
        return out

    def close(self):
        L.lib.ohmhip_buffer_destroy(self.handle)


def new_map(layers=("occupancy", "mean"), map_type=GpuMap, region=REGION, coalesce=256, **kwargs):
    map_ = OccupancyMap(RESOLUTION, region, layers=layers)
    gm = map_type(map_, **kwargs)
    if coalesce is not None:
        gm.setBatchCoalescing(coalesce)
    return map_, gm


def model_output(stages, rays):
    """(kept rays as (2K, 3), their flag bytes, keep mask) of the model: what the oracle is fed."""
    keep, out, flags = cases.run_model(stages, rays)
    kept = np.empty((2 * int(keep.sum()), 3))
    kept[0::2] = out[0::2][keep]
    kept[1::2] = out[1::2][keep]
    return kept, flags[keep], keep


def map_rays(n, seed):
    return cases.random_rays(n, seed=seed)


# -- the arithmetic --------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def query_map(gpu):
    map_, gm = new_map()
    yield gm
    gm.close()


@pytest.mark.parametrize("chain_name", sorted(cases.CHAINS))
def test_apply_ray_filter_equals_model(query_map, chain_name):
    gm = query_map
    rays = cases.all_rays()
    gm.setRayFilter(cases.device_filter(cases.CHAINS[chain_name]))
    keep, out, flags = gm.applyRayFilter(rays)
    cases.assert_equals_model(chain_name, keep, out, flags, "applyRayFilter, host pointers")
    n = rays.shape[0] // 2
    d_in, d_out, d_flags = DeviceArray(rays), DeviceArray(nbytes=rays.nbytes), DeviceArray(nbytes=n)
    try:
        kept = gm.applyRayFilterDevice(d_in.ptr, rays.shape[0], d_out.ptr, d_flags.ptr)
        flags = d_flags.read(np.uint8, n)
        out = d_out.read(np.float64, rays.size).reshape(-1, 3)
        assert cases.same_bits(d_in.read(np.float64, rays.size), rays.reshape(-1)).all()  # the input is not written
        assert kept == gm.applyRayFilterDevice(d_in.ptr, rays.shape[0])                      # outputs are optional
    finally:
        for buf in (d_in, d_out, d_flags):
            buf.close()
    assert kept == int(cases.model(chain_name)[0].sum())
    cases.assert_equals_model(chain_name, (flags & 1) == 0, out, flags, "applyRayFilter, device pointers")
    gm.clearRayFilter()


def test_stage_readback_and_refusals(gpu):
    map_, gm = new_map()
    h = gm._handle
    count = C.c_uint(9)
    assert L.lib.ohmhip_map_ray_filter_stages(h, None, 0, C.byref(count)) == L.OK and count.value == 0
    gm.setRayFilter(cases.device_filter(cases.CHAINS["four_stages"]))
    got = (L.RayFilterStage * 4)()
    assert L.lib.ohmhip_map_ray_filter_stages(h, got, 4, C.byref(count)) == L.OK and count.value == 4
    assert [s.kind for s in got] == [1, 3, 4, 2] and got[0].range == 50.0 and got[3].range == 2.5
    assert tuple(got[1].box_min) == cases.BOX[0] and tuple(got[2].box_max) == cases.BODY[1]
    bad = (L.RayFilterStage * 5)()
    for st in bad:
        st.kind = L.RFS_GOOD
    set_stages = L.lib.ohmhip_map_set_ray_filter_stages
    assert set_stages(h, bad, 5) == L.ERR_INVALID_ARG
    assert set_stages(h, None, 1) == L.ERR_INVALID_ARG
    bad[1].kind = 5
    assert set_stages(h, bad, 2) == L.ERR_INVALID_ARG
    bad[1].kind = 0
    assert set_stages(h, bad, 2) == L.ERR_INVALID_ARG
    bad[1].kind, bad[1].reserved = L.RFS_CLIP, 7
    assert set_stages(h, bad, 2) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_ray_filter_stages(h, None, 0, C.byref(count)) == L.OK and count.value == 4  # still the chain
    bad[1].reserved, bad[1].range = 0, math.nan  # a NaN is accepted: the comparisons decide
    assert set_stages(h, bad, 2) == L.OK
    assert set_stages(h, None, 0) == L.OK
    assert L.lib.ohmhip_map_ray_filter_stages(h, None, 0, C.byref(count)) == L.OK and count.value == 0
    # no chain: rays come back as given, flags 0
    rays = cases.edge_rays()[1]
    keep, out, flags = gm.applyRayFilter(rays)
    assert keep.all() and not flags.any() and cases.same_bits(out, rays).all()
    gm.close()


# -- maps against the oracle fed the model's output ---------------------------------------------------------------------------

def integrate_host(gm, rays, flags, **arrays):
    return gm.integrateRays(rays, ray_update_flags=flags, **arrays)


def integrate_device(gm, rays, flags, **arrays):
    assert not arrays
    buf = DeviceArray(rays)
    try:
        return gm.integrateRaysDevice(buf.ptr, rays.shape[0], flags)
    finally:
        gm.wait()
        buf.close()


@pytest.mark.parametrize("route", [integrate_host, integrate_device], ids=["host", "device"])
@pytest.mark.parametrize("chain_name", MAP_CHAINS)
def test_occupancy_and_mean_match_oracle(gpu, chain_name, route):
    stages = cases.CHAINS[chain_name]
    layers = ("occupancy", "mean")
    map_, gm = new_map(layers)
    gm.setRayFilter(cases.device_filter(stages))
    assert isinstance(gm.rayFilter(), RF.DeviceRayFilter) and gm.effectiveRayFilter() is gm.rayFilter()
    om = make_oracle(map_)
    rays = map_rays(1500, seed=11)
    for flags in (0, int(RayFlag.kRfExcludeOrigin)):
        for at in range(0, rays.shape[0], 2 * 700):  # 700, 700 and 100 rays: direct batches and one collected call
            chunk = rays[at:at + 2 * 700]
            kept, fflags, keep = model_output(stages, chunk)
            assert route(gm, chunk, flags) == kept.shape[0]
            om.integrate_occupancy(kept, flags=flags, filter_flags=fflags)
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
    gm.close()


@pytest.mark.parametrize("chain_name", MAP_CHAINS)
def test_ndt_and_tsdf_match_oracle(gpu, chain_name):
    stages = cases.CHAINS[chain_name]
    rays = map_rays(1200, seed=12)
    map_n, gn = new_map(("occupancy",), GpuNdtMap)
    on = make_oracle(map_n)
    on.set_ndt(sensor_noise=gn.sensor_noise, sample_threshold=gn.sample_threshold, adaptation_rate=gn.adaptation_rate,
               reinit_threshold=gn.reinitialise_covariance_threshold,
               reinit_count=gn.reinitialise_covariance_point_count, ndt_tm=False)
    map_t, gt = new_map(("tsdf",), GpuTsdfMap, default_truncation_distance=0.5)
    ot = make_oracle(map_t)
    opts = gt.tsdf_options
    ot.set_tsdf(max_weight=opts[0], trunc=opts[1], dropoff=opts[2], sparsity=opts[3])
    for gm in (gn, gt):
        gm.setRayFilter(cases.device_filter(stages))
    for route in (integrate_host, integrate_device):
        for at in range(0, rays.shape[0], 2 * 500):
            chunk = rays[at:at + 2 * 500]
            kept, fflags, _ = model_output(stages, chunk)
            assert route(gn, chunk, 0) == kept.shape[0]
            assert route(gt, chunk, 0) == kept.shape[0]
            on.integrate_ndt(kept, filter_flags=fflags)
            ot.integrate_tsdf(kept, filter_flags=fflags)
    gn.syncVoxels()
    gt.syncVoxels()
    assert_parity(compare_maps(on.chunks(), map_n.chunks, list(map_n.layers), rel=1e-5))
    assert_parity(compare_maps(ot.chunks(), map_t.chunks, ["tsdf"], exact_float=True))
    gn.close()
    gt.close()


@pytest.mark.parametrize("route", [integrate_host, integrate_device], ids=["host", "device"])
def test_collected_calls_count_for_themselves_and_keep_their_chain(gpu, route):
    """Seven 300-ray calls wait in the coalescing buffer as one device batch, each reporting its own count.  Setting
    another chain launches them first: they were counted by the old chain and are filtered by it."""
    layers = ("occupancy", "mean")
    map_, gm = new_map(layers, coalesce=1 << 16)
    om = make_oracle(map_)
    first, second = cases.CHAINS["clip_bounded"], cases.CHAINS["clip_then_clip_bounded"]
    rays = map_rays(2 * 7 * 300, seed=13)
    gm.setRayFilter(cases.device_filter(first))
    launched = gm.batchesLaunched()
    buffers = []
    for call in range(14):
        if call == 7:
            assert gm.batchesLaunched() == launched      # nothing has run yet
            gm.setRayFilter(cases.device_filter(second))
            assert gm.batchesLaunched() == launched + 1  # the seven calls, as one batch, under the chain that counted them
        stages = first if call < 7 else second
        chunk = rays[call * 600:(call + 1) * 600]
        kept, fflags, _ = model_output(stages, chunk)
        if route is integrate_device:
            buffers.append(DeviceArray(chunk))
            assert gm.integrateRaysDevice(buffers[-1].ptr, chunk.shape[0]) == kept.shape[0]
        else:
            assert gm.integrateRays(chunk) == kept.shape[0]
        om.integrate_occupancy(kept, filter_flags=fflags)
    gm.syncVoxels()
    assert gm.batchesLaunched() == launched + 2
    for buf in buffers:
        buf.close()
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
    gm.close()


def test_all_rejected_returns_zero_and_creates_no_region(gpu):
    map_, gm = new_map()
    gm.setRayFilter(RF.on_device(RF.good_ray(1e-3)))
    rays = map_rays(400, seed=14)
    assert gm.integrateRays(rays) == 0                     # a batch of its own
    assert gm.integrateRays(rays[:200]) == 0               # a collected call
    buf = DeviceArray(rays)
    assert gm.integrateRaysDevice(buf.ptr, rays.shape[0]) == 0
    gm.syncVoxels()
    buf.close()
    assert len(map_.chunks) == 0 and gm.cacheStats()["regions_resident"] == 0
    assert gm.stats()["rays_integrated"] == 0
    gm.close()


def test_time_base_is_the_first_stamp_submitted(gpu):
    """The base of the touch-time layer comes from the first stamp of the call as submitted, also when the chain
    rejects that ray (ohmgpu/GpuMap.cpp:593 runs before the filter at :736)."""
    layers = ("occupancy", "mean", "touch_time")
    stages = cases.CHAINS["good_then_clip_bounded"]
    for route in ("host", "device"):
        map_, gm = new_map(layers)
        om = make_oracle(map_)
        gm.setRayFilter(cases.device_filter(stages))
        rays = map_rays(600, seed=15).copy()
        rays[0], rays[1] = (-3.0, 0.0, 0.2), (4.0, 0.3, 0.3)  # 7 m: goodRay(6) rejects the first ray
        ts = 1000.5 + 0.01 * np.arange(rays.shape[0] // 2)
        kept, fflags, keep = model_output(stages, rays)
        assert not keep[0] and gm.firstRayTime() < 0
        if route == "host":
            assert gm.integrateRays(rays, timestamps=ts) == kept.shape[0]
        else:
            d_rays, d_ts = DeviceArray(rays), DeviceArray(ts)
            assert gm.integrateRaysDevice(d_rays.ptr, rays.shape[0], d_timestamps=d_ts.ptr) == kept.shape[0]
            gm.wait()
            d_rays.close()
            d_ts.close()
        assert gm.firstRayTime() == ts[0]
        om.set_first_ray_time(ts[0])
        om.integrate_occupancy(kept, timestamps=ts[keep], filter_flags=fflags)
        gm.syncVoxels()
        assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
        gm.close()


def test_nan_end_clip_to_bounds_creates_no_null_key_region(gpu):
    """clipToBounds on a ray whose end has a NaN coordinate: Aabb::contains counts it as contained, the end is flagged
    clipped and no sample lands on Key::kNull's voxel, region (-32768)^3."""
    map_, gm = new_map()
    map_.ray_filter = None  # (the chain stands in place of the built-in filter either way)
    stages = cases.CHAINS["clip_to_bounds"]
    gm.setRayFilter(cases.device_filter(stages))
    rays = map_rays(300, seed=16).copy()
    rays[0], rays[1] = (0.0, 0.0, 0.0), (math.nan, 0.5, 0.5)
    keep, out, flags = gm.applyRayFilter(rays)
    assert keep[0] and flags[0] == RF.kRffClippedEnd
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    assert map_.chunks and not any(-32768 in key for key in map_.chunks)
    gm.close()


def test_clear_ray_filter_brings_the_built_in_filter_back(gpu):
    layers = ("occupancy", "mean")
    map_, gm = new_map(layers)
    map_.ray_filter = ("good", 4.0)
    om = make_oracle(map_)
    rays = map_rays(800, seed=17)
    stages = cases.CHAINS["clip_bounded"]
    gm.setRayFilter(cases.device_filter(stages))
    kept, fflags, _ = model_output(stages, rays)
    assert gm.integrateRays(rays) == kept.shape[0]
    om.integrate_occupancy(kept, filter_flags=fflags)
    gm.clearRayFilter()
    assert gm.rayFilter() is None
    good, _, _ = model_output([("good", 4.0)], rays)
    assert 0 < good.shape[0] < rays.shape[0]
    assert gm.integrateRays(rays) == good.shape[0]  # goodRayFilter(4): the map's own
    om.integrate_occupancy(rays)
    # a host callable takes the place of a device chain, and the other way round
    gm.setRayFilter(cases.device_filter(stages))
    gm.setRayFilter(RF.clip_to_bounds(RF.Aabb(*cases.BODY)))
    count = C.c_uint(9)
    assert L.lib.ohmhip_map_ray_filter_stages(gm._handle, None, 0, C.byref(count)) == L.OK and count.value == 0
    assert not isinstance(gm.rayFilter(), RF.DeviceRayFilter)
    gm.clearRayFilter()
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
    gm.close()


def test_caller_filtered_batch_with_an_invalid_flag_counts_what_it_integrates(gpu):
    """ohmhip_map_integrate_rays_filtered: a ray handed over with kRffInvalid all the same is neither integrated nor
    counted, in a batch of its own (the device counts) and in a collected call (the host counts)."""
    layers = ("occupancy", "mean")
    map_, gm = new_map(layers)
    om = make_oracle(map_)
    rays = map_rays(900, seed=21)
    for at, n in ((0, 600), (600, 200), (800, 100)):  # a batch of its own, then two collected calls
        chunk = np.ascontiguousarray(rays[2 * at:2 * (at + n)])
        fflags = np.zeros(n, dtype=np.uint8)
        fflags[::7] = RF.kRffInvalid
        fflags[3::11] |= RF.kRffClippedEnd
        valid = (fflags & RF.kRffInvalid) == 0
        done = C.c_size_t(0)
        L.check(L.lib.ohmhip_map_integrate_rays_filtered(gm._handle, chunk.ctypes.data, chunk.shape[0], None, None, 0,
                                                         fflags.ctypes.data, C.byref(done)))
        assert done.value == 2 * int(valid.sum())
        om.integrate_occupancy(chunk[np.repeat(valid, 2)], filter_flags=fflags[valid])
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
    gm.close()


# -- additional legs --------------------------------------------------------------------------------------------------------

def test_tiled_map_with_large_regions(gpu):
    layers = ("occupancy", "mean")
    stages = cases.CHAINS["clip_bounded_then_clip"]
    map_, gm = new_map(layers, region=(64, 64, 64))
    gm.setRayFilter(cases.device_filter(stages))
    om = make_oracle(map_)
    rays = map_rays(1500, seed=18)
    kept, fflags, _ = model_output(stages, rays)
    assert gm.integrateRays(rays) == kept.shape[0]
    om.integrate_occupancy(kept, filter_flags=fflags)
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
    gm.close()


def test_memory_limit_with_spill(gpu):
    """A residency limit of 40 regions (2 m each) under batches that touch more: a batch is repeated after evictions, and
    presented again as halves when it alone does not fit (a 3 m ray crosses at most 9 regions) -- every attempt filters
    the rays as presented.  (The pool's size and the limit are those of tests/test_gpu_host_batches.py.)"""
    layers = ("occupancy", "mean")
    stages = cases.CHAINS["clip_then_clip_bounded"]
    map_, gm = new_map(layers, region=(8, 8, 8), coalesce=0, region_capacity=64)
    gm.setMemoryLimit(40 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    gm.setRayFilter(cases.device_filter(stages))
    om = make_oracle(map_)
    rays = map_rays(900, seed=19)
    for at in range(0, rays.shape[0], 2 * 300):
        chunk = rays[at:at + 2 * 300]
        kept, fflags, _ = model_output(stages, chunk)
        assert gm.integrateRays(chunk) == kept.shape[0]
        om.integrate_occupancy(kept, filter_flags=fflags)
    gm.syncVoxels()
    assert gm.cacheStats()["evictions"] > 0
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))
    gm.close()


def test_clearing_pattern_under_a_chain(gpu):
    """ClearingPattern.apply builds its rays on the device and integrates them through the map: the chain filters them
    there.  Against the pattern's CPU model filtered by the chain's model."""
    stages = cases.CHAINS["clip_bounded"]
    map_, gm = new_map(("occupancy",))
    map_.setMissProbability(0.1)
    om = make_oracle(map_)
    cone = RayPatternConical((1.0, 0.0, 0.0), math.radians(50.0), 4.0, math.radians(10.0))
    clearing = ClearingPattern(cone)
    flags = int(ClearingPattern.kDefaultRayFlags)
    walls = map_rays(600, seed=20)
    assert gm.integrateRays(walls) == walls.shape[0]
    om.integrate_occupancy(walls)
    gm.setRayFilter(cases.device_filter(stages))
    for position in ((0.05, 0.05, 0.05), (-2.5, 0.3, 0.1)):  # a sensor inside the box, and one outside looking in
        pose = np.array(position + tuple(R.angle_axis(0.3, (0, 0, 1))))
        pattern_rays = R.build_rays(cone.rayPoints(), [pose])
        kept, fflags, keep = model_output(stages, pattern_rays)
        assert clearing.apply(gm, pose[:3], pose[3:]) == kept.shape[0]
        om.integrate_occupancy(kept, flags=flags & ~int(RayFlag.kRfReverseWalk), filter_flags=fflags)
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy"], exact_float=True))
    gm.close()


def test_partitioned_maps_refuse_a_chain(gpu):
    chain = cases.device_filter(cases.CHAINS["clip_bounded"])
    map_a, a = new_map()
    a.setRegionPartition(RegionPartition(2, 1))
    with pytest.raises(OhmHipError) as err:
        a.setRayFilter(chain)
    assert err.value.status == L.ERR_UNSUPPORTED and a.rayFilter() is None
    map_b, b = new_map()
    b.setRayFilter(chain)
    with pytest.raises(OhmHipError) as err:
        b.setRegionPartition(RegionPartition(2, 1))
    assert err.value.status == L.ERR_UNSUPPORTED
    with pytest.raises(OhmHipError) as err:
        b.setRegionOwnership(2, 0)
    assert err.value.status == L.ERR_UNSUPPORTED
    b.clearRayFilter()
    b.setRegionOwnership(2, 0)
    with pytest.raises(OhmHipError) as err:
        b.setRayFilter(chain)
    assert err.value.status == L.ERR_UNSUPPORTED
    a.close()
    b.close()
