"""-m gpu: the persistent per-slot state (csrc/slot_state.h: layer blocks, replay-mask row, dirty word, use stamps, merge
base) through every mover of the region pool -- growth with kept slots, compaction after a removal, roll-back of a
failed batch, eviction to the host store, re-admission by slot and by name, upload -- on the smallest maps on which each
mover has something to get wrong, checked byte for byte against the CPU oracle.

Every batch is one short ray per region, inside the region, along the row of regions (i, 0, 0): which regions a batch
touches is known exactly, and asserted on the oracle before anything runs on the device."""
import ctypes as C

import numpy as np
import pytest

from ohm_amd import GpuMap, GpuTsdfMap, OccupancyMap, _lib as L

from parity import assert_parity, compare_maps, make_oracle

pytestmark = pytest.mark.gpu

REMOVED = (1, 6, 9, 15)


def row_rays(om, dims, regions, variant):
    """One ray per region (i, 0, 0) of `regions`, from one voxel centre to another of the same region, both at least
    two voxels from the region's faces (a TSDF ray reaches one truncation distance -- a voxel -- behind its sample);
    `variant` moves both ends, so no two batches repeat a ray."""
    rays = np.empty((2 * len(regions), 3), dtype=np.float64)
    for n, i in enumerate(regions):
        rays[2 * n] = om.voxel_centre((i, 0, 0), (2 + variant % 3, 2, 2 + variant % 2))
        rays[2 * n + 1] = om.voxel_centre((i, 0, 0), (dims[0] - 3 - variant % 2, dims[1] - 3, dims[2] - 3 - variant % 3))
    rays[0::2] += 0.013  # (off the voxel centres: no ray runs along a voxel boundary)
    return rays


def row(regions):
    return {(int(i), 0, 0) for i in regions}


def keys_of(regions):
    return np.array([[i, 0, 0] for i in regions], dtype=np.int16)


def key_set(keys):
    return {tuple(int(v) for v in k) for k in keys}


def has_slot(gm, region):
    slot = C.c_uint32(0)
    status = L.lib.ohmhip_map_region_slot(gm._handle, keys_of([region]).ctypes.data, C.byref(slot))
    assert status in (L.OK, L.ERR_NOT_FOUND), status
    return status == L.OK


@pytest.mark.parametrize("dims", [(16, 16, 16), (10, 12, 9)])
@pytest.mark.parametrize("kind", ["occupancy", "tsdf"])
def test_every_mover_then_byte_equality_with_the_oracle(gpu, kind, dims):
    """(10, 12, 9): 1080 voxels, a mask row of 34 words, no layer stride a multiple of 256 -- the store record's rounding
    and both spellings of the mask row size matter.  region_capacity=4: the pool grows while earlier slots are kept.

    Steps 5 and 6 as the library behaves (the memory limit bounds pool GROWTH; a pool that was larger than the limit
    when the limit was set keeps its capacity): batch D's two regions come back into free slots of the 16-slot pool
    without an eviction, and an upload does not mark its region as modified -- the host holds what it wrote -- so the
    written key is listed by dirty_only only after the next batch touches it."""
    tsdf = kind == "tsdf"
    layers = ("tsdf",) if tsdf else ("occupancy", "mean")
    written_layer, written_lid = ("tsdf", L.LID_TSDF) if tsdf else ("occupancy", L.LID_OCCUPANCY)
    map_ = OccupancyMap(0.1, dims, layers=layers)
    gm = (GpuTsdfMap if tsdf else GpuMap)(map_, region_capacity=4)
    gm.setBatchCoalescing(0)  # every call is a device batch of its own: batch A's regions carry an older stamp than B's

    def oracle():
        om = make_oracle(map_)
        if tsdf:
            opts = gm.tsdf_options
            om.set_tsdf(max_weight=opts[0], trunc=opts[1], dropoff=opts[2], sparsity=opts[3])
        return om

    def integrate(om, rays):
        om.integrate_tsdf(rays) if tsdf else om.integrate_occupancy(rays)

    om = oracle()
    regions = {"A": range(0, 8), "B": range(8, 16), "C": range(16, 22), "D": (0, 2), "last": range(0, 22)}
    rays = {name: row_rays(om, dims, list(r), v) for v, (name, r) in enumerate(regions.items())}
    for name, r in regions.items():
        probe = oracle()
        integrate(probe, rays[name])
        assert key_set(probe.region_keys()) == row(r), name
    survivors = [i for i in range(16) if i not in REMOVED]
    a_survivors = [i for i in range(8) if i not in REMOVED]
    # the block step 6 writes: what another batch leaves in a region of this shape (a valid state of the layer)
    donor = oracle()
    integrate(donor, row_rays(donor, dims, [5], 7))
    integrate(donor, row_rays(donor, dims, [5], 8))
    block = donor.region_layer((5, 0, 0), written_layer)

    # 1. two batches, the pool grows from 4 slots to 8 and to 16
    for name in ("A", "B"):
        assert gm.integrateRays(rays[name]) == rays[name].shape[0]
    assert gm.cacheStats()["region_capacity"] == 16
    # 2. removal: holes below the new end, survivors in the tail, the last slot removed
    assert gm.removeRegions(keys_of(REMOVED)) == len(REMOVED)
    assert key_set(gm.regionKeys()) == row(survivors)
    assert key_set(gm.regionKeys(dirty_only=True)) == row(survivors)
    gm.syncVoxels()
    assert len(gm.regionKeys(dirty_only=True)) == 0
    # 3. / 4. twelve regions allowed, six new ones: the six survivors of batch A -- the older stamp -- leave
    gm.setMemoryLimit(12 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    assert gm.integrateRays(rays["C"]) == rays["C"].shape[0]
    st = gm.cacheStats()
    assert (st["evictions"], st["regions_spilled"], st["regions_resident"]) == (6, 6, 12), st
    listed = sorted(k[0] for k in key_set(gm.regionKeys()))
    assert listed == survivors + list(regions["C"])
    assert [i for i in listed if not has_slot(gm, i)] == a_survivors  # the use stamps moved with their slots in step 2
    # 5. two stored regions come back by slot
    assert gm.integrateRays(rays["D"]) == rays["D"].shape[0]
    st = gm.cacheStats()
    assert (st["readmissions"], st["evictions"], st["regions_spilled"], st["regions_resident"]) == (2, 6, 4, 14), st
    assert has_slot(gm, 0) and has_slot(gm, 2)
    # 6. two more come back by name: an upload onto one, ensure_regions on the other
    assert not has_slot(gm, 3) and not has_slot(gm, 4)
    src = (C.c_void_p * 1)(block.ctypes.data)
    L.check(L.lib.ohmhip_map_write_regions(gm._handle, written_lid, keys_of([3]).ctypes.data, 1, src), "write_regions")
    slots = np.zeros(1, dtype=np.uint32)
    L.check(L.lib.ohmhip_map_ensure_regions(gm._handle, keys_of([4]).ctypes.data, 1, slots.ctypes.data), "ensure_regions")
    assert has_slot(gm, 3) and has_slot(gm, 4)
    st = gm.cacheStats()
    # (each call makes room first: a quarter of the residents, three regions, leaves -- 14 - 3 + 1 = 12, 12 - 3 + 1 = 10)
    assert (st["readmissions"], st["evictions"], st["regions_spilled"], st["regions_resident"]) == (4, 12, 8, 10), st
    assert key_set(gm.regionKeys(dirty_only=True)) == row(list(regions["C"]) + [0, 2])
    # 7. every region once more (the removed ones start again), then the host copy
    assert gm.integrateRays(rays["last"]) == rays["last"].shape[0]
    assert key_set(gm.regionKeys(dirty_only=True)) == row(range(22))  # ... the written key (3, 0, 0) among them
    gm.syncVoxels()
    # 8. the oracle: the same batches, removed regions restarting from unobserved, the written block substituted
    keep = {"A": [i for i in regions["A"] if i not in REMOVED], "B": [i for i in regions["B"] if i not in REMOVED]}
    for v, name in enumerate(regions):
        if name == "last":
            om.region_layer_view((3, 0, 0), written_layer)[:] = block
        integrate(om, row_rays(om, dims, keep.get(name, list(regions[name])), v))
    assert len(map_.chunks) == 22
    assert_parity(compare_maps(om.chunks(), map_.chunks, list(layers), exact_float=True))


def test_the_merge_base_moves_with_its_slot(gpu):
    """A merging map through pool growth and compaction: the base of a region batch A created is what the map held when
    merging was enabled, wherever its slot went; a region created afterwards has an unobserved base.  The delta rule is
    the one test_merge_rule_on_a_non_trivial_base states, compared bitwise."""
    dims = (16, 16, 16)
    voxels = dims[0] * dims[1] * dims[2]
    map_ = OccupancyMap(0.1, dims, layers=("occupancy",))
    gm = GpuMap(map_, region_capacity=4)
    gm.setBatchCoalescing(0)
    om = make_oracle(map_)
    survivors = [i for i in range(16) if i not in REMOVED]
    batches = [row_rays(om, dims, list(range(0, 8)), 0), row_rays(om, dims, list(range(8, 16)), 1),
               row_rays(om, dims, survivors, 2)]
    for rays, expect in zip(batches, (range(0, 8), range(8, 16), survivors)):
        probe = make_oracle(map_)
        probe.integrate_occupancy(rays)
        assert key_set(probe.region_keys()) == row(expect)
    assert gm.integrateRays(batches[0]) == batches[0].shape[0]
    gm.syncVoxels()
    base = {k: c["occupancy"].copy() for k, c in map_.chunks.items()}
    assert set(base) == row(range(8))
    L.check(L.lib.ohmhip_map_enable_merge(gm._handle), "enable_merge")
    assert gm.integrateRays(batches[1]) == batches[1].shape[0]  # the pool grows with a merge base present
    assert gm.cacheStats()["region_capacity"] == 16
    assert gm.removeRegions(keys_of(REMOVED)) == len(REMOVED)
    assert gm.integrateRays(batches[2]) == batches[2].shape[0]
    keys = keys_of(survivors)
    n = len(keys)
    delta_buf, obs_buf, d_delta, d_obs = L._vp(), L._vp(), L._vp(), L._vp()
    L.check(L.lib.ohmhip_buffer_create(C.byref(delta_buf), 4 * n * voxels, 3))
    L.check(L.lib.ohmhip_buffer_create(C.byref(obs_buf), n * voxels, 3))
    L.check(L.lib.ohmhip_buffer_ptr(delta_buf, C.byref(d_delta)))
    L.check(L.lib.ohmhip_buffer_ptr(obs_buf, C.byref(d_obs)))
    L.check(L.lib.ohmhip_map_merge_pack(gm._handle, keys.ctypes.data, n, d_delta, d_obs), "merge_pack")
    delta = np.zeros(n * voxels, dtype=np.float32)
    L.check(L.lib.ohmhip_buffer_read(delta_buf, delta.ctypes.data, delta.nbytes, 0, None, None, None))
    L.lib.ohmhip_buffer_destroy(delta_buf)
    L.lib.ohmhip_buffer_destroy(obs_buf)
    gm.syncVoxels()
    zero = np.float32(0)
    for at, i in enumerate(survivors):
        v = map_.chunks[(i, 0, 0)]["occupancy"]
        assert np.isfinite(v).any()
        b = base.get((i, 0, 0), np.full(voxels, np.inf, dtype=np.float32))
        b0 = np.where(np.isinf(b), zero, b).astype(np.float32)
        expected = np.where(np.isinf(v), zero, v - b0).astype(np.float32)
        got = delta[at * voxels:(at + 1) * voxels]
        assert np.array_equal(got.view(np.uint32), expected.view(np.uint32)), (i, 0, 0)
