"""-m gpu: the device's voxel mean update on the constructed cases of tests/mean_cases.py, held bit for bit to the exact
model (tests/mean_ref.py), to the CPU oracle and, where the exact value forces the cell, to floor(t_exact).

The arithmetic runs at three places on the device and each is a SITE here: subVoxelUpdate under applyHits
(`occupancy`), the same function in the committing pass of the kRfStopOnFirstOccupied replay (`stop`) and the second
copy, subVoxelUpdateD3 under k_replay_ndt (`ndt`); `tiled` is the occupancy site in a 48 x 48 x 48 region, which the
library cuts into z slabs, so the voxel centre has to be rebuilt from tile coordinates.  States are planted by uploading
a host map and read back from the device itself (ohmhip_map_read_regions into fresh buffers: syncVoxels copies only
regions marked as modified); coalescing is off, so a call is a device batch.  One map per sheet and site.

Every sheet is fed three ways and the three must agree bit for bit: one ray per voxel per call with a sync after every
call (each state judged), everything in one call, and one ray per voxel per call without syncs in between (the
`sequence` cases cut between every pair of their samples).  A planted count of 0xffffffff makes the update divide by
zero; the expectation there is what the x86 conversion gives (hostInt): cell 0 on every axis, count 0.  Those are
ordinary comparisons of in-range loads and stores.

test_mean_ref.py (CPU) holds the conditions the cases meet and prints their kill table; the table below says which
mutants the cases of each site catch."""
import ctypes as C

import numpy as np
import pytest

import mean_cases
from mean_cases import (NDT, calls, check_case, flags_of, geometry, layers_of, make_oracle, oracle_integrate, plant,
                        planted_tiles, read_voxel, sites_of, step_cases)
from ohm_amd import GpuMap, GpuNdtMap, NdtMode, OccupancyMap
from ohm_amd import _lib as L
from ohm_amd.gpumap import LAYERS
from parity import assert_parity, compare_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sheets():
    return mean_cases.build()


def device_map(sheet, site):
    geo = geometry(sheet.config)
    map_ = OccupancyMap(geo.res, (geo.dim,) * 3, layers=layers_of(site))
    map_.setOrigin(geo.origin)
    map_.chunks[tuple(geo.region)] = planted_tiles(sheet, site)
    if site == "ndt":
        gm = GpuNdtMap(map_, ndt_mode=NdtMode.kOccupancy)
        gm.sensor_noise = NDT["sensor_noise"]
        gm.sample_threshold = NDT["sample_threshold"]
        gm.adaptation_rate = float(np.float32(NDT["adaptation_rate"]))
        gm.reinitialise_covariance_threshold = NDT["reinit_threshold"]      # never re-initialises by value
        gm.reinitialise_covariance_point_count = NDT["reinit_count"]
    else:
        gm = GpuMap(map_)
    gm.setBatchCoalescing(0)
    return map_, gm


def synced(map_, gm):
    gm.syncVoxels()
    return {k: {n: np.array(v, copy=True) for n, v in c.items()} for k, c in map_.chunks.items()}


def read_device(map_, gm):
    """Every region the device map lists, every layer, read from the device into fresh buffers -- whether or not the
    region is marked as modified (syncVoxels copies only marked regions, and an upload marks none).  The buffers start
    as 0xa5 bytes, so a block the read did not fill cannot pass for planted data."""
    keys = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16).reshape(-1, 3)
    volume = map_.regionVoxelVolume()
    out = {tuple(int(v) for v in k): {} for k in keys}
    for name in map_.layers:
        lid, dtype, comps = LAYERS[name]
        blocks = np.full((keys.shape[0], volume * comps * np.dtype(dtype).itemsize), 0xa5, dtype=np.uint8)
        dsts = (C.c_void_p * max(1, keys.shape[0]))(*[blocks[i].ctypes.data for i in range(keys.shape[0])])
        L.check(L.lib.ohmhip_map_read_regions(gm._handle, lid, keys.ctypes.data, keys.shape[0], dsts), "read_regions")
        for i, k in enumerate(out):
            out[k][name] = blocks[i].view(dtype)
    gm.wait()
    return out


def assert_whole_map(site, oracle_chunks, device_chunks):
    if site == "ndt":
        assert_parity(compare_maps(oracle_chunks, device_chunks, layers_of(site), rel=1e-5))
        assert_parity(compare_maps(oracle_chunks, device_chunks, ["mean"]))
    else:
        assert_parity(compare_maps(oracle_chunks, device_chunks, layers_of(site), exact_float=True))


def feed(sheet, site, segment_of=None):
    """Every ray of the sheet in one call, or one call per segment, with a single sync at the end."""
    map_, gm = device_map(sheet, site)
    for rays in calls(sheet, segment_of):
        assert gm.integrateRays(rays, None, None, flags_of(site)) == rays.shape[0]
    chunks = synced(map_, gm)
    gm.close()
    return chunks


@pytest.mark.parametrize("site", mean_cases.SITES)
def test_device_mean_holds_to_the_model_and_the_oracle(gpu, sheets, site, capsys):
    judged = 0
    for sheet in sheets:
        if site not in sites_of(sheet.config):
            continue
        geo = geometry(sheet.config)
        region = tuple(geo.region)
        map_, gm = device_map(sheet, site)
        om = make_oracle(sheet, site)
        planted = plant(om, sheet, site)
        before = read_device(map_, gm)                            # the upload round trip keeps every planted bit
        assert set(before) == {region}
        for name, tile in planted.items():
            assert np.array_equal(before[region][name].view(np.uint32), tile.view(np.uint32)), (sheet.config, name)
        vi = [geo.index(c.local) for c in sheet.cases]
        held = before[region]["mean"].reshape(-1, 2)[vi]
        assert [(int(a), int(b)) for a, b in held] == [(c.coord, c.count) for c in sheet.cases]
        for k, rays in enumerate(calls(sheet, lambda case, k: k)):
            assert gm.integrateRays(rays, None, None, flags_of(site)) == rays.shape[0]
            oracle_integrate(om, site, rays)
            after = synced(map_, gm)
            theirs = {"mean": om.region_layer(region, "mean")}
            for case in step_cases(sheet, k):
                got = read_voxel(after[region], geo, case)
                check_case(case, k, got, "device, " + site)
                assert got == read_voxel(theirs, geo, case), ("device differs from the oracle", site, case.local, k)
                judged += 1
        stepped = synced(map_, gm)
        gm.close()
        assert_whole_map(site, om.chunks(), stepped)
    assert judged
    with capsys.disabled():
        mean_cases.show_site_table(sheets, only=site)


@pytest.mark.parametrize("site", mean_cases.SITES)
def test_batching_does_not_change_a_bit(gpu, sheets, site):
    """One call, and one ray per voxel per call without syncs, against the oracle's one call: the mean layer (pattern and
    count) of the whole region bit for bit, the other layers at the site's bar."""
    for sheet in sheets:
        if site not in sites_of(sheet.config):
            continue
        geo = geometry(sheet.config)
        region = tuple(geo.region)
        one = feed(sheet, site)
        cut = feed(sheet, site, lambda case, k: k)
        om = make_oracle(sheet, site)
        plant(om, sheet, site)
        for rays in calls(sheet):
            oracle_integrate(om, site, rays)
        assert_whole_map(site, om.chunks(), one)
        assert_whole_map(site, om.chunks(), cut)
        for case in sheet.cases:
            k = len(case.ends) - 1
            a, b = read_voxel(one[region], geo, case), read_voxel(cut[region], geo, case)
            check_case(case, k, a, "device, one call, " + site)
            assert a == b, ("calls cut between a voxel's samples differ from one call", site, case.family, case.local)
        assert np.array_equal(one[region]["mean"], cut[region]["mean"])
