"""-m gpu: the device's NDT voxel update on the constructed single-voxel states and scripts of tests/ndt_cases.py, held
to the exact model (tests/ndt_ref.py) and to the CPU oracle.  States are planted by uploading a host map (uploadRegions,
which also rebuilds the per-voxel ordered-replay mask, k_rebuild_mask); coalescing is off, so a call is a device batch.

Every sheet is fed three ways:
  * one event per voxel per call, synced after every call: each transition is judged against the model from the state
    the DEVICE held before it, with the CPU bars unchanged (tests/test_ndt_ref.py: integers exact, value within one
    float32 ulp at max(|delta|, |initial|, |result|), factor terms within one ulp or, for h_zero_diag, 1e-6 relative) --
    a device exp / log a few fp64 ulp off can flip a float32 rounding but cannot leave the one-ulp ceiling;
  * everything in one call;
  * split before and after every sample that takes a voxel's count to sample_threshold (the persistent replay mask is
    set by that sample: earlier misses of a batch are counted, later ones replayed).
The three feedings must agree BIT FOR BIT: a voxel's events are the same operations in the same order however the rays
are batched.
Against the oracle: a voxel that has only seen samples must be bit identical in every layer (no transcendental on that
path; fp64 sqrt and divide are correctly rounded and contraction is off); after a miss the value may differ by the same
one ulp, measured on the single-event cases where both start from the same planted bits.  The whole map, surrounding
voxels included, passes compare_maps at the NDT comparisons' existing 1e-5."""
import numpy as np
import pytest

import ndt_cases
import ndt_ref
from ndt_cases import (Worst, geometry, judge, layers_of, make_oracle, plant, planted_tiles, read_state, same_bits,
                       step_rays)
from ohm_amd import GpuNdtMap, NdtMode, OccupancyMap
from parity import assert_parity, compare_maps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def built():
    return ndt_cases.build()


def device_map(sheet):
    geo = geometry(sheet.config)
    prm = geo.prm
    map_ = OccupancyMap(ndt_cases.RES, geo.region, layers=layers_of(prm))
    map_.setOrigin(geo.origin)
    map_.setHitValue(prm.hit_value)
    map_.setMissValue(prm.miss_value)
    map_.min_voxel_value, map_.max_voxel_value = np.float32(prm.min_value), np.float32(prm.max_value)
    map_.saturate_at_min_value, map_.saturate_at_max_value = prm.saturate_at_min, prm.saturate_at_max
    map_.ray_filter = geo.ray_filter
    map_.chunks[(0, 0, 0)] = planted_tiles(sheet)
    gm = GpuNdtMap(map_, ndt_mode=NdtMode.kTraversability if prm.ndt_tm else NdtMode.kOccupancy)
    gm.sensor_noise = prm.sensor_noise
    gm.sample_threshold = prm.sample_threshold
    gm.adaptation_rate = float(np.float32(prm.adaptation_rate))
    gm.reinitialise_covariance_threshold = prm.reinit_threshold
    gm.reinitialise_covariance_point_count = prm.reinit_count
    gm.initial_intensity_covariance = prm.initial_intensity_cov
    gm.setBatchCoalescing(0)
    return map_, gm


def device_tiles(map_, gm):
    gm.syncVoxels()
    return {name: np.array(map_.chunks[(0, 0, 0)][name], copy=True) for name in map_.layers}


def crossing_segments(sheet):
    """(case, event index) -> call number, with a cut before and after every sample that takes the count to
    sample_threshold (by the model's account of the script)."""
    geo = geometry(sheet.config)
    segment = {}
    for case in sheet.cases:
        steps = ndt_cases.run_model(geo.prm, case, geo.centre(case.local))
        seg = 0
        for k, step in enumerate(steps):
            crossing = step.kind == "H" and step.state.count == geo.prm.sample_threshold
            seg += 1 if crossing else 0
            segment[(id(case), k)] = seg
            seg += 1 if crossing else 0
    return lambda case, k: segment[(id(case), k)]


def feed(sheet, segment_of=None):
    geo = geometry(sheet.config)
    map_, gm = device_map(sheet)
    for rays, intensities in ndt_cases.all_rays(sheet, segment_of):
        assert gm.integrateRays(rays, intensities, None, geo.flags) == rays.shape[0]
    tiles = device_tiles(map_, gm)
    gm.syncVoxels()
    chunks = {k: {n: np.array(v, copy=True) for n, v in c.items()} for k, c in map_.chunks.items()}
    gm.close()
    return tiles, chunks


def test_device_transitions_hold_to_the_model_and_the_oracle(gpu, built, capsys):
    sheets, _ = built
    worst = Worst()
    equal = {}           # family -> [single-event cases bit equal to the oracle, cases, worst value gap in ulp]
    for sheet in sheets:
        geo = geometry(sheet.config)
        prm = geo.prm
        map_, gm = device_map(sheet)
        om = make_oracle(sheet.config)
        plant(om, sheet)
        before = device_tiles(map_, gm)
        planted = planted_tiles(sheet)
        for name in planted:          # the upload round trip keeps every planted bit
            assert np.array_equal(before[name].view(np.uint32), planted[name].view(np.uint32)), name
        hits_only = {id(c): True for c in sheet.cases}
        depth = max(len(c.events) for c in sheet.cases)
        for k in range(depth):
            cases, rays, intensities = step_rays(sheet, k)
            assert gm.integrateRays(rays, intensities, None, geo.flags) == rays.shape[0]
            om.integrate_ndt(rays, intensities=intensities, flags=geo.flags)
            after = device_tiles(map_, gm)
            oracle = {name: om.region_layer((0, 0, 0), name) for name in layers_of(prm)}
            for case in cases:
                vi = geo.index(case.local)
                centre = geo.centre(case.local)
                pre, post = read_state(before, vi), read_state(after, vi)
                worst.add(case.family, judge(prm, pre, case.model_events[k], centre, post, case.factor_bar))
                hits_only[id(case)] &= case.events[k][0] == "H"
                theirs = read_state(oracle, vi)
                if hits_only[id(case)]:
                    assert same_bits(post, theirs), ("hit-only path differs from the oracle", case.family, case.cell, k,
                                                     pre, post, theirs)
                if len(case.events) == 1:
                    row = equal.setdefault(case.family, [0, 0, 0.0])
                    row[1] += 1
                    row[0] += int(same_bits(post, theirs))
                    assert (post.coord, post.count, post.hit_miss, post.cov, post.intensity) == (
                        theirs.coord, theirs.count, theirs.hit_miss, theirs.cov, theirs.intensity), (case.family, pre)
                    if post.value != theirs.value:
                        step = ndt_ref.apply(prm, pre, case.model_events[k], centre)
                        gap = abs(float(post.value) - float(theirs.value)) / ndt_ref.ulp32(step.scale)
                        row[2] = max(row[2], gap)
                        assert gap <= 1.0, (case.family, case.cell, gap, pre, post, theirs)
            before = after
        gm.syncVoxels()
        # surroundings and all: the existing NDT bar over the whole map
        assert_parity(compare_maps(om.chunks(), map_.chunks, list(map_.layers), rel=1e-5))
        gm.close()
    with capsys.disabled():
        worst.show("device against the exact model, event by event (worst per family)")
        print("\n%-22s %9s %7s %16s" % ("family", "bit equal", "cases", "worst gap / ulp"))
        for family, (same, total, gap) in equal.items():
            print("%-22s %9d %7d %16.3f" % (family, same, total, gap))


def test_batching_does_not_change_a_bit(gpu, built):
    """One call, and calls cut around every threshold crossing, against one event per voxel per call."""
    sheets, _ = built
    for sheet in sheets:
        geo = geometry(sheet.config)
        depth = max(len(c.events) for c in sheet.cases)
        per_call, chunks_per_call = feed(sheet, lambda case, k: k)
        one, chunks_one = feed(sheet) if depth > 1 else (per_call, chunks_per_call)
        cut, _ = feed(sheet, crossing_segments(sheet)) if depth > 1 else (per_call, None)
        om = make_oracle(sheet.config)
        plant(om, sheet)
        for rays, intensities in ndt_cases.all_rays(sheet):
            om.integrate_ndt(rays, intensities=intensities, flags=geo.flags)
        for case in sheet.cases:
            vi = geo.index(case.local)
            a, b, c = read_state(per_call, vi), read_state(one, vi), read_state(cut, vi)
            assert same_bits(a, b), ("one call differs from one event per call", case.family, case.cell, a, b)
            assert same_bits(a, c), ("calls cut at the threshold differ", case.family, case.cell, a, c)
        assert_parity(compare_maps(om.chunks(), chunks_one, layers_of(geo.prm), rel=1e-5))
