"""-m gpu: surface normals in the device heightmap (OHMHIP_HM_SURFACE_NORMALS, Heightmap.surface_normals) against the
decomposition model (tests/covariance_eigen_ref.py, D6) applied to the ground voxel of each cell, bit for bit, in the
planar and the flood-fill mode and under all six up axes; every other field and array equal to the build with the flag
off; zeros in free (virtual), and unwritten cells and on maps without the covariance layer.  Planted scenes hold exactly
one occupied voxel per source column, with the covariances of tests/covariance_cases.py cycled through them; one scene
is integrated from rays by the NDT mapper."""
import os
import sys

import numpy as np
import pytest

from ohm_amd import GpuMap, GpuNdtMap, Heightmap, HeightmapMode, OccupancyMap, UpAxis

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covariance_cases as cases  # noqa: E402
import covariance_eigen_ref as cov_ref  # noqa: E402
import heightmap_normals_ref as N  # noqa: E402
import heightmap_ref as R  # noqa: E402
from heightmap_cases import two_level_scene  # noqa: E402

pytestmark = pytest.mark.gpu

DIM = (16, 16, 16)
UP_AXES = [-3, -2, -1, 0, 1, 2]
NO_VISIT = 0xFFFFFFFF
NORMALS = ("normal_x", "normal_y", "normal_z")
INF = np.float32(np.inf)


def planted_chunks(up_axis, two_level=False):
    """Host chunks of a scene with one occupied voxel per column of a 26 x 20 patch -- a tilted plane of 17 levels one
    voxel apart, or two flat levels seven voxels apart (up coordinates 3 and 10: inside the map's extents, whose lowest
    voxel layer the reference's downward search does not reach) --, the covariance cases cycled through them, and a
    strip of columns that hold one free voxel each (virtual surface cells).  Returns (chunks, {(ga, gb): case index})."""
    a, b, up = R.axis_indices(up_axis)
    P = cases.all_p()
    chunks, case_of = {}, {}

    def voxel(g):
        region = tuple(g[c] // DIM[c] for c in range(3))
        local = [g[c] % DIM[c] for c in range(3)]
        if region not in chunks:
            chunks[region] = {"occupancy": np.full(4096, INF, dtype=np.float32), "mean": np.zeros(8192, dtype=np.uint32),
                              "covariance": np.zeros(4096 * 6, dtype=np.float32)}
        return chunks[region], local[0] + 16 * (local[1] + 16 * local[2])

    k = 0
    for gb in range(-6, 14):
        for ga in range(-5, 21):
            g = [0, 0, 0]
            g[a], g[b] = ga, gb
            g[up] = (3 if ga < 8 else 10) if two_level else (ga + 2 * gb) // 4
            chunk, vi = voxel(g)
            chunk["occupancy"][vi] = np.float32(2.0)
            chunk["covariance"][6 * vi:6 * vi + 6] = P[k % P.shape[0]]
            case_of[(ga, gb)] = k % P.shape[0]
            k += 1
    for gb in (15, 16):
        for ga in range(-5, 21):
            g = [0, 0, 0]
            g[a], g[b], g[up] = ga, gb, 2
            chunk, vi = voxel(g)
            chunk["occupancy"][vi] = np.float32(-1.0)
            chunk["covariance"][6 * vi:6 * vi + 6] = P[5]  # must not show: the cell's ground voxel is free
    return chunks, case_of


def planted_map(up_axis, layers=("occupancy", "mean", "covariance"), cls=GpuNdtMap, two_level=False):
    chunks, case_of = planted_chunks(up_axis, two_level)
    map_ = OccupancyMap(0.1, DIM, layers=layers)
    for key, c in chunks.items():
        map_.chunks[key] = {name: c[name].copy() for name in layers}
    gm = cls(map_)
    gm.uploadRegions(sorted(chunks))
    return map_, gm, case_of


def build(gm, p, normals, mode=HeightmapMode.kPlanar):
    hm = Heightmap(p.grid_resolution, p.min_clearance, UpAxis(p.up_axis), p.region_size)
    hm.generate_virtual_surface = p.virtual_surface
    hm.ignore_voxel_mean = p.ignore_voxel_mean
    hm.mode = mode
    hm.keep_visit_log = mode == HeightmapMode.kSimpleFill
    hm.surface_normals = normals
    hm.set_occupancy_map(gm)
    cull = (p.cull_min, p.cull_max)
    assert hm.build_heightmap(p.reference_pos, cull)
    return hm


def normals_of(voxels):
    return np.stack([voxels[name] for name in NORMALS], axis=-1)


def assert_only_normals_differ(on, off, what=""):
    """Every field and array of the build with normals equals the build without, the three normal floats aside, and
    the build without holds zeros there."""
    assert not normals_of(off.voxels).view(np.uint32).any(), what
    stripped = on.voxels.copy()
    for name in NORMALS:
        stripped[name] = 0
    assert stripped.tobytes() == off.voxels.tobytes(), what
    assert on.occupancy.tobytes() == off.occupancy.tobytes(), what
    assert (on.mean is None) == (off.mean is None) and (on.mean is None or np.array_equal(on.mean, off.mean)), what
    for name in ("source_column", "source_visit", "visit_log"):
        x, y = getattr(on, name), getattr(off, name)
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), (what, name)
    assert (on.populated_count, on.cell_count) == (off.populated_count, off.cell_count), what


def assert_normals(hm, want, what=""):
    got = normals_of(hm.voxels)
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=2))
    assert bad[0].size == 0, (what, bad[0].size, bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4])
    # free (virtual) and unwritten cells hold zeros, the sign bit included
    assert not got.view(np.uint32)[hm.occupancy != 1.0].any(), what


def source(map_):
    return R.Source(map_.resolution, map_.region_voxel_dimensions, map_.chunks, map_.occupancy_threshold_value,
                    map_.origin, has_mean="mean" in map_.layers)


def extents_of(hm):
    e = hm.extents
    lo = [int(e.min_region[c]) * DIM[c] + int(e.min_local[c]) for c in range(3)]
    hi = [int(e.max_region[c]) * DIM[c] + int(e.max_local[c]) for c in range(3)]
    return lo, hi


def planted_params(up_axis):
    return R.Params(0.1, 0.0, up_axis=up_axis, virtual_surface=True, ignore_voxel_mean=True)


@pytest.mark.parametrize("up_axis", UP_AXES)
def test_planar_tilted_plane(gpu, up_axis):
    map_, gm, case_of = planted_map(up_axis)
    p = planted_params(up_axis)
    off, on = build(gm, p, False), build(gm, p, True)
    assert_only_normals_differ(on, off, "planar up %d" % up_axis)
    want, occupied = N.expected_normals(source(map_), p, extents_of(on), int(on.extents.na), on.source_column)
    assert occupied >= cases.all_p().shape[0] and (on.occupancy == -1.0).any() and (on.occupancy == INF).any()
    assert_normals(on, want, "planar up %d" % up_axis)
    gm.close()


@pytest.mark.parametrize("up_axis", UP_AXES)
@pytest.mark.parametrize("two_level", [True, False], ids=["two_levels", "tilted_plane"])
def test_fill(gpu, up_axis, two_level):
    map_, gm, case_of = planted_map(up_axis, two_level=two_level)
    p = planted_params(up_axis)
    off = build(gm, p, False, HeightmapMode.kSimpleFill)
    on = build(gm, p, True, HeightmapMode.kSimpleFill)
    what = "fill up %d two_level %d" % (up_axis, two_level)
    assert_only_normals_differ(on, off, what)
    # the ground voxel of a cell is the single occupied voxel of the column its visit walked
    a, b, up = R.axis_indices(up_axis)
    lo, _ = extents_of(on)
    results = cases.model_results()
    want = np.zeros(on.occupancy.shape + (3,), dtype=np.float32)
    reached = set()
    for cb, ca in zip(*np.nonzero(on.source_visit != NO_VISIT)):
        if on.occupancy[cb, ca] != 1.0:
            continue
        ia, ib, _ = on.visit_log[int(on.source_visit[cb, ca])]
        column = (lo[a] + int(ia), lo[b] + int(ib))
        want[cb, ca] = cov_ref.normal_for_up(results[case_of[column]], N.up_vector(up_axis))
        reached.add(column)
    assert reached == set(case_of) and (on.occupancy == -1.0).any()  # every planted column, both levels
    levels = np.unique(np.round(on.voxels["height"][on.occupancy == 1.0], 3))
    assert len(levels) == (2 if two_level else 17), levels
    assert_normals(on, want, what)
    gm.close()


def test_map_without_the_covariance_layer(gpu):
    map_, gm, _ = planted_map(2, layers=("occupancy", "mean"), cls=GpuMap)
    p = planted_params(2)
    for mode in (HeightmapMode.kPlanar, HeightmapMode.kSimpleFill):
        off, on = build(gm, p, False, mode), build(gm, p, True, mode)
        assert_only_normals_differ(on, off, "no covariance layer")
        assert on.voxels.tobytes() == off.voxels.tobytes() and (on.occupancy == 1.0).sum() > 300
    gm.close()


def test_ray_integrated_ndt_scene(gpu):
    """A map the NDT mapper built from rays: the voxel mean is in use, the covariances are the mapper's own."""
    map_ = OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean", "covariance"))
    gm = GpuNdtMap(map_)
    rays = two_level_scene()
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    p = R.Params(0.1, 0.0, virtual_surface=True, cull_min=(-1.05, -1.0, 0.0), cull_max=(1.55, 1.33, 0.0))
    off, on = build(gm, p, False), build(gm, p, True)
    assert_only_normals_differ(on, off, "rays")
    e = on.extents
    dims = map_.region_voxel_dimensions
    ext = ([int(e.min_region[c]) * dims[c] + int(e.min_local[c]) for c in range(3)],
           [int(e.max_region[c]) * dims[c] + int(e.max_local[c]) for c in range(3)])
    want, occupied = N.expected_normals(source(map_), p, ext, int(e.na), on.source_column)
    assert occupied > 200
    lengths = np.linalg.norm(want[on.occupancy == 1.0].astype(np.float64), axis=1)
    assert np.abs(lengths - 1.0).max() < 1e-6 and (want[on.occupancy == 1.0][:, 2] >= 0).all()
    assert len(np.unique(want[on.occupancy == 1.0], axis=0)) > 50  # the mapper's covariances, not one planted value
    assert_normals(on, want, "rays")
    gm.close()


def test_spill_to_host_same_normals(gpu):
    """Ground voxels of regions in the host store give the same normals from their pinned records, and building the
    heightmap leaves the cache counters alone."""
    chunks, _ = planted_chunks(2)
    resident_map, resident, _ = planted_map(2)
    map_ = OccupancyMap(0.1, DIM, layers=("occupancy", "mean", "covariance"))
    gm = GpuNdtMap(map_, region_capacity=8)
    gm.setMemoryLimit(8 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    regions = sorted(chunks)
    assert len(regions) > 8
    for base in range(0, len(regions), 6):  # six regions a call: later calls evict the regions of earlier ones
        key_regions, key_locals, occupancy, covariance = [], [], [], []
        for region in regions[base:base + 6]:
            for vi in np.flatnonzero(chunks[region]["occupancy"] != INF):
                key_regions.append(region)
                key_locals.append((vi % 16, (vi // 16) % 16, vi // 256))
                occupancy.append(chunks[region]["occupancy"][vi])
                covariance.append(chunks[region]["covariance"][6 * vi:6 * vi + 6])
        keys = (np.array(key_regions, dtype=np.int16), np.array(key_locals, dtype=np.uint8))
        assert gm.writeVoxels(keys, "occupancy", np.array(occupancy, dtype=np.float32)) == len(occupancy)
        assert gm.writeVoxels(keys, "covariance", np.array(covariance, dtype=np.float32)) == len(covariance)
    before = gm.cacheStats()
    assert before["regions_spilled"] > 0 and len(gm.regionKeys()) == len(regions)
    p = planted_params(2)
    for mode in (HeightmapMode.kPlanar, HeightmapMode.kSimpleFill):
        want, got = build(resident, p, True, mode), build(gm, p, True, mode)
        assert normals_of(want.voxels)[want.occupancy == 1.0].any()
        assert got.voxels.tobytes() == want.voxels.tobytes() and got.occupancy.tobytes() == want.occupancy.tobytes()
    assert gm.cacheStats() == before
    resident.close()
    gm.close()
