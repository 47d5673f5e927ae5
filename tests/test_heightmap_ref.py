"""CPU: tests/heightmap_ref.py -- the restatement the device heightmap is held to -- pinned to the reference's own
known answers and to hand-derived cases for every quirk the rule list of include/ohmhip.h ("HEIGHTMAP") names.

Geometry of the hand-made maps: 1 m voxels, 4 x 4 x 4 regions, origin 0.  Region r covers global voxels 4r .. 4r + 3;
voxel g spans [g - 2, g - 1) and its centre is g - 1.5.  Without a mean layer and with the heightmap's origin at 0 the
height field of a cell is the ground voxel's centre on the up axis."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
from heightmap_cases import SS_DIM, SS_ORIGIN, surface_selection_cases  # noqa: E402
from oracle.oracle import OracleMap, lib as _olib  # noqa: E402

HIT = np.float32(_olib.oracle_probability_to_value(0.9))
MISS = np.float32(_olib.oracle_probability_to_value(0.45))
DIM = (4, 4, 4)


class Grid:
    """Occupancy (and mean) by global voxel coordinate on the 4^3 geometry."""

    def __init__(self, regions=(), mean=False, dim=DIM):
        self.dim = dim
        self.chunks = {}
        self.with_mean = mean
        for r in regions:
            self.region(r)

    def region(self, r):
        n = self.dim[0] * self.dim[1] * self.dim[2]
        c = self.chunks.setdefault(tuple(r), {"occupancy": np.full(n, np.inf, dtype=np.float32)})
        if self.with_mean and "mean" not in c:
            c["mean"] = np.zeros(2 * n, dtype=np.uint32)
        return c

    def put(self, g, value, mean=None):
        r = tuple(g[a] // self.dim[a] for a in range(3))
        l = tuple(g[a] % self.dim[a] for a in range(3))
        vi = l[0] + l[1] * self.dim[0] + l[2] * self.dim[0] * self.dim[1]
        c = self.region(r)
        c["occupancy"][vi] = value
        if mean is not None:
            c["mean"][2 * vi], c["mean"][2 * vi + 1] = mean

    def source(self, resolution=1.0):
        return R.Source(resolution, self.dim, self.chunks, 0.0, has_mean=self.with_mean)


def column_params(z_lo, z_hi, ref_z, **kw):
    """Cull to the single column of global voxel x = y = 2 (x, y in [0, 1)) and to z in [z_lo, z_hi]."""
    return R.Params(1.0, kw.pop("min_clearance", 0.0), reference_pos=(0.5, 0.5, ref_z), cull_min=(0.25, 0.25, z_lo),
                    cull_max=(0.75, 0.75, z_hi), **kw)


def single_cell(res):
    """(occupancy, ground voxel g on z, clearance, flags) of a one-column build."""
    # (the dense grid's upper corner, centre + resolution / 2, is the lower edge of the NEXT cell: one cell more)
    assert res is not None and (res.na, res.nb, res.ma, res.mb) == (1, 1, 2, 2)
    assert (res.occupancy.reshape(-1)[1:] == np.inf).all()
    v = res.voxels[0, 0]
    occ = float(res.occupancy[0, 0])
    return occ, (float(v["height"]) + 1.5 if occ != np.inf else None), float(v["clearance"]), int(v["flags"])


# -- the reference's known answers ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(surface_selection_cases(HIT, MISS)), ids=lambda c: c[0])
def test_surface_selection(case):
    """Heightmap.SurfaceSelection (tests/ohmtestheightmap/HeightmapTests.cpp:686-878): expected voxel type and exact
    pos.z of the voxel at the heightmap's voxelKey((0, 0, 0)), all 39 cases."""
    _, chunks, p, expected_type, expected_height = case
    src = R.Source(1.0, SS_DIM, chunks, 0.0, SS_ORIGIN)
    res = R.build_heightmap(src, p)
    if res is None:
        voxel_type, pos = R.HM_UNKNOWN, None
    else:
        hm, dims, first, _, _ = R.heightmap_geometry(src, p, (res.min_ext, res.max_ext))
        key = hm.voxel_key((0.0, 0.0, 0.0))
        cell = (key[0][0] * dims[0] + key[1][0] - first[0], key[0][1] * dims[1] + key[1][1] - first[1])
        voxel_type, pos, _ = R.voxel_info(res, src, p, cell)
    assert voxel_type == expected_type
    if expected_type != R.HM_UNKNOWN:
        assert pos[2] == expected_height


def test_surface_selection_has_39_cases():
    assert len(list(surface_selection_cases(HIT, MISS))) == 39


def two_level_grid():
    """A floor plane at z voxel 1 over 8 x 8 columns and a platform at z voxel 5 above the columns x in 2 .. 5."""
    grid = Grid([(rx, ry, rz) for rx in (0, 1) for ry in (0, 1) for rz in (0, 1)])
    for x in range(8):
        for y in range(8):
            grid.put((x, y, 1), HIT)
            grid.put((x, y, 2), MISS)
            if 2 <= x <= 5:
                grid.put((x, y, 5), HIT)
                grid.put((x, y, 6), MISS)
    return grid


def test_clearance_property():
    """Heightmap.Clearance (HeightmapTests.cpp:880-947) on a map written directly: with min_clearance 0 every cell is
    the floor and the cells under the platform report the platform's height as clearance; with half the platform height
    the cells equal the unconstrained ones wherever those had enough clearance (:936-945)."""
    src = two_level_grid().source()
    ref_pos = (0.5, 0.5, -0.5)  # in the floor voxel
    ref = R.build_heightmap(src, R.Params(1.0, 0.0, reference_pos=ref_pos))
    platform_height = 4.0  # voxel 5 above voxel 1
    assert (ref.na, ref.nb) == (9, 9)  # 8 columns of data + the one beyond (rule 1)
    for x in range(8):
        for y in range(8):
            assert ref.occupancy[y, x] == 1.0
            assert ref.voxels[y, x]["height"] == np.float32(-0.5)
            assert ref.voxels[y, x]["clearance"] == (platform_height if 2 <= x <= 5 else 0.0)
            assert ref.voxels[y, x]["flags"] == R.HVF_OBSERVED_ABOVE
    assert (ref.occupancy[8, :] == np.inf).all() and (ref.occupancy[:, 8] == np.inf).all()
    constraint = 0.5 * platform_height
    con = R.build_heightmap(src, R.Params(1.0, constraint, reference_pos=ref_pos))
    checked = 0
    for x in range(8):
        for y in range(8):
            if con.voxels[y, x]["clearance"] > 0:
                assert con.voxels[y, x]["clearance"] >= constraint
            if ref.voxels[y, x]["clearance"] >= constraint:
                assert con.voxels[y, x]["height"] == ref.voxels[y, x]["height"]
                checked += 1
    assert checked == 4 * 8
    # a constraint the platform violates: those cells move up to the platform
    high = R.build_heightmap(src, R.Params(1.0, platform_height + 1.0, reference_pos=ref_pos))
    for x in range(8):
        for y in range(8):
            assert high.voxels[y, x]["height"] == np.float32(3.5 if 2 <= x <= 5 else -0.5)
            assert high.voxels[y, x]["clearance"] == 0.0


# -- rule 3: the missing-region jump ---------------------------------------------------------------------------------------

def gap_grid():
    """z regions 0 and 2 exist, region 1 (voxels 4 .. 7) does not."""
    return Grid([(0, 0, 0), (0, 0, 2)])


def test_jump_up_to_an_occupied_voxel():
    """Seed 1.  Up: 2, 3 (unobserved), 4 (no region: jump of 4, i += 3), 8, 9 occupied at i = 7, offset 8."""
    grid = gap_grid()
    grid.put((2, 2, 9), HIT)
    src = grid.source()
    assert R._search(src, [2, 2, 1], [2, 2, 11], 2, 0, True, 0) == ([2, 2, 9], 8, False)
    assert single_cell(R.build_heightmap(src, column_params(-1.5, 9.5, -0.5))) == (1.0, 9.0, 0.0, 0)


def test_jump_up_with_a_free_voxel_on_the_far_side():
    """The voxel visited inside the missing region (4) is the `last unobserved` when the walk lands on the free voxel
    8: the virtual candidate is key 4 -- a voxel of a region that does not exist -- and findGround, walking up from it
    through kNull voxels, makes 8 the virtual surface."""
    grid = gap_grid()
    grid.put((2, 2, 8), MISS)
    src = grid.source()
    key, offset, is_virtual = R._search(src, [2, 2, 1], [2, 2, 11], 2, 0, True, R.F_VIRTUAL)
    assert (key, is_virtual) == ([2, 2, 4], True) and offset >= 0
    assert single_cell(R.build_heightmap(src, column_params(-1.5, 9.5, -0.5, virtual_surface=True))) == \
        (-1.0, 8.0, 0.0, 0)
    # virtual surfaces off: nothing
    assert single_cell(R.build_heightmap(src, column_params(-1.5, 9.5, -0.5)))[0] == np.inf


def test_jump_up_without_a_free_voxel_on_the_far_side():
    src = gap_grid().source()
    res = R.build_heightmap(src, column_params(-1.5, 9.5, -0.5, virtual_surface=True))
    assert single_cell(res)[0] == np.inf and res.populated == 0


def test_jump_down_and_the_range_asymmetry():
    """Seed 9, limit 0: vertical_range = |0 - 9 + 1| = 8, + 1 for the downward search = 9 iterations: 9, 8, 7 (no
    region, local 3: jump of -4, i += 3), 3, 2, 1 at i = 0, 1, 2, 6, 7, 8.  Voxel 0 -- min_ext_key itself -- is never
    visited."""
    for g, found in ((2, True), (1, True), (0, False)):
        grid = gap_grid()
        grid.put((2, 2, g), HIT)
        src = grid.source()
        key, offset, _ = R._search(src, [2, 2, 9], [2, 2, 0], 2, 0, False, 0)
        assert (key is not None) == found
        if found:
            assert key == [2, 2, g] and offset == 10 - g  # i + 1 with i = 9 - g
        cell = single_cell(R.build_heightmap(src, column_params(-1.5, 9.5, 7.5)))
        assert cell == ((1.0, float(g), 0.0, 0) if found else (np.inf, None, 0.0, 0))


def test_downward_search_returns_the_unobserved_voxel_below_the_free_one():
    grid = Grid([(0, 0, 0), (0, 0, 1)])
    grid.put((2, 2, 3), MISS)
    grid.put((2, 2, 4), MISS)
    src = grid.source()
    key, offset, is_virtual = R._search(src, [2, 2, 6], [2, 2, 0], 2, 0, False, R.F_VIRTUAL)
    assert (key, is_virtual) == ([2, 2, 2], True)
    # ... and findGround reports the free voxel above it
    assert single_cell(R.build_heightmap(src, column_params(-1.5, 5.5, 4.5, virtual_surface=True))) == \
        (-1.0, 3.0, 0.0, R.HVF_OBSERVED_ABOVE)


# -- rule 3: offsets and the selection ladder ------------------------------------------------------------------------------

def test_offset_series_and_the_tie_at_distance_one():
    """Offsets: up 0, 2, 3, ...; down 1, 2, 3, ... -- the downward search starts ON the seed, the upward one above it.
    Occupied voxels at distance 1 on both sides (4 and 6 around the seed 5): offset_below = 2, offset_above = 0."""
    grid = Grid([(0, 0, 0), (0, 0, 1), (0, 0, 2)])
    grid.put((2, 2, 4), HIT)
    grid.put((2, 2, 6), HIT)
    src = grid.source()
    seed, lo, hi = [2, 2, 5], [2, 2, 0], [2, 2, 11]
    assert R._search(src, seed, lo, 2, 0, False, 0) == ([2, 2, 4], 2, False)
    assert R._search(src, seed, hi, 2, 0, True, 0) == ([2, 2, 6], 0, False)
    flags = R.F_IGNORE_VIRTUAL_ABOVE
    # clearance 0: permissive count max(1, 0 - 1) = 1; 2 <= 0 fails, 2 + 0 >= 1 holds: below
    assert R.supporting_voxel(src, seed, 2, lo, hi, 0, 0, 1, flags) == [2, 2, 4]
    # clearance 4 m: permissive count 3; 2 + 0 >= 3 fails: above
    assert R.supporting_voxel(src, seed, 2, lo, hi, 0, 0, 3, flags) == [2, 2, 6]
    # the seed itself occupied: offset_below = 1 against offset_above = 0
    grid.put((2, 2, 5), HIT)
    assert R._search(src, seed, lo, 2, 0, False, 0) == ([2, 2, 5], 1, False)
    assert R.supporting_voxel(src, seed, 2, lo, hi, 0, 0, 1, flags) == [2, 2, 5]
    assert R.supporting_voxel(src, seed, 2, lo, hi, 0, 0, 2, flags) == [2, 2, 6]
    # the whole build, clearance 0: ground 5, the occupied voxel 6 ends the scan at clearance 1 -- and, being an
    # observed voxel, sets observed_above before the clearance branch is taken (:463)
    assert single_cell(R.build_heightmap(src, column_params(-1.5, 9.5, 3.5))) == (1.0, 5.0, 1.0, R.HVF_OBSERVED_ABOVE)


def test_floor_and_ceiling_limits():
    """Seed 6.  floor 2 m: 2 + 1 iterations 6, 5, 4; floor 4 m: 6 .. 2.  ceiling 2 m: 7, 8; ceiling 3 m: 7, 8, 9."""
    regions = [(0, 0, 0), (0, 0, 1), (0, 0, 2)]
    below = Grid(regions)
    below.put((2, 2, 2), HIT)
    assert single_cell(R.build_heightmap(below.source(), column_params(-1.5, 9.5, 4.5, floor=2.0)))[0] == np.inf
    assert single_cell(R.build_heightmap(below.source(), column_params(-1.5, 9.5, 4.5, floor=4.0)))[:2] == (1.0, 2.0)
    assert single_cell(R.build_heightmap(below.source(), column_params(-1.5, 9.5, 4.5)))[:2] == (1.0, 2.0)
    above = Grid(regions)
    above.put((2, 2, 9), HIT)
    assert single_cell(R.build_heightmap(above.source(), column_params(-1.5, 9.5, 4.5, ceiling=2.0)))[0] == np.inf
    assert single_cell(R.build_heightmap(above.source(), column_params(-1.5, 9.5, 4.5, ceiling=3.0)))[:2] == (1.0, 9.0)


# -- rules 1, 2: extents, axes ---------------------------------------------------------------------------------------------

def test_walked_range_is_one_voxel_beyond_the_data():
    """One region: extents -2 .. +2; voxelKey(+2) is voxel 0 of the NEXT region."""
    grid = Grid([(0, 0, 0)])
    grid.put((1, 3, 1), HIT)
    res = R.build_heightmap(grid.source(), R.Params(1.0, 0.0))
    assert (res.min_ext, res.max_ext) == ([0, 0, 0], [4, 4, 4])
    assert (res.na, res.nb, res.ma, res.mb) == (5, 5, 6, 6)  # (the grid's upper corner is a point of the next cell)
    assert res.populated == 1 and res.occupancy[3, 1] == 1.0 and res.source_column[3, 1] == 3 * 5 + 1


def test_empty_map_builds_nothing():
    assert R.build_heightmap(Grid().source(), R.Params(1.0, 0.0)) is None


@pytest.mark.parametrize("up_axis", [-3, -2, -1, 0, 1, 2])
def test_up_axes(up_axis):
    """One occupied voxel with a free one above it -- `above` along the up axis, so below it in key space for a
    negative axis -- at a position that is different on every axis."""
    a, b, up = R.axis_indices(up_axis)
    assert (a, b, up) == {0: (1, 2, 0), 1: (0, 2, 1), 2: (0, 1, 2)}[up]
    sign = 1 if up_axis >= 0 else -1
    grid = Grid([(rx, ry, rz) for rx in (-1, 0, 1) for ry in (-1, 0, 1) for rz in (-1, 0, 1)])
    g = [1, 2, 3]
    free = list(g)
    free[up] += sign
    grid.put(g, HIT)
    grid.put(free, MISS)
    res = R.build_heightmap(grid.source(), R.Params(1.0, 0.0, up_axis=up_axis))
    assert res.min_ext == [-4, -4, -4] and res.max_ext == [8, 8, 8]  # regions -1 .. 1 and the voxel beyond
    assert res.populated == 1
    ca, cb = g[a] + 4, g[b] + 4
    assert res.occupancy[cb, ca] == 1.0 and res.source_column[cb, ca] == cb * res.na + ca
    v = res.voxels[cb, ca]
    assert v["height"] == np.float32(sign * (g[up] - 1.5))
    assert v["flags"] == R.HVF_OBSERVED_ABOVE and v["clearance"] == 0.0


# -- rules 5, 6: the heightmap's own geometry ------------------------------------------------------------------------------

def mean_pattern(ix, iy, iz):
    return ix | (iy << 10) | (iz << 20) | (1 << 31)


def mean_cell(ix):
    """The cell (on a) of one occupied voxel (global 2, 2, 1: centre 0.5 on x) whose mean has sub-voxel index ix on x,
    for a heightmap of the source's resolution with its origin shifted by half a cell (cell edges at k + 0.5)."""
    grid = Grid([(0, 0, 0)], mean=True)
    grid.put((2, 2, 1), HIT, mean=(mean_pattern(ix, 511, 511), 3))
    p = R.Params(1.0, 0.0, origin=(0.5, 0.5, 0.0))
    res = R.build_heightmap(grid.source(), p)
    assert res.populated == 1
    (cb,), (ca,) = np.nonzero(res.occupancy == 1.0)
    assert res.voxels[cb, ca]["contributing_samples"] == 3 and res.mean[cb, ca, 1] == 1
    return ca, res


def test_half_cell_origin_splits_a_source_voxel():
    """Means in the two halves of one source voxel land in neighbouring cells; the pattern 1023 (the +1/2 voxel edge)
    goes wherever the heightmap's voxelKey puts its position."""
    lower, _ = mean_cell(256)   # x = 0.5 - 0.2497..: in [-0.5, 0.5)
    upper, _ = mean_cell(767)   # x = 0.5 + 0.2497..: in [0.5, 1.5)
    assert upper == lower + 1
    edge, res = mean_cell(1023)
    x = 0.5 + R.sub_voxel_to_local(mean_pattern(1023, 511, 511), 1.0)[0]
    hm = OracleMap(1.0, (128, 128, 1))
    hm.set_origin((0.5, 0.5, 0.0))
    key = hm.voxel_key((x, 0.5, 0.0))
    assert edge == key[0][0] * 128 + key[1][0] - res.first_cell[0]
    assert edge in (upper, upper + 1)


def test_collisions_the_larger_walk_index_stands():
    """A heightmap of twice the source's resolution with an offset origin: up to four source columns share a cell."""
    grid = Grid([(0, 0, 0)])
    for x in range(4):
        for y in range(4):
            grid.put((x, y, 1), HIT)
    p = R.Params(2.0, 0.0, origin=(0.5, -0.5, 0.0), region_size=16)
    res = R.build_heightmap(grid.source(), p)
    cells = int((res.source_column != R.NO_COLUMN).sum())
    assert res.populated == 16 and res.populated > cells
    # independently: every column's cell from the heightmap's voxelKey of its voxel centre; the largest index stands
    hm = OracleMap(2.0, (16, 16, 1))
    hm.set_origin(p.origin)
    expected = {}
    for y in range(4):
        for x in range(4):
            key = hm.voxel_key((x - 1.5, y - 1.5, 0.0))
            cell = (key[0][1] * 16 + key[1][1] - res.first_cell[1], key[0][0] * 16 + key[1][0] - res.first_cell[0])
            expected[cell] = max(expected.get(cell, -1), y * res.na + x)
    assert len(expected) == cells
    for (cb, ca), column in expected.items():
        assert res.source_column[cb, ca] == column and res.occupancy[cb, ca] == 1.0
