"""CPU: tests/heightmap_fill_ref.py -- the restatement the device flood fill is held to -- pinned to the reference's own
known answers on its multi-level scene, to the generation-wise replay on every case of tests/heightmap_fill_cases.py,
and to hand-derived visit logs for every quirk rules F2-F6 of include/ohmhip.h name.

Geometry of the hand-made maps: 1 m voxels, 4 x 4 x 4 regions, origin 0.  Voxel g spans [g - 2, g - 1); the cull box
opens columns from global x = y = 2 and z voxels 0 .. 3 (.. 4), so a height offset h IS the global z voxel.  Cell (ia,
ib) is column (2 + ia, 2 + ib).  Neighbour offers go out row -1 .. 1 on b (outer), column -1 .. 1 on a (inner)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
import heightmap_fill_ref as F  # noqa: E402
from heightmap_fill_cases import HIT, Scene, fill_cases, multi_level_scene  # noqa: E402


# -- the reference's known answers -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def multi_level():
    scene, surface, virtual, seam = multi_level_scene()  # the defaults: 6.0 / 2.0, platform at 1.5, occlusion
    # testHeightmapVirtualSurface (HeightmapTests.cpp:1200-1301): clearance 0, setCeiling(floor = 0) then setCeiling(2.0)
    # -- the floor stays 0 --, virtual surfaces, the heightmap's origin the map's
    p = R.Params(0.1, 0.0, reference_pos=(0.0, 0.0, 1.1 * 1.5), ceiling=2.0, virtual_surface=True)
    return scene, scene.source(), p, surface, virtual, seam


def missed(res, scene, src, p, surface, virtual, seam):
    """The validation of :1246-1300: (surface voxels the heightmap missed, seams apart; virtual ones missed)."""
    surface, virtual = set(surface), set(virtual)
    hm, dims, first, _, _ = R.heightmap_geometry(src, p, (res.min_ext, res.max_ext))
    for cb in range(res.mb):
        for ca in range(res.ma):
            voxel_type, pos, _ = R.voxel_info(res, src, p, (ca, cb))
            if voxel_type == R.HM_SURFACE:
                key = tuple(scene.key(pos))
                assert scene.is_occupied(key)
                surface.discard(key)
            elif voxel_type == R.HM_VIRTUAL:
                key = tuple(scene.key(pos))
                assert scene.is_free(key)
                virtual.discard(key)
    return len(surface - seam), len(virtual)


def test_scene_is_the_reference_scene(multi_level):
    """Heightmap.VirtualSurfacePlanar (:1304-1311) on the restated scene with the existing planar restatement."""
    scene, src, p, surface, virtual, seam = multi_level
    res = R.build_heightmap(src, p)
    assert (res.na, res.nb) == (161, 161)
    assert missed(res, scene, src, p, surface, virtual, seam) == (2215, 0)


def test_virtual_surface_fill(multi_level):
    """Heightmap.VirtualSurfaceFill (:1313-1320): the same 2215 voxels below the platform, no virtual voxel missed.  The
    scene exercises every quirk: accepted revisits, pops that raise a cell, several keys of a cell in a generation."""
    scene, src, p, surface, virtual, seam = multi_level
    res = F.build_fill(src, p)
    assert missed(res, scene, src, p, surface, virtual, seam) == (2215, 0)
    assert res.revisits > 0 and res.raising_pops > 0 and res.max_cell_multiplicity >= 2
    assert res.generations > 1 and sum(res.generation_sizes) == res.visits
    assert res.visits > res.na * res.nb  # cells are visited again


# -- FIFO against the generation-wise replay --------------------------------------------------------------------------------

def assert_same_result(a, b):
    assert np.array_equal(a.log, b.log)
    assert np.array_equal(a.occupancy.view(np.uint32), b.occupancy.view(np.uint32))
    assert a.voxels.tobytes() == b.voxels.tobytes()
    assert (a.mean is None) == (b.mean is None) and (a.mean is None or np.array_equal(a.mean, b.mean))
    assert np.array_equal(a.source_visit, b.source_visit)
    for name in ("visits", "populated", "cells", "revisits", "generations", "largest_generation", "raising_pops",
                 "max_cell_multiplicity", "generation_sizes"):
        assert getattr(a, name) == getattr(b, name), name


@pytest.mark.parametrize("case", list(fill_cases()), ids=lambda c: c[0])
def test_generations_equal_the_fifo(case):
    _, scene, p = case
    fifo = F.build_fill(scene.source(), p)
    assert fifo is not None and fifo.visits >= fifo.na * fifo.nb  # every cell of these scenes is reached
    assert_same_result(fifo, F.build_fill_generations(scene.source(), p))


# -- hand-derived logs ---------------------------------------------------------------------------------------------------

def hand_scene(columns):
    """columns: {(ia, ib): occupied z voxels}."""
    s = Scene(1.0, (4, 4, 4))
    s.region((0, 0, 0))
    for (ia, ib), zs in columns.items():
        for z in zs:
            s.put((2 + ia, 2 + ib, z), HIT)
    return s


def hand_params(na, nb, seed, top=3):
    """Cull to na x nb columns and z voxels 0 .. top; seed = (ia, ib, h) or a point."""
    ref = (seed[0] + 0.5, seed[1] + 0.5, seed[2] - 1.5) if all(isinstance(v, int) for v in seed) else seed
    return R.Params(1.0, 0.0, reference_pos=ref, cull_min=(0.25, 0.25, -1.5),
                    cull_max=(na - 1 + 0.75, nb - 1 + 0.75, top - 1.5))


def both(scene, p):
    fifo = F.build_fill(scene.source(), p)
    assert_same_result(fifo, F.build_fill_generations(scene.source(), p))
    return fifo


def test_seed_cell_is_added_again_by_a_neighbour():
    """Two columns with the floor at 1.  The seed (0, 0, 1) is visited without being popped, so its cell stays
    unvisited and column 1's offer of 1 is accepted; the second visit's offer back finds 1 < 1 false."""
    res = both(hand_scene({(0, 0): [1], (1, 0): [1]}), hand_params(2, 1, (0, 0, 1)))
    assert res.log.tolist() == [[0, 0, 1], [1, 0, 1], [0, 0, 1]]
    assert (res.visits, res.populated, res.cells, res.revisits) == (3, 3, 2, 0)
    assert res.source_visit[0, :2].tolist() == [2, 1]
    assert res.generation_sizes == [1, 1, 1]


def test_lower_offer_is_accepted():
    """A row of three: floors at 3, 1, 1, seed (0, 0, 3).  Visit 0 offers 3 to cell 1.  Visit 1 (1, 0, 3) finds the floor
    at 1 and offers 1 to cells 0 (unvisited seed cell) and 2.  Visit 2 (0, 0, 1) climbs to the floor at 3 (only
    candidate above) and offers 3 to cell 1, which holds 3: refused.  Visit 3 (2, 0, 1) offers 1 to cell 1: 1 < 3,
    accepted -- the revisit.  Visit 4 (1, 0, 1) offers 1 to cells that hold 1."""
    res = both(hand_scene({(0, 0): [3], (1, 0): [1], (2, 0): [1]}), hand_params(3, 1, (0, 0, 3), top=4))
    assert res.log.tolist() == [[0, 0, 3], [1, 0, 3], [0, 0, 1], [2, 0, 1], [1, 0, 1]]
    assert (res.revisits, res.raising_pops, res.populated, res.cells) == (1, 0, 5, 3)
    assert res.source_visit[0, :3].tolist() == [2, 4, 3]
    assert res.voxels[0, 0]["height"] == np.float32(1.5)  # voxel 3's centre


def test_pop_raises_a_cell_and_a_later_offer_gets_in():
    """2 x 2: floors A (0, 0) 1, B (1, 0) 1, C (0, 1) 2, D (1, 1) 2; seed C at 2.
    v0 C2: hg 2, offers A, B, D accepted at 2.                         queue A2 B2 D2
    v1 A2: floor below, hg 1; B 1 < 2, C unvisited, D 1 < 2 accepted.  queue B2 D2 B1 C1 D1   grid B 1, C 1, D 1
    v2 B2: the pop RAISES B to 2; hg 1; A 1 < 2 accepted.              queue D2 B1 C1 D1 A1   grid A 1
    v3 D2: the pop RAISES D to 2; hg 2; nothing accepted.
    v4 B1: hg 1; D holds 2 again, so 1 < 2: accepted a second time.    queue C1 D1 A1 D1
    v5 C1, v6 D1, v7 A1, v8 D1: nothing accepted (C and D climb to their floor at 2 and offer 2).
    Had the pops not raised the cells, v4's offer to D would have met 1 and the walk would have 8 visits."""
    res = both(hand_scene({(0, 0): [1], (1, 0): [1], (0, 1): [2], (1, 1): [2]}), hand_params(2, 2, (0, 1, 2)))
    assert res.log.tolist() == [[0, 1, 2], [0, 0, 2], [1, 0, 2], [1, 1, 2], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0, 0, 1],
                                [1, 1, 1]]
    assert (res.visits, res.revisits, res.raising_pops) == (9, 4, 2)
    assert res.generation_sizes == [1, 3, 4, 1]  # C2 | A2 B2 D2 | B1 C1 D1 A1 | D1
    assert res.source_visit[:2, :2].tolist() == [[7, 4], [5, 8]]


def test_seed_outside_the_extents():
    """The reference position far off on all three axes is clamped to cell (1, 0) and the top voxel 3."""
    res = both(hand_scene({(0, 0): [1], (1, 0): [1]}), hand_params(2, 1, (10.5, -7.0, 9.0)))
    assert res.log.tolist() == [[1, 0, 3], [0, 0, 1], [1, 0, 1]]
    assert (res.populated, res.cells) == (3, 2)


def test_seed_over_a_column_without_a_candidate():
    """Column 0 is unobserved: visits there write nothing and offer the WALK key's height.  v0 (0, 0, 2) offers 2;
    v1 (1, 0, 2) finds the floor at 1 and offers 1 to the unvisited seed cell; v2 (0, 0, 1) offers 1 to cell 1, which
    its pop set to 2: accepted; v3 (1, 0, 1) offers 1 to a cell that holds 1."""
    res = both(hand_scene({(1, 0): [1]}), hand_params(2, 1, (0, 0, 2)))
    assert res.log.tolist() == [[0, 0, 2], [1, 0, 2], [0, 0, 1], [1, 0, 1]]
    assert (res.populated, res.cells, res.revisits) == (2, 1, 1)
    assert res.source_visit[0, :2].tolist() == [F.NO_VISIT, 3] and res.occupancy[0, 0] == np.inf


def test_first_visit_without_bias_above_chooses_differently():
    """Column 0 holds voxels 1 and 3 around the seed height 2: offset_below 2, offset_above 0.  Visit 0 has no
    kBiasAbove: 2 <= 0 fails, 2 + 0 >= 1 holds, the voxel BELOW is taken and hg = 1.  Column 1 (floor at 2) sends the
    walk back at height 2, and visit 2 of the same key, now with kBiasAbove, takes the closer voxel ABOVE: the cell ends
    with voxel 3's height, written by visit 2."""
    res = both(hand_scene({(0, 0): [1, 3], (1, 0): [2]}), hand_params(2, 1, (0, 0, 2), top=4))
    assert res.log.tolist() == [[0, 0, 2], [1, 0, 1], [0, 0, 2]]
    assert res.source_visit[0, :2].tolist() == [2, 1]
    assert res.voxels[0, 0]["height"] == np.float32(1.5)
    # visit 0's own choice, seen when nothing comes back: a single column
    alone = both(hand_scene({(0, 0): [1, 3]}), hand_params(1, 1, (0, 0, 2), top=4))
    assert alone.log.tolist() == [[0, 0, 2]] and alone.voxels[0, 0]["height"] == np.float32(-0.5)


def test_empty_map_and_null_reference_build_nothing():
    assert F.build_fill(Scene(1.0, (4, 4, 4)).source(), R.Params(1.0, 0.0)) is None
    assert F.build_fill_generations(Scene(1.0, (4, 4, 4)).source(), R.Params(1.0, 0.0)) is None
