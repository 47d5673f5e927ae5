"""CPU: tests/heightmap_layered_ref.py -- the restatement the device layered heightmaps are held to -- pinned to the
reference's own tests on its multi-level scene (Heightmap.LayeredAbove / LayeredBelow / LayeredExternal / LayeredBase /
VirtualSurfaceSimpleLayered, tests/ohmtestheightmap/HeightmapTests.cpp:956-1330), to the generation-wise replay on every
case of tests/heightmap_layered_cases.py -- each case first showing the quirk it exists for --, and to hand-derived
walks.

Geometry of the hand-derived maps: that of tests/test_heightmap_fill_ref.py (1 m voxels, 4^3 regions, voxel g spans
[g - 2, g - 1), cell (ia, ib) is column (2 + ia, 2 + ib), a height offset h is the global z voxel); the heightmap's slot
k is centred on height k."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heightmap_ref as R  # noqa: E402
import heightmap_layered_ref as LR  # noqa: E402
import heightmap_layered_cases as LC  # noqa: E402
from heightmap_fill_cases import multi_level_scene  # noqa: E402
from test_heightmap_fill_ref import hand_params, hand_scene  # noqa: E402


def assert_same_result(a, b):
    assert np.array_equal(a.log, b.log)
    assert np.array_equal(a.occupancy.view(np.uint32), b.occupancy.view(np.uint32))
    assert a.voxels.tobytes() == b.voxels.tobytes()
    assert (a.mean is None) == (b.mean is None) and (a.mean is None or np.array_equal(a.mean, b.mean))
    assert np.array_equal(a.source_visit, b.source_visit)
    assert np.array_equal(a.layer_count, b.layer_count)
    assert LR.stats_of(a) == LR.stats_of(b)
    assert a.generation_sizes == b.generation_sizes and a.quirks == b.quirks and a.slots == b.slots


# -- the deque against the generation-wise replay ------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(LC.layered_cases()), ids=lambda c: c[0])
def test_generations_equal_the_deque(case):
    name, scene, p, mode, threshold, quirks = case
    fifo = LR.build_layered(scene.source(), p, mode, threshold)
    assert fifo is not None and fifo.visits >= fifo.na * fifo.nb  # every column of these scenes is reached
    counts = LC.quirk_counts(fifo)
    for quirk in quirks:
        assert counts[quirk] > 0, quirk  # the case shows what it is about
    assert sum(fifo.generation_sizes) == fifo.visits and fifo.voxels_kept == fifo.populated - fifo.filtered
    assert_same_result(fifo, LR.build_layered_generations(scene.source(), p, mode, threshold))


def test_hand_made_cases_cover_the_list():
    """Every quirk the hand-made columns exist for is named by some case."""
    named = set(sum((list(c[5]) for c in LC.hand_made_cases()), []))
    assert {"repeats", "too_close_real", "column_rule_refusals", "seed_column_again", "permuted_columns",
            "base_not_nearest", "base_by_distance", "base_ties", "filtered_single", "filtered_multi", "virtual_kept",
            "two_base_columns", "mean_in_upper_slot"} <= named
    assert {c[2].up_axis for c in LC.hand_made_cases()} == {-3, -2, -1, 0, 1, 2}


# -- the reference's own tests -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def multi_level():
    scene, surface, _, seam = multi_level_scene(virtual_surfaces=False)  # HeightmapParams' defaults (:39-54)
    return scene, scene.source(), surface, seam


def surface_keys(res, scene, src, p):
    """heightmapLayeredTest's conversion back (:1032-1047): the source key of every kSurface voxel, one entry per voxel."""
    hm, dims, first, _, _ = R.heightmap_geometry(src, p, (res.min_ext, res.max_ext))
    keys = []
    for slot, cb, ca in zip(*np.nonzero(res.occupancy == 1.0)):
        g = [first[0] + int(ca), first[1] + int(cb), int(slot)]
        centre = hm.voxel_centre([g[c] // dims[c] for c in range(3)], [g[c] % dims[c] for c in range(3)])
        pos = (centre[0], centre[1], centre[2] + float(res.voxels["height"][slot, cb, ca]))  # getHeightmapVoxelInfo
        keys.append(tuple(scene.key(pos)))
    return keys


SEEDS = {"above": (0.0, 0.0, 1.5), "below": (0.0, 0.0, 0.0), "external": None}
_BUILT = {}


def layered_test(multi_level, start, min_clearance=-1.0):
    scene, src, surface, seam = multi_level
    if (start, min_clearance) not in _BUILT:
        seed = SEEDS[start]
        if seed is None:  # calculateExtents' minimum key: the first voxel of the lowest region
            seed = tuple(scene.centre([min(r[c] for r in scene.chunks) * scene.dim[c] for c in range(3)]))
        p = R.Params(0.1, min_clearance, reference_pos=seed)
        _BUILT[(start, min_clearance)] = (p, LR.build_layered(src, p, LR.MODE_ORDERED, 0))
    return _BUILT[(start, min_clearance)]


@pytest.mark.parametrize("start", ["above", "below", "external"])
def test_layered_rebuilds_the_source_map(multi_level, start):
    """Heightmap.LayeredAbove / LayeredBelow / LayeredExternal (:1094-1106, :1174-1177): the heightmap's surface voxels
    turned back into a map give every non-seam voxel of the source its type, and as many surface voxels as the source
    has."""
    scene, src, surface, seam = multi_level
    p, res = layered_test(multi_level, start)
    keys = surface_keys(res, scene, src, p)
    rebuilt = set(keys)
    assert len(keys) > 0
    # the scene holds hits only, so a voxel is occupied or unobserved and the rebuilt map has the source's types exactly
    # when it holds the source's occupied voxels and no others, seam voxels apart (:1072-1076)
    occupied = set()
    strides = (1, scene.dim[0], scene.dim[0] * scene.dim[1])
    for region, chunk in scene.chunks.items():
        occupancy = np.asarray(chunk["occupancy"])
        assert not (occupancy < 0).any()
        for vi in np.nonzero(occupancy != np.inf)[0].tolist():
            occupied.add(tuple(region[c] * scene.dim[c] + (vi // strides[c]) % scene.dim[c] for c in range(3)))
    assert occupied == set(surface)  # populateMultiLevelMap's own record
    assert rebuilt - seam == occupied - seam
    reference_count = len(occupied - seam)
    assert reference_count > 0 and len(keys) == reference_count
    assert res.multi_layer_columns > 0 and res.layers == 2
    assert start != "above" or res.quirks["permuted_columns"] > 0  # from the platform its columns fill top first


@pytest.mark.parametrize("start", ["above", "below", "external"])
def test_clearance_zero_builds_what_minus_one_builds(multi_level, start):
    """The reference's Layered* tests pass min_clearance = -1 (:974).  The device refuses a negative clearance; 0 builds
    the same heightmap: rule 4's test clearance >= min_clearance holds for every second voxel found either way, and L5's
    too-close interval (0, min_clearance] is empty for both."""
    _, minus_one = layered_test(multi_level, start, -1.0)
    _, zero = layered_test(multi_level, start, 0.0)
    assert_same_result(minus_one, zero)
    assert minus_one.too_close == 0 and minus_one.repeats > 0


def test_layered_base(multi_level):
    """Heightmap.LayeredBase (:1109-1172): every occupied base-layer voxel of the layered heightmap built from under
    the platform lies, within 1e-3, where the planar heightmap with a clearance of 1.1 voxels has its voxel."""
    scene, src, surface, seam = multi_level
    p, res = layered_test(multi_level, "below")
    planar = R.build_heightmap(src, R.Params(0.1, 1.1 * 0.1, reference_pos=SEEDS["below"]))
    assert (planar.ma, planar.mb, planar.first_cell) == (res.ma, res.mb, res.first_cell)
    checked = 0
    for slot, cb, ca in zip(*np.nonzero((res.occupancy == 1.0) & (res.voxels["layer"] == LR.HVL_BASE))):
        layered_height = slot * 0.1 + float(res.voxels["height"][slot, cb, ca])  # both centres differ by the slot's rise
        planar_height = float(planar.voxels["height"][cb, ca])
        assert abs(layered_height - planar_height) < 1e-3, (slot, cb, ca)
        checked += 1
    assert checked == res.cells  # one base-layer voxel per column that holds any
    assert ((res.occupancy == 1.0) & (res.voxels["layer"] == LR.HVL_BASE)).sum(axis=0).max() == 1


def test_virtual_surface_simple_layered():
    """Heightmap.VirtualSurfaceSimpleLayered (:1324-1330, testHeightmapVirtualSurface :1200-1301): kLayeredFillUnordered
    with virtual surfaces, clearance 0, setCeiling(0.5) twice -- the floor stays 0 --: no surface voxel missed outside the
    seam, no virtual voxel missed."""
    scene, surface, virtual, seam = multi_level_scene()
    src = scene.source()
    p = R.Params(0.1, 0.0, reference_pos=(0.0, 0.0, 1.1 * 1.5), ceiling=0.5, virtual_surface=True)
    res = LR.build_layered(src, p, LR.MODE_UNORDERED, 0)
    hm, dims, first, _, _ = R.heightmap_geometry(src, p, (res.min_ext, res.max_ext))
    surface, virtual = set(surface), set(virtual)
    for slot, cb, ca in zip(*np.nonzero(res.occupancy != np.inf)):
        g = [first[0] + int(ca), first[1] + int(cb), int(slot)]
        centre = hm.voxel_centre([g[c] // dims[c] for c in range(3)], [g[c] % dims[c] for c in range(3)])
        key = tuple(scene.key((centre[0], centre[1], centre[2] + float(res.voxels["height"][slot, cb, ca]))))
        if res.occupancy[slot, cb, ca] > 0:
            assert scene.is_occupied(key)
            surface.discard(key)
        else:
            assert res.occupancy[slot, cb, ca] == -1.0 and scene.is_free(key)
            virtual.discard(key)
    assert (len(surface - seam), len(virtual)) == (0, 0)
    assert res.multi_layer_columns == 0 and res.filtered == 0 and res.layers >= 2


# -- hand-derived walks ------------------------------------------------------------------------------------------------------

def both(scene, p, mode, threshold=0):
    fifo = LR.build_layered(scene.source(), p, mode, threshold)
    assert_same_result(fifo, LR.build_layered_generations(scene.source(), p, mode, threshold))
    return fifo


def test_seed_column_is_queued_again_and_repeats():
    """Two columns with the floor at 1, seed (0, 0, 1).  begin touches nothing, so column 1's offer (cell 0, 1) is
    accepted and the seed's column is visited again: the same ground, a repeat.  Its offer (cell 1, 1) is refused."""
    res = both(hand_scene({(0, 0): [1], (1, 0): [1]}), hand_params(2, 1, (0, 0, 1)), LR.MODE_ORDERED)
    assert res.log.tolist() == [[0, 0, 1], [1, 0, 1], [0, 0, 1]]
    assert LR.stats_of(res) == (3, 2, 2, 2, 1, 0, 0, 0, 1, 3, 1)
    assert res.source_visit[0, 0, :2].tolist() == [0, 1] and res.layer_count[0, :2].tolist() == [1, 1]
    assert res.voxels["layer"][0, 0, :2].tolist() == [LR.HVL_BASE, LR.HVL_BASE]  # L7: a single voxel is the base layer


def _three_columns(mode):
    """L (0, 0) holds voxel 3, A (1, 0) voxels 1 and 3, R (2, 0) voxel 1; seed L at 3; z voxels 0 .. 4.
    v0 L3: ground 3, offers (A, 3).                                        v1 A3: ground 3 -> A slot 0, height 1.5, no
    clearance and nothing observed above: kHvlExtended; offers (L, 3) -- the seed was never touched -- and (R, 3).
    v2 L3: a repeat.   v3 R3: the only voxel is 1 -> hg 1, offers (A, 1).  v4 A1: ground 1, clearance 2 -> a base
    candidate, into slot 1: height -0.5 - 1 = -1.5; offers (L, 1), (R, 1).   v5 L1: climbs to 3, a repeat.   v6 R1: a
    repeat."""
    return both(hand_scene({(0, 0): [3], (1, 0): [1, 3], (2, 0): [1]}), hand_params(3, 1, (0, 0, 3), top=4), mode)


def test_two_layers_sorted_and_the_base_layer():
    res = _three_columns(LR.MODE_ORDERED)
    assert res.log.tolist() == [[0, 0, 3], [1, 0, 3], [0, 0, 3], [2, 0, 3], [1, 0, 1], [0, 0, 1], [2, 0, 1]]
    assert LR.stats_of(res) == (7, 4, 3, 4, 3, 0, 0, 1, 2, 5, 2)
    assert res.generation_sizes == [1, 1, 2, 1, 2]
    assert res.layer_count[0, :3].tolist() == [1, 2, 1] and res.quirks["permuted_columns"] == 1
    # A: sorted by height, each height relative to its new slot's centre; the voxel with clearance is the base layer
    assert res.voxels["height"][:, 0, 1].tolist() == [-0.5, 0.5]
    assert res.voxels["layer"][:, 0, 1].tolist() == [LR.HVL_BASE, LR.HVL_EXTENDED]
    assert res.voxels["clearance"][:, 0, 1].tolist() == [2.0, 0.0]
    assert res.source_visit[:, 0, 1].tolist() == [4, 1]
    # L and R: single voxels become the base layer; their empty slot is cleared
    assert res.voxels["layer"][0, 0, [0, 2]].tolist() == [LR.HVL_BASE, LR.HVL_BASE]
    assert res.voxels["height"][0, 0, [0, 2]].tolist() == [1.5, -0.5]
    assert np.isinf(res.occupancy[1, 0, [0, 2]]).all() and res.source_visit[1, 0, 0] == LR.NO_VISIT


def test_unordered_keeps_insertion_order_and_layers():
    res = _three_columns(LR.MODE_UNORDERED)
    assert LR.stats_of(res) == (7, 4, 3, 4, 3, 0, 0, 0, 2, 5, 2)
    assert res.voxels["height"][:, 0, 1].tolist() == [1.5, -1.5]
    assert res.voxels["layer"][:, 0, 1].tolist() == [LR.HVL_EXTENDED, LR.HVL_BASE]
    assert res.voxels["layer"][0, 0, [0, 2]].tolist() == [LR.HVL_EXTENDED, LR.HVL_EXTENDED]
    assert res.source_visit[:, 0, 1].tolist() == [1, 4]


def test_too_close_is_refused_for_a_real_voxel():
    """The three columns with min_clearance 2: rule 4 now passes voxel 3 as clearance from voxel 1 just the same (2 >= 2),
    and v4's add finds the voxel at 1.5 above it by 2 <= 2: dropped as too close, though both are real surfaces."""
    scene = hand_scene({(0, 0): [3], (1, 0): [1, 3], (2, 0): [1]})
    p = hand_params(3, 1, (0, 0, 3), top=4)
    p.min_clearance = 2.0
    res = both(scene, p, LR.MODE_ORDERED)
    assert (res.too_close, res.quirks["too_close_real"], res.multi_layer_columns) == (1, 1, 0)
    assert res.layer_count[0, :3].tolist() == [1, 1, 1] and res.voxels["height"][0, 0, 1] == 1.5


def test_empty_map_builds_nothing():
    from heightmap_fill_cases import Scene
    assert LR.build_layered(Scene(1.0, (4, 4, 4)).source(), R.Params(1.0, 0.0)) is None
    assert LR.build_layered_generations(Scene(1.0, (4, 4, 4)).source(), R.Params(1.0, 0.0)) is None
