"""CPU: the restatement of copyMap's selection (tests/copy_ref.py) on hand-derived cases, and the Python mirror's
helpers (ohm_amd/copyutil.py) against it.  No device.

The geometry of the hand-derived cases is exact in binary: resolution 0.25 and 8 voxels per axis give regions of 2.0, so
region c spans [2c - 1, 2c + 1] about its centre 2c with no rounding anywhere."""
import itertools

import numpy as np

import copy_ref as R
from ohm_amd import copyutil as U

SPATIAL = R.spatial_dimensions(0.25, (8, 8, 8))
INF = float("inf")


def _up(x):
    return float(np.nextafter(x, INF))


def _down(x):
    return float(np.nextafter(x, -INF))


def _box(axis, lo, hi):
    mn, mx = [-INF] * 3, [INF] * 3
    mn[axis], mx[axis] = lo, hi
    return mn, mx


def test_geometry_is_exact():
    assert SPATIAL == (2.0, 2.0, 2.0)
    assert R.region_centre((3, -2, 0), SPATIAL) == (6.0, -4.0, 0.0)


def test_touching_passes_one_ulp_apart_fails():
    for axis in range(3):
        coord = [0, 0, 0]
        coord[axis] = 2          # lo = 3, hi = 5 on `axis`
        # hi == min_ext exactly: not (hi < min_ext)
        assert R.passes_extents(coord, SPATIAL, *_box(axis, 5.0, 9.0))
        # hi one ulp below min_ext
        assert not R.passes_extents(coord, SPATIAL, *_box(axis, _up(5.0), 9.0))
        assert R.passes_extents(coord, SPATIAL, *_box(axis, _down(5.0), 9.0))
        # lo == max_ext exactly: not (lo > max_ext)
        assert R.passes_extents(coord, SPATIAL, *_box(axis, -9.0, 3.0))
        # lo one ulp above max_ext
        assert not R.passes_extents(coord, SPATIAL, *_box(axis, -9.0, _down(3.0)))
        assert R.passes_extents(coord, SPATIAL, *_box(axis, -9.0, _up(3.0)))


def test_every_axis_must_pass():
    box = ([1.0, 1.0, 1.0], [3.0, 3.0, 3.0])
    assert R.passes_extents((1, 1, 1), SPATIAL, *box)
    assert R.passes_extents((0, 0, 0), SPATIAL, *box)          # hi == 1 on every axis: touching
    assert R.passes_extents((2, 2, 2), SPATIAL, *box)          # lo == 3
    assert not R.passes_extents((3, 1, 1), SPATIAL, *box)      # lo == 5 > 3 on x alone
    assert not R.passes_extents((1, -1, 1), SPATIAL, *box)     # hi == -1 < 1 on y alone


def test_infinite_box_passes_everything():
    box = ([-INF] * 3, [INF] * 3)
    for coord in itertools.product((-32768, -1, 0, 7, 32767), repeat=3):
        assert R.passes_extents(coord, SPATIAL, *box)
    # an inverted infinite box passes nothing
    assert not R.passes_extents((0, 0, 0), SPATIAL, [INF] * 3, [-INF] * 3)


def test_box_is_relative_to_the_map_origin():
    """MapRegion::centre is coord * region dimension without the origin (ohm/MapRegion.cpp:40-42): with the origin at
    (1.3, -2.7, 0.05) region 0 covers the world's [0.3, 2.3] on x, yet the filter sees [-1, 1]."""
    origin = (1.3, -2.7, 0.05)
    box = ([1.5, -INF, -INF], [3.0, INF, INF])
    assert R.region_centre((1, 0, 0), SPATIAL, origin) == (2.0, 0.0, 0.0)
    assert not R.passes_extents((0, 0, 0), SPATIAL, *box, origin=origin)   # hi = 1 < 1.5 although 2.3 > 1.5 in the world
    assert R.passes_extents((1, 0, 0), SPATIAL, *box, origin=origin)
    assert R.passes_extents((2, 0, 0), SPATIAL, *box, origin=origin)       # lo = 3 == max: touching; world lo is 4.3
    regions = [(x, 0, 0) for x in range(-2, 5)]
    assert R.select_regions(regions, SPATIAL, extents=box, origin=origin) == R.select_regions(regions, SPATIAL, extents=box)
    assert R.select_regions(regions, SPATIAL, extents=box)[0] == [(1, 0, 0), (2, 0, 0)]


def test_inexact_geometry_follows_the_operation_order():
    """0.1 * 32: the sums round, and the rule is judged on the rounded values."""
    spatial = R.spatial_dimensions(0.1, (32, 32, 32))
    s = 32.0 * 0.1
    hi = 1.0 * s + 0.5 * s
    assert R.passes_extents((1, 0, 0), spatial, [hi, -INF, -INF], [INF] * 3)
    assert not R.passes_extents((1, 0, 0), spatial, [_up(hi), -INF, -INF], [INF] * 3)
    assert hi != 4.8  # (what exact arithmetic would give: the restatement must not "simplify")


def test_key_list_absent_and_repeated():
    regions = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
    passed, absent = R.select_regions(regions, SPATIAL, keys=[(1, 0, 0), (5, 5, 5), (1, 0, 0), (0, 0, 0), (-3, 0, 0)])
    assert passed == [(1, 0, 0), (0, 0, 0)] and absent == 2
    passed, absent = R.select_regions(regions, SPATIAL, keys=[(1, 0, 0), (0, 1, 0)], dirty={(0, 1, 0)},
                                      extents=([-INF] * 3, [INF] * 3))
    assert passed == [(0, 1, 0)] and absent == 0
    # without a list: the callers' region order, z then y then x
    assert R.select_regions(regions, SPATIAL)[0] == [(0, 0, 0), (1, 0, 0), (0, 1, 0)]


def test_layers():
    assert R.copied_layers(["occupancy", "mean", "covariance"], ["mean", "occupancy", "traversal"]) == ["occupancy", "mean"]
    assert R.copied_layers(["tsdf"], ["occupancy"]) is None
    assert R.copied_layers(["occupancy", "mean"], ["occupancy", "mean"], lambda n: n == "mean") == ["mean"]
    assert R.copied_layers(["occupancy", "mean"], ["occupancy", "mean"], lambda n: False) == []


def test_predicted_stats():
    st = R.predict_stats([(0, 0, 0), (1, 0, 0)], [(1, 0, 0)], SPATIAL, ["occupancy", "mean"], ["occupancy", "mean", "tsdf"],
                         512, keys=[(0, 0, 0), (1, 0, 0), (9, 9, 9)])
    assert st == {"regions_passed": 2, "regions_created": 1, "keys_absent": 1, "bytes_copied": 2 * 512 * 12,
                  "layers_copied": 3}
    st = R.predict_stats([(0, 0, 0)], [], SPATIAL, ["occupancy"], ["occupancy"], 512, layer_filter=lambda n: False)
    assert st["regions_created"] == 1 and st["bytes_copied"] == 0 and st["layers_copied"] == 0


# ---- the Python mirror's helpers against the restatement ------------------------------------------------------------
def _chunks(dirty=()):
    return [U.chunk_view(c, SPATIAL, c in dirty) for c in itertools.product(range(-2, 4), repeat=3)]


def test_mirror_extents_filter_agrees():
    boxes = [([1.0, 1.0, 1.0], [3.0, 3.0, 3.0]), ([_up(1.0), -INF, -INF], [INF] * 3), ([-INF] * 3, [_down(3.0), INF, INF]),
             ([-INF] * 3, [INF] * 3), ([0.3, -2.2, 1.7], [0.4, 5.1, 1.9])]
    for mn, mx in boxes:
        f = U.copyFilterExtents(mn, mx)
        for chunk in _chunks():
            assert f(chunk) == R.passes_extents(chunk.region.coord, SPATIAL, mn, mx), (mn, mx, chunk)
    # the view's centre is the restatement's, for an inexact geometry too
    spatial = R.spatial_dimensions(0.1, (5, 3, 7))
    assert U.region_spatial_dimensions(type("M", (), {"resolution": 0.1, "region_voxel_dimensions": (5, 3, 7)})) == spatial
    for c in ((3, -7, 11), (-32768, 32767, 1)):
        assert U.chunk_view(c, spatial).region.centre == R.region_centre(c, spatial)


def test_mirror_dirty_filter():
    dirty = {(0, 0, 0), (1, 2, 3)}
    f = U.copyFilterDirty()
    assert [c.region.coord for c in _chunks(dirty) if f(c)] == sorted(dirty)


def test_mirror_combinators_with_empty_operands():
    a = U.copyFilterExtents([1.0] * 3, [3.0] * 3)
    b = U.copyFilterDirty()
    # And: with an empty operand, the other one; empty when both are (CopyUtil.h:50-57)
    assert U.copyFilterAnd(a, None) is a and U.copyFilterAnd(None, b) is b and U.copyFilterAnd(None, None) is None
    # Or: an empty operand is an implied pass, the result is empty (:67-75)
    assert U.copyFilterOr(a, None) is None and U.copyFilterOr(None, b) is None and U.copyFilterOr(None, None) is None
    # Negate: the negation of an empty filter passes nothing (:81-91)
    none = U.copyFilterNegate(None)
    assert not any(none(c) for c in _chunks({(0, 0, 0)}))
    dirty = {(1, 1, 1), (3, 3, 3)}
    for chunk in _chunks(dirty):
        assert U.copyFilterAnd(a, b)(chunk) == (a(chunk) and b(chunk))
        assert U.copyFilterOr(a, b)(chunk) == (a(chunk) or b(chunk))
        assert U.copyFilterNegate(a)(chunk) == (not a(chunk))
    assert any(U.copyFilterAnd(a, b)(c) for c in _chunks(dirty)) and not all(U.copyFilterOr(a, b)(c) for c in _chunks(dirty))


def test_mirror_layer_filters():
    f = U.copyLayersFilter(["mean", "tsdf"])
    assert [n for n in R.LAYER_IDS if f(n)] == ["mean", "tsdf"]
    assert [n for n in R.LAYER_IDS if U.copyFilterNegate(f)(n)] == [n for n in R.LAYER_IDS if n not in ("mean", "tsdf")]
    assert not any(U.copyFilterNegate(None)(n) for n in R.LAYER_IDS)
    # the restatement's table is the library's
    from ohm_amd import LAYERS
    assert {n: LAYERS[n][0] for n in LAYERS} == R.LAYER_IDS
    assert {n: np.dtype(LAYERS[n][1]).itemsize * LAYERS[n][2] for n in LAYERS} == R.LAYER_BYTES
