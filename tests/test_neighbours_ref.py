"""CPU: the NearestNeighbours restatement (tests/neighbours_ref.py) on hand-computed cases.  Resolution 0.25 with 8^3
regions: a region spans 2.0, the centre of local coordinate l of region r is 2 r - 1 + 0.25 l + 0.125, so every centre,
difference and square below is exact in float32."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import neighbours_ref as NR  # noqa: E402

RES, DIM = 0.25, (8, 8, 8)
INF = np.float32(np.inf)
THRESHOLD = np.float32(0.0)


def block(occupied, value=1.0, fill=INF):
    b = np.full(512, fill, dtype=np.float32)
    for (x, y, z) in occupied:
        b[x + 8 * y + 64 * z] = np.float32(value)
    return b


def query(blocks, point, radius, flags=0, origin=(0.0, 0.0, 0.0)):
    return NR.nearest_neighbours(blocks, RES, DIM, origin, THRESHOLD, [point], radius, flags)


def as_tuples(keys):
    return [(tuple(int(v) for v in k["region"]), tuple(int(v) for v in k["voxel"][:3])) for k in keys]


def test_centres_are_the_clearance_helper():
    c, local = NR.local_centres((-3, 2, 0), DIM, RES)
    for i in (0, 7, 100, 511):
        for a in range(3):
            assert c[i, a] == NR.centre((-3, 2, 0)[a], int(local[i, a]), RES, 8)
    assert c[0, 0] == np.float32(-6.875) and c[511, 1] == np.float32(4.875)


def test_voxel_on_the_sphere_is_included():
    centre = (-0.375, -0.375, -0.375)  # the centre of local (2, 2, 2) of region (0, 0, 0)
    for offset, radius in (((3, 0, 0), 0.75), ((3, 4, 0), 1.25)):
        target = (2 + offset[0], 2 + offset[1], 2 + offset[2])
        blocks = {(0, 0, 0): block([target])}
        counts, keys, ranges = query(blocks, centre, radius)
        assert counts.tolist() == [1] and as_tuples(keys) == [((0, 0, 0), target)]
        assert ranges.dtype == np.float32 and ranges[0] == np.float32(radius)  # r2 == r * r exactly
        inside = np.nextafter(np.float32(radius), np.float32(0))
        counts, keys, ranges = query(blocks, centre, inside)
        assert counts.tolist() == [0] and keys.size == 0 and ranges.size == 0


def test_corner_of_eight_voxels_in_two_regions():
    # (1, 0, 0): x = 1 is the face between regions 0 and 1; y = z = 0 the face between locals 3 and 4
    blocks = {(0, 0, 0): block([(7, y, z) for y in (3, 4) for z in (3, 4)]),
              (1, 0, 0): block([(0, y, z) for y in (3, 4) for z in (3, 4)])}
    counts, keys, ranges = query(blocks, (1.0, 0.0, 0.0), 0.25)
    assert counts.tolist() == [8]
    want = [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (7, 4, 3)), ((0, 0, 0), (7, 3, 4)), ((0, 0, 0), (7, 4, 4)),
            ((1, 0, 0), (0, 3, 3)), ((1, 0, 0), (0, 4, 3)), ((1, 0, 0), (0, 3, 4)), ((1, 0, 0), (0, 4, 4))]
    assert as_tuples(keys) == want
    assert (ranges == np.sqrt(np.float32(0.046875))).all()  # 3 * 0.125^2
    counts, keys, ranges = query(blocks, (1.0, 0.0, 0.0), 0.25, NR.QF_NEAREST_RESULT)
    assert counts.tolist() == [1] and as_tuples(keys) == want[:1] and ranges[0] == np.sqrt(np.float32(0.046875))
    # a strictly closer voxel later in the order takes it
    counts, keys, _ = query(blocks, (1.0625, 0.0, 0.0), 0.5, NR.QF_NEAREST_RESULT)
    assert counts.tolist() == [1] and as_tuples(keys) == [((1, 0, 0), (0, 3, 3))]


def test_obstruction_rule():
    centre = (-0.375, -0.375, -0.375)
    at_threshold = {(0, 0, 0): block([(3, 2, 2)], value=THRESHOLD, fill=np.float32(-1.0))}
    assert query(at_threshold, centre, 0.3)[0].tolist() == [1]
    below = {(0, 0, 0): block([(3, 2, 2)], value=np.nextafter(THRESHOLD, np.float32(-1)), fill=np.float32(-1.0))}
    assert query(below, centre, 0.3)[0].tolist() == [0]
    nan = {(0, 0, 0): block([(3, 2, 2)], value=np.nan, fill=np.float32(-1.0))}
    assert query(nan, centre, 0.3)[0].tolist() == [0]
    assert query(nan, centre, 0.3, NR.QF_UNKNOWN_AS_OCCUPIED)[0].tolist() == [0]
    unobserved = {(0, 0, 0): block([(3, 2, 2)], value=np.inf, fill=np.float32(-1.0))}
    assert query(unobserved, centre, 0.3)[0].tolist() == [0]
    counts, keys, ranges = query(unobserved, centre, 0.3, NR.QF_UNKNOWN_AS_OCCUPIED)
    assert counts.tolist() == [1] and as_tuples(keys) == [((0, 0, 0), (3, 2, 2))] and ranges[0] == np.float32(0.25)


def test_absent_region():
    centre = (-0.375, -0.375, -0.375)
    assert query({}, centre, 0.3)[0].tolist() == [0]
    counts, keys, ranges = query({}, centre, 0.3, NR.QF_UNKNOWN_AS_OCCUPIED)
    # the voxel itself and its six face neighbours (0.25 away; the edge neighbours are 0.3536 away)
    assert counts.tolist() == [7]
    assert as_tuples(keys) == [((0, 0, 0), v) for v in [(2, 2, 1), (2, 1, 2), (1, 2, 2), (2, 2, 2), (3, 2, 2), (2, 3, 2),
                                                         (2, 2, 3)]]
    assert ranges.tolist() == [0.25, 0.25, 0.25, 0.0, 0.25, 0.25, 0.25]
    nearest = query({}, centre, 0.3, NR.QF_UNKNOWN_AS_OCCUPIED | NR.QF_NEAREST_RESULT)
    assert nearest[0].tolist() == [1] and as_tuples(nearest[1]) == [((0, 0, 0), (2, 2, 2))] and nearest[2][0] == 0


def test_queries_concatenate_and_origin_shifts():
    blocks = {(0, 0, 0): block([(5, 2, 2)])}
    origin = (10.0, -4.0, 0.5)
    points = [(9.625, -4.375, 0.125), (100.0, 100.0, 100.0), (10.375, -4.375, 0.125)]
    counts, keys, ranges = NR.nearest_neighbours(blocks, RES, DIM, origin, THRESHOLD, points, 0.75)
    assert counts.tolist() == [1, 0, 1] and ranges.tolist() == [0.75, 0.0]
    assert as_tuples(keys) == [((0, 0, 0), (5, 2, 2))] * 2


def test_region_box():
    assert NR.query_regions((1.0, 0.0, 0.0), 0.25, (0, 0, 0), DIM, RES) == [(0, 0, 0), (1, 0, 0)]
    assert len(NR.query_regions((0.0, 0.0, 0.0), 1.0, (0, 0, 0), DIM, RES)) == 8  # regionKey(-1) is region 0
    box = NR.query_regions((0.0, 0.0, 0.0), 1.5, (0, 0, 0), DIM, RES)
    assert len(box) == 27 and box[0] == (-1, -1, -1) and box[1] == (0, -1, -1) and box[3] == (-1, 0, -1)


def test_occupancy_types():
    values = np.array([np.inf, np.nan, -1.0, 0.0, 2.0, 2.0], dtype=np.float32)
    present = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)
    assert NR.occupancy_types(values, present, 0.0).tolist() == [-1, -1, 0, 1, 1, -2]
