"""CPU: the point cloud restatement (tests/cloud_ref.py) against answers derived by hand.

One region of 2 x 2 x 2 voxels at resolution 1.0 (a region spans 2.0), region key (1, -1, 0), map origin (10, 20, 30).
voxelCentre per axis = region * 2 - 1 + origin + local + 0.5:
  global  x = 11.5 + lx    y = 17.5 + ly    z = 29.5 + lz
  local   x =  1.5 + lx    y = -2.5 + ly    z = -0.5 + lz      (origin zero: TSDF and CLEARANCE)
A mean cell is 1 / 1023 wide and the decoded offset is cell * (1 / 1023) - 0.5 per axis: coord 0 decodes to -0.5 on
every axis, coord (1023, 0, 1023) to (+0.5, -0.5, +0.5)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as CR  # noqa: E402
import heightmap_ref as HR  # noqa: E402

DIM = (2, 2, 2)
ORIGIN = (10.0, 20.0, 30.0)
REGION = (1, -1, 0)
THRESHOLD = np.float32(0.0)
INF = np.float32(np.inf)


def centre(index, local=False):
    lx, ly, lz = index % 2, (index // 2) % 2, index // 4
    if local:
        return [1.5 + lx, -2.5 + ly, -0.5 + lz]
    return [11.5 + lx, 17.5 + ly, 29.5 + lz]


def extract(chunks, layers, **kw):
    return CR.extract(chunks, 1.0, DIM, ORIGIN, THRESHOLD, layers, CR.Params(**kw))


def indices(cloud):
    v = cloud.keys["voxel"].astype(int)
    return list(v[:, 0] + 2 * v[:, 1] + 4 * v[:, 2])


#           index   0     1     2     3      4     5      6     7
OCC = np.array([0.0, 2.5, -1.0, INF, np.nan, -0.0, -np.inf, 1e-30], dtype=np.float32)


def test_occupancy_rules():
    chunks = {REGION: {"occupancy": OCC}}
    c = extract(chunks, ["occupancy"])
    # equal to the threshold passes (index 0, and -0.0 == 0.0 at index 5); +inf and NaN do not; free voxels do not
    assert indices(c) == [0, 1, 5, 7] and c.count == 4 and c.considered == 8
    assert c.positions.tolist() == [centre(i) for i in (0, 1, 5, 7)]
    assert np.array_equal(c.values.view(np.uint32), OCC[[0, 1, 5, 7]].view(np.uint32))
    assert c.keys["region"].tolist() == [list(REGION)] * 4
    assert c.keys["voxel"].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 1, 0], [1, 1, 1, 0]]
    f = extract(chunks, ["occupancy"], export_free=True)
    assert indices(f) == [0, 1, 2, 5, 6, 7]  # free: -1 and -inf; still neither +inf nor NaN


def test_mean_positions():
    mean = np.zeros((8, 2), dtype=np.uint32)
    mean[1] = (1023 | (0 << 10) | (1023 << 20) | (1 << 31), 3)
    mean[7] = (512 | (1 << 31), 1)
    chunks = {REGION: {"occupancy": OCC, "mean": mean.reshape(-1)}}
    c = extract(chunks, ["occupancy", "mean"], export_free=True)
    assert indices(c) == [0, 1, 2, 5, 6, 7]
    p = dict(zip(indices(c), c.positions.tolist()))
    # the free voxel at index 2 was never written: coord 0 still decodes, to the voxel's lower corner
    assert p[2] == [11.5 - 0.5, 18.5 - 0.5, 29.5 - 0.5]
    assert p[1] == [12.5 + (1023 * (1.0 / 1023.0) - 0.5), 17.5 - 0.5, 29.5 + (1023 * (1.0 / 1023.0) - 0.5)]
    assert p[7] == [12.5 + (512 * (1.0 / 1023.0) - 0.5), 18.5 - 0.5, 30.5 - 0.5]
    i = extract(chunks, ["occupancy", "mean"], export_free=True, ignore_voxel_mean=True)
    assert i.positions.tolist() == [centre(k) for k in (0, 1, 2, 5, 6, 7)]
    # a map without the mean layer: the centre
    n = extract({REGION: {"occupancy": OCC}}, ["occupancy"], export_free=True)
    assert n.positions.tolist() == i.positions.tolist()


def test_helpers_agree_with_the_oracle():
    """The vectorised key maths of the restatement against the oracle's scalar functions (heightmap_ref)."""
    src = HR.Source(0.1, (5, 7, 3), {}, 0.0, origin=(0.3, -0.7, 12.25))
    region = (-3, 2, 117)
    got, local = CR.voxel_centres(region, (5, 7, 3), 0.1, (0.3, -0.7, 12.25))
    for index in (0, 4, 5, 34, 35, 104):
        assert tuple(got[index]) == src.om.voxel_centre(region, tuple(int(v) for v in local[index]))
    coords = np.array([0, 1, 1023, 1 << 10, (1 << 31) | 12345678, 0xffffffff], dtype=np.uint32)
    off = CR.sub_voxel_to_local(coords, 0.1)
    for i, coord in enumerate(coords):
        assert off[i].tolist() == HR.sub_voxel_to_local(int(coord), 0.1)


def test_density_rules():
    #                  count 0   traversal 0   2 / 4    1 / 0.5   traversal < 0   count 0, traversal 0
    count = np.array([0, 3, 2, 1, 5, 0, 0, 0], dtype=np.uint32)
    traversal = np.array([1.0, 0.0, 4.0, 0.5, -1.0, 0.0, 2.0, 3.0], dtype=np.float32)
    mean = np.zeros((8, 2), dtype=np.uint32)
    mean[:, 1] = count
    chunks = {REGION: {"occupancy": OCC, "mean": mean.reshape(-1), "traversal": traversal}}
    layers = ["occupancy", "mean", "traversal"]
    c = extract(chunks, layers, mode=CR.DENSITY)  # threshold 0: every voxel
    assert indices(c) == list(range(8))
    assert c.values.tolist() == [0.0, np.inf, 0.5, 2.0, np.inf, 0.0, 0.0, 0.0]
    assert c.positions.tolist() == [[v - 0.5 for v in centre(i)] for i in range(8)]  # coord 0 everywhere
    h = extract(chunks, layers, mode=CR.DENSITY, density_threshold=0.5)
    assert indices(h) == [1, 2, 3, 4]
    g = extract(chunks, layers, mode=CR.DENSITY, density_threshold=0.5, ignore_voxel_mean=True)
    assert g.positions.tolist() == [centre(i) for i in (1, 2, 3, 4)]  # the origin is part of the position
    assert extract(chunks, layers, mode=CR.DENSITY, density_threshold=np.inf).count == 2


def test_tsdf_rules():
    #                   weight 0    |d| == 0.25   negative   beyond    inside
    tsdf = np.array([[0.0, 0.0], [1.0, 0.25], [2.0, -0.1], [1.0, 0.3], [0.5, 0.2], [1.0, -0.25], [-1.0, 0.0],
                     [1.0, 0.0]], dtype=np.float32)
    chunks = {REGION: {"tsdf": tsdf.reshape(-1)}}
    c = extract(chunks, ["tsdf"], mode=CR.TSDF, surface_distance=0.25)
    assert indices(c) == [2, 4, 7]
    assert c.values.tolist() == [float(np.float32(-0.1)), float(np.float32(0.2)), 0.0]
    assert c.positions.tolist() == [centre(i, local=True) for i in (2, 4, 7)]  # no origin


def test_clearance_rules():
    #                 occupied  free   unobserved  occupied  free  NaN (unobserved)  occupied  free
    occ = np.array([1.0, -1.0, INF, 2.0, -2.0, np.nan, 0.0, -0.5], dtype=np.float32)
    clr = np.array([0.5, 1.5, -1.0, -1.0, 0.0, 2.0, -3.0, -1.0], dtype=np.float32)
    chunks = {REGION: {"occupancy": occ, "clearance": clr}}
    layers = ["occupancy", "clearance"]
    c = extract(chunks, layers, mode=CR.CLEARANCE, colour_range=4.0, export_type=-1)
    assert indices(c) == list(range(8))
    assert c.values.tolist() == [0.5, 1.5, 4.0, 4.0, 0.0, 2.0, 4.0, 4.0]  # negative ranges become colour_range
    assert c.positions.tolist() == [centre(i, local=True) for i in range(8)]
    f = extract(chunks, layers, mode=CR.CLEARANCE, colour_range=4.0, export_type=0)
    assert indices(f) == [0, 1, 3, 4, 6, 7]
    o = extract(chunks, layers, mode=CR.CLEARANCE, colour_range=4.0, export_type=1)
    assert indices(o) == [0, 3, 6]
    d = extract(chunks, layers, mode=CR.CLEARANCE, colour_range=-1.0, export_type=-1)
    assert indices(d) == [0, 1, 4, 5]  # a voxel without a range is dropped when colour_range < 0
    z = extract(chunks, layers, mode=CR.CLEARANCE, colour_range=0.0, export_type=1)
    assert indices(z) == [0, 3, 6] and z.values.tolist() == [0.5, 0.0, 0.0]


def _one(value=1.0):
    block = np.full(8, INF, dtype=np.float32)
    block[0] = value
    return {"occupancy": block}


def test_region_order_and_extents():
    regions = [(0, 0, 0), (-1, 0, 0), (1, -1, 0), (0, 0, -1), (5, -2, -1), (-3, 1, 1), (2, 0, 0)]
    chunks = {r: _one() for r in regions}
    c = extract(chunks, ["occupancy"])
    assert [tuple(r) for r in c.keys["region"].tolist()] == [(5, -2, -1), (0, 0, -1), (1, -1, 0), (-1, 0, 0), (0, 0, 0),
                                                             (2, 0, 0), (-3, 1, 1)]
    # regionKey(p) = floor((p - origin) / 2 + 0.5): x in [9, 11) is region 0, [11, 13) region 1; whole regions take part
    e = extract(chunks, ["occupancy"], extents=((9.0, 17.0, 29.0), (12.9, 20.9, 30.9)))
    assert [tuple(r) for r in e.keys["region"].tolist()] == [(1, -1, 0), (0, 0, 0)]
    assert e.considered == 16
    assert CR.region_key((12.9, 17.0, 26.99), ORIGIN, DIM, 1.0) == (1, -1, -2)
    # inverted extents select nothing
    assert extract(chunks, ["occupancy"], extents=((12.9, 20.9, 30.9), (9.0, 17.0, 29.0))).count == 0
    # in every mode
    t = {r: {"tsdf": np.tile(np.array([1.0, 0.0], dtype=np.float32), 8)} for r in regions}
    assert extract(t, ["tsdf"], mode=CR.TSDF, surface_distance=1.0,
                   extents=((9.0, 17.0, 29.0), (12.9, 20.9, 30.9))).count == 16


@pytest.mark.parametrize("mode,layers", [(CR.OCCUPANCY, ["mean"]), (CR.DENSITY, ["occupancy", "mean"]),
                                         (CR.DENSITY, ["occupancy", "traversal"]), (CR.TSDF, ["occupancy"]),
                                         (CR.CLEARANCE, ["occupancy"]), (CR.CLEARANCE, ["clearance"])])
def test_missing_layer_gives_an_empty_cloud(mode, layers):
    c = extract({REGION: _one()}, layers, mode=mode, surface_distance=1.0)
    assert c.count == 0 and c.positions.shape == (0, 3) and c.keys.shape == (0,) and c.values.shape == (0,)


def test_empty_map():
    assert extract({}, ["occupancy"]).count == 0
