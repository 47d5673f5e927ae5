"""CPU: the point-query entry points of the C ABI (ohmhip_map_nearest_neighbours / _device, ohmhip_map_voxel_keys,
ohmhip_map_read_voxels / _device) are exported, declared and bound, stay out of the core ABI list, and refuse invalid
arguments with OHMHIP_ERR_INVALID_ARG before any device work -- so the refusals run without a GPU; the Python mirrors'
classes and flag values.  (tests/test_gpu_nearest_neighbours.py repeats each refusal against a live map.)"""
import ctypes as C
import os

import numpy as np

import cpp_driver
import ohm_amd
from ohm_amd import GPU_KEY_DTYPE, GpuMap, NearestNeighbours, QueryFlag
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_nearest_neighbours", "ohmhip_map_nearest_neighbours_device", "ohmhip_map_voxel_keys",
         "ohmhip_map_read_voxels", "ohmhip_map_read_voxels_device")


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int


def test_declared_and_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_nearest_neighbours_device(" in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_read_voxels_device(" in header
    assert "OHMHIP_LID_COUNT = 10" in header  # no new layer
    assert "#define OHMHIP_QF_NEAREST_RESULT (1u << 1)" in header


def test_params_layout():
    assert C.sizeof(L.NeighboursParams) == 8
    assert L.NeighboursParams.search_radius.offset == 0 and L.NeighboursParams.query_flags.offset == 4
    assert (L.QF_UNKNOWN_AS_OCCUPIED, L.QF_NEAREST_RESULT) == (1, 2)
    assert int(QueryFlag.kQfUnknownAsOccupied) == 1 and int(QueryFlag.kQfNearestResult) == 2


def _nn(fn, map_=None, points=True, nq=1, params=True, radius=1.0, flags=0, capacity=0, counts=True, keys=None,
        total=True, point=(0.0, 0.0, 0.0)):
    p = L.NeighboursParams(radius, flags)
    pts = np.array([point] * max(nq, 1), dtype=np.float64)
    cnt = np.zeros(max(nq, 1), dtype=np.uint64)
    tot = C.c_uint64(0)
    return fn(map_, pts.ctypes.data if points else None, nq, C.byref(p) if params else None, capacity,
              cnt.ctypes.data if counts else None, keys, None, C.byref(tot) if total else None)


def test_nearest_neighbours_refusals():
    keys = np.zeros(4, dtype=GPU_KEY_DTYPE)
    for fn in (L.lib.ohmhip_map_nearest_neighbours, L.lib.ohmhip_map_nearest_neighbours_device):
        assert _nn(fn) == L.ERR_INVALID_ARG  # null map
        assert _nn(fn, params=False) == L.ERR_INVALID_ARG
        assert _nn(fn, points=False) == L.ERR_INVALID_ARG
        assert _nn(fn, counts=False) == L.ERR_INVALID_ARG
        assert _nn(fn, total=False) == L.ERR_INVALID_ARG
        assert _nn(fn, point=(0.0, float("nan"), 0.0)) == L.ERR_INVALID_ARG
        assert _nn(fn, point=(float("inf"), 0.0, 0.0)) == L.ERR_INVALID_ARG
        assert _nn(fn, radius=-1.0) == L.ERR_INVALID_ARG
        assert _nn(fn, radius=float("inf")) == L.ERR_INVALID_ARG
        assert _nn(fn, radius=float("nan")) == L.ERR_INVALID_ARG
        assert _nn(fn, flags=4) == L.ERR_INVALID_ARG
        assert _nn(fn, capacity=4) == L.ERR_INVALID_ARG
        assert _nn(fn, capacity=4, keys=keys.ctypes.data) == L.ERR_INVALID_ARG  # (still no map)
        assert _nn(fn, nq=0, points=False) == L.ERR_INVALID_ARG
        assert fn(None, None, 0, None, 0, None, None, None, None) == L.ERR_INVALID_ARG


def test_voxel_refusals():
    keys = np.zeros(2, dtype=GPU_KEY_DTYPE)
    values = np.zeros(2, dtype=np.float32)
    present = np.zeros(2, dtype=np.uint8)
    points = np.zeros((2, 3))
    assert L.lib.ohmhip_map_voxel_keys(None, points.ctypes.data, 2, keys.ctypes.data) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_voxel_keys(None, None, 0, None) == L.ERR_INVALID_ARG
    for fn in (L.lib.ohmhip_map_read_voxels, L.lib.ohmhip_map_read_voxels_device):
        assert fn(None, 0, keys.ctypes.data, 2, values.ctypes.data, present.ctypes.data) == L.ERR_INVALID_ARG
        assert fn(None, -1, keys.ctypes.data, 2, values.ctypes.data, present.ctypes.data) == L.ERR_INVALID_ARG
        assert fn(None, L.LID_COUNT, keys.ctypes.data, 2, values.ctypes.data, present.ctypes.data) == L.ERR_INVALID_ARG
        assert fn(None, 0, None, 2, None, None) == L.ERR_INVALID_ARG
        assert fn(None, 0, None, 0, None, None) == L.ERR_INVALID_ARG


def test_mirrors():
    for name in ("nearestNeighbours", "voxelKeys", "readVoxels", "occupancyTypes"):
        assert callable(getattr(GpuMap, name))
    assert ohm_amd.NearestNeighbours is NearestNeighbours
    q = NearestNeighbours(None, (1.0, 2.0, 3.0), 0.75, QueryFlag.kQfNearestResult)
    assert q.nearPoint() == (1.0, 2.0, 3.0) and q.searchRadius() == 0.75
    assert q.queryFlags() == int(QueryFlag.kQfNearestResult)
    q.setNearPoint((0.5, 0.0, -1.0))
    q.setSearchRadius(0.1)
    q.setQueryFlags(QueryFlag.kQfUnknownAsOccupied)
    assert q.nearPoint() == (0.5, 0.0, -1.0) and q.searchRadius() == float(np.float32(0.1))  # a float, as in the reference
    assert q.queryFlags() == 1
    assert q.execute() is False  # no map: nothing runs
    assert q.numberOfResults() == 0 and q.intersectedVoxels().dtype == GPU_KEY_DTYPE
    assert q.ranges().dtype == np.float64 and q.ranges().shape == (0,)
    q.reset()
    assert q.numberOfResults() == 0


def test_cpp_mirror_declares_the_same_interface():
    text = cpp_driver.host_mirror_text()
    for token in ("class NearestNeighbours", "setNearPoint", "setSearchRadius", "setQueryFlags", "numberOfResults",
                  "intersectedVoxels", "nearestNeighbours(", "voxelKeys(", "readVoxels(", "occupancyTypes("):
        assert token in text, token
