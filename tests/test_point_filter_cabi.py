"""CPU: the point-filter entry points of the C ABI (ohmhip_map_filter_points / _device) are exported, declared and bound,
stay out of the core ABI list, and refuse invalid arguments with OHMHIP_ERR_INVALID_ARG before any device work -- so the
refusals run without a GPU; the parameter struct's layout, the constants, and the Python and C++ mirrors.
(tests/test_gpu_point_filter.py repeats the refusals that need a live map.)"""
import ctypes as C
import os

import numpy as np

import cpp_driver
import ohm_amd
from ohm_amd import GPU_KEY_DTYPE, GpuMap
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_filter_points", "ohmhip_map_filter_points_device")


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
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_filter_points_device(" in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_filter_points(" not in header
    assert "/* POINT FILTER." in header and "utils/ohmfilter/ohmfilter.cpp:150-279" in header
    assert "OHMHIP_LID_COUNT = 10" in header  # no new layer
    assert "#define OHMHIP_PF_OCCUPANCY_ONLY (1u << 0)" in header
    assert "#define OHMHIP_PF_PIECE_POINTS (1u << 18)" in header


def test_params_layout_and_constants():
    assert C.sizeof(L.PointFilterParams) == 16
    assert L.PointFilterParams.expected_value_tolerance.offset == 0 and L.PointFilterParams.flags.offset == 8
    assert L.PF_OCCUPANCY_ONLY == 1 and L.PF_PIECE_POINTS == 1 << 18


def _call(device, map_=None, points=True, count=2, params=True, tolerance=0.0, flags=0, capacity=0, indices=None, kept=True,
          stride=3, point=(0.0, 0.0, 0.0)):
    p = L.PointFilterParams(tolerance, flags)
    pts = np.array([point] * max(count, 1), dtype=np.float64)
    status = np.zeros(max(count, 1), dtype=np.uint8)
    values = np.zeros(max(count, 1), dtype=np.float64)
    keys = np.zeros(max(count, 1), dtype=GPU_KEY_DTYPE)
    n = C.c_uint64(77)
    common = (C.byref(p) if params else None, capacity, status.ctypes.data, indices, values.ctypes.data, keys.ctypes.data,
              C.byref(n) if kept else None)
    if device:
        return L.lib.ohmhip_map_filter_points_device(map_, pts.ctypes.data if points else None, stride, count, *common)
    return L.lib.ohmhip_map_filter_points(map_, pts.ctypes.data if points else None, count, *common)


def test_refusals_without_a_map():
    indices = np.zeros(4, dtype=np.uint64)
    for device in (False, True):
        assert _call(device) == L.ERR_INVALID_ARG  # null map
        assert _call(device, params=False) == L.ERR_INVALID_ARG
        assert _call(device, kept=False) == L.ERR_INVALID_ARG
        assert _call(device, points=False) == L.ERR_INVALID_ARG
        assert _call(device, flags=2) == L.ERR_INVALID_ARG
        assert _call(device, flags=0x80000001) == L.ERR_INVALID_ARG
        assert _call(device, tolerance=float("nan")) == L.ERR_INVALID_ARG
        assert _call(device, capacity=4) == L.ERR_INVALID_ARG
        assert _call(device, capacity=4, indices=indices.ctypes.data) == L.ERR_INVALID_ARG  # (still no map)
        assert _call(device, count=0, points=False) == L.ERR_INVALID_ARG
    assert _call(True, stride=2) == L.ERR_INVALID_ARG and _call(True, stride=0) == L.ERR_INVALID_ARG
    assert _call(False, point=(0.0, float("nan"), 0.0)) == L.ERR_INVALID_ARG
    assert _call(False, point=(float("-inf"), 0.0, 0.0)) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_filter_points(None, None, 0, None, 0, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_filter_points_device(None, None, 3, 0, None, 0, None, None, None, None,
                                                 None) == L.ERR_INVALID_ARG


def test_mirrors():
    assert callable(GpuMap.filterPoints) and callable(GpuMap.lastFilterKept)
    assert callable(ohm_amd.filter_cloud) and callable(ohm_amd.write_filtered_ply)
    text = cpp_driver.host_mirror_text()
    for token in ("int filterPoints(", "ohmhip_map_filter_points(", "ohmhip_point_filter_params", "OHMHIP_PF_OCCUPANCY_ONLY"):
        assert token in text, token
    assert '{ "filter", &modeFilterPoints,' in cpp_driver.driver_text()  # the driver's mode table
