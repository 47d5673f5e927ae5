"""CPU: the clearance layer's C ABI (ohmhip_map_clearance_stale_regions / _update / _update_regions) is exported and
bound, refuses null arguments with OHMHIP_ERR_INVALID_ARG before any device work, stays out of the core ABI list; the
layer id and its voxel size; the Python mirrors (LAYERS["clearance"], MappingProcessResult, Mapper); and the stale-set
restatement (tests/clearance_update_ref.py) on hand-built logs."""
import ctypes as C
import os
import sys

import numpy as np

from ohm_amd import LAYERS, ClearanceProcess, Mapper, MappingProcessResult, OccupancyMap
from ohm_amd import _lib as L

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from clearance_update_ref import ClearanceLog, neighbourhood, params_of, reach  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_clearance_stale_regions", "ohmhip_map_clearance_update", "ohmhip_map_clearance_update_regions")


def _params(radius=0.5):
    p = L.ClearanceParams()
    p.search_radius = radius
    for i in range(3):
        p.axis_scaling[i] = 1.0
    return p


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int


def test_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    assert "OHMHIP_LID_CLEARANCE = 9" in header and "OHMHIP_LID_COUNT = 10" in header


def test_null_arguments():
    p = _params()
    keys = np.zeros((1, 3), dtype=np.int16)
    n = C.c_size_t(7)
    processed, remaining = C.c_size_t(7), C.c_size_t(7)
    assert L.lib.ohmhip_map_clearance_stale_regions(None, C.byref(p), keys.ctypes.data, 1, C.byref(n)) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_stale_regions(None, None, None, 0, None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_update(None, C.byref(p), 0, C.byref(processed), C.byref(remaining)) == \
        L.ERR_INVALID_ARG
    assert processed.value == 0 and remaining.value == 0
    assert L.lib.ohmhip_map_clearance_update(None, None, 0, None, None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_update_regions(None, keys.ctypes.data, 1, C.byref(p), 1, C.byref(processed)) == \
        L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_clearance_update_regions(None, None, 1, None, 0, None) == L.ERR_INVALID_ARG


def test_layer_id_and_size():
    assert L.LID_CLEARANCE == 9 and L.LID_COUNT == 10
    assert L.lib.ohmhip_layer_voxel_bytes(9) == 4
    assert L.lib.ohmhip_layer_voxel_bytes(10) == 0
    assert LAYERS["clearance"] == (L.LID_CLEARANCE, np.float32, 1)


def test_mirrors():
    assert MappingProcessResult.kMprUpToDate == 0 and MappingProcessResult.kMprProgressing == 1
    mapper = Mapper()
    cp = ClearanceProcess(1.0)
    mapper.addProcess(cp)
    assert mapper.processes() == [cp]
    assert mapper.update() == MappingProcessResult.kMprUpToDate  # (no map, nothing to do: no device call)
    map_ = OccupancyMap(0.25)
    ClearanceProcess.ensureClearanceLayer(map_)
    assert "clearance" in map_.layers and map_.layers.count("clearance") == 1


def test_reach():
    assert reach(0, (32, 32, 32)) == (0, 0, 0)
    assert reach(5, (32, 32, 32)) == (1, 1, 1)
    assert reach(32, (32, 32, 32)) == (1, 1, 1)
    assert reach(33, (32, 32, 32)) == (2, 2, 2)
    assert reach(20, (16, 16, 16)) == (2, 2, 2)
    assert reach(12, (5, 16, 7)) == (3, 1, 2)
    assert len(neighbourhood((0, 0, 0), (1, 1, 1))) == 27
    assert len(neighbourhood((0, 0, 0), (2, 0, 1))) == 15


def test_new_regions_are_stale_in_key_order():
    log = ClearanceLog(0.25, (32, 32, 32))
    present = [(1, 0, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0)]
    p = params_of(1.0)
    assert log.stale(present, p) == [(0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 0, 1)]
    log.written(present, p)
    assert log.stale(present, p) == []


def test_change_reaches_the_neighbourhood_only():
    log = ClearanceLog(0.25, (32, 32, 32))  # radius 1 m: h = 4, D = 1
    present = [(x, 0, 0) for x in range(-3, 4)]
    p = params_of(1.0)
    log.written(present, p)
    log.change([(0, 0, 0)])
    assert log.stale(present, p) == [(-1, 0, 0), (0, 0, 0), (1, 0, 0)]
    log.written([(-1, 0, 0)], p)  # a partial update
    assert log.stale(present, p) == [(0, 0, 0), (1, 0, 0)]


def test_reach_two():
    """16^3 regions at h = 20: D = 2, a change two regions away makes R stale; three away does not."""
    log = ClearanceLog(0.1, (16, 16, 16))
    p = params_of(2.0)
    assert reach(20, (16, 16, 16)) == (2, 2, 2)
    present = [(0, 0, 0), (2, 0, 0), (0, 0, 3)]
    log.written(present, p)
    log.change([(2, 0, 0)])
    assert log.stale(present, p) == [(0, 0, 0), (2, 0, 0)]
    log.written(present, p)
    log.change([(0, 0, 3)])
    assert log.stale(present, p) == [(0, 0, 3)]


def test_int16_wrap():
    log = ClearanceLog(0.25, (32, 32, 32))
    p = params_of(1.0)
    present = [(32767, 0, 0), (-32768, 0, 0), (0, 0, 0)]
    log.written(present, p)
    log.change([(-32768, 0, 0)])
    assert log.stale(present, p) == [(-32768, 0, 0), (32767, 0, 0)]


def test_params_removal_and_host_writes():
    log = ClearanceLog(0.25, (32, 32, 32))
    p, q = params_of(1.0), params_of(1.0, flags=1)
    present = [(0, 0, 0), (1, 0, 0), (3, 0, 0)]
    log.written(present, p)
    assert log.stale(present, q) == present
    assert params_of(1.0, flags=4) == p  # (flags that change no result)
    log.host_write([(3, 0, 0)])
    assert log.stale(present, p) == [(3, 0, 0)]
    log.written(present, p)
    log.remove([(2, 0, 0)])
    assert log.stale(present, p) == [(1, 0, 0), (3, 0, 0)]
