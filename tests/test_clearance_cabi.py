"""CPU: the clearance entry points of the C ABI are exported and bound, refuse null arguments with
OHMHIP_ERR_INVALID_ARG before any device work (so on a machine without a GPU too), stay out of the core ABI list, and
the Python mirrors exist with the reference's flag values."""
import ctypes as C
import os

import numpy as np

from ohm_amd import ClearanceProcess, LineQueryGpu, QueryFlag
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_clearance_regions", "ohmhip_map_clearance_regions_device", "ohmhip_map_clearance_keys")


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 5


def test_params_layout():
    assert C.sizeof(L.ClearanceParams) == 20
    assert L.ClearanceParams.flags.offset == 16


def test_null_arguments():
    keys = np.zeros((1, 3), dtype=np.int16)
    out = np.zeros(32 ** 3, dtype=np.float32)
    p = L.ClearanceParams()
    p.search_radius = 0.5
    for i in range(3):
        p.axis_scaling[i] = 1.0
    for name in NAMES:
        fn = getattr(L.lib, name)
        assert fn(None, keys.ctypes.data, 1, C.byref(p), out.ctypes.data) == L.ERR_INVALID_ARG
        assert fn(None, None, 0, None, None) == L.ERR_INVALID_ARG


def test_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    assert "#define OHMHIP_QF_UNKNOWN_AS_OCCUPIED (1u << 0)" in header
    assert "#define OHMHIP_QF_REPORT_UNSCALED (1u << 4)" in header


def test_query_flags_match_the_reference():
    """ohm/QueryFlag.h:37-53."""
    assert QueryFlag.kQfUnknownAsOccupied == 1
    assert QueryFlag.kQfNearestResult == 2
    assert QueryFlag.kQfGpuEvaluate == 4
    assert QueryFlag.kQfNoCache == 8
    assert QueryFlag.kQfReportUnscaledResults == 16
    assert ClearanceProcess.kQfInstantiateUnknown == 1 << 16


def test_mirror_accessors():
    cp = ClearanceProcess(1.5, QueryFlag.kQfUnknownAsOccupied)
    assert cp.searchRadius() == 1.5 and cp.queryFlags() == QueryFlag.kQfUnknownAsOccupied
    assert cp.axisScaling() == (1.0, 1.0, 1.0)
    cp.setAxisScaling((1, 2, 3))
    assert cp.axisScaling() == (1.0, 2.0, 3.0)
    assert cp.regionClearance((0, 0, 0)) is None
    lq = LineQueryGpu(None, (0, 0, 0), (1, 0, 0), 0.5, QueryFlag.kQfNearestResult)
    assert lq.defaultRange() == -1.0 and lq.queryFlags() & QueryFlag.kQfGpuEvaluate
    lq.setDefaultRange(2.5)
    assert lq.defaultRange() == 2.5 and lq.numberOfResults() == 0
