"""CPU: the RaysQuery entry points of the C ABI are exported and bound, refuse null or inconsistent arguments with
OHMHIP_ERR_INVALID_ARG before any device work (so on a machine without a GPU too), and stay out of the core ABI list
(the binding core does not call them)."""
import ctypes as C
import os

import numpy as np

from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_rays_query", "ohmhip_map_rays_query_device")


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        fn = getattr(L.lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 8


def test_null_and_invalid_arguments():
    rays = np.zeros((4, 3))
    out_d = np.zeros(2)
    out_v = np.zeros(2)
    out_t = np.zeros(2, dtype=np.int8)
    for name in NAMES:
        fn = getattr(L.lib, name)
        # no map
        assert fn(None, rays.ctypes.data, 4, 1.0, out_d.ctypes.data, out_v.ctypes.data, out_t.ctypes.data,
                  None) == L.ERR_INVALID_ARG
        assert fn(None, None, 0, 1.0, None, None, None, None) == L.ERR_INVALID_ARG


def test_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
