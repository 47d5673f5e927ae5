"""CPU: the ray pattern entry points of the C ABI are declared, exported and bound, stay out of the core ABI list, refuse
invalid arguments with OHMHIP_ERR_INVALID_ARG before any device work, and report a missing device instead of faking one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ohm_amd
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_pattern_create", "ohmhip_pattern_destroy", "ohmhip_pattern_ray_count", "ohmhip_pattern_build_rays",
         "ohmhip_pattern_last_rays", "ohmhip_map_apply_pattern")


def _header():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        return fh.read()


def test_symbols_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = C.CDLL(ohm_amd.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int
    assert len(L.lib.ohmhip_pattern_create.argtypes) == 3
    assert len(L.lib.ohmhip_pattern_build_rays.argtypes) == 6
    assert len(L.lib.ohmhip_pattern_last_rays.argtypes) == 3
    assert len(L.lib.ohmhip_map_apply_pattern.argtypes) == 9
    assert "#define OHMHIP_POSE_QUAT 0" in header and "#define OHMHIP_POSE_MAT4 1" in header
    for name in ("RayPattern", "RayPatternConical", "ClearingPattern"):
        assert hasattr(ohm_amd, name)
    from ohm_amd import raypattern
    assert (raypattern.POSE_QUAT, raypattern.POSE_MAT4) == (0, 1)


def test_not_in_the_core_abi():
    header = _header()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    assert not any(n.startswith("ohmhip_pattern_") for n in core)


def test_null_and_range_errors():
    """Checked before anything touches a device: the same with and without a GPU."""
    invalid = L.ERR_INVALID_ARG
    pairs = np.zeros((2, 6), dtype=np.float64)
    poses = np.zeros((1, 7), dtype=np.float64)
    handle = L._vp()
    n = C.c_size_t(5)
    assert L.lib.ohmhip_pattern_create(pairs.ctypes.data, 2, None) == invalid
    assert L.lib.ohmhip_pattern_create(None, 2, C.byref(handle)) == invalid and not handle
    assert L.lib.ohmhip_pattern_create(pairs.ctypes.data, 1 << 28, C.byref(handle)) == L.ERR_CAPACITY and not handle
    assert L.lib.ohmhip_pattern_ray_count(None, C.byref(n)) == invalid
    assert L.lib.ohmhip_pattern_build_rays(None, poses.ctypes.data, 1, 0, 1.0, None) == invalid
    assert L.lib.ohmhip_pattern_last_rays(None, None, C.byref(n)) == invalid and n.value == 0
    assert L.lib.ohmhip_pattern_destroy(None) == L.OK            # like free(NULL) and ohmhip_map_destroy(NULL)
    done = C.c_size_t(9)
    assert L.lib.ohmhip_map_apply_pattern(None, None, poses.ctypes.data, 1, 0, 1.0, 1.0, 0, C.byref(done)) == invalid
    assert done.value == 0
    assert L.lib.ohmhip_map_apply_pattern(None, None, None, 0, 2, 1.0, 1.0, 0, None) == invalid


def test_no_device_is_reported_not_faked():
    """Without a GPU a pattern cannot be made resident: OHMHIP_ERR_NO_DEVICE, and the mirror raises -- nothing is
    computed on the host instead."""
    if ohm_amd.device_count() > 0:
        pytest.skip("a GPU is present")
    pairs = np.zeros((2, 6), dtype=np.float64)
    handle = L._vp()
    assert L.lib.ohmhip_pattern_create(pairs.ctypes.data, 2, C.byref(handle)) == L.ERR_NO_DEVICE and not handle
    assert L.lib.ohmhip_pattern_create(None, 0, C.byref(handle)) == L.ERR_NO_DEVICE and not handle
    pattern = ohm_amd.RayPattern()
    pattern.addPoint((0.0, 1.0, 0.0))
    with pytest.raises(ohm_amd.OhmHipError) as err:
        pattern.buildRays((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    assert err.value.status == L.ERR_NO_DEVICE
