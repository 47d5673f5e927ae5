"""CPU: ohmhip_map_can_copy / ohmhip_map_copy are exported, declared and bound, stay out of the core ABI list, the two
structs have the header's layout, and the refusals that need no live map are made before any device work (so on a
machine without a GPU too)."""
import ctypes as C
import os

import numpy as np
import pytest

import ohm_amd
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_can_copy", "ohmhip_map_copy")


def _header():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        return fh.read()


def test_symbols_exported_and_bound():
    raw = C.CDLL(ohm_amd.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name)
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int
    assert len(L.lib.ohmhip_map_can_copy.argtypes) == 2 and len(L.lib.ohmhip_map_copy.argtypes) == 4
    for name in ("canCopy", "copyMap", "copyFilterExtents", "copyFilterDirty", "copyFilterAnd", "copyFilterOr",
                 "copyFilterNegate", "copyLayersFilter"):
        assert hasattr(ohm_amd, name)
    assert hasattr(ohm_amd.GpuMap, "clone")


def test_header_declares_what_is_bound():
    header = _header()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert "int " + name + "(" in header
        assert "OHMHIP_EXPERIMENTAL int " + name not in header
    assert "/* MAP COPY." in header
    assert "OHMHIP_LID_COUNT = 10" in header
    assert "#define OHMHIP_COPY_DIRTY_ONLY (1u << 0)" in header and "#define OHMHIP_COPY_USE_EXTENTS (1u << 1)" in header
    assert (L.COPY_DIRTY_ONLY, L.COPY_USE_EXTENTS) == (1, 2)
    assert L.LID_COUNT == 10


def test_struct_layout():
    """ohmhip_copy_params: two unsigned, six doubles, a pointer, a size_t; ohmhip_copy_stats: four uint64, one unsigned,
    padded to the uint64s' alignment."""
    P, S = L.CopyParams, L.CopyStats
    assert C.sizeof(P) == 72
    assert (P.flags.offset, P.layers.offset, P.min_extents.offset, P.max_extents.offset, P.keys_xyz.offset,
            P.key_count.offset) == (0, 4, 8, 32, 56, 64)
    assert C.sizeof(S) == 40
    assert (S.regions_passed.offset, S.regions_created.offset, S.keys_absent.offset, S.bytes_copied.offset,
            S.layers_copied.offset) == (0, 8, 16, 24, 32)


def _copy(params, dst=None, src=None):
    stats = L.CopyStats()
    stats.regions_passed = 77  # (the call zeroes the stats before it refuses)
    status = L.lib.ohmhip_map_copy(dst, src, None if params is None else C.byref(params), C.byref(stats))
    assert stats.regions_passed == 0 and stats.bytes_copied == 0
    return status


def test_null_maps():
    assert L.lib.ohmhip_map_can_copy(None, None) == L.ERR_INVALID_ARG
    assert _copy(None) == L.ERR_INVALID_ARG
    assert _copy(L.CopyParams()) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_copy(None, None, None, None) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("flags", [4, 8, 0x80000000, 0xfffffffc, 7])
def test_unknown_flag_bits(flags):
    p = L.CopyParams()
    p.flags = flags
    assert _copy(p) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("layers", [1 << 10, 1 << 31, 0xffffffff, (1 << 10) | 1])
def test_layer_mask_beyond_the_layer_ids(layers):
    p = L.CopyParams()
    p.layers = layers
    assert _copy(p) == L.ERR_INVALID_ARG


def test_keys_and_count_must_agree():
    keys = np.zeros((2, 3), dtype=np.int16)
    p = L.CopyParams()
    p.keys_xyz = keys.ctypes.data
    p.key_count = 0
    assert _copy(p) == L.ERR_INVALID_ARG
    p = L.CopyParams()
    p.keys_xyz = None
    p.key_count = 2
    assert _copy(p) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("which,index", [("min_extents", 0), ("min_extents", 2), ("max_extents", 1)])
def test_nan_extents(which, index):
    p = L.CopyParams()
    p.flags = L.COPY_USE_EXTENTS
    for a in range(3):
        p.min_extents[a], p.max_extents[a] = -float("inf"), float("inf")
    getattr(p, which)[index] = float("nan")
    assert _copy(p) == L.ERR_INVALID_ARG


def test_mirror_without_a_device():
    """copyutil's filters are plain host objects: they are built and combined without a map."""
    from ohm_amd import copyutil as U
    f = U.copyFilterAnd(U.copyFilterExtents((0, 0, 0), (1, 1, 1)), None)
    assert f.min_ext == (0.0, 0.0, 0.0) and f.max_ext == (1.0, 1.0, 1.0)
    assert U.copyFilterNegate(None)(None) is False
