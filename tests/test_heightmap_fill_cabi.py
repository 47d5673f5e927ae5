"""CPU: the flood-fill heightmap entry points of the C ABI are exported and bound, stay out of the core ABI list, and
refuse with the documented codes before any device work (a null map, so on a machine without a GPU too); the planar
entry points still refuse mode 1."""
import ctypes as C
import os

import numpy as np
import pytest

from ohm_amd import HEIGHTMAP_VOXEL_DTYPE, Heightmap, HeightmapMode
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_heightmap_fill_extents", "ohmhip_map_heightmap_fill", "ohmhip_map_heightmap_fill_device")


def good_params(mode=1):
    p = L.HeightmapParams()
    p.grid_resolution = 0.1
    p.up_axis = 2
    p.mode = mode
    return p


def call(p, occupancy=True, voxels=True, stats=True, device=False):
    occ = np.zeros(4, dtype=np.float32)
    vox = np.zeros(4, dtype=HEIGHTMAP_VOXEL_DTYPE)
    st = L.HeightmapFillStats()
    fn = L.lib.ohmhip_map_heightmap_fill_device if device else L.lib.ohmhip_map_heightmap_fill
    return fn(None, C.byref(p) if p is not None else None, occ.ctypes.data if occupancy else None,
              vox.ctypes.data if voxels else None, None, None, None, 0, C.byref(st) if stats else None)


def extents(p):
    e = L.HeightmapExtents()
    return L.lib.ohmhip_map_heightmap_fill_extents(None, C.byref(p), C.byref(e))


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int
    assert len(L.lib.ohmhip_map_heightmap_fill_extents.argtypes) == 3
    assert len(L.lib.ohmhip_map_heightmap_fill.argtypes) == 9
    assert len(L.lib.ohmhip_map_heightmap_fill_device.argtypes) == 9


def test_struct_layout():
    assert C.sizeof(L.HeightmapFillStats) == 40
    s = L.HeightmapFillStats
    assert (s.visits.offset, s.populated.offset, s.cells.offset, s.revisits.offset) == (0, 8, 16, 24)
    assert (s.generations.offset, s.largest_generation.offset) == (32, 36)
    assert C.sizeof(L.HeightmapParams) == 144 and L.HeightmapParams.mode.offset == 106  # the planar call's struct


def test_null_arguments():
    p = good_params()
    for device in (False, True):
        assert call(p, device=device) == L.ERR_INVALID_ARG  # null map
        assert call(None, device=device) == L.ERR_INVALID_ARG
        assert call(p, occupancy=False, device=device) == L.ERR_INVALID_ARG
        assert call(p, voxels=False, device=device) == L.ERR_INVALID_ARG
        assert call(p, stats=False, device=device) == L.ERR_INVALID_ARG
    assert extents(p) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_heightmap_fill_extents(None, C.byref(p), None) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("field,value", [("grid_resolution", 0.0), ("grid_resolution", float("nan")),
                                         ("floor", -1.0), ("ceiling", float("inf")), ("min_clearance", -1e-9),
                                         ("up_axis", 3), ("up_axis", -4)])
def test_invalid_parameters(field, value):
    p = good_params()
    setattr(p, field, value)
    assert call(p) == L.ERR_INVALID_ARG and call(p, device=True) == L.ERR_INVALID_ARG
    assert extents(p) == L.ERR_INVALID_ARG


def test_mode_codes():
    """mode 0 belongs to the planar call; the layered fills are not provided; named before a map is looked at."""
    p = good_params(0)
    assert call(p) == L.ERR_INVALID_ARG and call(p, device=True) == L.ERR_INVALID_ARG
    assert extents(p) == L.ERR_INVALID_ARG
    for mode in (2, 3, 4):
        p = good_params(mode)
        assert call(p) == L.ERR_UNSUPPORTED and call(p, device=True) == L.ERR_UNSUPPORTED
        assert extents(p) == L.ERR_UNSUPPORTED


def test_planar_entry_points_still_refuse_the_fill_mode():
    p = good_params(1)
    occ = np.zeros(4, dtype=np.float32)
    vox = np.zeros(4, dtype=HEIGHTMAP_VOXEL_DTYPE)
    populated, cells = C.c_uint64(0), C.c_uint64(0)
    assert L.lib.ohmhip_map_heightmap(None, C.byref(p), occ.ctypes.data, vox.ctypes.data, None, None,
                                      C.byref(populated), C.byref(cells)) == L.ERR_UNSUPPORTED
    e = L.HeightmapExtents()
    assert L.lib.ohmhip_map_heightmap_extents(None, C.byref(p), C.byref(e)) == L.ERR_UNSUPPORTED
    assert L.lib.ohmhip_map_heightmap_device(None, C.byref(p), occ.ctypes.data, vox.ctypes.data, None, None,
                                             None) == L.ERR_UNSUPPORTED


def test_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    assert "ohmhip_heightmap_fill_stats;" in header


def test_mirror():
    hm = Heightmap(0.1, 0.0)
    hm.mode = HeightmapMode.kSimpleFill
    assert hm.params((0, 0, 0)).mode == 1
    assert hm.build_heightmap((0, 0, 0)) is False  # no occupancy map set
    assert hm.source_visit is None and hm.visit_log is None and hm.fill_stats is None
