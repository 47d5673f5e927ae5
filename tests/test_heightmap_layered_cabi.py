"""CPU: the layered heightmap entry points of the C ABI are exported and bound, stay out of the core ABI list, and refuse
with the documented codes before any device work (a null map, so on a machine without a GPU too); the planar and the
flood-fill entry points still answer the layered modes as before."""
import ctypes as C
import os

import numpy as np
import pytest

from ohm_amd import HEIGHTMAP_VOXEL_DTYPE, Heightmap, HeightmapMode, LayeredHeightmap
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_heightmap_layered_extents", "ohmhip_map_heightmap_layered", "ohmhip_map_heightmap_layered_device")


def good_params(mode=3):
    p = L.HeightmapLayeredParams()
    p.base.grid_resolution = 0.1
    p.base.up_axis = 2
    p.base.mode = mode
    return p


def call(p, occupancy=True, voxels=True, stats=True, device=False, layer_capacity=2):
    occ = np.zeros(8, dtype=np.float32)
    vox = np.zeros(8, dtype=HEIGHTMAP_VOXEL_DTYPE)
    st = L.HeightmapLayeredStats()
    fn = L.lib.ohmhip_map_heightmap_layered_device if device else L.lib.ohmhip_map_heightmap_layered
    return fn(None, C.byref(p) if p is not None else None, layer_capacity, occ.ctypes.data if occupancy else None,
              vox.ctypes.data if voxels else None, None, None, None, None, 0, C.byref(st) if stats else None)


def extents(p):
    e = L.HeightmapExtents()
    return L.lib.ohmhip_map_heightmap_layered_extents(None, C.byref(p), C.byref(e))


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int
    assert len(L.lib.ohmhip_map_heightmap_layered_extents.argtypes) == 3
    assert len(L.lib.ohmhip_map_heightmap_layered.argtypes) == 11
    assert len(L.lib.ohmhip_map_heightmap_layered_device.argtypes) == 11


def test_struct_layouts():
    p = L.HeightmapLayeredParams
    assert C.sizeof(L.HeightmapParams) == 144 and L.HeightmapParams.mode.offset == 106  # the planar call's struct
    assert C.sizeof(p) == 152
    assert (p.base.offset, p.virtual_surface_filter_threshold.offset, p.reserved.offset) == (0, 144, 148)
    s = L.HeightmapLayeredStats
    assert C.sizeof(s) == 80
    assert (s.visits.offset, s.populated.offset, s.cells.offset, s.voxels.offset) == (0, 8, 16, 24)
    assert (s.repeats.offset, s.too_close.offset, s.filtered.offset, s.multi_layer_columns.offset) == (32, 40, 48, 56)
    assert (s.layers.offset, s.generations.offset, s.largest_generation.offset) == (64, 68, 72)


def test_null_and_invalid_arguments():
    for mode in (2, 3):
        p = good_params(mode)
        for device in (False, True):
            assert call(p, device=device) == L.ERR_INVALID_ARG  # null map
            assert call(None, device=device) == L.ERR_INVALID_ARG
            assert call(p, occupancy=False, device=device) == L.ERR_INVALID_ARG
            assert call(p, voxels=False, device=device) == L.ERR_INVALID_ARG
            assert call(p, stats=False, device=device) == L.ERR_INVALID_ARG
            assert call(p, layer_capacity=0, device=device) == L.ERR_INVALID_ARG
        assert extents(p) == L.ERR_INVALID_ARG
        assert L.lib.ohmhip_map_heightmap_layered_extents(None, C.byref(p), None) == L.ERR_INVALID_ARG
        p.reserved = 1
        assert call(p) == L.ERR_INVALID_ARG and call(p, device=True) == L.ERR_INVALID_ARG
        assert extents(p) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("field,value", [("grid_resolution", 0.0), ("grid_resolution", float("nan")),
                                         ("floor", -1.0), ("ceiling", float("inf")), ("min_clearance", -1e-9),
                                         ("min_clearance", -1.0), ("up_axis", 3), ("up_axis", -4)])
def test_invalid_parameters(field, value):
    p = good_params()
    setattr(p.base, field, value)
    assert call(p) == L.ERR_INVALID_ARG and call(p, device=True) == L.ERR_INVALID_ARG
    assert extents(p) == L.ERR_INVALID_ARG


def test_mode_codes():
    """Modes 0 and 1 have calls of their own; anything beyond 3 is not a mode; named before a map is looked at: with a
    supported mode the null map is the invalid argument."""
    for mode in (0, 1):
        p = good_params(mode)
        assert call(p) == L.ERR_INVALID_ARG and call(p, device=True) == L.ERR_INVALID_ARG
        assert extents(p) == L.ERR_INVALID_ARG
    for mode in (4, 5, 255):
        p = good_params(mode)
        assert call(p) == L.ERR_UNSUPPORTED and call(p, device=True) == L.ERR_UNSUPPORTED
        assert extents(p) == L.ERR_UNSUPPORTED


def test_planar_and_fill_entry_points_answer_as_before():
    occ = np.zeros(4, dtype=np.float32)
    vox = np.zeros(4, dtype=HEIGHTMAP_VOXEL_DTYPE)
    populated, cells = C.c_uint64(0), C.c_uint64(0)
    e = L.HeightmapExtents()
    st = L.HeightmapFillStats()
    want = {0: (L.ERR_INVALID_ARG, L.ERR_INVALID_ARG), 1: (L.ERR_UNSUPPORTED, L.ERR_INVALID_ARG),
            2: (L.ERR_UNSUPPORTED, L.ERR_UNSUPPORTED), 3: (L.ERR_UNSUPPORTED, L.ERR_UNSUPPORTED),
            4: (L.ERR_UNSUPPORTED, L.ERR_UNSUPPORTED)}  # (planar, fill); where the mode is theirs, the null map
    for mode, (planar, fill) in want.items():
        p = L.HeightmapParams()
        p.grid_resolution, p.up_axis, p.mode = 0.1, 2, mode
        assert L.lib.ohmhip_map_heightmap(None, C.byref(p), occ.ctypes.data, vox.ctypes.data, None, None,
                                          C.byref(populated), C.byref(cells)) == planar
        assert L.lib.ohmhip_map_heightmap_extents(None, C.byref(p), C.byref(e)) == planar
        assert L.lib.ohmhip_map_heightmap_device(None, C.byref(p), occ.ctypes.data, vox.ctypes.data, None, None,
                                                 None) == planar
        assert L.lib.ohmhip_map_heightmap_fill(None, C.byref(p), occ.ctypes.data, vox.ctypes.data, None, None, None, 0,
                                               C.byref(st)) == fill
        assert L.lib.ohmhip_map_heightmap_fill_device(None, C.byref(p), occ.ctypes.data, vox.ctypes.data, None, None,
                                                      None, 0, C.byref(st)) == fill
        assert L.lib.ohmhip_map_heightmap_fill_extents(None, C.byref(p), C.byref(e)) == fill


def test_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    assert "ohmhip_heightmap_layered_params;" in header and "ohmhip_heightmap_layered_stats;" in header
    for rule in ("L1 ", "L2 ", "L3 ", "L4 ", "L5 ", "L6 ", "L7 "):
        assert " *  " + rule in header


def test_mirror():
    hm = LayeredHeightmap(0.1, 0.0)
    assert hm.mode == HeightmapMode.kLayeredFill and hm.virtual_surface_filter_threshold == 0
    hm.virtual_surface_filter_threshold = 5
    p = hm.layered_params((0, 0, 0))
    assert (p.base.mode, p.virtual_surface_filter_threshold, p.reserved) == (3, 5, 0)
    hm.mode = HeightmapMode.kLayeredFillUnordered
    assert hm.layered_params((0, 0, 0)).base.mode == 2
    with pytest.raises(ValueError):
        hm.virtual_surface_filter_threshold = -1
    assert hm.build_heightmap((0, 0, 0)) is False  # no occupancy map set
    assert hm.occupancy is None and hm.layer_count is None and hm.layered_stats is None
    assert isinstance(hm, Heightmap) and Heightmap(0.1, 0.0).mode == HeightmapMode.kPlanar
