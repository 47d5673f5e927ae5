"""CPU: the heightmap entry points of the C ABI are exported and bound, stay out of the core ABI list, and refuse
invalid arguments with OHMHIP_ERR_INVALID_ARG / OHMHIP_ERR_UNSUPPORTED before any device work (so on a machine without
a GPU too); the Python mirror exists with the reference's enumerations and the HeightmapVoxel layout."""
import ctypes as C
import os

import numpy as np
import pytest

from ohm_amd import HEIGHTMAP_VOXEL_DTYPE, Heightmap, HeightmapMode, HeightmapVoxelType, UpAxis
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_heightmap_extents", "ohmhip_map_heightmap", "ohmhip_map_heightmap_device")


def good_params():
    p = L.HeightmapParams()
    p.grid_resolution = 0.1
    p.up_axis = 2
    return p


def call(p, occupancy=True, voxels=True, counts=True, map_=None):
    occ = np.zeros(4, dtype=np.float32)
    vox = np.zeros(4, dtype=HEIGHTMAP_VOXEL_DTYPE)
    populated, cells = C.c_uint64(7), C.c_uint64(7)
    return L.lib.ohmhip_map_heightmap(map_, C.byref(p) if p is not None else None,
                                      occ.ctypes.data if occupancy else None, vox.ctypes.data if voxels else None,
                                      None, None, C.byref(populated) if counts else None,
                                      C.byref(cells) if counts else None)


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int
    assert len(L.lib.ohmhip_map_heightmap_extents.argtypes) == 3
    assert len(L.lib.ohmhip_map_heightmap.argtypes) == 8
    assert len(L.lib.ohmhip_map_heightmap_device.argtypes) == 7


def test_struct_layouts():
    assert C.sizeof(L.HeightmapParams) == 144
    assert L.HeightmapParams.grid_resolution.offset == 72
    assert L.HeightmapParams.region_size.offset == 104 and L.HeightmapParams.up_axis.offset == 105
    assert L.HeightmapParams.mode.offset == 106 and L.HeightmapParams.floor.offset == 112
    assert L.HeightmapParams.flags.offset == 136
    assert C.sizeof(L.HeightmapExtents) == 44
    assert L.HeightmapExtents.max_region.offset == 10 and L.HeightmapExtents.na.offset == 20
    assert L.HeightmapExtents.ma.offset == 36
    assert HEIGHTMAP_VOXEL_DTYPE.itemsize == 24  # ohmheightmap/HeightmapVoxel.h:68-97
    assert HEIGHTMAP_VOXEL_DTYPE.fields["layer"][1] == 20 and HEIGHTMAP_VOXEL_DTYPE.fields["flags"][1] == 21
    assert HEIGHTMAP_VOXEL_DTYPE.fields["contributing_samples"][1] == 22


def test_null_arguments():
    p = good_params()
    assert call(p) == L.ERR_INVALID_ARG  # null map
    assert call(None) == L.ERR_INVALID_ARG
    assert call(p, occupancy=False) == L.ERR_INVALID_ARG
    assert call(p, voxels=False) == L.ERR_INVALID_ARG
    assert call(p, counts=False) == L.ERR_INVALID_ARG
    e = L.HeightmapExtents()
    assert L.lib.ohmhip_map_heightmap_extents(None, C.byref(p), C.byref(e)) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_heightmap_extents(None, C.byref(p), None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_map_heightmap_device(None, C.byref(p), None, None, None, None, None) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("field,value", [("grid_resolution", 0.0), ("grid_resolution", -0.1),
                                         ("grid_resolution", float("nan")), ("grid_resolution", float("inf")),
                                         ("floor", -1.0), ("floor", float("nan")), ("ceiling", -0.5),
                                         ("ceiling", float("inf")), ("min_clearance", -1e-9),
                                         ("min_clearance", float("nan")), ("up_axis", 3), ("up_axis", -4)])
def test_invalid_parameters(field, value):
    p = good_params()
    setattr(p, field, value)
    assert call(p) == L.ERR_INVALID_ARG
    e = L.HeightmapExtents()
    assert L.lib.ohmhip_map_heightmap_extents(None, C.byref(p), C.byref(e)) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_flood_fill_modes_are_unsupported(mode):
    """The refusal names the mode even before a map is looked at: nothing of the device is touched."""
    p = good_params()
    p.mode = mode
    assert call(p) == L.ERR_UNSUPPORTED
    e = L.HeightmapExtents()
    assert L.lib.ohmhip_map_heightmap_extents(None, C.byref(p), C.byref(e)) == L.ERR_UNSUPPORTED
    occ = np.zeros(4, dtype=np.float32)
    assert L.lib.ohmhip_map_heightmap_device(None, C.byref(p), occ.ctypes.data, occ.ctypes.data, None, None,
                                             None) == L.ERR_UNSUPPORTED


def test_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    assert "#define OHMHIP_HM_GENERATE_VIRTUAL_SURFACE (1u << 0)" in header
    assert "#define OHMHIP_HM_PROMOTE_VIRTUAL_BELOW (1u << 1)" in header
    assert "#define OHMHIP_HM_IGNORE_VOXEL_MEAN (1u << 2)" in header


def test_enumerations_match_the_reference():
    """ohmheightmap/UpAxis.h, HeightmapVoxelType.h, HeightmapMode.h."""
    assert [int(v) for v in (UpAxis.kNegZ, UpAxis.kNegY, UpAxis.kNegX, UpAxis.kX, UpAxis.kY, UpAxis.kZ)] == \
        [-3, -2, -1, 0, 1, 2]
    assert [int(v) for v in (HeightmapVoxelType.kUnknown, HeightmapVoxelType.kVacant, HeightmapVoxelType.kSurface,
                             HeightmapVoxelType.kVirtualSurface)] == [0, 1, 2, 3]
    assert int(HeightmapMode.kPlanar) == 0 and int(HeightmapMode.kLayeredFill) == 3


def test_mirror_parameters():
    hm = Heightmap(0.2, 0.5, UpAxis.kNegY, region_size=16)
    hm.ceiling, hm.floor = 1.5, 0.75
    hm.generate_virtual_surface = True
    hm.ignore_voxel_mean = True
    hm.heightmap_origin = (1.0, 2.0, 3.0)
    p = hm.params((4.0, 5.0, 6.0), ((-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)))
    assert (p.grid_resolution, p.min_clearance, p.up_axis, p.region_size, p.mode) == (0.2, 0.5, -2, 16, 0)
    assert (p.ceiling, p.floor) == (1.5, 0.75)
    assert p.flags == L.HM_GENERATE_VIRTUAL_SURFACE | L.HM_IGNORE_VOXEL_MEAN
    assert list(p.reference_pos) == [4.0, 5.0, 6.0] and list(p.origin) == [1.0, 2.0, 3.0]
    assert list(p.cull_min) == [-1.0, -2.0, -3.0] and list(p.cull_max) == [1.0, 2.0, 3.0]
    assert hm.up_axis_index() == 1 and hm.up_axis_normal() == (0.0, -1.0, 0.0)
    assert hm.surface_axis_indices() == (0, 2)
    assert Heightmap(0.1, 0.0).params((0, 0, 0)).region_size == 0  # the default: Heightmap::kDefaultRegionSize
    assert hm.build_heightmap((0, 0, 0)) is False  # no occupancy map set (Heightmap.cpp:337-340)
    assert hm.get_heightmap_voxel_info(((0, 0, 0), (0, 0, 0)))[0] == HeightmapVoxelType.kUnknown
