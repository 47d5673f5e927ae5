"""CPU: the point cloud entry points of the C ABI are exported and bound, stay out of the core ABI list, and refuse
invalid arguments with OHMHIP_ERR_INVALID_ARG before any device work (so on a machine without a GPU too); the params
struct has the header's layout and the Python mirror maps its arguments onto it."""
import ctypes as C
import os

import numpy as np
import pytest

import ohm_amd
from ohm_amd import CLOUD_CHUNK_VOXELS, GPU_KEY_DTYPE, CloudMode, VoxelCloud, cloud_params
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_cloud_count", "ohmhip_map_cloud", "ohmhip_map_cloud_device")


def good_params():
    p = L.CloudParams()
    p.surface_distance = 0.1
    return p


def calls(p, map_=None, count=True, capacity=4, positions=True):
    """The status of each of the three entry points for the same request."""
    pos = np.zeros((4, 3), dtype=np.float64)
    n = C.c_uint64(7)
    ref = C.byref(p) if p is not None else None
    cnt = C.byref(n) if count else None
    ptr = pos.ctypes.data if positions else None
    return (L.lib.ohmhip_map_cloud_count(map_, ref, cnt),
            L.lib.ohmhip_map_cloud(map_, ref, capacity, ptr, None, None, cnt),
            L.lib.ohmhip_map_cloud_device(map_, ref, capacity, ptr, None, None, C.addressof(n) if count else None))


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int
    assert len(L.lib.ohmhip_map_cloud_count.argtypes) == 3
    assert len(L.lib.ohmhip_map_cloud.argtypes) == 7
    assert len(L.lib.ohmhip_map_cloud_device.argtypes) == 7
    for name in ("CloudMode", "VoxelCloud", "extract_cloud", "save_cloud", "save_density_cloud", "save_tsdf_cloud",
                 "save_clearance_cloud"):
        assert hasattr(ohm_amd, name)


def test_struct_layout():
    """ohmhip_cloud_params: 6 doubles, 3 floats, int32, uint32, uint8, padded to the doubles' alignment."""
    assert C.sizeof(L.CloudParams) == 72
    assert L.CloudParams.min_extents.offset == 0 and L.CloudParams.max_extents.offset == 24
    assert L.CloudParams.density_threshold.offset == 48 and L.CloudParams.surface_distance.offset == 52
    assert L.CloudParams.colour_range.offset == 56 and L.CloudParams.export_type.offset == 60
    assert L.CloudParams.flags.offset == 64 and L.CloudParams.mode.offset == 68
    assert GPU_KEY_DTYPE.itemsize == 10 and GPU_KEY_DTYPE.fields["voxel"][1] == 6  # ohmgpu/GpuKey.h:37-46


def test_header_declares_what_is_bound():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    for line in ("#define OHMHIP_CLOUD_OCCUPANCY 0", "#define OHMHIP_CLOUD_DENSITY 1", "#define OHMHIP_CLOUD_TSDF 2",
                 "#define OHMHIP_CLOUD_CLEARANCE 3", "#define OHMHIP_CLOUD_EXPORT_FREE (1u << 0)",
                 "#define OHMHIP_CLOUD_IGNORE_VOXEL_MEAN (1u << 1)", "#define OHMHIP_CLOUD_USE_EXTENTS (1u << 2)",
                 "#define OHMHIP_CLOUD_CHUNK_VOXELS %d" % CLOUD_CHUNK_VOXELS):
        assert line in header, line
    assert [int(m) for m in (CloudMode.OCCUPANCY, CloudMode.DENSITY, CloudMode.TSDF, CloudMode.CLEARANCE)] == [0, 1, 2, 3]
    assert (L.CLOUD_EXPORT_FREE, L.CLOUD_IGNORE_VOXEL_MEAN, L.CLOUD_USE_EXTENTS) == (1, 2, 4)
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_cloud_device(" in header


def test_null_arguments():
    p = good_params()
    assert calls(p) == (L.ERR_INVALID_ARG,) * 3  # null map
    assert calls(None) == (L.ERR_INVALID_ARG,) * 3
    assert calls(p, count=False) == (L.ERR_INVALID_ARG,) * 3
    assert calls(p, positions=False)[1:] == (L.ERR_INVALID_ARG,) * 2  # capacity > 0 with null positions


@pytest.mark.parametrize("field,value", [("mode", 4), ("mode", 255), ("flags", 8), ("flags", 0x80000001),
                                         ("density_threshold", float("nan")), ("surface_distance", float("nan")),
                                         ("colour_range", float("nan"))])
def test_invalid_parameters(field, value):
    p = good_params()
    setattr(p, field, value)
    assert calls(p) == (L.ERR_INVALID_ARG,) * 3


@pytest.mark.parametrize("which,index,value", [("min_extents", 0, float("nan")), ("min_extents", 2, float("inf")),
                                               ("max_extents", 1, float("-inf")), ("max_extents", 2, float("nan"))])
def test_non_finite_extents(which, index, value):
    p = good_params()
    p.flags = L.CLOUD_USE_EXTENTS
    getattr(p, which)[index] = value
    assert calls(p) == (L.ERR_INVALID_ARG,) * 3


def test_mirror_parameters():
    p = cloud_params(CloudMode.CLEARANCE, colour_range=2.5, export_type=-1,
                     extents=((-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)))
    assert (p.mode, p.flags, p.colour_range, p.export_type) == (3, L.CLOUD_USE_EXTENTS, 2.5, -1)
    assert list(p.min_extents) == [-1.0, -2.0, -3.0] and list(p.max_extents) == [1.0, 2.0, 3.0]
    p = cloud_params(CloudMode.OCCUPANCY, export_free=True, ignore_voxel_mean=True)
    assert (p.mode, p.flags) == (0, L.CLOUD_EXPORT_FREE | L.CLOUD_IGNORE_VOXEL_MEAN)
    p = cloud_params(CloudMode.DENSITY, density_threshold=0.25)
    assert (p.mode, p.flags, p.density_threshold) == (1, 0, 0.25)
    p = cloud_params(CloudMode.TSDF, surface_distance=0.125)
    assert (p.mode, p.surface_distance) == (2, 0.125)
    assert cloud_params().surface_distance == float("inf") and cloud_params().mode == 0
    cloud = VoxelCloud(np.zeros((2, 3)), np.zeros(2, dtype=GPU_KEY_DTYPE), np.zeros(2, dtype=np.float32), 5)
    assert len(cloud) == 2 and cloud.count == 5 and cloud.mode == CloudMode.OCCUPANCY
