"""CPU: the voxel-edit entry points of the C ABI (ohmhip_map_write_voxels / _device, ohmhip_map_integrate_voxels /
_device) are exported, declared and bound, stay out of the core ABI list, and refuse invalid arguments with
OHMHIP_ERR_INVALID_ARG before any device work -- so the refusals run without a GPU; the stats record's layout; the
Python and C++ mirrors declare the interface.  (tests/test_gpu_voxel_edit.py repeats the refusals against a live map.)"""
import ctypes as C
import os

import numpy as np

import cpp_driver
import ohm_amd
from ohm_amd import GPU_KEY_DTYPE, GpuMap, VoxelEdit
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_write_voxels", "ohmhip_map_write_voxels_device", "ohmhip_map_integrate_voxels",
         "ohmhip_map_integrate_voxels_device")


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
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_write_voxels_device(" in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_integrate_voxels_device(" in header
    assert "OHMHIP_LID_COUNT = 10" in header  # no new layer
    for line in ("#define OHMHIP_EDIT_HIT 1", "#define OHMHIP_EDIT_MISS 2", "#define OHMHIP_EDIT_HIT_SAMPLE 3"):
        assert line in header
    for rule in range(1, 10):
        assert " E%d " % rule in header


def test_stats_layout():
    assert C.sizeof(L.VoxelEditStats) == 40
    fields = ("applied", "null_keys", "distinct_voxels", "regions_touched", "regions_created")
    assert [name for name, _ in L.VoxelEditStats._fields_] == list(fields)
    assert [getattr(L.VoxelEditStats, name).offset for name in fields] == [0, 8, 16, 24, 32]
    assert (L.EDIT_HIT, L.EDIT_MISS, L.EDIT_HIT_SAMPLE) == (1, 2, 3)
    assert (int(VoxelEdit.kHit), int(VoxelEdit.kMiss), int(VoxelEdit.kHitSample)) == (1, 2, 3)


def test_refusals_without_a_map():
    keys = np.zeros(2, dtype=GPU_KEY_DTYPE)
    values = np.zeros(2, dtype=np.float32)
    points = np.zeros((2, 3))
    ops = np.array([1, 2], dtype=np.uint8)
    stats = L.VoxelEditStats(1, 2, 3, 4, 5)
    k, v, p, o = keys.ctypes.data, values.ctypes.data, points.ctypes.data, ops.ctypes.data
    for fn in (L.lib.ohmhip_map_write_voxels, L.lib.ohmhip_map_write_voxels_device):
        assert fn(None, 0, k, 2, v, C.byref(stats)) == L.ERR_INVALID_ARG  # null map
        assert stats.applied == 0 and stats.regions_created == 0              # (the stats are zeroed all the same)
        assert fn(None, 0, k, 2, v, None) == L.ERR_INVALID_ARG
        assert fn(None, -1, k, 2, v, None) == L.ERR_INVALID_ARG
        assert fn(None, L.LID_COUNT, k, 2, v, None) == L.ERR_INVALID_ARG
        assert fn(None, 0, None, 2, v, None) == L.ERR_INVALID_ARG
        assert fn(None, 0, k, 2, None, None) == L.ERR_INVALID_ARG
        assert fn(None, 0, k, 0x80000000, v, None) == L.ERR_INVALID_ARG
        assert fn(None, 0, None, 0, None, None) == L.ERR_INVALID_ARG
    for fn in (L.lib.ohmhip_map_integrate_voxels, L.lib.ohmhip_map_integrate_voxels_device):
        assert fn(None, None, 1, k, None, 2, None) == L.ERR_INVALID_ARG      # null map
        assert fn(None, o, 0, k, None, 2, None) == L.ERR_INVALID_ARG
        assert fn(None, None, 1, k, p, 2, None) == L.ERR_INVALID_ARG         # both
        assert fn(None, None, 1, None, None, 2, None) == L.ERR_INVALID_ARG   # neither
        assert fn(None, None, 0, k, None, 2, None) == L.ERR_INVALID_ARG      # op outside 1 .. 3
        assert fn(None, None, 4, None, p, 2, None) == L.ERR_INVALID_ARG
        assert fn(None, None, 3, k, None, 2, None) == L.ERR_INVALID_ARG      # HIT_SAMPLE needs points
        assert fn(None, None, 1, k, None, 0x80000000, None) == L.ERR_INVALID_ARG
        assert fn(None, None, 1, None, None, 0, None) == L.ERR_INVALID_ARG


def test_mirrors():
    for name in ("writeVoxels", "integrateHits", "integrateMisses", "integrateVoxels", "lastEditStats", "keyRange"):
        assert callable(getattr(GpuMap, name))
    assert ohm_amd.VoxelEdit is VoxelEdit and callable(ohm_amd.key_range)


def test_cpp_mirror_declares_the_same_interface():
    text = cpp_driver.host_mirror_text()
    for token in ("writeVoxels(", "integrateVoxels(", "integrateHits(", "integrateMisses(", "integrateHit(",
                  "integrateMiss(", "lastEditStats(", "keyRange(", "enum class VoxelEdit"):
        assert token in text, token
