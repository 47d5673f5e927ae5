"""CPU: the ray-filter chain entry points of the C ABI are declared, exported and bound and stay out of the core ABI
list; the stage record of ohm_amd/_lib.py has the header's size and offsets (a C program compiled against the header
prints them); the constants match; invalid arguments are refused with OHMHIP_ERR_INVALID_ARG before any device work.
(tests/test_gpu_rayfilter_chain.py repeats the refusals against a live map.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import cpp_driver
import ohm_amd
from ohm_amd import GpuMap
from ohm_amd import _lib as L
from ohm_amd import rayfilter as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_set_ray_filter_stages", "ohmhip_map_ray_filter_stages", "ohmhip_map_apply_ray_filter",
         "ohmhip_map_apply_ray_filter_device")


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
    assert len(L.lib.ohmhip_map_set_ray_filter_stages.argtypes) == 3
    assert len(L.lib.ohmhip_map_ray_filter_stages.argtypes) == 4
    assert len(L.lib.ohmhip_map_apply_ray_filter.argtypes) == 6
    assert len(L.lib.ohmhip_map_apply_ray_filter_device.argtypes) == 6


def test_not_in_the_core_abi_and_nothing_pinned_moved():
    header = _header()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    assert "OHMHIP_LID_COUNT = 10" in header  # no new layer, and ohmhip_map_config is as it was:
    assert C.sizeof(L.MapConfig) == 152


def test_constants():
    header = _header()
    for name, value in (("OHMHIP_RFS_GOOD", 1), ("OHMHIP_RFS_CLIP", 2), ("OHMHIP_RFS_CLIP_BOUNDED", 3),
                        ("OHMHIP_RFS_CLIP_TO_BOUNDS", 4)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    assert "#define OHMHIP_MAX_RAY_FILTER_STAGES 4" in header
    assert (L.RFS_GOOD, L.RFS_CLIP, L.RFS_CLIP_BOUNDED, L.RFS_CLIP_TO_BOUNDS) == (1, 2, 3, 4)
    assert L.MAX_RAY_FILTER_STAGES == 4
    assert (RF.kStageGood, RF.kStageClip, RF.kStageClipBounded, RF.kStageClipToBounds, RF.kMaxStages) == (1, 2, 3, 4, 4)
    assert (RF.kRffInvalid, RF.kRffClippedStart, RF.kRffClippedEnd) == (1, 2, 4)


def test_stage_layout_matches_the_header(tmp_path):
    fields = ("kind", "reserved", "range", "box_min", "box_max")
    src = tmp_path / "layout.c"
    src.write_text('#include <ohmhip.h>\n#include <stddef.h>\n#include <stdio.h>\nint main(void)\n{\n'
                   '  printf("%zu", sizeof(ohmhip_ray_filter_stage));\n' +
                   "".join('  printf(" %%zu", offsetof(ohmhip_ray_filter_stage, %s));\n' % f for f in fields) +
                   '  printf(" %d\\n", OHMHIP_MAX_RAY_FILTER_STAGES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    numbers = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert numbers[0] == C.sizeof(L.RayFilterStage) == 64
    assert numbers[1:6] == [getattr(L.RayFilterStage, f).offset for f in fields] == [0, 4, 8, 16, 40]
    assert numbers[6] == L.MAX_RAY_FILTER_STAGES
    assert [name for name, _ in L.RayFilterStage._fields_] == list(fields)


def test_refusals_without_a_map():
    """Checked before anything touches a device: the same with and without a GPU."""
    invalid = L.ERR_INVALID_ARG
    stages = (L.RayFilterStage * 5)()
    for st in stages:
        st.kind = L.RFS_GOOD
    set_stages = L.lib.ohmhip_map_set_ray_filter_stages
    assert set_stages(None, stages, 1) == invalid            # null map
    assert set_stages(None, None, 0) == invalid
    assert set_stages(None, None, 1) == invalid              # null stages with a count
    assert set_stages(None, stages, 5) == invalid            # above the maximum
    stages[0].kind = 0
    assert set_stages(None, stages, 1) == invalid            # kinds outside 1 .. 4
    stages[0].kind = 5
    assert set_stages(None, stages, 1) == invalid
    stages[0].kind, stages[0].reserved = L.RFS_CLIP, 1
    assert set_stages(None, stages, 1) == invalid            # a non-zero reserved
    count = C.c_uint(7)
    assert L.lib.ohmhip_map_ray_filter_stages(None, stages, 5, C.byref(count)) == invalid
    rays = np.zeros((4, 3))
    out = np.zeros((4, 3))
    flags = np.zeros(2, dtype=np.uint8)
    passed = C.c_size_t(9)
    for fn in (L.lib.ohmhip_map_apply_ray_filter, L.lib.ohmhip_map_apply_ray_filter_device):
        assert fn(None, rays.ctypes.data, 4, out.ctypes.data, flags.ctypes.data, C.byref(passed)) == invalid
        assert passed.value == 0
        passed.value = 9
        assert fn(None, None, 0, None, None, None) == invalid


def test_mirrors():
    for name in ("setRayFilter", "rayFilter", "effectiveRayFilter", "clearRayFilter", "applyRayFilter"):
        assert callable(getattr(GpuMap, name))
    for name in ("DeviceRayFilter", "RayFilterStage", "on_device", "good_ray", "clip_ray", "clip_bounded_stage",
                 "clip_to_bounds_stage"):
        assert hasattr(RF, name)
    text = cpp_driver.host_mirror_text()
    for token in ("class DeviceRayFilter", "applyRayFilter(", "setRayFilter(const DeviceRayFilter",
                  "ohmhip_map_set_ray_filter_stages"):
        assert token in text, token
