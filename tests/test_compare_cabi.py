"""CPU: ohmhip_map_compare / ohmhip_map_compare_device are exported, declared and bound, stay out of the core ABI list,
the two structs have the header's layout, the refusals that need no live map are made before any device work (so on a
machine without a GPU too), and configureTolerance stores the reference's bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import ohm_amd
from ohm_amd import _lib as L

try:
    from ohm_amd import compare as M
except ImportError:  # (a library without the feature: the tests below then fail one by one, not at collection)
    M = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_compare", "ohmhip_map_compare_device")


def _header():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        return fh.read()


def test_symbols_exported_and_bound():
    raw = C.CDLL(ohm_amd.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name)
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int
        assert len(getattr(L.lib, name).argtypes) == 8
    for name in ("Severity", "kContinue", "VoxelsResult", "Tolerance", "configureTolerance", "compareLayoutLayer",
                 "compareVoxels", "occupancy_stats", "compare_maps"):
        assert hasattr(ohm_amd, name)


def test_header_declares_what_is_bound():
    header = _header()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    assert "/* MAP COMPARE." in header
    assert "\nint ohmhip_map_compare(" in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_compare(" not in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_compare_device(" in header
    assert "#define OHMHIP_CMP_CONTINUE (1u << 0)" in header and "#define OHMHIP_CMP_MAX_MEMBERS 6" in header
    assert (L.CMP_CONTINUE, L.CMP_MAX_MEMBERS, M.kContinue) == (1, 6, 1)
    assert "OHMHIP_LID_COUNT = 10" in header and L.LID_COUNT == 10
    block = header.split("/* MAP COMPARE.", 1)[1].split("*/", 1)[0]
    for rule in ("K1", "K2", "K3", "K4", "K5", "K6", "K7"):
        assert " %s " % rule in block
    assert "compareDatum :58-75" in block and "CompareMaps.cpp:78-144" in block and "CompareMaps.cpp:359-383" in block


def test_struct_layout():
    """ohmhip_compare_params: three 4-byte words and padding, six uint64, a pointer, a size_t; ohmhip_compare_result: two
    uint64, two 4-byte words, five uint64, two arrays of six uint64."""
    P, S = L.CompareParams, L.CompareResult
    assert C.sizeof(P) == 80
    assert (P.flags.offset, P.layer_id.offset, P.tolerance_members.offset, P.tolerance_bits.offset, P.keys_xyz.offset,
            P.key_count.offset) == (0, 4, 8, 16, 64, 72)
    assert C.sizeof(S) == 160
    assert (S.voxels_passed.offset, S.voxels_failed.offset, S.layout_match.offset, S.member_count.offset,
            S.regions_compared.offset, S.regions_missing.offset, S.keys_absent.offset, S.mismatch_count.offset,
            S.missing_count.offset, S.member_failed.offset, S.member_max_diff.offset) == (0, 8, 16, 20, 24, 32, 40, 48, 56,
                                                                                         64, 112)


def _compare(params, eval_=None, ref=None, result=True, mismatch=(0, None), missing=(0, None), device=False):
    res = L.CompareResult()
    fn = L.lib.ohmhip_map_compare_device if device else L.lib.ohmhip_map_compare
    return fn(eval_, ref, None if params is None else C.byref(params), mismatch[0], mismatch[1], missing[0], missing[1],
              (C.byref(res) if not device else C.addressof(res)) if result else None)


@pytest.mark.parametrize("device", [False, True])
def test_null_arguments(device):
    assert _compare(L.CompareParams(), device=device) == L.ERR_INVALID_ARG
    assert _compare(None, device=device) == L.ERR_INVALID_ARG
    assert _compare(L.CompareParams(), result=False, device=device) == L.ERR_INVALID_ARG
    fn = L.lib.ohmhip_map_compare_device if device else L.lib.ohmhip_map_compare
    assert fn(None, None, None, 0, None, 0, None, None) == L.ERR_INVALID_ARG


# (Without a device there is no live map to pass: tests/test_gpu_compare.py repeats these with two live maps, where the
# named argument is the only thing wrong.)
@pytest.mark.parametrize("flags", [2, 4, 0x80000000, 0xfffffffe, 3])
def test_unknown_flag_bits(flags):
    p = L.CompareParams()
    p.flags = flags
    assert _compare(p) == L.ERR_INVALID_ARG


@pytest.mark.parametrize("layer_id", [-1, 10, 11, 1 << 20, -(1 << 31)])
def test_layer_id_out_of_range(layer_id):
    p = L.CompareParams()
    p.layer_id = layer_id
    assert _compare(p) == L.ERR_INVALID_ARG


def test_capacity_without_an_array_and_keys_without_a_count():
    p = L.CompareParams()
    assert _compare(p, mismatch=(4, None)) == L.ERR_INVALID_ARG
    assert _compare(p, missing=(1, None)) == L.ERR_INVALID_ARG
    keys = np.zeros((2, 3), dtype=np.int16)
    p = L.CompareParams()
    p.keys_xyz, p.key_count = keys.ctypes.data, 0
    assert _compare(p) == L.ERR_INVALID_ARG
    p = L.CompareParams()
    p.keys_xyz, p.key_count = None, 2
    assert _compare(p) == L.ERR_INVALID_ARG


def test_members_table_matches_the_layers():
    for name, (lid, dtype, comps) in ohm_amd.LAYERS.items():
        assert len(M.MEMBERS[name]) == comps == L.lib.ohmhip_layer_voxel_bytes(lid) // 4 <= L.CMP_MAX_MEMBERS
        assert all(np.dtype(t) == np.dtype(dtype) for _, t in M.MEMBERS[name])


@pytest.mark.parametrize("epsilon,dtype,bits", [
    (np.float32(-0.01), np.float32, 0x3c23d70a),
    (0.01, np.float32, 0x3c23d70a),                     # a Python float is a float32
    (np.float64(-0.5), np.float64, 0x3fe0000000000000),
    (np.int8(-128), np.int8, 128),                      # std::abs widens before it negates
    (np.uint8(200), np.uint8, 200),
    (np.int16(-3), np.int16, 3),
    (np.uint16(65535), np.uint16, 65535),
    (np.int32(-7), np.int32, 7),
    (np.uint32(0xfffffffe), np.uint32, 0xfffffffe),
    (np.int64(-(1 << 40)), np.int64, 1 << 40),
    (np.uint64((1 << 63) + 5), np.uint64, (1 << 63) + 5),
    (3, np.uint32, 3),
    (-3, np.int32, 3),
    (np.float32(np.inf), np.float32, 0x7f800000),
])
def test_configure_tolerance_bytes(epsilon, dtype, bits):
    tol = M.Tolerance("mean")
    M.configureTolerance(tol, "count", epsilon)
    assert tol.indexOf("count") == 0 and tol.indexOf("coord") == -1
    name, got_dtype, got_bits = tol.members[0]
    assert (name, np.dtype(got_dtype), got_bits) == ("count", np.dtype(dtype), bits)


def test_params_from_a_tolerance():
    """Members are matched by name, names the layer lacks are ignored, and the stored bytes go down as they are: a float32
    1.0 on `count` is eps = 0x3f800000."""
    tol = M.Tolerance("mean")
    M.configureTolerance(tol, "count", np.float32(1))
    M.configureTolerance(tol, "occupancy", np.float32(2))
    p, _ = M.compare_params("mean", tol, M.kContinue)
    assert (p.flags, p.layer_id, p.tolerance_members) == (1, L.LID_MEAN, 0b10)
    assert list(p.tolerance_bits) == [0, 0x3f800000, 0, 0, 0, 0]
    tol = M.default_tolerances()["covariance"]
    p, _ = M.compare_params("covariance", tol)
    assert p.tolerance_members == 0x3f and set(p.tolerance_bits) == {0x3c23d70a}
    assert sorted(M.default_tolerances()) == ["clearance", "covariance", "intensity", "occupancy"]
    p, _ = M.compare_params("occupancy", M.default_tolerances()["occupancy"])
    assert p.tolerance_bits[0] == 0x42c80000  # 1e2f
    assert bool(M.VoxelsResult(5, 0, True)) and not M.VoxelsResult(5, 1, True) and not M.VoxelsResult(5, 0, False)
