"""CPU: the layer-change entry points of the C ABI (ohmhip_map_update_layers, ohmhip_map_layers) are exported, declared
and bound, tagged experimental and outside the core ABI list -- the binding core does not call them --, refuse invalid
arguments with OHMHIP_ERR_INVALID_ARG before any device work, so the refusals run without a GPU; the stats record's
layout; the header carries the rules U1 - U10; both mirrors declare the interface.  (tests/test_gpu_layout.py repeats
the refusals against live maps.)"""
import ctypes as C
import os

import cpp_driver
from ohm_amd import ClearanceProcess, GpuMap, OccupancyMap
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_map_update_layers", "ohmhip_map_layers")


def test_symbols_exported_and_bound():
    lib = C.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name)
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int


def test_declared_experimental_and_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert "OHMHIP_EXPERIMENTAL int " + name + "(" in header
    with open(os.path.join(ROOT, "ohm_amd", "host", "ref_adaptor", "private", "HipBindingCore.cpp")) as fh:
        binding_core = fh.read()
    assert not any(name in binding_core for name in NAMES)
    assert "LAYER CHANGES" in header and "#define OHMHIP_LAYOUT_DISCARD_MAP 1u" in header
    assert "OHMHIP_LID_COUNT = 10" in header  # no new layer
    for rule in range(1, 11):
        assert " U%d " % rule in header


def test_stats_layout():
    fields = ("layers_before", "layers_after", "regions_resident", "regions_in_store", "regions_evicted",
              "bytes_per_region_before", "bytes_per_region_after")
    assert [name for name, _ in L.LayerChangeStats._fields_] == list(fields)
    assert [getattr(L.LayerChangeStats, name).offset for name in fields] == [0, 4, 8, 16, 24, 32, 40]
    assert C.sizeof(L.LayerChangeStats) == 48 and L.LAYOUT_DISCARD_MAP == 1


def test_refusals_without_a_map():
    stats = L.LayerChangeStats(1, 2, 3, 4, 5, 6, 7)
    update = L.lib.ohmhip_map_update_layers
    assert update(None, 1, 0, C.byref(stats)) == L.ERR_INVALID_ARG  # null map
    assert bytes(stats) == bytes(C.sizeof(stats))                    # (the stats are zeroed all the same)
    assert update(None, 1, 0, None) == L.ERR_INVALID_ARG
    assert update(None, 0, 0, None) == L.ERR_INVALID_ARG
    assert update(None, 1 << L.LID_COUNT, 0, None) == L.ERR_INVALID_ARG
    assert update(None, 1, 2, None) == L.ERR_INVALID_ARG
    layers = C.c_uint(77)
    assert L.lib.ohmhip_map_layers(None, C.byref(layers)) == L.ERR_INVALID_ARG and layers.value == 77
    assert L.lib.ohmhip_map_layers(None, None) == L.ERR_INVALID_ARG


def test_mirrors():
    for name in ("updateLayout", "addLayer", "removeLayer", "addVoxelMeanLayer", "addTraversalLayer", "addTouchTimeLayer",
                 "addIncidentNormalLayer", "voxelMeanEnabled", "traversalEnabled", "touchTimeEnabled",
                 "incidentNormalEnabled", "lastLayerChangeStats", "hasLayer"):
        assert callable(getattr(GpuMap, name)), name
    for name in ("updateLayout", "removeLayer", "addLayer"):
        assert callable(getattr(OccupancyMap, name)), name
    assert "GpuMap.addLayer(\"clearance\")" in ClearanceProcess.ensureClearanceLayer.__doc__


def test_cpp_mirror_declares_the_same_interface():
    text = cpp_driver.host_mirror_text()
    for token in ("void updateLayout(unsigned layers, bool preserve_map = true)", "void removeLayer(int layer_id)",
                  "addVoxelMeanLayer()", "addTraversalLayer()", "addTouchTimeLayer()", "addIncidentNormalLayer()",
                  "voxelMeanEnabled()", "traversalEnabled()", "touchTimeEnabled()", "incidentNormalEnabled()",
                  "lastLayerChangeStats()", "ohmhip_map_update_layers("):
        assert token in text, token
    assert text.count("void updateLayout(unsigned layers, bool preserve_map = true)") == 2  # OccupancyMap and GpuMap
    assert "{ \"layout\"," in cpp_driver.driver_text()
