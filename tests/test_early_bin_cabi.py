"""CPU: ohmhip_map_pipeline_counts is declared, exported and bound, tagged as a measurement call (not core ABI), mirrored
as GpuMap.pipelineCounts, and refuses NULL arguments before any device work."""
import ctypes as C
import os
import re

import ohm_amd
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ohmhip_map_pipeline_counts"


def _header():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        return fh.read()


def test_symbol_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"OHMHIP_EXPERIMENTAL\s+int\s+%s\s*\(\s*ohmhip_map_t\s+\w+\s*,\s*uint64_t\s*\*\s*\w+\s*,\s*uint64_t\s*\*\s*\w+\s*\)"
                     % NAME, header)
    assert hasattr(C.CDLL(ohm_amd.LIB_PATH), NAME)
    assert NAME in L.EXPORTED_SYMBOLS
    fn = getattr(L.lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 3
    assert callable(getattr(ohm_amd.GpuMap, "pipelineCounts"))


def test_not_in_the_core_abi():
    header = _header()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and NAME not in core


def test_null_arguments_are_refused():
    """Checked before anything touches a device: the same with and without a GPU, and the outputs stay as they were."""
    batches, early = C.c_uint64(7), C.c_uint64(9)
    assert L.lib.ohmhip_map_pipeline_counts(None, C.byref(batches), C.byref(early)) == L.ERR_INVALID_ARG
    assert (batches.value, early.value) == (7, 9)
    assert L.lib.ohmhip_map_pipeline_counts(None, None, None) == L.ERR_INVALID_ARG
