"""Oracle restatement vs the REAL reference code for the incident-normal leaf: oracle/_ref/libohmref.so holds
ohm/VoxelIncidentCompute.h compiled where it lies, in its GPUTIL_DEVICE form (recipe oracle/Makefile +
oracle/ref_shim_incident.cpp).  Bit-exact agreement required, also of the committed fixture with the live library.
CPU only; skipped when the prebuilt reference library is absent (it cannot be rebuilt without the reference checkout)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle as O
from ohm_amd import synth

import secondary_cases as S

if not os.path.exists(O.REF_LIB_PATH):
    pytest.skip("oracle/_ref/libohmref.so not built (reference checkout absent)", allow_module_level=True)

_REF_LIB = C.CDLL(O.REF_LIB_PATH)
if not hasattr(_REF_LIB, "ref_update_incident_normal"):
    # a library built before oracle/ref_shim_incident.cpp existed, on a machine that cannot rebuild it
    pytest.skip("oracle/_ref/libohmref.so predates the incident shim (reference checkout absent)", allow_module_level=True)

REF = S.CLeaf(_REF_LIB, "ref")
ORACLE = S.CLeaf(O.lib, "oracle")


def _u(seed, n, stream):
    return synth.uniform01(seed, np.arange(n, dtype=np.uint64), stream)


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def test_decode_and_encode_bit_exact():
    n = 20000
    words = (_u(41, n, 0) * 2.0**32).astype(np.uint64).astype(np.uint32)
    for w in words:
        assert np.array_equal(_bits(ORACLE.decode(w)), _bits(REF.decode(w))), hex(int(w))
    v = np.stack([(_u(42, n, s) - 0.5) * 2.2 for s in range(3)], axis=1).astype(np.float32)
    v[::97, 0] = np.nan
    v[5::97, 1] = np.nan
    v[9::97, 2] = np.nan
    for row in v:
        assert ORACLE.encode(row) == REF.encode(row), row


def test_chained_updates_bit_exact():
    """Chains of updates per lane, like a voxel sees them: most NaN decodes arise only from a previous encode."""
    n, lanes = 40000, 64
    ray = np.stack([(_u(43, n, s) - 0.5) for s in range(3)], axis=1)
    ray[:, 2] *= np.where(_u(43, n, 3) < 0.5, 1e-4, 1.0)  # half of them nearly in plane: the decoder's NaN region
    ray *= (10.0 ** (_u(43, n, 4) * 5.0 - 4.0))[:, None]
    ray = ray.astype(np.float32)
    state = [0] * lanes
    count = [0] * lanes
    nan_decodes = 0
    for i in range(n):
        lane = i % lanes
        nan_decodes += bool(np.isnan(REF.decode(state[lane])[2]))
        a = ORACLE.update_normal(state[lane], ray[i], count[lane])
        b = REF.update_normal(state[lane], ray[i], count[lane])
        assert a == b, (i, hex(state[lane]), ray[i], count[lane])
        state[lane] = b
        count[lane] = (count[lane] + 1) % (1 + lane % 7)  # short chains: small counts are where NaN decodes live
    assert nan_decodes > 1000


def test_fixture_is_what_the_reference_header_compiles_to():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_incident.npz"))
    assert np.array_equal(np.array([_bits(REF.decode(w)) for w in g["dec_in"]], dtype=np.uint32), g["dec_out"])
    assert np.array_equal(np.array([REF.encode(r) for r in g["enc_in"].view(np.float32)], dtype=np.uint32),
                          g["enc_out"])
    got = [REF.update_normal(p, r, c) for p, r, c in zip(g["upd_packed"], g["upd_ray"].view(np.float32), g["upd_count"])]
    assert np.array_equal(np.array(got, dtype=np.uint32), g["upd_out"])
    assert np.array_equal(np.array([REF.encode_time(b, t) for b, t in g["touch_in"]], dtype=np.uint32), g["touch_out"])
    cs = S.cases()
    assert S.digest(cs) == bytes(g["case_digest"]).hex()
    for name, with_mean in (("mean", True), ("nomean", False)):
        trace = []
        S.replay(cs, REF, with_mean=with_mean, trace=trace)
        assert np.array_equal(np.array([t[3] for t in trace], dtype=np.uint32), g["case_inc_" + name])
    assert np.array_equal(np.array([REF.encode_time(cs.stamps[0], t) for t in cs.stamps], dtype=np.uint32),
                          g["case_touch"])
