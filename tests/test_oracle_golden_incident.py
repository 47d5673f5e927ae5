"""The oracle's incident-normal and touch-time leaves against committed golden vectors of the REAL reference code
(tests/golden/ref_incident.npz: ohm/VoxelIncidentCompute.h in its device form and ohm/VoxelTouchTimeCompute.h compiled in
place -- generator tests/golden/make_ref_vectors.py).  Bit-exact agreement required, on seeded rows, on stamps outside
[base, base + 2^32 ms), and on every update of the constructed set of tests/secondary_cases.py.  CPU only; needs neither
the reference checkout nor oracle/_ref."""
import os

import numpy as np

from oracle import oracle as O

import secondary_cases as S

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_incident.npz"))
LEAF = S.CLeaf(O.lib, "oracle")


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def test_golden_decode_normal():
    got = np.array([_bits(LEAF.decode(w)) for w in G["dec_in"]], dtype=np.uint32)
    assert np.array_equal(got, G["dec_out"])  # NaN z included: compared as bits
    assert np.isnan(G["dec_out"][:, 2].view(np.float32)).sum() > 50


def test_golden_encode_normal():
    rows = G["enc_in"].view(np.float32)
    got = np.array([LEAF.encode(r) for r in rows], dtype=np.uint32)
    assert np.array_equal(got, G["enc_out"])
    assert np.isnan(rows).any(axis=1).sum() >= 7  # NaN operands of the clamps are among the rows


def test_golden_update_incident_normal():
    rays = G["upd_ray"].view(np.float32)
    got = np.array([LEAF.update_normal(p, r, c) for p, r, c in zip(G["upd_packed"], rays, G["upd_count"])],
                   dtype=np.uint32)
    assert np.array_equal(got, G["upd_out"])
    assert np.count_nonzero((G["upd_packed"] == 0) & (G["upd_count"] > 0)) > 100  # "a zero normal restarts the count"


def test_golden_touch_time_outside_the_range():
    """5 s before the base and 5e6 s after it among them: the reference's x86-64 build truncates toward zero to 64 bits
    and keeps the low 32, and so does the oracle, in defined operations."""
    got = np.array([LEAF.encode_time(b, t) for b, t in G["touch_in"]], dtype=np.uint32)
    assert np.array_equal(got, G["touch_out"])
    assert LEAF.encode_time(100.0, 95.0) == 4294962296 and LEAF.encode_time(100.0, 100.0 + 5e6) == 705032704


def test_golden_constructed_set():
    cs = S.cases()
    assert S.digest(cs) == bytes(G["case_digest"]).hex(), "the set changed: regenerate tests/golden/ref_incident.npz"
    for name, with_mean in (("mean", True), ("nomean", False)):
        trace = []
        S.replay(cs, LEAF, with_mean=with_mean, trace=trace)
        assert np.array_equal(np.array([t[3] for t in trace], dtype=np.uint32), G["case_inc_" + name])
    got = np.array([LEAF.encode_time(cs.stamps[0], t) for t in cs.stamps], dtype=np.uint32)
    assert np.array_equal(got, G["case_touch"])
