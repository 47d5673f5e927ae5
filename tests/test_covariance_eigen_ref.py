"""CPU: the covariance decomposition rule D1-D6 (include/ohmhip.h).

 * the model (tests/covariance_eigen_ref.py) against mpmath.eigsy at 60 digits on family B, in multiples of eps = 2^-52,
   bounded by 4 x what numpy.linalg.eigh (LAPACK, an independent fp64 solver) reaches on the same inputs;
 * termination below the sweep cap on every case, asserted as a condition;
 * D2, D4, D5 and D6 on the planted states of family A against hand-written outcomes;
 * the library's host evaluation of the rule (ohmhip_covariance_decompose: the text the kernels compile) equal to the
   model bit for bit on every case -- tests/test_gpu_covariance_eigen.py holds the device to the same bytes;
 * the quaternion helper reproduces the D4 matrix to 8 eps."""
import functools

import mpmath
import numpy as np

import covariance_cases as cases
import covariance_eigen_ref as ref
import ohm_amd

EPS = 2.0 ** -52
UP_AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1))


model_results = cases.model_results


def _exact_c(p):
    m = [mpmath.mpf(float(x)) for x in p]
    s = mpmath.matrix([[m[0], 0, 0], [m[1], m[2], 0], [m[3], m[4], m[5]]])
    return s * s.T


def _metrics(c, exact_values, exact_vectors, values, vectors):
    """The four distances of one decomposition from the exact one, in eps.  vectors[r][c]; everything in mpmath."""
    norm = max(abs(x) for x in exact_values)
    v = mpmath.matrix(3, 3)
    for r in range(3):
        for col in range(3):
            v[r, col] = mpmath.mpf(float(vectors[r][col]))
    lam = [mpmath.mpf(float(x)) for x in values]
    value_error = max(abs(lam[i] - exact_values[i]) for i in range(3)) / norm
    residual = max(mpmath.norm(c * v[:, i] - lam[i] * v[:, i]) for i in range(3)) / norm
    orthogonality = mpmath.mnorm(v.T * v - mpmath.eye(3), "f")
    a, b = v[:, 0], exact_vectors[:, 0]
    cross = mpmath.matrix([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    sine = mpmath.norm(cross) / (mpmath.norm(a) * mpmath.norm(b))
    angle = sine * (exact_values[1] - exact_values[0]) / norm
    return np.array([float(x / EPS) for x in (value_error, residual, orthogonality, angle)])


@functools.lru_cache(maxsize=None)
def family_b_figures():
    """(worst of the model, worst of LAPACK, smallest relative gap) over family B."""
    mpmath.mp.dps = 60
    worst_model, worst_lapack, smallest_gap = np.zeros(4), np.zeros(4), np.inf
    offset = len(cases.FAMILY_A)
    for k, (_, p, _) in enumerate(cases.FAMILY_B):
        c = _exact_c(p)
        exact_values, exact_vectors = mpmath.eigsy(c)
        order = sorted(range(3), key=lambda i: exact_values[i])
        exact_values = [exact_values[i] for i in order]
        exact_vectors = mpmath.matrix([[exact_vectors[r, i] for i in order] for r in range(3)])
        smallest_gap = min(smallest_gap, float((exact_values[1] - exact_values[0]) / exact_values[2]))
        d = model_results()[offset + k]
        model_vectors = d.eigenvectors.reshape(3, 3).T  # [r][c]
        worst_model = np.maximum(worst_model, _metrics(c, exact_values, exact_vectors, d.eigenvalues, model_vectors))
        c64 = ref.covariance_matrix(p)  # LAPACK sees the fp64 matrix the model sees
        full = np.array([[c64[0], c64[1], c64[2]], [c64[1], c64[3], c64[4]], [c64[2], c64[4], c64[5]]])
        w, v = np.linalg.eigh(full)
        worst_lapack = np.maximum(worst_lapack, _metrics(c, exact_values, exact_vectors, w, v))
    return worst_model, worst_lapack, smallest_gap


def test_family_b_gap_is_what_the_case_list_promises():
    assert len(cases.FAMILY_B) >= 300
    assert family_b_figures()[2] >= 2.0 ** -20


def test_model_against_arbitrary_precision():
    worst_model, worst_lapack, _ = family_b_figures()
    names = ("eigenvalue error / |C|", "residual |Cv - lv| / |C|", "|VtV - I|", "sin(angle) gap / |C|")
    for name, m, l in zip(names, worst_model, worst_lapack):
        print("%-28s model %.3f eps   LAPACK %.3f eps" % (name, m, l))
    assert np.all(worst_lapack > 0)
    assert np.all(worst_model <= 4.0 * worst_lapack), (worst_model, worst_lapack)


def test_terminates_below_the_sweep_cap():
    sweeps = np.array([d.sweeps for d in model_results()])
    print("sweeps that rotated -> cases:", dict(zip(*np.unique(sweeps, return_counts=True))))
    assert sweeps.max() < ref.SWEEP_CAP, [cases.ALL_CASES[i][0] for i in np.flatnonzero(sweeps >= ref.SWEEP_CAP)]


def _same(a, b):
    """Equal with signs: -0.0 is not 0.0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_planted_outcomes():
    results = model_results()
    checked = {"status": 0, "eigenvalues": 0, "eigenvectors": 0, "scale": 0, "normal": 0, "flip_up": 0}
    for (name, p, expect), d in zip(cases.FAMILY_A, results):
        assert d.status == expect["status"], name
        for field in ("eigenvalues", "eigenvectors", "scale", "normal"):
            if field in expect:
                assert _same(getattr(d, field), expect[field]), (name, field, getattr(d, field))
                checked[field] += 1
        for up in expect.get("flip_up", ()):
            # the dot product is exactly zero: flip = 1.0, so the normal is narrowed as it stands, -0.0 included
            assert np.array_equal(ref.normal_for_up(d, up).view(np.uint32), d.normal.astype(np.float32).view(np.uint32)), \
                (name, up)
            checked["flip_up"] += 1
        checked["status"] += 1
    assert sum(1 for _, _, e in cases.FAMILY_A if e["status"] == 2) >= 18  # NaN, +inf, -inf in each slot
    assert min(checked.values()) >= 10, checked


def test_general_properties_on_every_case():
    for (name, p, _), d in zip(cases.ALL_CASES, model_results()):
        assert np.all(np.diff(d.eigenvalues) >= 0), name  # ascending
        v = d.eigenvectors.reshape(3, 3).T
        assert abs(np.linalg.det(v) - 1.0) < 64 * EPS, name  # D4: a rotation
        assert abs(np.linalg.norm(d.normal) - 1.0) < 8 * EPS, name
        for up in UP_AXES:
            n = ref.normal_for_up(d, up)
            assert float(np.dot(n.astype(np.float64), up)) >= 0.0, (name, up)
        expected_scale = [np.sqrt(x) if x > 1e-9 else x for x in np.abs(d.eigenvalues)]
        assert _same(d.scale, expected_scale), name


def test_host_evaluation_equals_the_model_bit_for_bit():
    got = ohm_amd.covariance_decompose(cases.all_p())
    results = model_results()
    assert got.status.tolist() == [d.status for d in results]
    for field, have in (("eigenvalues", got.eigenvalues), ("eigenvectors", got.eigenvectors.reshape(-1, 9)),
                        ("scale", got.scales), ("normal", got.normals)):
        want = np.stack([getattr(d, field) for d in results])
        differs = np.flatnonzero(np.any(have.view(np.uint64) != want.view(np.uint64), axis=1))
        assert differs.size == 0, (field, [cases.ALL_CASES[i][0] for i in differs[:5]])


def test_quaternion_reproduces_the_rotation():
    P = cases.all_p()
    q, scale = ohm_amd.covariance_unit_sphere_transformation(P)
    d = ohm_amd.covariance_decompose(P)
    assert _same(scale, d.scales)
    rotation = np.transpose(d.eigenvectors, (0, 2, 1))  # [i, r, c]
    back = ohm_amd.quaternion_to_rotation(q)
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 8 * EPS
    assert np.abs(back - rotation).max() <= 8 * EPS, np.abs(back - rotation).max() / EPS
    assert ohm_amd.covariance_estimate_primary_normal(P[:3]).shape == (3, 3)
