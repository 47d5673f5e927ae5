"""The covariances the decomposition rule D1-D6 is tested on (tests/covariance_eigen_ref.py is the model, DESIGN.md
4.14 the rule).  A case is (name, p, expect): p the six floats of a CovarianceVoxel -- S lower triangular with rows
(p0, 0, 0), (p1, p2, 0), (p3, p4, p5) --, expect a dict of hand-written outcomes (possibly empty):

  status        1 decomposed, 2 the non-finite branch D2
  eigenvalues   exact, ascending
  eigenvectors  exact, 9 values column-major after D4 (compared with signs: -0.0 is not 0.0)
  scale         exact D5 scales
  normal        exact D6 normal before the heightmap's flip
  flip_up       up axis normals whose dot product with the normal is exactly zero: the flip keeps the normal

FAMILY_A plants states; FAMILY_B is seeded random and ill-conditioned S whose two smallest exact eigenvalues lie at
least 2^-20 * |C|_2 apart (test_covariance_eigen_ref.py asserts that against the arbitrary-precision spectrum)."""
import functools

import numpy as np

F32_MAX = float(np.finfo(np.float32).max)
NZ = -0.0


def _f32(p):
    return np.array(p, dtype=np.float32)


def _planted():
    cases = []

    def add(name, p, **expect):
        cases.append((name, _f32(p), expect))

    identity = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    add("zero", [0, 0, 0, 0, 0, 0], status=1, eigenvalues=[0, 0, 0], eigenvectors=identity, scale=[0, 0, 0],
        normal=[1, 0, 0])
    # initialiseCovariance of a fresh voxel at 0.1 m resolution: 0.1f * float(resolution) on the diagonal
    s = np.float32(0.1) * np.float32(0.1)
    add("fresh", [s, 0, s, 0, 0, s], status=1, eigenvalues=[float(s) * float(s)] * 3, eigenvectors=identity,
        normal=[1, 0, 0])
    add("sphere", [2, 0, 2, 0, 0, 2], status=1, eigenvalues=[4, 4, 4], eigenvectors=identity, scale=[2, 2, 2],
        normal=[1, 0, 0])
    add("diag_sorted", [1, 0, 2, 0, 0, 3], status=1, eigenvalues=[1, 4, 9], eigenvectors=identity, scale=[1, 2, 3],
        normal=[1, 0, 0], flip_up=[(0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    # ascending order permutes the columns cyclically: (e1, e2, e0) has determinant +1
    add("diag_cyclic", [3, 0, 1, 0, 0, 2], status=1, eigenvalues=[1, 4, 9], eigenvectors=[0, 1, 0, 0, 0, 1, 1, 0, 0],
        scale=[1, 2, 3], normal=[0, 1, 0], flip_up=[(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)])
    # one transposition: (e1, e0, e2) has determinant -1, so D4 negates column 0 and keeps its -0.0
    add("diag_det_minus_xy", [2, 0, 1, 0, 0, 3], status=1, eigenvalues=[1, 4, 9],
        eigenvectors=[NZ, -1, NZ, 1, 0, 0, 0, 0, 1], scale=[1, 2, 3], normal=[NZ, -1, NZ],
        flip_up=[(1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)])
    add("diag_det_minus_xz", [3, 0, 2, 0, 0, 1], status=1, eigenvalues=[1, 4, 9],
        eigenvectors=[NZ, NZ, -1, 0, 1, 0, 1, 0, 0], scale=[1, 2, 3], normal=[NZ, NZ, -1],
        flip_up=[(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)])
    add("diag_det_minus_yz", [1, 0, 3, 0, 0, 2], status=1, eigenvalues=[1, 4, 9],
        eigenvectors=[-1, NZ, NZ, 0, 0, 1, 0, 1, 0], scale=[1, 2, 3], normal=[-1, NZ, NZ],
        flip_up=[(0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    # two equal smallest eigenvalues: equal values keep the order of their diagonal positions
    add("equal_smallest_first", [1, 0, 1, 0, 0, 5], status=1, eigenvalues=[1, 1, 25], eigenvectors=identity,
        normal=[1, 0, 0])
    add("equal_smallest_last", [5, 0, 1, 0, 0, 1], status=1, eigenvalues=[1, 1, 25],
        eigenvectors=[0, 1, 0, 0, 0, 1, 1, 0, 0], normal=[0, 1, 0])
    add("equal_largest", [1, 0, 5, 0, 0, 5], status=1, eigenvalues=[1, 25, 25], eigenvectors=identity, normal=[1, 0, 0])
    add("rank1", [1, 2, 0, 3, 0, 0], status=1)
    add("rank1_axis", [0, 0, 0, 0, 0, 2], status=1, eigenvalues=[0, 0, 4], eigenvectors=identity, scale=[0, 0, 2],
        normal=[1, 0, 0])
    add("rank2", [1, 2, 1, 3, -1, 0], status=1)
    add("rank2_axis", [2, 0, 0, 0, 0, 3], status=1, eigenvalues=[0, 4, 9], eigenvectors=[NZ, -1, NZ, 1, 0, 0, 0, 0, 1],
        scale=[0, 2, 3], normal=[NZ, -1, NZ])
    # the smallest eigenvector lies exactly in a coordinate plane: its dot product with the third axis is exactly zero
    add("block_xy", [2, 1, 1, 0, 0, 3], status=1, flip_up=[(0, 0, 1), (0, 0, -1)])
    add("block_yz", [3, 0, 2, 0, 1, 1], status=1, flip_up=[(1, 0, 0), (-1, 0, 0)])
    add("block_xz", [2, 0, 3, 1, 0, 1], status=1, flip_up=[(0, 1, 0), (0, -1, 0)])
    for e in (40, 30, 24, 20, 10, 5, 1, 0):
        r = 2.0 ** -e
        add("offdiag_2^-%d" % e, [1, r, 2, r, r, 3], status=1)
        add("offdiag_equal_diag_2^-%d" % e, [1, r, 1, -r, r, 1], status=1)
    for e in range(-3, 4):
        k = 10.0 ** e
        add("scale_1e%d" % e, [0.7 * k, -0.2 * k, 0.5 * k, 0.3 * k, 0.1 * k, 0.05 * k], status=1)
    base = [0.7, -0.2, 0.5, 0.3, 0.1, 0.05]
    for slot in range(6):
        for name, bad in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            p = list(base)
            p[slot] = bad
            add("%s_p%d" % (name, slot), p, status=2, eigenvalues=[1, 1, 1], eigenvectors=identity, scale=[1, 1, 1],
                normal=[1, 0, 0])
    add("nan_all", [np.nan] * 6, status=2, eigenvalues=[1, 1, 1], eigenvectors=identity, scale=[1, 1, 1],
        normal=[1, 0, 0])
    add("inf_with_zeros", [np.inf, 0, 1, 0, 0, 1], status=2, eigenvalues=[1, 1, 1], eigenvectors=identity,
        scale=[1, 1, 1], normal=[1, 0, 0])
    add("negative_zero_all", [NZ] * 6, status=1, eigenvalues=[0, 0, 0], eigenvectors=identity, scale=[0, 0, 0],
        normal=[1, 0, 0])
    add("negative_zero_offdiag", [1, NZ, 2, NZ, NZ, 3], status=1, eigenvalues=[1, 4, 9], eigenvectors=identity,
        normal=[1, 0, 0])
    add("negative_diagonal", [-1, 0, -2, 0, 0, -3], status=1, eigenvalues=[1, 4, 9], eigenvectors=identity,
        normal=[1, 0, 0])
    # FLT_MAX squared is 1.16e77: C is finite in fp64, so these decompose (D2 needs a non-finite ENTRY OF C, and six
    # floats can only produce one from a non-finite float)
    m2 = F32_MAX * F32_MAX
    add("flt_max_diag", [F32_MAX, 0, F32_MAX, 0, 0, F32_MAX], status=1, eigenvalues=[m2, m2, m2], eigenvectors=identity,
        scale=[F32_MAX] * 3, normal=[1, 0, 0])
    add("flt_max_all", [F32_MAX] * 6, status=1)
    add("flt_max_mixed", [F32_MAX, 1, 1e-30, -F32_MAX, 1e20, 1], status=1)
    tiny = float(np.float32(1.4e-45))
    add("denormal_diag", [tiny, 0, tiny, 0, 0, tiny], status=1, eigenvalues=[tiny * tiny] * 3, eigenvectors=identity,
        normal=[1, 0, 0])
    add("denormal_all", [tiny] * 6, status=1)
    # eigenvalues either side of D5's 1e-9: at or below it the scale is the eigenvalue itself, above it the root
    lo, hi = float(np.float32(3.1622e-5)), float(np.float32(3.1623e-5))
    assert lo * lo < 1e-9 < hi * hi
    add("straddle_1e-9", [lo, 0, hi, 0, 0, 1], status=1, eigenvalues=[lo * lo, hi * hi, 1], eigenvectors=identity,
        scale=[lo * lo, float(np.sqrt(np.float64(hi * hi))), 1], normal=[1, 0, 0])
    add("straddle_1e-9_rotated", [hi, lo, lo, hi, lo, 1], status=1)
    return cases


def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    return q * np.sign(np.diag(r))


def _seeded():
    rng = np.random.default_rng(20240614)
    cases = []

    def gap_ok(p):
        # what the construction promises, with margin for the float32 rounding of S: the test re-checks it exactly
        s = np.array([[p[0], 0, 0], [p[1], p[2], 0], [p[3], p[4], p[5]]], dtype=np.float64)
        lam = np.linalg.eigvalsh(s @ s.T)
        return np.all(np.isfinite(lam)) and lam[2] > 0 and (lam[1] - lam[0]) >= 2.0 ** -18 * lam[2]

    # plain random S at several magnitudes
    while len(cases) < 120:
        k = 10.0 ** rng.uniform(-3, 3)
        p = _f32(rng.standard_normal(6) * k)
        if gap_ok(p):
            cases.append(("random_%03d" % len(cases), p, {"status": 1}))
    # prescribed spectra: condition numbers up to 1e14, smallest gaps down to 2^-17 of the largest eigenvalue, the two
    # largest eigenvalues close or equal
    n = 0
    while n < 200:
        big = 10.0 ** rng.uniform(-4, 4)
        gap = 2.0 ** -rng.uniform(0.5, 17.0)
        l0 = 10.0 ** -rng.uniform(0, 14)
        l1 = l0 + gap
        kind = n % 4
        l2 = (l1, l1 * (1 + 2.0 ** -rng.uniform(10, 40)), 1.0 + l1, 1.0 + l1)[kind]
        lam = np.array([l0, l1, l2]) / max(l2, 1.0) * big
        q = _random_rotation(rng)
        c = (q * lam) @ q.T
        c = 0.5 * (c + c.T)
        try:
            s = np.linalg.cholesky(c)
        except np.linalg.LinAlgError:
            continue
        p = _f32([s[0, 0], s[1, 0], s[1, 1], s[2, 0], s[2, 1], s[2, 2]])
        if gap_ok(p):
            cases.append(("spectrum_%03d" % n, p, {"status": 1}))
            n += 1
    return cases


FAMILY_A = _planted()
FAMILY_B = _seeded()
ALL_CASES = FAMILY_A + FAMILY_B


def all_p():
    """(N, 6) float32: every case's covariance, family A first."""
    return np.stack([p for _, p, _ in ALL_CASES])


@functools.lru_cache(maxsize=None)
def model_results():
    """The model's Decomposition of every case, in all_p()'s order: computed once, shared by the tests, never changed."""
    import covariance_eigen_ref
    return tuple(covariance_eigen_ref.decompose(p) for _, p, _ in ALL_CASES)
