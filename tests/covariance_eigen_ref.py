"""The covariance decomposition rule D1-D6 (include/ohmhip.h) restated in numpy float64 scalars, one
operation per line, in the order the device function (ohm_amd/csrc/covariance_eigen_device.h) evaluates them.  Only
+ - * / sqrt, compares and selects: each is correctly rounded in both places, so the two agree bit for bit.

decompose(p) takes the six floats of a CovarianceVoxel and returns a Decomposition; normal_for_up(d, up) is the
heightmap's part of D6."""
import collections

import numpy as np

F = np.float64
ZERO = F(0.0)
ONE = F(1.0)
HALF = F(0.5)
HUNDRED = F(100.0)
DBL_MAX = F(np.finfo(np.float64).max)
SCALE_EPSILON = F(1e-9)
SWEEP_CAP = 16  # kCovSweepCap
STATUS_ABSENT, STATUS_DECOMPOSED, STATUS_NON_FINITE = 0, 1, 2

Decomposition = collections.namedtuple("Decomposition", "eigenvalues eigenvectors status sweeps scale normal")


def covariance_matrix(p):
    """D1: the six distinct entries (c00, c01, c02, c11, c12, c22) of C = S S^T."""
    p0, p1, p2, p3, p4, p5 = (F(np.float32(x)) for x in p)
    c00 = p0 * p0
    c01 = p0 * p1
    c02 = p0 * p3
    c11 = p1 * p1
    c11 = c11 + p2 * p2
    c12 = p1 * p3
    c12 = c12 + p2 * p4
    c22 = p3 * p3
    c22 = c22 + p4 * p4
    c22 = c22 + p5 * p5
    return c00, c01, c02, c11, c12, c22


def _finite(x):
    return abs(x) <= DBL_MAX  # false for NaN


def _rotate(g, h, s, tau):
    """(g, h) -> (g - s (h + g tau), h + s (g - h tau))"""
    t0 = g * tau
    t0 = h + t0
    t0 = s * t0
    t1 = h * tau
    t1 = g - t1
    t1 = s * t1
    return g - t0, h + t1


def jacobi(c):
    """D3 before the ordering: cyclic Jacobi over (0,1), (0,2), (1,2).  Returns (diagonal, V as rows of rows, sweeps):
    `sweeps` counts the sweeps that rotated; the loop ends when the off-diagonal sum is exactly zero."""
    a = [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]  # only the upper triangle is used
    v = [[ONE, ZERO, ZERO], [ZERO, ONE, ZERO], [ZERO, ZERO, ONE]]
    sweeps = 0
    for sweep in range(SWEEP_CAP):
        off = abs(a[0][1]) + abs(a[0][2])
        off = off + abs(a[1][2])
        if off == ZERO:
            break
        sweeps = sweep + 1
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = a[p][q]
            if apq == ZERO:
                continue
            g = HUNDRED * abs(apq)
            if sweep >= 3 and abs(a[p][p]) + g == abs(a[p][p]) and abs(a[q][q]) + g == abs(a[q][q]):
                a[p][q] = ZERO  # the classic cut-off: the rotation would not change either diagonal entry
                continue
            h = a[q][q] - a[p][p]
            if abs(h) + g == abs(h):
                t = apq / h
            else:
                theta = HALF * h
                theta = theta / apq
                t = theta * theta
                t = t + ONE
                t = np.sqrt(t)
                t = abs(theta) + t
                t = ONE / t
                if theta < ZERO:
                    t = -t
            cs = t * t
            cs = cs + ONE
            cs = np.sqrt(cs)
            cs = ONE / cs
            s = t * cs
            tau = ONE + cs
            tau = s / tau
            h = t * apq
            a[p][p] = a[p][p] - h
            a[q][q] = a[q][q] + h
            a[p][q] = ZERO
            # the third index r: its entries against p and q, in the upper triangle
            rp = (r, p) if r < p else (p, r)
            rq = (r, q) if r < q else (q, r)
            a[rp[0]][rp[1]], a[rq[0]][rq[1]] = _rotate(a[rp[0]][rp[1]], a[rq[0]][rq[1]], s, tau)
            for k in range(3):
                v[k][p], v[k][q] = _rotate(v[k][p], v[k][q], s, tau)
    else:
        sweeps = SWEEP_CAP + 1  # never converged: the tests assert this does not happen
    return [a[0][0], a[1][1], a[2][2]], v, sweeps


def determinant(v):
    """D4's operation order; v[r][c]."""
    m0 = v[1][1] * v[2][2]
    m0 = m0 - v[1][2] * v[2][1]
    m1 = v[1][0] * v[2][2]
    m1 = m1 - v[1][2] * v[2][0]
    m2 = v[1][0] * v[2][1]
    m2 = m2 - v[1][1] * v[2][0]
    det = v[0][0] * m0
    det = det - v[0][1] * m1
    det = det + v[0][2] * m2
    return det


def _identity():
    return [[ONE, ZERO, ZERO], [ZERO, ONE, ZERO], [ZERO, ZERO, ONE]]


def decompose(p):
    with np.errstate(all="ignore"):
        c = covariance_matrix(p)
        if not all(_finite(x) for x in c):  # D2
            lam, v, status, sweeps = [ONE, ONE, ONE], _identity(), STATUS_NON_FINITE, 0
        else:
            lam, v, sweeps = jacobi(c)
            status = STATUS_DECOMPOSED
            # D3 order: ascending, equal values keep the order of their diagonal positions (adjacent strict swaps)
            for i, j in ((0, 1), (1, 2), (0, 1)):
                if lam[j] < lam[i]:
                    lam[i], lam[j] = lam[j], lam[i]
                    for k in range(3):
                        v[k][i], v[k][j] = v[k][j], v[k][i]
        det = determinant(v)  # D4
        if det < ZERO:
            for k in range(3):
                v[k][0] = -v[k][0]
        elif det == ZERO:
            v = _identity()
        scale = []  # D5
        for i in range(3):
            e = abs(lam[i])
            scale.append(np.sqrt(e) if e > SCALE_EPSILON else e)
        index = 0  # D6
        for i in range(3):
            if lam[i] < lam[index]:
                index = i
        n = [v[0][index], v[1][index], v[2][index]]
        length2 = n[0] * n[0]
        length2 = length2 + n[1] * n[1]
        length2 = length2 + n[2] * n[2]
        if length2 > ZERO:
            length = np.sqrt(length2)
            n = [n[0] / length, n[1] / length, n[2] / length]
    eigenvectors = np.array([v[r][c_] for c_ in range(3) for r in range(3)], dtype=np.float64)  # column-major
    return Decomposition(np.array(lam, dtype=np.float64), eigenvectors, status, sweeps,
                         np.array(scale, dtype=np.float64), np.array(n, dtype=np.float64))


def normal_for_up(d, up):
    """The heightmap's part of D6: `up` is the up axis normal (a signed unit axis); float32[3]."""
    u = [F(x) for x in up]
    n = [F(x) for x in d.normal]
    dot = n[0] * u[0]
    dot = dot + n[1] * u[1]
    dot = dot + n[2] * u[2]
    flip = ONE if dot >= ZERO else -ONE
    with np.errstate(all="ignore"):
        return np.array([np.float32(n[0] * flip), np.float32(n[1] * flip), np.float32(n[2] * flip)], dtype=np.float32)

