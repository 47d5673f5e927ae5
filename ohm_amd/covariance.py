"""Host-side mirrors of ohm's covariance helpers (ohm/CovarianceVoxel.h:33-67) for covariances the caller holds: the
decomposition rule D1-D6 of include/ohmhip.h evaluated on the host by the library (ohmhip_covariance_decompose: the text
the kernels compile), so a value computed here equals what GpuMap.covarianceEigen and the heightmap's surface normals
compute on the device.  P is (N, 6) or (6,) float32: CovarianceVoxel::trianglar_covariance."""
import collections

import numpy as np

from . import _lib as L

CovarianceDecomposition = collections.namedtuple("CovarianceDecomposition",
                                                 "eigenvalues eigenvectors scales normals status")


def covariance_decompose(P):
    """D1-D6 for every row of P: eigenvalues (N, 3) ascending, eigenvectors (N, 3, 3) with eigenvectors[i, c] the column
    of eigenvalue c after D4, scales (N, 3) (D5), normals (N, 3) (D6, before a heightmap's flip), status (N,) uint8 (1
    decomposed, 2 non-finite).  All float64."""
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 6)
    n = P.shape[0]
    values, vectors = np.zeros((n, 3)), np.zeros((n, 3, 3))
    scales, normals = np.zeros((n, 3)), np.zeros((n, 3))
    status = np.zeros(n, dtype=np.uint8)
    L.check(L.lib.ohmhip_covariance_decompose(P.ctypes.data, n, values.ctypes.data, vectors.ctypes.data,
                                              scales.ctypes.data, normals.ctypes.data, status.ctypes.data),
            "covariance_decompose")
    return CovarianceDecomposition(values, vectors, scales, normals, status)


def covariance_estimate_primary_normal(P):
    """covarianceEstimatePrimaryNormal with preferred_axis 0 (ohm/CovarianceVoxel.cpp:157-177): (N, 3) float64."""
    return covariance_decompose(P).normals


def rotation_to_quaternion(R):
    """The unit quaternion (w, x, y, z) of rotation matrices R (N, 3, 3), R[i, r, c] row r column c, by Shepperd's
    method: of 4w^2 = 1 + R00 + R11 + R22, 4x^2 = 1 + R00 - R11 - R22, 4y^2 = 1 - R00 + R11 - R22 and 4z^2 = 1 - R00 -
    R11 + R22 the largest (the first among equals) gives its component as sqrt(.) / 2, and the other three are the
    matching sums or differences of off-diagonal pairs -- R21 - R12, R02 - R20, R10 - R01 against w; R01 + R10, R02 +
    R20, R12 + R21 among x, y, z -- divided by four times it.  No division by a small number for any rotation."""
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    q = np.zeros((R.shape[0], 4))
    for i, m in enumerate(R):
        four = [1.0 + m[0, 0] + m[1, 1] + m[2, 2], 1.0 + m[0, 0] - m[1, 1] - m[2, 2],
                1.0 - m[0, 0] + m[1, 1] - m[2, 2], 1.0 - m[0, 0] - m[1, 1] + m[2, 2]]
        k = int(np.argmax(four))
        big = 0.5 * np.sqrt(max(four[k], 0.0))
        f = 0.25 / big
        wx, wy, wz = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]
        xy, xz, yz = m[0, 1] + m[1, 0], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1]
        q[i] = ((big, wx * f, wy * f, wz * f), (wx * f, big, xy * f, xz * f), (wy * f, xy * f, big, yz * f),
                (wz * f, xz * f, yz * f, big))[k]
    return q


def quaternion_to_rotation(q):
    """The rotation matrices (N, 3, 3) of unit quaternions (w, x, y, z)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def covariance_unit_sphere_transformation(P):
    """covarianceUnitSphereTransformation (ohm/CovarianceVoxel.cpp:180-206): the rotation, as quaternions (N, 4) in
    (w, x, y, z) order built from the D4 matrix by rotation_to_quaternion, and the scale (N, 3) of D5 that deform a unit
    sphere into the covariance's ellipsoid (scale first, then rotate)."""
    d = covariance_decompose(P)
    # eigenvectors[i, c, r] is column-major storage: the matrix with rows r is its transpose
    return rotation_to_quaternion(np.transpose(d.eigenvectors, (0, 2, 1))), d.scales
