// covariance_eigen_device.h -- the covariance decomposition rule D1-D6 (include/ohmhip.h): the
// eigenvalues and eigenvectors of C = S S^T for the six floats of a CovarianceVoxel, by a cyclic Jacobi in fp64, and
// what ohm derives from them -- the rotation of covarianceUnitSphereTransformation, its scale, and the primary normal
// (ohm/CovarianceVoxel.cpp:147-206).  One voxel per lane, registers only.  Every operation is one of + - * / sqrt, a
// compare or a select, each correctly rounded on gfx950 and on the host, and the unit is compiled with
// -ffp-contract=off: tests/covariance_eigen_ref.py restates the function one operation per line and equals it bit for
// bit.  Host and device compile the same text (ohmhip_covariance_decompose runs it on the host).
#ifndef OHMHIP_COVARIANCE_EIGEN_DEVICE_H
#define OHMHIP_COVARIANCE_EIGEN_DEVICE_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ohmhip
{
constexpr int kCovSweepCap = 16;  ///< D3: no case of tests/covariance_cases.py rotates in more than 6 sweeps
constexpr uint8_t kCovAbsent = 0, kCovDecomposed = 1, kCovNonFinite = 2;  ///< OHMHIP_COV_*

struct CovEigen
{
  double value[3];    ///< ascending (D3)
  double vector[9];   ///< column-major: vector[3 * c + r], after D4
  double scale[3];    ///< D5
  double normal[3];   ///< D6, before the heightmap's flip
  uint8_t status;     ///< kCovDecomposed or kCovNonFinite
};

__host__ __device__ inline double covAbs(double x)
{
  return __builtin_fabs(x);
}

/// (g, h) -> (g - s (h + g tau), h + s (g - h tau)): the Jacobi rotation in Rutishauser's form
__host__ __device__ inline void covRotate(double &g, double &h, double s, double tau)
{
  const double g0 = g, h0 = h;
  g = g0 - s * (h0 + g0 * tau);
  h = h0 + s * (g0 - h0 * tau);
}

/// One Jacobi rotation annihilating apq; arp / arq are the third index's entries against p and q, vp / vq columns p
/// and q of V (three rows each, stride 3 in the column-major store).  `sweep` gates the small-off-diagonal cut-off.
__host__ __device__ inline void covJacobiPair(int sweep, double &app, double &aqq, double &apq, double &arp, double &arq,
                                              double *vp, double *vq)
{
  if (apq == 0.0)
  {
    return;
  }
  const double g = 100.0 * covAbs(apq);
  if (sweep >= 3 && covAbs(app) + g == covAbs(app) && covAbs(aqq) + g == covAbs(aqq))
  {
    apq = 0.0;  // the rotation would change neither diagonal entry
    return;
  }
  double h = aqq - app;
  double t;
  if (covAbs(h) + g == covAbs(h))
  {
    t = apq / h;
  }
  else
  {
    const double theta = (0.5 * h) / apq;
    t = 1.0 / (covAbs(theta) + __builtin_sqrt(theta * theta + 1.0));
    t = (theta < 0.0) ? -t : t;
  }
  const double c = 1.0 / __builtin_sqrt(t * t + 1.0);
  const double s = t * c;
  const double tau = s / (1.0 + c);
  h = t * apq;
  app = app - h;
  aqq = aqq + h;
  apq = 0.0;
  covRotate(arp, arq, s, tau);
  covRotate(vp[0], vq[0], s, tau);
  covRotate(vp[1], vq[1], s, tau);
  covRotate(vp[2], vq[2], s, tau);
}

__host__ __device__ inline void covSwapIfLess(double *value, double *vector, int i, int j)
{
  if (value[j] < value[i])
  {
    double t = value[i];
    value[i] = value[j];
    value[j] = t;
    for (int r = 0; r < 3; ++r)
    {
      t = vector[3 * i + r];
      vector[3 * i + r] = vector[3 * j + r];
      vector[3 * j + r] = t;
    }
  }
}

__host__ __device__ inline void covIdentity(double *vector)
{
  for (int i = 0; i < 9; ++i)
  {
    vector[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
}

/// D1-D6 for the six floats p of one CovarianceVoxel.
__host__ __device__ inline CovEigen covarianceEigen(const float *p)
{
  CovEigen e;
  // D1: S rows (p0, 0, 0), (p1, p2, 0), (p3, p4, p5); each entry of C summed left to right
  const double p0 = double(p[0]), p1 = double(p[1]), p2 = double(p[2]), p3 = double(p[3]), p4 = double(p[4]),
               p5 = double(p[5]);
  double a00 = p0 * p0;
  double a01 = p0 * p1;
  double a02 = p0 * p3;
  double a11 = p1 * p1 + p2 * p2;
  double a12 = p1 * p3 + p2 * p4;
  double a22 = (p3 * p3 + p4 * p4) + p5 * p5;
  double *v = e.vector;
  covIdentity(v);
  const double dbl_max = 1.7976931348623157e308;
  const bool finite = covAbs(a00) <= dbl_max && covAbs(a01) <= dbl_max && covAbs(a02) <= dbl_max &&
                      covAbs(a11) <= dbl_max && covAbs(a12) <= dbl_max && covAbs(a22) <= dbl_max;
  if (!finite)
  {
    // D2: the Eigen build's answer when its solver does not report success (CovarianceVoxel.cpp:58-65)
    e.value[0] = e.value[1] = e.value[2] = 1.0;
    e.status = kCovNonFinite;
  }
  else
  {
    // D3: cyclic Jacobi over (0,1), (0,2), (1,2) until the off-diagonal sum is exactly zero
    for (int sweep = 0; sweep < kCovSweepCap; ++sweep)
    {
      const double off = (covAbs(a01) + covAbs(a02)) + covAbs(a12);
      if (off == 0.0)
      {
        break;
      }
      covJacobiPair(sweep, a00, a11, a01, a02, a12, v + 0, v + 3);
      covJacobiPair(sweep, a00, a22, a02, a01, a12, v + 0, v + 6);
      covJacobiPair(sweep, a11, a22, a12, a01, a02, v + 3, v + 6);
    }
    e.value[0] = a00;
    e.value[1] = a11;
    e.value[2] = a22;
    // ascending; adjacent strict swaps keep equal values in the order of their diagonal positions
    covSwapIfLess(e.value, v, 0, 1);
    covSwapIfLess(e.value, v, 1, 2);
    covSwapIfLess(e.value, v, 0, 1);
    e.status = kCovDecomposed;
  }
  // D4 (:66-74, :187-195), V(r, c) = v[3 * c + r]: cofactors along row 0
  const double m0 = v[4] * v[8] - v[7] * v[5];
  const double m1 = v[1] * v[8] - v[7] * v[2];
  const double m2 = v[1] * v[5] - v[4] * v[2];
  const double det = (v[0] * m0 - v[3] * m1) + v[6] * m2;
  if (det < 0.0)
  {
    v[0] = -v[0];
    v[1] = -v[1];
    v[2] = -v[2];
  }
  else if (det == 0.0)
  {
    covIdentity(v);
  }
  // D5 (:198-203)
  for (int i = 0; i < 3; ++i)
  {
    const double eval = covAbs(e.value[i]);
    e.scale[i] = (eval > 1e-9) ? __builtin_sqrt(eval) : eval;
  }
  // D6 (:164-175), preferred_axis 0
  int index = 0;
  for (int i = 0; i < 3; ++i)
  {
    index = (e.value[i] < e.value[index]) ? i : index;
  }
  // (selects, not an indexed read: the arrays stay in registers)
  const double nx = (index == 0) ? v[0] : (index == 1) ? v[3] : v[6];
  const double ny = (index == 0) ? v[1] : (index == 1) ? v[4] : v[7];
  const double nz = (index == 0) ? v[2] : (index == 1) ? v[5] : v[8];
  const double length2 = (nx * nx + ny * ny) + nz * nz;
  const double length = __builtin_sqrt(length2);
  e.normal[0] = (length2 > 0.0) ? nx / length : nx;
  e.normal[1] = (length2 > 0.0) ? ny / length : ny;
  e.normal[2] = (length2 > 0.0) ? nz / length : nz;
  return e;
}

/// The heightmap's part of D6 (ohmheightmap/Heightmap.cpp:820-825): the normal turned towards `up`, as floats.
__host__ __device__ inline void covarianceSurfaceNormal(const CovEigen &e, const double up[3], float out[3])
{
  const double dot = (e.normal[0] * up[0] + e.normal[1] * up[1]) + e.normal[2] * up[2];
  const double flip = (dot >= 0.0) ? 1.0 : -1.0;
  out[0] = float(e.normal[0] * flip);
  out[1] = float(e.normal[1] * flip);
  out[2] = float(e.normal[2] * flip);
}
}  // namespace ohmhip

#endif  // OHMHIP_COVARIANCE_EIGEN_DEVICE_H
