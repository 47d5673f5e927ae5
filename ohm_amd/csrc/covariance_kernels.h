// covariance_kernels.h -- the covariance decomposition (covariance_eigen_device.h) over voxels read by key.
//
//   k_covariance_eigen       1 lane / key   eigenvalues, eigenvectors and a status byte from the voxel k_read_voxels
//                                           fetched
//   k_covariance_ellipsoids  1 lane / row   axes (D4) and scales (D5) for the rows a cloud call emitted, from the voxels
//                                           k_read_voxels fetched at the emitted keys
//
// The voxels come from k_read_voxels (neighbours_kernels.h), so the map is observed exactly as ohmhip_map_read_voxels
// observes it; this kernel never sees the map.  No LDS, and no divergence beyond the solver's own tests.
#ifndef OHMHIP_COVARIANCE_KERNELS_H
#define OHMHIP_COVARIANCE_KERNELS_H

#include "covariance_eigen_device.h"

namespace ohmhip
{
struct CovEigenArgs
{
  const float *covariance;  ///< [n][6]: the covariance layer's voxels as k_read_voxels wrote them
  const uint8_t *present;   ///< [n]: k_read_voxels' present flags
  uint32_t n;
  double *eigenvalues;      ///< [n][3]
  double *eigenvectors;     ///< [n][9]
  uint8_t *status;          ///< [n]
};

__global__ void __launch_bounds__(256) k_covariance_eigen(CovEigenArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n)
  {
    return;
  }
  double *values = a.eigenvalues + size_t(i) * 3u;
  double *vectors = a.eigenvectors + size_t(i) * 9u;
  if (!a.present[i])
  {
    // the map holds no such region, or the key names no voxel: nothing to decompose
    for (int c = 0; c < 3; ++c)
    {
      values[c] = 0.0;
    }
    for (int c = 0; c < 9; ++c)
    {
      vectors[c] = 0.0;
    }
    a.status[i] = kCovAbsent;
    return;
  }
  float p[6];
  for (int c = 0; c < 6; ++c)
  {
    p[c] = a.covariance[size_t(i) * 6u + c];
  }
  const CovEigen e = covarianceEigen(p);
  for (int c = 0; c < 3; ++c)
  {
    values[c] = e.value[c];
  }
  for (int c = 0; c < 9; ++c)
  {
    vectors[c] = e.vector[c];
  }
  a.status[i] = e.status;
}

struct CovEllipsoidArgs
{
  const float *covariance;          ///< [n][6]: the covariance voxels at the cloud's keys
  uint32_t n;                       ///< rows the arrays hold
  const unsigned long long *total;  ///< device variant: the cloud's count on the device -- rows past it are not written
  double *axes;                     ///< [n][9] column-major rotation (D4)
  double *scales;                   ///< [n][3] (D5)
};

__global__ void __launch_bounds__(256) k_covariance_ellipsoids(CovEllipsoidArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n || (a.total && (unsigned long long)i >= *a.total))
  {
    return;
  }
  float p[6];
  for (int c = 0; c < 6; ++c)
  {
    p[c] = a.covariance[size_t(i) * 6u + c];
  }
  const CovEigen e = covarianceEigen(p);
  for (int c = 0; c < 9; ++c)
  {
    a.axes[size_t(i) * 9u + c] = e.vector[c];
  }
  for (int c = 0; c < 3; ++c)
  {
    a.scales[size_t(i) * 3u + c] = e.scale[c];
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_COVARIANCE_KERNELS_H
