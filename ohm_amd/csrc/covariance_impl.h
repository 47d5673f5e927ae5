// covariance_impl.h -- host side of the covariance decomposition (covariance_kernels.h, covariance_eigen_device.h):
// by key on the device map, and on the host for covariances the caller already holds.  The voxels are fetched by the
// voxel read's own code (neighbours_impl.h: readVoxelsRefusal, readVoxelsDevice), so the map is observed exactly as
// ohmhip_map_read_voxels observes it.  The ellipsoid cloud is the occupancy cloud (cloud_impl.h: its refusal, work list,
// count-and-scan and emit, unchanged) followed by a decomposition at the keys it emitted.  Included at the end of
// ohmhip_map.hip's translation unit, after voxel_edit_impl.h.
#ifndef OHMHIP_COVARIANCE_IMPL_H
#define OHMHIP_COVARIANCE_IMPL_H

namespace
{
/// What both entry points check before any device work.
int covarianceEigenRefusal(ohmhip_map_t m, const void *keys, size_t count, const void *eigenvalues,
                           const void *eigenvectors, const void *status)
{
  if (!m || (count && (!eigenvalues || !eigenvectors)))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return readVoxelsRefusal(m, OHMHIP_LID_COVARIANCE, keys, count, eigenvalues, status);
}

/// Read and decompose on device arrays, enqueued on the map's stream; the map is settled.
int covarianceEigenDevice(ohmhip_map_t m, const GpuKeyOut *d_keys, uint32_t count, double *d_eigenvalues,
                          double *d_eigenvectors, uint8_t *d_status)
{
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  OHMHIP_CHECK(qs.cov_voxels.ensure(kLayerBytes[OHMHIP_LID_COVARIANCE] * size_t(count), false, s));
  OHMHIP_CHECK(qs.cov_present.ensure(count, false, s));
  OHMHIP_CHECK(readVoxelsDevice(m, OHMHIP_LID_COVARIANCE, d_keys, count, qs.cov_voxels.ptr,
                                static_cast<uint8_t *>(qs.cov_present.ptr)));
  CovEigenArgs a{};
  a.covariance = static_cast<const float *>(qs.cov_voxels.ptr);
  a.present = static_cast<const uint8_t *>(qs.cov_present.ptr);
  a.n = count;
  a.eigenvalues = d_eigenvalues;
  a.eigenvectors = d_eigenvectors;
  a.status = d_status;
  hipLaunchKernelGGL(k_covariance_eigen, dim3((count + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}

/// What every ellipsoid entry point checks before any device work: the cloud's refusals, then its own.
int ellipsoidsRefusal(ohmhip_map_t m, const ohmhip_cloud_params *p, const uint64_t *count, uint64_t capacity,
                      const double *positions, const double *axes, const double *scales)
{
  OHMHIP_CHECK(cloudRefusal(m, p, count, capacity, positions));
  if (p->mode != OHMHIP_CLOUD_OCCUPANCY || (p->flags & (OHMHIP_CLOUD_EXPORT_FREE | OHMHIP_CLOUD_IGNORE_VOXEL_MEAN)))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (capacity > 0 && (!axes || !scales))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (!m->pool.layers[OHMHIP_LID_OCCUPANCY] || !m->pool.layers[OHMHIP_LID_MEAN] || !m->pool.layers[OHMHIP_LID_COVARIANCE])
  {
    return OHMHIP_ERR_UNSUPPORTED;  // ohm2ply refuses such a map (utils/ohm2ply/ohm2ply.cpp:863-873)
  }
  return OHMHIP_OK;
}

/// Axes and scales for the `rows` rows a cloud emit wrote keys for, enqueued on the map's stream.
int ellipsoidsDevice(ohmhip_map_t m, const GpuKeyOut *d_keys, uint64_t rows, const unsigned long long *d_total,
                     double *d_axes, double *d_scales)
{
  if (rows > uint64_t(0x7fffffff))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  const uint32_t n = uint32_t(rows);
  OHMHIP_CHECK(qs.cov_voxels.ensure(kLayerBytes[OHMHIP_LID_COVARIANCE] * size_t(n), false, s));
  OHMHIP_CHECK(qs.cov_present.ensure(n, false, s));
  OHMHIP_CHECK(readVoxelsDevice(m, OHMHIP_LID_COVARIANCE, d_keys, n, qs.cov_voxels.ptr,
                                static_cast<uint8_t *>(qs.cov_present.ptr)));
  CovEllipsoidArgs a{};
  a.covariance = static_cast<const float *>(qs.cov_voxels.ptr);
  a.n = n;
  a.total = d_total;
  a.axes = d_axes;
  a.scales = d_scales;
  hipLaunchKernelGGL(k_covariance_ellipsoids, dim3((n + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError();
}
}  // namespace

extern "C" {

int ohmhip_covariance_decompose(const float *covariance6, size_t count, double *eigenvalues, double *eigenvectors,
                                double *scales, double *normals, uint8_t *status)
try
{
  if (count && !covariance6)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  for (size_t i = 0; i < count; ++i)
  {
    const CovEigen e = covarianceEigen(covariance6 + 6 * i);
    for (int c = 0; c < 3; ++c)
    {
      if (eigenvalues)
      {
        eigenvalues[3 * i + c] = e.value[c];
      }
      if (scales)
      {
        scales[3 * i + c] = e.scale[c];
      }
      if (normals)
      {
        normals[3 * i + c] = e.normal[c];
      }
    }
    for (int c = 0; eigenvectors && c < 9; ++c)
    {
      eigenvectors[9 * i + c] = e.vector[c];
    }
    if (status)
    {
      status[i] = e.status;
    }
  }
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

int ohmhip_map_covariance_eigen(ohmhip_map_t m, const void *keys10, size_t count, double *eigenvalues,
                                double *eigenvectors, uint8_t *status)
try
{
  OHMHIP_CHECK(covarianceEigenRefusal(m, keys10, count, eigenvalues, eigenvectors, status));
  const GpuKeyOut *k = static_cast<const GpuKeyOut *>(keys10);
  for (size_t i = 0; i < count; ++i)
  {
    for (int c = 0; c < 3; ++c)
    {
      if (int(k[i].voxel[c]) >= m->mc.kdim[c])
      {
        return OHMHIP_ERR_INVALID_ARG;  // not a voxel of the map's regions
      }
    }
  }
  OHMHIP_SETTLE(m);
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  OHMHIP_CHECK(qs.rv_keys.ensure(sizeof(GpuKeyOut) * count, false, s));
  OHMHIP_CHECK(qs.cov_values.ensure(sizeof(double) * 3u * count, false, s));
  OHMHIP_CHECK(qs.cov_vectors.ensure(sizeof(double) * 9u * count, false, s));
  OHMHIP_CHECK(qs.cov_status.ensure(count, false, s));
  OHMHIP_CHECK(hipMemcpyAsync(qs.rv_keys.ptr, keys10, sizeof(GpuKeyOut) * count, hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(covarianceEigenDevice(m, static_cast<const GpuKeyOut *>(qs.rv_keys.ptr), uint32_t(count),
                                     static_cast<double *>(qs.cov_values.ptr), static_cast<double *>(qs.cov_vectors.ptr),
                                     static_cast<uint8_t *>(qs.cov_status.ptr)));
  OHMHIP_CHECK(hipMemcpyAsync(eigenvalues, qs.cov_values.ptr, sizeof(double) * 3u * count, hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipMemcpyAsync(eigenvectors, qs.cov_vectors.ptr, sizeof(double) * 9u * count, hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipMemcpyAsync(status, qs.cov_status.ptr, count, hipMemcpyDeviceToHost, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_covariance_eigen_device(ohmhip_map_t m, const void *d_keys10, size_t count, double *d_eigenvalues,
                                       double *d_eigenvectors, uint8_t *d_status)
try
{
  OHMHIP_CHECK(covarianceEigenRefusal(m, d_keys10, count, d_eigenvalues, d_eigenvectors, d_status));
  OHMHIP_SETTLE(m);
  return covarianceEigenDevice(m, static_cast<const GpuKeyOut *>(d_keys10), uint32_t(count), d_eigenvalues,
                               d_eigenvectors, d_status);
}
OHMHIP_ABI_CATCH

int ohmhip_map_covariance_ellipsoids_count(ohmhip_map_t m, const ohmhip_cloud_params *params, uint64_t *count)
try
{
  OHMHIP_CHECK(ellipsoidsRefusal(m, params, count, 0, nullptr, nullptr, nullptr));
  OHMHIP_SETTLE(m);
  CloudArgs a;
  std::vector<CloudChunk> chunks;
  return cloudCountHost(m, params, a, chunks, count);
}
OHMHIP_ABI_CATCH

int ohmhip_map_covariance_ellipsoids(ohmhip_map_t m, const ohmhip_cloud_params *params, uint64_t capacity,
                                     double *positions_xyz, double *axes9, double *scales3, void *keys10, float *values,
                                     uint64_t *count)
try
{
  OHMHIP_CHECK(ellipsoidsRefusal(m, params, count, capacity, positions_xyz, axes9, scales3));
  OHMHIP_SETTLE(m);
  CloudArgs a;
  std::vector<CloudChunk> chunks;
  OHMHIP_CHECK(cloudCountHost(m, params, a, chunks, count));
  const size_t n = size_t(std::min<uint64_t>(*count, capacity));
  if (n == 0)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  double *d_pos;
  float *d_values;
  OHMHIP_CHECK(stageOut(qs.cloud_pos, positions_xyz, 3 * n, s, d_pos));
  OHMHIP_CHECK(qs.cloud_keys.ensure(sizeof(GpuKeyOut) * n, false, s));  // the decomposition reads them: always staged
  GpuKeyOut *d_keys = static_cast<GpuKeyOut *>(qs.cloud_keys.ptr);
  OHMHIP_CHECK(stageOut(qs.cloud_values, values, n, s, d_values));
  OHMHIP_CHECK(qs.cov_vectors.ensure(sizeof(double) * 9u * n, false, s));
  OHMHIP_CHECK(qs.cov_values.ensure(sizeof(double) * 3u * n, false, s));
  double *d_axes = static_cast<double *>(qs.cov_vectors.ptr);
  double *d_scales = static_cast<double *>(qs.cov_values.ptr);
  OHMHIP_CHECK(cloudEmit(m, a, chunks.size(), n, d_pos, d_keys, d_values));
  OHMHIP_CHECK(ellipsoidsDevice(m, d_keys, n, nullptr, d_axes, d_scales));
  OHMHIP_CHECK(copyOut(positions_xyz, d_pos, 3 * n, s));
  OHMHIP_CHECK(copyOut(axes9, d_axes, 9 * n, s));
  OHMHIP_CHECK(copyOut(scales3, d_scales, 3 * n, s));
  OHMHIP_CHECK(copyOut(keys10, d_keys, n, s));
  OHMHIP_CHECK(copyOut(values, d_values, n, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_covariance_ellipsoids_device(ohmhip_map_t m, const ohmhip_cloud_params *params, uint64_t capacity,
                                            double *d_positions_xyz, double *d_axes9, double *d_scales3, void *d_keys10,
                                            float *d_values, uint64_t *d_count)
try
{
  OHMHIP_CHECK(ellipsoidsRefusal(m, params, d_count, capacity, d_positions_xyz, d_axes9, d_scales3));
  if (capacity > 0 && !d_keys10)
  {
    return OHMHIP_ERR_INVALID_ARG;  // the decomposition reads the keys where the caller receives them
  }
  if (capacity > uint64_t(0x7fffffff))
  {
    return OHMHIP_ERR_CAPACITY;  // every row of the arrays is a lane of the decomposition
  }
  OHMHIP_SETTLE(m);
  hipStream_t s = m->stream;
  OHMHIP_CHECK(hipStreamSynchronize(s));  // (the host mirror of the region table, and the work list's buffer)
  CloudArgs a;
  std::vector<CloudChunk> chunks;
  OHMHIP_CHECK(cloudWorkList(m, params, a, chunks));
  if (chunks.empty())
  {
    return hipMemsetAsync(d_count, 0, sizeof(uint64_t), s);
  }
  OHMHIP_CHECK(cloudCount(m, a, chunks));
  const unsigned long long *d_total = a.offsets + chunks.size() * kCloudWaves;
  if (capacity > 0)
  {
    // rows past the count are not emitted: zeroed there, so the read that precedes the decomposition sees defined keys
    OHMHIP_CHECK(hipMemsetAsync(d_keys10, 0, sizeof(GpuKeyOut) * size_t(capacity), s));
    OHMHIP_CHECK(cloudEmit(m, a, chunks.size(), capacity, d_positions_xyz, d_keys10, d_values));
    OHMHIP_CHECK(ellipsoidsDevice(m, static_cast<const GpuKeyOut *>(d_keys10), capacity, d_total, d_axes9, d_scales3));
  }
  return hipMemcpyAsync(d_count, d_total, sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_COVARIANCE_IMPL_H
