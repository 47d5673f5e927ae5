// point_filter_impl.h -- host side of the point filter (point_filter_kernels.h): argument checks, the map as the kernels
// see it with its three layers, classify, scan (read_side.h: countAndScan) and emit on the map's stream; the host
// variant's pieces.  Included at the end of ohmhip_map.hip's translation unit, after neighbours_impl.h.
#ifndef OHMHIP_POINT_FILTER_IMPL_H
#define OHMHIP_POINT_FILTER_IMPL_H

namespace
{
/// Points one launch takes: the grid stays below 2^31 workgroups.
constexpr uint64_t kPfMaxLaunchPoints = uint64_t(1) << 36;

/// What both entry points check before any device work.
int pointFilterRefusal(ohmhip_map_t m, const double *points, uint64_t stride, uint64_t count,
                       const ohmhip_point_filter_params *p, uint64_t capacity, const void *kept_indices, const void *kept,
                       bool host_points)
{
  if (!m || !p || !kept || (count && !points) || stride < 3 || (capacity > 0 && !kept_indices))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if ((p->flags & ~uint32_t(OHMHIP_PF_OCCUPANCY_ONLY)) != 0u || std::isnan(p->expected_value_tolerance))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (host_points)
  {
    for (uint64_t i = 0; i < 3 * count; ++i)
    {
      if (!std::isfinite(points[i]))
      {
        return OHMHIP_ERR_INVALID_ARG;
      }
    }
  }
  return readSideRefusal(m, OHMHIP_LID_OCCUPANCY);  // (ohmfilter refuses a map without the layer too: ohmfilter.cpp:178-182)
}

/// The kernel arguments that do not depend on the points: the read view with the mean and covariance layers beside
/// the occupancy layer, and which filter the layers and the parameters select (ohmfilter.cpp:187-221).  The map is
/// settled.
int pointFilterView(ohmhip_map_t m, const ohmhip_point_filter_params *p, PointFilterArgs &a)
{
  OHMHIP_CHECK(mapReadView(m, a));
  const bool layers = m->pool.layers[OHMHIP_LID_MEAN] && m->pool.layers[OHMHIP_LID_COVARIANCE];
  a.test = (!(p->flags & OHMHIP_PF_OCCUPANCY_ONLY) && layers && p->expected_value_tolerance >= 0) ? 1 : 0;
  a.limit = 3.0 + p->expected_value_tolerance;
  a.mean = layerView(m, OHMHIP_LID_MEAN, a.test);
  a.covariance = layerView(m, OHMHIP_LID_COVARIANCE, a.test);
  return OHMHIP_OK;
}

/// Classify and scan `n` points on the map's stream.  Afterwards a.offsets is the scan and *d_total points at the
/// number of kept points (device memory).  a.status must be set.
int pointFilterClassify(ohmhip_map_t m, PointFilterArgs &a, uint64_t n, const unsigned long long **d_total)
{
  hipStream_t s = m->stream;
  const uint32_t blocks = uint32_t((n + 255u) / 256u);
  CountScan cs;
  const int err = countAndScan(m->query.pf_scan, size_t(blocks) * 4, s, cs, [&] {
    a.n = n;
    a.counts = cs.counts;
    a.offsets = cs.offsets;
    hipLaunchKernelGGL(k_pf_classify, dim3(blocks), dim3(256), 0, s, a);
  });
  *d_total = cs.total;
  return err;
}

int pointFilterEmit(ohmhip_map_t m, const PointFilterArgs &a)
{
  hipLaunchKernelGGL(k_pf_emit, dim3(uint32_t((a.n + 255u) / 256u)), dim3(256), 0, m->stream, a);
  return hipGetLastError();
}
}  // namespace

extern "C" {

int ohmhip_map_filter_points(ohmhip_map_t m, const double *points_xyz, uint64_t count,
                             const ohmhip_point_filter_params *params, uint64_t capacity, uint8_t *status,
                             uint64_t *kept_indices, double *values, void *keys10, uint64_t *kept)
try
{
  OHMHIP_CHECK(pointFilterRefusal(m, points_xyz, 3, count, params, capacity, kept_indices, kept, true));
  *kept = 0;
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_SETTLE(m);
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  PointFilterArgs a{};
  OHMHIP_CHECK(pointFilterView(m, params, a));
  const uint64_t piece = OHMHIP_PF_PIECE_POINTS;
  const size_t most = size_t(std::min<uint64_t>(piece, count));
  const size_t piece_bytes = sizeof(double) * 3 * size_t(piece);
  if (!qs.pf_staging.ptr)
  {
    // two pieces of points and one word for the piece's kept count
    OHMHIP_CHECK(qs.pf_staging.alloc(2 * piece_bytes + sizeof(unsigned long long), hipHostMallocDefault));
  }
  OHMHIP_CHECK(qs.pf_points.ensure(sizeof(double) * 3 * most, false, s));
  OHMHIP_CHECK(qs.pf_status.ensure(most, false, s));
  OHMHIP_CHECK(stageOut(qs.pf_values, values, most, s, a.values));
  OHMHIP_CHECK(stageOut(qs.pf_keys, keys10, most, s, a.keys));
  if (capacity > 0)
  {
    OHMHIP_CHECK(qs.pf_kept.ensure(sizeof(unsigned long long) * size_t(std::min<uint64_t>(capacity, most)), false, s));
  }
  char *staging = qs.pf_staging.get();
  unsigned long long *h_total = reinterpret_cast<unsigned long long *>(staging + 2 * piece_bytes);
  a.points = static_cast<const double *>(qs.pf_points.ptr);
  a.stride = 3;
  a.status = static_cast<uint8_t *>(qs.pf_status.ptr);
  a.capacity = capacity;
  a.kept = static_cast<unsigned long long *>(qs.pf_kept.ptr);
  OHMHIP_CHECK(hipStreamSynchronize(s));  // (an earlier call's copies out of the staging block)
  auto stage = [&](uint64_t at, int half) {
    std::memcpy(staging + size_t(half) * piece_bytes, points_xyz + 3 * at,
                sizeof(double) * 3 * size_t(std::min<uint64_t>(piece, count - at)));
  };
  stage(0, 0);
  uint64_t kept_so_far = 0;
  int half = 0;
  for (uint64_t at = 0; at < count; at += piece, half ^= 1)
  {
    const size_t n = size_t(std::min<uint64_t>(piece, count - at));
    OHMHIP_CHECK(hipMemcpyAsync(qs.pf_points.ptr, staging + size_t(half) * piece_bytes, sizeof(double) * 3 * n,
                                hipMemcpyHostToDevice, s));
    a.first_index = at;
    a.first_slot = kept_so_far;
    const unsigned long long *d_total = nullptr;
    OHMHIP_CHECK(pointFilterClassify(m, a, n, &d_total));
    OHMHIP_CHECK(hipMemcpyAsync(h_total, d_total, sizeof(*h_total), hipMemcpyDeviceToHost, s));
    if (at + piece < count)
    {
      stage(at + piece, half ^ 1);  // (the next piece, while the device works on this one)
    }
    OHMHIP_CHECK(hipStreamSynchronize(s));
    const uint64_t piece_kept = *h_total;
    const uint64_t fetch = (kept_so_far < capacity) ? std::min<uint64_t>(piece_kept, capacity - kept_so_far) : 0;
    if (fetch)
    {
      OHMHIP_CHECK(pointFilterEmit(m, a));
      OHMHIP_CHECK(hipMemcpyAsync(kept_indices + kept_so_far, a.kept, sizeof(uint64_t) * size_t(fetch), hipMemcpyDeviceToHost, s));
    }
    OHMHIP_CHECK(copyOut(status ? status + at : nullptr, a.status, n, s));
    OHMHIP_CHECK(copyOut(values ? values + at : nullptr, a.values, n, s));
    OHMHIP_CHECK(copyOut(keys10 ? static_cast<GpuKeyOut *>(keys10) + at : nullptr, a.keys, n, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));
    kept_so_far += piece_kept;
  }
  *kept = kept_so_far;
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

int ohmhip_map_filter_points_device(ohmhip_map_t m, const double *d_points, uint64_t stride_doubles, uint64_t count,
                                    const ohmhip_point_filter_params *params, uint64_t capacity, uint8_t *d_status,
                                    uint64_t *d_kept_indices, double *d_values, void *d_keys10, uint64_t *d_kept)
try
{
  OHMHIP_CHECK(pointFilterRefusal(m, d_points, stride_doubles, count, params, capacity, d_kept_indices, d_kept, false));
  if (count > kPfMaxLaunchPoints)
  {
    return OHMHIP_ERR_CAPACITY;
  }
  OHMHIP_SETTLE(m);
  hipStream_t s = m->stream;
  if (count == 0)
  {
    return hipMemsetAsync(d_kept, 0, sizeof(uint64_t), s);
  }
  ohmhip_map_s::QueryState &qs = m->query;
  PointFilterArgs a{};
  OHMHIP_CHECK(pointFilterView(m, params, a));
  if (!d_status)
  {
    OHMHIP_CHECK(qs.pf_status.ensure(size_t(count), false, s));  // (the emit pass reads it)
  }
  a.points = d_points;
  a.stride = stride_doubles;
  a.status = d_status ? d_status : static_cast<uint8_t *>(qs.pf_status.ptr);
  a.values = d_values;
  a.keys = static_cast<GpuKeyOut *>(d_keys10);
  a.capacity = capacity;
  a.kept = reinterpret_cast<unsigned long long *>(d_kept_indices);
  const unsigned long long *d_total = nullptr;
  OHMHIP_CHECK(pointFilterClassify(m, a, count, &d_total));
  if (capacity > 0)
  {
    OHMHIP_CHECK(pointFilterEmit(m, a));
  }
  return hipMemcpyAsync(d_kept, d_total, sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_POINT_FILTER_IMPL_H
