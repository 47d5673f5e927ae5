// query_impl.h -- host side of the read-only queries (query_kernels.h): the line-keys query and the rays query with its
// two entry points.  Included at the end of ohmhip_map.hip's translation unit, after read_side.h (mapReadView, the
// refusal, the optional outputs).
#ifndef OHMHIP_QUERY_IMPL_H
#define OHMHIP_QUERY_IMPL_H

extern "C" {

int ohmhip_map_line_keys(ohmhip_map_t m, const double *lines, size_t line_count, uint32_t max_keys_per_line,
                         void *keys_out, uint32_t *counts_out)
try
{
  if (!m || (line_count && (!lines || !keys_out || !counts_out)) || max_keys_per_line == 0)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (line_count == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_CHECK(settleLaunch(m));  // (the query shares the map's stream and reads its configuration)
  hipStream_t s = m->stream;
  const size_t key_bytes = sizeof(GpuKeyOut) * line_count * size_t(max_keys_per_line);
  DevArray<double> d_lines;
  DevArray<GpuKeyOut> d_keys;
  DevArray<uint32_t> d_counts;
  OHMHIP_CHECK(d_lines.alloc(sizeof(double) * 6 * line_count));
  OHMHIP_CHECK(d_keys.alloc(key_bytes));
  OHMHIP_CHECK(d_counts.alloc(sizeof(uint32_t) * line_count));
  int status = hipMemcpyAsync(d_lines, lines, sizeof(double) * 6 * line_count, hipMemcpyHostToDevice, s);
  if (!status)
  {
    hipLaunchKernelGGL(k_line_keys, dim3(uint32_t((line_count + 255) / 256)), dim3(256), 0, s, m->mc, d_lines,
                       uint32_t(line_count), max_keys_per_line, d_keys, d_counts);
    status = hipMemcpyAsync(keys_out, d_keys, key_bytes, hipMemcpyDeviceToHost, s);
  }
  if (!status)
  {
    status = hipMemcpyAsync(counts_out, d_counts, sizeof(uint32_t) * line_count, hipMemcpyDeviceToHost, s);
  }
  if (!status)
  {
    status = hipStreamSynchronize(s);
  }
  return status;
}
OHMHIP_ABI_CATCH

}  // extern "C"

namespace
{
/// What both query entry points check before any device work (OHMHIP_ERR_INVALID_ARG / OHMHIP_ERR_UNSUPPORTED).
int raysQueryRefusal(ohmhip_map_t m, const void *rays, size_t element_count, const void *ranges,
                     const void *unobserved_volumes, const void *terminal_types)
{
  const size_t n = element_count / 2;
  if (!m || (n && (!rays || !ranges || !unobserved_volumes || !terminal_types)) || n > size_t(0x7fffffff))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return readSideRefusal(m, OHMHIP_LID_OCCUPANCY);  // (the CPU query refuses maps without the layer too: valid_layers)
}

/// The query on device arrays, enqueued on the map's stream.  The map is observed as ohmhip_map_read_regions would
/// observe it: collected rays launched and an asynchronous launch settled first (the caller's OHMHIP_SETTLE), regions
/// of the host store included.  It changes nothing of the map: no voxel, dirty bit, residency, use stamp or counter.
int raysQueryDevice(ohmhip_map_t m, const double *d_rays, uint32_t n, double coef, double *d_ranges, double *d_volumes,
                    int8_t *d_types, GpuKeyOut *d_keys)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  RaysQueryArgs a;
  OHMHIP_CHECK(mapReadView(m, a));
  if (n == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_CHECK(qs.walked.ensure(sizeof(int32_t) * n, false, s));
  OHMHIP_CHECK(qs.last_walked.ensure(sizeof(int32_t) * n, false, s));
  size_t scan_bytes = 0;
  int32_t *walked = static_cast<int32_t *>(qs.walked.ptr);
  int32_t *last_walked = static_cast<int32_t *>(qs.last_walked.ptr);
  OHMHIP_CHECK(rocprim::inclusive_scan(nullptr, scan_bytes, walked, last_walked, size_t(n), rocprim::maximum<int32_t>(), s));
  OHMHIP_CHECK(qs.scan_temp.ensure(scan_bytes, false, s));
  a.rays = d_rays;
  a.n_rays = n;
  a.coef = coef;
  a.ranges = d_ranges;
  a.volumes = d_volumes;
  a.types = d_types;
  a.keys = d_keys;
  a.walked = walked;
  hipLaunchKernelGGL(k_rays_query, dim3((n + 255) / 256), dim3(256), 0, s, a);
  OHMHIP_CHECK(hipGetLastError());
  OHMHIP_CHECK(rocprim::inclusive_scan(qs.scan_temp.ptr, scan_bytes, walked, last_walked, size_t(n),
                                       rocprim::maximum<int32_t>(), s));
  hipLaunchKernelGGL(k_rays_query_carry, dim3((n + 255) / 256), dim3(256), 0, s, d_types, d_keys,
                     static_cast<const int32_t *>(last_walked), n);
  return hipGetLastError();
}
}  // namespace

extern "C" {

int ohmhip_map_rays_query(ohmhip_map_t m, const double *rays, size_t element_count, double volume_coefficient,
                          double *ranges, double *unobserved_volumes, int8_t *terminal_types, void *terminal_keys)
try
{
  OHMHIP_CHECK(raysQueryRefusal(m, rays, element_count, ranges, unobserved_volumes, terminal_types));
  OHMHIP_SETTLE(m);
  const uint32_t n = uint32_t(element_count / 2);
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  double *d_ranges = nullptr, *d_volumes = nullptr;
  int8_t *d_types = nullptr;
  GpuKeyOut *d_keys = nullptr;
  if (n)
  {
    OHMHIP_CHECK(qs.rays.ensure(sizeof(double) * 6 * n, false, s));
    OHMHIP_CHECK(stageOut(qs.ranges, ranges, n, s, d_ranges));
    OHMHIP_CHECK(stageOut(qs.volumes, unobserved_volumes, n, s, d_volumes));
    OHMHIP_CHECK(stageOut(qs.types, terminal_types, n, s, d_types));
    OHMHIP_CHECK(stageOut(qs.keys, terminal_keys, n, s, d_keys));
    OHMHIP_CHECK(hipMemcpyAsync(qs.rays.ptr, rays, sizeof(double) * 6 * n, hipMemcpyHostToDevice, s));
  }
  OHMHIP_CHECK(raysQueryDevice(m, static_cast<const double *>(qs.rays.ptr), n, volume_coefficient, d_ranges, d_volumes,
                               d_types, d_keys));
  if (n)
  {
    OHMHIP_CHECK(copyOut(ranges, d_ranges, n, s));
    OHMHIP_CHECK(copyOut(unobserved_volumes, d_volumes, n, s));
    OHMHIP_CHECK(copyOut(terminal_types, d_types, n, s));
    OHMHIP_CHECK(copyOut(terminal_keys, d_keys, n, s));
  }
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_rays_query_device(ohmhip_map_t m, const double *d_rays, size_t element_count, double volume_coefficient,
                                 double *d_ranges, double *d_unobserved_volumes, int8_t *d_terminal_types,
                                 void *d_terminal_keys)
try
{
  OHMHIP_CHECK(raysQueryRefusal(m, d_rays, element_count, d_ranges, d_unobserved_volumes, d_terminal_types));
  OHMHIP_SETTLE(m);
  return raysQueryDevice(m, d_rays, uint32_t(element_count / 2), volume_coefficient, d_ranges, d_unobserved_volumes,
                         d_terminal_types, static_cast<GpuKeyOut *>(d_terminal_keys));
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_QUERY_IMPL_H
