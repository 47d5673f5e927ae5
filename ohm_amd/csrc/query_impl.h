// query_impl.h -- host side of the read-only queries (query_kernels.h): the line-keys query, the map as the read-side
// kernels see it (mapReadView, which the clearance, heightmap and cloud host code share) and the rays query with its
// two entry points.  Included at the end of ohmhip_map.hip's translation unit, ahead of the other read-side parts.
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
/// The map as the read-only kernels see it (MapReadView): configuration, region hash, occupancy layer and the table of
/// the host store's regions (QuerySpillTable; empty without spill to host).  `layer`: the layer whose blocks the view
/// addresses (the voxel reads by key look at any layer through the same view).
int mapReadView(ohmhip_map_t m, MapReadView &view, int layer = OHMHIP_LID_OCCUPANCY)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  view.mc = m->mc;
  view.rt = regionTable(m);
  view.occupancy = static_cast<const float *>(m->pool.layers[layer].get());
  view.spill = QuerySpillTable{ nullptr, nullptr, 0 };
  if (!m->spilled.empty())
  {
    // Regions in the host store answer from their pinned records (device visible), without re-admission.  The table is
    // rebuilt per call: the store changes with every batch that evicts or re-admits.  (Evictions copy on the copy
    // stream; the previous query may still read the table being replaced.)
    OHMHIP_CHECK(hipStreamSynchronize(m->copy_stream));
    OHMHIP_CHECK(hipStreamSynchronize(s));
    uint32_t cap = 16;
    while (cap < 2 * m->spilled.size())
    {
      cap <<= 1;
    }
    std::vector<unsigned long long> keys(cap, 0ull);
    std::vector<const float *> blocks(cap, nullptr);
    for (const auto &entry : m->spilled)
    {
      uint32_t idx = hashRegionKey(entry.first, cap - 1);
      while (keys[idx] != 0)
      {
        idx = (idx + 1) & (cap - 1);
      }
      keys[idx] = entry.first;
      blocks[idx] = reinterpret_cast<const float *>(entry.second.record + m->store.layer_offset[layer]);
    }
    OHMHIP_CHECK(qs.spill_keys.ensure(sizeof(unsigned long long) * cap, false, s));
    OHMHIP_CHECK(qs.spill_blocks.ensure(sizeof(const float *) * cap, false, s));
    OHMHIP_CHECK(hipMemcpy(qs.spill_keys.ptr, keys.data(), sizeof(unsigned long long) * cap, hipMemcpyHostToDevice));
    OHMHIP_CHECK(hipMemcpy(qs.spill_blocks.ptr, blocks.data(), sizeof(const float *) * cap, hipMemcpyHostToDevice));
    view.spill = QuerySpillTable{ static_cast<const unsigned long long *>(qs.spill_keys.ptr),
                                  static_cast<const float *const *>(qs.spill_blocks.ptr), cap - 1 };
  }
  return OHMHIP_OK;
}

/// What both query entry points check before any device work (OHMHIP_ERR_INVALID_ARG / OHMHIP_ERR_UNSUPPORTED).
int raysQueryRefusal(ohmhip_map_t m, const void *rays, size_t element_count, const void *ranges,
                     const void *unobserved_volumes, const void *terminal_types)
{
  const size_t n = element_count / 2;
  if (!m || (n && (!rays || !ranges || !unobserved_volumes || !terminal_types)) || n > size_t(0x7fffffff))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (!m->pool.layers[OHMHIP_LID_OCCUPANCY])
  {
    return OHMHIP_ERR_UNSUPPORTED;  // the CPU query refuses maps without the layer too (valid_layers)
  }
  if (m->mc.owner_world > 1u)
  {
    return OHMHIP_ERR_UNSUPPORTED;  // a rank holds only its territory
  }
  return OHMHIP_OK;
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
  if (n)
  {
    OHMHIP_CHECK(qs.rays.ensure(sizeof(double) * 6 * n, false, s));
    OHMHIP_CHECK(qs.ranges.ensure(sizeof(double) * n, false, s));
    OHMHIP_CHECK(qs.volumes.ensure(sizeof(double) * n, false, s));
    OHMHIP_CHECK(qs.types.ensure(n, false, s));
    if (terminal_keys)
    {
      OHMHIP_CHECK(qs.keys.ensure(sizeof(GpuKeyOut) * n, false, s));
    }
    OHMHIP_CHECK(hipMemcpyAsync(qs.rays.ptr, rays, sizeof(double) * 6 * n, hipMemcpyHostToDevice, s));
  }
  double *d_ranges = static_cast<double *>(qs.ranges.ptr);
  double *d_volumes = static_cast<double *>(qs.volumes.ptr);
  int8_t *d_types = static_cast<int8_t *>(qs.types.ptr);
  GpuKeyOut *d_keys = terminal_keys ? static_cast<GpuKeyOut *>(qs.keys.ptr) : nullptr;
  OHMHIP_CHECK(raysQueryDevice(m, static_cast<const double *>(qs.rays.ptr), n, volume_coefficient, d_ranges, d_volumes,
                               d_types, d_keys));
  if (n)
  {
    OHMHIP_CHECK(hipMemcpyAsync(ranges, d_ranges, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    OHMHIP_CHECK(hipMemcpyAsync(unobserved_volumes, d_volumes, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    OHMHIP_CHECK(hipMemcpyAsync(terminal_types, d_types, n, hipMemcpyDeviceToHost, s));
    if (terminal_keys)
    {
      OHMHIP_CHECK(hipMemcpyAsync(terminal_keys, d_keys, sizeof(GpuKeyOut) * n, hipMemcpyDeviceToHost, s));
    }
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
