// clearance_impl.h -- host side of the clearance queries (clearance_kernels.h): argument checks and search parameters
// (clearanceSetup), the per-region search on the map's stream (clearanceRegionsDevice) and the three entry points.
// Included at the end of ohmhip_map.hip's translation unit, after read_side.h (mapReadView, the refusal).
#ifndef OHMHIP_CLEARANCE_IMPL_H
#define OHMHIP_CLEARANCE_IMPL_H

namespace
{
/// ClearanceArgs of a clearance query: the checks every entry point makes before any device work, then the search
/// parameters.  OHMHIP_ERR_INVALID_ARG / OHMHIP_ERR_UNSUPPORTED as include/ohmhip.h lists them.
int clearanceSetup(ohmhip_map_t m, const void *keys, size_t count, const ohmhip_clearance_params *p, const void *out,
                   ClearanceArgs &a)
{
  if (!m || !p || (count && (!keys || !out)) || count > size_t(0x7fffffff))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (!(p->search_radius >= 0.0f) || !std::isfinite(p->search_radius))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  for (int c = 0; c < 3; ++c)
  {
    if (!std::isfinite(p->axis_scaling[c]) || p->axis_scaling[c] == 0.0f)
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
  }
  OHMHIP_CHECK(readSideRefusal(m, OHMHIP_LID_OCCUPANCY));
  // calculateVoxelSearchHalfExtents (ohm/private/VoxelAlgorithms.cpp:16): float radius / double resolution
  const double h = std::ceil(double(p->search_radius) / m->mc.resolution);
  if (!(h <= double(kClearanceMaxH)))
  {
    return OHMHIP_ERR_UNSUPPORTED;
  }
  a = ClearanceArgs{};
  a.mc = m->mc;
  a.h = int(h);
  a.radius = p->search_radius;
  for (int c = 0; c < 3; ++c)
  {
    a.scale[c] = p->axis_scaling[c];
  }
  a.unknown_as_occupied = (p->flags & OHMHIP_QF_UNKNOWN_AS_OCCUPIED) ? 1 : 0;
  a.report_unscaled = (p->flags & OHMHIP_QF_REPORT_UNSCALED) ? 1 : 0;
  return OHMHIP_OK;
}

/// Region mode on the map's stream: `count` caller region keys (host), every voxel of each into d_out
/// ([count][region voxels]).  The map is settled by the caller; the map is read, never written.
int clearanceRegionsDevice(ohmhip_map_t m, ClearanceArgs &a, const int16_t *keys_xyz, uint32_t count, float *d_out)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_CHECK(mapReadView(m, a));
  OHMHIP_CHECK(qs.clear_regions.ensure(sizeof(int16_t) * 3 * count, false, s));
  OHMHIP_CHECK(hipMemcpyAsync(qs.clear_regions.ptr, keys_xyz, sizeof(int16_t) * 3 * count, hipMemcpyHostToDevice, s));
  const int16_t *d_regions = static_cast<const int16_t *>(qs.clear_regions.ptr);
  const MapConst &mc = m->mc;
  const size_t kvox = size_t(mc.kdim[0]) * size_t(mc.kdim[1]) * size_t(mc.kdim[2]);
  // The LDS path while the window's bitmask and its table of tiles fit: a window of W coordinates touches at most
  // ceil((W - 1) / dim) + 1 tiles per axis.
  const int w = kClearanceTile + 2 * a.h;
  size_t tiles = 1;
  for (int c = 0; c < 3; ++c)
  {
    tiles *= size_t((w - 1 + mc.dim[c] - 1) / mc.dim[c] + 1);
  }
  if (a.h <= kClearanceLdsMaxH && tiles <= size_t(kClearanceMaxTileBlocks))
  {
    const size_t lds = clearanceLdsBytes(a.h);
    OHMHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_clearance_regions_lds),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, int(lds)));
    const size_t per_region =
      size_t(clearanceSubTiles(mc.kdim[0])) * clearanceSubTiles(mc.kdim[1]) * clearanceSubTiles(mc.kdim[2]);
    // (grid.x < 2^31: batches of regions)
    const uint32_t batch = uint32_t(std::max<size_t>(1, std::min<size_t>(count, size_t(0x7fffffff) / per_region)));
    for (uint32_t r0 = 0; r0 < count; r0 += batch)
    {
      const uint32_t nb = std::min(batch, count - r0);
      a.regions = d_regions + size_t(r0) * 3;
      a.n = nb;
      a.out = d_out + size_t(r0) * kvox;
      hipLaunchKernelGGL(k_clearance_regions_lds, dim3(uint32_t(nb * per_region)), dim3(kClearanceThreads), lds, s, a);
      OHMHIP_CHECK(hipGetLastError());
    }
    return OHMHIP_OK;
  }
  // Large windows: the bitmask of each region's padded box in global memory, in batches of at most 256 MiB.
  for (int c = 0; c < 3; ++c)
  {
    a.pad[c] = mc.kdim[c] + 2 * a.h;
  }
  a.words = (a.pad[0] + 63) / 64;
  const size_t mask_words = size_t(a.pad[2]) * size_t(a.pad[1]) * size_t(a.words);
  const uint32_t batch = uint32_t(std::max<size_t>(1, std::min<size_t>(count, (size_t(256) << 20) / (8 * mask_words))));
  OHMHIP_CHECK(qs.clear_mask.ensure(8 * mask_words * batch, false, s));
  a.mask = static_cast<unsigned long long *>(qs.clear_mask.ptr);
  for (uint32_t r0 = 0; r0 < count; r0 += batch)
  {
    const uint32_t nb = std::min(batch, count - r0);
    a.regions = d_regions + size_t(r0) * 3;
    a.n = nb;
    a.out = d_out + size_t(r0) * kvox;
    const size_t items = mask_words * nb;
    hipLaunchKernelGGL(k_clearance_mask, dim3(uint32_t(std::min<size_t>((items + 3) / 4, 65536))), dim3(256), 0, s, a);
    OHMHIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_clearance_regions_global, dim3(uint32_t((kvox * nb + 255) / 256)), dim3(256), 0, s, a);
    OHMHIP_CHECK(hipGetLastError());
  }
  return OHMHIP_OK;
}
}  // namespace

extern "C" {

int ohmhip_map_clearance_regions(ohmhip_map_t m, const int16_t *keys_xyz, size_t count,
                                 const ohmhip_clearance_params *params, float *const *dsts)
try
{
  ClearanceArgs a;
  OHMHIP_CHECK(clearanceSetup(m, keys_xyz, count, params, dsts, a));
  for (size_t i = 0; i < count; ++i)
  {
    if (!dsts[i])
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
  }
  OHMHIP_SETTLE(m);
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  const size_t kvox = size_t(m->mc.kdim[0]) * size_t(m->mc.kdim[1]) * size_t(m->mc.kdim[2]);
  OHMHIP_CHECK(m->query.clear_out.ensure(sizeof(float) * kvox * count, false, s));
  float *d_out = static_cast<float *>(m->query.clear_out.ptr);
  OHMHIP_CHECK(clearanceRegionsDevice(m, a, keys_xyz, uint32_t(count), d_out));
  for (size_t i = 0; i < count; ++i)
  {
    OHMHIP_CHECK(hipMemcpyAsync(dsts[i], d_out + i * kvox, sizeof(float) * kvox, hipMemcpyDeviceToHost, s));
  }
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_clearance_regions_device(ohmhip_map_t m, const int16_t *keys_xyz, size_t count,
                                        const ohmhip_clearance_params *params, float *d_out)
try
{
  ClearanceArgs a;
  OHMHIP_CHECK(clearanceSetup(m, keys_xyz, count, params, d_out, a));
  OHMHIP_SETTLE(m);
  return clearanceRegionsDevice(m, a, keys_xyz, uint32_t(count), d_out);
}
OHMHIP_ABI_CATCH

int ohmhip_map_clearance_keys(ohmhip_map_t m, const void *keys, size_t count, const ohmhip_clearance_params *params,
                              float *out)
try
{
  ClearanceArgs a;
  OHMHIP_CHECK(clearanceSetup(m, keys, count, params, out, a));
  const GpuKeyOut *k = static_cast<const GpuKeyOut *>(keys);
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
  OHMHIP_CHECK(mapReadView(m, a));
  OHMHIP_CHECK(qs.clear_keys.ensure(sizeof(GpuKeyOut) * count, false, s));
  OHMHIP_CHECK(qs.clear_out.ensure(sizeof(float) * count, false, s));
  OHMHIP_CHECK(hipMemcpyAsync(qs.clear_keys.ptr, keys, sizeof(GpuKeyOut) * count, hipMemcpyHostToDevice, s));
  a.keys = static_cast<const GpuKeyOut *>(qs.clear_keys.ptr);
  a.n = uint32_t(count);
  a.out = static_cast<float *>(qs.clear_out.ptr);
  hipLaunchKernelGGL(k_clearance_keys, dim3(uint32_t((count + 255) / 256)), dim3(256), 0, s, a);
  OHMHIP_CHECK(hipGetLastError());
  OHMHIP_CHECK(hipMemcpyAsync(out, a.out, sizeof(float) * count, hipMemcpyDeviceToHost, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_CLEARANCE_IMPL_H
