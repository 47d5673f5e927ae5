// ray_filter_impl.h -- the map's ray-filter chain: setting and reading it, and ohmhip_map_apply_ray_filter, the pass on
// its own (GpuMap::setRayFilter / effectiveRayFilter for the stock filters, ohmgpu/GpuMap.cpp:348-369, 736-746).  Where
// the chain meets a batch: BatchRun::prepare / frontHalf (batch_run.h), hostFilterCount and k_count_passed (ray_entry.h).
//
// Part of ohmhip_map.hip's translation unit (included there, in order): not a stand-alone header.
#ifndef OHMHIP_RAY_FILTER_IMPL_H
#define OHMHIP_RAY_FILTER_IMPL_H

namespace
{
int applyRayFilterDevice(ohmhip_map_t m, const double *d_rays, size_t n_rays, double *d_rays_out,
                         unsigned char *d_flags_out, size_t *passed)
{
  ohmhip_map_s::RayFilterChain &rc = m->ray_chain;
  OHMHIP_CHECK(rc.q_passed.ensure(sizeof(uint32_t), false, m->stream));
  OHMHIP_CHECK(hipMemsetAsync(rc.q_passed.ptr, 0, sizeof(uint32_t), m->stream));
  hipLaunchKernelGGL(k_ray_filter, dim3(uint32_t((n_rays + 255) / 256)), dim3(256), 0, m->stream,
                     static_cast<const ohmhip_ray_filter_stage *>(rc.d_stages.ptr), rc.count, d_rays, uint32_t(n_rays),
                     d_rays_out, d_flags_out, static_cast<uint32_t *>(rc.q_passed.ptr));
  OHMHIP_CHECK(hipGetLastError());
  uint32_t kept = 0;
  OHMHIP_CHECK(hipMemcpyAsync(&kept, rc.q_passed.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
  OHMHIP_CHECK(hipStreamSynchronize(m->stream));
  if (passed)
  {
    *passed = kept;
  }
  return OHMHIP_OK;
}
}  // namespace

extern "C" {

int ohmhip_map_set_ray_filter_stages(ohmhip_map_t m, const ohmhip_ray_filter_stage *stages, unsigned count)
try
{
  if (!m || count > OHMHIP_MAX_RAY_FILTER_STAGES || (count && !stages))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  for (unsigned i = 0; i < count; ++i)
  {
    if (stages[i].kind < OHMHIP_RFS_GOOD || stages[i].kind > OHMHIP_RFS_CLIP_TO_BOUNDS || stages[i].reserved != 0)
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
  }
  if (count && m->mc.owner_world > 1u)
  {
    return OHMHIP_ERR_UNSUPPORTED;  // routed rays would be filtered twice (include/ohmhip.h)
  }
  // The rays waiting in the coalescing buffer were counted by the chain as it is: they run under it.
  OHMHIP_SETTLE(m);
  // Nothing of the map's may still read the device copy: the set-up passes on the front stream, the per-call counts on
  // the copy stream, a query on the compute stream.
  OHMHIP_CHECK(hipStreamSynchronize(m->front_stream));
  OHMHIP_CHECK(hipStreamSynchronize(m->copy_stream));
  OHMHIP_CHECK(hipStreamSynchronize(m->stream));
  ohmhip_map_s::RayFilterChain &rc = m->ray_chain;
  if (count)
  {
    OHMHIP_CHECK(rc.d_stages.ensure(sizeof(ohmhip_ray_filter_stage) * OHMHIP_MAX_RAY_FILTER_STAGES, false, m->stream));
    OHMHIP_CHECK(hipMemcpy(rc.d_stages.ptr, stages, sizeof(ohmhip_ray_filter_stage) * count, hipMemcpyHostToDevice));
    std::memcpy(rc.stages, stages, sizeof(ohmhip_ray_filter_stage) * count);
    // The pass's output, both parities, for the largest batch the map's per-ray buffers hold already (a batch seen or
    // ohmhip_map_reserve_rays): otherwise the first filtered batch pays four hipMallocs in its middle.  Larger batches
    // grow it on demand (BatchRun::prepare).
    const size_t sized_for = m->walks_buf[0].bytes / sizeof(RayWalk);
    for (int p = 0; p < 2 && sized_for; ++p)
    {
      OHMHIP_CHECK(rc.rays[p].ensure(sized_for * 48, false, m->stream));
      OHMHIP_CHECK(rc.flags[p].ensure(sized_for, false, m->stream));
    }
  }
  rc.count = count;
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

int ohmhip_map_ray_filter_stages(ohmhip_map_t m, ohmhip_ray_filter_stage *out, unsigned capacity, unsigned *count)
try
{
  if (!m || !count)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  *count = m->ray_chain.count;
  for (unsigned i = 0; out && i < m->ray_chain.count && i < capacity; ++i)
  {
    out[i] = m->ray_chain.stages[i];
  }
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

int ohmhip_map_apply_ray_filter_device(ohmhip_map_t m, const double *d_rays, size_t element_count, double *d_rays_out,
                                       unsigned char *d_flags_out, size_t *passed)
try
{
  if (passed)
  {
    *passed = 0;
  }
  const size_t n_rays = element_count / 2;
  if (!m || (!d_rays && n_rays) || n_rays > 0xffffffffull)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (n_rays == 0)
  {
    return OHMHIP_OK;
  }
  return applyRayFilterDevice(m, d_rays, n_rays, d_rays_out, d_flags_out, passed);
}
OHMHIP_ABI_CATCH

int ohmhip_map_apply_ray_filter(ohmhip_map_t m, const double *rays, size_t element_count, double *rays_out,
                                unsigned char *flags_out, size_t *passed)
try
{
  if (passed)
  {
    *passed = 0;
  }
  const size_t n_rays = element_count / 2;
  if (!m || (!rays && n_rays) || n_rays > 0xffffffffull)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (n_rays == 0)
  {
    return OHMHIP_OK;
  }
  ohmhip_map_s::RayFilterChain &rc = m->ray_chain;
  OHMHIP_CHECK(rc.q_rays.ensure(n_rays * 48, false, m->stream));
  OHMHIP_CHECK(rc.q_out.ensure(n_rays * 48, false, m->stream));
  OHMHIP_CHECK(rc.q_flags.ensure(n_rays, false, m->stream));
  OHMHIP_CHECK(hipMemcpyAsync(rc.q_rays.ptr, rays, n_rays * 48, hipMemcpyHostToDevice, m->stream));
  OHMHIP_CHECK(applyRayFilterDevice(m, static_cast<const double *>(rc.q_rays.ptr), n_rays,
                                    static_cast<double *>(rc.q_out.ptr), static_cast<unsigned char *>(rc.q_flags.ptr),
                                    passed));
  if (rays_out)
  {
    OHMHIP_CHECK(hipMemcpy(rays_out, rc.q_out.ptr, n_rays * 48, hipMemcpyDeviceToHost));
  }
  if (flags_out)
  {
    OHMHIP_CHECK(hipMemcpy(flags_out, rc.q_flags.ptr, n_rays, hipMemcpyDeviceToHost));
  }
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_RAY_FILTER_IMPL_H
