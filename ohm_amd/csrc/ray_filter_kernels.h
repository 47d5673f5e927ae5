// ray_filter_kernels.h -- the map's ray-filter chain as a pass of its own (gfx950): one lane per ray, ahead of
// k_ray_setup on the batch's front stream, and only when a chain is set (ohmhip_map_set_ray_filter_stages).
//
// The pass writes every ray as the chain leaves it and the ray's RayFilterFlag byte; k_ray_setup then reads the moved
// rays and takes the flags through MapConst::batch_filter_flags exactly as for a caller-filtered batch (kRffInvalid: not
// passed, kRffClippedEnd: the end voxel is part of the ray, no sample).  Nothing is compacted, so the ray indices of
// intensities and timestamps stay what they were.  The stage arithmetic is ray_filter_chain.h's, shared with the host.
#ifndef OHMHIP_RAY_FILTER_KERNELS_H
#define OHMHIP_RAY_FILTER_KERNELS_H

#include "ray_filter_chain.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ohmhip
{
/// `stages`: n_stages records in a device buffer the map owns (uniform reads).  `rays_out` / `flags_out` / `passed` may
/// each be null; `rays_out` may alias `rays` (a lane reads its ray before it writes it).  `passed` (a device word,
/// zeroed by the caller) receives the number of rays kept, one atomic per wave.
__global__ void __launch_bounds__(256)
  k_ray_filter(const ohmhip_ray_filter_stage *__restrict__ stages, uint32_t n_stages, const double *rays,
               uint32_t n_rays, double *rays_out, unsigned char *flags_out, uint32_t *passed)
{
  const uint32_t ray = blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (ray < n_rays)
  {
    double start[3], end[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      start[a] = rays[size_t(ray) * 6 + a];
      end[a] = rays[size_t(ray) * 6 + 3 + a];
    }
    unsigned flags = 0;
    keep = rayFilterChain(stages, n_stages, start, end, &flags);
    if (rays_out)
    {
#pragma unroll
      for (int a = 0; a < 3; ++a)
      {
        rays_out[size_t(ray) * 6 + a] = start[a];
        rays_out[size_t(ray) * 6 + 3 + a] = end[a];
      }
    }
    if (flags_out)
    {
      flags_out[ray] = static_cast<unsigned char>(flags);
    }
  }
  if (passed)
  {
    const unsigned long long kept = __ballot(keep);
    if ((threadIdx.x & 63u) == 0 && kept)
    {
      atomicAdd(passed, uint32_t(__popcll(kept)));
    }
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_RAY_FILTER_KERNELS_H
