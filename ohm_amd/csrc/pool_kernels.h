// pool_kernels.h -- the region pool's utility kernels: lists of byte copies between pool slots and pinned host records
// (spill, re-admission, compaction), fills and masks over whole layers, and the use stamps of the spill policy.
#ifndef OHMHIP_POOL_KERNELS_H
#define OHMHIP_POOL_KERNELS_H

#include "batch_scratch.h"

namespace ohmhip
{
/// dst[i] &= mask
__global__ void k_and_u32(uint32_t *dst, uint32_t mask, size_t count)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
  {
    dst[i] &= mask;
  }
}

/// dst[index[i]] |= bits  (indices may repeat)
__global__ void k_or_at_u32(uint32_t *dst, const uint32_t *__restrict__ index, size_t count, uint32_t bits)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
  {
    atomicOr(&dst[index[i]], bits);
  }
}

/// A list of independent byte copies done by ONE launch: pool slot <-> pinned host record (the device reads / writes
/// the mapped host memory itself, so an eviction or re-admission of hundreds of regions is a single PCIe-saturating
/// kernel instead of one copy-engine call per region and layer: measured 10 GB/s with the calls, their per-call
/// overhead dominating 256 KiB copies), or slot -> slot inside the pool (compaction).
struct CopyJob
{
  const char *src;
  char *dst;
  uint64_t bytes;
};

constexpr uint32_t kCopyBlocksPerJob = 16;

__global__ void __launch_bounds__(256) k_copy_jobs(const CopyJob *__restrict__ jobs, uint32_t n_jobs)
{
  const uint32_t job_index = blockIdx.x / kCopyBlocksPerJob;
  const uint32_t part = blockIdx.x % kCopyBlocksPerJob;
  if (job_index >= n_jobs)
  {
    return;
  }
  const CopyJob job = jobs[job_index];
  const bool aligned = ((reinterpret_cast<uintptr_t>(job.src) | reinterpret_cast<uintptr_t>(job.dst)) & 15u) == 0;
  const uint64_t vectors = aligned ? job.bytes / 16u : 0u;
  const uint4 *src = reinterpret_cast<const uint4 *>(job.src);
  uint4 *dst = reinterpret_cast<uint4 *>(job.dst);
  // (interleaved over the job's blocks so that the blocks of a job stream neighbouring lines)
  for (uint64_t i = uint64_t(part) * 256u + threadIdx.x; i < vectors; i += uint64_t(kCopyBlocksPerJob) * 256u)
  {
    dst[i] = src[i];
  }
  if (part == 0)
  {
    for (uint64_t i = vectors * 16u + threadIdx.x; i < job.bytes; i += 256u)
    {
      job.dst[i] = job.src[i];
    }
  }
}

/// The same list of copies done by a SMALL persistent grid (the background write-back of the spill path): `gridDim.x`
/// workgroups walk the (job, part) pairs with a stride, so the launch holds at most that many CUs while batches run --
/// the walk kernel needs whole CUs, and a flood of short copy workgroups over all of them stalls it.
__global__ void __launch_bounds__(256) k_copy_jobs_few(const CopyJob *__restrict__ jobs, uint32_t n_jobs)
{
  const uint32_t units = n_jobs * kCopyBlocksPerJob;
  for (uint32_t unit = blockIdx.x; unit < units; unit += gridDim.x)
  {
    const CopyJob job = jobs[unit / kCopyBlocksPerJob];
    const uint32_t part = unit % kCopyBlocksPerJob;
    const bool aligned = ((reinterpret_cast<uintptr_t>(job.src) | reinterpret_cast<uintptr_t>(job.dst)) & 15u) == 0;
    const uint64_t vectors = aligned ? job.bytes / 16u : 0u;
    const uint4 *src = reinterpret_cast<const uint4 *>(job.src);
    uint4 *dst = reinterpret_cast<uint4 *>(job.dst);
    for (uint64_t i = uint64_t(part) * 256u + threadIdx.x; i < vectors; i += uint64_t(kCopyBlocksPerJob) * 256u)
    {
      dst[i] = src[i];
    }
    if (part == 0)
    {
      for (uint64_t i = vectors * 16u + threadIdx.x; i < job.bytes; i += 256u)
      {
        job.dst[i] = job.src[i];
      }
    }
  }
}

/// use[2 * index[i]] is touched with `stamp` (touchRegionUse)
__global__ void k_touch_use_at(uint32_t *use, const uint32_t *__restrict__ index, size_t count, uint32_t stamp)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
  {
    touchRegionUse(use, index[i], stamp);
  }
}

/// pairs = (slot, stamp): the slot's "use before the gap" becomes stamp (a region back from the host store)
__global__ void k_set_prev_use(uint32_t *use, const uint32_t *__restrict__ pairs, size_t count)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
  {
    use[2 * size_t(pairs[2 * i]) + 1] = pairs[2 * i + 1];
  }
}

/// Fill a float layer with a value (pool initialisation: occupancy clears to +inf, ohm/DefaultLayer.cpp:87-91).
__global__ void k_fill_u32(uint32_t *dst, uint32_t value, size_t count)
{
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride)
  {
    dst[i] = value;
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_POOL_KERNELS_H
