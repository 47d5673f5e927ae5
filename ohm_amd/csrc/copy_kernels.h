// copy_kernels.h -- k_copy_map: ohmhip_map_copy's one launch (include/ohmhip.h, MAP COPY).  Every
// (tile, layer) block of every region a copy moves is one job; where the layer is the one the destination's "ordered
// replay" mask is derived from (MapCopyJob::mask_kind), the wave that moves 64 lanes' worth of voxels also writes their
// mask words, by replayMaskBit (replay_kernels.h) from the values in its registers: the layer is not read a second time
// and no launch follows per region.
#ifndef OHMHIP_COPY_KERNELS_H
#define OHMHIP_COPY_KERNELS_H

#include "replay_kernels.h"

namespace ohmhip
{
/// One block of one layer.  `src` is a pool slot's block of the source map or a layer block inside a record of its
/// pinned host store (device visible); null: the source holds no such tile, the destination block takes the layer's
/// clear value.  Every layer's voxel is a multiple of 4 bytes and every block starts on a 4-byte boundary; the blocks
/// of the 8-byte layers the masks are derived from start on an 8-byte boundary.
struct MapCopyJob
{
  const char *src;
  char *dst;
  uint32_t *mask;  ///< the destination slot's mask row (mask_kind != kReplayMaskNone)
  uint32_t bytes;
  uint32_t clear_word;
  uint32_t mask_kind;  ///< ReplayMaskKind, under the DESTINATION's truncation distance
  uint32_t pad_;
};

/// The bits 0..15 of v at the even positions of a 32-bit word.
__device__ inline uint32_t spreadBits16(uint32_t v)
{
  v &= 0xffffu;
  v = (v | (v << 8)) & 0x00ff00ffu;
  v = (v | (v << 4)) & 0x0f0f0f0fu;
  v = (v | (v << 2)) & 0x33333333u;
  v = (v | (v << 1)) & 0x55555555u;
  return v;
}

/// grid: n_jobs * parts workgroups of 256; the `parts` workgroups of a job interleave over it wave by wave, so
/// neighbouring waves stream neighbouring lines.
__global__ void __launch_bounds__(256)
  k_copy_map(const MapCopyJob *__restrict__ jobs, uint32_t n_jobs, uint32_t parts, float tsdf_trunc)
{
  const uint32_t job_index = blockIdx.x / parts;
  if (job_index >= n_jobs)
  {
    return;
  }
  const MapCopyJob job = jobs[job_index];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (blockIdx.x % parts) * 4u + (threadIdx.x >> 6);
  const uint32_t waves = parts * 4u;
  const bool aligned = ((reinterpret_cast<uintptr_t>(job.src) | reinterpret_cast<uintptr_t>(job.dst)) & 15u) == 0;
  const uint32_t cw = job.clear_word;

  if (job.mask_kind == kReplayMaskNone)
  {
    // 16-byte vectors where both sides allow them, 4-byte words for the rest: the whole block when one side is not
    // 16-byte aligned (a 5 x 3 x 7 region's 4-byte layer is 420 bytes: every other slot), else the tail.
    const uint32_t vectors = aligned ? job.bytes / 16u : 0u;
    const uint4 *src4 = reinterpret_cast<const uint4 *>(job.src);
    uint4 *dst4 = reinterpret_cast<uint4 *>(job.dst);
    for (uint32_t i = wave * 64u + lane; i < vectors; i += waves * 64u)
    {
      dst4[i] = job.src ? src4[i] : make_uint4(cw, cw, cw, cw);
    }
    const uint32_t *src1 = reinterpret_cast<const uint32_t *>(job.src);
    uint32_t *dst1 = reinterpret_cast<uint32_t *>(job.dst);
    for (uint32_t i = vectors * 4u + wave * 64u + lane; i < job.bytes / 4u; i += waves * 64u)
    {
      dst1[i] = job.src ? src1[i] : cw;
    }
    return;
  }

  // A layer of 8-byte voxels that defines the mask.  Per step a wave moves 128 voxels (two per lane, one 16-byte vector)
  // or, when a side is only 8-byte aligned, 64 (one per lane): whole mask words either way, so no two waves share one.
  const uint32_t voxels = job.bytes / 8u;
  const uint32_t mask_words = (voxels + 31u) >> 5;
  const uint32_t per_lane = aligned ? 2u : 1u;
  const uint32_t step_voxels = 64u * per_lane;
  // (the bound is wave uniform: the ballots below see every lane)
  for (uint32_t base = wave * step_voxels; base < voxels; base += waves * step_voxels)
  {
    const uint32_t v0 = base + lane * per_lane;
    const uint32_t here = (v0 < voxels) ? min(per_lane, voxels - v0) : 0u;
    uint4 q = make_uint4(cw, cw, cw, cw);
    if (here == 2u)
    {
      if (job.src)
      {
        q = *reinterpret_cast<const uint4 *>(job.src + size_t(v0) * 8u);
      }
      *reinterpret_cast<uint4 *>(job.dst + size_t(v0) * 8u) = q;
    }
    else if (here == 1u)
    {
      if (job.src)
      {
        const uint2 h = *reinterpret_cast<const uint2 *>(job.src + size_t(v0) * 8u);
        q.x = h.x;
        q.y = h.y;
      }
      *reinterpret_cast<uint2 *>(job.dst + size_t(v0) * 8u) = make_uint2(q.x, q.y);
    }
    const bool f0 = here >= 1u && replayMaskBit(job.mask_kind, q.x, q.y, tsdf_trunc);
    const bool f1 = here == 2u && replayMaskBit(job.mask_kind, q.z, q.w, tsdf_trunc);
    const unsigned long long b0 = __ballot(f0);
    const unsigned long long b1 = __ballot(f1);
    // Mask word k of the step covers voxels base + 32 k ...: 32 lanes' first voxels, or 16 lanes' two voxels each.
    const uint32_t words_here = step_voxels / 32u;
    const uint32_t word = base / 32u + lane;
    if (lane < words_here && word < mask_words)
    {
      job.mask[word] = aligned ? (spreadBits16(uint32_t(b0 >> (16u * lane))) | (spreadBits16(uint32_t(b1 >> (16u * lane))) << 1))
                               : uint32_t(b0 >> (32u * lane));
    }
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_COPY_KERNELS_H
