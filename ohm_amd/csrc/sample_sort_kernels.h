// sample_sort_kernels.h -- ordering a batch's sample keys per region, between binning and the walk (gfx950).
//
//   k_sort_region_hits  1 workgroup/region order a region's sample keys by (voxel, ray) in LDS
//                                          (fallback for very dense regions: device-wide radix sort + k_hit_bounds)
//   k_reset_cursors     1 lane / region    undo a binning pass's cursor movement so that it can be repeated
//   k_stream_marker     empty              a stop event between two kernels of a stream (BatchRun::frontHalf)
#ifndef OHMHIP_SAMPLE_SORT_KERNELS_H
#define OHMHIP_SAMPLE_SORT_KERNELS_H

#include "batch_scratch.h"
#include "region_table.h"

namespace ohmhip
{
// ---------------------------------------------------------------------------------------------------------------------
// k_hit_bounds: [begin, end) of each region slot in the sorted hit list, and the sample mask bit of every voxel in it.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
  k_hit_bounds(const unsigned long long *__restrict__ sorted, BatchScratch bs, int region_voxels,
               uint32_t *__restrict__ hit_mask)
{
  const uint32_t n_hits = bs.info->n_hits;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_hits)
  {
    return;
  }
  const unsigned long long group = hitGroup(sorted[i]);
  if (i == 0 || hitGroup(sorted[i - 1]) != group)
  {
    // First sample of its voxel: entry point for ordering misses against this voxel's samples.  Entries are only
    // ever read for voxels whose mask bit is set in the same batch, so the table needs no clearing.
    const uint32_t slot = hitSlot(sorted[i]);
    const uint32_t vi = hitVoxel(sorted[i]);
    bs.voxel_first_hit[size_t(slot) * size_t(region_voxels) + vi] = i;
    atomicOr(&hit_mask[size_t(slot) * (uint32_t(region_voxels + 31) >> 5) + (vi >> 5)], 1u << (vi & 31));
  }
  const uint32_t slot = hitSlot(sorted[i]);
  if (i == 0 || hitSlot(sorted[i - 1]) != slot)
  {
    bs.hit_begin[slot] = i;
  }
  if (i + 1 == n_hits || hitSlot(sorted[i + 1]) != slot)
  {
    bs.hit_end[slot] = i + 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_sort_region_hits: one workgroup per touched region orders the region's samples by (voxel, ray) in LDS (bitonic
// network over the next power of two) and records each voxel's first sample.  Replaces a device-wide radix sort of all
// sample keys plus k_hit_bounds when no region holds more than kSortRegionHits samples.
// ---------------------------------------------------------------------------------------------------------------------
/// LDS position of sort element i: one pad element per 32 keeps the power-of-two strides of the network (8 consecutive
/// keys per lane in the last trip of every merge level) off a single group of banks.
__device__ inline uint32_t sortSlot(uint32_t i)
{
  return i + (i >> 5);
}

/// R fused bitonic stages on the 2^R elements they connect (register butterflies between one LDS read and write).
template <int R>
__device__ inline void bitonicFused(unsigned long long *l_keys, uint32_t g, uint32_t s_shift, uint32_t k)
{
  constexpr uint32_t kCount = 1u << R;
  const uint32_t low = g & ((1u << s_shift) - 1u);
  const uint32_t base = ((g >> s_shift) << (s_shift + R)) | low;
  const bool ascending = (base & k) == 0;
  unsigned long long v[kCount];
#pragma unroll
  for (uint32_t m = 0; m < kCount; ++m)
  {
    v[m] = l_keys[sortSlot(base | (m << s_shift))];
  }
#pragma unroll
  for (int t = 0; t < R; ++t)
  {
    const uint32_t d = 1u << (R - 1 - t);
#pragma unroll
    for (uint32_t m = 0; m < kCount; ++m)
    {
      if ((m & d) == 0)
      {
        const unsigned long long a = v[m];
        const unsigned long long c = v[m | d];
        const bool swap = (a > c) == ascending;
        v[m] = swap ? c : a;
        v[m | d] = swap ? a : c;
      }
    }
  }
#pragma unroll
  for (uint32_t m = 0; m < kCount; ++m)
  {
    l_keys[sortSlot(base | (m << s_shift))] = v[m];
  }
}

constexpr uint32_t kSortRegionHits = 8192;
constexpr int kSortThreads = 1024;
#ifndef OHMHIP_SORT_SMALL
#define OHMHIP_SORT_SMALL 2048  // regions with at most this many samples are ordered by 256-thread workgroups (0: off)
#endif
constexpr uint32_t kSortSmallHits = OHMHIP_SORT_SMALL;
constexpr int kSortSmallThreads = 256;

/// kCap / kThreads: the instantiation's LDS capacity in keys and workgroup size; it orders the regions of the list with
/// min_hits < samples <= kCap.  The network of a region with ~10^3 samples keeps 128 lanes busy per fused stage: the
/// 1024-thread, 66 KiB instantiation (two workgroups per CU) spends its time in barriers of mostly idle waves, so regions
/// of at most kSortSmallHits samples -- nearly all of them -- go to a 256-thread, 17 KiB one that runs eight per CU.
template <uint32_t kCap, int kThreads>
__global__ void __launch_bounds__(kThreads)
  k_sort_region_hits(RegionTable rt, BatchScratch bs, const unsigned long long *__restrict__ keys,
                     unsigned long long *__restrict__ sorted, int region_voxels, uint32_t min_hits,
                     uint32_t *__restrict__ hit_mask)
{
  __shared__ unsigned long long l_keys[kCap + kCap / 32];
  const uint32_t mask_words = uint32_t(region_voxels + 31) >> 5;
  // Grid-stride over the list (its length lives on the device: the launch may be issued before the host knows it).
  const uint32_t n_regions = bs.info->n_hit_regions;
  for (uint32_t list_index = blockIdx.x; list_index < n_regions; list_index += gridDim.x)
  {
  const uint32_t h = bs.sort_list[list_index];
  const uint32_t slot = rt.vals[h];
  if (slot >= rt.slot_capacity)
  {
    continue;
  }
  const uint32_t begin = bs.hit_begin[slot];
  const uint32_t n = bs.hit_end[slot] - begin;
  if (n <= min_hits || n > kCap)
  {
    continue;
  }
  uint32_t padded = 64;
  while (padded < n)
  {
    padded <<= 1;
  }
  for (uint32_t i = threadIdx.x; i < padded; i += kThreads)
  {
    l_keys[sortSlot(i)] = (i < n) ? keys[begin + i] : ~0ull;
  }
  __syncthreads();
  // Bitonic network, up to three consecutive compare distances (j, j/2, j/4) fused per LDS round trip: a thread pulls
  // the 8 (4, 2) elements those stages connect into registers, runs the butterflies there and writes them back.
  // The network is LDS-bandwidth bound, so this cuts its cost by the same factor as the traffic (~2.6x).
  for (uint32_t k = 2; k <= padded; k <<= 1)
  {
    uint32_t j = k >> 1;
    while (j > 0)
    {
      // levels fused this trip: r in 1..3, distances j, j/2, .., s = j >> (r - 1)
      const uint32_t levels_left = uint32_t(32 - __clz(int(j)));  // log2(j) + 1
      const uint32_t r = min(3u, levels_left);
      const uint32_t s_shift = levels_left - r;  // log2 of the smallest distance s
      const uint32_t group_count = padded >> r;
      for (uint32_t g = threadIdx.x; g < group_count; g += kThreads)
      {
        if (r == 3)
        {
          bitonicFused<3>(l_keys, g, s_shift, k);
        }
        else if (r == 2)
        {
          bitonicFused<2>(l_keys, g, s_shift, k);
        }
        else
        {
          bitonicFused<1>(l_keys, g, s_shift, k);
        }
      }
      __syncthreads();
      j >>= r;
    }
  }
  for (uint32_t base = 0; base < n; base += kThreads)  // (every lane takes every trip: the shuffles below)
  {
    const uint32_t i = base + threadIdx.x;
    uint32_t word = 0xffffffffu, bits = 0;
    if (i < n)
    {
      const unsigned long long key = l_keys[sortSlot(i)];
      sorted[begin + i] = key;
      const uint32_t vi = hitVoxel(key);
      word = vi >> 5;
      if (i == 0 || hitGroup(l_keys[sortSlot(i - 1)]) != hitGroup(key))
      {
        // First sample of its voxel: entry point for ordering misses against this voxel's samples, and the voxel's bit
        // of the sample mask.
        bs.voxel_first_hit[size_t(slot) * size_t(region_voxels) + vi] = begin + i;
        bits = 1u << (vi & 31);
      }
    }
    // The keys are in voxel order, so the lanes of a wave whose voxels share a mask word are neighbours: their bits are
    // ORed along each such run and the run's last lane sets them with one atomic (one per voxel, from neighbouring lanes
    // to the same address, cost the two sort launches 32 us per C1 batch).
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1)
    {
      const uint32_t up_bits = __shfl_up(bits, d, 64);
      const uint32_t up_word = __shfl_up(word, d, 64);
      bits |= (lane >= d && up_word == word) ? up_bits : 0u;
    }
    const uint32_t next_word = __shfl_down(word, 1u, 64);
    if (bits && (lane == 63u || next_word != word))
    {
      atomicOr(&hit_mask[size_t(slot) * mask_words + word], bits);
    }
  }
  __syncthreads();  // l_keys is reused by the next region
  }  // regions
}

/// Nothing: a place in a stream whose stop event another stream can wait for.
__global__ void k_stream_marker() {}

/// Undo the cursor movement of a k_ray_bin pass over the touched regions (segment cursors back to zero, sample cursors
/// back to the start of the region's range) so the pass can be repeated with other launch parameters.
__global__ void __launch_bounds__(256) k_reset_cursors(RegionTable rt, BatchScratch bs)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bs.info->n_touched)
  {
    return;
  }
  const uint32_t h = bs.touched[i];
  bs.seg_cursor[h] = 0;
  const uint32_t slot = rt.vals[h];
  if (slot < rt.slot_capacity)
  {
    bs.hit_end[slot] = bs.hit_begin[slot];
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_SAMPLE_SORT_KERNELS_H
