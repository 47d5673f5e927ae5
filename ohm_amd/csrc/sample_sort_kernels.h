// sample_sort_kernels.h -- ordering a batch's sample keys per region, between binning and the walk (gfx950).
//
//   k_sort_region_hits  1 workgroup/region order a region's sample keys by (voxel, ray) in LDS: counting placement by
//                                          bucket (voxel >> 5) and a rank among the few keys that share a bucket; a
//                                          region whose buckets are crowded (walls, one voxel many rays end in) runs the
//                                          bitonic network instead
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
// k_sort_region_hits: one workgroup per touched region orders the region's samples by (voxel, ray) in LDS and records
// each voxel's first sample where the walk can ask for it.  Replaces a device-wide radix sort of all sample keys plus
// k_hit_bounds when no region holds more than kSortRegionHits samples.
//
// RANKED ORDERING.  A batch of a moving sensor puts about one sample into a sampled voxel and three into the 32 voxels
// that share a word of the sample mask, so a region's keys are placed by counting and only finished by comparing:
//   histogram   one LDS add per key on the count of its bucket b = voxel >> shift; the key is staged in the network's
//               layout meanwhile, so a region that falls back has read its keys once, as before
//   scan        exclusive scan of the counts (shuffles) -> every bucket's first position; the same pass adds up
//               W = sum of count^2, the exact number of compares the rank step would make
//   placement   a returning LDS add on the bucket's position gives every key its own place inside the bucket's range
//               (any order); afterwards the word holds the END of the bucket's range, the start of the next one
//   rank        one lane per staged key counts the keys of its bucket's range that come before it (ties -- no caller
//               produces them: one sample per ray -- broken by staged position, so the ranks of a range are always a
//               permutation of it) and notes range start + rank in the key's slot field: the keys of a region share
//               that field, only the 44 bits below it are staged and compared
//   move        barrier, every lane reads its (up to 8) staged keys, barrier, writes them to their positions with the
//               slot field restored, barrier
// The result does not depend on the order in which the adds arrive.  Neighbouring lanes rank neighbouring staged keys,
// i.e. keys of the same bucket: their loops have the same length and read the same LDS addresses (broadcast).
// That is about 10 + W/n LDS accesses per key and 8 barriers per region, against 52-70 accesses and 22-35 barriers of
// the network.  One region alone on the device (scripts/sample_order_probe.py, profiles/r09_notes.md): 512 / 2048 /
// 8192 uniform samples 6 / 15 / 26 us, the network 12 / 25 / 53 us.
//
// FALLBACK.  W > kOrderRankLimit * n (decided from LDS values, the same for every lane): the rank step would turn
// quadratic -- a wall (hundreds of samples per bucket), a voxel that all rays end in (W = n^2).  The region then runs the
// bitonic network over the next power of two as before.  The two cost the same at W/n = 60 (512 samples), 36 (2048) and
// 60 (8192); the limit is 32.  The histogram and the scan cost such a region 1.5-2 us on top of the network (its keys are
// staged for the network while they are counted: it reads them once).
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

/// The bitonic network over `padded` (a power of two >= 64) keys staged at sortSlot positions, padding keys ~0 included.
/// Up to three consecutive compare distances (j, j/2, j/4) fused per LDS round trip: a thread pulls the 8 (4, 2) elements
/// those stages connect into registers, runs the butterflies there and writes them back.  The network is LDS-bandwidth
/// bound, so this cuts its cost by the same factor as the traffic (~2.6x).  Ends behind a barrier.
template <int kThreads>
__device__ inline void bitonicNetwork(unsigned long long *l_keys, uint32_t padded, uint32_t tid)
{
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
      for (uint32_t g = tid; g < group_count; g += kThreads)
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
}

constexpr uint32_t kSortRegionHits = 8192;
constexpr int kSortThreads = 1024;
#ifndef OHMHIP_SORT_SMALL
#define OHMHIP_SORT_SMALL 2048  // regions with at most this many samples are ordered by 256-thread workgroups (0: off)
#endif
constexpr uint32_t kSortSmallHits = OHMHIP_SORT_SMALL;
constexpr int kSortSmallThreads = 256;

/// Bucket of the ranked ordering: voxel >> shift, per instantiation.  5 is the word of the sample mask (and the walk's
/// own bucket index): 32768 voxels -- the most a key's voxel field holds -- make 1024 buckets, whose counts and positions
/// (at most kSortRegionHits = 8192) are kept as 16-bit halves of 512 LDS words, which the LDS adds address as word + half.
/// Every step down doubles the buckets and their LDS and quarters the compares of a wall (profiles/r09_notes.md).
#ifndef OHMHIP_ORDER_SHIFT_SMALL
#define OHMHIP_ORDER_SHIFT_SMALL 5
#endif
#ifndef OHMHIP_ORDER_SHIFT_DENSE
#define OHMHIP_ORDER_SHIFT_DENSE 5
#endif
#ifndef OHMHIP_ORDER_RANK_LIMIT
#define OHMHIP_ORDER_RANK_LIMIT 32  // a region with sum(count^2) > this * samples runs the network (0: every region)
#endif
constexpr uint32_t kOrderRankLimit = OHMHIP_ORDER_RANK_LIMIT;
static_assert(kSortRegionHits < 65536u, "bucket positions are 16-bit halves");
/// The bits of a sample key below its slot field (voxel, ray): what orders the keys of one region.
constexpr unsigned long long kBelowSlot = (1ull << kHitSlotShift) - 1ull;
static_assert(kSortRegionHits <= (1u << (64 - kHitSlotShift)), "a key's final position travels in its slot field");

/// kCap / kThreads: the instantiation's LDS capacity in keys and workgroup size; it orders the regions of the list with
/// min_hits < samples <= kCap.  A region with ~10^3 samples keeps few lanes of a 1024-thread, 68 KiB workgroup (two per
/// CU) busy between its barriers, so regions of at most kSortSmallHits samples -- nearly all of them -- go to a
/// 256-thread, 19 KiB one that runs eight per CU.  Both move kCap / kThreads = 8 staged keys per lane.
/// `order_counts`: [0] regions ordered by rank, [1] regions ordered by the network (ohmhip_map_order_counts).
/// `walk_lds_hits`: samples of a region the batch's walk shape stages in LDS (G::kLdsHits of k_region_walk).
template <uint32_t kCap, int kThreads>
__global__ void __launch_bounds__(kThreads, 8)
  k_sort_region_hits(RegionTable rt, BatchScratch bs, const unsigned long long *__restrict__ keys,
                     unsigned long long *__restrict__ sorted, int region_voxels, uint32_t min_hits,
                     uint32_t *__restrict__ hit_mask, unsigned long long *__restrict__ order_counts,
                     uint32_t walk_lds_hits)
{
  constexpr uint32_t kPerLane = (kCap + uint32_t(kThreads) - 1u) / uint32_t(kThreads);
  constexpr uint32_t kWaves = uint32_t(kThreads) / 64u;
  // (the scan: every lane of the first kScanLanes takes kScanWords words = 2 * kScanWords buckets)
  constexpr uint32_t kOrderShift = kThreads == kSortThreads ? OHMHIP_ORDER_SHIFT_DENSE : OHMHIP_ORDER_SHIFT_SMALL;
  constexpr uint32_t kOrderWords = ((1u << kHitVoxelBits) >> kOrderShift) / 2u;
  constexpr uint32_t kScanLanes = uint32_t(kThreads) < kOrderWords ? uint32_t(kThreads) : kOrderWords;
  constexpr uint32_t kScanWords = kOrderWords / kScanLanes;
  static_assert(kThreads % 64 == 0 && kCap <= kSortRegionHits, "launch shape");
  __shared__ unsigned long long l_keys[kCap + kCap / 32];
  __shared__ uint32_t l_bucket[kOrderWords];  // per bucket, 16 bits: count -> next free position -> end of its range
  __shared__ uint32_t l_wave_sum[kWaves], l_wave_sq[kWaves];
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
  // (what is computed from the lane's index is computed per region: hoisted out of this loop, the addresses and
  // predicates of the unrolled passes live through the network and take the kernel from 64 to 86 VGPRs -- five
  // workgroups per CU instead of eight)
  uint32_t tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  // ---- histogram: one LDS add per key, and the key staged where the network wants it
  for (uint32_t w = tid; w < kOrderWords; w += kThreads)
  {
    l_bucket[w] = 0;
  }
  __syncthreads();
#pragma unroll 2
  for (uint32_t i = tid; i < n; i += kThreads)
  {
    const unsigned long long key = keys[begin + i];
    l_keys[sortSlot(i)] = key;
    const uint32_t b = hitVoxel(key) >> kOrderShift;
    atomicAdd(&l_bucket[b >> 1], 1u << ((b & 1u) * 16u));
  }
  __syncthreads();
  // ---- scan: counts -> first positions, and W = sum of count^2
  uint32_t sum = 0, sq = 0;
#pragma unroll
  for (uint32_t w = 0; w < kScanWords; ++w)
  {
    const uint32_t word = tid < kScanLanes ? l_bucket[tid * kScanWords + w] : 0u;
    sum += (word & 0xffffu) + (word >> 16);
    sq += (word & 0xffffu) * (word & 0xffffu) + (word >> 16) * (word >> 16);
  }
  uint32_t inclusive = sum;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1)
  {
    const uint32_t up = __shfl_up(inclusive, d, 64);
    inclusive += lane >= d ? up : 0u;
    sq += __shfl_xor(sq, d, 64);
  }
  if (lane == 63u)
  {
    l_wave_sum[wave] = inclusive;
    l_wave_sq[wave] = sq;
  }
  __syncthreads();
  uint32_t position = inclusive - sum, compares = 0;
#pragma unroll
  for (uint32_t w = 0; w < kWaves; ++w)
  {
    position += w < wave ? l_wave_sum[w] : 0u;
    compares += l_wave_sq[w];
  }
  // (the same LDS values for every lane; the compiler is told so, there are barriers on both sides of the branch)
  const bool ranked = kOrderRankLimit != 0 &&
                      __builtin_amdgcn_readfirstlane(compares) <= kOrderRankLimit * n;
  if (ranked)
  {
    if (tid < kScanLanes)
    {
#pragma unroll
      for (uint32_t w = 0; w < kScanWords; ++w)
      {
        const uint32_t word = l_bucket[tid * kScanWords + w];  // (the lane's own words: nobody else writes them)
        const uint32_t first = position;
        position += word & 0xffffu;
        l_bucket[tid * kScanWords + w] = first | (position << 16);
        position += word >> 16;
      }
    }
    __syncthreads();
    // ---- placement: inside its bucket's range, in the order the adds arrive, over the keys staged for the network.
    // (The keys a second time, from L2: held in registers since the histogram they cost the kernel three of its eight
    // workgroups per CU.)  A region's keys share their slot field, so only the 44 bits below it -- voxel, ray -- are
    // staged: the field carries the key's rank.
#pragma unroll 2
    for (uint32_t i = tid; i < n; i += kThreads)
    {
      const unsigned long long key = keys[begin + i];
      const uint32_t b = hitVoxel(key) >> kOrderShift;
      const uint32_t half = (b & 1u) * 16u;
      const uint32_t place = (atomicAdd(&l_bucket[b >> 1], 1u << half) >> half) & 0xffffu;
      l_keys[sortSlot(place)] = key & kBelowSlot;
    }
    __syncthreads();
    // ---- rank: lane i takes the key staged at i; every bucket's word now holds the end of its range.  The final
    // position goes into the staged key's own slot field while other lanes still read that key, with no barrier in
    // between: this is correct only because every reader masks the field -- the 44 bits below it never change, so a
    // read that sees the field before, after or half-way through the write compares the same value.
#pragma unroll 1
    for (uint32_t i = tid; i < n; i += kThreads)
    {
      const unsigned long long key = l_keys[sortSlot(i)];
      const uint32_t b = hitVoxel(key) >> kOrderShift;
      const uint32_t range_end = (l_bucket[b >> 1] >> ((b & 1u) * 16u)) & 0xffffu;
      const uint32_t range_begin = b ? (l_bucket[(b - 1u) >> 1] >> (((b - 1u) & 1u) * 16u)) & 0xffffu : 0u;
      uint32_t rank = 0;
#pragma unroll 4
      for (uint32_t q = range_begin; q < range_end; ++q)
      {
        const unsigned long long other = l_keys[sortSlot(q)] & kBelowSlot;
        rank += (other < key || (other == key && q < i)) ? 1u : 0u;
      }
      l_keys[sortSlot(i)] = key | ((unsigned long long)(range_begin + rank) << kHitSlotShift);
    }
    __syncthreads();
    // ---- every key to its position, the slot field restored
    unsigned long long own[kPerLane];
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; ++j)
    {
      const uint32_t i = j * kThreads + tid;
      own[j] = i < n ? l_keys[sortSlot(i)] : 0ull;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kPerLane; ++j)
    {
      if (j * kThreads + tid < n)
      {
        l_keys[sortSlot(uint32_t(own[j] >> kHitSlotShift))] =
          (own[j] & kBelowSlot) | ((unsigned long long)slot << kHitSlotShift);
      }
    }
    __syncthreads();
  }
  else
  {
    // ---- crowded buckets: the bitonic network over the next power of two
    uint32_t padded = 64;
    while (padded < n)
    {
      padded <<= 1;
    }
    for (uint32_t i = n + tid; i < padded; i += kThreads)  // (the keys are staged since the histogram)
    {
      l_keys[sortSlot(i)] = kHitInvalid;
    }
    __syncthreads();
    bitonicNetwork<kThreads>(l_keys, padded, tid);
  }
  if (threadIdx.x == 0 && order_counts)
  {
    atomicAdd(&order_counts[ranked ? 0 : 1], 1ull);
  }
  uint32_t tail_tid = threadIdx.x;  // (again: nothing of the lane's index lives through the network)
  asm volatile("" : "+v"(tail_tid));
  const uint32_t tail_lane = tail_tid & 63u;
  for (uint32_t base = 0; base < n; base += kThreads)  // (every lane takes every trip: the shuffles below)
  {
    const uint32_t i = base + tail_tid;
    uint32_t word = 0xffffffffu, bits = 0;
    if (i < n)
    {
      const unsigned long long key = l_keys[sortSlot(i)];
      sorted[begin + i] = key;
      const uint32_t vi = hitVoxel(key);
      word = vi >> 5;
      if (i == 0 || hitGroup(l_keys[sortSlot(i - 1)]) != hitGroup(key))
      {
        // First sample of its voxel: the voxel's bit of the sample mask, and the entry point for ordering misses
        // against this voxel's samples.  Only resolveFlaggedMiss reads the entry, and only for a region whose samples
        // the walk cannot stage in LDS (more than `walk_lds_hits`): every other region's misses are ordered against the
        // staged keys, and its scattered stores -- one cache line per sampled voxel -- would be written for nobody.
        if (n > walk_lds_hits)
        {
          bs.voxel_first_hit[size_t(slot) * size_t(region_voxels) + vi] = begin + i;
        }
        bits = 1u << (vi & 31);
      }
    }
    // The keys are in voxel order, so the lanes of a wave whose voxels share a mask word are neighbours: their bits are
    // ORed along each such run and the run's last lane sets them with one atomic (one per voxel, from neighbouring lanes
    // to the same address, cost the two sort launches 32 us per C1 batch).
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1)
    {
      const uint32_t up_bits = __shfl_up(bits, d, 64);
      const uint32_t up_word = __shfl_up(word, d, 64);
      bits |= (tail_lane >= d && up_word == word) ? up_bits : 0u;
    }
    const uint32_t next_word = __shfl_down(word, 1u, 64);
    if (bits && (tail_lane == 63u || next_word != word))
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
