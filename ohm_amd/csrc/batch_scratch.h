// batch_scratch.h -- what one ray batch keeps between its kernels: the per-region counters, cursors and lists of
// BatchScratch (indexed by the region table's hash index or by pool slot), the regions each binning workgroup feeds
// (WgRegion), the slots' use history (touchRegionUse), and the workgroup-level LDS region table in which k_ray_setup and
// k_ray_bin aggregate their per-region atomics.
#ifndef OHMHIP_BATCH_SCRATCH_H
#define OHMHIP_BATCH_SCRATCH_H

#include "ohmhip_internal.h"

namespace ohmhip
{
/// Per-batch scratch indexed by hash index / slot.
struct BatchScratch
{
  uint32_t *seg_count;     ///< [hash_capacity]
  uint32_t *seg_cursor;    ///< [hash_capacity]
  uint32_t *seg_offset;    ///< [hash_capacity]
  uint32_t *touched_flag;  ///< [hash_capacity]
  uint32_t *touched;       ///< [hash_capacity] list of touched hash indices
  uint32_t *hit_count;     ///< [hash_capacity] samples per region (k_ray_setup -> k_plan, which zeroes it again)
  uint32_t *sort_list;     ///< [hash_capacity] regions receiving samples, most samples first (k_plan -> sort)
  uint32_t *apply_counts_list;  ///< [hash_capacity] regions cut into several chunks: k_apply_counts_list applies their counts
  uint32_t *apply_hits_list;    ///< [hash_capacity] regions whose samples the walk does not replay itself: k_apply_hits_list
  uint32_t *hit_begin;     ///< [slot_capacity] first sample of the region in the sorted list
  uint32_t *hit_end;       ///< [slot_capacity]
  uint32_t *dirty;         ///< [slot_capacity]
  uint32_t *last_use;      ///< [2 x slot_capacity] use history per slot (touchRegionUse; spill to host)
  uint32_t stamp;          ///< this batch's stamp
  /// [slot_capacity * region_voxels] index of a voxel's first sample in the sorted list; written, and read, only for
  /// regions with more samples than the walk stages in LDS (k_sort_region_hits, resolveFlaggedMiss)
  uint32_t *voxel_first_hit;
  BatchInfo *info;
  struct WgRegion *wg_regions;  ///< [workgroups * kLtabSize] regions each binning workgroup feeds (k_ray_setup -> bin)
  uint32_t *wg_region_count;    ///< [workgroups]
};

/// Top bit of BatchScratch::hit_begin[slot], set by the walk kernel once it has replayed the region's samples itself
/// (the array is this batch's own copy -- see ohmhip_map.hip: parity -- and k_plan rewrites the entry of every region a
/// batch touches, so the mark lives exactly from the walk to the end of the batch).
constexpr uint32_t kSamplesApplied = 0x80000000u;

/// One region a binning workgroup feeds: written by k_ray_setup, consumed by k_ray_bin (same workgroup -> rays mapping),
/// which therefore does not have to enumerate the rays' regions a second time just to count.
struct WgRegion
{
  unsigned long long key;
  uint32_t count;  ///< segments of the workgroup's rays in the region
  uint32_t entry;  ///< position in the workgroup's LDS region table
  uint32_t hash;   ///< index in the global region table
  uint32_t hits;   ///< samples of the workgroup's rays in the region
};

__device__ inline void markTouched(const BatchScratch &bs, uint32_t h)
{
  if (bs.touched_flag[h] == 0 && atomicExch(&bs.touched_flag[h], 1u) == 0)
  {
    const uint32_t t = atomicAdd(&bs.info->n_touched, 1u);
    bs.touched[t] = h;
  }
}

/// A region's use history, two words per pool slot: [0] the stamp of the batch that used it last, [1] the stamp of its
/// last use BEFORE the current run of consecutive batches (0: none).  last - before = the period a region comes back with
/// (a sweep that revisits it every N batches), which is what the spill policy predicts its next use from.
__device__ inline void touchRegionUse(uint32_t *use, uint32_t slot, uint32_t stamp)
{
  const uint32_t last = use[2 * size_t(slot)];
  if (last != stamp)
  {
    if (last != 0 && last + 1u != stamp)
    {
      use[2 * size_t(slot) + 1] = last;  // back after a gap
    }
    use[2 * size_t(slot)] = stamp;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Block-level region table in LDS.
//
// Rays of one workgroup cross the same few dozen regions.  Counting (k_ray_setup) and bucket reservation (k_ray_bin)
// therefore aggregate per workgroup in an LDS hash table and touch each global per-region counter ONCE per workgroup:
// the per-region counters of the regions around a sensor are otherwise hit by every wave of the launch, and atomics on
// one address serialise at the memory side (that, not arithmetic, dominated the first version of these kernels).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kBinThreads = 512;        ///< workgroup size of the binning kernels for large batches (launch bound)
constexpr int kBinRaysPerBlock = 1024;  ///< rays per binning workgroup for large batches; small batches use fewer so the
                                        ///< launch still spreads over the CUs (the host picks both per batch)
constexpr uint32_t kLtabSize = 2048;  ///< entries (power of two)

constexpr uint32_t kLtabSmall = 256;  ///< entries of the small-batch instantiations (128-ray workgroups)

/// kTab entries (kLtabSize, or kLtabSmall for the small-batch instantiations of k_ray_setup / k_ray_bin: with the full
/// table's 40 KiB of static LDS only three of their two-wave workgroups fit a CU and the kernels are latency bound).
template <uint32_t kTab>
struct LdsRegionTableT
{
  unsigned long long keys[kTab];
  uint32_t count[kTab];   ///< k_ray_setup: segments of this workgroup in the region; k_ray_bin: sample cursor
  uint32_t cursor[kTab];  ///< k_ray_setup: samples of this workgroup in the region; k_ray_bin: segment cursor
                          ///< (next free global position of the workgroup's reserved range)
};

/// Hash of a packed region key for the workgroups' LDS tables.  The global table's hashRegionKey multiplies 64-bit
/// values -- four quarter-rate 32-bit multiplies on gfx950, ~60 cycles of issue per look-up, and the binning kernels look
/// a region up for every ray-region segment.  Three full-rate 24-bit multiplies of the 16-bit coordinates do here: a
/// workgroup's regions are a compact neighbourhood, odd multipliers spread neighbours over the table.
__device__ inline uint32_t ltabHash(uint64_t key, uint32_t mask)
{
  const uint32_t lo = uint32_t(key);
  const uint32_t h = __umul24(lo & 0xffffu, 0x9E3Bu) ^ __umul24(lo >> 16, 0x85EBu) ^
                     __umul24(uint32_t(key >> 32) & 0xffffu, 0xC2B3u);
  return (h ^ (h >> 11)) & mask;
}

/// Find or insert `key`; returns the entry index or kLtabSize when the table is full (caller falls back to global).
/// `mask` = entries in use - 1 (a power of two <= kLtabSize: small workgroups use a small table so clearing and scanning
/// it does not dominate their run time).
template <uint32_t kTab>
__device__ inline uint32_t ltabFindOrInsert(LdsRegionTableT<kTab> &tab, uint64_t key, uint32_t mask)
{
  uint32_t idx = ltabHash(key, mask);
  for (uint32_t probe = 0; probe < 64; ++probe)
  {
    unsigned long long prev = tab.keys[idx];
    if (prev == 0)
    {
      prev = atomicCAS(&tab.keys[idx], 0ull, (unsigned long long)key);
    }
    if (prev == 0 || prev == key)
    {
      return idx;
    }
    idx = (idx + 1) & mask;
  }
  return kLtabSize;
}

template <uint32_t kTab>
__device__ inline uint32_t ltabFind(const LdsRegionTableT<kTab> &tab, uint64_t key, uint32_t mask)
{
  uint32_t idx = ltabHash(key, mask);
  for (uint32_t probe = 0; probe < 64; ++probe)
  {
    const unsigned long long k = tab.keys[idx];
    if (k == key)
    {
      return idx;
    }
    if (k == 0)
    {
      break;
    }
    idx = (idx + 1) & mask;
  }
  return kLtabSize;
}
}  // namespace ohmhip

#endif  // OHMHIP_BATCH_SCRATCH_H
