// region_table.h -- the device region hash table: packed tile key -> pool slot.  Every stage of the write path inserts
// into it or looks regions up in it, and it is all the read-side kernels (query_kernels.h and the headers built on it)
// need of the integration path.  With it the wave-level helpers both sides share (laneId, shfl64, waveMatch).
#ifndef OHMHIP_REGION_TABLE_H
#define OHMHIP_REGION_TABLE_H

#include "ohmhip_internal.h"

namespace ohmhip
{
struct RegionTable
{
  unsigned long long *keys;  ///< [hash_capacity] packed region key or 0
  uint32_t *vals;            ///< [hash_capacity] slot index
  uint64_t *slot_keys;       ///< [slot_capacity] packed key per slot
  uint32_t *n_slots;         ///< number of slots handed out
  uint32_t hash_mask;
  uint32_t slot_capacity;
};

enum : uint32_t
{
  kErrHashFull = 1u << 0,
  kErrSlotsFull = 1u << 1,
  kErrSegments = 1u << 2
};

// ---------------------------------------------------------------------------------------------------------------------
// Region hash table
// ---------------------------------------------------------------------------------------------------------------------
__device__ inline uint32_t regionInsert(const RegionTable &rt, uint64_t key, uint32_t *error)
{
  uint32_t idx = hashRegionKey(key, rt.hash_mask);
  for (uint32_t probe = 0; probe <= rt.hash_mask; ++probe)
  {
    unsigned long long prev = rt.keys[idx];
    if (prev == 0)
    {
      prev = atomicCAS(&rt.keys[idx], 0ull, (unsigned long long)key);
      if (prev == 0)
      {
        const uint32_t slot = atomicAdd(rt.n_slots, 1u);
        if (slot < rt.slot_capacity)
        {
          rt.slot_keys[slot] = key;
        }
        else
        {
          atomicOr(error, kErrSlotsFull);
        }
        // Published for later kernels; nothing in this kernel reads vals[].
        rt.vals[idx] = slot;
        return idx;
      }
    }
    if (prev == key)
    {
      return idx;
    }
    idx = (idx + 1) & rt.hash_mask;
  }
  atomicOr(error, kErrHashFull);
  return 0;
}

__device__ inline uint32_t regionFind(const RegionTable &rt, uint64_t key)
{
  uint32_t idx = hashRegionKey(key, rt.hash_mask);
  for (uint32_t probe = 0; probe <= rt.hash_mask; ++probe)
  {
    const unsigned long long k = rt.keys[idx];
    if (k == key)
    {
      return idx;
    }
    if (k == 0)
    {
      break;
    }
    idx = (idx + 1) & rt.hash_mask;
  }
  return 0xffffffffu;
}

// ---------------------------------------------------------------------------------------------------------------------
// Wave-level aggregation: lanes with equal 64-bit keys elect a leader which performs one operation for the group.
// ---------------------------------------------------------------------------------------------------------------------
__device__ inline unsigned laneId()
{
  return __lane_id();
}

__device__ inline uint64_t shfl64(uint64_t v, int src)
{
  const uint32_t lo = __shfl(uint32_t(v), src);
  const uint32_t hi = __shfl(uint32_t(v >> 32), src);
  return (uint64_t(hi) << 32) | lo;
}

/// Wave-level match: for every lane with `has`, find the lowest lane holding the same 32-bit value and the mask of all
/// lanes holding it.  Compute only (no memory traffic), one loop trip per distinct value in the wave.
__device__ inline void waveMatch(bool has, uint32_t value, unsigned lane, int &leader, unsigned long long &group)
{
  leader = -1;
  group = 0;
  unsigned long long todo = __ballot(has);
  while (todo)
  {
    const int l = __ffsll((long long)todo) - 1;
    const uint32_t lv = __shfl(value, l);
    const bool mine = has && value == lv;
    const unsigned long long same = __ballot(mine);
    if (mine)
    {
      leader = l;
      group = same;
    }
    todo &= ~same;
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_REGION_TABLE_H
