// voxel_edit_kernels.h -- voxels edited by key on the device (include/ohmhip.h, VOXEL EDITS): set,
// ohm::integrateHit(map, key), ohm::integrateMiss(map, key) (ohm/VoxelOccupancy.h:57-108) and ohm::integrateHit(map,
// sample) (ohm/VoxelMean.h:196-203).
//
//   k_edit_tiles    1 lane / element      the packed key of the element's tile (0: a null element), the null count
//   k_edit_locate   1 lane / element      sort key slot << 15 | voxel (all ones: a null element), value = element index
//   k_edit_apply    1 lane / sorted pair  run heads walk their voxel's elements in input order and write the voxel once
//
// Between locate and apply a STABLE radix sort (rocprim::radix_sort_pairs) over the significant bits of the key: every
// voxel's elements end up adjacent and in input order.  No atomic decides an order or a value; the only atomics are the
// counters of the stats and the OR / AND on the replay mask word, where lanes of different voxels share a word.  The
// bit itself is replayMaskBit's (replay_kernels.h), for the kind the host picked (EditArgs::mask_kind).
#ifndef OHMHIP_VOXEL_EDIT_KERNELS_H
#define OHMHIP_VOXEL_EDIT_KERNELS_H

#include "occupancy_math.h"
#include "query_kernels.h"
#include "region_table.h"
#include "replay_kernels.h"

namespace ohmhip
{
constexpr unsigned long long kEditNullKey = ~0ull;
constexpr uint32_t kEditVoxelBits = 15;  ///< a tile holds at most 32768 voxels (MapConst::dim)

enum : uint32_t
{
  kEditCountNull = 0,      ///< null elements
  kEditCountVoxels = 1,    ///< run heads: voxels written
  kEditCountUnplaced = 2,  ///< elements whose tile the region hash does not hold (never, after the regions are named)
  kEditCounters = 4
};

struct EditArgs
{
  MapConst mc;
  RegionTable rt;
  const GpuKeyOut *keys;  ///< [n] or null
  const double *points;   ///< [n][3] or null
  const uint8_t *ops;     ///< [n] or null: every element is `op`
  uint32_t op;
  uint32_t n;
  uint32_t set;  ///< write_voxels: no ops, the layer's bytes are replaced
  unsigned long long *counters;  ///< [kEditCounters]
  // k_edit_tiles
  unsigned long long *tile_keys;  ///< [n]
  // k_edit_locate -> sort -> k_edit_apply
  unsigned long long *sort_keys;
  uint32_t *sort_vals;
  const unsigned long long *sorted_keys;
  const uint32_t *sorted_vals;
  // k_edit_apply
  uint32_t *layer;         ///< SET: the layer written, [slot][tile voxel][voxel_dwords]
  const uint32_t *values;  ///< SET: [n][voxel_dwords]
  uint32_t voxel_dwords;
  float *occupancy;
  uint32_t *mean;  ///< null: the map has no mean layer (updatePositionSafe does nothing)
  uint32_t *hit_mask;
  uint32_t mask_kind;  ///< ReplayMaskKind of the layer written (SET) or of the mean (HIT_SAMPLE)
};

/// Element i: whether it names a voxel, and then the voxel's tile, its index in the tile and its key in the caller's
/// coordinates.  A null key, a point voxelKey() hands Key::kNull for, local coordinates beyond the region, an op outside
/// 1 .. 3, HIT_SAMPLE without points and a tile beyond the packed key's range name none.
__device__ inline bool editElement(const EditArgs &a, uint32_t i, int tile[3], uint32_t &voxel, int region[3], int local[3])
{
  const MapConst &mc = a.mc;
  const uint32_t op = a.set ? uint32_t(OHMHIP_EDIT_HIT) : (a.ops ? uint32_t(a.ops[i]) : a.op);
  if (op < uint32_t(OHMHIP_EDIT_HIT) || op > uint32_t(OHMHIP_EDIT_HIT_SAMPLE))
  {
    return false;
  }
  if (a.points)
  {
    const double p[3] = { a.points[size_t(i) * 3], a.points[size_t(i) * 3 + 1], a.points[size_t(i) * 3 + 2] };
    const bool ok = voxelKey(mc, p, region, local);
    if (keyIsNull(ok, region))
    {
      return false;
    }
  }
  else
  {
    const GpuKeyOut k = a.keys[i];
    for (int c = 0; c < 3; ++c)
    {
      region[c] = int(k.region[c]);
      local[c] = int(k.voxel[c]);
    }
    if (op == uint32_t(OHMHIP_EDIT_HIT_SAMPLE) || keyIsNull(true, region) || local[0] >= mc.kdim[0] ||
        local[1] >= mc.kdim[1] || local[2] >= mc.kdim[2])
    {
      return false;
    }
  }
  const int jy = local[1] / mc.dim[1], jz = local[2] / mc.dim[2];
  tile[0] = region[0];
  tile[1] = region[1] * mc.tile_split[1] + jy;
  tile[2] = region[2] * mc.tile_split[2] + jz;
  if (tile[1] < -32768 || tile[1] > 32767 || tile[2] < -32768 || tile[2] > 32767)
  {
    return false;  // (LARGE REGIONS: the tile key must not wrap onto another tile)
  }
  voxel = uint32_t(local[0]) + uint32_t(local[1] - jy * mc.dim[1]) * uint32_t(mc.dim[0]) +
          uint32_t(local[2] - jz * mc.dim[2]) * uint32_t(mc.dim[0]) * uint32_t(mc.dim[1]);
  return true;
}

/// One add per wave of the lanes with `flag`.
__device__ inline void editCount(unsigned long long *counter, bool flag)
{
  const unsigned long long votes = __ballot(flag);
  if (votes && laneId() == unsigned(__ffsll((long long)votes) - 1))
  {
    atomicAdd(counter, (unsigned long long)__popcll(votes));
  }
}

__global__ void __launch_bounds__(256) k_edit_tiles(EditArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  int tile[3], region[3], local[3];
  uint32_t voxel = 0;
  const bool valid = i < a.n && editElement(a, i, tile, voxel, region, local);
  if (i < a.n)
  {
    a.tile_keys[i] = valid ? packRegionKey(tile[0], tile[1], tile[2]) : 0ull;
    a.sort_vals[i] = i;  // (the sort's value column)
  }
  editCount(a.counters + kEditCountNull, i < a.n && !valid);
}

__global__ void __launch_bounds__(256) k_edit_locate(EditArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  int tile[3], region[3], local[3];
  uint32_t voxel = 0;
  const bool valid = i < a.n && editElement(a, i, tile, voxel, region, local);
  uint32_t slot = kSlotUnassigned;
  if (valid)
  {
    const uint32_t h = regionFind(a.rt, packRegionKey(tile[0], tile[1], tile[2]));
    if (h != 0xffffffffu && a.rt.vals[h] < a.rt.slot_capacity)
    {
      slot = a.rt.vals[h];
    }
  }
  if (i < a.n)
  {
    a.sort_keys[i] = (slot != kSlotUnassigned) ? ((unsigned long long)slot << kEditVoxelBits) | voxel : kEditNullKey;
    a.sort_vals[i] = i;
  }
  editCount(a.counters + kEditCountUnplaced, valid && slot == kSlotUnassigned);
}

/// One lane per sorted pair; the lane of a run's first pair applies the run.
__global__ void __launch_bounds__(256) k_edit_apply(EditArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const MapConst &mc = a.mc;
  const unsigned long long key = (i < a.n) ? a.sorted_keys[i] : kEditNullKey;
  const bool head = key != kEditNullKey && (i == 0 || a.sorted_keys[i - 1] != key);
  editCount(a.counters + kEditCountVoxels, head);
  if (!head)
  {
    return;
  }
  const uint32_t slot = uint32_t(key >> kEditVoxelBits);
  const uint32_t voxel = uint32_t(key) & ((1u << kEditVoxelBits) - 1u);
  const size_t gi = size_t(slot) * size_t(mc.region_voxels) + voxel;
  bool flag = false, flag_known = false;
  if (a.set)
  {
    // E2: the last element in input order wins
    uint32_t j = i;
    while (j + 1 < a.n && a.sorted_keys[j + 1] == key)
    {
      ++j;
    }
    const uint32_t *src = a.values + size_t(a.sorted_vals[j]) * a.voxel_dwords;
    uint32_t *dst = a.layer + gi * a.voxel_dwords;
    for (uint32_t w = 0; w < a.voxel_dwords; ++w)
    {
      dst[w] = src[w];
    }
    if (a.mask_kind != kReplayMaskNone)
    {
      flag = replayMaskBit(a.mask_kind, src[0], src[1], mc.tsdf_trunc);
      flag_known = true;
    }
  }
  else
  {
    float x = a.occupancy[gi];
    uint32_t mcoord = 0, mcount = 0;
    double centre[3] = { 0, 0, 0 };
    bool sampled = false;
    for (uint32_t j = i; j < a.n && a.sorted_keys[j] == key; ++j)
    {
      const uint32_t e = a.sorted_vals[j];
      const uint32_t op = a.ops ? uint32_t(a.ops[e]) : a.op;
      // E3: occupancyAdjustHit / occupancyAdjustMiss with the argument lists of ohm/VoxelOccupancy.h:63-65, 94-96 --
      // the mapper's update without a ray flag
      x = (op == uint32_t(OHMHIP_EDIT_MISS)) ? occMiss(mc, 0u, x) : occHit(mc, 0u, x);
      if (op == uint32_t(OHMHIP_EDIT_HIT_SAMPLE) && a.mean)
      {
        const double p[3] = { a.points[size_t(e) * 3], a.points[size_t(e) * 3 + 1], a.points[size_t(e) * 3 + 2] };
        if (!sampled)
        {
          int region[3], local[3];
          (void)voxelKey(mc, p, region, local);
          for (int c = 0; c < 3; ++c)
          {
            centre[c] = voxelCentreAxis(mc, c, region[c], local[c]);
          }
          mcoord = a.mean[2 * gi];
          mcount = a.mean[2 * gi + 1];
          sampled = true;
        }
        // E4: updatePosition (ohm/VoxelMean.h:158-163); the count saturates
        const double v[3] = { p[0] - centre[0], p[1] - centre[1], p[2] - centre[2] };
        mcoord = subVoxelUpdate(mcoord, mcount, v, mc.resolution);
        mcount = (mcount < 0xfffffffeu ? mcount : 0xfffffffeu) + 1u;
      }
    }
    a.occupancy[gi] = x;
    if (sampled)
    {
      a.mean[2 * gi] = mcoord;
      a.mean[2 * gi + 1] = mcount;
      if (a.mask_kind == kReplayMaskMean)
      {
        flag = replayMaskBit(kReplayMaskMean, mcoord, mcount, mc.tsdf_trunc);
        flag_known = true;
      }
    }
  }
  if (flag_known)
  {
    // E6: the voxel's bit of the ordered-replay mask (replayMaskBit above)
    const uint32_t mask_words = uint32_t(mc.region_voxels + 31) >> 5;
    uint32_t *word = a.hit_mask + size_t(slot) * mask_words + (voxel >> 5);
    if (flag)
    {
      atomicOr(word, 1u << (voxel & 31u));
    }
    else
    {
      atomicAnd(word, ~(1u << (voxel & 31u)));
    }
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_VOXEL_EDIT_KERNELS_H
