// apply_kernels.h -- the apply stage of the occupancy ray-integration path: what the walk left in global counters
// becomes voxel values (gfx950).
//
//   k_apply_hits        1 lane / sample    ordered replay (misses-before-hit counts, hit, mean) for voxels with samples
//   k_apply_counts      1 workgroup/region remaining miss counts of multi-chunk regions, clear scratch
//   k_apply_lists       occupancy-only maps: both of the above, over the listed regions that still need them
//   k_batch_cleanup     1 workgroup/region every touched region's mask and scratch back to idle
#ifndef OHMHIP_APPLY_KERNELS_H
#define OHMHIP_APPLY_KERNELS_H

#include "batch_scratch.h"
#include "occupancy_math.h"
#include "region_table.h"
#include "secondary_device.h"

namespace ohmhip
{
// ---------------------------------------------------------------------------------------------------------------------
// k_apply_hits: one lane per sorted hit; the first hit of each voxel group replays the whole group in ray order.
// ---------------------------------------------------------------------------------------------------------------------
__device__ inline void applyHits(uint32_t i, const MapConst &mc, const RegionTable &rt, const BatchScratch &bs,
                                 unsigned ray_flags, const unsigned long long *__restrict__ sorted,
                                 uint32_t *__restrict__ interval_counts, uint32_t *__restrict__ miss_counts,
                                 const double *__restrict__ rays, float *__restrict__ occupancy,
                                 uint32_t *__restrict__ mean, const SecondaryLayers &sec,
                                 const RayWalk *__restrict__ walks)
{
  const uint32_t n_hits = bs.info->n_hits;
  if (i >= n_hits)
  {
    return;
  }
  const unsigned long long key = sorted[i];
  const unsigned long long group = hitGroup(key);  // slot | voxel
  if (i > 0 && hitGroup(sorted[i - 1]) == group)
  {
    return;  // not the head of its voxel group
  }
  const uint32_t slot = hitSlot(key);
  if (bs.hit_begin[slot] & kSamplesApplied)
  {
    return;  // the walk kernel replayed this region's samples itself (WalkArgs::inline_hits)
  }
  const uint32_t vi = hitVoxel(key);
  const size_t gi = size_t(slot) * size_t(mc.region_voxels) + vi;
  float x = occupancy[gi];

  uint32_t mcoord = 0, mcount = 0;
  double centre[3] = { 0, 0, 0 };
  if (mean)
  {
    mcoord = mean[2 * gi];
    mcount = mean[2 * gi + 1];
    int16_t rk[3];
    unpackRegionKey(rt.slot_keys[slot], rk);
    const int lx = int(vi % uint32_t(mc.dim[0]));
    const int ly = int((vi / uint32_t(mc.dim[0])) % uint32_t(mc.dim[1]));
    const int lz = int(vi / uint32_t(mc.dim[0] * mc.dim[1]));
    centre[0] = globalVoxelCentreAxis(mc, 0, int(rk[0]) * mc.dim[0] + lx);
    centre[1] = globalVoxelCentreAxis(mc, 1, int(rk[1]) * mc.dim[1] + ly);
    centre[2] = globalVoxelCentreAxis(mc, 2, int(rk[2]) * mc.dim[2] + lz);
  }

  uint32_t packed_normal = sec.incident ? sec.incident[gi] : 0u;
  float traversal_add = 0.0f;
  float traversal = sec.traversal ? sec.traversal[gi] : 0.0f;
  uint32_t last_ray = 0;
  for (uint32_t j = i; j < n_hits && hitGroup(sorted[j]) == group; ++j)
  {
    x = occMissN(mc, ray_flags, x, interval_counts[j]);
    interval_counts[j] = 0;
    x = occHit(mc, ray_flags, x);
    const uint32_t ray = uint32_t(sorted[j] & ((1ull << kHitRayBits) - 1ull));
    last_ray = ray;
    if (sec.incident)
    {
      // ohm/RayMapperOccupancy.cpp:319-325: incident ray = start - end (converted to float), weight = sample count
      // before this sample (0 without a mean layer).
      const float dir[3] = { float(rays[size_t(ray) * 6 + 0] - rays[size_t(ray) * 6 + 3]),
                             float(rays[size_t(ray) * 6 + 1] - rays[size_t(ray) * 6 + 4]),
                             float(rays[size_t(ray) * 6 + 2] - rays[size_t(ray) * 6 + 5]) };
      packed_normal = updateIncidentNormal(packed_normal, dir, mean ? mcount : 0u);
    }
    if (sec.traversal)
    {
      // ohm/RayMapperOccupancy.cpp:299-305: remaining ray length inside the sample voxel.
      const double dx = rays[size_t(ray) * 6 + 3] - rays[size_t(ray) * 6 + 0];
      const double dy = rays[size_t(ray) * 6 + 4] - rays[size_t(ray) * 6 + 1];
      const double dz = rays[size_t(ray) * 6 + 5] - rays[size_t(ray) * 6 + 2];
      traversal += float(sqrt((dx * dx + dy * dy) + dz * dz) - lastExitRange(walks, ray));
    }
    if (mean)
    {
      // NOTE: uses the ray's sample as submitted; the clip filter never applies a hit to a moved end point.
      const double local[3] = { rays[size_t(ray) * 6 + 3] - centre[0], rays[size_t(ray) * 6 + 4] - centre[1],
                                rays[size_t(ray) * 6 + 5] - centre[2] };
      mcoord = subVoxelUpdate(mcoord, mcount, local, mc.resolution);
      ++mcount;
    }
  }
  // Misses after the last hit.
  x = occMissN(mc, ray_flags, x, miss_counts[gi]);
  miss_counts[gi] = 0;
  occupancy[gi] = x;
  if (mean)
  {
    mean[2 * gi] = mcoord;
    mean[2 * gi + 1] = mcount;
  }
  (void)traversal_add;
  if (sec.incident)
  {
    sec.incident[gi] = packed_normal;
  }
  if (sec.traversal)
  {
    sec.traversal[gi] = traversal;
  }
  if (sec.touch_time && sec.timestamps)
  {
    // The CPU mapper overwrites the touch time at every sample: the last sample in ray order wins
    // (ohm/RayMapperOccupancy.cpp:313-317).
    sec.touch_time[gi] = encodeVoxelTouchTime(sec.time_base, sec.timestamps[last_ray]);
  }
}

__global__ void __launch_bounds__(256)
  k_apply_hits(MapConst mc, RegionTable rt, BatchScratch bs, unsigned ray_flags,
               const unsigned long long *__restrict__ sorted, uint32_t *__restrict__ interval_counts,
               uint32_t *__restrict__ miss_counts, const double *__restrict__ rays, float *__restrict__ occupancy,
               uint32_t *__restrict__ mean, SecondaryLayers sec, const RayWalk *__restrict__ walks)
{
  applyHits(blockIdx.x * blockDim.x + threadIdx.x, mc, rt, bs, ray_flags, sorted, interval_counts, miss_counts, rays,
            occupancy, mean, sec, walks);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_apply_counts: one block per touched region: apply plain miss counts, clear scratch.
// ---------------------------------------------------------------------------------------------------------------------

constexpr double kTraversalScale = 1099511627776.0;  ///< 2^40 fixed-point units per metre of traversal

/// `skip_masked`: voxels whose mask bit is set are somebody else's (NDT: the ordered replay; occupancy, when this runs
/// beside applyHits in one launch: applyHits) -- their counts are neither applied nor touched.
__device__ inline void applyCounts(uint32_t region_index, const MapConst &mc, const RegionTable &rt,
                                   const BatchScratch &bs, unsigned ray_flags, uint32_t *__restrict__ miss_counts,
                                   uint32_t *__restrict__ hit_mask, float *__restrict__ occupancy, int clear_mask,
                                   uint32_t *__restrict__ hit_miss_counts, uint32_t direct_chunk_segments,
                                   int skip_masked, int preserve_masked, float *__restrict__ traversal = nullptr,
                                   unsigned long long *__restrict__ traversal_acc = nullptr)
{
  const uint32_t h = bs.touched[region_index];
  const uint32_t slot = rt.vals[h];
  const size_t base = size_t(slot) * size_t(mc.region_voxels);
  // Regions with a single chunk were applied by the walk kernel itself (direct_chunk_segments != 0).
  const bool applied_by_walk = direct_chunk_segments && bs.seg_count[h] > 0 && bs.seg_count[h] <= direct_chunk_segments;
  if (!applied_by_walk)
  {
    // 4 voxels per lane per step: 16-byte loads of the count and log-odds layers (region blocks are 16-byte aligned
    // whenever region_voxels is a multiple of 4; otherwise fall back to scalar accesses).
    const uint32_t n4 = (mc.region_voxels % 4 == 0) ? uint32_t(mc.region_voxels) / 4u : 0u;
    uint4 *counts4 = reinterpret_cast<uint4 *>(miss_counts + base);
    float4 *occ4 = reinterpret_cast<float4 *>(occupancy + base);
    const uint32_t *mask = hit_mask + size_t(slot) * (uint32_t(mc.region_voxels + 31) >> 5);
    for (uint32_t q = threadIdx.x; q < n4; q += blockDim.x)
    {
      uint4 n = counts4[q];
      if (n.x | n.y | n.z | n.w)
      {
        uint32_t bits = 0;
        if (skip_masked)
        {
          // NDT: voxels holding samples are updated by the ordered replay only; their tile entry is not used.
          bits = (mask[(4 * q) >> 5] >> ((4 * q) & 31)) & 15u;
          n.x = (bits & 1u) ? 0u : n.x;
          n.y = (bits & 2u) ? 0u : n.y;
          n.z = (bits & 4u) ? 0u : n.z;
          n.w = (bits & 8u) ? 0u : n.w;
        }
        const float4 before = occ4[q];
        float4 o = before;
        o.x = n.x ? occMissN(mc, ray_flags, o.x, n.x) : o.x;
        o.y = n.y ? occMissN(mc, ray_flags, o.y, n.y) : o.y;
        o.z = n.z ? occMissN(mc, ray_flags, o.z, n.z) : o.z;
        o.w = n.w ? occMissN(mc, ray_flags, o.w, n.w) : o.w;
        // (voxels at their clamp do not move: a settled map's free space needs no log-odds write)
        const bool moved = !sameValue(o.x, before.x) || !sameValue(o.y, before.y) || !sameValue(o.z, before.z) ||
                           !sameValue(o.w, before.w);
        if (preserve_masked && bits)
        {
          // A masked voxel's log-odds and count belong to applyHits, which may be at work on them right now: only the
          // other voxels of the group are written.
          float *o1 = occupancy + base + 4 * q;
          uint32_t *c1 = miss_counts + base + 4 * q;
          if (!(bits & 1u)) { o1[0] = o.x; c1[0] = 0; }
          if (!(bits & 2u)) { o1[1] = o.y; c1[1] = 0; }
          if (!(bits & 4u)) { o1[2] = o.z; c1[2] = 0; }
          if (!(bits & 8u)) { o1[3] = o.w; c1[3] = 0; }
        }
        else
        {
          if (moved)
          {
            occ4[q] = o;
          }
          counts4[q] = make_uint4(0, 0, 0, 0);
        }
        if (hit_miss_counts)
        {
          // NDT-TM: every plain miss increments HitMissCount::miss_count (ohm/RayMapperNdt.cpp:171-178).
          hit_miss_counts[2 * (base + 4 * q + 0) + 1] += n.x;
          hit_miss_counts[2 * (base + 4 * q + 1) + 1] += n.y;
          hit_miss_counts[2 * (base + 4 * q + 2) + 1] += n.z;
          hit_miss_counts[2 * (base + 4 * q + 3) + 1] += n.w;
        }
      }
    }
    for (uint32_t vi = 4 * n4 + threadIdx.x; vi < uint32_t(mc.region_voxels); vi += blockDim.x)
    {
      uint32_t n = miss_counts[base + vi];
      if (n && skip_masked && ((mask[vi >> 5] >> (vi & 31)) & 1u))
      {
        if (!preserve_masked)
        {
          miss_counts[base + vi] = 0;
        }
        n = 0;
      }
      if (n)
      {
        occupancy[base + vi] = occMissN(mc, ray_flags, occupancy[base + vi], n);
        miss_counts[base + vi] = 0;
        if (hit_miss_counts)
        {
          hit_miss_counts[2 * (base + vi) + 1] += n;
        }
      }
    }
  }
  if (traversal_acc)
  {
    // This batch's ray lengths through the region's voxels (k_region_traversal, traversal_kernels.h), summed exactly.
    for (uint32_t vi = threadIdx.x; vi < uint32_t(mc.region_voxels); vi += blockDim.x)
    {
      const unsigned long long sum = traversal_acc[base + vi];
      if (sum)
      {
        traversal[base + vi] = float(double(traversal[base + vi]) + double(sum) * (1.0 / kTraversalScale));
        traversal_acc[base + vi] = 0;
      }
    }
  }
  if (clear_mask)
  {
    __syncthreads();  // (the loops above read the mask)
    const uint32_t mask_words = uint32_t(mc.region_voxels + 31) >> 5;
    for (uint32_t i = threadIdx.x; i < mask_words; i += blockDim.x)
    {
      hit_mask[size_t(slot) * mask_words + i] = 0;
    }
  }
  if (threadIdx.x == 0)
  {
    bs.seg_count[h] = 0;
    bs.seg_cursor[h] = 0;
    bs.touched_flag[h] = 0;
  }
}

__global__ void __launch_bounds__(1024)
  k_apply_counts(MapConst mc, RegionTable rt, BatchScratch bs, unsigned ray_flags, uint32_t *__restrict__ miss_counts,
                 uint32_t *__restrict__ hit_mask, float *__restrict__ occupancy, int clear_mask,
                 uint32_t *__restrict__ hit_miss_counts, uint32_t direct_chunk_segments, int skip_masked,
                 float *__restrict__ traversal, unsigned long long *__restrict__ traversal_acc)
{
  applyCounts(blockIdx.x, mc, rt, bs, ray_flags, miss_counts, hit_mask, occupancy, clear_mask, hit_miss_counts,
              direct_chunk_segments, skip_masked, 0, traversal, traversal_acc);
}

// ---------------------------------------------------------------------------------------------------------------------
// The apply phase of occupancy-only maps (round 5).  The walk kernel applies every region it holds in ONE chunk itself --
// counts and samples, straight from LDS -- so in the steady state of C1 the two kernels above found work in ~80 of
// 1243 regions and spent their 46 us on workgroups and lanes that looked at a region or a sample and left.  k_plan now
// lists the regions that DO need them (BatchScratch::apply_counts_list / apply_hits_list): the kernels below run over
// those lists only, and the per-region bookkeeping every touched region needs moves to k_batch_cleanup.
// ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kApplyListParts = 16;  ///< workgroups sharing one listed region's count application (whole mask words each)

/// One launch for both lists (256-thread workgroups; the first hit_blocks of them replay samples, the others apply
/// counts): a listed region's samples and its plain counts touch DIFFERENT voxels -- the count part skips every voxel
/// whose sample-mask bit is set, those counts are the sample replay's (which applies and clears them) -- so the two run
/// side by side instead of one behind the other (22 + 17 us as two launches: both are chains of dependent loads).
///   sample part: workgroup (r, p) replays samples [256 p, 256 p + 256) of listed region r -- one lane per sample, the
///     head of a voxel's run replays the run (applyHits); blocks_per_region covers the batch's densest region
///   count part: workgroup (r, p) applies 1 / kApplyListParts of listed region r's counts (whole mask words)
__global__ void __launch_bounds__(256)
  k_apply_lists(MapConst mc, RegionTable rt, BatchScratch bs, unsigned ray_flags,
                const unsigned long long *__restrict__ sorted, uint32_t *__restrict__ interval_counts,
                uint32_t *__restrict__ miss_counts, const uint32_t *__restrict__ hit_mask,
                const double *__restrict__ rays, float *__restrict__ occupancy, uint32_t hit_blocks,
                uint32_t blocks_per_region, unsigned long long hit_tiles)
{
  if (blockIdx.x < hit_blocks)
  {
    // (region, 256-sample tile) pairs, strided over the sample part's workgroups: hit_blocks == hit_tiles except for
    // skewed multi-million-ray batches, whose product of listed regions and tiles of the densest one is capped by the
    // host (the product used to be the grid, in 32 bits).
    for (unsigned long long tile = blockIdx.x; tile < hit_tiles; tile += hit_blocks)
    {
      const uint32_t slot = rt.vals[bs.apply_hits_list[uint32_t(tile / blocks_per_region)]];
      if (slot >= rt.slot_capacity)
      {
        continue;
      }
      const uint32_t begin = bs.hit_begin[slot] & ~kSamplesApplied;
      const uint32_t i = begin + uint32_t(tile % blocks_per_region) * 256u + threadIdx.x;
      if (i < bs.hit_end[slot])
      {
        SecondaryLayers none{};
        applyHits(i, mc, rt, bs, ray_flags, sorted, interval_counts, miss_counts, rays, occupancy, nullptr, none,
                  nullptr);
      }
    }
    return;
  }
  const uint32_t block = blockIdx.x - hit_blocks;
  const uint32_t h = bs.apply_counts_list[block / kApplyListParts];
  const uint32_t part = block % kApplyListParts;
  const uint32_t slot = rt.vals[h];
  if (slot >= rt.slot_capacity)
  {
    return;
  }
  const size_t base = size_t(slot) * size_t(mc.region_voxels);
  const uint32_t words = uint32_t(mc.region_voxels + 31) >> 5;
  const uint32_t *mask = hit_mask + size_t(slot) * words;
  const uint32_t v_lo = uint32_t(uint64_t(words) * part / kApplyListParts) * 32u;
  const uint32_t v_hi = min(uint32_t(uint64_t(words) * (part + 1u) / kApplyListParts) * 32u, uint32_t(mc.region_voxels));
  if (mc.region_voxels % 4 == 0)
  {
    uint4 *counts4 = reinterpret_cast<uint4 *>(miss_counts + base);
    float4 *occ4 = reinterpret_cast<float4 *>(occupancy + base);
    for (uint32_t q = v_lo / 4u + threadIdx.x; q < v_hi / 4u; q += blockDim.x)
    {
      uint4 n = counts4[q];
      if (n.x | n.y | n.z | n.w)
      {
        const uint32_t bits = (mask[(4u * q) >> 5] >> ((4u * q) & 31u)) & 15u;
        n.x = (bits & 1u) ? 0u : n.x;
        n.y = (bits & 2u) ? 0u : n.y;
        n.z = (bits & 4u) ? 0u : n.z;
        n.w = (bits & 8u) ? 0u : n.w;
        const float4 before = occ4[q];
        float4 o = before;
        o.x = n.x ? occMissN(mc, ray_flags, o.x, n.x) : o.x;
        o.y = n.y ? occMissN(mc, ray_flags, o.y, n.y) : o.y;
        o.z = n.z ? occMissN(mc, ray_flags, o.z, n.z) : o.z;
        o.w = n.w ? occMissN(mc, ray_flags, o.w, n.w) : o.w;
        // (only the voxels that are this part's: a masked voxel's log-odds and count may be under the sample replay's
        // hands right now)
        float *o1 = occupancy + base + 4 * q;
        uint32_t *c1 = miss_counts + base + 4 * q;
        if (n.x) { if (!sameValue(o.x, before.x)) { o1[0] = o.x; } c1[0] = 0; }
        if (n.y) { if (!sameValue(o.y, before.y)) { o1[1] = o.y; } c1[1] = 0; }
        if (n.z) { if (!sameValue(o.z, before.z)) { o1[2] = o.z; } c1[2] = 0; }
        if (n.w) { if (!sameValue(o.w, before.w)) { o1[3] = o.w; } c1[3] = 0; }
      }
    }
    return;
  }
  for (uint32_t vi = v_lo + threadIdx.x; vi < v_hi; vi += blockDim.x)
  {
    const uint32_t n = miss_counts[base + vi];
    if (n && !((mask[vi >> 5] >> (vi & 31u)) & 1u))
    {
      occupancy[base + vi] = occMissN(mc, ray_flags, occupancy[base + vi], n);
      miss_counts[base + vi] = 0;
    }
  }
}

/// Every touched region back to its idle state: the sample mask cleared, the per-batch scratch reset (what applyCounts
/// does for a region when k_apply_counts runs over all of them).
__global__ void __launch_bounds__(256)
  k_batch_cleanup(MapConst mc, RegionTable rt, BatchScratch bs, uint32_t n_touched, uint32_t *__restrict__ hit_mask)
{
  const uint32_t mask_words = uint32_t(mc.region_voxels + 31) >> 5;
  for (uint32_t r = blockIdx.x; r < n_touched; r += gridDim.x)
  {
    const uint32_t h = bs.touched[r];
    const uint32_t slot = rt.vals[h];
    if (slot < rt.slot_capacity)
    {
      for (uint32_t w = threadIdx.x; w < mask_words; w += blockDim.x)
      {
        hit_mask[size_t(slot) * mask_words + w] = 0;
      }
    }
    if (threadIdx.x == 0)
    {
      bs.seg_count[h] = 0;
      bs.seg_cursor[h] = 0;
      bs.touched_flag[h] = 0;
    }
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_APPLY_KERNELS_H
