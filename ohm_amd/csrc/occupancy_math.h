// occupancy_math.h -- the per-voxel arithmetic of the occupancy mapper, shared by the walk kernel's inline apply and the
// apply kernels.
//
// Ordering argument (why integer counting reproduces the sequential CPU result exactly): every miss applies the
// same function m(x) and every hit the same h(x) to a voxel's value.  The CPU result for a voxel is the composition
// of its events in ray order; that composition is fully determined by the NUMBER of misses between consecutive
// hits.  Integer atomics are order-independent, so counting is deterministic, and the float updates are then
// replayed one voxel per lane in exactly the CPU order -> bit-identical log-odds.
#ifndef OHMHIP_OCCUPANCY_MATH_H
#define OHMHIP_OCCUPANCY_MATH_H

#include "walk_device.h"

namespace ohmhip
{
// ---------------------------------------------------------------------------------------------------------------------
// Occupancy update functions (bit-for-bit the CPU mapper's per-voxel arithmetic).
// ---------------------------------------------------------------------------------------------------------------------
__device__ inline float fInf()
{
  return __int_as_float(0x7f800000);
}

/// Whether two log-odds are the same stored value.  The write guards of the apply kernels ask this, not ==: the CPU
/// mapper stores every result, so a -0.0 that receives a zero adjustment (an excluding flag, a saturated voxel, a miss
/// probability of 0.5) becomes +0.0 -- equal to what was there, and another value.
__device__ inline bool sameValue(float a, float b)
{
  return __float_as_uint(a) == __float_as_uint(b);
}

/// One miss: ohm/RayMapperOccupancy.cpp:143-163 + ohm/VoxelOccupancyCompute.h:110-120 (null_update == false).
__device__ inline float occMiss(const MapConst &mc, unsigned ray_flags, float initial)
{
  const float inf = fInf();
  const bool unobserved = initial == inf;
  const bool is_free = !unobserved && initial < mc.threshold_value;
  const bool is_occ = !unobserved && initial >= mc.threshold_value;
  float adj = mc.miss_value;
  adj = (unobserved && (ray_flags & OHMHIP_RF_EXCLUDE_UNOBSERVED)) ? inf : adj;
  adj = (is_free && (ray_flags & OHMHIP_RF_EXCLUDE_FREE)) ? 0.0f : adj;
  adj = (is_occ && (ray_flags & OHMHIP_RF_EXCLUDE_OCCUPIED)) ? 0.0f : adj;
  const float base = unobserved ? 0.0f : initial;
  adj = (unobserved || (mc.sat_min < initial && initial < mc.sat_max)) ? adj : 0.0f;
  return (base != inf) ? fmaxf(mc.min_value, base + adj) : base;
}

/// One hit: ohm/RayMapperOccupancy.cpp:261-281 + ohm/VoxelOccupancyCompute.h:44-54.
__device__ inline float occHit(const MapConst &mc, unsigned ray_flags, float initial)
{
  const float inf = fInf();
  const bool unobserved = initial == inf;
  const bool is_free = !unobserved && initial < mc.threshold_value;
  const bool is_occ = !unobserved && initial >= mc.threshold_value;
  float adj = mc.hit_value;
  adj = (unobserved && (ray_flags & OHMHIP_RF_EXCLUDE_UNOBSERVED)) ? inf : adj;
  adj = (is_free && (ray_flags & OHMHIP_RF_EXCLUDE_FREE)) ? 0.0f : adj;
  adj = (is_occ && (ray_flags & OHMHIP_RF_EXCLUDE_OCCUPIED)) ? 0.0f : adj;
  const float base = unobserved ? 0.0f : initial;
  adj = (unobserved || (mc.sat_min < initial && initial < mc.sat_max)) ? adj : 0.0f;
  return (base != inf) ? fminf(base + adj, mc.max_value) : base;
}

/// A null update (ohm/VoxelOccupancyCompute.h:110-120 with null_update == true): what a ray stopped by
/// kRfStopOnFirstOccupied gives the voxels behind its stop.  Not the identity: base + 0.0f and the min clamp still run, so
/// a value below min, a NaN and -inf become min and -0.0 becomes +0.0.
__device__ inline float occNullMiss(const MapConst &mc, float initial)
{
  return (initial != fInf()) ? fmaxf(mc.min_value, initial + 0.0f) : initial;
}

/// n sequential misses.  The update is a deterministic function of the value alone, so once it reaches a fixed point
/// (the min clamp) the remaining applications are the identity and can be skipped without changing the result.  The exit
/// returns the update's OUTPUT: nx == x holds for the same value and for (x, nx) = (-0.0, +0.0), a -0.0 that received a
/// zero adjustment -- there the CPU mapper has stored +0.0, and +0.0 is a fixed point (the update never tells the two
/// zeros apart, and +0.0 + 0.0f is +0.0).
__device__ inline float occMissN(const MapConst &mc, unsigned ray_flags, float x, uint32_t n)
{
  constexpr unsigned kExcludeFlags = OHMHIP_RF_EXCLUDE_UNOBSERVED | OHMHIP_RF_EXCLUDE_FREE | OHMHIP_RF_EXCLUDE_OCCUPIED;
  if (n == 0)
  {
    return x;
  }
  if (!(ray_flags & kExcludeFlags))
  {
    // Without the exclusion flags only the FIRST miss can meet an unobserved voxel; every later one is occMiss() of an
    // observed value, which is these three operations (same operations, same order: bit identical) -- a voxel that is
    // not yet at the clamp pays them up to ~10 times per batch (a map the sensor is moving through).
    // The first miss is occMiss() with the exclusion flags known to be clear: its three flag selects and the free / occupied
    // classification drop out, the remaining operations are the same in the same order (bit identical; -3 us per C1 batch).
    const bool unobserved = x == fInf();
    const float base = unobserved ? 0.0f : x;
    const float first_adj = (unobserved || (mc.sat_min < x && x < mc.sat_max)) ? mc.miss_value : 0.0f;
    float nx = fmaxf(mc.min_value, base + first_adj);
    if (nx == x)
    {
      return nx;
    }
    x = nx;
    for (uint32_t k = 1; k < n; ++k)
    {
      const float adj = (mc.sat_min < x && x < mc.sat_max) ? mc.miss_value : 0.0f;
      nx = fmaxf(mc.min_value, x + adj);
      const bool fixed = nx == x;
      x = nx;
      if (fixed)
      {
        break;
      }
    }
    return x;
  }
  for (uint32_t k = 0; k < n; ++k)
  {
    const float nx = occMiss(mc, ray_flags, x);
    const bool fixed = nx == x;
    x = nx;
    if (fixed)
    {
      break;
    }
  }
  return x;
}

/// The constants of a miss, by value: what a function that is not inlined into its kernel is handed in registers.
struct MissConst
{
  float miss_value, min_value, sat_min, sat_max;
};

/// occMissN() for a batch without exclusion flags, written for a whole wave: the walk's lean direct apply calls it for
/// every lane of a tile word, whatever the lane's n.  The first application is occMissN()'s plain path without its
/// branches (same operations, same order: bit identical); the repeat loop -- only voxels that are not yet at the clamp
/// need it -- is entered when some lane of the wave has n > 1 and a value the first miss moved.  n == 0 returns x itself,
/// bit for bit, so the caller's sameValue() write guard also covers "nothing to apply".
__device__ inline float occMissNPlainWave(const MissConst mc, float x, uint32_t n)
{
  const bool unobserved = x == fInf();
  const float base = unobserved ? 0.0f : x;
  // (& and |: the compiler turns && and || into branches around the comparisons)
  const bool first_moves = unobserved | ((mc.sat_min < x) & (x < mc.sat_max));
  const float first_adj = first_moves ? mc.miss_value : 0.0f;
  float nx = fmaxf(mc.min_value, base + first_adj);
  const bool repeat = (n > 1u) & !(nx == x);
  if (__ballot(repeat))
  {
    if (repeat)
    {
      float cur = nx;
      for (uint32_t k = 1; k < n; ++k)
      {
        const float adj = (mc.sat_min < cur && cur < mc.sat_max) ? mc.miss_value : 0.0f;
        nx = fmaxf(mc.min_value, cur + adj);
        const bool fixed = nx == cur;
        cur = nx;
        if (fixed)
        {
          break;
        }
      }
    }
  }
  return n ? nx : x;
}

/// ohm/VoxelMeanCompute.h:134-152 with Vec3 = dvec3, coord_real = double (as the CPU mappers instantiate it).
__device__ inline uint32_t subVoxelUpdate(uint32_t coord, uint32_t point_count, const double v[3], double resolution)
{
  const int mean_positions = (1 << 10) - 1;
  const double mean_resolution = resolution / double(mean_positions);
  const double offset = double(0.5f) * resolution;
  double mean[3];
  mean[0] = int(coord & mean_positions) * mean_resolution - offset;
  mean[1] = int((coord >> 10) & mean_positions) * mean_resolution - offset;
  mean[2] = int((coord >> 20) & mean_positions) * mean_resolution - offset;
  const double one_on_count_plus_one = double(1) / double(point_count + 1);
  uint32_t pattern = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    mean[a] += (v[a] - mean[a]) * one_on_count_plus_one;
    int pos = pointToRegionCoord(mean[a] + offset, mean_resolution);
    pos = (pos >= 0 ? (pos < (1 << 10) ? pos : mean_positions) : 0);
    pattern |= uint32_t(pos) << (10 * a);
  }
  return pattern | (1u << 31);
}
}  // namespace ohmhip

#endif  // OHMHIP_OCCUPANCY_MATH_H
