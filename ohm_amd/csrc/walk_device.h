// walk_device.h -- fp64 device maths shared by the gfx950 kernels: voxel keys, voxel centres, line-walk set-up, the
// closed-form "resume the walk at step (axis, j)" that lets a region workgroup pick a ray up mid-walk, the exact
// next-axis decision (timeNext / nextAxis / exactNextAxis) and LaneWalk, the one voxel-by-voxel walker of the kernels
// that walk a whole ray in one lane (k_line_keys, k_tsdf_flag, k_rays_query).  The key maths (hostInt ... voxelCentreAxis)
// is __host__ __device__: the host computes its keys with the very functions the kernels use.
//
// Everything here follows the CPU instantiation of the reference's shared compute headers (WalkReal = double) with
// the same operation order; the library is compiled with -ffp-contract=off so no FMA is formed, and fp64 divide /
// sqrt are IEEE on gfx950.  Citations are reference file:line.
#ifndef OHMHIP_WALK_DEVICE_H
#define OHMHIP_WALK_DEVICE_H

#include "ohmhip_internal.h"

namespace ohmhip
{
__device__ inline double dInf()
{
  return __longlong_as_double(0x7ff0000000000000ll);
}

/// double -> int the way the host the reference runs on does it (x86 cvttsd2si): values outside the int range and
/// NaN give INT_MIN, where the device conversion would saturate.  Only matters for absurd inputs (points 10^5 km from
/// the map origin), but those still have to produce the same keys as the CPU mapper.
__host__ __device__ inline int hostInt(double v)
{
  return (v >= -2147483648.0 && v < 2147483648.0) ? int(v) : int(0x80000000u);
}

/// ohm/MapCoord.h:85-93
__host__ __device__ inline int pointToRegionCoord(double coord, double resolution)
{
  return hostInt(floor(coord / resolution + 0.5));
}

/// ohm/MapCoord.h:45-80
__host__ __device__ inline int pointToRegionVoxel(double coord, double voxel_resolution, double region_resolution)
{
  const double epsilon = double(1e-6f);
  if (-epsilon <= coord && coord < 0)
  {
    coord = 0;
  }
  else if (coord >= region_resolution && coord - epsilon < region_resolution)
  {
    coord -= epsilon;
  }
  return hostInt(floor(coord / voxel_resolution));
}

/// ohm/OccupancyMap.cpp:859-886 -> ohm/MapRegion.cpp:32-69.  Returns false when the point is not addressable (the
/// reference then hands out Key::kNull).  See keyIsNull() for the one addressable key that still reads as null.
/// @param[out] region Region coordinate per axis.
/// @param[out] local Local voxel coordinate per axis.
/// @param[out] beyond_tiles Optional: set when the point is addressable in the reference's sense and only the tile
///   coordinates of a map cut into tiles leave the key's range.
__host__ __device__ inline bool voxelKey(const MapConst &mc, const double p[3], int region[3], int local[3],
                                         bool *beyond_tiles = nullptr)
{
  bool ok = true;
  bool tiles_ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    const int coord = pointToRegionCoord(p[a] - mc.origin[a], mc.region_dim[a]);
    // The reference stores the region coordinate in an int16: anything outside wraps to a far-away region, whose local
    // coordinate is then out of range, i.e. the key is null (ohm/MapRegion.cpp:32-69).
    ok = ok && coord >= -32768 && coord <= 32767;
    const double centre = coord * mc.region_dim[a];
    const double region_min = centre - 0.5 * mc.region_dim[a];
    const double pl = p[a] - mc.origin[a] - region_min;
    const int q = pointToRegionVoxel(pl, mc.resolution, mc.region_dim[a]);
    ok = ok && 0 <= q && q < mc.kdim[a];
    // (regions cut into tiles: the tile coordinate coord * tile_split + j has to fit the 16-bit field of the packed
    // key too -- include/ohmhip.h, "LARGE REGIONS")
    tiles_ok = tiles_ok && coord * mc.tile_split[a] >= -32768 && coord * mc.tile_split[a] + (mc.tile_split[a] - 1) <= 32767;
    region[a] = coord;
    local[a] = q;
  }
  if (beyond_tiles)
  {
    *beyond_tiles = ok && !tiles_ok;
  }
  return ok && tiles_ok;
}

/// Key::isNull() is "all three region coordinates == int16 lowest" (ohm/Key.h:206): that one corner region reads as
/// null -- for the line walk -- even when the point is addressable.
__host__ __device__ inline bool keyIsNull(bool addressable, const int region[3])
{
  return !addressable || (region[0] == -32768 && region[1] == -32768 && region[2] == -32768);
}

/// ohm/OccupancyMap.h:757-778 (one axis).
__host__ __device__ inline double voxelCentreAxis(const MapConst &mc, int a, int region, int local)
{
  double v = double(float(region));
  v *= mc.region_dim[a];
  v -= 0.5 * mc.region_dim[a];
  v += mc.origin[a];
  v += double(local) * mc.resolution;
  v += 0.5 * mc.resolution;
  return v;
}

/// floor division / modulo for global voxel coordinate -> (region, local), or -> (tile, local) with the tile edge.
__device__ inline void splitGlobal(int g, int dim, int &region, int &local)
{
  if ((dim & (dim - 1)) == 0)
  {
    // power-of-two region edge (the default 32): arithmetic shift == floor division, mask == floor modulo
    region = g >> (__ffs(dim) - 1);
    local = g & (dim - 1);
    return;
  }
  int q = g / dim;
  int r = g - q * dim;
  if (r < 0)
  {
    r += dim;
    --q;
  }
  region = q;
  local = r;
}

/// Local voxel coordinate of a global voxel coordinate (floor modulo); a mask when the region edge is a power of two.
__device__ inline int localCoord(int g, int dim)
{
  if ((dim & (dim - 1)) == 0)
  {
    return g & (dim - 1);
  }
  int r = g % dim;
  return (r < 0) ? r + dim : r;
}

/// Voxel centre along one axis from the GLOBAL voxel coordinate, evaluated as the reference evaluates it: from the
/// caller's region coordinate and the voxel's coordinate inside that region (voxelCentreAxis) -- which is what a tile
/// coordinate has to be turned back into first.
__device__ inline double globalVoxelCentreAxis(const MapConst &mc, int a, int g)
{
  int region, local;
  splitGlobal(g, mc.kdim[a], region, local);
  return voxelCentreAxis(mc, a, region, local);
}

/// Time at which the j-th step (j >= 1) along an axis is taken: the value `time_next[axis]` holds after j-1 steps on
/// that axis (ohm/LineWalkCompute.h:299-301 and :375-378).
__device__ inline double stepTime(double init, double delta, int j)
{
  return (j <= 1) ? init : init + delta * double(j - 1);
}

/// Does the i-th step of axis b come before the j-th step of axis a in the walk?  The walk always takes the smallest
/// time_next, ties going to the HIGHER axis index (ohm/LineWalkCompute.h:282-289).
__device__ inline bool stepPrecedes(double tb, int b, double ta, int a)
{
  return tb < ta || (tb == ta && b > a);
}

/// time_next of one axis after k steps along it (ohm/LineWalkCompute.h:299-301, :375-378).
__device__ inline double timeNext(double init, double delta, int k, int total)
{
  return (k < total) ? ((k == 0) ? init : init + delta * double(k)) : dInf();
}

/// walkSelectNextAxis (ohm/LineWalkCompute.h:282-289): the axis with the smallest time_next, ties go to the higher axis.
__device__ inline int nextAxis(double t0, double t1, double t2)
{
  const bool c01 = t0 < t1;
  const double t01 = c01 ? t0 : t1;
  const bool c2 = t01 < t2;
  return c2 ? (c01 ? 0 : 1) : 2;
}

/// Select one of three per-axis values without indexing an array at run time (run-time indexed locals end up in
/// scratch memory on gfx950; every per-axis quantity in the kernels is therefore a named scalar).
template <typename T>
__device__ inline T sel3(int axis, T v0, T v1, T v2)
{
  return (axis == 0) ? v0 : ((axis == 1) ? v1 : v2);
}

template <typename T>
__device__ inline T sel3(int axis, const T v[3])
{
  return (axis == 0) ? v[0] : ((axis == 1) ? v[1] : v[2]);
}

/// Number of steps already taken along axis b at the moment the j-th step of axis a (time ta) is about to be taken.
/// T_b(i) is non-decreasing in i so the preceding steps form a prefix [1, n]; estimate n arithmetically and fix up
/// with the exact predicate so the result is identical to running the reference walk step by step.  The estimate only
/// has to be close: `rdelta` is a (rounded) reciprocal of delta computed once per ray, which keeps the fp64 division
/// out of the per-crossing work.
__device__ inline int stepsBefore(double init, double delta, double rdelta, int total, int b, int a, double ta)
{
  if (total == 0)
  {
    return 0;
  }
  int n;
  if (delta > 0 && delta < dInf())
  {
    const double x = (ta - init) * rdelta;
    // In real arithmetic T_b(i) <= ta  <=>  i - 1 <= x.  The fp64 values the exact predicate compares -- T_b(i) =
    // fl(init + fl(delta * (i - 1))) against ta -- differ from that by rounding of at most 2^-51 * (i + |init| / delta)
    // steps, and x itself carries three roundings (2^-51 * |x|): for |x| < 2^20 and |init| <= 4 delta both stay below
    // 1e-9 steps.  So when x keeps a distance of 1e-5 from every integer the predicate's outcome for every i is the real
    // one -- no tie, no doubt -- and the count follows without evaluating it (the loops below evaluate it at least twice
    // per call; the set-up kernels call this twice per ray-region segment).  Everything else takes the exact route.
    const double whole = floor(x);
    const double frac = x - whole;
    if (frac > 1e-5 && frac < 1.0 - 1e-5 && x > -1048576.0 && x < 1048576.0 && fabs(init) <= 4.0 * delta)
    {
      const int count = int(whole) + 1;
      return (x < 0) ? 0 : ((count > total) ? total : count);
    }
    // T_b(i) <= ta  <=>  i - 1 <= x
    n = (x < 0) ? 0 : ((x >= double(total)) ? total : int(x) + 1);
    n = (n > total) ? total : n;
    while (n < total && stepPrecedes(stepTime(init, delta, n + 1), b, ta, a))
    {
      ++n;
    }
    while (n > 0 && !stepPrecedes(stepTime(init, delta, n), b, ta, a))
    {
      --n;
    }
    return n;
  }
  // Degenerate deltas (zero-length rays): binary search on the monotone predicate.
  int lo = 0;
  int hi = total;
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (stepPrecedes(stepTime(init, delta, mid), b, ta, a))
    {
      lo = mid;
    }
    else
    {
      hi = mid - 1;
    }
  }
  return lo;
}

/// Ray filter: ohm/RayFilter.cpp:12-58 (goodRayFilter / clipRayFilter).  May move `end` (clip).  Returns false for
/// a rejected ray.
__device__ inline bool filterRay(const MapConst &mc, const double start[3], double end[3], bool &clipped_end,
                                 uint32_t ray)
{
  clipped_end = false;
  if (mc.batch_filter_flags)
  {
    // Filtered (and possibly moved) by the caller's RayFilterFunction: only the flag is consumed here -- kRffClippedEnd
    // makes the end voxel part of the ray and suppresses the sample (ohm/RayMapperOccupancy.cpp:209-223).
    // kRffInvalid: a ray the map's device filter chain rejected (k_ray_filter writes this array then) is not passed.
    const unsigned filter_flags = mc.batch_filter_flags[ray];
    clipped_end = (filter_flags & 4u) != 0;  // kRffClippedEnd, ohm/RayFilter.h:21-29
    return (filter_flags & 1u) == 0;
  }
  if (mc.filter_mode == OHMHIP_FILTER_NONE)
  {
    return true;
  }
  bool good = isfinite(start[0]) && isfinite(start[1]) && isfinite(start[2]) && isfinite(end[0]) && isfinite(end[1]) &&
              isfinite(end[2]);
  const double rx = end[0] - start[0];
  const double ry = end[1] - start[1];
  const double rz = end[2] - start[2];
  const double len2 = (rx * rx + ry * ry) + rz * rz;
  if (mc.filter_mode == OHMHIP_FILTER_GOOD)
  {
    good = good && (mc.filter_range <= 0 || len2 <= mc.filter_range * mc.filter_range);
  }
  else if (good && mc.filter_range > 0 && len2 > mc.filter_range * mc.filter_range)
  {
    const double len = sqrt(len2);
    end[0] = start[0] + (rx / len) * mc.filter_range;
    end[1] = start[1] + (ry / len) * mc.filter_range;
    end[2] = start[2] + (rz / len) * mc.filter_range;
    clipped_end = true;
  }
  return good;
}

/// Ray filter + key + line-walk set-up for one ray.  Mirrors, in order:
///   ohm/RayFilter.cpp:12-58 (goodRayFilter / clipRayFilter), ohm/LineWalk.h:112-129 (walkSegmentKeys),
///   ohm/LineWalkCompute.h:188-248 (walkInitRay) and :260-280 (walkCalculateSteps).
/// `start`/`end` may be modified by the clip filter.
__device__ inline void setupRay(const MapConst &mc, double start[3], double end[3], unsigned ray_flags, RayWalk &rw,
                                uint32_t ray)
{
  rw.flags = 0;
  rw.pad = 0;
  rw.length = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    rw.init[a] = rw.delta[a] = 0;
    rw.g0[a] = rw.total[a] = 0;
  }

  bool clipped_end = false;
  if (!filterRay(mc, start, end, clipped_end, ray))
  {
    return;
  }
  rw.flags = kRwPassed;

  int r0[3], l0[3], r1[3], l1[3];
  bool beyond0 = false, beyond1 = false;
  const bool addressable0 = voxelKey(mc, start, r0, l0, &beyond0);
  const bool addressable1 = voxelKey(mc, end, r1, l1, &beyond1);
  const bool ok0 = !keyIsNull(addressable0, r0);
  const bool ok1 = !keyIsNull(addressable1, r1);
  if (!ok0 || !ok1)
  {
    // walkSegmentKeys returns 0 for null keys (ohm/LineWalk.h:119-122): no voxel of the ray is visited.  The mappers
    // still apply the SAMPLE update afterwards with voxelKey(end) and no null check (ohm/RayMapperOccupancy.cpp:234-239,
    // ohm/RayMapperNdt.cpp:280-286): an addressable end point gets its hit although the start was not addressable, and an
    // unaddressable end point lands on Key::kNull -- region (-32768)^3, voxel 0 (an end point in that corner region IS
    // addressable and keeps its voxel; only the walk treats its key as null).  Mirrored here so the maps stay identical: a ray with no walk whose "start voxel" is the voxel the sample goes to.
    const bool include_end = clipped_end || (ray_flags & OHMHIP_RF_END_POINT_AS_FREE);
    // (a map whose regions are cut into tiles cannot address Key::kNull's region -- its tile coordinates leave the
    // packed key's range: there the sample of an unaddressable end point is dropped)
    const bool tiled = (mc.tile_split[1] | mc.tile_split[2]) > 1;
    if (!include_end && !(ray_flags & OHMHIP_RF_EXCLUDE_SAMPLE) && (addressable1 || !tiled))
    {
#pragma unroll
      for (int a = 0; a < 3; ++a)
      {
        rw.g0[a] = addressable1 ? (r1[a] * mc.kdim[a] + l1[a]) : (-32768 * mc.kdim[a]);
      }
      rw.flags = kRwPassed | kRwValid | kRwApplySample;
    }
    // (the caller can see that rays were cut for key-range reasons: ohmhip_map_rays_beyond_tiles)
    rw.flags |= (beyond0 || beyond1) ? unsigned(kRwBeyondTiles) : 0u;
    return;
  }

  // walkInitRay
  double dir[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    dir[a] = end[a] - start[a];
  }
  double length = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
  length = (length > 1e-6) ? sqrt(length) : 0;
  unsigned flags = kRwValid | kRwPassed;
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    const int sign = dir[a] < 0;
    flags |= sign ? (kRwSign0 << a) : 0u;
    dir[a] /= length;
    const double dir_inv = (length > 0) ? 1 / dir[a] : 0;
    const double centre = voxelCentreAxis(mc, a, r0[a], l0[a]);
    double vmin = centre - 0.5 * mc.resolution;
    double vmax = centre + 0.5 * mc.resolution;
    const double exit0 = ((sign ? vmin : vmax) - start[a]) * dir_inv;
    const double shift = double(-2 * sign + 1) * mc.resolution;
    vmin += shift;
    vmax += shift;
    double exit1 = ((sign ? vmin : vmax) - start[a]) * dir_inv;
    if (exit1 != dInf())
    {
      exit1 -= exit0;
    }
    rw.init[a] = exit0;
    rw.delta[a] = exit1;
    rw.g0[a] = r0[a] * mc.kdim[a] + l0[a];
    const int g1 = r1[a] * mc.kdim[a] + l1[a];
    const int diff = g1 - rw.g0[a];
    rw.total[a] = diff < 0 ? -diff : diff;
    // The step direction the reference uses comes from the sign of the ray direction, while the step COUNT comes
    // from the key difference.  They agree whenever there is at least one step to take.
  }

  rw.length = length;
  const bool include_end = clipped_end || (ray_flags & OHMHIP_RF_END_POINT_AS_FREE);
  flags |= include_end ? kRwIncludeEnd : 0u;
  flags |= (!include_end && !(ray_flags & OHMHIP_RF_EXCLUDE_SAMPLE)) ? kRwApplySample : 0u;
  flags |= (ray_flags & OHMHIP_RF_EXCLUDE_ORIGIN) ? kRwExcludeStart : 0u;
  flags |= !(ray_flags & OHMHIP_RF_EXCLUDE_RAY) ? kRwWalk : 0u;
  rw.flags = flags;
}

__device__ inline int rwSign(const RayWalk &rw, int a)
{
  return (rw.flags >> (1 + a)) & 1u;
}

__device__ inline int rwDir(const RayWalk &rw, int a)
{
  return 1 - 2 * rwSign(rw, a);
}

/// Local voxel coordinates of voxel index `vi` of a region.
__device__ inline void voxelLocal(const MapConst &mc, uint32_t vi, int &lx, int &ly, int &lz)
{
  const uint32_t dx = uint32_t(mc.dim[0]);
  const uint32_t dxy = dx * uint32_t(mc.dim[1]);
  lz = int(vi / dxy);
  const uint32_t r = vi - uint32_t(lz) * dxy;
  ly = int(r / dx);
  lx = int(r - uint32_t(ly) * dx);
}

/// Steps a ray has taken along each axis when it stands in voxel `vi` of region (rx, ry, rz): the walk moves
/// monotonically away from the start voxel on every axis.
__device__ inline void stepsAtVoxel(const MapConst &mc, const RayWalk &rw, int rx, int ry, int rz, uint32_t vi, int &k0,
                                    int &k1, int &k2)
{
  int lx, ly, lz;
  voxelLocal(mc, vi, lx, ly, lz);
  k0 = abs(rx * mc.dim[0] + lx - rw.g0[0]);
  k1 = abs(ry * mc.dim[1] + ly - rw.g0[1]);
  k2 = abs(rz * mc.dim[2] + lz - rw.g0[2]);
}

/// The exact decision of the reference walk for a ray standing in voxel `vi` of region (rx, ry, rz): the axis of the
/// next step.
__device__ inline int exactNextAxis(const MapConst &mc, const RayWalk &rw, int rx, int ry, int rz, uint32_t vi)
{
  int k0, k1, k2;
  stepsAtVoxel(mc, rw, rx, ry, rz, vi, k0, k1, k2);
  return nextAxis(timeNext(rw.init[0], rw.delta[0], k0, rw.total[0]), timeNext(rw.init[1], rw.delta[1], k1, rw.total[1]),
                  timeNext(rw.init[2], rw.delta[2], k2, rw.total[2]));
}

/// The reference's walk (ohm/LineWalkCompute.h:282-307), voxel by voxel, for the kernels that give a ray a lane of its
/// own.  Named scalars per axis: see sel3.
struct LaneWalk
{
  double init0, init1, init2, delta0, delta1, delta2;
  double t0, t1, t2;           ///< time_next
  double k0, k1, k2;           ///< steps taken (a whole number; kept as the double the step multiplies by)
  int rem0, rem1, rem2;        ///< steps left
  int g0, g1, g2;              ///< the current voxel, global coordinates
  int d0, d1, d2;              ///< step direction
};

/// The walk of `rw` after s0, s1, s2 steps along the axes (a valid prefix of the walk; zeros: its start voxel).
__device__ inline void laneStart(LaneWalk &w, const RayWalk &rw, int s0, int s1, int s2)
{
  w.init0 = rw.init[0], w.init1 = rw.init[1], w.init2 = rw.init[2];
  w.delta0 = rw.delta[0], w.delta1 = rw.delta[1], w.delta2 = rw.delta[2];
  w.rem0 = rw.total[0] - s0, w.rem1 = rw.total[1] - s1, w.rem2 = rw.total[2] - s2;
  w.d0 = rwDir(rw, 0), w.d1 = rwDir(rw, 1), w.d2 = rwDir(rw, 2);
  w.k0 = double(s0), w.k1 = double(s1), w.k2 = double(s2);
  w.g0 = rw.g0[0] + w.d0 * s0, w.g1 = rw.g0[1] + w.d1 * s1, w.g2 = rw.g0[2] + w.d2 * s2;
  w.t0 = timeNext(w.init0, w.delta0, s0, rw.total[0]);
  w.t1 = timeNext(w.init1, w.delta1, s1, rw.total[1]);
  w.t2 = timeNext(w.init2, w.delta2, s2, rw.total[2]);
}

/// The lane stands in the walk's last voxel.
__device__ inline bool laneFinished(const LaneWalk &w)
{
  return (w.rem0 | w.rem1 | w.rem2) == 0;
}

/// The time at which the walk leaves the current voxel: the time_next of the axis the next step takes (+inf in the
/// last voxel).
__device__ inline double laneExitTime(const LaneWalk &w)
{
  const double t01 = (w.t0 < w.t1) ? w.t0 : w.t1;  // (nextAxis' comparisons: the value it selects)
  return (t01 < w.t2) ? t01 : w.t2;
}

/// One step along one axis: timeNext() after k >= 1 steps, with k carried as a double (no conversion per step).
__device__ inline void laneStepAxis(int &g, int d, double &k, int &rem, double &t, double init, double delta)
{
  g += d;
  --rem;
  k += 1.0;
  t = rem ? init + delta * k : dInf();
}

/// One voxel on (not in the last voxel).
__device__ inline void laneStep(LaneWalk &w)
{
  const int axis = nextAxis(w.t0, w.t1, w.t2);
  if (axis == 2)
  {
    laneStepAxis(w.g2, w.d2, w.k2, w.rem2, w.t2, w.init2, w.delta2);
  }
  else if (axis == 0)
  {
    laneStepAxis(w.g0, w.d0, w.k0, w.rem0, w.t0, w.init0, w.delta0);
  }
  else
  {
    laneStepAxis(w.g1, w.d1, w.k1, w.rem1, w.t1, w.init1, w.delta1);
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_WALK_DEVICE_H
