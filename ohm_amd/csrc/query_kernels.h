// query_kernels.h -- RaysQueryGpu: read-only ray casts against the device-resident occupancy layer.
//
//   k_rays_query        1 lane / ray     the CPU query's walk (ohm/RaysQuery.cpp:102-203 onExecute) over the pool
//   k_rays_query_carry  1 lane / ray     the terminal type / key of rays that visit no voxel (see below)
//
// The reference's GPU kernel (raysQuery, ohmgpu/gpu/RaysQuery.cl:193) walks in fp32 and classifies with `>=`; this one
// follows the CPU query: fp64 walk with the enter / exit ranges of walkSegmentKeys (ohm/LineWalk.h:112-129, flags 0:
// start and end voxel visited; exit = the selected axis' time_next, the last voxel exits at the walk's length,
// ohm/LineWalkCompute.h:386-405), `v > threshold` for occupied, and the per-visit arithmetic of the CPU's visit lambda
// in its order (no FMA: the library builds with -ffp-contract=off).  The result is bit-identical to the CPU query.
//
// Voxels are resolved through the device region hash (regionFind on the TILE key): the hash is probed only when the
// walk crosses a tile boundary, the tile's block address stays in registers, and the occupancy word is a plain load --
// the query is ordered on the map's stream behind every queued batch, so nothing writes the pool while it runs.
// Regions in the host store (spill to host) are found in a small table of their pinned records; a key in neither is
// an unknown region (+inf, like MapChunk-less voxels on the CPU).
#ifndef OHMHIP_QUERY_KERNELS_H
#define OHMHIP_QUERY_KERNELS_H

#include "occupancy_kernels.h"
#include "replay_kernels.h"

namespace ohmhip
{
/// ohm::OccupancyType (ohm/OccupancyType.h:14-24).
enum : int8_t
{
  kOtNull = -2,
  kOtUnobserved = -1,
  kOtFree = 0,
  kOtOccupied = 1,
  kOtCarry = 127  ///< k_rays_query -> k_rays_query_carry: passed the filter, visited no voxel
};

/// Regions of the host store: packed tile key -> the occupancy block inside the region's pinned store record (device
/// visible host memory).  keys == null: nothing is stored.
struct QuerySpillTable
{
  const unsigned long long *keys;  ///< [mask + 1] packed key or 0
  const float *const *blocks;      ///< [mask + 1]
  uint32_t mask;
};

struct RaysQueryArgs
{
  MapConst mc;
  RegionTable rt;
  QuerySpillTable spill;
  const float *occupancy;  ///< pool layer: [slot][tile voxel]
  const double *rays;      ///< [n_rays][6] origin, end point
  uint32_t n_rays;
  double coef;             ///< RaysQuery::volumeCoefficient()
  double *ranges;
  double *volumes;
  int8_t *types;
  GpuKeyOut *keys;         ///< null: not requested
  int32_t *walked;         ///< [n_rays] the ray's index when it visited a voxel, -1 otherwise (max-scanned afterwards)
  uint32_t *ray_cursor;    ///< refill variant: rays handed out beyond the first grid (zero at launch)
};

/// Idle lanes of a wave that make the refill variant fetch new rays (one atomic per wave).
constexpr int kQueryRefillIdle = 16;

__device__ inline GpuKeyOut queryNullKey()
{
  GpuKeyOut k;  // Key::kNull (ohm/Key.cpp:14): region lowest() x 3, voxel 0
  k.region[0] = k.region[1] = k.region[2] = int16_t(-32768);
  k.voxel[0] = k.voxel[1] = k.voxel[2] = k.voxel[3] = 0;
  return k;
}

/// The occupancy block of tile (tx, ty, tz): resident slot, then the host store; null when the map has no such tile.
/// Args: any argument block with mc, rt, spill and occupancy (RaysQueryArgs, ClearanceArgs).
template <typename Args>
__device__ inline const float *queryTileBlock(const Args &a, int tx, int ty, int tz)
{
  // (a region the reference addresses whose tile coordinates leave the packed key's 16-bit fields cannot be in the
  // map: the key must not wrap onto another tile)
  if (tx < -32768 || tx > 32767 || ty < -32768 || ty > 32767 || tz < -32768 || tz > 32767)
  {
    return nullptr;
  }
  const uint64_t key = packRegionKey(tx, ty, tz);
  const uint32_t h = regionFind(a.rt, key);
  if (h != 0xffffffffu)
  {
    const uint32_t slot = a.rt.vals[h];
    if (slot < a.rt.slot_capacity)
    {
      return a.occupancy + size_t(slot) * size_t(a.mc.region_voxels);
    }
  }
  if (a.spill.keys)
  {
    uint32_t idx = hashRegionKey(key, a.spill.mask);
    for (uint32_t probe = 0; probe <= a.spill.mask; ++probe)
    {
      const unsigned long long k = a.spill.keys[idx];
      if (k == key)
      {
        return a.spill.blocks[idx];
      }
      if (k == 0)
      {
        break;
      }
      idx = (idx + 1) & a.spill.mask;
    }
  }
  return nullptr;
}

/// One lane's query state: the CPU walk of one ray (k_line_keys' stepping) and the visit lambda's accumulators.
struct QueryLane
{
  double init0, init1, init2, delta0, delta1, delta2;
  double t0, t1, t2, k0, k1, k2;
  double length, enter, volume;
  int g0, g1, g2, rem0, rem1, rem2, d0, d1, d2;
  int tx, ty, tz;  ///< tile of `block`
  const float *block;
  float range;
  int8_t type;
  uint32_t ray;
};

__device__ inline void queryWrite(const RaysQueryArgs &a, uint32_t ray, float range, double volume, int8_t type,
                                  const GpuKeyOut &key, bool walked)
{
  a.ranges[ray] = double(range);
  a.volumes[ray] = volume;
  a.types[ray] = type;
  if (a.keys)
  {
    a.keys[ray] = key;
  }
  a.walked[ray] = walked ? int32_t(ray) : -1;
}

/// Filter + walk set-up of ray `ray` (ohm/RaysQuery.cpp:174-188).  Returns true when the ray visits voxels; a ray that
/// does not is finished here: filtered (range 0, volume 0, kNull, Key::kNull), or passed with a null start / end key
/// (range 0, volume 0, type and key carried -- kOtCarry).
__device__ inline bool queryStart(const RaysQueryArgs &a, uint32_t ray, QueryLane &q)
{
  double start[3], end[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
  {
    start[c] = a.rays[size_t(ray) * 6 + c];
    end[c] = a.rays[size_t(ray) * 6 + 3 + c];
  }
  // The map's own filter (map->rayFilter(), ohm/RaysQuery.cpp:118), then walkSegmentKeys: the reference's key maths
  // with no tile range (the keys are the caller's), start and end voxel visited.
  MapConst kc = a.mc;
  kc.batch_filter_flags = nullptr;
  kc.tile_split[0] = kc.tile_split[1] = kc.tile_split[2] = 1;
  RayWalk rw;
  setupRay(kc, start, end, OHMHIP_RF_END_POINT_AS_FREE, rw, ray);
  if (!(rw.flags & kRwValid))
  {
    const bool passed = (rw.flags & kRwPassed) != 0;
    queryWrite(a, ray, 0.0f, 0.0, passed ? int8_t(kOtCarry) : int8_t(kOtNull), queryNullKey(), false);
    return false;
  }
  q.ray = ray;
  q.init0 = rw.init[0];
  q.init1 = rw.init[1];
  q.init2 = rw.init[2];
  q.delta0 = rw.delta[0];
  q.delta1 = rw.delta[1];
  q.delta2 = rw.delta[2];
  q.length = rw.length;
  q.d0 = rwDir(rw, 0);
  q.d1 = rwDir(rw, 1);
  q.d2 = rwDir(rw, 2);
  q.g0 = rw.g0[0];
  q.g1 = rw.g0[1];
  q.g2 = rw.g0[2];
  q.rem0 = rw.total[0];
  q.rem1 = rw.total[1];
  q.rem2 = rw.total[2];
  const double inf = dInf();
  q.k0 = q.k1 = q.k2 = 0;
  q.t0 = q.rem0 ? q.init0 : inf;
  q.t1 = q.rem1 ? q.init1 : inf;
  q.t2 = q.rem2 ? q.init2 : inf;
  q.enter = 0;
  q.volume = 0;
  q.range = 0.0f;
  q.type = kOtNull;
  q.block = nullptr;
  q.tx = q.ty = q.tz = 0x7fffffff;  // (no tile coordinate: the first visit resolves)
  return true;
}

/// Visit the lane's current voxel and step on.  Returns false when the ray is finished (its results written).
__device__ inline bool queryStep(const RaysQueryArgs &a, QueryLane &q)
{
  const MapConst &mc = a.mc;
  const bool last = (q.rem0 | q.rem1 | q.rem2) == 0;
  // exit range: time_next of the axis walkSelectNextAxis picks (ohm/LineWalkCompute.h:282-289), the walk's length at
  // the end voxel
  const bool c01 = q.t0 < q.t1;
  const double t01 = c01 ? q.t0 : q.t1;
  const bool c2 = t01 < q.t2;
  const double exit = last ? q.length : (c2 ? t01 : q.t2);

  int tx, lx, ty, ly, tz, lz;
  splitGlobal(q.g0, mc.dim[0], tx, lx);
  splitGlobal(q.g1, mc.dim[1], ty, ly);
  splitGlobal(q.g2, mc.dim[2], tz, lz);
  if (tx != q.tx || ty != q.ty || tz != q.tz)
  {
    q.block = queryTileBlock(a, tx, ty, tz);
    q.tx = tx;
    q.ty = ty;
    q.tz = tz;
  }
  const float unobserved_value = __int_as_float(0x7f800000);
  const float v = q.block ? q.block[lx + ly * mc.dim[0] + lz * mc.dim[0] * mc.dim[1]] : unobserved_value;

  // ohm/RaysQuery.cpp:144-156, in its order
  const bool is_unobserved = v == unobserved_value;
  const bool is_occupied = !is_unobserved && v > mc.threshold_value;
  q.volume += is_unobserved ? (a.coef * (exit * exit * exit - q.enter * q.enter * q.enter)) : 0.0;
  q.range = (!is_occupied) ? float(exit) : q.range;
  q.type = is_unobserved ? int8_t(kOtUnobserved) : (is_occupied ? int8_t(kOtOccupied) : int8_t(kOtFree));

  if (is_occupied || last)
  {
    int r0, r1, r2, l0, l1, l2;  // the caller's region key
    splitGlobal(q.g0, mc.kdim[0], r0, l0);
    splitGlobal(q.g1, mc.kdim[1], r1, l1);
    splitGlobal(q.g2, mc.kdim[2], r2, l2);
    GpuKeyOut key;
    key.region[0] = int16_t(r0);
    key.region[1] = int16_t(r1);
    key.region[2] = int16_t(r2);
    key.voxel[0] = uint8_t(l0);
    key.voxel[1] = uint8_t(l1);
    key.voxel[2] = uint8_t(l2);
    key.voxel[3] = 0;
    queryWrite(a, q.ray, q.range, q.volume, q.type, key, true);
    return false;
  }
  q.enter = exit;
  // ohm/LineWalkCompute.h:291-307 as k_line_keys steps it
  const double inf = dInf();
  if (!c2)
  {
    q.g2 += q.d2;
    --q.rem2;
    q.k2 += 1.0;
    q.t2 = q.rem2 ? q.init2 + q.delta2 * q.k2 : inf;
  }
  else if (c01)
  {
    q.g0 += q.d0;
    --q.rem0;
    q.k0 += 1.0;
    q.t0 = q.rem0 ? q.init0 + q.delta0 * q.k0 : inf;
  }
  else
  {
    q.g1 += q.d1;
    --q.rem1;
    q.k1 += 1.0;
    q.t1 = q.rem1 ? q.init1 + q.delta1 * q.k1 : inf;
  }
  return true;
}

/// kRefill = false: one lane per ray, the lane is done when its ray is (a wave waits for its longest ray).
/// kRefill = true: lanes that finished pick the next ray from a device-wide cursor (one atomic per wave for all of its
/// idle lanes, once kQueryRefillIdle of them are idle), the walk kernel's lane refill.
template <bool kRefill>
__global__ void __launch_bounds__(256) k_rays_query(RaysQueryArgs a)
{
  const uint32_t grid_lanes = gridDim.x * blockDim.x;
  uint32_t ray = blockIdx.x * blockDim.x + threadIdx.x;
  QueryLane q;
  if (!kRefill)
  {
    if (ray >= a.n_rays || !queryStart(a, ray, q))
    {
      return;
    }
    while (queryStep(a, q))
    {
    }
    return;
  }
  bool want = ray < a.n_rays;  // the lane holds a ray that is not set up yet
  bool active = false;
  bool exhausted = grid_lanes >= a.n_rays;
  const uint32_t lane = threadIdx.x & 63u;
  while (true)
  {
    if (want)
    {
      want = false;
      active = queryStart(a, ray, q);
    }
    const unsigned long long am = __ballot(active);
    const int n_idle = 64 - __popcll(am);
    if (n_idle >= kQueryRefillIdle)
    {
      if (exhausted)
      {
        if (am == 0)
        {
          break;
        }
      }
      else
      {
        uint32_t base = 0;
        if (lane == 0)
        {
          base = atomicAdd(a.ray_cursor, uint32_t(n_idle));
        }
        base = grid_lanes + __builtin_amdgcn_readfirstlane(base);
        exhausted = base + uint32_t(n_idle) >= a.n_rays;
        const unsigned long long idle = ~am;
        const uint32_t mine =
          base + __builtin_amdgcn_mbcnt_hi(uint32_t(idle >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(idle), 0u));
        if (!active && mine < a.n_rays)
        {
          ray = mine;
          want = true;
        }
        continue;
      }
    }
    if (active)
    {
      active = queryStep(a, q);
    }
  }
}

/// ohm/RaysQuery.cpp:116-117 declare the terminal type and key OUTSIDE the ray loop and reset only range and volume per
/// ray: a ray that passes the filter but visits no voxel (a null start or end key) reports the type and key of the last
/// preceding ray that visited one (kNull / Key::kNull before any).  `last_walked[i]` is the max-scan of `walked`.
__global__ void __launch_bounds__(256)
  k_rays_query_carry(int8_t *__restrict__ types, GpuKeyOut *__restrict__ keys, const int32_t *__restrict__ last_walked,
                     uint32_t n_rays)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rays || types[i] != int8_t(kOtCarry))
  {
    return;
  }
  const int32_t j = last_walked[i];  // < i: ray i itself did not visit a voxel
  types[i] = (j >= 0) ? types[j] : int8_t(kOtNull);
  if (keys)
  {
    keys[i] = (j >= 0) ? keys[j] : queryNullKey();
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_QUERY_KERNELS_H
