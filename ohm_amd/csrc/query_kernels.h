// query_kernels.h -- the read side of the device-resident map: what every reader shares (MapReadView, mapFindTile,
// LayerView for a second layer of a found tile, the caller's GpuKeyOut), LineKeysQueryGpu and RaysQueryGpu, read-only ray
// casts against the occupancy layer.
//
//   k_line_keys         1 lane / line    the keys of every voxel on a line, in walk order
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

#include "region_table.h"
#include "walk_device.h"

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

/// What a read-only kernel needs to find a voxel of the map: filled by mapReadView() on the host.
struct MapReadView
{
  MapConst mc;
  RegionTable rt;
  QuerySpillTable spill;
  const float *occupancy;  ///< pool layer: [slot][tile voxel]
};

/// Where mapFindTile found a tile: resident in pool slot `slot` (!= kSlotUnassigned), else in the host store with its
/// occupancy block at `stored`, else (null) the map has no such tile.
struct FoundTile
{
  uint32_t slot;
  const float *stored;
};

/// Tile (tx, ty, tz) of the map: the device region hash, then the host store.
__device__ inline FoundTile mapFindTile(const MapReadView &v, int tx, int ty, int tz)
{
  FoundTile t = { kSlotUnassigned, nullptr };
  // (a region the reference addresses whose tile coordinates leave the packed key's 16-bit fields cannot be in the
  // map: the key must not wrap onto another tile)
  if (tx < -32768 || tx > 32767 || ty < -32768 || ty > 32767 || tz < -32768 || tz > 32767)
  {
    return t;
  }
  const uint64_t key = packRegionKey(tx, ty, tz);
  const uint32_t h = regionFind(v.rt, key);
  if (h != 0xffffffffu)
  {
    const uint32_t slot = v.rt.vals[h];
    if (slot < v.rt.slot_capacity)
    {
      t.slot = slot;
      return t;
    }
  }
  if (v.spill.keys)
  {
    uint32_t idx = hashRegionKey(key, v.spill.mask);
    for (uint32_t probe = 0; probe <= v.spill.mask; ++probe)
    {
      const unsigned long long k = v.spill.keys[idx];
      if (k == key)
      {
        t.stored = v.spill.blocks[idx];
        return t;
      }
      if (k == 0)
      {
        break;
      }
      idx = (idx + 1) & v.spill.mask;
    }
  }
  return t;
}

/// A second layer of the map for a kernel that finds tiles itself (the occupancy layer is MapReadView's): filled by
/// layerView() on the host.
struct LayerView
{
  const char *pool;        ///< pool layer: [slot][tile voxel]; null: the map lacks the layer, or the kernel does not read it
  long long stored_delta;  ///< bytes from a store record's occupancy block to this layer's block
};

/// Tile `t`'s block of layer `l`, `tile_elements` elements of T; null when the map has no such tile or the view no layer.
template <typename T>
__device__ inline const T *foundTileLayer(const FoundTile &t, const LayerView &l, size_t tile_elements)
{
  if (!l.pool)
  {
    return nullptr;
  }
  if (t.slot != kSlotUnassigned)
  {
    return reinterpret_cast<const T *>(l.pool) + size_t(t.slot) * tile_elements;
  }
  return t.stored ? reinterpret_cast<const T *>(reinterpret_cast<const char *>(t.stored) + l.stored_delta) : nullptr;
}

/// The occupancy block of tile (tx, ty, tz); null when the map has no such tile.
__device__ inline const float *queryTileBlock(const MapReadView &v, int tx, int ty, int tz)
{
  const FoundTile t = mapFindTile(v, tx, ty, tz);
  return (t.slot != kSlotUnassigned) ? v.occupancy + size_t(t.slot) * size_t(v.mc.region_voxels) : t.stored;
}

/// GpuKey layout of the reference (ohmgpu/GpuKey.h:37-46): short region[3]; uchar voxel[4].
struct GpuKeyOut
{
  int16_t region[3];
  uint8_t voxel[4];
};
// The reference's record, from its own header compiled in place (tests/golden/ref_vectors.npz: gpukey_layout).
static_assert(sizeof(GpuKeyOut) == 10 && alignof(GpuKeyOut) == 2 && offsetof(GpuKeyOut, region) == 0 &&
                offsetof(GpuKeyOut, voxel) == 6,
              "GpuKeyOut must keep the layout of ohm::GpuKey (ohmgpu/GpuKey.h:37-46)");

/// The caller's key of global voxel (g0, g1, g2): split on the region edge, not the tile edge.
__device__ inline GpuKeyOut callerKey(const MapConst &mc, int g0, int g1, int g2)
{
  int r0, r1, r2, l0, l1, l2;
  splitGlobal(g0, mc.kdim[0], r0, l0);
  splitGlobal(g1, mc.kdim[1], r1, l1);
  splitGlobal(g2, mc.kdim[2], r2, l2);
  GpuKeyOut k;
  k.region[0] = int16_t(r0);
  k.region[1] = int16_t(r1);
  k.region[2] = int16_t(r2);
  k.voxel[0] = uint8_t(l0);
  k.voxel[1] = uint8_t(l1);
  k.voxel[2] = uint8_t(l2);
  k.voxel[3] = 0;
  return k;
}

__device__ inline GpuKeyOut queryNullKey()
{
  GpuKeyOut k;  // Key::kNull (ohm/Key.cpp:14): region lowest() x 3, voxel 0
  k.region[0] = k.region[1] = k.region[2] = int16_t(-32768);
  k.voxel[0] = k.voxel[1] = k.voxel[2] = k.voxel[3] = 0;
  return k;
}

/// LineKeysQueryGpu / `calculateLines` (ohmgpu/gpu/LineKeys.cl:66-100) with the CPU walk's semantics
/// (ohm/LineWalk.h:112-129 walkSegmentKeys, flags 0: start and end voxel included): one lane per query line writes the
/// keys of every voxel on the line, in walk order.  counts[i] is the full number of voxels even when it exceeds
/// max_keys_per_line (only the first max_keys_per_line keys are stored).
__global__ void __launch_bounds__(256)
  k_line_keys(MapConst mc, const double *__restrict__ lines, uint32_t n_lines, uint32_t max_keys_per_line,
              GpuKeyOut *__restrict__ keys_out, uint32_t *__restrict__ counts)
{
  const uint32_t line = blockIdx.x * blockDim.x + threadIdx.x;
  if (line >= n_lines)
  {
    return;
  }
  double start[3], end[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    start[a] = lines[size_t(line) * 6 + a];
    end[a] = lines[size_t(line) * 6 + 3 + a];
  }
  MapConst nofilter = mc;
  nofilter.filter_mode = OHMHIP_FILTER_NONE;
  nofilter.batch_filter_flags = nullptr;
  RayWalk rw;
  setupRay(nofilter, start, end, OHMHIP_RF_END_POINT_AS_FREE, rw, line);
  if (!(rw.flags & kRwValid))
  {
    counts[line] = 0;
    return;
  }
  LaneWalk w;
  laneStart(w, rw, 0, 0, 0);
  uint32_t n = 0;
  GpuKeyOut *out = keys_out + size_t(line) * max_keys_per_line;
  while (true)
  {
    if (n < max_keys_per_line)
    {
      out[n] = callerKey(mc, w.g0, w.g1, w.g2);
    }
    ++n;
    if (laneFinished(w))
    {
      break;
    }
    laneStep(w);
  }
  counts[line] = n;
}

struct RaysQueryArgs : MapReadView
{
  const double *rays;      ///< [n_rays][6] origin, end point
  uint32_t n_rays;
  double coef;             ///< RaysQuery::volumeCoefficient()
  double *ranges;
  double *volumes;
  int8_t *types;
  GpuKeyOut *keys;         ///< null: not requested
  int32_t *walked;         ///< [n_rays] the ray's index when it visited a voxel, -1 otherwise (max-scanned afterwards)
};

/// One lane's query state: the CPU walk of one ray and the visit lambda's accumulators.
struct QueryLane
{
  LaneWalk w;
  double length, enter, volume;
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
  laneStart(q.w, rw, 0, 0, 0);
  q.length = rw.length;
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
  const bool last = laneFinished(q.w);
  // exit range: time_next of the axis walkSelectNextAxis picks (ohm/LineWalkCompute.h:282-289), the walk's length at
  // the end voxel
  const double exit = last ? q.length : laneExitTime(q.w);

  int tx, lx, ty, ly, tz, lz;
  splitGlobal(q.w.g0, mc.dim[0], tx, lx);
  splitGlobal(q.w.g1, mc.dim[1], ty, ly);
  splitGlobal(q.w.g2, mc.dim[2], tz, lz);
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
    queryWrite(a, q.ray, q.range, q.volume, q.type, callerKey(mc, q.w.g0, q.w.g1, q.w.g2), true);
    return false;
  }
  q.enter = exit;
  laneStep(q.w);
  return true;
}

/// One lane per ray; the lane is done when its ray is (a wave waits for its longest ray).
__global__ void __launch_bounds__(256) k_rays_query(RaysQueryArgs a)
{
  const uint32_t ray = blockIdx.x * blockDim.x + threadIdx.x;
  QueryLane q;
  if (ray >= a.n_rays || !queryStart(a, ray, q))
  {
    return;
  }
  while (queryStep(a, q))
  {
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
