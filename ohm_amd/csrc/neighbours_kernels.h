// neighbours_kernels.h -- point queries against the resident map, read only: ohm::NearestNeighbours (ohm/
// NearestNeighbours.cpp:35-181, 240-284) and voxels read by key (ohm::Voxel<T>).
//
//   k_nn_count         1 workgroup / chunk   the query's test per voxel; one count (and one closest voxel) per wave
//   (exclusive scan of the counts, 64 bit: rocPRIM, neighbours_impl.h)
//   k_nn_emit          1 workgroup / chunk   the same traversal; a passing voxel writes key and range at the offset of
//                                            its wave + its rank among the passing voxels before it in the wave
//   k_nn_query_counts  1 lane / query        results per query from the scan
//   k_nn_nearest       1 wave / query        kQfNearestResult: the closest of the query's waves' closest voxels
//   k_nn_nearest_emit  1 lane / query        ... written at the query's offset
//   k_read_voxels      1 lane / key          the voxel of one layer, and whether the map holds its region
//
// The rules are those of include/ohmhip.h ("POINT QUERIES"); tests/neighbours_ref.py is the same restatement on the CPU.
//
// Shape.  The cloud's (cloud_kernels.h): the host lists the work as (query, chunk) records ordered by query, then region
// (rz, ry, rx), then chunk -- the reference's visiting order (ohm/private/OccupancyQueryAlg.h:47-58, then z, y, x inside
// a region) --, a chunk being up to kCloudChunkVoxels consecutive voxels of a region's MapChunk block.  One workgroup of
// four waves per chunk; wave w owns the chunk's voxels [w * 1024, (w + 1) * 1024) and reads them in runs of 64, so the
// flat array of per-wave counts is in visiting order and its exclusive scan is every wave's first result slot.  Counting
// is __popcll(__ballot(pass)), ranking __popcll(ballot & lanes below).  No atomics: two calls return identical bytes.
// A chunk with a null block reads +inf throughout: a tile of a tiled region that holds no data, or -- listed only
// with kQfUnknownAsOccupied -- a region the map does not hold.
#ifndef OHMHIP_NEIGHBOURS_KERNELS_H
#define OHMHIP_NEIGHBOURS_KERNELS_H

#include "cloud_kernels.h"

namespace ohmhip
{
/// Consecutive voxels of one tile, for one query.
struct NnChunk
{
  const float *sel;   ///< occupancy of the chunk's FIRST voxel; null: every voxel reads +inf
  uint32_t first;     ///< index of the first voxel in the REGION's block: x + y * dx + z * dx * dy
  uint32_t count;     ///< voxels, <= kCloudChunkVoxels
  int16_t region[3];  ///< the caller's region key
  uint16_t pad;
  uint32_t query;
  uint32_t pad2;
};
static_assert(sizeof(NnChunk) == 32, "work list records are two 16-byte words");

constexpr unsigned long long kNnNone = ~0ull;  ///< no voxel passed (above every (r2 bits, index) pair: r2 >= +0)

/// The closest result of a query: wave `part` of the work list, voxel `voxel` of its chunk.
struct NnBest
{
  uint32_t part;
  uint32_t voxel;
  uint32_t r2_bits;
  uint32_t found;
};

struct NnArgs
{
  MapConst mc;  ///< key maths; origin zeroed (voxelCentreLocal)
  const NnChunk *chunks;
  const float *near_local;  ///< [queries][3] vec3(near_point - origin)
  float radius2;         ///< search_radius * search_radius, fp32
  int unknown_as_occupied;
  int nearest;           ///< kQfNearestResult
  uint32_t n_queries;
  const uint32_t *chunk_begin;          ///< [queries + 1] the chunks of query q: [chunk_begin[q], chunk_begin[q + 1])
  uint32_t *counts;                     ///< [chunks * kCloudWaves + 1: a zero, so that the scan ends in the total]
  unsigned long long *best;             ///< [chunks * kCloudWaves] nearest: (r2 bits << 32) | voxel of chunk, or kNnNone
  const unsigned long long *offsets;    ///< exclusive scan of counts
  unsigned long long *query_counts;     ///< [queries]
  uint32_t *query_found;                ///< [queries + 1] nearest: 0 or 1 (+ a zero, as for counts)
  const unsigned long long *query_offsets;  ///< nearest: exclusive scan of query_found
  NnBest *query_best;                   ///< [queries] nearest
  unsigned long long capacity;          ///< results the arrays hold
  GpuKeyOut *out_keys;                  ///< [capacity]
  float *out_ranges;                    ///< [capacity] or null
};

/// Voxel i of chunk c as a caller key.
__device__ inline GpuKeyOut nnKey(const MapConst &mc, const NnChunk &c, uint32_t i)
{
  const uint32_t index = c.first + i;
  const uint32_t dx = uint32_t(mc.kdim[0]), dy = uint32_t(mc.kdim[1]);
  const uint32_t row = index / dx;
  const uint32_t lz = row / dy;
  GpuKeyOut k;
  k.region[0] = c.region[0];
  k.region[1] = c.region[1];
  k.region[2] = c.region[2];
  k.voxel[0] = uint8_t(index - row * dx);
  k.voxel[1] = uint8_t(row - lz * dy);
  k.voxel[2] = uint8_t(lz);
  k.voxel[3] = 0;
  return k;
}

/// The query's test of voxel i of chunk c (ohm/NearestNeighbours.cpp:78-85, 103-111), fp32 as the reference evaluates it:
/// the voxel obstructs, and its centre lies within the radius of the near point.  r2: the squared range.
__device__ inline bool nnTest(const NnArgs &a, const NnChunk &c, uint32_t i, float qx, float qy, float qz, float &r2)
{
  const float inf = __int_as_float(0x7f800000);
  const float v = c.sel ? c.sel[i] : inf;
  // (a NaN is not +inf and not >= anything)
  const bool obstructs = (v == inf) ? (a.unknown_as_occupied != 0) : (v >= a.mc.threshold_value);
  if (!obstructs)
  {
    return false;
  }
  const GpuKeyOut k = nnKey(a.mc, c, i);
  // glm::vec3(voxelCentreLocal(key)) - query_origin, then glm::dot: (x * x + y * y) + z * z
  const float dx = float(voxelCentreAxis(a.mc, 0, k.region[0], k.voxel[0])) - qx;
  const float dy = float(voxelCentreAxis(a.mc, 1, k.region[1], k.voxel[1])) - qy;
  const float dz = float(voxelCentreAxis(a.mc, 2, k.region[2], k.voxel[2])) - qz;
  r2 = (dx * dx + dy * dy) + dz * dz;
  return r2 <= a.radius2;
}

/// The traversal both kernels share: wave `wave` of the workgroup over its share of chunk c.  EMIT: passing voxels are
/// written from slot `base` on.  Returns the wave's count; best: the wave's closest passing voxel, the earliest of
/// equals, as (r2 bits << 32) | voxel (valid in every lane).
template <bool EMIT>
__device__ inline uint32_t nnWalkWave(const NnArgs &a, const NnChunk &c, uint32_t wave, unsigned long long base,
                                      unsigned long long &best)
{
  const uint32_t lane = threadIdx.x & 63u;
  const float qx = a.near_local[3u * c.query], qy = a.near_local[3u * c.query + 1u],
              qz = a.near_local[3u * c.query + 2u];
  const uint32_t end = min((wave + 1u) * kCloudWaveVoxels, c.count);
  const unsigned long long below = cloudLanesBelow();
  uint32_t total = 0;
  best = kNnNone;
  for (uint32_t at = wave * kCloudWaveVoxels; at < end; at += 64u)
  {
    const uint32_t i = at + lane;
    float r2 = 0.0f;
    const bool pass = i < end && nnTest(a, c, i, qx, qy, qz, r2);
    const unsigned long long b = __ballot(pass);
    if (EMIT)
    {
      const unsigned long long slot = base + total + uint32_t(__popcll(b & below));
      if (pass && slot < a.capacity)
      {
        a.out_keys[slot] = nnKey(a.mc, c, i);
        if (a.out_ranges)
        {
          a.out_ranges[slot] = __builtin_sqrtf(r2);
        }
      }
    }
    else if (pass)
    {
      // (r2 >= +0: the bit pattern orders as the value; i ascends, so a lane keeps its first smallest)
      const unsigned long long mine = ((unsigned long long)__float_as_uint(r2) << 32) | i;
      best = (mine < best) ? mine : best;
    }
    total += uint32_t(__popcll(b));
  }
  if (!EMIT && a.nearest)
  {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
    {
      const unsigned long long other = shfl64(best, int(lane) ^ off);
      best = (other < best) ? other : best;
    }
  }
  return total;
}

__global__ void __launch_bounds__(256) k_nn_count(NnArgs a)
{
  const NnChunk c = a.chunks[blockIdx.x];
  const uint32_t wave = threadIdx.x >> 6;
  unsigned long long best;
  const uint32_t total = nnWalkWave<false>(a, c, wave, 0ull, best);
  if ((threadIdx.x & 63u) == 0u)
  {
    const size_t part = size_t(blockIdx.x) * kCloudWaves + wave;
    a.counts[part] = total;
    if (a.nearest)
    {
      a.best[part] = best;
    }
  }
}

__global__ void __launch_bounds__(256) k_nn_emit(NnArgs a)
{
  const uint32_t wave = threadIdx.x >> 6;
  const size_t part = size_t(blockIdx.x) * kCloudWaves + wave;
  const unsigned long long base = a.offsets[part];
  if (a.counts[part] == 0u || base >= a.capacity)
  {
    return;  // nothing passes in this wave's share, or everything it holds lies beyond the arrays
  }
  const NnChunk c = a.chunks[blockIdx.x];
  unsigned long long best;
  nnWalkWave<true>(a, c, wave, base, best);
}

/// Results per query: the scan's span over the query's chunks.
__global__ void __launch_bounds__(256) k_nn_query_counts(NnArgs a)
{
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < a.n_queries)
  {
    a.query_counts[q] = a.offsets[size_t(a.chunk_begin[q + 1u]) * kCloudWaves] - a.offsets[size_t(a.chunk_begin[q]) * kCloudWaves];
  }
}

/// kQfNearestResult: one wave per query over the closest voxels of the query's waves.  The first voxel in visiting
/// order whose r2 is strictly smaller than every earlier one (ClosestResult, ohm/private/QueryDetail.h:39-43) is the
/// smallest (r2, position); a wave's entry is already its earliest smallest, and parts ascend in visiting order.
__global__ void __launch_bounds__(64) k_nn_nearest(NnArgs a)
{
  const uint32_t q = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const uint32_t begin = a.chunk_begin[q] * kCloudWaves, end = a.chunk_begin[q + 1u] * kCloudWaves;
  unsigned long long best = kNnNone;
  for (uint32_t part = begin + lane; part < end; part += 64u)
  {
    const unsigned long long b = a.best[part];
    if (b != kNnNone)
    {
      const unsigned long long mine = (b & 0xffffffff00000000ull) | part;
      best = (mine < best) ? mine : best;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
  {
    const unsigned long long other = shfl64(best, int(lane) ^ off);
    best = (other < best) ? other : best;
  }
  if (lane == 0u)
  {
    NnBest r = { 0u, 0u, 0u, 0u };
    if (best != kNnNone)
    {
      r.part = uint32_t(best);
      r.voxel = uint32_t(a.best[r.part]);
      r.r2_bits = uint32_t(best >> 32);
      r.found = 1u;
    }
    a.query_best[q] = r;
    a.query_counts[q] = r.found;
    a.query_found[q] = r.found;
  }
}

__global__ void __launch_bounds__(256) k_nn_nearest_emit(NnArgs a)
{
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= a.n_queries)
  {
    return;
  }
  const NnBest r = a.query_best[q];
  const unsigned long long slot = a.query_offsets[q];
  if (!r.found || slot >= a.capacity)
  {
    return;
  }
  const NnChunk c = a.chunks[r.part / kCloudWaves];
  a.out_keys[slot] = nnKey(a.mc, c, r.voxel);
  if (a.out_ranges)
  {
    a.out_ranges[slot] = __builtin_sqrtf(__uint_as_float(r.r2_bits));
  }
}

/// ohmhip_map_read_voxels.  The view's `occupancy` and the spill table's blocks are those of the REQUESTED layer
/// (mapReadView(m, view, layer)), in dwords: every layer's voxel is a whole number of them.
struct ReadVoxelsArgs : MapReadView
{
  const GpuKeyOut *keys;
  uint32_t n;
  uint32_t voxel_dwords;  ///< dwords per voxel of the layer
  uint32_t clear_word;    ///< what a voxel the map does not hold reads (layerClearWord)
  uint32_t *values;       ///< [n][voxel_dwords]
  uint8_t *present;       ///< [n]
};

/// One lane per key.  The tile's block is resolved as mapFindTile resolves it -- region hash, then the host store --;
/// lanes of a wave that ask for the same tile share one probe (waveMatch on a 32-bit mix of the tile key; a lane whose
/// key only collides with its leader's probes for itself).
__global__ void __launch_bounds__(256) k_read_voxels(ReadVoxelsArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned lane = laneId();
  const MapConst &mc = a.mc;
  GpuKeyOut k = queryNullKey();
  if (i < a.n)
  {
    k = a.keys[i];
  }
  // Key::isNull (ohm/Key.h:206); such a key names no voxel, and neither does one beyond the region's dimensions (the
  // host entry point refuses those; device arrays are not inspected)
  const bool valid = i < a.n && !(k.region[0] == -32768 && k.region[1] == -32768 && k.region[2] == -32768) &&
                     int(k.voxel[0]) < mc.kdim[0] && int(k.voxel[1]) < mc.kdim[1] && int(k.voxel[2]) < mc.kdim[2];
  const int jy = int(k.voxel[1]) / mc.dim[1], jz = int(k.voxel[2]) / mc.dim[2];
  const int tx = int(k.region[0]);
  const int ty = int(k.region[1]) * mc.tile_split[1] + jy;
  const int tz = int(k.region[2]) * mc.tile_split[2] + jz;
  const uint32_t mix = uint32_t(tx) ^ (uint32_t(ty) * 0x9e3779b1u) ^ (uint32_t(tz) * 0x85ebca6bu);
  int leader;
  unsigned long long group;
  waveMatch(valid, mix, lane, leader, group);
  const int src = (leader < 0) ? int(lane) : leader;
  const bool same = __shfl(tx, src) == tx && __shfl(ty, src) == ty && __shfl(tz, src) == tz;
  const bool probes = valid && (leader == int(lane) || !same);
  FoundTile t = { kSlotUnassigned, nullptr };
  if (probes)
  {
    t = mapFindTile(a, tx, ty, tz);
  }
  const uint32_t leader_slot = __shfl(t.slot, src);
  const uint64_t leader_stored = shfl64(uint64_t(reinterpret_cast<uintptr_t>(t.stored)), src);
  if (valid && !probes)
  {
    t.slot = leader_slot;
    t.stored = reinterpret_cast<const float *>(uintptr_t(leader_stored));
  }
  if (i >= a.n)
  {
    return;
  }
  const uint32_t *block = nullptr;
  if (t.slot != kSlotUnassigned)
  {
    block = reinterpret_cast<const uint32_t *>(a.occupancy) + size_t(t.slot) * size_t(mc.region_voxels) * a.voxel_dwords;
  }
  else if (t.stored)
  {
    block = reinterpret_cast<const uint32_t *>(t.stored);
  }
  bool present = block != nullptr;
  if (!present && valid && (mc.tile_split[1] > 1 || mc.tile_split[2] > 1))
  {
    // a tile of a tiled region that holds no data: the region is present when any of its tiles is
    for (int z = 0; z < mc.tile_split[2] && !present; ++z)
    {
      for (int y = 0; y < mc.tile_split[1] && !present; ++y)
      {
        const FoundTile o = mapFindTile(a, tx, int(k.region[1]) * mc.tile_split[1] + y, int(k.region[2]) * mc.tile_split[2] + z);
        present = o.slot != kSlotUnassigned || o.stored != nullptr;
      }
    }
  }
  const int ly = int(k.voxel[1]) - jy * mc.dim[1], lz = int(k.voxel[2]) - jz * mc.dim[2];
  const size_t voxel = size_t(k.voxel[0]) + size_t(ly) * size_t(mc.dim[0]) + size_t(lz) * size_t(mc.dim[0]) * size_t(mc.dim[1]);
  uint32_t *out = a.values + size_t(i) * a.voxel_dwords;
  for (uint32_t w = 0; w < a.voxel_dwords; ++w)
  {
    out[w] = block ? block[voxel * a.voxel_dwords + w] : a.clear_word;
  }
  a.present[i] = present ? 1 : 0;
}
}  // namespace ohmhip

#endif  // OHMHIP_NEIGHBOURS_KERNELS_H
