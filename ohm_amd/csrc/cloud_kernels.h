// cloud_kernels.h -- point clouds out of the resident map (ohmtools::saveCloud, saveDensityCloud, saveTsdfCloud,
// saveClearanceCloud: ohmtools/OhmCloud.cpp), read only: a stream compaction over the region blocks in a fixed order.
//
//   k_cloud_count  1 workgroup / chunk   the mode's test per voxel; one count per wave and chunk
//   (exclusive scan of the counts, 64 bit: rocPRIM, cloud_impl.h)
//   k_cloud_emit   1 workgroup / chunk   the same traversal; a passing voxel writes position, key and value at
//                                        offset of its wave + rank among the passing voxels before it in the wave
//
// The rules are those of include/ohmhip.h ("POINT CLOUDS"); tests/cloud_ref.py is the same restatement on the CPU.
//
// Shape.  The host lists the work (cloud_impl.h): the tiles of the selected regions in (rz, ry, rx) order, each cut
// into chunks of kCloudChunkVoxels consecutive voxels of the region's MapChunk block, with the addresses of the layer
// blocks the mode reads -- pool slot or pinned store record -- resolved once per tile.  A chunk is one workgroup of four
// waves; wave w owns the chunk's voxels [w * 1024, (w + 1) * 1024), so the flat array of per-wave counts is in voxel
// order and its exclusive scan is every wave's first output slot.  A wave reads its voxels in runs of 64 (one dword a
// lane, 256 contiguous bytes a wave) or, where the selecting layer is a float layer whose chunk starts on a 16-byte
// boundary, in groups of 256 (one float4 a lane); blocks of other alignments (a region of 105 voxels in pool slot 1)
// take the 64-voxel runs throughout.  Counting is __popcll(__ballot(pass)), ranking __popcll(ballot & lanes below);
// in a 256-voxel group lane l holds voxels 4l .. 4l + 3, so its rank adds the four ballots' bits below it and its own
// earlier components.  No atomics: the order -- and with it every byte of the result -- is the same on every call.
// The emit pass skips waves whose count is 0 and loads the mean word only for voxels that pass.
#ifndef OHMHIP_CLOUD_KERNELS_H
#define OHMHIP_CLOUD_KERNELS_H

#include "ndt_tsdf_device.h"
#include "query_kernels.h"

namespace ohmhip
{
constexpr uint32_t kCloudChunkVoxels = OHMHIP_CLOUD_CHUNK_VOXELS;
constexpr uint32_t kCloudWaves = 4;  ///< waves of a workgroup = counts per chunk
constexpr uint32_t kCloudWaveVoxels = kCloudChunkVoxels / kCloudWaves;
static_assert(kCloudWaveVoxels % 256 == 0, "a wave's share is whole 256-voxel groups");

/// Consecutive voxels of one tile.  Block addresses are those of the chunk's FIRST voxel; null: a tile of a tiled
/// region that holds no data, which reads as a cleared chunk does (occupancy +inf, clearance -1, zeros).
struct CloudChunk
{
  const void *sel;    ///< the layer the test reads: occupancy (OCCUPANCY, CLEARANCE), traversal (DENSITY), tsdf (TSDF)
  const void *aux;    ///< mean (OCCUPANCY when in use, DENSITY), clearance (CLEARANCE), else null
  uint32_t first;     ///< index of the first voxel in the REGION's block: x + y * dx + z * dx * dy
  uint32_t count;     ///< voxels, <= kCloudChunkVoxels
  int16_t region[3];  ///< the caller's region key
  uint16_t wide;      ///< sel is a float layer and 16-byte aligned here: float4 loads
};
static_assert(sizeof(CloudChunk) == 32, "work list records are two 16-byte words");

struct CloudArgs
{
  MapConst mc;  ///< key maths; origin zeroed for the modes that export voxelCentreLocal
  const CloudChunk *chunks;
  int mode;                ///< OHMHIP_CLOUD_*
  int export_free;         ///< OCCUPANCY
  int use_mean;            ///< positions carry the decoded mean (layer present and not ignored)
  int export_type;         ///< CLEARANCE
  float density_threshold, surface_distance, colour_range;
  uint32_t *counts;                     ///< [chunks * kCloudWaves (+ 1: a zero, so that the scan ends in the total)]
  const unsigned long long *offsets;    ///< exclusive scan of counts
  unsigned long long capacity;          ///< points the result arrays hold
  double *out_pos;                      ///< [capacity][3]
  GpuKeyOut *out_keys;                  ///< [capacity] or null
  float *out_values;                    ///< [capacity] or null
};

/// The mode's test of voxel i of chunk c and the value it exports.  s: the voxel's word of the selecting layer (TSDF:
/// weight, s2 distance).  fp32 as the reference evaluates it.
__device__ inline bool cloudTest(const CloudArgs &a, const CloudChunk &c, uint32_t i, float s, float s2, float &value)
{
  const float inf = __int_as_float(0x7f800000);
  const float threshold = a.mc.threshold_value;
  switch (a.mode)
  {
  case OHMHIP_CLOUD_OCCUPANCY:
  {
    // isOccupied (ohm/VoxelOccupancy.h:161-164) and isFree: a NaN is neither
    value = s;
    const bool observed = s != inf;
    return (observed && s >= threshold) || (a.export_free && observed && s < threshold);
  }
  case OHMHIP_CLOUD_DENSITY:
  {
    // voxelDensity (ohm/Density.h:43-55)
    const uint32_t count = c.aux ? static_cast<const uint2 *>(c.aux)[i].y : 0u;
    value = (count > 0u) ? ((s > 0.0f) ? float(count) / s : inf) : 0.0f;
    return value >= a.density_threshold;
  }
  case OHMHIP_CLOUD_TSDF:
    value = s2;
    return s > 0.0f && fabsf(s2) < a.surface_distance;
  default:  // OHMHIP_CLOUD_CLEARANCE
  {
    // occupancyType (ohm/VoxelOccupancy.h:116-128)
    const int type = (s < inf) ? ((s < threshold) ? int(kOtFree) : int(kOtOccupied)) : int(kOtUnobserved);
    if (type < a.export_type)
    {
      return false;
    }
    float range = c.aux ? static_cast<const float *>(c.aux)[i] : -1.0f;
    range = (range < 0.0f) ? a.colour_range : range;
    value = range;
    return range >= 0.0f;
  }
  }
}

/// Voxel i of chunk c as the run loads it: a dword of a float layer, or the TSDF voxel's two.
__device__ inline void cloudLoad(const CloudArgs &a, const CloudChunk &c, uint32_t i, float &s, float &s2)
{
  s2 = 0.0f;
  if (a.mode == OHMHIP_CLOUD_TSDF)
  {
    const float2 t = c.sel ? static_cast<const float2 *>(c.sel)[i] : make_float2(0.0f, 0.0f);
    s = t.x;
    s2 = t.y;
    return;
  }
  const float cleared = (a.mode == OHMHIP_CLOUD_DENSITY) ? 0.0f : __int_as_float(0x7f800000);
  s = c.sel ? static_cast<const float *>(c.sel)[i] : cleared;
}

/// Four consecutive float voxels from 4 * i4 (wide chunks only).
__device__ inline float4 cloudLoad4(const CloudArgs &a, const CloudChunk &c, uint32_t i4)
{
  const float cleared = (a.mode == OHMHIP_CLOUD_DENSITY) ? 0.0f : __int_as_float(0x7f800000);
  return c.sel ? static_cast<const float4 *>(c.sel)[i4] : make_float4(cleared, cleared, cleared, cleared);
}

__device__ inline unsigned long long cloudLanesBelow()
{
  return (1ull << (threadIdx.x & 63u)) - 1ull;
}

/// Point `slot` of the result: voxel i of chunk c.  Positions in fp64 in the reference's order (voxelCentre,
/// ohm/OccupancyMap.h:757-778; positionSafe, ohm/VoxelMean.h:47-54: a coord of 0 decodes like any other).
__device__ inline void cloudWrite(const CloudArgs &a, const CloudChunk &c, uint32_t i, unsigned long long slot, float value)
{
  if (slot >= a.capacity)
  {
    return;
  }
  const uint32_t index = c.first + i;
  const uint32_t dx = uint32_t(a.mc.kdim[0]), dy = uint32_t(a.mc.kdim[1]);
  const uint32_t row = index / dx;
  const int lx = int(index - row * dx);
  const int lz = int(row / dy);
  const int ly = int(row - uint32_t(lz) * dy);
  double x = voxelCentreAxis(a.mc, 0, c.region[0], lx);
  double y = voxelCentreAxis(a.mc, 1, c.region[1], ly);
  double z = voxelCentreAxis(a.mc, 2, c.region[2], lz);
  if (a.use_mean)
  {
    const uint32_t coord = c.aux ? static_cast<const uint2 *>(c.aux)[i].x : 0u;
    const D3 off = subVoxelToLocal(coord, a.mc.resolution);
    x += off.x;
    y += off.y;
    z += off.z;
  }
  double *pos = a.out_pos + 3ull * slot;
  pos[0] = x;
  pos[1] = y;
  pos[2] = z;
  if (a.out_keys)
  {
    GpuKeyOut k;
    k.region[0] = c.region[0];
    k.region[1] = c.region[1];
    k.region[2] = c.region[2];
    k.voxel[0] = uint8_t(lx);
    k.voxel[1] = uint8_t(ly);
    k.voxel[2] = uint8_t(lz);
    k.voxel[3] = 0;
    a.out_keys[slot] = k;
  }
  if (a.out_values)
  {
    a.out_values[slot] = value;
  }
}

/// The traversal both kernels share: wave `wave` of the workgroup over its share of chunk c.  EMIT: passing voxels are
/// written from slot `base` on.  Returns the wave's count.
template <bool EMIT>
__device__ inline uint32_t cloudWalkWave(const CloudArgs &a, const CloudChunk &c, uint32_t wave, unsigned long long base)
{
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t at = wave * kCloudWaveVoxels;
  const uint32_t end = min(at + kCloudWaveVoxels, c.count);
  const unsigned long long below = cloudLanesBelow();
  uint32_t total = 0;
  if (c.wide)
  {
    for (; at + 256u <= end; at += 256u)
    {
      const float4 v = cloudLoad4(a, c, (at >> 2) + lane);
      const uint32_t i = at + 4u * lane;
      float value[4];
      const bool p0 = cloudTest(a, c, i, v.x, 0.0f, value[0]);
      const bool p1 = cloudTest(a, c, i + 1u, v.y, 0.0f, value[1]);
      const bool p2 = cloudTest(a, c, i + 2u, v.z, 0.0f, value[2]);
      const bool p3 = cloudTest(a, c, i + 3u, v.w, 0.0f, value[3]);
      const unsigned long long b0 = __ballot(p0), b1 = __ballot(p1), b2 = __ballot(p2), b3 = __ballot(p3);
      if (EMIT)
      {
        unsigned long long slot =
          base + total + uint32_t(__popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below));
        if (p0)
        {
          cloudWrite(a, c, i, slot++, value[0]);
        }
        if (p1)
        {
          cloudWrite(a, c, i + 1u, slot++, value[1]);
        }
        if (p2)
        {
          cloudWrite(a, c, i + 2u, slot++, value[2]);
        }
        if (p3)
        {
          cloudWrite(a, c, i + 3u, slot, value[3]);
        }
      }
      total += uint32_t(__popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3));
    }
  }
  for (; at < end; at += 64u)
  {
    const uint32_t i = at + lane;
    bool pass = false;
    float value = 0.0f;
    if (i < end)
    {
      float s, s2;
      cloudLoad(a, c, i, s, s2);
      pass = cloudTest(a, c, i, s, s2, value);
    }
    const unsigned long long b = __ballot(pass);
    if (EMIT && pass)
    {
      cloudWrite(a, c, i, base + total + uint32_t(__popcll(b & below)), value);
    }
    total += uint32_t(__popcll(b));
  }
  return total;
}

__global__ void __launch_bounds__(256) k_cloud_count(CloudArgs a)
{
  const CloudChunk c = a.chunks[blockIdx.x];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t total = cloudWalkWave<false>(a, c, wave, 0ull);
  if ((threadIdx.x & 63u) == 0u)
  {
    a.counts[size_t(blockIdx.x) * kCloudWaves + wave] = total;
  }
}

__global__ void __launch_bounds__(256) k_cloud_emit(CloudArgs a)
{
  const uint32_t wave = threadIdx.x >> 6;
  const size_t part = size_t(blockIdx.x) * kCloudWaves + wave;
  const unsigned long long base = a.offsets[part];
  if (a.counts[part] == 0u || base >= a.capacity)
  {
    return;  // nothing passes in this wave's share, or everything it holds lies beyond the arrays
  }
  const CloudChunk c = a.chunks[blockIdx.x];
  cloudWalkWave<true>(a, c, wave, base);
}
}  // namespace ohmhip

#endif  // OHMHIP_CLOUD_KERNELS_H
