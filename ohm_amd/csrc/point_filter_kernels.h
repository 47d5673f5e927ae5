// point_filter_kernels.h -- a point cloud filtered against the resident map, read only: ohmfilter's filterCloud (utils/
// ohmfilter/ohmfilter.cpp:150-279) with filterPointByCovariance (:67-91).
//
//   k_pf_classify  1 lane / point   key, occupancy, the covariance test; status, value and key per point, one kept
//                                   count per wave
//   (exclusive scan of the counts, 64 bit: rocPRIM, point_filter_impl.h)
//   k_pf_emit      1 lane / point   a kept point writes its index at the offset of its wave + its rank among the kept
//                                   points before it in the wave
//
// The rule is that of include/ohmhip.h ("POINT FILTER"); tests/point_filter_ref.py is the same restatement on the CPU.
//
// Shape.  Points are independent; lane i of the grid owns point i, so the flat array of per-wave counts is in input
// order and its exclusive scan is every wave's first slot of the kept indices.  The tile of a point is resolved as
// k_read_voxels resolves it -- region hash, then the host store -- and lanes of a wave that fall in the same tile share
// one probe (waveMatch): the points of a scan are spatially coherent.  The one probe serves all three layers: a pool
// slot addresses three pool blocks, a store record holds its layers at fixed offsets from the occupancy block
// (LayerView / foundTileLayer, query_kernels.h).  The mean and covariance voxels are loaded only by lanes whose voxel is
// occupied.  Counting is __popcll(__ballot(kept)), ranking __popcll(ballot & lanes below).  No atomics: two calls return
// identical bytes.
#ifndef OHMHIP_POINT_FILTER_KERNELS_H
#define OHMHIP_POINT_FILTER_KERNELS_H

#include "neighbours_kernels.h"

namespace ohmhip
{
enum : uint8_t
{
  kPfDropped = 0,  ///< null key or not occupied
  kPfKept = 1,
  kPfRemoved = 2   ///< occupied, removed by the covariance test
};

struct PointFilterArgs : MapReadView
{
  LayerView mean;             ///< [tile voxel]; no layer: no covariance test
  LayerView covariance;       ///< [tile voxel][6]
  int test;                   ///< the covariance test runs
  double limit;               ///< 3.0 + expected_value_tolerance, fp64
  const double *points;       ///< point i at points[i * stride]
  unsigned long long stride;  ///< doubles, >= 3
  unsigned long long n;
  unsigned long long first_index;  ///< index of point 0 in the caller's array (pieces of the host variant)
  uint8_t *status;                 ///< [n]
  double *values;                  ///< [n] or null
  GpuKeyOut *keys;                 ///< [n] or null
  uint32_t *counts;                ///< [waves (+ 1: a zero, so that the scan ends in the total)]
  const unsigned long long *offsets;  ///< exclusive scan of counts
  unsigned long long first_slot;      ///< kept points of the pieces before this one
  unsigned long long capacity;        ///< indices the caller's array holds
  unsigned long long *kept;           ///< slot s at kept[s - first_slot]
};

/// filterPointByCovariance's value (utils/ohmfilter/ohmfilter.cpp:86-88) for d = point - mean and the voxel's packed
/// square root c (covarianceSqrtMatrix, ohm/CovarianceVoxel.h:71-91): v = inverse(S) * d, a = dot(v, v).  The inverse
/// is the adjugate times 1 / determinant over the FULL 3 x 3 matrix, zeros included, in the order include/ohmhip.h
/// states; m[c][r] is column c, row r, as glm stores it.
__device__ inline double pointFilterValue(const float c[6], double dx, double dy, double dz)
{
  const double m[3][3] = { { double(c[0]), double(c[1]), double(c[3]) },
                           { 0.0, double(c[2]), double(c[4]) },
                           { 0.0, 0.0, double(c[5]) } };
  const double one_over_det = 1.0 / (m[0][0] * (m[1][1] * m[2][2] - m[2][1] * m[1][2]) -
                                     m[1][0] * (m[0][1] * m[2][2] - m[2][1] * m[0][2]) +
                                     m[2][0] * (m[0][1] * m[1][2] - m[1][1] * m[0][2]));
  double inv[3][3];
  inv[0][0] = (m[1][1] * m[2][2] - m[2][1] * m[1][2]) * one_over_det;
  inv[1][0] = -(m[1][0] * m[2][2] - m[2][0] * m[1][2]) * one_over_det;
  inv[2][0] = (m[1][0] * m[2][1] - m[2][0] * m[1][1]) * one_over_det;
  inv[0][1] = -(m[0][1] * m[2][2] - m[2][1] * m[0][2]) * one_over_det;
  inv[1][1] = (m[0][0] * m[2][2] - m[2][0] * m[0][2]) * one_over_det;
  inv[2][1] = -(m[0][0] * m[2][1] - m[2][0] * m[0][1]) * one_over_det;
  inv[0][2] = (m[0][1] * m[1][2] - m[1][1] * m[0][2]) * one_over_det;
  inv[1][2] = -(m[0][0] * m[1][2] - m[1][0] * m[0][2]) * one_over_det;
  inv[2][2] = (m[0][0] * m[1][1] - m[1][0] * m[0][1]) * one_over_det;
  const double vx = (inv[0][0] * dx + inv[1][0] * dy) + inv[2][0] * dz;
  const double vy = (inv[0][1] * dx + inv[1][1] * dy) + inv[2][1] * dz;
  const double vz = (inv[0][2] * dx + inv[1][2] * dy) + inv[2][2] * dz;
  return (vx * vx + vy * vy) + vz * vz;
}

__global__ void __launch_bounds__(256) k_pf_classify(PointFilterArgs a)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned lane = laneId();
  const MapConst &mc = a.mc;
  const bool in_range = i < a.n;
  double p[3] = { 0.0, 0.0, 0.0 };
  if (in_range)
  {
    const double *src = a.points + i * a.stride;
    p[0] = src[0];
    p[1] = src[1];
    p[2] = src[2];
  }
  // OccupancyMap::voxelKey: the caller's key where the reference has one (a region whose TILE coordinates leave the
  // packed key's range still has a key, as ohmhip_map_voxel_keys writes it; the map cannot hold it)
  int region[3], local[3];
  bool beyond_tiles = false;
  const bool addressable = voxelKey(mc, p, region, local, &beyond_tiles);
  GpuKeyOut k = queryNullKey();
  if (addressable || beyond_tiles)
  {
    k.region[0] = int16_t(region[0]);
    k.region[1] = int16_t(region[1]);
    k.region[2] = int16_t(region[2]);
    k.voxel[0] = uint8_t(local[0]);
    k.voxel[1] = uint8_t(local[1]);
    k.voxel[2] = uint8_t(local[2]);
  }
  // Key::isNull (ohm/Key.h:206): the one addressable corner region reads as null
  const bool valid = in_range && !keyIsNull(addressable, region);
  const int jy = valid ? local[1] / mc.dim[1] : 0, jz = valid ? local[2] / mc.dim[2] : 0;
  const int tx = region[0];
  const int ty = region[1] * mc.tile_split[1] + jy;
  const int tz = region[2] * mc.tile_split[2] + jz;
  const uint32_t mix = uint32_t(tx) ^ (uint32_t(ty) * 0x9e3779b1u) ^ (uint32_t(tz) * 0x85ebca6bu);
  int leader;
  unsigned long long group;
  waveMatch(valid, mix, lane, leader, group);
  const int src_lane = (leader < 0) ? int(lane) : leader;
  const bool same = __shfl(tx, src_lane) == tx && __shfl(ty, src_lane) == ty && __shfl(tz, src_lane) == tz;
  const bool probes = valid && (leader == int(lane) || !same);
  FoundTile t = { kSlotUnassigned, nullptr };
  if (probes)
  {
    t = mapFindTile(a, tx, ty, tz);
  }
  const uint32_t leader_slot = __shfl(t.slot, src_lane);
  const uint64_t leader_stored = shfl64(uint64_t(reinterpret_cast<uintptr_t>(t.stored)), src_lane);
  if (valid && !probes)
  {
    t.slot = leader_slot;
    t.stored = reinterpret_cast<const float *>(uintptr_t(leader_stored));
  }

  // (compiler builtins below, not the HIP headers' wrappers -- fabs, __longlong_as_double, __int_as_float: one more caller
  // of a wrapper the integration kernels share changes how those kernels are compiled, scripts/kernel_fingerprint.py)
  uint8_t status = kPfDropped;
  double value = __builtin_bit_cast(double, 0x7ff8000000000000ull);  // a quiet NaN
  const bool resident = t.slot != kSlotUnassigned;
  if (valid && (resident || t.stored))
  {
    const size_t voxel = size_t(local[0]) + size_t(local[1] - jy * mc.dim[1]) * size_t(mc.dim[0]) +
                         size_t(local[2] - jz * mc.dim[2]) * size_t(mc.dim[0]) * size_t(mc.dim[1]);
    const size_t pool_voxel = size_t(t.slot) * size_t(mc.region_voxels) + voxel;
    const float v = resident ? a.occupancy[pool_voxel] : t.stored[voxel];
    // isOccupied (ohm/VoxelOccupancy.h:161-164): a NaN is not
    if (v != __builtin_huge_valf() && v >= mc.threshold_value)
    {
      status = kPfKept;
      if (a.test)
      {
        // (a.test: both views hold a layer, and the tile was found)
        const uint2 *mean_at = foundTileLayer<uint2>(t, a.mean, size_t(mc.region_voxels)) + voxel;
        const float *cov_at = foundTileLayer<float>(t, a.covariance, 6u * size_t(mc.region_voxels)) + 6u * voxel;
        const uint32_t coord = mean_at->x;
        // (24-byte voxels: 8-byte aligned)
        const float2 c01 = reinterpret_cast<const float2 *>(cov_at)[0];
        const float2 c23 = reinterpret_cast<const float2 *>(cov_at)[1];
        const float2 c45 = reinterpret_cast<const float2 *>(cov_at)[2];
        const float c[6] = { c01.x, c01.y, c23.x, c23.y, c45.x, c45.y };
        // positionUnsafe (ohm/VoxelMean.h:47-54): the centre, then the decoded mean added
        const D3 off = subVoxelToLocal(coord, mc.resolution);
        double mx = voxelCentreAxis(mc, 0, region[0], local[0]);
        double my = voxelCentreAxis(mc, 1, region[1], local[1]);
        double mz = voxelCentreAxis(mc, 2, region[2], local[2]);
        mx += off.x;
        my += off.y;
        mz += off.z;
        value = pointFilterValue(c, p[0] - mx, p[1] - my, p[2] - mz);
        status = (__builtin_fabs(value) < a.limit) ? uint8_t(kPfKept) : uint8_t(kPfRemoved);
      }
    }
  }
  const unsigned long long kept = __ballot(status == kPfKept);
  if (lane == 0u)
  {
    a.counts[i >> 6] = uint32_t(__popcll(kept));
  }
  if (!in_range)
  {
    return;
  }
  a.status[i] = status;
  if (a.values)
  {
    a.values[i] = value;
  }
  if (a.keys)
  {
    a.keys[i] = k;
  }
}

__global__ void __launch_bounds__(256) k_pf_emit(PointFilterArgs a)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool kept = i < a.n && a.status[i] == kPfKept;
  const unsigned long long b = __ballot(kept);
  const unsigned long long slot = a.first_slot + a.offsets[i >> 6] + uint32_t(__popcll(b & cloudLanesBelow()));
  if (kept && slot < a.capacity)
  {
    a.kept[slot - a.first_slot] = a.first_index + i;
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_POINT_FILTER_KERNELS_H
