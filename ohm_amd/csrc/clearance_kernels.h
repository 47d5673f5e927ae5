// clearance_kernels.h -- ClearanceProcess / LineQueryGpu: the clearance of voxels (distance to the nearest obstructing
// voxel within a search radius) against the device-resident occupancy layer, read only.
//
//   k_clearance_regions_lds    512 lanes / 8^3 target voxels   window staged in LDS as a candidate bitmask (h <= 32)
//   k_clearance_mask           1 wave / mask word              large windows: candidate bitmask of a region's padded box
//   k_clearance_regions_global 1 lane / target voxel           large windows: the same walk over the global bitmask
//   k_clearance_keys           1 lane / key                    arbitrary voxels (line queries): occupancy read directly
//
// Every path computes calculateNearestNeighbour (ohm/private/VoxelAlgorithms.cpp:22-98) as written, bit for bit: the
// window of moveKey() neighbours (the region key adds in int16 and wraps), fp32 centres from the fp64 voxelCentre
// (ohm/OccupancyMap.h:757-777, origin 0), the separation, its dot products and the radius test in fp32 in the CPU's
// order (no FMA: the library builds with -ffp-contract=off), and selection of the smallest scaled range.  The CPU scans
// z, y, x from -h to h and takes a candidate only when it is strictly closer, so ties go to the earliest in scan order;
// the device visits rows centre-out (the best range tightens early) and selects by (scaled range, scan index)
// lexicographically, which picks the same voxel.
//
// Pruning is conservative in float: for a row (dy, dz) every candidate's scaled range s2 = fl(fl(fl(x^2) + fl(y^2)) +
// fl(z^2)) is >= fl(fl(y^2) + fl(z^2)) >= fl(z^2) because rounding is monotone and fl(x^2) >= 0.  A row or plane whose
// bound exceeds the best s2 cannot hold a candidate that ties or beats it; the same bound on the unscaled range skips
// rows beyond the search radius.
//
// The occupancy is found as the rays query finds it (queryTileBlock: resident tile through the region hash, else the
// host store's pinned record, else no region).  The map is not written.
#ifndef OHMHIP_CLEARANCE_KERNELS_H
#define OHMHIP_CLEARANCE_KERNELS_H

#include "query_kernels.h"

namespace ohmhip
{
constexpr int kClearanceTile = 8;                ///< target voxels per axis of a k_clearance_regions_lds workgroup
constexpr int kClearanceThreads = kClearanceTile * kClearanceTile * kClearanceTile;
constexpr int kClearanceLdsMaxH = 32;            ///< largest half extent staged in LDS (72^2 rows x 2 words: 81 KiB)
constexpr int kClearanceMaxH = 127;              ///< largest half extent at all (scan index and window fit easily)
constexpr int kClearanceMaxTileBlocks = 1024;    ///< LDS table of the tiles a staged window touches
constexpr uint32_t kClearanceNone = 0xffffffffu;

struct ClearanceArgs : MapReadView
{
  int h;                   ///< voxel search half extent, every axis (calculateVoxelSearchHalfExtents)
  float radius;            ///< search_radius (0: no radius test)
  float scale[3];          ///< axis_scaling
  int unknown_as_occupied;
  int report_unscaled;
  const int16_t *regions;  ///< region mode: [n][3] the caller's region keys
  const GpuKeyOut *keys;   ///< key mode: [n]
  uint32_t n;              ///< regions (of this launch) or keys
  float *out;              ///< region mode: [n][region voxels], MapChunk order; key mode: [n]
  unsigned long long *mask;  ///< k_clearance_mask / _global: [n][pad z][pad y][words]
  int pad[3];              ///< region dims + 2h (global path)
  int words;               ///< u64 words per padded row (global path)
};

/// moveKeyAlongAxis (ohm/private/OccupancyMapDetail.cpp:27-93) on one axis: local key `l` of region `r` moved by
/// `step`.  Either branch of the reference is a floor division of the local key; the region key adds in int16
/// (glm::i16vec3) and wraps at its limits.
__device__ inline void clearanceMove(int r, int l, int step, int kd, int &r_out, int &l_out)
{
  const int ll = l + step;
  const int q = (ll >= 0) ? ll / kd : -((kd - 1 - ll) / kd);
  r_out = int(int16_t(uint16_t(r + q)));
  l_out = ll - q * kd;
}

/// One component of glm::vec3(map.voxelCentreLocal(key)): OccupancyMap::voxelCentre (ohm/OccupancyMap.h:757-777) in
/// fp64 in its order, origin 0, rounded to float.
__device__ inline float clearanceCentre(const MapConst &mc, int axis, int r, int l)
{
  double c = double(float(r));  // glm::vec3(key.regionKey())
  c *= mc.region_dim[axis];
  c -= 0.5 * mc.region_dim[axis];
  c += double(l) * mc.resolution;
  c += 0.5 * mc.resolution;
  return float(c);
}

/// isOccupied (ohm/VoxelOccupancy.h:161: value != +inf && value >= threshold) or, with unknown_as_occupied,
/// isUnobservedOrNull.  block == null: no such region.
__device__ inline bool clearanceCandidate(const ClearanceArgs &a, const float *block, int vi)
{
  if (!block)
  {
    return a.unknown_as_occupied != 0;
  }
  const float v = block[vi];
  if (v == __int_as_float(0x7f800000))
  {
    return a.unknown_as_occupied != 0;
  }
  return v >= a.mc.threshold_value;
}

struct ClearanceBest
{
  float s2;      ///< scaled_closest_range_sqr
  float r2;      ///< closest_range_sqr
  uint32_t idx;  ///< scan index of the selected candidate (kClearanceNone: none yet)
};

__device__ inline void clearanceTake(const ClearanceArgs &a, float ex, float ey, float ez, uint32_t idx,
                                     ClearanceBest &b)
{
  // ohm/private/VoxelAlgorithms.cpp:66-83 in its order (glm::dot: (x*x + y*y) + z*z)
  float r2 = (ex * ex + ey * ey) + ez * ez;
  const float sx = ex * a.scale[0];
  const float sy = ey * a.scale[1];
  const float sz = ez * a.scale[2];
  const float s2 = (sx * sx + sy * sy) + sz * sz;
  if (!a.report_unscaled)
  {
    r2 = s2;
  }
  if (a.radius == 0.0f || r2 <= a.radius * a.radius)
  {
    if (s2 < b.s2 || (s2 == b.s2 && b.idx != kClearanceNone && idx < b.idx))
    {
      b.s2 = s2;
      b.r2 = r2;
      b.idx = idx;
    }
  }
}

__device__ inline float clearanceResult(const ClearanceBest &b)
{
  return (b.r2 < __int_as_float(0x7f800000)) ? __builtin_sqrtf(b.r2) : -1.0f;
}

/// k-th offset of the centre-out order 0, -1, 1, -2, 2, ...
__device__ inline int clearanceOffset(int k)
{
  return (k & 1) ? -((k + 1) >> 1) : (k >> 1);
}

/// True when no candidate of a plane / row whose separations so far give the lower bounds `lb_scaled` (scaled) and
/// `lb_unscaled` can be taken: beyond the best scaled range (a tie must still be visited) or beyond the radius.
__device__ inline bool clearancePrune(const ClearanceArgs &a, float lb_scaled, float lb_unscaled, const ClearanceBest &b)
{
  if (lb_scaled > b.s2)
  {
    return true;
  }
  const float lb_range = a.report_unscaled ? lb_unscaled : lb_scaled;
  return a.radius != 0.0f && lb_range > a.radius * a.radius;
}

/// The walk of one target voxel over a candidate bitmask: rows of `nw` u64 words, row (y, z) at (z * rows_y + y) * nw,
/// bit x of a row = padded x coordinate.  (cx, cy, cz): the target's padded coordinates (the window is [c - h, c + h]
/// per axis).  centre(axis, padded coordinate) -> float centre.  The target itself is not a candidate.
template <typename CentreFn>
__device__ inline float clearanceWalk(const ClearanceArgs &a, const unsigned long long *mask, int rows_y, int nw, int cx,
                                      int cy, int cz, CentreFn centre)
{
  const int h = a.h;
  const int span = 2 * h + 1;
  const float c0x = centre(0, cx);
  const float c0y = centre(1, cy);
  const float c0z = centre(2, cz);
  ClearanceBest b = { __int_as_float(0x7f800000), __int_as_float(0x7f800000), kClearanceNone };
  const int x0 = cx - h;
  const int w_first = x0 >> 6;
  const int w_last = (x0 + 2 * h) >> 6;
  for (int kz = 0; kz < span; ++kz)
  {
    const int dz = clearanceOffset(kz);
    const float ez = centre(2, cz + dz) - c0z;
    const float sz = ez * a.scale[2];
    const float fz = sz * sz;
    const float uz = ez * ez;
    if (clearancePrune(a, fz, uz, b))
    {
      continue;
    }
    for (int ky = 0; ky < span; ++ky)
    {
      const int dy = clearanceOffset(ky);
      const float ey = centre(1, cy + dy) - c0y;
      const float sy = ey * a.scale[1];
      if (clearancePrune(a, sy * sy + fz, ey * ey + uz, b))
      {
        continue;
      }
      const unsigned long long *row = mask + size_t((cz + dz) * rows_y + (cy + dy)) * size_t(nw);
      const uint32_t base = uint32_t(((dz + h) * span + (dy + h)) * span);
      for (int w = w_first; w <= w_last; ++w)
      {
        unsigned long long bits = row[w];
        const int lo = x0 - w * 64;
        const int hi = x0 + 2 * h - w * 64;
        if (lo > 0)
        {
          bits &= ~0ull << lo;
        }
        if (hi < 63)
        {
          bits &= (2ull << hi) - 1ull;
        }
        while (bits)
        {
          const int p = w * 64 + __builtin_ctzll(bits);
          bits &= bits - 1ull;
          clearanceTake(a, centre(0, p) - c0x, ey, ez, base + uint32_t(p - x0), b);
        }
      }
    }
  }
  return clearanceResult(b);
}

/// Sub-tiles of kClearanceTile^3 per region, per axis.
__host__ __device__ inline int clearanceSubTiles(int kd)
{
  return (kd + kClearanceTile - 1) / kClearanceTile;
}

/// Bytes of dynamic LDS k_clearance_regions_lds needs at half extent h.
__host__ __device__ inline size_t clearanceLdsBytes(int h)
{
  const int w = kClearanceTile + 2 * h;
  const int nw = (w + 63) >> 6;
  return size_t(w) * size_t(w) * size_t(nw) * 8u + size_t(kClearanceMaxTileBlocks) * sizeof(const float *) +
         size_t(3 * w) * 4u * 4u;
}

/// Region mode, windows that fit in LDS.  One workgroup per 8^3 target voxels of a region (blockIdx.x = region *
/// sub-tiles + sub-tile): per-axis tables of the window's neighbour keys (tile, offset, float centre), a table of the
/// tiles the window touches (one hash probe each), then the window's candidate bitmask -- one wave per row word, one
/// lane per voxel, __ballot -- and one lane per target voxel walks it.
__global__ void __launch_bounds__(kClearanceThreads) k_clearance_regions_lds(ClearanceArgs a)
{
  extern __shared__ __attribute__((aligned(16))) unsigned long long c_lds[];
  __shared__ int l_nt[3];
  const MapConst &mc = a.mc;
  const int h = a.h;
  const int W = kClearanceTile + 2 * h;
  const int nw = (W + 63) >> 6;
  unsigned long long *l_mask = c_lds;                                                        // [W][W][nw]
  const float **l_blocks = reinterpret_cast<const float **>(l_mask + size_t(W) * W * nw);    // [nt z][nt y][nt x]
  float *l_centre = reinterpret_cast<float *>(l_blocks + kClearanceMaxTileBlocks);           // [3][W]
  int *l_offset = reinterpret_cast<int *>(l_centre + 3 * W);  // [3][W] the coordinate's part of the tile voxel index
  int *l_run = l_offset + 3 * W;                              // [3][W] index of the coordinate's tile in the window
  int *l_run_tile = l_run + 3 * W;                            // [3][W] tile coordinate per index

  const int st0 = clearanceSubTiles(mc.kdim[0]);
  const int st1 = clearanceSubTiles(mc.kdim[1]);
  const int st2 = clearanceSubTiles(mc.kdim[2]);
  const uint32_t per_region = uint32_t(st0 * st1 * st2);
  const uint32_t ri = blockIdx.x / per_region;
  const uint32_t sub = blockIdx.x - ri * per_region;
  const int o[3] = { int(sub % uint32_t(st0)) * kClearanceTile, int((sub / uint32_t(st0)) % uint32_t(st1)) * kClearanceTile,
                     int(sub / uint32_t(st0 * st1)) * kClearanceTile };
  const int tid = int(threadIdx.x);
  if (tid < 3)
  {
    const int axis = tid;
    const int r = a.regions[size_t(ri) * 3 + axis];
    const int kd = mc.kdim[axis];
    const int dim = mc.dim[axis];
    const int stride = axis == 0 ? 1 : (axis == 1 ? mc.dim[0] : mc.dim[0] * mc.dim[1]);
    int n = 0;
    int prev = 0;
    for (int i = 0; i < W; ++i)
    {
      int rr, ll;
      clearanceMove(r, o[axis], i - h, kd, rr, ll);
      const int tile = rr * mc.tile_split[axis] + ll / dim;
      l_centre[axis * W + i] = clearanceCentre(mc, axis, rr, ll);
      l_offset[axis * W + i] = (ll % dim) * stride;
      if (i == 0 || tile != prev)
      {
        l_run_tile[axis * W + n] = tile;
        prev = tile;
        ++n;
      }
      l_run[axis * W + i] = n - 1;
    }
    l_nt[axis] = n;
  }
  __syncthreads();
  const int nt0 = l_nt[0];
  const int nt1 = l_nt[1];
  const int n_blocks = nt0 * nt1 * l_nt[2];  // <= kClearanceMaxTileBlocks (the host chose this path by that bound)
  for (int e = tid; e < n_blocks; e += kClearanceThreads)
  {
    const int ix = e % nt0;
    const int iy = (e / nt0) % nt1;
    const int iz = e / (nt0 * nt1);
    l_blocks[e] = queryTileBlock(a, l_run_tile[ix], l_run_tile[W + iy], l_run_tile[2 * W + iz]);
  }
  __syncthreads();
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int items = W * W * nw;
  for (int it = wave; it < items; it += kClearanceThreads / 64)
  {
    const int row = it / nw;
    const int x = (it - row * nw) * 64 + lane;
    const int y = row % W;
    const int z = row / W;
    bool cand = false;
    if (x < W)
    {
      const float *block = l_blocks[l_run[x] + nt0 * (l_run[W + y] + nt1 * l_run[2 * W + z])];
      cand = clearanceCandidate(a, block, l_offset[x] + l_offset[W + y] + l_offset[2 * W + z]);
    }
    const unsigned long long bits = __ballot(cand);
    if (lane == 0)
    {
      l_mask[it] = bits;
    }
  }
  __syncthreads();

  const int tx = tid & (kClearanceTile - 1);
  const int ty = (tid / kClearanceTile) & (kClearanceTile - 1);
  const int tz = tid / (kClearanceTile * kClearanceTile);
  const int lx = o[0] + tx;
  const int ly = o[1] + ty;
  const int lz = o[2] + tz;
  if (lx >= mc.kdim[0] || ly >= mc.kdim[1] || lz >= mc.kdim[2])
  {
    return;
  }
  const int cx = tx + h;
  const int cy = ty + h;
  const int cz = tz + h;
  float result = 0.0f;  // the target itself is a candidate: 0 (VoxelAlgorithms.cpp:41-46)
  if (!((l_mask[size_t(cz * W + cy) * nw + (cx >> 6)] >> (cx & 63)) & 1ull))
  {
    result = clearanceWalk(a, l_mask, W, nw, cx, cy, cz,
                           [&](int axis, int i) { return l_centre[axis * W + i]; });
  }
  a.out[size_t(ri) * size_t(mc.kdim[0] * mc.kdim[1] * mc.kdim[2]) + size_t(lx + ly * mc.kdim[0] + lz * mc.kdim[0] * mc.kdim[1])] =
    result;
}

/// Tile block and tile voxel index of the neighbour at padded coordinates (px, py, pz) of region r (padded coordinate
/// = local + h): the global path's occupancy read.
__device__ inline bool clearancePaddedCandidate(const ClearanceArgs &a, const int r[3], int px, int py, int pz)
{
  const MapConst &mc = a.mc;
  int t[3], off = 0;
  const int p[3] = { px, py, pz };
  const int stride[3] = { 1, mc.dim[0], mc.dim[0] * mc.dim[1] };
#pragma unroll
  for (int axis = 0; axis < 3; ++axis)
  {
    int rr, ll;
    clearanceMove(r[axis], 0, p[axis] - a.h, mc.kdim[axis], rr, ll);
    t[axis] = rr * mc.tile_split[axis] + ll / mc.dim[axis];
    off += (ll % mc.dim[axis]) * stride[axis];
  }
  return clearanceCandidate(a, queryTileBlock(a, t[0], t[1], t[2]), off);
}

/// Large windows, pass 1: the candidate bitmask of each region's padded box (region dims + 2h per axis).  One wave per
/// row word (grid-stride), one lane per voxel; the occupancy is probed per voxel (no LDS tables: this path is for windows
/// beyond them and need not be fast).
__global__ void __launch_bounds__(256) k_clearance_mask(ClearanceArgs a)
{
  const int lane = int(threadIdx.x & 63u);
  const size_t per_region = size_t(a.pad[2]) * size_t(a.pad[1]) * size_t(a.words);
  const size_t items = per_region * a.n;
  const size_t waves = size_t(gridDim.x) * (blockDim.x / 64u);
  for (size_t it = size_t(blockIdx.x) * (blockDim.x / 64u) + (threadIdx.x / 64u); it < items; it += waves)
  {
    const size_t ri = it / per_region;
    const size_t rest = it - ri * per_region;
    const size_t row = rest / size_t(a.words);
    const int x = int(rest - row * size_t(a.words)) * 64 + lane;
    const int y = int(row % size_t(a.pad[1]));
    const int z = int(row / size_t(a.pad[1]));
    bool cand = false;
    if (x < a.pad[0])
    {
      const int r[3] = { a.regions[ri * 3 + 0], a.regions[ri * 3 + 1], a.regions[ri * 3 + 2] };
      cand = clearancePaddedCandidate(a, r, x, y, z);
    }
    const unsigned long long bits = __ballot(cand);
    if (lane == 0)
    {
      a.mask[it] = bits;
    }
  }
}

/// Large windows, pass 2: one lane per target voxel walks its region's bitmask; centres computed in place.
__global__ void __launch_bounds__(256) k_clearance_regions_global(ClearanceArgs a)
{
  const MapConst &mc = a.mc;
  const size_t kvox = size_t(mc.kdim[0]) * size_t(mc.kdim[1]) * size_t(mc.kdim[2]);
  const size_t t = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= kvox * a.n)
  {
    return;
  }
  const size_t ri = t / kvox;
  const int v = int(t - ri * kvox);
  const int lx = v % mc.kdim[0];
  const int ly = (v / mc.kdim[0]) % mc.kdim[1];
  const int lz = v / (mc.kdim[0] * mc.kdim[1]);
  const int r[3] = { a.regions[ri * 3 + 0], a.regions[ri * 3 + 1], a.regions[ri * 3 + 2] };
  const unsigned long long *mask = a.mask + ri * size_t(a.pad[2]) * size_t(a.pad[1]) * size_t(a.words);
  const int h = a.h;
  float result = 0.0f;
  const int cx = lx + h;
  const int cy = ly + h;
  const int cz = lz + h;
  if (!((mask[size_t(cz * a.pad[1] + cy) * a.words + (cx >> 6)] >> (cx & 63)) & 1ull))
  {
    result = clearanceWalk(a, mask, a.pad[1], a.words, cx, cy, cz, [&](int axis, int i) {
      int rr, ll;
      clearanceMove(r[axis], 0, i - h, mc.kdim[axis], rr, ll);
      return clearanceCentre(mc, axis, rr, ll);
    });
  }
  a.out[t] = result;
}

/// Key mode: one lane per key (local coordinates checked by the host), the same selection with the occupancy read
/// directly -- rows centre-out, x from -h to h, the tile block cached while the tile stays the same.
__global__ void __launch_bounds__(256) k_clearance_keys(ClearanceArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n)
  {
    return;
  }
  const MapConst &mc = a.mc;
  const GpuKeyOut key = a.keys[i];
  const int r[3] = { key.region[0], key.region[1], key.region[2] };
  const int l[3] = { key.voxel[0], key.voxel[1], key.voxel[2] };
  const int h = a.h;
  const int span = 2 * h + 1;
  const int stride[3] = { 1, mc.dim[0], mc.dim[0] * mc.dim[1] };
  auto tileOf = [&](int axis, int rr, int ll, int &tile, int &off) {
    tile = rr * mc.tile_split[axis] + ll / mc.dim[axis];
    off = (ll % mc.dim[axis]) * stride[axis];
  };
  int t[3], off[3];
  for (int axis = 0; axis < 3; ++axis)
  {
    tileOf(axis, r[axis], l[axis], t[axis], off[axis]);
  }
  if (clearanceCandidate(a, queryTileBlock(a, t[0], t[1], t[2]), off[0] + off[1] + off[2]))
  {
    a.out[i] = 0.0f;
    return;
  }
  const float c0x = clearanceCentre(mc, 0, r[0], l[0]);
  const float c0y = clearanceCentre(mc, 1, r[1], l[1]);
  const float c0z = clearanceCentre(mc, 2, r[2], l[2]);
  ClearanceBest b = { __int_as_float(0x7f800000), __int_as_float(0x7f800000), kClearanceNone };
  int ctx = 0x7fffffff, cty = 0, ctz = 0;
  const float *cblock = nullptr;
  for (int kz = 0; kz < span; ++kz)
  {
    const int dz = clearanceOffset(kz);
    int rz, lz, tz, oz;
    clearanceMove(r[2], l[2], dz, mc.kdim[2], rz, lz);
    const float ez = clearanceCentre(mc, 2, rz, lz) - c0z;
    const float sz = ez * a.scale[2];
    const float fz = sz * sz;
    const float uz = ez * ez;
    if (clearancePrune(a, fz, uz, b))
    {
      continue;
    }
    tileOf(2, rz, lz, tz, oz);
    for (int ky = 0; ky < span; ++ky)
    {
      const int dy = clearanceOffset(ky);
      int ry, ly, ty, oy;
      clearanceMove(r[1], l[1], dy, mc.kdim[1], ry, ly);
      const float ey = clearanceCentre(mc, 1, ry, ly) - c0y;
      const float sy = ey * a.scale[1];
      if (clearancePrune(a, sy * sy + fz, ey * ey + uz, b))
      {
        continue;
      }
      tileOf(1, ry, ly, ty, oy);
      const uint32_t base = uint32_t(((dz + h) * span + (dy + h)) * span);
      for (int dx = -h; dx <= h; ++dx)
      {
        int rx, lx, tx, ox;
        clearanceMove(r[0], l[0], dx, mc.kdim[0], rx, lx);
        tileOf(0, rx, lx, tx, ox);
        if (tx != ctx || ty != cty || tz != ctz)
        {
          cblock = queryTileBlock(a, tx, ty, tz);
          ctx = tx;
          cty = ty;
          ctz = tz;
        }
        if (clearanceCandidate(a, cblock, ox + oy + oz))
        {
          clearanceTake(a, clearanceCentre(mc, 0, rx, lx) - c0x, ey, ez, base + uint32_t(dx + h), b);
        }
      }
    }
  }
  a.out[i] = clearanceResult(b);
}
}  // namespace ohmhip

#endif  // OHMHIP_CLEARANCE_KERNELS_H
