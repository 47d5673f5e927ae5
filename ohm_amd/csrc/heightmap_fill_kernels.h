// heightmap_fill_kernels.h -- the flood-fill heightmap (ohm::Heightmap::buildHeightmap, HeightmapMode::kSimpleFill)
// built on the device from the resident map, read only.  Rules F1-F6 of include/ohmhip.h ("HEIGHTMAP, FLOOD FILL").
//
// The reference pops one key at a time from a FIFO.  Numbered in FIFO order its visits fall into generations:
// generation 0 is the seed, generation t + 1 the keys accepted while generation t is visited, in acceptance order.  The
// queue is one device array, a generation is a range of it, and the host launches one round per generation:
//
//   k_hmfill_columns  1 lane / key of the generation   F3, F6: supporting voxel, ground, the cell value (the device
//                                                      functions of heightmap_kernels.h); atomicMax of the visit number
//                                                      per heightmap cell; the key's 9 cell events as sort keys
//   (radix sort)                                       the events by (cell, key index)
//   k_hmfill_replay   1 lane / sorted event            the first event of a cell replays the cell's events in order --
//                                                      F5 a pop sets the cell, F4 an offer is accepted when the cell is
//                                                      unvisited or the offer lower -- and flags the accepted offers;
//                                                      lanes below the generation's size also commit their key's cell
//                                                      value when it is the cell's winner so far
//   (exclusive scan)                                   of the accept flags in (key index, neighbour slot) order
//   k_hmfill_append   1 lane / offer                   accepted offers become the next generation, behind this one
//
// Exactness.  grid[c] is read and written only by pops of keys at c and by offers to c.  Key i of a generation adds at
// most one event to cell c: its pop when it sits at c, else one offer when c is one of its 8 neighbours.  In the
// reference key i is popped, then makes its offers in slot order, then key i + 1 is popped: the events of one cell,
// ordered by i, are in the reference's order, and nothing else a decision depends on is shared between cells.
// Generations run in order on one stream, so the winner of a heightmap cell -- the largest visit number -- may be
// committed per generation: a later generation overwrites.
#ifndef OHMHIP_HEIGHTMAP_FILL_KERNELS_H
#define OHMHIP_HEIGHTMAP_FILL_KERNELS_H

#include "heightmap_kernels.h"

namespace ohmhip
{
constexpr uint32_t kHmFillNoCell = 0xffffffffu;

struct HeightmapFillArgs : HeightmapArgs  ///< `winner` is not used; rec_* hold one record per key of the generation
{
  uint2 *queue;              ///< every visit in sequence order: (grid cell ib * na + ia, height offset h)
  uint32_t gen_begin;        ///< the generation: queue[gen_begin .. gen_begin + gen_count)
  uint32_t gen_count;
  int seed_generation;       ///< generation 0: its key is not popped
  unsigned index_bits;       ///< sort key: cell << index_bits | key index in the generation
  uint32_t grid_cells;       ///< na * nb; a sort key of this cell is "no event"
  int *grid;                 ///< [na * nb] PlaneFillWalker::Visit::height, -1: unvisited
  uint32_t *ground_h;        ///< [gen_count] hg of each key
  uint32_t *rec_cell;        ///< [gen_count] the heightmap cell the key writes, kHmFillNoCell: none
  unsigned long long *keys;  ///< [9 * gen_count] events, slot-major: [0] the pop, [1 + k] the offer through slot k
  const unsigned long long *sorted;
  uint32_t *accept;          ///< [8 * gen_count + 1] accept flag of offer (i, k) at 8 * i + k; the last one is 0
  const uint32_t *accept_at; ///< its exclusive scan
  uint32_t *cell_visit;      ///< [ma * mb] 1 + the largest visit number that wrote the cell, 0: none
  uint32_t *out_visit;       ///< null: not requested
  uint32_t *out_log;         ///< null: not requested
  uint32_t log_count;        ///< visits to write to out_log
};

/// Rule 3, the selection ladder of findNearestSupportingVoxel (:346-419) as the fill walks: kBiasAbove on every visit
/// but the first, never kIgnoreVirtualAbove.  Returns false when there is no candidate.
__device__ inline bool hmSupportingVoxelFill(const HeightmapArgs &a, HmCursor &c, const int seed[3], bool bias_above,
                                             int &candidate)
{
  const int min_up = sel3(a.up, a.min_g), max_up = sel3(a.up, a.max_g);
  const int down_to = a.up_positive ? min_up : max_up;
  const int up_to = a.up_positive ? max_up : min_up;
  int below = 0, above = 0;
  bool virtual_below = false, virtual_above = false;
  const int offset_below = hmSearch(a, c, seed, down_to, a.voxel_floor, false, below, virtual_below);
  const int offset_above = hmSearch(a, c, seed, up_to, a.voxel_ceiling, true, above, virtual_above);
  const bool have_below = offset_below >= 0;
  const bool have_above = offset_above >= 0;
  virtual_below = have_below && virtual_below && !(a.flags & kHmPromoteVirtualBelow);
  bool take_below;
  if (bias_above && have_below && have_above)
  {
    take_below = offset_below < offset_above;  // :367-373 the closer one, the one above on a tie
  }
  else if (have_below && virtual_above && !virtual_below)
  {
    take_below = true;
  }
  else if (have_above && !virtual_above && virtual_below)
  {
    take_below = false;
  }
  else
  {
    take_below = have_below && (!have_above || offset_below <= offset_above ||
                                (!virtual_above && offset_below + offset_above >= a.clearance_permissive));
  }
  candidate = take_below ? below : above;
  return take_below ? have_below : have_above;
}

// The functions below are the ground search and the cell value of k_heightmap_columns, statement for statement.  They
// are written out a second time because that kernel's machine code is held fixed (scripts/kernel_fingerprint.py) and
// it keeps them in its body; calling its hmSubVoxelCoord from a second place changed how the compiler inlines it there
// (6232 -> 6253 instructions), hence the copy of that one too.

/// Rule 4, findGround (:422-512) from `candidate` up the column of `walk`.  False when the column has no ground.
__device__ inline bool hmGround(const HeightmapArgs &a, HmCursor &c, const int walk[3], int candidate,
                                const double up_vec[3], int &ground_up, double &clearance, bool &ground_observed_above)
{
  const int up = a.up;
  const int min_up = sel3(up, a.min_g), max_up = sel3(up, a.max_g);
  const int step_dir = a.up_positive ? 1 : -1;
  bool observed_above = false;
  double column_height = 1.7976931348623157e308;
  double column_clearance_height = column_height;
  int candidate_type = kOtNull;
  int last_type = kOtNull;
  int key[3] = { walk[0], walk[1], walk[2] };
  for (int key_up = candidate; key_up >= min_up && key_up <= max_up; key_up += step_dir)
  {
    hmPut(key, up, key_up);
    const int voxel_type = hmType(a, c, key);
    const bool last_is_unobserved = last_type == kOtUnobserved || last_type == kOtNull;
    observed_above = observed_above || (voxel_type != kOtNull && voxel_type != kOtUnobserved);
    if (voxel_type == kOtOccupied ||
        (a.generate_virtual && last_is_unobserved && voxel_type == kOtFree && candidate_type == kOtNull))
    {
      // sourceVoxelHeight (:167-184): the mean position for occupied voxels, the centre otherwise
      double pos[3];
      hmPosition(a, c, key, hmSeek(a, c, key), voxel_type == kOtOccupied, pos);
      const double height = hmDot(pos, up_vec);
      if (candidate_type != kOtNull)
      {
        column_clearance_height = height;
        if (column_clearance_height - column_height >= a.min_clearance)
        {
          break;
        }
      }
      column_height = column_clearance_height = height;
      ground_up = key_up;
      candidate_type = voxel_type;
      observed_above = false;
    }
    last_type = voxel_type;
  }
  if (candidate_type == kOtNull)
  {
    return false;
  }
  clearance = column_clearance_height - column_height;
  ground_observed_above = observed_above;
  return true;
}

/// subVoxelCoord (ohm/VoxelMeanCompute.h:69-92), as hmSubVoxelCoord.
__device__ inline uint32_t hmFillSubVoxelCoord(const double v[3], double resolution)
{
  const int mean_positions = (1 << 10) - 1;
  const double mean_resolution = resolution / double(mean_positions);
  const double offset = double(0.5f) * resolution;
  uint32_t pattern = 0;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis)
  {
    int pos = pointToRegionCoord(v[axis] + offset, mean_resolution);
    pos = (pos >= 0 ? (pos < (1 << 10) ? pos : mean_positions) : 0);
    pattern |= uint32_t(pos) << (10 * axis);
  }
  return pattern | (1u << 31);
}

constexpr long long kHmCellOutside = -2;  ///< hmCellRecord: the cell is not in the dense grid (cannot happen)

/// Rule 5 (Heightmap.cpp:619-671, addSurfaceVoxel :703-835) for ground voxel `ground`: writes the cell's value into
/// record `rec` of rec_occ / rec_vox / rec_mean and returns the dense index of the heightmap cell; kHmNoCell when the
/// voxel writes nothing.
__device__ inline long long hmCellRecord(const HeightmapArgs &a, HmCursor &c, const int ground[3], bool have_candidate,
                                         bool have_ground, double clearance, bool ground_observed_above,
                                         const double up_vec[3], size_t rec)
{
  const int up = a.up;
  const int voxel_type = have_candidate ? hmType(a, c, ground) : int(kOtNull);
  if (!(voxel_type == kOtOccupied || (voxel_type == kOtFree && a.generate_virtual)))
  {
    return kHmNoCell;
  }
  const int vi = hmSeek(a, c, ground);
  double pos[3];
  hmPosition(a, c, ground, vi, voxel_type == kOtOccupied, pos);
  const double src_height = hmDot(up_vec, pos);
  hmPut(pos, up, 0.0);
  int hr[3], hl[3];
  const bool ok = voxelKey(a.hm, pos, hr, hl);
  hmPut(hr, up, 0);
  hmPut(hl, up, 0);
  const int ca = sel3(a.a, hr) * sel3(a.a, a.hm.kdim) + sel3(a.a, hl) - a.cell0_a;
  const int cb = sel3(a.b, hr) * sel3(a.b, a.hm.kdim) + sel3(a.b, hl) - a.cell0_b;
  if (!(ok && ca >= 0 && ca < a.ma && cb >= 0 && cb < a.mb))
  {
    return kHmCellOutside;
  }
  double centre[3];
#pragma unroll
  for (int axis = 0; axis < 3; ++axis)
  {
    centre[axis] = voxelCentreAxis(a.hm, axis, hr[axis], hl[axis]);
  }
  const float height = float(src_height - hmDot(centre, up_vec));
  uint32_t samples = 0;
  if (c.mean)
  {
    samples = min(c.mean[vi].y, 0xffffu);
    const double rel[3] = { pos[0] - centre[0], pos[1] - centre[1], pos[2] - centre[2] };
    a.rec_mean[rec] = make_uint2(hmFillSubVoxelCoord(rel, a.hm.resolution), 1u);
  }
  a.rec_occ[rec] = (voxel_type == kOtOccupied) ? 1.0f : -1.0f;
  uint32_t *vox = a.rec_vox + rec * kHmVoxelWords;
  vox[0] = __float_as_uint(height);
  vox[1] = __float_as_uint(float(clearance));
  hmSurfaceNormal(a, c, vi, voxel_type == kOtOccupied, up_vec, vox);
  // layer kHvlBaseLayer (0) | flags << 8 | contributing_samples << 16
  vox[5] = ((have_ground && ground_observed_above) ? 0x100u : 0u) | (samples << 16);
  return (long long)(size_t(cb) * size_t(a.ma) + size_t(ca));
}

/// Neighbour slot k (0 .. 7) of PlaneFillWalker::visit's loops, row_delta on b outer, col_delta on a inner, self skipped.
__device__ inline void hmFillSlotDelta(int k, int &col_delta, int &row_delta)
{
  const int at = k + (k >= 4 ? 1 : 0);
  row_delta = at / 3 - 1;
  col_delta = at % 3 - 1;
}

/// Every cell cleared: occupancy +inf, zeros, no visit.
__global__ void __launch_bounds__(256) k_hmfill_clear(HeightmapFillArgs f)
{
  const size_t cell = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (cell < size_t(f.ma) * size_t(f.mb))
  {
    f.out_occ[cell] = __int_as_float(0x7f800000);
    uint32_t *vox = f.out_vox + cell * kHmVoxelWords;
#pragma unroll
    for (uint32_t i = 0; i < kHmVoxelWords; ++i)
    {
      vox[i] = 0u;
    }
    if (f.out_mean)
    {
      f.out_mean[cell] = make_uint2(0u, 0u);
    }
    f.cell_visit[cell] = 0u;
  }
}

__global__ void __launch_bounds__(64) k_hmfill_columns(HeightmapFillArgs f)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  bool wrote = false;
  HmCursor c;
  c.tx = 0x7fffffff;
  c.ty = c.tz = 0;
  c.occ = nullptr;
  c.mean = nullptr;
  c.rx = 0x7fffffff;
  c.ry = c.rz = 0;
  c.region_exists = false;
  c.inspected = 0;
  if (i < f.gen_count)
  {
    const uint32_t n = f.gen_count;
    const uint2 item = f.queue[size_t(f.gen_begin) + i];
    const int ia = int(item.x % uint32_t(f.na));
    const int ib = int(item.x / uint32_t(f.na));
    const int up = f.up;
    double up_vec[3] = { 0.0, 0.0, 0.0 };
    hmPut(up_vec, up, f.up_positive ? 1.0 : -1.0);
    const int min_up = sel3(up, f.min_g);
    int walk[3] = { 0, 0, 0 };
    hmPut(walk, f.a, sel3(f.a, f.min_g) + ia);
    hmPut(walk, f.b, sel3(f.b, f.min_g) + ib);
    hmPut(walk, up, min_up + int(item.y));
    int candidate = 0;
    const bool have_candidate = hmSupportingVoxelFill(f, c, walk, f.gen_begin + i != 0u, candidate);
    double clearance = 0.0;
    int ground_up = 0;
    bool ground_observed_above = false;
    const bool have_ground =
      have_candidate && hmGround(f, c, walk, candidate, up_vec, ground_up, clearance, ground_observed_above);
    int ground[3] = { walk[0], walk[1], walk[2] };
    if (have_ground)
    {
      hmPut(ground, up, ground_up);
    }
    f.ground_h[i] = uint32_t(sel3(up, ground) - min_up);
    const long long cell =
      hmCellRecord(f, c, ground, have_candidate, have_ground, clearance, ground_observed_above, up_vec, size_t(i));
    f.rec_cell[i] = (cell >= 0) ? uint32_t(cell) : kHmFillNoCell;
    if (cell >= 0)
    {
      atomicMax(&f.cell_visit[cell], f.gen_begin + i + 1u);
      wrote = true;
    }
    else if (cell == kHmCellOutside)
    {
      atomicAdd(&f.counts[2], 1ull);
    }
    // F4 / F5: this key's events
    const unsigned long long none = (unsigned long long)f.grid_cells << f.index_bits;
    f.keys[i] = f.seed_generation ? none : (((unsigned long long)item.x << f.index_bits) | i);
#pragma unroll
    for (int k = 0; k < 8; ++k)
    {
      int col_delta, row_delta;
      hmFillSlotDelta(k, col_delta, row_delta);
      const int na = ia + col_delta, nb = ib + row_delta;
      const bool on_grid = na >= 0 && na < f.na && nb >= 0 && nb < f.nb;
      const unsigned long long to = (unsigned long long)(uint32_t(nb) * uint32_t(f.na) + uint32_t(na));
      f.keys[size_t(1 + k) * n + i] = on_grid ? ((to << f.index_bits) | i) : none;
      f.accept[size_t(8) * i + uint32_t(k)] = 0u;
    }
    if (i == 0u)
    {
      f.accept[size_t(8) * n] = 0u;
    }
  }
  const unsigned long long wrote_mask = __ballot(wrote);
  if (threadIdx.x == 0u && wrote_mask)
  {
    atomicAdd(&f.counts[0], (unsigned long long)__popcll(wrote_mask));
  }
  if (f.count_inspected && c.inspected)
  {
    atomicAdd(&f.counts[3], (unsigned long long)c.inspected);
  }
}

__global__ void __launch_bounds__(256) k_hmfill_replay(HeightmapFillArgs f)
{
  const size_t p = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t n = f.gen_count;
  const size_t events = 9 * n;
  if (p >= events)
  {
    return;
  }
  const unsigned long long index_mask = (1ull << f.index_bits) - 1ull;
  const uint32_t cell = uint32_t(f.sorted[p] >> f.index_bits);
  if (cell < f.grid_cells && (p == 0 || uint32_t(f.sorted[p - 1] >> f.index_bits) != cell))
  {
    const int ca = int(cell % uint32_t(f.na)), cb = int(cell / uint32_t(f.na));
    int value = f.grid[cell];
    uint32_t revisits = 0;
    for (size_t q = p; q < events; ++q)
    {
      const unsigned long long key = f.sorted[q];
      if (uint32_t(key >> f.index_bits) != cell)
      {
        break;
      }
      const uint32_t i = uint32_t(key & index_mask);
      const uint2 item = f.queue[size_t(f.gen_begin) + i];
      if (item.x == cell)
      {
        value = int(item.y);  // F5: the pop sets the cell, also to a greater height
        continue;
      }
      const int offered = int(f.ground_h[i]);
      if (value < 0 || offered < value)  // F4: Revisit::kLower
      {
        const int col_delta = ca - int(item.x % uint32_t(f.na)), row_delta = cb - int(item.x / uint32_t(f.na));
        const int at = (row_delta + 1) * 3 + (col_delta + 1);
        f.accept[size_t(8) * i + uint32_t(at > 4 ? at - 1 : at)] = 1u;
        revisits += (value >= 0) ? 1u : 0u;
        value = offered;
      }
    }
    f.grid[cell] = value;
    if (revisits)
    {
      atomicAdd(&f.counts[4], (unsigned long long)revisits);
    }
  }
  // F6: key p of the generation writes its heightmap cell when no later visit so far does
  if (p < n)
  {
    const uint32_t to = f.rec_cell[p];
    if (to != kHmFillNoCell && f.cell_visit[to] == f.gen_begin + uint32_t(p) + 1u)
    {
      f.out_occ[to] = f.rec_occ[p];
      uint32_t *vox = f.out_vox + size_t(to) * kHmVoxelWords;
#pragma unroll
      for (uint32_t w = 0; w < kHmVoxelWords; ++w)
      {
        vox[w] = f.rec_vox[p * kHmVoxelWords + w];
      }
      if (f.out_mean && f.use_mean)
      {
        f.out_mean[to] = f.rec_mean[p];
      }
    }
  }
}

__global__ void __launch_bounds__(256) k_hmfill_append(HeightmapFillArgs f)
{
  const size_t j = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (j < size_t(8) * f.gen_count && f.accept[j])
  {
    const uint32_t i = uint32_t(j >> 3);
    const uint2 item = f.queue[size_t(f.gen_begin) + i];
    int col_delta, row_delta;
    hmFillSlotDelta(int(j & 7u), col_delta, row_delta);
    const uint32_t to = uint32_t(int(item.x) + row_delta * f.na + col_delta);
    f.queue[size_t(f.gen_begin) + f.gen_count + f.accept_at[j]] = make_uint2(to, f.ground_h[i]);
  }
}

/// After the last generation: source_visit and the count of cells that hold a value; the visit log.
__global__ void __launch_bounds__(256) k_hmfill_finish(HeightmapFillArgs f)
{
  const size_t at = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  bool written = false;
  if (at < size_t(f.ma) * size_t(f.mb))
  {
    const uint32_t v = f.cell_visit[at];
    written = v != 0u;
    if (f.out_visit)
    {
      f.out_visit[at] = v - 1u;  // none: 0xffffffff
    }
  }
  const unsigned long long mask = __ballot(written);
  if ((threadIdx.x & 63u) == 0u && mask)
  {
    atomicAdd(&f.counts[1], (unsigned long long)__popcll(mask));
  }
  if (f.out_log && at < size_t(f.log_count))
  {
    const uint2 item = f.queue[at];
    f.out_log[3 * at + 0] = item.x % uint32_t(f.na);
    f.out_log[3 * at + 1] = item.x / uint32_t(f.na);
    f.out_log[3 * at + 2] = item.y;
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_HEIGHTMAP_FILL_KERNELS_H
