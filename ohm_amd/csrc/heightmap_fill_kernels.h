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
  HmCursor c = hmCursorStart();
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
    const bool have_candidate = hmSupportingVoxel(f, c, walk, f.gen_begin + i != 0u, false, candidate);
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
  hmColumnTail(f, c, wrote);
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
