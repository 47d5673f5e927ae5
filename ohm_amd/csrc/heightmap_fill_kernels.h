// heightmap_fill_kernels.h -- the flood-fill heightmap (ohm::Heightmap::buildHeightmap, HeightmapMode::kSimpleFill)
// built on the device from the resident map, read only.  Rules F1-F6 of include/ohmhip.h ("HEIGHTMAP, FLOOD FILL").
//
// The walk -- queue, generations, the round of kernels per generation -- is heightmap_walk_kernels.h's.  The fill's own:
//
//   k_hmfill_columns  1 lane / key of the generation   F3, F6: the walk's column evaluation; atomicMax of the visit
//                                                      number per heightmap cell; the key's pop as its event of its own
//   k_hmfill_replay   1 lane / sorted event            the first event of a cell replays the cell's events in order --
//                                                      F5 a pop sets the cell, F4 an offer is accepted when the cell is
//                                                      unvisited or the offer lower -- and flags the accepted offers;
//                                                      lanes below the generation's size also commit their key's cell
//                                                      value when it is the cell's winner so far
//
// Exactness.  grid[c] is read and written only by pops of keys at c and by offers to c.  Key i of a generation adds at
// most one event to cell c: its pop when it sits at c, else one offer when c is one of its 8 neighbours.  In the
// reference key i is popped, then makes its offers in slot order, then key i + 1 is popped: the events of one cell,
// ordered by i, are in the reference's order, and nothing else a decision depends on is shared between cells.
// Generations run in order on one stream, so the winner of a heightmap cell -- the largest visit number -- may be
// committed per generation: a later generation overwrites.
#ifndef OHMHIP_HEIGHTMAP_FILL_KERNELS_H
#define OHMHIP_HEIGHTMAP_FILL_KERNELS_H

#include "heightmap_walk_kernels.h"

namespace ohmhip
{
/// Event ids: a grid cell, grid_cells for "no event".
struct HeightmapFillArgs : HeightmapWalkArgs
{
  int *grid;             ///< [na * nb] PlaneFillWalker::Visit::height, -1: unvisited
  uint32_t *cell_visit;  ///< [ma * mb] 1 + the largest visit number that wrote the cell, 0: none
  uint32_t *out_visit;   ///< null: not requested
};

/// Every cell cleared, no visit.
__global__ void __launch_bounds__(256) k_hmfill_clear(HeightmapFillArgs f)
{
  const size_t cell = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (cell < size_t(f.ma) * size_t(f.mb))
  {
    hmWalkClearCell(f, cell);
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
    const HmWalkColumn col = hmWalkColumn(f, c, i);
    if (col.cell >= 0)
    {
      atomicMax(&f.cell_visit[col.cell], f.gen_begin + i + 1u);
      wrote = true;
    }
    // F4 / F5: this key's events; the seed is not popped
    const unsigned long long none = (unsigned long long)f.grid_cells << f.index_bits;
    f.keys[i] = f.seed_generation ? none : (((unsigned long long)col.at << f.index_bits) | i);
    hmWalkOffers(f, i, col.ia, col.ib, none);
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
  if (cell < f.grid_cells && hmWalkFirstOf(f, p, cell))
  {
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
        f.accept[size_t(8) * i + hmWalkSlotOf(f, cell, item.x)] = 1u;
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
  hmWalkLogEntry(f, at);
}
}  // namespace ohmhip

#endif  // OHMHIP_HEIGHTMAP_FILL_KERNELS_H
