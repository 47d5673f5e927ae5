// heightmap_walk_kernels.h -- the generation walk that the flood-fill heightmap (heightmap_fill_kernels.h) and the
// layered heightmaps (heightmap_layered_kernels.h) share, device side.
//
// The reference pops one key at a time from a FIFO.  Numbered in FIFO order its visits fall into generations:
// generation 0 is the seed, generation t + 1 the keys accepted while generation t is visited, in acceptance order.  The
// queue is one device array, a generation is a range of it, and the host (heightmap_walk_impl.h) launches one round per
// generation:
//
//   the build's columns kernel  1 lane / key    hmWalkColumn: supporting voxel, ground, the cell record (the device
//                                               functions of heightmap_kernels.h); what the build does with the cell and
//                                               its one event key of its own; hmWalkOffers: the key's 8 offers
//   (radix sort)                                the 9 events per key by (event id, key index)
//   the build's event kernels   1 lane / event  the first event of an id (hmWalkFirstOf) replays the id's events in key
//                                               order and flags the accepted offers (hmWalkSlotOf)
//   (exclusive scan)                            of the accept flags in (key index, neighbour slot) order
//   k_hmwalk_append             1 lane / offer  accepted offers become the next generation, behind this one
//
// and after the last generation the build's finish kernel, which also writes the visit log (hmWalkLogEntry).
//
// A walking build supplies: an argument struct derived from HeightmapWalkArgs, a columns kernel made of hmCursorStart,
// hmWalkColumn, its own lines, hmWalkOffers and hmColumnTail, event kernels that set `accept`, and a finish kernel.
#ifndef OHMHIP_HEIGHTMAP_WALK_KERNELS_H
#define OHMHIP_HEIGHTMAP_WALK_KERNELS_H

#include "heightmap_kernels.h"

namespace ohmhip
{
constexpr uint32_t kHmFillNoCell = 0xffffffffu;

/// What a generation's kernels share.  `winner` and `out_col` are not used; rec_* hold one record per key of the
/// generation.  An event id is a grid cell or whatever the build puts behind the grid cells.
struct HeightmapWalkArgs : HeightmapArgs
{
  uint2 *queue;              ///< every visit in sequence order: (grid cell ib * na + ia, height offset h)
  uint32_t gen_begin;        ///< the generation: queue[gen_begin .. gen_begin + gen_count)
  uint32_t gen_count;
  int seed_generation;       ///< generation 0
  unsigned index_bits;       ///< sort key: event id << index_bits | key index in the generation
  uint32_t grid_cells;       ///< na * nb
  uint32_t *ground_h;        ///< [gen_count] hg of each key
  uint32_t *rec_cell;        ///< [gen_count] the heightmap cell the key writes, kHmFillNoCell: none
  unsigned long long *keys;  ///< [9 * gen_count] events, slot-major: [0] the build's own, [1 + k] the offer through slot k
  const unsigned long long *sorted;
  uint32_t *accept;          ///< [8 * gen_count + 1] accept flag of offer (i, k) at 8 * i + k; the last one is 0
  const uint32_t *accept_at; ///< its exclusive scan
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

/// Its inverse: the slot through which grid cell `from` offers to its neighbour `to`.
__device__ inline uint32_t hmWalkSlotOf(const HeightmapWalkArgs &f, uint32_t to, uint32_t from)
{
  const int col_delta = int(to % uint32_t(f.na)) - int(from % uint32_t(f.na));
  const int row_delta = int(to / uint32_t(f.na)) - int(from / uint32_t(f.na));
  const int at = (row_delta + 1) * 3 + (col_delta + 1);
  return uint32_t(at > 4 ? at - 1 : at);
}

/// Sorted event p is the first one of event id `id`: its lane replays the id's events.
__device__ inline bool hmWalkFirstOf(const HeightmapWalkArgs &f, size_t p, unsigned long long id)
{
  return p == 0 || (f.sorted[p - 1] >> f.index_bits) != id;
}

/// Key i of the generation evaluated: rules F3 / L2 and the cell record.
struct HmWalkColumn
{
  uint32_t at;      ///< the key's grid cell: ib * na + ia
  int ia, ib;
  int ground[3];    ///< the ground key; the walk key when there is no ground
  double up_vec[3];
  double clearance;
  bool have_candidate, have_ground, ground_observed_above;
  long long cell;   ///< hmCellRecord's answer: record i of rec_* holds the value when >= 0
};

/// Evaluates key i: writes ground_h[i], rec_cell[i], record i of rec_* and the outside-the-grid count.
__device__ inline HmWalkColumn hmWalkColumn(const HeightmapWalkArgs &f, HmCursor &c, uint32_t i)
{
  HmWalkColumn col;
  const uint2 item = f.queue[size_t(f.gen_begin) + i];
  col.at = item.x;
  col.ia = int(item.x % uint32_t(f.na));
  col.ib = int(item.x / uint32_t(f.na));
  const int up = f.up;
  col.up_vec[0] = col.up_vec[1] = col.up_vec[2] = 0.0;
  hmPut(col.up_vec, up, f.up_positive ? 1.0 : -1.0);
  const int min_up = sel3(up, f.min_g);
  int walk[3] = { 0, 0, 0 };
  hmPut(walk, f.a, sel3(f.a, f.min_g) + col.ia);
  hmPut(walk, f.b, sel3(f.b, f.min_g) + col.ib);
  hmPut(walk, up, min_up + int(item.y));
  int candidate = 0;
  col.have_candidate = hmSupportingVoxel(f, c, walk, f.gen_begin + i != 0u, false, candidate);
  col.clearance = 0.0;
  int ground_up = 0;
  col.ground_observed_above = false;
  col.have_ground = col.have_candidate &&
                    hmGround(f, c, walk, candidate, col.up_vec, ground_up, col.clearance, col.ground_observed_above);
  col.ground[0] = walk[0], col.ground[1] = walk[1], col.ground[2] = walk[2];
  if (col.have_ground)
  {
    hmPut(col.ground, up, ground_up);
  }
  f.ground_h[i] = uint32_t(sel3(up, col.ground) - min_up);
  col.cell = hmCellRecord(f, c, col.ground, col.have_candidate, col.have_ground, col.clearance,
                          col.ground_observed_above, col.up_vec, size_t(i));
  f.rec_cell[i] = (col.cell >= 0) ? uint32_t(col.cell) : kHmFillNoCell;
  if (col.cell == kHmCellOutside)
  {
    atomicAdd(&f.counts[2], 1ull);
  }
  return col;
}

/// The 8 offers of key i at grid cell (ia, ib) in slot order, `none` for those that leave the grid; the key's accept
/// flags cleared, and by key 0 the sentinel behind the last flag.
__device__ inline void hmWalkOffers(const HeightmapWalkArgs &f, uint32_t i, int ia, int ib, unsigned long long none)
{
  const uint32_t n = f.gen_count;
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

/// Output cell `to` cleared: occupancy +inf, zeros.
__device__ inline void hmWalkClearCell(const HeightmapArgs &a, size_t to)
{
  a.out_occ[to] = __int_as_float(0x7f800000);
  uint32_t *vox = a.out_vox + to * kHmVoxelWords;
#pragma unroll
  for (uint32_t w = 0; w < kHmVoxelWords; ++w)
  {
    vox[w] = 0u;
  }
  if (a.out_mean)
  {
    a.out_mean[to] = make_uint2(0u, 0u);
  }
}

/// Visit `at` into the log when it is among the visits asked for: (ia, ib, height offset).
__device__ inline void hmWalkLogEntry(const HeightmapWalkArgs &f, size_t at)
{
  if (f.out_log && at < size_t(f.log_count))
  {
    const uint2 item = f.queue[at];
    f.out_log[3 * at + 0] = item.x % uint32_t(f.na);
    f.out_log[3 * at + 1] = item.x / uint32_t(f.na);
    f.out_log[3 * at + 2] = item.y;
  }
}

__global__ void __launch_bounds__(256) k_hmwalk_append(HeightmapWalkArgs f)
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
}  // namespace ohmhip

#endif  // OHMHIP_HEIGHTMAP_WALK_KERNELS_H
