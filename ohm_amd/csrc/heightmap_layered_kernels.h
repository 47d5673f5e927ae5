// heightmap_layered_kernels.h -- the layered heightmaps (ohm::Heightmap::buildHeightmap, HeightmapMode::kLayeredFill and
// kLayeredFillUnordered) built on the device from the resident map, read only.  Rules L1-L7 of include/ohmhip.h
// ("HEIGHTMAP, LAYERED").
//
// The walk -- queue, generations, the round of kernels per generation -- is heightmap_walk_kernels.h's.  The layered
// builds' own is what a generation's keys share:
//
//   k_hml_columns  1 lane / key of the generation   L2, L4: the walk's column evaluation; the key's flags and fp64
//                                                   src_height; its add keyed (heightmap cell, key index) as its event
//                                                   of its own, sorted behind the offers' grid cells
//   k_hml_offers   1 lane / sorted event            L3: the first offer of a grid cell replays the cell's offers in order
//                                                   against the cell's touched list -- a head per cell, (height, next)
//                                                   nodes in one pool -- and flags the accepted ones
//   k_hml_adds     1 lane / sorted event            L5: the first add of a heightmap cell applies the cell's adds in order
//                                                   to the column's slots
//
// Exactness.  The fill's argument (heightmap_fill_kernels.h) carries over to two independent per-cell orders.  A touched
// list is read and written only by offers to its grid cell, and key i of a generation makes at most one offer to a cell;
// a column of slots is read and written only by adds to its heightmap cell, and key i makes at most one add.  In the
// reference key i makes its offers, then its add, then key i + 1 follows: the events of one cell ordered by i are in the
// reference's order, and neither decision reads what the other writes.  Generations run in order on one stream, so lists
// and slots carry over.
//
// The slots are planes [slot][cell] of the walk's own, not the caller's: a column may need more slots than the caller
// asked for, and L7 permutes them.  When the adds of one cell could outgrow the planes the cell's lane applies none of
// them and raises the capacity asked for in a word the host reads with the generation's size; the host grows the planes
// and runs k_hml_adds again, which skips the cells whose adds it has applied (a stamp per cell).
//
//   k_hml_keys, (radix sort), k_hml_filter          L6: the ground keys of the voxels that stood, sorted; 1 lane / slot
//                                                   counts a virtual voxel's 26 neighbours by binary search
//   k_hml_finish   1 lane / heightmap cell          L7 and the results: ranks by counting (slots^2 reads, no array in
//                                                   registers indexed at run time), the base layer, the caller's planes,
//                                                   layer_count, the counts; the visit log
#ifndef OHMHIP_HEIGHTMAP_LAYERED_KERNELS_H
#define OHMHIP_HEIGHTMAP_LAYERED_KERNELS_H

#include "heightmap_walk_kernels.h"

namespace ohmhip
{
enum : uint32_t
{
  kHvlBaseLayer = 0,  ///< HeightmapVoxelLayer (ohmheightmap/HeightmapVoxel.h:17-28)
  kHvlExtended = 1,
  kHvlInvalid = 2
};

enum : uint32_t
{
  kHmlNullCandidate = 1u << 0,  ///< the visit found no candidate: L3's column rule
  kHmlBaseCandidate = 1u << 1   ///< L4
};

enum : int  ///< counts[] beyond HeightmapArgs' [0] populated [2] outside [3] inspected
{
  kHmlRepeats = 4,
  kHmlTooClose = 5,
  kHmlFiltered = 6,
  kHmlMultiColumns = 7,
  kHmlCells = 8,
  kHmlVoxels = 9,
  kHmlLayers = 10,
  kHmlCountWords = 12
};

/// Event ids: a grid cell, grid_cells + a heightmap cell, grid_cells + hm_cells for "no event".
struct HeightmapLayeredArgs : HeightmapWalkArgs
{
  uint32_t hm_cells;           ///< ma * mb
  uint32_t stamp;              ///< 1 + the generation's number
  int ordered;                 ///< kLayeredFill
  uint32_t filter_threshold;   ///< L6, 0: off
  double epsilon;              ///< haveRecordedHeight: 1e-3 * grid_resolution
  double seed_height;          ///< dot(up, reference_pos)
  // per key of the generation
  uint32_t *key_flags;         ///< kHml*Candidate
  double *src_height;          ///< rule 5's src_height, valid where rec_cell is a cell
  // the walker's touched lists (PlaneFillLayeredWalker.h)
  uint32_t *touched_head;      ///< [grid_cells] 1 + index of the cell's first node, 0: none
  uint2 *nodes;                ///< (height, next)
  uint32_t node_capacity;
  uint32_t *words;             ///< [0] nodes taken [1] slots a column asked for beyond slot_capacity, else 0
  // the heightmap's columns
  uint32_t slot_capacity;
  uint32_t *slot_count;        ///< [hm_cells] slots in use
  uint32_t *applied;           ///< [hm_cells] stamp of the last generation whose adds the cell took
  uint32_t *multi;             ///< [hm_cells] L5: noted as multi-layered
  float *sl_occ;               ///< [slot_capacity][hm_cells]
  uint32_t *sl_vox;            ///< [slot_capacity][hm_cells][6]
  uint2 *sl_mean;
  uint32_t *sl_visit;          ///< sequence number of the visit that added the voxel
  unsigned long long *sl_ground;  ///< its ground key: grid cell << 32 | height offset
  const unsigned long long *ground_sorted;  ///< L6: every sl_ground in use, sorted; ~0 for the others
  // results: layer_capacity planes
  uint32_t layer_capacity;
  uint8_t *out_count;          ///< null: not requested
  uint32_t *out_source;        ///< null: not requested
};

/// dot(voxelCentreGlobal(key of slot `slot`), up): the cell's key moved `slot` steps along the raw up axis is region
/// `slot`, local 0 there (the heightmap's regions are one voxel high), and the other two terms of the dot are zeros.
__device__ inline double hmlSlotCentreHeight(const HeightmapLayeredArgs &f, uint32_t slot)
{
  const double centre = voxelCentreAxis(f.hm, f.up, int(slot), 0);
  return f.up_positive ? centre : -centre;
}

/// DstVoxel::setPosition for slot `slot` > 0: rule 5's coord was taken against slot 0's centre; only its up field moves.
__device__ inline uint32_t hmlSlotMeanCoord(const HeightmapLayeredArgs &f, uint32_t coord, uint32_t slot)
{
  double rel[3] = { 0.0, 0.0, 0.0 };
  hmPut(rel, f.up, 0.0 - voxelCentreAxis(f.hm, f.up, int(slot), 0));
  const uint32_t field = 0x3ffu << (10 * f.up);
  return (coord & ~field) | (hmSubVoxelCoord(rel, f.hm.resolution) & field);
}

__global__ void __launch_bounds__(256) k_hml_clear(HeightmapLayeredArgs f)
{
  const size_t at = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (at < size_t(f.hm_cells))
  {
    f.slot_count[at] = 0u;
    f.applied[at] = 0u;
    f.multi[at] = 0u;
  }
  if (at < size_t(f.grid_cells))
  {
    f.touched_head[at] = 0u;
  }
  if (at < 2)
  {
    f.words[at] = 0u;
  }
  if (at < size_t(kHmlCountWords))
  {
    f.counts[at] = 0ull;
  }
}

__global__ void __launch_bounds__(64) k_hml_columns(HeightmapLayeredArgs f)
{
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  HmCursor c = hmCursorStart();
  if (i < f.gen_count)
  {
    const HmWalkColumn col = hmWalkColumn(f, c, i);
    f.key_flags[i] =
      (col.have_candidate ? 0u : uint32_t(kHmlNullCandidate)) |
      ((col.have_ground && (col.clearance > 0.0 || col.ground_observed_above)) ? uint32_t(kHmlBaseCandidate) : 0u);
    if (col.cell >= 0)
    {
      // rule 5's src_height once more, in fp64: hmCellRecord keeps it as the float relative to slot 0
      double pos[3];
      hmPosition(f, c, col.ground, hmSeek(f, c, col.ground), f.rec_occ[i] > 0.0f, pos);
      f.src_height[i] = hmDot(col.up_vec, pos);
    }
    const unsigned long long none = ((unsigned long long)f.grid_cells + f.hm_cells) << f.index_bits;
    const unsigned long long add = (unsigned long long)f.grid_cells + (unsigned long long)col.cell;
    f.keys[i] = (col.cell >= 0) ? ((add << f.index_bits) | i) : none;
    hmWalkOffers(f, i, col.ia, col.ib, none);
  }
  hmColumnTail(f, c, false);
}

/// L3.  PlaneFillLayeredWalker::visit's test and touch for every offer to one grid cell, in key order.
__global__ void __launch_bounds__(256) k_hml_offers(HeightmapLayeredArgs f)
{
  const size_t p = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t events = size_t(9) * f.gen_count;
  if (p >= events)
  {
    return;
  }
  const unsigned long long index_mask = (1ull << f.index_bits) - 1ull;
  const unsigned long long id = f.sorted[p] >> f.index_bits;
  if (id >= f.grid_cells || !hmWalkFirstOf(f, p, id))
  {
    return;
  }
  const uint32_t cell = uint32_t(id);
  uint32_t head = f.touched_head[cell];
  for (size_t q = p; q < events; ++q)
  {
    const unsigned long long key = f.sorted[q];
    if ((key >> f.index_bits) != id)
    {
      break;
    }
    const uint32_t i = uint32_t(key & index_mask);
    const uint32_t offered = f.ground_h[i];
    bool touched = false;
    if (f.key_flags[i] & kHmlNullCandidate)
    {
      touched = head != 0u;  // kAddUnvisitedColumnNeighbours: hasTouched(idx)
    }
    else
    {
      for (uint32_t at = head; at != 0u && !touched;)  // kAddUnvisitedNeighbours: hasTouched(idx, height)
      {
        const uint2 node = f.nodes[at - 1u];
        touched = node.x == offered;
        at = node.y;
      }
    }
    if (!touched)
    {
      const uint32_t node = atomicAdd(&f.words[0], 1u);
      if (node >= f.node_capacity)
      {
        atomicAdd(&f.counts[2], 1ull);  // (the pool holds a node per queue entry: cannot happen)
        break;
      }
      f.nodes[node] = make_uint2(offered, head);
      head = node + 1u;
      f.accept[size_t(8) * i + hmWalkSlotOf(f, cell, f.queue[size_t(f.gen_begin) + i].x)] = 1u;
    }
  }
  f.touched_head[cell] = head;
}

/// L5.  addSurfaceVoxel's multi-layer branch for every add to one heightmap cell, in key order.
__global__ void __launch_bounds__(256) k_hml_adds(HeightmapLayeredArgs f)
{
  const size_t p = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t events = size_t(9) * f.gen_count;
  if (p >= events)
  {
    return;
  }
  const unsigned long long index_mask = (1ull << f.index_bits) - 1ull;
  const unsigned long long id = f.sorted[p] >> f.index_bits;
  const unsigned long long first_cell = f.grid_cells;
  if (id < first_cell || id >= first_cell + f.hm_cells || !hmWalkFirstOf(f, p, id))
  {
    return;
  }
  const size_t cell = size_t(id - first_cell);
  if (f.applied[cell] == f.stamp)
  {
    return;
  }
  size_t end = p + 1;
  while (end < events && (f.sorted[end] >> f.index_bits) == id)
  {
    ++end;
  }
  uint32_t n = f.slot_count[cell];
  if (size_t(n) + (end - p) > size_t(f.slot_capacity))
  {
    const size_t asked = size_t(n) + (end - p);
    atomicMax(&f.words[1], asked < 0xffffffffu ? uint32_t(asked) : 0xffffffffu);
    return;
  }
  const size_t cells = f.hm_cells;
  uint32_t stood = 0, repeats = 0, too_close = 0;
  for (size_t q = p; q < end; ++q)
  {
    const uint32_t i = uint32_t(f.sorted[q] & index_mask);
    const double src_height = f.src_height[i];
    bool add = true;
    if (n != 0u)
    {
      bool repeat = false;  // haveRecordedHeight
      for (uint32_t k = 0; k < n && !repeat; ++k)
      {
        double voxel_height = double(__uint_as_float(f.sl_vox[(size_t(k) * cells + cell) * kHmVoxelWords]));
        voxel_height += hmlSlotCentreHeight(f, k);
        repeat = fabs(voxel_height - src_height) < f.epsilon;
      }
      if (repeat)
      {
        ++repeats;
        add = false;
      }
      else
      {
        double nearest_below = 0.0, nearest_above = 0.0;  // Heightmap.cpp:754-776
        for (uint32_t k = 0; k < n; ++k)
        {
          const double current =
            double(__uint_as_float(f.sl_vox[(size_t(k) * cells + cell) * kHmVoxelWords])) + hmlSlotCentreHeight(f, k);
          const double delta = current - src_height;
          nearest_below = (delta < 0.0 && (nearest_below <= 0.0 || -delta < nearest_below)) ? -delta : nearest_below;
          nearest_above = (delta > 0.0 && (nearest_above <= 0.0 || delta < nearest_above)) ? delta : nearest_above;
        }
        if ((nearest_below > 0.0 && nearest_below <= f.min_clearance) ||
            (nearest_above > 0.0 && nearest_above <= f.min_clearance))
        {
          ++too_close;
          add = false;
        }
      }
    }
    if (!add)
    {
      continue;
    }
    const size_t to = size_t(n) * cells + cell;
    const uint32_t *rec = f.rec_vox + size_t(i) * kHmVoxelWords;
    uint32_t *vox = f.sl_vox + to * kHmVoxelWords;
    f.sl_occ[to] = f.rec_occ[i];
    vox[0] = (n == 0u) ? rec[0] : __float_as_uint(float(src_height - hmlSlotCentreHeight(f, n)));
    vox[1] = rec[1];
    vox[2] = rec[2];
    vox[3] = rec[3];
    vox[4] = rec[4];
    vox[5] = rec[5] | ((f.key_flags[i] & kHmlBaseCandidate) ? uint32_t(kHvlBaseLayer) : uint32_t(kHvlExtended));
    if (f.use_mean)
    {
      const uint2 mean = f.rec_mean[i];
      f.sl_mean[to] = make_uint2((n == 0u) ? mean.x : hmlSlotMeanCoord(f, mean.x, n), mean.y);
    }
    f.sl_visit[to] = f.gen_begin + i;
    f.sl_ground[to] = ((unsigned long long)f.queue[size_t(f.gen_begin) + i].x << 32) | f.ground_h[i];
    if (n != 0u && f.ordered && !f.multi[cell])
    {
      f.multi[cell] = 1u;
      atomicAdd(&f.counts[kHmlMultiColumns], 1ull);
    }
    ++n;
    ++stood;
  }
  f.slot_count[cell] = n;
  f.applied[cell] = f.stamp;
  if (stood)
  {
    atomicAdd(&f.counts[0], (unsigned long long)stood);
  }
  if (repeats)
  {
    atomicAdd(&f.counts[kHmlRepeats], (unsigned long long)repeats);
  }
  if (too_close)
  {
    atomicAdd(&f.counts[kHmlTooClose], (unsigned long long)too_close);
  }
}

/// L6, first half: the ground key of every slot in use as a sort key, ~0 for the others.  `keys` has slot_capacity *
/// hm_cells entries here.
__global__ void __launch_bounds__(256) k_hml_keys(HeightmapLayeredArgs f)
{
  const size_t at = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t cells = f.hm_cells;
  if (at < size_t(f.slot_capacity) * cells)
  {
    const bool in_use = uint32_t(at / cells) < f.slot_count[at % cells];
    f.keys[at] = in_use ? f.sl_ground[at] : ~0ull;
  }
}

__device__ inline bool hmlGroundKeyPresent(const HeightmapLayeredArgs &f, size_t count, unsigned long long key)
{
  size_t lo = 0, hi = count;
  while (lo < hi)
  {
    const size_t mid = lo + (hi - lo) / 2;
    if (f.ground_sorted[mid] < key)
    {
      lo = mid + 1;
    }
    else
    {
      hi = mid;
    }
  }
  return lo < count && f.ground_sorted[lo] == key;
}

/// L6, second half (filterVirtualVoxels): a virtual voxel with fewer than filter_threshold of its 26 neighbours, in the
/// source map's key space, among the ground keys becomes kHvlInvalid.  Of two voxels of one ground key -- they share a
/// column -- only the earlier one is in the reference's map.
__global__ void __launch_bounds__(256) k_hml_filter(HeightmapLayeredArgs f)
{
  const size_t at = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t cells = f.hm_cells;
  const size_t total = size_t(f.slot_capacity) * cells;
  if (at >= total)
  {
    return;
  }
  const size_t cell = at % cells;
  const uint32_t n = f.slot_count[cell];
  if (uint32_t(at / cells) >= n || f.sl_occ[at] != -1.0f)
  {
    return;
  }
  const unsigned long long key = f.sl_ground[at];
  const uint32_t visit = f.sl_visit[at];
  for (uint32_t k = 0; k < n; ++k)
  {
    const size_t other = size_t(k) * cells + cell;
    if (other != at && f.sl_ground[other] == key && f.sl_visit[other] < visit)
    {
      return;
    }
  }
  const uint32_t from = uint32_t(key >> 32);
  const int ia = int(from % uint32_t(f.na)), ib = int(from / uint32_t(f.na));
  const long long h = (long long)(key & 0xffffffffull);
  uint32_t present = 0;
  for (int t = 0; t < 27; ++t)
  {
    const int da = t % 3 - 1, db = (t / 3) % 3 - 1, dh = t / 9 - 1;
    const int na = ia + da, nb = ib + db;
    const long long nh = h + dh;
    if (t == 13 || na < 0 || na >= f.na || nb < 0 || nb >= f.nb || nh < 0 || nh > 0xffffffffll)
    {
      continue;
    }
    const unsigned long long neighbour =
      ((unsigned long long)(uint32_t(nb) * uint32_t(f.na) + uint32_t(na)) << 32) | (unsigned long long)nh;
    present += hmlGroundKeyPresent(f, total, neighbour) ? 1u : 0u;
  }
  if (present < f.filter_threshold)
  {
    uint32_t *vox = f.sl_vox + at * kHmVoxelWords;
    vox[5] = (vox[5] & ~0xffu) | uint32_t(kHvlInvalid);
    f.sl_occ[at] = __int_as_float(0xff800000);  // kHeightmapVirtualSurfaceFilteredValue
    atomicAdd(&f.counts[kHmlFiltered], 1ull);
  }
}

/// One voxel into slot `slot` of the caller's planes when it is among them.
__device__ inline void hmlStore(const HeightmapLayeredArgs &f, uint32_t slot, size_t cell, size_t from, uint32_t height,
                                uint32_t layer)
{
  if (slot >= f.layer_capacity)
  {
    return;
  }
  const size_t to = size_t(slot) * f.hm_cells + cell;
  f.out_occ[to] = f.sl_occ[from];
  uint32_t *vox = f.out_vox + to * kHmVoxelWords;
  const uint32_t *src = f.sl_vox + from * kHmVoxelWords;
  vox[0] = height;
  vox[1] = src[1];
  vox[2] = src[2];
  vox[3] = src[3];
  vox[4] = src[4];
  vox[5] = (src[5] & ~0xffu) | layer;
  if (f.out_mean)
  {
    f.out_mean[to] = f.use_mean ? f.sl_mean[from] : make_uint2(0u, 0u);
  }
  if (f.out_source)
  {
    f.out_source[to] = f.sl_visit[from];
  }
}

/// L7 (finaliseLayeredHeightmap) in ordered mode, the copy in unordered mode; slots behind a column's last voxel get the
/// cleared values; the counts; the visit log.
__global__ void __launch_bounds__(256) k_hml_finish(HeightmapLayeredArgs f)
{
  const size_t cell = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t cells = f.hm_cells;
  uint32_t kept = 0;
  if (cell < cells)
  {
    const uint32_t n = f.slot_count[cell];
    if (n != 0u)
    {
      atomicMax(&f.counts[kHmlLayers], (unsigned long long)n);
    }
    if (!f.ordered)
    {
      for (uint32_t k = 0; k < n; ++k)
      {
        const size_t from = size_t(k) * cells + cell;
        hmlStore(f, k, cell, from, f.sl_vox[from * kHmVoxelWords], f.sl_vox[from * kHmVoxelWords + 5] & 0xffu);
      }
      kept = n;
    }
    else if (!f.multi[cell])
    {
      // a single-voxel column: removed when filtered, else the base layer
      if (n != 0u && (f.sl_vox[cell * kHmVoxelWords + 5] & 0xffu) != kHvlInvalid)
      {
        hmlStore(f, 0u, cell, cell, f.sl_vox[cell * kHmVoxelWords], kHvlBaseLayer);
        kept = 1u;
      }
    }
    else
    {
      const double inf = __longlong_as_double(0x7ff0000000000000ll);
      bool have_best = false, best_clear = false;
      double best_distance = 0.0;
      uint32_t best_rank = 0;
      for (uint32_t k = 0; k < n; ++k)
      {
        const size_t from = size_t(k) * cells + cell;
        const uint32_t layer = f.sl_vox[from * kHmVoxelWords + 5] & 0xffu;
        if (layer == kHvlInvalid)
        {
          continue;  // sorts behind every valid voxel and is cleared there
        }
        // getVoxelHeight of the slot the voxel sits in
        const double height = hmlSlotCentreHeight(f, k) + double(__uint_as_float(f.sl_vox[from * kHmVoxelWords]));
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j)
        {
          const size_t other = size_t(j) * cells + cell;
          const bool invalid = (f.sl_vox[other * kHmVoxelWords + 5] & 0xffu) == kHvlInvalid;
          const double other_height =
            invalid ? inf : hmlSlotCentreHeight(f, j) + double(__uint_as_float(f.sl_vox[other * kHmVoxelWords]));
          rank += (other_height < height || (other_height == height && j < k)) ? 1u : 0u;
        }
        ++kept;
        hmlStore(f, rank, cell, from, __float_as_uint(float(height - hmlSlotCentreHeight(f, rank))), kHvlExtended);
        if (layer == kHvlBaseLayer)
        {
          // isOtherCandidateBetter walked in sorted order: the least (no clearance above, distance to the seed, rank)
          const bool clear = __uint_as_float(f.sl_vox[from * kHmVoxelWords + 1]) > 0.0f ||
                             ((f.sl_vox[from * kHmVoxelWords + 5] >> 8) & 1u) != 0u;
          const double distance = fabs(height - f.seed_height);
          const bool better =
            !have_best || (!best_clear && clear) ||
            (best_clear == clear && (distance < best_distance || (distance == best_distance && rank < best_rank)));
          if (better)
          {
            have_best = true;
            best_clear = clear;
            best_distance = distance;
            best_rank = rank;
          }
        }
      }
      if (have_best && best_rank < f.layer_capacity)
      {
        uint32_t *vox = f.out_vox + (size_t(best_rank) * cells + cell) * kHmVoxelWords;
        vox[5] = (vox[5] & ~0xffu) | uint32_t(kHvlBaseLayer);
      }
    }
    for (uint32_t k = kept; k < f.layer_capacity; ++k)
    {
      const size_t to = size_t(k) * cells + cell;
      hmWalkClearCell(f, to);
      if (f.out_source)
      {
        f.out_source[to] = 0xffffffffu;
      }
    }
    if (f.out_count)
    {
      f.out_count[cell] = uint8_t(kept < 255u ? kept : 255u);
    }
    if (kept)
    {
      atomicAdd(&f.counts[kHmlVoxels], (unsigned long long)kept);
    }
  }
  const unsigned long long mask = __ballot(kept != 0u);
  if ((threadIdx.x & 63u) == 0u && mask)
  {
    atomicAdd(&f.counts[kHmlCells], (unsigned long long)__popcll(mask));
  }
  hmWalkLogEntry(f, cell);
}
}  // namespace ohmhip

#endif  // OHMHIP_HEIGHTMAP_LAYERED_KERNELS_H
