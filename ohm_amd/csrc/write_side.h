// write_side.h -- what the host code of the features that write voxels into the resident pool from outside the ray
// pipeline shares (region_io.h: ohmhip_map_write_regions; copy_impl.h; voxel_edit_impl.h; ohmhip_map_mark_dirty): which
// layer defines a map's replay mask, the naming of the tiles a call writes, and the marks a write leaves.  The mask rule
// itself is replayMaskBit (replay_kernels.h).  Included in ohmhip_map.hip's translation unit after tiling_impl.h and
// ahead of region_io.h: not a stand-alone header.  DESIGN.md 5c says what a new writer calls, and in what order.
#ifndef OHMHIP_WRITE_SIDE_H
#define OHMHIP_WRITE_SIDE_H

namespace
{
/// The kind for which a write to `layer_id` defines this map's "ordered replay" mask: the mean on an NDT map, the TSDF
/// layer on a TSDF map, where the map holds that layer.  The only place that maps (mode, layer) to a kind.
ReplayMaskKind replayMaskKind(ohmhip_map_t m, int layer_id)
{
  const int mode = m->config.mode;
  if (!m->pool.layers[layer_id])
  {
    return kReplayMaskNone;
  }
  if ((mode == OHMHIP_MODE_NDT_OM || mode == OHMHIP_MODE_NDT_TM) && layer_id == OHMHIP_LID_MEAN)
  {
    return kReplayMaskMean;
  }
  return (mode == OHMHIP_MODE_TSDF && layer_id == OHMHIP_LID_TSDF) ? kReplayMaskTsdf : kReplayMaskNone;
}

/// What nameWrittenTiles hands back.
struct WrittenTiles
{
  std::vector<uint32_t> slots;  ///< per tile key given, its pool slot
  uint64_t regions = 0;         ///< distinct caller's regions among the tiles
  uint64_t created = 0;         ///< those of which the map held no tile, neither in the pool nor in the host store
};

/// The tiles a call is about to write, by key (a caller's region of a tiled map: every tile of it, or only the ones
/// written).  Precondition: the map is settled, its compute stream drained and the host mirror of the region table
/// fresh (refreshHostRegionTable).  The write-back's pre-cleaned copy of every key is void and dropped; then the tiles
/// are created or brought back from the host store (appendNamedRegions).  All of them are named before the first voxel
/// is written: on failure the map holds what it held.
int nameWrittenTiles(ohmhip_map_t m, const int16_t *tile_keys, size_t n_tiles, WrittenTiles &out)
{
  out = WrittenTiles{};
  // The caller's regions seen so far: a flat hash set (a packed key is never 0), cheap enough for a copy of every region.
  uint32_t seen_mask = 15;
  while (size_t(seen_mask) + 1 < 2 * n_tiles)
  {
    seen_mask = 2 * seen_mask + 1;
  }
  std::vector<uint64_t> seen(size_t(seen_mask) + 1, 0);
  std::vector<TileRef> of_region;
  for (size_t i = 0; i < n_tiles; ++i)
  {
    const int16_t *t = tile_keys + 3 * i;
    const uint64_t region_key = callerRegionKey(m, packRegionKey(t));
    uint32_t idx = hashRegionKey(region_key, seen_mask);
    while (seen[idx] != 0 && seen[idx] != region_key)
    {
      idx = (idx + 1) & seen_mask;
    }
    if (seen[idx] == region_key)
    {
      continue;
    }
    seen[idx] = region_key;
    ++out.regions;
    int16_t r[3];
    regionOfTile(m->mc, t, r);
    tilesOfRegion(m->mc, r, of_region);
    bool held = false;
    for (const TileRef &o : of_region)
    {
      held = held || tileExists(m, o.key);
    }
    out.created += held ? 0u : 1u;
  }
  for (size_t i = 0; i < n_tiles && !m->precleaned.empty(); ++i)
  {
    dropPrecleanedKey(m, packRegionKey(tile_keys + 3 * i));
  }
  out.slots.resize(n_tiles);
  return appendNamedRegions(m, tile_keys, n_tiles, out.slots.data());
}

/// OR `dirty_bits` into the listed slots' dirty words on `stream`.  The list is read until the stream gets to the copy:
/// the caller keeps it alive, by the stream wait it owns.
int markWrittenSlots(ohmhip_map_t m, const uint32_t *slots, size_t count, uint32_t dirty_bits, hipStream_t stream)
{
  const uint32_t *d_index = nullptr;
  OHMHIP_CHECK(uploadSlotIndex(m, slots, count, stream, false, d_index));
  orSlotBits(m, d_index, count, dirty_bits, stream);
  return OHMHIP_OK;
}

/// The marks a write of `layers` (OHMHIP_LAYER_BIT mask) into the named tiles leaves: `dirty_bits` on their slots (0:
/// none -- an upload through ohmhip_map_write_regions leaves none; otherwise as markWrittenSlots, the caller owning the
/// stream wait), and the clearance marks by the one rule: occupancy written makes the neighbourhood's clearance stale
/// (clearanceMarkChanged), clearance written makes the region's own no longer a computed result (clearanceMarkUnwritten).
int markWrittenTiles(ohmhip_map_t m, const int16_t *tile_keys, const uint32_t *slots, size_t n_tiles, unsigned layers,
                     uint32_t dirty_bits, hipStream_t stream)
{
  if (dirty_bits && n_tiles)
  {
    OHMHIP_CHECK(markWrittenSlots(m, slots, n_tiles, dirty_bits, stream));
  }
  const bool occupancy = (layers & OHMHIP_LAYER_BIT(OHMHIP_LID_OCCUPANCY)) != 0;
  const bool clearance = (layers & OHMHIP_LAYER_BIT(OHMHIP_LID_CLEARANCE)) != 0;
  for (size_t i = 0; i < n_tiles && (occupancy || clearance); ++i)
  {
    const uint64_t key = packRegionKey(tile_keys + 3 * i);
    if (occupancy)
    {
      clearanceMarkChanged(m, key);
    }
    if (clearance)
    {
      clearanceMarkUnwritten(m, key);
    }
  }
  return OHMHIP_OK;
}
}  // namespace

#endif  // OHMHIP_WRITE_SIDE_H
