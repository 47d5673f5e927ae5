// copy_impl.h -- ohmhip_map_can_copy / ohmhip_map_copy: ohm::canCopy and ohm::copyMap (ohm/CopyUtil.cpp:52-165) between
// two device maps, device to device (include/ohmhip.h, MAP COPY).  The source is a read-side subject
// (read_side.h): settled, then only read -- its regions in the host store where they lie.  The destination is written
// through write_side.h, for all layers at once and with one kernel launch.
//
// Part of ohmhip_map.hip's translation unit (included there, after read_side.h and write_side.h): not a stand-alone
// header.
#ifndef OHMHIP_COPY_IMPL_H
#define OHMHIP_COPY_IMPL_H

namespace
{
/// C1 (CopyUtil.cpp:52-56): two different maps of equal resolution, region voxel dimensions and origin, each compared
/// with ==.
bool mapsCanCopy(ohmhip_map_t dst, ohmhip_map_t src)
{
  bool same = dst != src && src->config.resolution == dst->config.resolution;
  for (int a = 0; a < 3; ++a)
  {
    same = same && src->config.region_dim[a] == dst->config.region_dim[a] && src->config.origin[a] == dst->config.origin[a];
  }
  return same;
}

/// C3 (b), copyFilterExtents (CopyUtil.cpp:37-45) in its operation order, in double.  The centre is MapRegion::centre:
/// coord * region_dimension, without the map origin (ohm/MapRegion.cpp:40-42, ohm/MapCoord.h:37-40).
bool regionPassesExtents(const MapConst &mc, const int16_t region[3], const double min_ext[3], const double max_ext[3])
{
  bool below = false, above = false;
  for (int a = 0; a < 3; ++a)
  {
    const double half = 0.5 * mc.region_dim[a];
    const double centre = double(region[a]) * mc.region_dim[a];
    const double lo = centre - half;
    const double hi = centre + half;
    below = below || hi < min_ext[a];
    above = above || lo > max_ext[a];
  }
  return !below && !above;
}

/// Queue k_copy_map for `jobs` on the destination's compute stream.
int launchMapCopy(ohmhip_map_t dst, const std::vector<MapCopyJob> &jobs)
{
  if (jobs.empty())
  {
    return OHMHIP_OK;
  }
  uint32_t largest = 0;
  for (const MapCopyJob &job : jobs)
  {
    largest = std::max(largest, job.bytes);
  }
  // (a workgroup per 16 KiB of the largest block, at most 16 per job -- k_copy_jobs' figure -- and one for small regions)
  const uint32_t parts = std::max(1u, std::min(16u, (largest + 16383u) / 16384u));
  OHMHIP_CHECK(hipStreamSynchronize(dst->copy_stream));  // (an eviction's job list may still be read from copy_jobs)
  OHMHIP_CHECK(dst->copy_jobs.ensure(sizeof(MapCopyJob) * jobs.size(), false, dst->stream));
  OHMHIP_CHECK(hipMemcpy(dst->copy_jobs.ptr, jobs.data(), sizeof(MapCopyJob) * jobs.size(), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_copy_map, dim3(uint32_t(jobs.size()) * parts), dim3(256), 0, dst->stream,
                     static_cast<const MapCopyJob *>(dst->copy_jobs.ptr), uint32_t(jobs.size()), parts, dst->mc.tsdf_trunc);
  return hipGetLastError();
}
}  // namespace

extern "C" {

int ohmhip_map_can_copy(ohmhip_map_t dst, ohmhip_map_t src)
try
{
  return (dst && src && mapsCanCopy(dst, src)) ? OHMHIP_OK : OHMHIP_ERR_INVALID_ARG;
}
OHMHIP_ABI_CATCH

int ohmhip_map_copy(ohmhip_map_t dst, ohmhip_map_t src, const ohmhip_copy_params *params, ohmhip_copy_stats *stats)
try
{
  ohmhip_copy_stats local_stats;
  ohmhip_copy_stats &st = stats ? *stats : local_stats;
  std::memset(&st, 0, sizeof(st));
  // C8: the argument refusals, before any device work.
  const unsigned flags = params ? params->flags : 0u;
  if (params)
  {
    if ((flags & ~unsigned(OHMHIP_COPY_DIRTY_ONLY | OHMHIP_COPY_USE_EXTENTS)) || (params->layers >> OHMHIP_LID_COUNT) ||
        ((params->keys_xyz != nullptr) != (params->key_count != 0)))
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
    for (int a = 0; a < 3 && (flags & OHMHIP_COPY_USE_EXTENTS); ++a)
    {
      if (std::isnan(params->min_extents[a]) || std::isnan(params->max_extents[a]))
      {
        return OHMHIP_ERR_INVALID_ARG;
      }
    }
  }
  if (!dst || !src || !mapsCanCopy(dst, src))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  OHMHIP_SETTLE(src);
  OHMHIP_SETTLE(dst);
  OHMHIP_CHECK(readSideRefusal(src, -1));
  OHMHIP_CHECK(readSideRefusal(dst, -1));
  if (dst->pool.d_merge_base)
  {
    return OHMHIP_ERR_UNSUPPORTED;  // (a merging replica keeps a base copy per region: an upload is not a delta)
  }
  // C2: the layers both maps hold, then the caller's mask.
  unsigned common = 0;
  for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
  {
    common |= (src->pool.layers[l] && dst->pool.layers[l]) ? OHMHIP_LAYER_BIT(l) : 0u;
  }
  if (common == 0)
  {
    return OHMHIP_ERR_NOT_FOUND;  // CopyUtil.cpp:78-82
  }
  const unsigned layers = (params && params->layers) ? (common & params->layers) : common;

  // C6: the source, settled and idle, is only read from here on.
  OHMHIP_CHECK(hipStreamSynchronize(src->stream));
  OHMHIP_CHECK(readTilesBegin(src));
  const MapConst &mc = src->mc;
  std::vector<uint64_t> present;
  presentRegionOrders(src, present);
  // C3: the regions, in the callers' region order or in the order of the key list.
  std::vector<uint64_t> wanted;
  if (params && params->keys_xyz)
  {
    std::unordered_map<uint64_t, char> seen;
    for (size_t i = 0; i < params->key_count; ++i)
    {
      const int16_t *key = params->keys_xyz + 3 * i;
      const uint64_t order = regionOrder(key[0], key[1], key[2]);
      if (!seen.emplace(order, 1).second)
      {
        continue;
      }
      if (std::binary_search(present.begin(), present.end(), order))
      {
        wanted.push_back(order);
      }
      else
      {
        ++st.keys_absent;
      }
    }
  }
  else
  {
    wanted = present;
  }
  if (flags & OHMHIP_COPY_DIRTY_ONLY)
  {
    // (c) the regions ohmhip_map_dirty_regions lists: a tile's bit is its region's
    std::unordered_map<uint64_t, char> dirty;
    OHMHIP_CHECK(forEachDirtyRegion(src, kDirtySync, [&](uint64_t tile_key) {
      int16_t t[3], r[3];
      unpackRegionKey(tile_key, t);
      regionOfTile(mc, t, r);
      dirty.emplace(regionOrder(r[0], r[1], r[2]), 1);
    }));
    wanted.erase(std::remove_if(wanted.begin(), wanted.end(), [&](uint64_t order) { return !dirty.count(order); }),
                 wanted.end());
  }
  if (flags & OHMHIP_COPY_USE_EXTENTS)
  {
    wanted.erase(std::remove_if(wanted.begin(), wanted.end(),
                                [&](uint64_t order) {
                                  int16_t r[3];
                                  regionOfOrder(order, r);
                                  return !regionPassesExtents(mc, r, params->min_extents, params->max_extents);
                                }),
                 wanted.end());
  }
  st.regions_passed = wanted.size();
  if (wanted.empty())
  {
    return OHMHIP_OK;
  }

  // C7: the destination.  Every tile of a passing region is named: the ones the source lacks are cleared.
  OHMHIP_CHECK(hipStreamSynchronize(dst->stream));
  OHMHIP_CHECK(refreshHostRegionTable(dst));
  std::vector<int16_t> tile_keys;
  std::vector<TileRef> tiles;
  for (const uint64_t order : wanted)
  {
    int16_t r[3];
    regionOfOrder(order, r);
    tilesOfRegion(mc, r, tiles);
    for (const TileRef &t : tiles)
    {
      tile_keys.insert(tile_keys.end(), t.key, t.key + 3);
    }
  }
  const size_t n_tiles = tile_keys.size() / 3;
  WrittenTiles named;
  OHMHIP_CHECK(nameWrittenTiles(dst, tile_keys.data(), n_tiles, named));
  st.regions_created = named.created;

  const size_t tile_voxels = size_t(dst->mc.region_voxels);
  const size_t mask_words = (tile_voxels + 31) / 32;
  std::vector<MapCopyJob> jobs;
  jobs.reserve(n_tiles * 2);
  for (size_t i = 0; i < n_tiles; ++i)
  {
    const uint64_t tile_key = packRegionKey(&tile_keys[3 * i]);
    const TileHome home = tileHome(src, tile_key);
    for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
    {
      if (!(layers & OHMHIP_LAYER_BIT(l)))
      {
        continue;
      }
      MapCopyJob job{};
      job.src = tileLayerBlock(src, home, l);
      job.bytes = uint32_t(tile_voxels * kLayerBytes[l]);
      job.dst = static_cast<char *>(dst->pool.layers[l].get()) + size_t(named.slots[i]) * job.bytes;
      job.clear_word = layerClearWord(l);
      job.mask_kind = replayMaskKind(dst, l);
      job.mask = job.mask_kind ? dst->pool.d_hit_mask.get() + size_t(named.slots[i]) * mask_words : nullptr;
      jobs.push_back(job);
      st.bytes_copied += job.src ? job.bytes : 0u;
    }
  }
  OHMHIP_CHECK(launchMapCopy(dst, jobs));
  st.layers_copied = layers;
  // C5: the marks of an upload, with all three dirty bits; clearance by the caller's region.
  OHMHIP_CHECK(markWrittenTiles(dst, tile_keys.data(), named.slots.data(), n_tiles, layers,
                                kDirtySync | kDirtyMerge | kDirtyClearance, dst->stream));
  OHMHIP_CHECK(hipStreamSynchronize(dst->stream));  // C9: blocking (the slot list above is read until here)
  return hipGetLastError();
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_COPY_IMPL_H
