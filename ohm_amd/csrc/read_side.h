// read_side.h -- what the host code of the read-only features shares (query_impl.h, clearance_impl.h,
// clearance_update.h, heightmap_impl.h, heightmap_fill_impl.h, cloud_impl.h, neighbours_impl.h, point_filter_impl.h):
// the refusal every one of them makes, where a tile's data lives, the caller's region order, a tile cut into chunks, the
// map as the read-side kernels see it (and a second layer beside it), count per wave then scan, and the optional host
// outputs.  Included in
// ohmhip_map.hip's translation unit after tiling_impl.h and ahead of the read-side parts.  DESIGN.md 5a says what a new
// feature calls, and in what order.
#ifndef OHMHIP_READ_SIDE_H
#define OHMHIP_READ_SIDE_H

namespace
{
/// What every read-side entry point refuses after its own argument checks: a map without `layer` (< 0: none needed),
/// and a map that is one rank's share of a partitioned map (owner_table is only ever set beside owner_world > 1:
/// ohmhip_map_set_region_partition).
int readSideRefusal(ohmhip_map_t m, int layer)
{
  if (layer >= 0 && !m->pool.layers[layer])
  {
    return OHMHIP_ERR_UNSUPPORTED;
  }
  if (m->mc.owner_world > 1u || m->mc.owner_table)
  {
    return OHMHIP_ERR_UNSUPPORTED;  // a rank holds only its territory
  }
  return OHMHIP_OK;
}

/// Before the first tileHome of a call, with the map settled and its stream idle: the host mirror of the region table
/// is current and the records of the host store are complete (evictions fill them on the copy stream).
int readTilesBegin(ohmhip_map_t m)
{
  OHMHIP_CHECK(refreshHostRegionTable(m));
  return m->spilled.empty() ? int(OHMHIP_OK) : int(hipStreamSynchronize(m->copy_stream));
}

/// Where a tile's data lives: a pool slot, or a record of the pinned host store, or -- neither set -- nowhere.
struct TileHome
{
  uint32_t slot = kSlotUnassigned;
  ohmhip_map_s::SpilledRegion *stored = nullptr;
};

/// A slot counts only when the host mirror agrees on it from both sides.
TileHome tileHome(ohmhip_map_t m, uint64_t tile_key)
{
  TileHome home;
  const auto slot = m->region_slots.find(tile_key);
  if (slot != m->region_slots.end() && slot->second < m->slot_keys_host.size() &&
      m->slot_keys_host[slot->second] == tile_key)
  {
    home.slot = slot->second;
    return home;
  }
  const auto stored = m->spilled.find(tile_key);
  home.stored = (stored != m->spilled.end()) ? &stored->second : nullptr;
  return home;
}

/// The tile's block of `layer` (device visible in either home); null: the map has no such tile.
char *tileLayerBlock(ohmhip_map_t m, const TileHome &home, int layer)
{
  if (home.slot != kSlotUnassigned)
  {
    return static_cast<char *>(m->pool.layers[layer].get()) +
           size_t(home.slot) * size_t(m->mc.region_voxels) * kLayerBytes[layer];
  }
  return home.stored ? home.stored->record + m->store.layer_offset[layer] : nullptr;
}

/// Layer `layer` beside the occupancy layer of a MapReadView, for kernels that find tiles themselves (foundTileLayer);
/// `in_use` false, or a map without the layer: a view with no layer.
LayerView layerView(ohmhip_map_t m, int layer, bool in_use = true)
{
  if (!in_use || !m->pool.layers[layer])
  {
    return LayerView{ nullptr, 0 };
  }
  const size_t *at = m->store.layer_offset;
  return LayerView{ static_cast<const char *>(m->pool.layers[layer].get()),
                    (long long)(at[layer]) - (long long)(at[OHMHIP_LID_OCCUPANCY]) };
}

/// (rz, ry, rx) of a caller's region, biased: ascending == the order clouds, neighbour queries and clearance updates
/// visit regions in.
uint64_t regionOrder(int rx, int ry, int rz)
{
  return (uint64_t(rz + 32768) << 32) | (uint64_t(ry + 32768) << 16) | uint64_t(rx + 32768);
}

void regionOfOrder(uint64_t order, int16_t region[3])
{
  for (int c = 0; c < 3; ++c)
  {
    region[c] = int16_t(int((order >> (16 * c)) & 0xffffu) - 32768);
  }
}

/// Every tile of the map, by packed key: the resident ones in slot order, then the host store's.  After readTilesBegin.
std::vector<uint64_t> tileKeys(ohmhip_map_t m)
{
  std::vector<uint64_t> keys(m->slot_keys_host);
  for (const auto &entry : m->spilled)
  {
    keys.push_back(entry.first);
  }
  return keys;
}

/// The caller's regions present in the map (resident or in the host store), sorted, unique.  After readTilesBegin.
void presentRegionOrders(ohmhip_map_t m, std::vector<uint64_t> &out)
{
  out = tileKeys(m);
  for (uint64_t &key : out)
  {
    int16_t t[3], r[3];
    unpackRegionKey(key, t);
    regionOfTile(m->mc, t, r);
    key = regionOrder(r[0], r[1], r[2]);
  }
  std::sort(out.begin(), out.end());
  out.erase(std::unique(out.begin(), out.end()), out.end());
}

/// Tile `tile_index` (block order: tilesOfRegion) in pieces of at most kCloudChunkVoxels: fn(first, count, off) with
/// `first` the piece's first voxel in the region's block and `off` the same in the tile's.  fn returns OHMHIP_OK to go
/// on; anything else ends the walk and is returned.
template <typename Fn>
int forEachTileChunk(const MapConst &mc, uint32_t tile_index, Fn &&fn)
{
  const uint32_t split_y = uint32_t(mc.tile_split[1]);
  const size_t tile_voxels = size_t(mc.region_voxels);
  const size_t tile_first = tileVoxelOffset(mc, int(tile_index % split_y), int(tile_index / split_y));
  for (size_t off = 0; off < tile_voxels; off += kCloudChunkVoxels)
  {
    OHMHIP_CHECK(fn(uint32_t(tile_first + off), uint32_t(std::min<size_t>(kCloudChunkVoxels, tile_voxels - off)), off));
  }
  return OHMHIP_OK;
}

/// The map as the read-only kernels see it (MapReadView): configuration, region hash, occupancy layer and the table of
/// the host store's regions (QuerySpillTable; empty without spill to host).  `layer`: the layer whose blocks the view
/// addresses (the voxel reads by key look at any layer through the same view).
int mapReadView(ohmhip_map_t m, MapReadView &view, int layer = OHMHIP_LID_OCCUPANCY)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  view.mc = m->mc;
  view.rt = regionTable(m);
  view.occupancy = static_cast<const float *>(m->pool.layers[layer].get());
  view.spill = QuerySpillTable{ nullptr, nullptr, 0 };
  if (!m->spilled.empty())
  {
    // Regions in the host store answer from their pinned records (device visible), without re-admission.  The table is
    // rebuilt per call: the store changes with every batch that evicts or re-admits.  (Evictions copy on the copy
    // stream; the previous query may still read the table being replaced.)
    OHMHIP_CHECK(hipStreamSynchronize(m->copy_stream));
    OHMHIP_CHECK(hipStreamSynchronize(s));
    uint32_t cap = 16;
    while (cap < 2 * m->spilled.size())
    {
      cap <<= 1;
    }
    std::vector<unsigned long long> keys(cap, 0ull);
    std::vector<const float *> blocks(cap, nullptr);
    for (auto &entry : m->spilled)
    {
      uint32_t idx = hashRegionKey(entry.first, cap - 1);
      while (keys[idx] != 0)
      {
        idx = (idx + 1) & (cap - 1);
      }
      keys[idx] = entry.first;
      blocks[idx] = reinterpret_cast<const float *>(tileLayerBlock(m, TileHome{ kSlotUnassigned, &entry.second }, layer));
    }
    OHMHIP_CHECK(qs.spill_keys.ensure(sizeof(unsigned long long) * cap, false, s));
    OHMHIP_CHECK(qs.spill_blocks.ensure(sizeof(const float *) * cap, false, s));
    OHMHIP_CHECK(hipMemcpy(qs.spill_keys.ptr, keys.data(), sizeof(unsigned long long) * cap, hipMemcpyHostToDevice));
    OHMHIP_CHECK(hipMemcpy(qs.spill_blocks.ptr, blocks.data(), sizeof(const float *) * cap, hipMemcpyHostToDevice));
    view.spill = QuerySpillTable{ static_cast<const unsigned long long *>(qs.spill_keys.ptr),
                                  static_cast<const float *const *>(qs.spill_blocks.ptr), cap - 1 };
  }
  return OHMHIP_OK;
}

/// A ScanScratch sized for `parts` counts: counts[parts] is the zero behind them, offsets[parts] -- `total` -- their sum
/// once countAndScan has run.
struct CountScan
{
  uint32_t *counts = nullptr;
  unsigned long long *offsets = nullptr;
  const unsigned long long *total = nullptr;
  size_t temp_bytes = 0;
};

int scanReserve(ScanScratch &sc, size_t parts, hipStream_t s, CountScan &cs)
{
  OHMHIP_CHECK(sc.counts.ensure(sizeof(uint32_t) * (parts + 1), false, s));
  OHMHIP_CHECK(sc.offsets.ensure(sizeof(unsigned long long) * (parts + 1), false, s));
  cs.counts = static_cast<uint32_t *>(sc.counts.ptr);
  cs.offsets = static_cast<unsigned long long *>(sc.offsets.ptr);
  cs.total = cs.offsets + parts;
  OHMHIP_CHECK(rocprim::exclusive_scan(nullptr, cs.temp_bytes, cs.counts, cs.offsets, 0ull, parts + 1,
                                       rocprim::plus<unsigned long long>(), s));
  // (never a null pointer: that would ask rocPRIM for the size again)
  return sc.temp.ensure(std::max<size_t>(cs.temp_bytes, 16), false, s);
}

/// On stream s: `cs` filled in, the zero behind the counts, launch() -- the caller's kernels, which fill
/// cs.counts[0 .. parts) --, then the exclusive scan into cs.offsets.
template <typename Launch>
int countAndScan(ScanScratch &sc, size_t parts, hipStream_t s, CountScan &cs, Launch &&launch)
{
  OHMHIP_CHECK(scanReserve(sc, parts, s, cs));
  OHMHIP_CHECK(hipMemsetAsync(cs.counts + parts, 0, sizeof(uint32_t), s));
  launch();
  OHMHIP_CHECK(hipGetLastError());
  return rocprim::exclusive_scan(sc.temp.ptr, cs.temp_bytes, cs.counts, cs.offsets, 0ull, parts + 1,
                                 rocprim::plus<unsigned long long>(), s);
}

/// The device copy of a host output array of n elements: `buf` grown to hold it, or null when the caller passed none.
template <typename T>
int stageOut(DevBuf &buf, const void *host, size_t n, hipStream_t s, T *&dev)
{
  dev = nullptr;
  if (host)
  {
    OHMHIP_CHECK(buf.ensure(sizeof(T) * n, false, s));
    dev = static_cast<T *>(buf.ptr);
  }
  return OHMHIP_OK;
}

/// ... and back, when the caller passed one.
template <typename T>
int copyOut(void *host, const T *dev, size_t n, hipStream_t s)
{
  return host ? int(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, s)) : int(OHMHIP_OK);
}
}  // namespace

#endif  // OHMHIP_READ_SIDE_H
