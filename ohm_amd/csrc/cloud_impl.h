// cloud_impl.h -- host side of the point clouds (cloud_kernels.h): argument checks, the ordered work list, then count,
// scan and emit on the map's stream.  Where tiles live, the region order, the chunks of a tile and the count-and-scan
// are read_side.h's.  Included at the end of ohmhip_map.hip's translation unit.
#ifndef OHMHIP_CLOUD_IMPL_H
#define OHMHIP_CLOUD_IMPL_H

namespace
{
/// What every cloud entry point checks before any device work.
int cloudRefusal(ohmhip_map_t m, const ohmhip_cloud_params *p, const uint64_t *count, uint64_t capacity,
                 const double *positions)
{
  if (!p || !m || !count)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  const uint32_t known = OHMHIP_CLOUD_EXPORT_FREE | OHMHIP_CLOUD_IGNORE_VOXEL_MEAN | OHMHIP_CLOUD_USE_EXTENTS;
  if (p->mode > OHMHIP_CLOUD_CLEARANCE || (p->flags & ~known) != 0u)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (std::isnan(p->density_threshold) || std::isnan(p->surface_distance) || std::isnan(p->colour_range))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (p->flags & OHMHIP_CLOUD_USE_EXTENTS)
  {
    for (int c = 0; c < 3; ++c)
    {
      if (!std::isfinite(p->min_extents[c]) || !std::isfinite(p->max_extents[c]))
      {
        return OHMHIP_ERR_INVALID_ARG;
      }
    }
  }
  if (capacity > 0 && !positions)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return readSideRefusal(m, -1);  // (a missing layer is an empty cloud: cloudWorkList)
}

/// A tile of the map as the cloud's order sees it.
struct CloudTileSource
{
  uint64_t order;  ///< regionOrder of the caller's region
  uint32_t tile;   ///< index of the tile in its region, in block order (tilesOfRegion)
  uint64_t key;    ///< the tile's packed key
};

/// The work list of a call, in the cloud's order, and the kernel arguments that do not depend on the result arrays.
/// The map is settled and its stream idle.  chunks.empty(): no point can match.
int cloudWorkList(ohmhip_map_t m, const ohmhip_cloud_params *p, CloudArgs &a, std::vector<CloudChunk> &chunks)
{
  chunks.clear();
  a = CloudArgs{};
  const MapConst &mc = m->mc;
  a.mc = mc;
  a.mode = int(p->mode);
  a.export_free = (p->flags & OHMHIP_CLOUD_EXPORT_FREE) ? 1 : 0;
  a.export_type = p->export_type;
  a.density_threshold = p->density_threshold;
  a.surface_distance = p->surface_distance;
  a.colour_range = p->colour_range;
  int sel_layer = OHMHIP_LID_OCCUPANCY, aux_layer = -1;
  bool aux_needed = false;
  switch (a.mode)
  {
  case OHMHIP_CLOUD_OCCUPANCY:
    a.use_mean = (m->pool.layers[OHMHIP_LID_MEAN] && !(p->flags & OHMHIP_CLOUD_IGNORE_VOXEL_MEAN)) ? 1 : 0;
    aux_layer = a.use_mean ? OHMHIP_LID_MEAN : -1;
    break;
  case OHMHIP_CLOUD_DENSITY:
    sel_layer = OHMHIP_LID_TRAVERSAL;
    aux_layer = OHMHIP_LID_MEAN;
    aux_needed = true;
    a.use_mean = (p->flags & OHMHIP_CLOUD_IGNORE_VOXEL_MEAN) ? 0 : 1;
    break;
  case OHMHIP_CLOUD_TSDF:
    sel_layer = OHMHIP_LID_TSDF;
    break;
  default:
    aux_layer = OHMHIP_LID_CLEARANCE;
    aux_needed = true;
    break;
  }
  if (!m->pool.layers[sel_layer] || (aux_needed && !m->pool.layers[aux_layer]))
  {
    return OHMHIP_OK;  // the reference returns 0 for a map without the layer
  }
  if (a.mode == OHMHIP_CLOUD_TSDF || a.mode == OHMHIP_CLOUD_CLEARANCE)
  {
    a.mc.origin[0] = a.mc.origin[1] = a.mc.origin[2] = 0.0;  // voxelCentreLocal
  }

  OHMHIP_CHECK(readTilesBegin(m));
  // OccupancyMap::regionKey of the extents (the region coordinate is stored in an int16)
  int16_t rmin[3] = { -32768, -32768, -32768 }, rmax[3] = { 32767, 32767, 32767 };
  if (p->flags & OHMHIP_CLOUD_USE_EXTENTS)
  {
    for (int c = 0; c < 3; ++c)
    {
      rmin[c] = int16_t(pointToRegionCoord(p->min_extents[c] - mc.origin[c], mc.region_dim[c]));
      rmax[c] = int16_t(pointToRegionCoord(p->max_extents[c] - mc.origin[c], mc.region_dim[c]));
    }
  }
  const int split_y = mc.tile_split[1], split_z = mc.tile_split[2];
  std::vector<CloudTileSource> tiles;
  for (const uint64_t key : tileKeys(m))
  {
    int16_t t[3], r[3];
    unpackRegionKey(key, t);
    regionOfTile(mc, t, r);
    bool inside = true;
    for (int c = 0; c < 3; ++c)
    {
      inside = inside && r[c] >= rmin[c] && r[c] <= rmax[c];
    }
    if (inside)
    {
      const uint32_t tile = uint32_t((int(t[2]) - int(r[2]) * split_z) * split_y + (int(t[1]) - int(r[1]) * split_y));
      tiles.push_back(CloudTileSource{ regionOrder(r[0], r[1], r[2]), tile, key });
    }
  }
  std::sort(tiles.begin(), tiles.end(), [](const CloudTileSource &l, const CloudTileSource &r) {
    return l.order < r.order || (l.order == r.order && l.tile < r.tile);
  });

  const size_t sel_bytes = kLayerBytes[sel_layer];
  const size_t aux_bytes = (aux_layer >= 0) ? kLayerBytes[aux_layer] : 0;
  const uint32_t tiles_per_region = uint32_t(split_y * split_z);
  for (size_t at = 0; at < tiles.size();)
  {
    // one region: its tiles in block order; a tile without data reads as a cleared chunk does
    size_t next = at;
    int16_t region[3];
    regionOfOrder(tiles[at].order, region);
    for (uint32_t j = 0; j < tiles_per_region; ++j)
    {
      const bool present = next < tiles.size() && tiles[next].order == tiles[at].order && tiles[next].tile == j;
      const TileHome home = present ? tileHome(m, tiles[next].key) : TileHome{};
      const char *sel = tileLayerBlock(m, home, sel_layer);
      const char *aux = (aux_layer >= 0) ? tileLayerBlock(m, home, aux_layer) : nullptr;
      forEachTileChunk(mc, j, [&](uint32_t first, uint32_t count, size_t off) {
        CloudChunk c;
        c.sel = sel ? sel + off * sel_bytes : nullptr;
        c.aux = aux ? aux + off * aux_bytes : nullptr;
        c.first = first;
        c.count = count;
        c.region[0] = region[0];
        c.region[1] = region[1];
        c.region[2] = region[2];
        c.wide = (a.mode != OHMHIP_CLOUD_TSDF && (reinterpret_cast<uintptr_t>(c.sel) & 15u) == 0u) ? 1 : 0;
        chunks.push_back(c);
        return OHMHIP_OK;
      });
      next += present ? 1 : 0;
    }
    at = std::max(next, at + 1);
  }
  if (chunks.size() > size_t(0x7fffffff) / kCloudWaves)
  {
    chunks.clear();
    return OHMHIP_ERR_CAPACITY;
  }
  return OHMHIP_OK;
}

/// Count and scan on the map's stream: a.counts, a.offsets; the total is a.offsets[chunks * kCloudWaves].
int cloudCount(ohmhip_map_t m, CloudArgs &a, const std::vector<CloudChunk> &chunks)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  OHMHIP_CHECK(qs.cloud_chunks.ensure(sizeof(CloudChunk) * chunks.size(), false, s));
  // (the stream is idle -- cloudWorkList's caller waited for it -- so no earlier call still reads the list)
  OHMHIP_CHECK(hipMemcpy(qs.cloud_chunks.ptr, chunks.data(), sizeof(CloudChunk) * chunks.size(), hipMemcpyHostToDevice));
  a.chunks = static_cast<const CloudChunk *>(qs.cloud_chunks.ptr);
  CountScan cs;
  return countAndScan(qs.cloud_scan, chunks.size() * kCloudWaves, s, cs, [&] {
    a.counts = cs.counts;
    a.offsets = cs.offsets;
    hipLaunchKernelGGL(k_cloud_count, dim3(uint32_t(chunks.size())), dim3(64 * kCloudWaves), 0, s, a);
  });
}

int cloudEmit(ohmhip_map_t m, CloudArgs &a, size_t n_chunks, uint64_t capacity, double *d_pos, void *d_keys, float *d_values)
{
  a.capacity = capacity;
  a.out_pos = d_pos;
  a.out_keys = static_cast<GpuKeyOut *>(d_keys);
  a.out_values = d_values;
  hipLaunchKernelGGL(k_cloud_emit, dim3(uint32_t(n_chunks)), dim3(64 * kCloudWaves), 0, m->stream, a);
  return hipGetLastError();
}

/// Refusal, settled map, work list, count and scan; *total valid after return (the stream has been waited for).
int cloudCountHost(ohmhip_map_t m, const ohmhip_cloud_params *p, CloudArgs &a, std::vector<CloudChunk> &chunks,
                   uint64_t *total)
{
  *total = 0;
  OHMHIP_CHECK(hipStreamSynchronize(m->stream));
  OHMHIP_CHECK(cloudWorkList(m, p, a, chunks));
  if (chunks.empty())
  {
    return OHMHIP_OK;
  }
  OHMHIP_CHECK(cloudCount(m, a, chunks));
  unsigned long long n = 0;
  OHMHIP_CHECK(hipMemcpyAsync(&n, a.offsets + chunks.size() * kCloudWaves, sizeof(n), hipMemcpyDeviceToHost, m->stream));
  OHMHIP_CHECK(hipStreamSynchronize(m->stream));
  *total = n;
  return OHMHIP_OK;
}
}  // namespace

extern "C" {

int ohmhip_map_cloud_count(ohmhip_map_t m, const ohmhip_cloud_params *params, uint64_t *count)
try
{
  OHMHIP_CHECK(cloudRefusal(m, params, count, 0, nullptr));
  OHMHIP_SETTLE(m);
  CloudArgs a;
  std::vector<CloudChunk> chunks;
  return cloudCountHost(m, params, a, chunks, count);
}
OHMHIP_ABI_CATCH

int ohmhip_map_cloud(ohmhip_map_t m, const ohmhip_cloud_params *params, uint64_t capacity, double *positions_xyz,
                     void *keys10, float *values, uint64_t *count)
try
{
  OHMHIP_CHECK(cloudRefusal(m, params, count, capacity, positions_xyz));
  OHMHIP_SETTLE(m);
  CloudArgs a;
  std::vector<CloudChunk> chunks;
  OHMHIP_CHECK(cloudCountHost(m, params, a, chunks, count));
  const size_t n = size_t(std::min<uint64_t>(*count, capacity));
  if (n == 0)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  double *d_pos;
  GpuKeyOut *d_keys;
  float *d_values;
  OHMHIP_CHECK(stageOut(qs.cloud_pos, positions_xyz, 3 * n, s, d_pos));
  OHMHIP_CHECK(stageOut(qs.cloud_keys, keys10, n, s, d_keys));
  OHMHIP_CHECK(stageOut(qs.cloud_values, values, n, s, d_values));
  OHMHIP_CHECK(cloudEmit(m, a, chunks.size(), n, d_pos, d_keys, d_values));
  OHMHIP_CHECK(copyOut(positions_xyz, d_pos, 3 * n, s));
  OHMHIP_CHECK(copyOut(keys10, d_keys, n, s));
  OHMHIP_CHECK(copyOut(values, d_values, n, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_cloud_device(ohmhip_map_t m, const ohmhip_cloud_params *params, uint64_t capacity,
                            double *d_positions_xyz, void *d_keys10, float *d_values, uint64_t *d_count)
try
{
  OHMHIP_CHECK(cloudRefusal(m, params, d_count, capacity, d_positions_xyz));
  OHMHIP_SETTLE(m);
  OHMHIP_CHECK(hipStreamSynchronize(m->stream));  // (the host mirror of the region table, and the work list's buffer)
  CloudArgs a;
  std::vector<CloudChunk> chunks;
  OHMHIP_CHECK(cloudWorkList(m, params, a, chunks));
  if (chunks.empty())
  {
    return hipMemsetAsync(d_count, 0, sizeof(uint64_t), m->stream);
  }
  OHMHIP_CHECK(cloudCount(m, a, chunks));
  if (capacity > 0)
  {
    OHMHIP_CHECK(cloudEmit(m, a, chunks.size(), capacity, d_positions_xyz, d_keys10, d_values));
  }
  return hipMemcpyAsync(d_count, a.offsets + chunks.size() * kCloudWaves, sizeof(uint64_t), hipMemcpyDeviceToDevice,
                        m->stream);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_CLOUD_IMPL_H
