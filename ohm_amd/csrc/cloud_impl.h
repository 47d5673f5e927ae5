// cloud_impl.h -- host side of the point clouds (cloud_kernels.h): argument checks, the ordered work list, then count,
// scan and emit on the map's stream.  Included at the end of ohmhip_map.hip's translation unit.
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
  if (m->mc.owner_world > 1u || m->mc.owner_table)
  {
    return OHMHIP_ERR_UNSUPPORTED;  // a rank holds only its territory
  }
  return OHMHIP_OK;
}

/// Where a tile's record lives: a pool slot, or (slot == kSlotUnassigned) a record of the host store, or neither.
struct CloudTileSource
{
  uint64_t order;   ///< (rz, ry, rx) of the caller's region, biased: ascending == the cloud's region order
  uint32_t tile;    ///< index of the tile in its region, in block order (tilesOfRegion)
  uint32_t slot;
  const char *record;
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

  OHMHIP_CHECK(refreshHostRegionTable(m));
  if (!m->spilled.empty())
  {
    OHMHIP_CHECK(hipStreamSynchronize(m->copy_stream));  // (evictions fill the store's records on the copy stream)
  }
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
  tiles.reserve(m->slot_keys_host.size() + m->spilled.size());
  auto add = [&](uint64_t key, uint32_t slot, const char *record) {
    int16_t t[3];
    unpackRegionKey(key, t);
    const int r[3] = { int(t[0]), floorDiv(t[1], split_y), floorDiv(t[2], split_z) };
    for (int c = 0; c < 3; ++c)
    {
      if (r[c] < rmin[c] || r[c] > rmax[c])
      {
        return;
      }
    }
    CloudTileSource s;
    s.order = (uint64_t(r[2] + 32768) << 32) | (uint64_t(r[1] + 32768) << 16) | uint64_t(r[0] + 32768);
    s.tile = uint32_t((int(t[2]) - r[2] * split_z) * split_y + (int(t[1]) - r[1] * split_y));
    s.slot = slot;
    s.record = record;
    tiles.push_back(s);
  };
  for (size_t i = 0; i < m->slot_keys_host.size(); ++i)
  {
    add(m->slot_keys_host[i], uint32_t(i), nullptr);
  }
  for (const auto &entry : m->spilled)
  {
    add(entry.first, kSlotUnassigned, entry.second.record);
  }
  std::sort(tiles.begin(), tiles.end(), [](const CloudTileSource &l, const CloudTileSource &r) {
    return l.order < r.order || (l.order == r.order && l.tile < r.tile);
  });

  const size_t tile_voxels = size_t(mc.region_voxels);
  const size_t sel_bytes = kLayerBytes[sel_layer];
  const size_t aux_bytes = (aux_layer >= 0) ? kLayerBytes[aux_layer] : 0;
  auto block = [&](const CloudTileSource &s, int layer) -> const char * {
    return (s.slot != kSlotUnassigned) ?
             static_cast<const char *>(m->pool.layers[layer].get()) + size_t(s.slot) * tile_voxels * kLayerBytes[layer] :
             s.record + m->store.layer_offset[layer];
  };
  const uint32_t tiles_per_region = uint32_t(split_y * split_z);
  for (size_t at = 0; at < tiles.size();)
  {
    // one region: its tiles in block order; a tile without data reads as a cleared chunk does
    size_t next = at;
    for (uint32_t j = 0; j < tiles_per_region; ++j)
    {
      const bool present = next < tiles.size() && tiles[next].order == tiles[at].order && tiles[next].tile == j;
      const char *sel = present ? block(tiles[next], sel_layer) : nullptr;
      const char *aux = (present && aux_layer >= 0) ? block(tiles[next], aux_layer) : nullptr;
      const uint32_t jy = j % uint32_t(split_y), jz = j / uint32_t(split_y);
      // (tilesOfRegion's voxel_offset)
      const size_t tile_first =
        (size_t(jz) * size_t(mc.dim[2]) * size_t(mc.kdim[1]) + size_t(jy) * size_t(mc.dim[1])) * size_t(mc.kdim[0]);
      for (size_t off = 0; off < tile_voxels; off += kCloudChunkVoxels)
      {
        CloudChunk c;
        c.sel = sel ? sel + off * sel_bytes : nullptr;
        c.aux = aux ? aux + off * aux_bytes : nullptr;
        c.first = uint32_t(tile_first + off);
        c.count = uint32_t(std::min<size_t>(kCloudChunkVoxels, tile_voxels - off));
        c.region[0] = int16_t(int(tiles[at].order & 0xffffu) - 32768);
        c.region[1] = int16_t(int((tiles[at].order >> 16) & 0xffffu) - 32768);
        c.region[2] = int16_t(int((tiles[at].order >> 32) & 0xffffu) - 32768);
        c.wide = (a.mode != OHMHIP_CLOUD_TSDF && (reinterpret_cast<uintptr_t>(c.sel) & 15u) == 0u) ? 1 : 0;
        chunks.push_back(c);
      }
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
  const size_t parts = chunks.size() * kCloudWaves;
  OHMHIP_CHECK(qs.cloud_chunks.ensure(sizeof(CloudChunk) * chunks.size(), false, s));
  OHMHIP_CHECK(qs.cloud_partials.ensure(sizeof(uint32_t) * (parts + 1), false, s));
  OHMHIP_CHECK(qs.cloud_offsets.ensure(sizeof(unsigned long long) * (parts + 1), false, s));
  uint32_t *counts = static_cast<uint32_t *>(qs.cloud_partials.ptr);
  unsigned long long *offsets = static_cast<unsigned long long *>(qs.cloud_offsets.ptr);
  size_t scan_bytes = 0;
  OHMHIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, counts, offsets, 0ull, parts + 1,
                                       rocprim::plus<unsigned long long>(), s));
  OHMHIP_CHECK(qs.cloud_scan_temp.ensure(scan_bytes, false, s));
  // (the stream is idle -- cloudWorkList's caller waited for it -- so no earlier call still reads the list)
  OHMHIP_CHECK(hipMemcpy(qs.cloud_chunks.ptr, chunks.data(), sizeof(CloudChunk) * chunks.size(), hipMemcpyHostToDevice));
  a.chunks = static_cast<const CloudChunk *>(qs.cloud_chunks.ptr);
  a.counts = counts;
  a.offsets = offsets;
  OHMHIP_CHECK(hipMemsetAsync(counts + parts, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_cloud_count, dim3(uint32_t(chunks.size())), dim3(64 * kCloudWaves), 0, s, a);
  OHMHIP_CHECK(hipGetLastError());
  return rocprim::exclusive_scan(qs.cloud_scan_temp.ptr, scan_bytes, counts, offsets, 0ull, parts + 1,
                                 rocprim::plus<unsigned long long>(), s);
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
  OHMHIP_CHECK(qs.cloud_pos.ensure(sizeof(double) * 3 * n, false, s));
  if (keys10)
  {
    OHMHIP_CHECK(qs.cloud_keys.ensure(sizeof(GpuKeyOut) * n, false, s));
  }
  if (values)
  {
    OHMHIP_CHECK(qs.cloud_values.ensure(sizeof(float) * n, false, s));
  }
  OHMHIP_CHECK(cloudEmit(m, a, chunks.size(), n, static_cast<double *>(qs.cloud_pos.ptr),
                         keys10 ? qs.cloud_keys.ptr : nullptr,
                         values ? static_cast<float *>(qs.cloud_values.ptr) : nullptr));
  OHMHIP_CHECK(hipMemcpyAsync(positions_xyz, qs.cloud_pos.ptr, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s));
  if (keys10)
  {
    OHMHIP_CHECK(hipMemcpyAsync(keys10, qs.cloud_keys.ptr, sizeof(GpuKeyOut) * n, hipMemcpyDeviceToHost, s));
  }
  if (values)
  {
    OHMHIP_CHECK(hipMemcpyAsync(values, qs.cloud_values.ptr, sizeof(float) * n, hipMemcpyDeviceToHost, s));
  }
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
