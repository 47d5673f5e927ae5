// neighbours_impl.h -- host side of the point queries (neighbours_kernels.h): argument checks, the ordered and pruned
// work list of a NearestNeighbours call, count, scan and emit on the map's stream; voxel keys of points; voxels read by
// key.  Where tiles live, the region order, the chunks of a tile and the count-and-scan are read_side.h's.  Included at
// the end of ohmhip_map.hip's translation unit, after cloud_impl.h.
#ifndef OHMHIP_NEIGHBOURS_IMPL_H
#define OHMHIP_NEIGHBOURS_IMPL_H

namespace
{
constexpr size_t kNnMaxChunks = size_t(1) << 24;

/// What every NearestNeighbours entry point checks before any device work.
int nnRefusal(ohmhip_map_t m, const double *points, size_t query_count, const ohmhip_neighbours_params *p,
              uint64_t capacity, const void *counts, const void *keys, const void *total)
{
  if (!m || !p || !counts || !total || (query_count && !points) || query_count > size_t(0x7fffffff))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  for (size_t i = 0; i < 3 * query_count; ++i)
  {
    if (!std::isfinite(points[i]))
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
  }
  if (!(p->search_radius >= 0.0f) || !std::isfinite(p->search_radius))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if ((p->query_flags & ~(OHMHIP_QF_UNKNOWN_AS_OCCUPIED | OHMHIP_QF_NEAREST_RESULT)) != 0u)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (capacity > 0 && !keys)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return readSideRefusal(m, OHMHIP_LID_OCCUPANCY);
}

/// Smallest distance between p and the box [lo, hi], squared.
double boxDistance2(const double p[3], const double lo[3], const double hi[3])
{
  double d2 = 0;
  for (int c = 0; c < 3; ++c)
  {
    const double gap = std::max(std::max(lo[c] - p[c], p[c] - hi[c]), 0.0);
    d2 += gap * gap;
  }
  return d2;
}

/// The work list of a call, ordered by query, then region (rz, ry, rx), then chunk, and the kernel arguments that do not
/// depend on the result arrays.  The map is settled and its stream idle.
///
/// PRUNING.  A chunk is dropped when the fp64 distance from the near point to the box of its voxel centres exceeds the
/// radius by more than a margin that covers what fp32 can make of it: with M the largest magnitude among the centre
/// and near point coordinates, a centre narrowed to float moves by at most M * 2^-24, the fp32 difference by as much
/// again, and the dot product and radius * radius carry a few relative 2^-24 each -- under 10^-6 (radius + M) in all.
/// The margin is 10^-5 (radius + M) + 10^-18 (the constant covers squares that underflow to zero), so a dropped chunk
/// holds no voxel the fp32 test could pass and the result is the unpruned list's, byte for byte.  OHMHIP_NN_PRUNE=0
/// keeps every chunk (A/B runs).
int nnWorkList(ohmhip_map_t m, const double *points, size_t query_count, const ohmhip_neighbours_params *p, NnArgs &a,
               std::vector<NnChunk> &chunks, std::vector<uint32_t> &chunk_begin, std::vector<float> &near_local)
{
  chunks.clear();
  chunk_begin.assign(query_count + 1, 0u);
  near_local.resize(3 * query_count);
  a = NnArgs{};
  a.mc = m->mc;
  a.mc.origin[0] = a.mc.origin[1] = a.mc.origin[2] = 0.0;  // voxelCentreLocal
  a.radius2 = p->search_radius * p->search_radius;
  a.unknown_as_occupied = (p->query_flags & OHMHIP_QF_UNKNOWN_AS_OCCUPIED) ? 1 : 0;
  a.nearest = (p->query_flags & OHMHIP_QF_NEAREST_RESULT) ? 1 : 0;
  a.n_queries = uint32_t(query_count);
  const MapConst &mc = m->mc;

  OHMHIP_CHECK(readTilesBegin(m));
  const char *prune_env = std::getenv("OHMHIP_NN_PRUNE");
  const bool prune = !(prune_env && std::atoi(prune_env) == 0) && std::isfinite(a.radius2);
  const double radius = double(p->search_radius);
  const int split_y = mc.tile_split[1], split_z = mc.tile_split[2];
  const uint32_t dx = uint32_t(mc.kdim[0]), dy = uint32_t(mc.kdim[1]);

  // the map's regions in the caller's coordinates, in visiting order: what a query without kQfUnknownAsOccupied can see
  std::vector<uint64_t> present;  // (regionOrder)
  if (!a.unknown_as_occupied)
  {
    presentRegionOrders(m, present);
  }

  std::vector<const char *> tile_blocks(size_t(split_y) * size_t(split_z));
  for (size_t q = 0; q < query_count; ++q)
  {
    const double *point = points + 3 * q;
    double near_d[3];
    int rmin[3], rmax[3];
    double regions_in_box = 1;
    for (int c = 0; c < 3; ++c)
    {
      near_local[3 * q + c] = float(point[c] - mc.origin[c]);  // glm::vec3(near_point - origin)
      near_d[c] = double(near_local[3 * q + c]);
      // regionKey(near -+ radius) (ohm/NearestNeighbours.cpp:251-263, OccupancyMap.cpp:746-750): stored in an int16
      rmin[c] = int16_t(pointToRegionCoord((point[c] - radius) - mc.origin[c], mc.region_dim[c]));
      rmax[c] = int16_t(pointToRegionCoord((point[c] + radius) - mc.origin[c], mc.region_dim[c]));
      regions_in_box *= double(std::max(0, rmax[c] - rmin[c] + 1));
    }
    chunk_begin[q] = uint32_t(chunks.size());

    // one region of the box, in order
    auto visit = [&](int rx, int ry, int rz) -> int {
      const int16_t region[3] = { int16_t(rx), int16_t(ry), int16_t(rz) };
      double lo[3], hi[3], magnitude = 0;
      for (int c = 0; c < 3; ++c)
      {
        lo[c] = voxelCentreAxis(a.mc, c, region[c], 0);
        hi[c] = voxelCentreAxis(a.mc, c, region[c], mc.kdim[c] - 1);
        magnitude = std::max(magnitude, std::max(std::fabs(near_d[c]), std::max(std::fabs(lo[c]), std::fabs(hi[c]))));
      }
      const double reach = radius + (1e-5 * (radius + magnitude) + 1e-18);
      const double reach2 = reach * reach;
      if (prune && boxDistance2(near_d, lo, hi) > reach2)
      {
        return OHMHIP_OK;
      }
      bool any = false;
      const bool fits = regionFitsTileKeys(mc, region);
      for (int jz = 0; jz < split_z; ++jz)
      {
        for (int jy = 0; jy < split_y; ++jy)
        {
          const TileHome home = fits ? tileHome(m, packRegionKey(rx, ry * split_y + jy, rz * split_z + jz)) : TileHome{};
          const char *block = tileLayerBlock(m, home, OHMHIP_LID_OCCUPANCY);
          tile_blocks[size_t(jz) * split_y + jy] = block;
          any = any || block != nullptr;
        }
      }
      if (!any && !a.unknown_as_occupied)
      {
        return OHMHIP_OK;  // unknown space, considered free (:54-61)
      }
      for (size_t j = 0; j < tile_blocks.size(); ++j)
      {
        OHMHIP_CHECK(forEachTileChunk(mc, uint32_t(j), [&](uint32_t first, uint32_t count, size_t off) -> int {
          NnChunk c{};
          c.first = first;
          c.count = count;
          if (prune)
          {
            // the box of the chunk's voxels: whole layers, else whole rows of one layer, else a piece of one row
            const uint32_t last = c.first + c.count - 1u;
            uint32_t l0[3] = { 0u, 0u, c.first / (dx * dy) }, l1[3] = { dx - 1u, dy - 1u, last / (dx * dy) };
            if (l0[2] == l1[2])
            {
              l0[1] = (c.first / dx) % dy;
              l1[1] = (last / dx) % dy;
              if (l0[1] == l1[1])
              {
                l0[0] = c.first % dx;
                l1[0] = last % dx;
              }
            }
            double clo[3], chi[3];
            for (int k = 0; k < 3; ++k)
            {
              clo[k] = voxelCentreAxis(a.mc, k, region[k], int(l0[k]));
              chi[k] = voxelCentreAxis(a.mc, k, region[k], int(l1[k]));
            }
            if (boxDistance2(near_d, clo, chi) > reach2)
            {
              return OHMHIP_OK;
            }
          }
          const char *block = tile_blocks[j];
          c.sel = block ? reinterpret_cast<const float *>(block) + off : nullptr;
          c.region[0] = region[0];
          c.region[1] = region[1];
          c.region[2] = region[2];
          c.query = uint32_t(q);
          if (chunks.size() >= kNnMaxChunks)
          {
            return OHMHIP_ERR_CAPACITY;
          }
          chunks.push_back(c);
          return OHMHIP_OK;
        }));
      }
      return OHMHIP_OK;
    };

    if (a.unknown_as_occupied || regions_in_box <= double(present.size()))
    {
      // every region of the box is listed (or looked up)
      // (a sphere fills more than half of its box of regions and every region it reaches lists at least one chunk: a
      // box of four times the limit cannot stay under it, and is not worth walking)
      if (regions_in_box > double(kNnMaxChunks) * 4.0)
      {
        chunks.clear();
        return OHMHIP_ERR_CAPACITY;
      }
      for (int rz = rmin[2]; rz <= rmax[2]; ++rz)
      {
        for (int ry = rmin[1]; ry <= rmax[1]; ++ry)
        {
          for (int rx = rmin[0]; rx <= rmax[0]; ++rx)
          {
            const int err = visit(rx, ry, rz);
            if (err != OHMHIP_OK)
            {
              chunks.clear();
              return err;
            }
          }
        }
      }
    }
    else
    {
      for (const uint64_t order : present)
      {
        int16_t r[3];
        regionOfOrder(order, r);
        if (r[0] < rmin[0] || r[0] > rmax[0] || r[1] < rmin[1] || r[1] > rmax[1] || r[2] < rmin[2] || r[2] > rmax[2])
        {
          continue;
        }
        const int err = visit(r[0], r[1], r[2]);
        if (err != OHMHIP_OK)
        {
          chunks.clear();
          return err;
        }
      }
    }
  }
  chunk_begin[query_count] = uint32_t(chunks.size());
  return OHMHIP_OK;
}

/// Count, scan and -- kQfNearestResult -- the selection per query, on the map's stream.  Afterwards a.query_counts holds
/// the results per query and *d_total points at their sum (device memory).  chunks.empty(): zeros.
int nnCount(ohmhip_map_t m, NnArgs &a, const std::vector<NnChunk> &chunks, const std::vector<uint32_t> &chunk_begin,
            const std::vector<float> &near_local, const unsigned long long **d_total)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  const size_t nq = a.n_queries;
  const size_t parts = chunks.size() * kCloudWaves;
  OHMHIP_CHECK(qs.nn_query_counts.ensure(sizeof(unsigned long long) * (nq + 1), false, s));
  unsigned long long *query_counts = static_cast<unsigned long long *>(qs.nn_query_counts.ptr);
  a.query_counts = query_counts;
  if (chunks.empty())
  {
    *d_total = query_counts + nq;
    return hipMemsetAsync(query_counts, 0, sizeof(unsigned long long) * (nq + 1), s);
  }
  OHMHIP_CHECK(qs.nn_chunks.ensure(sizeof(NnChunk) * chunks.size(), false, s));
  OHMHIP_CHECK(qs.nn_chunk_begin.ensure(sizeof(uint32_t) * (nq + 1), false, s));
  OHMHIP_CHECK(qs.nn_near.ensure(sizeof(float) * 3 * nq, false, s));
  if (a.nearest)
  {
    OHMHIP_CHECK(qs.nn_best.ensure(sizeof(unsigned long long) * parts, false, s));
    OHMHIP_CHECK(qs.nn_query_best.ensure(sizeof(NnBest) * nq, false, s));
  }
  // (the stream is idle -- the caller waited for it -- so no earlier call still reads the lists)
  OHMHIP_CHECK(hipMemcpy(qs.nn_chunks.ptr, chunks.data(), sizeof(NnChunk) * chunks.size(), hipMemcpyHostToDevice));
  OHMHIP_CHECK(hipMemcpy(qs.nn_chunk_begin.ptr, chunk_begin.data(), sizeof(uint32_t) * (nq + 1), hipMemcpyHostToDevice));
  OHMHIP_CHECK(hipMemcpy(qs.nn_near.ptr, near_local.data(), sizeof(float) * 3 * nq, hipMemcpyHostToDevice));
  a.chunks = static_cast<const NnChunk *>(qs.nn_chunks.ptr);
  a.chunk_begin = static_cast<const uint32_t *>(qs.nn_chunk_begin.ptr);
  a.near_local = static_cast<const float *>(qs.nn_near.ptr);
  a.best = static_cast<unsigned long long *>(qs.nn_best.ptr);
  a.query_best = static_cast<NnBest *>(qs.nn_query_best.ptr);
  CountScan waves, found;
  auto count = [&] {
    a.counts = waves.counts;
    a.offsets = waves.offsets;
    hipLaunchKernelGGL(k_nn_count, dim3(uint32_t(chunks.size())), dim3(64 * kCloudWaves), 0, s, a);
  };
  if (!a.nearest)
  {
    OHMHIP_CHECK(countAndScan(qs.nn_scan, parts, s, waves, count));
    hipLaunchKernelGGL(k_nn_query_counts, dim3(uint32_t((nq + 255) / 256)), dim3(256), 0, s, a);
    *d_total = waves.total;
    return hipGetLastError();
  }
  // the closest voxel per wave, then per query; the scan is over the queries that found one
  OHMHIP_CHECK(scanReserve(qs.nn_scan, parts, s, waves));
  const int err = countAndScan(qs.nn_query_scan, nq, s, found, [&] {
    count();
    a.query_found = found.counts;
    a.query_offsets = found.offsets;
    hipLaunchKernelGGL(k_nn_nearest, dim3(uint32_t(nq)), dim3(64), 0, s, a);
  });
  *d_total = found.total;
  return err;
}

int nnEmit(ohmhip_map_t m, NnArgs &a, size_t n_chunks, uint64_t capacity, void *d_keys, float *d_ranges)
{
  a.capacity = capacity;
  a.out_keys = static_cast<GpuKeyOut *>(d_keys);
  a.out_ranges = d_ranges;
  if (a.nearest)
  {
    hipLaunchKernelGGL(k_nn_nearest_emit, dim3((a.n_queries + 255u) / 256u), dim3(256), 0, m->stream, a);
  }
  else
  {
    hipLaunchKernelGGL(k_nn_emit, dim3(uint32_t(n_chunks)), dim3(64 * kCloudWaves), 0, m->stream, a);
  }
  return hipGetLastError();
}

/// What both voxel-read entry points check before any device work.
int readVoxelsRefusal(ohmhip_map_t m, int layer_id, const void *keys, size_t count, const void *values,
                      const void *present)
{
  if (!m || layer_id < 0 || layer_id >= OHMHIP_LID_COUNT || (count && (!keys || !values || !present)) ||
      count > size_t(0x7fffffff))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return readSideRefusal(m, layer_id);
}

/// The read on device arrays, enqueued on the map's stream; the map is settled.
int readVoxelsDevice(ohmhip_map_t m, int layer_id, const GpuKeyOut *d_keys, uint32_t count, void *d_values,
                     uint8_t *d_present)
{
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  ReadVoxelsArgs a{};
  OHMHIP_CHECK(mapReadView(m, a, layer_id));
  a.keys = d_keys;
  a.n = count;
  a.voxel_dwords = uint32_t(kLayerBytes[layer_id] / sizeof(uint32_t));
  a.clear_word = layerClearWord(layer_id);
  a.values = static_cast<uint32_t *>(d_values);
  a.present = d_present;
  hipLaunchKernelGGL(k_read_voxels, dim3((count + 255u) / 256u), dim3(256), 0, m->stream, a);
  return hipGetLastError();
}
}  // namespace

extern "C" {

int ohmhip_map_nearest_neighbours(ohmhip_map_t m, const double *points_xyz, size_t query_count,
                                  const ohmhip_neighbours_params *params, uint64_t capacity, uint64_t *counts,
                                  void *keys10, float *ranges, uint64_t *total)
try
{
  OHMHIP_CHECK(nnRefusal(m, points_xyz, query_count, params, capacity, counts, keys10, total));
  *total = 0;
  if (query_count == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_SETTLE(m);
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  OHMHIP_CHECK(hipStreamSynchronize(s));
  NnArgs a;
  std::vector<NnChunk> chunks;
  std::vector<uint32_t> chunk_begin;
  std::vector<float> near_local;
  OHMHIP_CHECK(nnWorkList(m, points_xyz, query_count, params, a, chunks, chunk_begin, near_local));
  const unsigned long long *d_total = nullptr;
  OHMHIP_CHECK(nnCount(m, a, chunks, chunk_begin, near_local, &d_total));
  unsigned long long n_total = 0;
  OHMHIP_CHECK(hipMemcpyAsync(&n_total, d_total, sizeof(n_total), hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipMemcpyAsync(counts, a.query_counts, sizeof(uint64_t) * query_count, hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  *total = n_total;
  const size_t n = size_t(std::min<uint64_t>(n_total, capacity));
  if (n == 0)
  {
    return OHMHIP_OK;
  }
  GpuKeyOut *d_keys;
  float *d_ranges;
  OHMHIP_CHECK(stageOut(qs.nn_keys, keys10, n, s, d_keys));
  OHMHIP_CHECK(stageOut(qs.nn_ranges, ranges, n, s, d_ranges));
  OHMHIP_CHECK(nnEmit(m, a, chunks.size(), n, d_keys, d_ranges));
  OHMHIP_CHECK(copyOut(keys10, d_keys, n, s));
  OHMHIP_CHECK(copyOut(ranges, d_ranges, n, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_nearest_neighbours_device(ohmhip_map_t m, const double *points_xyz, size_t query_count,
                                         const ohmhip_neighbours_params *params, uint64_t capacity, uint64_t *d_counts,
                                         void *d_keys10, float *d_ranges, uint64_t *d_total)
try
{
  OHMHIP_CHECK(nnRefusal(m, points_xyz, query_count, params, capacity, d_counts, d_keys10, d_total));
  OHMHIP_SETTLE(m);
  hipStream_t s = m->stream;
  if (query_count == 0)
  {
    return hipMemsetAsync(d_total, 0, sizeof(uint64_t), s);
  }
  OHMHIP_CHECK(hipStreamSynchronize(s));  // (the host mirror of the region table, and the work list's buffers)
  NnArgs a;
  std::vector<NnChunk> chunks;
  std::vector<uint32_t> chunk_begin;
  std::vector<float> near_local;
  OHMHIP_CHECK(nnWorkList(m, points_xyz, query_count, params, a, chunks, chunk_begin, near_local));
  const unsigned long long *total = nullptr;
  OHMHIP_CHECK(nnCount(m, a, chunks, chunk_begin, near_local, &total));
  if (capacity > 0 && !chunks.empty())
  {
    OHMHIP_CHECK(nnEmit(m, a, chunks.size(), capacity, d_keys10, d_ranges));
  }
  OHMHIP_CHECK(hipMemcpyAsync(d_counts, a.query_counts, sizeof(uint64_t) * query_count, hipMemcpyDeviceToDevice, s));
  return hipMemcpyAsync(d_total, total, sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_voxel_keys(ohmhip_map_t m, const double *points_xyz, size_t count, void *keys10)
try
{
  if (!m || (count && (!points_xyz || !keys10)))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  // OccupancyMap::voxelKey (ohm/OccupancyMap.cpp:859-886): key maths of the map's configuration alone, evaluated by
  // the function the kernels evaluate (walk_device.h) on the host.  The keys are the caller's: a region whose TILE
  // coordinates leave the packed key's range still has a key.
  GpuKeyOut *out = static_cast<GpuKeyOut *>(keys10);
  for (size_t i = 0; i < count; ++i)
  {
    int region[3], local[3];
    bool beyond_tiles = false;
    const bool ok = voxelKey(m->mc, points_xyz + 3 * i, region, local, &beyond_tiles) || beyond_tiles;
    GpuKeyOut k;  // Key::kNull (ohm/Key.cpp:14): region lowest() x 3, voxel 0
    k.region[0] = k.region[1] = k.region[2] = int16_t(-32768);
    k.voxel[0] = k.voxel[1] = k.voxel[2] = k.voxel[3] = 0;
    if (ok)
    {
      for (int c = 0; c < 3; ++c)
      {
        k.region[c] = int16_t(region[c]);
        k.voxel[c] = uint8_t(local[c]);
      }
    }
    out[i] = k;
  }
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

int ohmhip_map_read_voxels(ohmhip_map_t m, int layer_id, const void *keys10, size_t count, void *values,
                           uint8_t *present)
try
{
  OHMHIP_CHECK(readVoxelsRefusal(m, layer_id, keys10, count, values, present));
  const GpuKeyOut *k = static_cast<const GpuKeyOut *>(keys10);
  for (size_t i = 0; i < count; ++i)
  {
    for (int c = 0; c < 3; ++c)
    {
      if (int(k[i].voxel[c]) >= m->mc.kdim[c])
      {
        return OHMHIP_ERR_INVALID_ARG;  // not a voxel of the map's regions
      }
    }
  }
  OHMHIP_SETTLE(m);
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  const size_t value_bytes = kLayerBytes[layer_id] * count;
  OHMHIP_CHECK(qs.rv_keys.ensure(sizeof(GpuKeyOut) * count, false, s));
  OHMHIP_CHECK(qs.rv_values.ensure(value_bytes, false, s));
  OHMHIP_CHECK(qs.rv_present.ensure(count, false, s));
  OHMHIP_CHECK(hipMemcpyAsync(qs.rv_keys.ptr, keys10, sizeof(GpuKeyOut) * count, hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(readVoxelsDevice(m, layer_id, static_cast<const GpuKeyOut *>(qs.rv_keys.ptr), uint32_t(count),
                                qs.rv_values.ptr, static_cast<uint8_t *>(qs.rv_present.ptr)));
  OHMHIP_CHECK(hipMemcpyAsync(values, qs.rv_values.ptr, value_bytes, hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipMemcpyAsync(present, qs.rv_present.ptr, count, hipMemcpyDeviceToHost, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_read_voxels_device(ohmhip_map_t m, int layer_id, const void *d_keys10, size_t count, void *d_values,
                                  uint8_t *d_present)
try
{
  OHMHIP_CHECK(readVoxelsRefusal(m, layer_id, d_keys10, count, d_values, d_present));
  OHMHIP_SETTLE(m);
  return readVoxelsDevice(m, layer_id, static_cast<const GpuKeyOut *>(d_keys10), uint32_t(count), d_values, d_present);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_NEIGHBOURS_IMPL_H
