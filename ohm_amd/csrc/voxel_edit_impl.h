// voxel_edit_impl.h -- ohmhip_map_write_voxels / ohmhip_map_integrate_voxels and their _device forms: voxels edited by
// key where they live, in the pool (include/ohmhip.h, VOXEL EDITS).  The tiles an edit names are
// created or brought back, and the marks of an upload left on them, by write_side.h; the voxels are
// written by voxel_edit_kernels.h.
//
// Part of ohmhip_map.hip's translation unit (included there, after read_side.h and write_side.h): not a stand-alone
// header.
#ifndef OHMHIP_VOXEL_EDIT_IMPL_H
#define OHMHIP_VOXEL_EDIT_IMPL_H

namespace
{
/// One edit with every array in device memory.
struct EditRequest
{
  int layer_id;  ///< SET: the layer written; otherwise the occupancy layer
  bool set;
  const void *d_keys;
  const double *d_points;
  const uint8_t *d_ops;
  int op;
  const void *d_values;
  uint32_t n;
};

/// E8, the part both calls share: what is refused before any device work, then what the map cannot do.
int editRefusal(ohmhip_map_t m, int layer_id, size_t count, const void *keys, const void *points)
{
  // (exactly one of keys and points; neither only when there is nothing to do)
  if (!m || count > size_t(0x7fffffff) || layer_id < 0 || layer_id >= OHMHIP_LID_COUNT || (keys && points) ||
      (count && !keys && !points))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  OHMHIP_CHECK(readSideRefusal(m, layer_id));
  // (a merging replica keeps a base copy per region: an edit is not a delta)
  return m->pool.d_merge_base ? int(OHMHIP_ERR_UNSUPPORTED) : int(OHMHIP_OK);
}

/// The edit, on the settled map: E5's regions first, then locate, sort, apply and E6's marks.  Returns with the
/// compute stream drained and `st` final.
int editDevice(ohmhip_map_t m, const EditRequest &rq, ohmhip_voxel_edit_stats &st)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::EditState &es = m->edit;
  const size_t n = rq.n;
  OHMHIP_CHECK(hipStreamSynchronize(s));
  OHMHIP_CHECK(refreshHostRegionTable(m));
  OHMHIP_CHECK(es.keys_a.ensure(sizeof(unsigned long long) * n, false, s));
  OHMHIP_CHECK(es.keys_b.ensure(sizeof(unsigned long long) * n, false, s));
  OHMHIP_CHECK(es.vals_a.ensure(sizeof(uint32_t) * n, false, s));
  OHMHIP_CHECK(es.vals_b.ensure(sizeof(uint32_t) * n, false, s));
  OHMHIP_CHECK(es.tiles.ensure(sizeof(unsigned long long) * n, false, s));
  OHMHIP_CHECK(es.counters.ensure(sizeof(unsigned long long) * kEditCounters, false, s));
  unsigned long long *keys_a = static_cast<unsigned long long *>(es.keys_a.ptr);
  unsigned long long *keys_b = static_cast<unsigned long long *>(es.keys_b.ptr);
  uint32_t *vals_a = static_cast<uint32_t *>(es.vals_a.ptr);
  uint32_t *vals_b = static_cast<uint32_t *>(es.vals_b.ptr);
  unsigned long long *d_tiles = static_cast<unsigned long long *>(es.tiles.ptr);
  unsigned long long *d_counters = static_cast<unsigned long long *>(es.counters.ptr);
  unsigned long long *d_tile_count = d_counters + kEditCounters - 1;
  OHMHIP_CHECK(hipMemsetAsync(d_counters, 0, sizeof(unsigned long long) * kEditCounters, s));

  EditArgs a{};
  a.mc = m->mc;
  a.rt = regionTable(m);
  a.keys = static_cast<const GpuKeyOut *>(rq.d_keys);
  a.points = rq.d_points;
  a.ops = rq.d_ops;
  a.op = uint32_t(rq.op);
  a.n = rq.n;
  a.set = rq.set ? 1u : 0u;
  a.counters = d_counters;
  const dim3 grid(uint32_t((n + 255u) / 256u)), block(256);

  // E5: the distinct tiles the edit names -- the one read-back of the call (the region table is the host's)
  a.tile_keys = keys_a;
  a.sort_vals = vals_a;
  hipLaunchKernelGGL(k_edit_tiles, grid, block, 0, s, a);
  OHMHIP_CHECK(hipGetLastError());
  {
    // (every bit of the packed tile key: kKeyOccupied alone tells tile (0, 0, 0) from the null element's 0.  The
    // pair sort of the second pass, its values unused here: one instantiation of rocPRIM's sort for both)
    size_t sort_bytes = 0, unique_bytes = 0;
    OHMHIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_a, keys_b, vals_a, vals_b, n, 0, 64, s));
    OHMHIP_CHECK(rocprim::unique(nullptr, unique_bytes, keys_b, d_tiles, d_tile_count, n,
                                 rocprim::equal_to<unsigned long long>(), s));
    OHMHIP_CHECK(es.temp.ensure(std::max<size_t>(std::max(sort_bytes, unique_bytes), 16), false, s));
    OHMHIP_CHECK(rocprim::radix_sort_pairs(es.temp.ptr, sort_bytes, keys_a, keys_b, vals_a, vals_b, n, 0, 64, s));
    OHMHIP_CHECK(rocprim::unique(es.temp.ptr, unique_bytes, keys_b, d_tiles, d_tile_count, n,
                                 rocprim::equal_to<unsigned long long>(), s));
  }
  unsigned long long counters[kEditCounters] = {};
  OHMHIP_CHECK(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  const size_t n_distinct = size_t(counters[kEditCounters - 1]);
  std::vector<unsigned long long> tiles(n_distinct);
  if (!tiles.empty())
  {
    OHMHIP_CHECK(hipMemcpy(tiles.data(), d_tiles, sizeof(unsigned long long) * tiles.size(), hipMemcpyDeviceToHost));
    if (tiles.front() == 0ull)
    {
      tiles.erase(tiles.begin());  // (the null elements' entry sorts first)
    }
  }
  const uint64_t null_keys = counters[kEditCountNull];
  if (tiles.empty())
  {
    st.null_keys = null_keys;
    return OHMHIP_OK;
  }
  const size_t n_tiles = tiles.size();
  std::vector<int16_t> tile_keys(3 * n_tiles);
  for (size_t i = 0; i < n_tiles; ++i)
  {
    unpackRegionKey(tiles[i], &tile_keys[3 * i]);
  }
  WrittenTiles named;  // (only the tiles written to)
  OHMHIP_CHECK(nameWrittenTiles(m, tile_keys.data(), n_tiles, named));

  a.rt = regionTable(m);  // (the pool may have grown)
  a.sort_keys = keys_a;
  a.sort_vals = vals_a;
  hipLaunchKernelGGL(k_edit_locate, grid, block, 0, s, a);
  OHMHIP_CHECK(hipGetLastError());
  {
    // slot << 15 | voxel: only the bits a committed slot can set take part; a null element's all-ones key sorts last
    int slot_bits = 1;
    while ((uint64_t(1) << slot_bits) <= uint64_t(m->slots_committed))
    {
      ++slot_bits;
    }
    const unsigned end_bit = kEditVoxelBits + unsigned(slot_bits);
    size_t sort_bytes = 0;
    OHMHIP_CHECK(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_a, keys_b, vals_a, vals_b, n, 0, end_bit, s));
    OHMHIP_CHECK(es.temp.ensure(std::max<size_t>(sort_bytes, 16), false, s));
    OHMHIP_CHECK(rocprim::radix_sort_pairs(es.temp.ptr, sort_bytes, keys_a, keys_b, vals_a, vals_b, n, 0, end_bit, s));
  }
  a.sorted_keys = keys_b;
  a.sorted_vals = vals_b;
  a.layer = static_cast<uint32_t *>(m->pool.layers[rq.layer_id].get());
  a.values = static_cast<const uint32_t *>(rq.d_values);
  a.voxel_dwords = uint32_t(kLayerBytes[rq.layer_id] / sizeof(uint32_t));
  a.occupancy = static_cast<float *>(m->pool.layers[OHMHIP_LID_OCCUPANCY].get());
  a.mean = static_cast<uint32_t *>(m->pool.layers[OHMHIP_LID_MEAN].get());
  a.hit_mask = m->pool.d_hit_mask.get();
  // (integrateHit(map, sample) writes the mean)
  a.mask_kind = replayMaskKind(m, rq.set ? rq.layer_id : int(OHMHIP_LID_MEAN));
  hipLaunchKernelGGL(k_edit_apply, grid, block, 0, s, a);
  OHMHIP_CHECK(hipGetLastError());
  // E6: the marks of an upload, with all three dirty bits; clearance by the caller's region.
  const unsigned written = rq.set ? OHMHIP_LAYER_BIT(rq.layer_id)
                                  : OHMHIP_LAYER_BIT(OHMHIP_LID_OCCUPANCY) | OHMHIP_LAYER_BIT(OHMHIP_LID_MEAN);
  OHMHIP_CHECK(markWrittenTiles(m, tile_keys.data(), named.slots.data(), n_tiles, written,
                                kDirtySync | kDirtyMerge | kDirtyClearance, s));
  OHMHIP_CHECK(hipMemcpyAsync(counters, d_counters, sizeof(counters), hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));  // (the slot list above is read until here)
  OHMHIP_CHECK(hipGetLastError());
  if (counters[kEditCountUnplaced] != 0)
  {
    return OHMHIP_ERR_INTERNAL;  // a named tile the region hash does not hold
  }
  st.applied = uint64_t(n) - null_keys;
  st.null_keys = null_keys;
  st.distinct_voxels = counters[kEditCountVoxels];
  st.regions_touched = named.regions;
  st.regions_created = named.created;
  return OHMHIP_OK;
}

/// A host array's copy on the device; null stays null.
template <typename T>
int editStageIn(DevBuf &buf, const void *host, size_t bytes, hipStream_t s, const T *&dev)
{
  dev = nullptr;
  if (host)
  {
    OHMHIP_CHECK(buf.ensure(bytes, false, s));
    OHMHIP_CHECK(hipMemcpyAsync(buf.ptr, host, bytes, hipMemcpyHostToDevice, s));
    dev = static_cast<const T *>(buf.ptr);
  }
  return OHMHIP_OK;
}

/// E7, host arrays: a key beyond the region dimensions.
bool editKeysInRegion(ohmhip_map_t m, const void *keys10, size_t count)
{
  const GpuKeyOut *k = static_cast<const GpuKeyOut *>(keys10);
  for (size_t i = 0; k && i < count; ++i)
  {
    for (int c = 0; c < 3; ++c)
    {
      if (int(k[i].voxel[c]) >= m->mc.kdim[c])
      {
        return false;
      }
    }
  }
  return true;
}

int writeVoxels(ohmhip_map_t m, int layer_id, const void *keys10, size_t count, const void *values,
                ohmhip_voxel_edit_stats *stats, bool on_device)
{
  ohmhip_voxel_edit_stats local_stats;
  ohmhip_voxel_edit_stats &st = stats ? *stats : local_stats;
  std::memset(&st, 0, sizeof(st));
  OHMHIP_CHECK(editRefusal(m, layer_id, count, keys10, nullptr));
  if (count && !values)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (!on_device && !editKeysInRegion(m, keys10, count))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_SETTLE(m);
  EditRequest rq{ layer_id, true, keys10, nullptr, nullptr, OHMHIP_EDIT_HIT, values, uint32_t(count) };
  if (!on_device)
  {
    const GpuKeyOut *d_keys = nullptr;
    const char *d_values = nullptr;
    OHMHIP_CHECK(editStageIn(m->edit.keys, keys10, sizeof(GpuKeyOut) * count, m->stream, d_keys));
    OHMHIP_CHECK(editStageIn(m->edit.values, values, kLayerBytes[layer_id] * count, m->stream, d_values));
    rq.d_keys = d_keys;
    rq.d_values = d_values;
  }
  const int err = editDevice(m, rq, st);
  if (err)
  {
    (void)hipStreamSynchronize(m->stream);  // (the caller's arrays are free again)
    std::memset(&st, 0, sizeof(st));
  }
  return err;
}

int integrateVoxels(ohmhip_map_t m, const uint8_t *ops, int op, const void *keys10, const double *points_xyz,
                    size_t count, ohmhip_voxel_edit_stats *stats, bool on_device)
{
  ohmhip_voxel_edit_stats local_stats;
  ohmhip_voxel_edit_stats &st = stats ? *stats : local_stats;
  std::memset(&st, 0, sizeof(st));
  OHMHIP_CHECK(editRefusal(m, OHMHIP_LID_OCCUPANCY, count, keys10, points_xyz));
  if (!ops && (op < OHMHIP_EDIT_HIT || op > OHMHIP_EDIT_HIT_SAMPLE || (op == OHMHIP_EDIT_HIT_SAMPLE && !points_xyz)))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (!on_device)
  {
    for (size_t i = 0; ops && i < count; ++i)
    {
      if (ops[i] < OHMHIP_EDIT_HIT || ops[i] > OHMHIP_EDIT_HIT_SAMPLE || (ops[i] == OHMHIP_EDIT_HIT_SAMPLE && !points_xyz))
      {
        return OHMHIP_ERR_INVALID_ARG;
      }
    }
    for (size_t i = 0; points_xyz && i < 3 * count; ++i)
    {
      if (!std::isfinite(points_xyz[i]))
      {
        return OHMHIP_ERR_INVALID_ARG;
      }
    }
    if (keys10 && count && !editKeysInRegion(m, keys10, count))
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
  }
  if (count == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_SETTLE(m);
  EditRequest rq{ OHMHIP_LID_OCCUPANCY, false, keys10, points_xyz, ops, op, nullptr, uint32_t(count) };
  if (!on_device)
  {
    const GpuKeyOut *d_keys = nullptr;
    OHMHIP_CHECK(editStageIn(m->edit.keys, keys10, sizeof(GpuKeyOut) * count, m->stream, d_keys));
    OHMHIP_CHECK(editStageIn(m->edit.points, points_xyz, sizeof(double) * 3 * count, m->stream, rq.d_points));
    OHMHIP_CHECK(editStageIn(m->edit.ops, ops, count, m->stream, rq.d_ops));
    rq.d_keys = d_keys;
  }
  const int err = editDevice(m, rq, st);
  if (err)
  {
    (void)hipStreamSynchronize(m->stream);
    std::memset(&st, 0, sizeof(st));
  }
  return err;
}
}  // namespace

extern "C" {

int ohmhip_map_write_voxels(ohmhip_map_t m, int layer_id, const void *keys10, size_t count, const void *values,
                            ohmhip_voxel_edit_stats *stats)
try
{
  return writeVoxels(m, layer_id, keys10, count, values, stats, false);
}
OHMHIP_ABI_CATCH

int ohmhip_map_write_voxels_device(ohmhip_map_t m, int layer_id, const void *d_keys10, size_t count, const void *d_values,
                                   ohmhip_voxel_edit_stats *stats)
try
{
  return writeVoxels(m, layer_id, d_keys10, count, d_values, stats, true);
}
OHMHIP_ABI_CATCH

int ohmhip_map_integrate_voxels(ohmhip_map_t m, const uint8_t *ops, int op, const void *keys10, const double *points_xyz,
                                size_t count, ohmhip_voxel_edit_stats *stats)
try
{
  return integrateVoxels(m, ops, op, keys10, points_xyz, count, stats, false);
}
OHMHIP_ABI_CATCH

int ohmhip_map_integrate_voxels_device(ohmhip_map_t m, const uint8_t *d_ops, int op, const void *d_keys10,
                                       const double *d_points_xyz, size_t count, ohmhip_voxel_edit_stats *stats)
try
{
  return integrateVoxels(m, d_ops, op, d_keys10, d_points_xyz, count, stats, true);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_VOXEL_EDIT_IMPL_H
