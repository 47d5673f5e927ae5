// compare_impl.h -- ohmhip_map_compare / ohmhip_map_compare_device: ohm::compare::compareVoxels (ohm/CompareMaps.cpp:
// 334-386) between two device maps (include/ohmhip.h, MAP COMPARE).  Both maps are read-side subjects
// (read_side.h): settled, then only read -- their regions in the host store where they lie.  The work list is laid out
// on the host, regions the evaluated map lacks are accounted here and cost no kernel work; the kernels
// (compare_kernels.h) run on the REFERENCE map's stream with its query buffers.
//
// Part of ohmhip_map.hip's translation unit (included there, after read_side.h): not a stand-alone header.
#ifndef OHMHIP_COMPARE_IMPL_H
#define OHMHIP_COMPARE_IMPL_H

namespace
{
/// K2: members per layer -- all 4 bytes -- and which of them are f32 (ohm/DefaultLayer.cpp:85-303).
const uint32_t kLayerFloatMembers[OHMHIP_LID_COUNT] = { 0x1u, 0x0u, 0x3fu, 0x1u, 0x0u, 0x0u, 0x3u, 0x0u, 0x3u, 0x1u };

/// K7 / K1: what both entry points refuse before any device work.
int compareRefusal(ohmhip_map_t eval, ohmhip_map_t ref, const ohmhip_compare_params *p, uint64_t mismatch_capacity,
                   const void *mismatch_keys, uint64_t missing_capacity, const void *missing_regions, const void *result)
{
  if (!eval || !ref || !p || !result)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if ((p->flags & ~unsigned(OHMHIP_CMP_CONTINUE)) || p->layer_id < 0 || p->layer_id >= OHMHIP_LID_COUNT ||
      (mismatch_capacity > 0 && !mismatch_keys) || (missing_capacity > 0 && !missing_regions) ||
      ((p->keys_xyz != nullptr) != (p->key_count != 0)))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  const uint32_t members = uint32_t(kLayerBytes[p->layer_id] / sizeof(uint32_t));
  if (p->tolerance_members >> members)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  for (int a = 0; a < 3; ++a)
  {
    if (eval->config.region_dim[a] != ref->config.region_dim[a])
    {
      return OHMHIP_ERR_INVALID_ARG;  // K1: the reference would index one block with the other's key
    }
  }
  OHMHIP_CHECK(readSideRefusal(eval, -1));
  return readSideRefusal(ref, -1);
}

/// The call, with every output in device memory, enqueued on ref's stream.  d_keys / d_missing may be null with a
/// capacity of 0.
int compareRun(ohmhip_map_t eval, ohmhip_map_t ref, const ohmhip_compare_params *p, uint64_t mismatch_capacity,
               GpuKeyOut *d_keys, uint64_t missing_capacity, int16_t *d_missing, ohmhip_compare_result *d_result)
{
  // K6: both settled and idle, then only read.
  OHMHIP_SETTLE(ref);
  if (eval != ref)
  {
    OHMHIP_SETTLE(eval);
    OHMHIP_CHECK(hipStreamSynchronize(eval->stream));
  }
  OHMHIP_CHECK(hipStreamSynchronize(ref->stream));
  hipStream_t s = ref->stream;
  ohmhip_map_s::QueryState &qs = ref->query;
  const int layer = p->layer_id;
  const MapConst &mc = ref->mc;

  CompareFinishArgs fin{};
  fin.result = d_result;
  fin.out_keys = d_keys;
  fin.out_missing = d_missing;
  fin.mismatch_capacity = mismatch_capacity;
  fin.missing_capacity = missing_capacity;
  fin.member_count = uint32_t(kLayerBytes[layer] / sizeof(uint32_t));
  fin.layout_match = (ref->pool.layers[layer] && eval->pool.layers[layer]) ? 1 : 0;  // K2
  fin.keep_going = (p->flags & OHMHIP_CMP_CONTINUE) ? 1 : 0;
  for (int a = 0; a < 3; ++a)
  {
    fin.kdim[a] = mc.kdim[a];
  }

  std::vector<CompareChunk> chunks;
  std::vector<int16_t> missing;
  if (fin.layout_match)
  {
    OHMHIP_CHECK(readTilesBegin(ref));
    if (eval != ref)
    {
      OHMHIP_CHECK(readTilesBegin(eval));
    }
    std::vector<uint64_t> present, held;
    presentRegionOrders(ref, present);
    presentRegionOrders(eval, held);
    // K3: every region of ref, narrowed by the key list
    std::vector<uint64_t> wanted;
    if (p->keys_xyz)
    {
      for (size_t i = 0; i < p->key_count; ++i)
      {
        const int16_t *key = p->keys_xyz + 3 * i;
        wanted.push_back(regionOrder(key[0], key[1], key[2]));
      }
      std::sort(wanted.begin(), wanted.end());
      wanted.erase(std::unique(wanted.begin(), wanted.end()), wanted.end());
      const size_t listed = wanted.size();
      wanted.erase(std::remove_if(wanted.begin(), wanted.end(),
                                  [&](uint64_t order) { return !std::binary_search(present.begin(), present.end(), order); }),
                   wanted.end());
      fin.keys_absent = listed - wanted.size();
    }
    else
    {
      wanted = present;
    }
    const size_t elem = kLayerBytes[layer];
    const uintptr_t align_mask = (elem == 4) ? 15u : 7u;
    const size_t tile_voxels = size_t(mc.region_voxels);
    std::vector<TileRef> tiles;
    for (const uint64_t order : wanted)
    {
      int16_t r[3];
      regionOfOrder(order, r);
      tilesOfRegion(mc, r, tiles);
      if (!std::binary_search(held.begin(), held.end(), order))
      {
        if (fin.regions_missing == 0)
        {
          fin.first_missing_chunk = uint32_t(chunks.size());
          std::memcpy(fin.first_missing, r, sizeof(r));
        }
        ++fin.regions_missing;
        fin.missing_voxels += tile_voxels * tiles.size();
        missing.insert(missing.end(), r, r + 3);
        continue;
      }
      ++fin.regions_compared;
      for (size_t j = 0; j < tiles.size(); ++j)
      {
        const uint64_t tile_key = packRegionKey(tiles[j].key);
        const char *ref_block = tileLayerBlock(ref, tileHome(ref, tile_key), layer);
        const char *eval_block = tileLayerBlock(eval, tileHome(eval, tile_key), layer);
        forEachTileChunk(mc, uint32_t(j), [&](uint32_t first, uint32_t count, size_t off) {
          CompareChunk c{};
          c.eval = eval_block ? eval_block + off * elem : nullptr;
          c.ref = ref_block ? ref_block + off * elem : nullptr;
          c.voxels_before = fin.compared_voxels;
          c.first = first;
          c.count = count;
          std::memcpy(c.region, r, sizeof(r));
          c.wide = (((reinterpret_cast<uintptr_t>(c.eval) | reinterpret_cast<uintptr_t>(c.ref)) & align_mask) == 0u) ? 1 : 0;
          chunks.push_back(c);
          fin.compared_voxels += count;
          return OHMHIP_OK;
        });
      }
    }
    if (chunks.size() > size_t(0x7fffffff) / kCloudWaves)
    {
      return OHMHIP_ERR_CAPACITY;
    }
  }
  fin.n_chunks = uint32_t(chunks.size());
  if (fin.regions_missing == 0)
  {
    fin.first_missing_chunk = fin.n_chunks;
  }
  // K3: the missing list is the host's; with stop-at-first k_compare_finish writes the one entry it may hold.
  if (fin.keep_going && d_missing && !missing.empty())
  {
    const size_t n = size_t(std::min<uint64_t>(missing.size() / 3, missing_capacity));
    OHMHIP_CHECK(hipMemcpy(d_missing, missing.data(), sizeof(int16_t) * 3 * n, hipMemcpyHostToDevice));
  }

  if (fin.n_chunks > 0)
  {
    CompareArgs a{};
    a.words = fin.member_count;
    a.float_mask = kLayerFloatMembers[layer];
    a.tol_mask = p->tolerance_members;
    a.clear_word = layerClearWord(layer);
    for (uint32_t i = 0; i < kCompareMaxMembers; ++i)
    {
      a.eps[i] = uint32_t(p->tolerance_bits[i] & 0xffffffffull);
    }
    std::memcpy(a.kdim, fin.kdim, sizeof(a.kdim));
    OHMHIP_CHECK(qs.compare_chunks.ensure(sizeof(CompareChunk) * chunks.size(), false, s));
    OHMHIP_CHECK(qs.compare_records.ensure(sizeof(CompareRecord) * chunks.size(), false, s));
    // (the stream is idle, so no earlier call still reads the list)
    OHMHIP_CHECK(hipMemcpy(qs.compare_chunks.ptr, chunks.data(), sizeof(CompareChunk) * chunks.size(), hipMemcpyHostToDevice));
    a.chunks = static_cast<const CompareChunk *>(qs.compare_chunks.ptr);
    a.records = static_cast<CompareRecord *>(qs.compare_records.ptr);
    const bool list = fin.keep_going && mismatch_capacity > 0;
    CountScan cs;
    const size_t parts = chunks.size() * kCloudWaves;
    if (list)
    {
      OHMHIP_CHECK(countAndScan(qs.compare_scan, parts, s, cs, [&] {
        a.counts = cs.counts;
        a.offsets = cs.offsets;
        hipLaunchKernelGGL(k_compare_count, dim3(fin.n_chunks), dim3(64 * kCloudWaves), 0, s, a);
      }));
      a.capacity = mismatch_capacity;
      a.out_keys = d_keys;
      hipLaunchKernelGGL(k_compare_emit, dim3(fin.n_chunks), dim3(64 * kCloudWaves), 0, s, a);
    }
    else
    {
      OHMHIP_CHECK(qs.compare_scan.counts.ensure(sizeof(uint32_t) * (parts + 1), false, s));
      a.counts = static_cast<uint32_t *>(qs.compare_scan.counts.ptr);
      hipLaunchKernelGGL(k_compare_count, dim3(fin.n_chunks), dim3(64 * kCloudWaves), 0, s, a);
    }
    OHMHIP_CHECK(hipGetLastError());
    fin.chunks = a.chunks;
    fin.records = a.records;
  }
  hipLaunchKernelGGL(k_compare_finish, dim3(1), dim3(256), 0, s, fin);
  return hipGetLastError();
}
}  // namespace

extern "C" {

int ohmhip_map_compare(ohmhip_map_t eval, ohmhip_map_t ref, const ohmhip_compare_params *params,
                       uint64_t mismatch_capacity, void *mismatch_keys10, uint64_t missing_capacity,
                       int16_t *missing_regions_xyz, ohmhip_compare_result *result)
try
{
  OHMHIP_CHECK(compareRefusal(eval, ref, params, mismatch_capacity, mismatch_keys10, missing_capacity,
                              missing_regions_xyz, result));
  std::memset(result, 0, sizeof(*result));
  hipStream_t s = ref->stream;
  ohmhip_map_s::QueryState &qs = ref->query;
  OHMHIP_SETTLE(ref);
  OHMHIP_CHECK(hipStreamSynchronize(s));  // (the staging buffers may still be read by an earlier _device call)
  // (no list is longer than the reference map: a generous capacity stages no more than that)
  OHMHIP_CHECK(readTilesBegin(ref));
  const uint64_t ref_tiles = tileKeys(ref).size();
  mismatch_capacity = std::min<uint64_t>(mismatch_capacity, ref_tiles * uint64_t(ref->mc.region_voxels));
  missing_capacity = std::min<uint64_t>(missing_capacity, ref_tiles);
  GpuKeyOut *d_keys;
  int16_t *d_missing;
  ohmhip_compare_result *d_result;
  OHMHIP_CHECK(stageOut(qs.compare_keys, mismatch_keys10, size_t(mismatch_capacity), s, d_keys));
  OHMHIP_CHECK(stageOut(qs.compare_missing, missing_regions_xyz, 3 * size_t(missing_capacity), s, d_missing));
  OHMHIP_CHECK(stageOut(qs.compare_result, result, 1, s, d_result));
  OHMHIP_CHECK(compareRun(eval, ref, params, mismatch_capacity, d_keys, missing_capacity, d_missing, d_result));
  OHMHIP_CHECK(copyOut(result, d_result, 1, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  // the lists: what the totals say landed, no more
  const size_t n_keys = size_t(std::min<uint64_t>(result->mismatch_count, mismatch_capacity));
  const size_t n_missing = size_t(std::min<uint64_t>(result->missing_count, missing_capacity));
  OHMHIP_CHECK(copyOut(n_keys ? mismatch_keys10 : nullptr, d_keys, n_keys, s));
  OHMHIP_CHECK(copyOut(n_missing ? missing_regions_xyz : nullptr, d_missing, 3 * n_missing, s));
  return hipStreamSynchronize(s);  // K7: blocking
}
OHMHIP_ABI_CATCH

int ohmhip_map_compare_device(ohmhip_map_t eval, ohmhip_map_t ref, const ohmhip_compare_params *params,
                              uint64_t mismatch_capacity, void *d_mismatch_keys10, uint64_t missing_capacity,
                              int16_t *d_missing_regions_xyz, ohmhip_compare_result *d_result)
try
{
  OHMHIP_CHECK(compareRefusal(eval, ref, params, mismatch_capacity, d_mismatch_keys10, missing_capacity,
                              d_missing_regions_xyz, d_result));
  return compareRun(eval, ref, params, mismatch_capacity, static_cast<GpuKeyOut *>(d_mismatch_keys10), missing_capacity,
                    d_missing_regions_xyz, d_result);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_COMPARE_IMPL_H
