// layout_impl.h -- layers added to and removed from a live map (include/ohmhip.h, "LAYER CHANGES": OccupancyMap::
// updateLayout, ohm/OccupancyMap.cpp:521-682, MapChunk::updateLayout, ohm/MapChunk.cpp:93-143).
//
// Every layer is an allocation of its own (RegionPool::layers), so a change of the set is allocations, fills and frees:
// the blocks of the layers that stay do not move.  What the strides, clear words and record offsets are is slot_state.h's
// business (slotArrays, clearSlots, layoutStoreRecord); this file stages the new blocks, exchanges them with the map's
// and rewrites the host store's records from the list before into the list after.
//
// Part of ohmhip_map.hip's translation unit (included there behind spill_impl.h): not a stand-alone header.
#ifndef OHMHIP_LAYOUT_IMPL_H
#define OHMHIP_LAYOUT_IMPL_H

namespace
{
/// The layers a map of mode `mode` integrates into: they cannot go (U7; validateBatchRequest refuses a map without them).
unsigned requiredLayers(int mode)
{
  const unsigned ndt =
    OHMHIP_LAYER_BIT(OHMHIP_LID_OCCUPANCY) | OHMHIP_LAYER_BIT(OHMHIP_LID_MEAN) | OHMHIP_LAYER_BIT(OHMHIP_LID_COVARIANCE);
  switch (mode)
  {
  case OHMHIP_MODE_OCCUPANCY:
    return OHMHIP_LAYER_BIT(OHMHIP_LID_OCCUPANCY);
  case OHMHIP_MODE_NDT_OM:
    return ndt;
  case OHMHIP_MODE_NDT_TM:
    return ndt | OHMHIP_LAYER_BIT(OHMHIP_LID_INTENSITY) | OHMHIP_LAYER_BIT(OHMHIP_LID_HIT_MISS);
  case OHMHIP_MODE_TSDF:
    return OHMHIP_LAYER_BIT(OHMHIP_LID_TSDF);
  default:
    return 0u;
  }
}

/// The half of a layer change that is not the map's: before the exchange the blocks of the layers to add (and the
/// traversal accumulator with that layer) beside the set to take, afterwards the blocks of the layers removed beside the
/// set the map had.  Exchanging twice leaves everything as it was; what the stage holds at the end is released with it.
struct StagedLayers
{
  ohmhip_map_s::RegionPool blocks;
  unsigned layers = 0;

  void exchange(ohmhip_map_t m)
  {
    const unsigned changed = m->config.layers ^ layers;
    for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
    {
      if (changed & OHMHIP_LAYER_BIT(l))
      {
        std::swap(m->pool.layers[l], blocks.layers[l]);
      }
    }
    if (changed & OHMHIP_LAYER_BIT(OHMHIP_LID_TRAVERSAL))
    {
      std::swap(m->pool.d_traversal_acc, blocks.d_traversal_acc);
    }
    std::swap(m->config.layers, layers);
  }
};

/// U4: the host store takes the record layout of the map's layer set as it is NOW; `before` is the list the records in
/// use were written from.  A part of the new list whose array was in the old one (same base: the blocks that stay do not
/// move) is copied, any other part holds its clear word.  The old slabs go when every record is rewritten -- with them
/// the free records of the old size.  On failure (pinned memory) the store is as it was.
int relayoutStore(ohmhip_map_t m, const SlotArrays &before)
{
  if (m->store.record_bytes == 0)
  {
    return OHMHIP_OK;  // never laid out: reserveStoreRecords does it from the set in force then
  }
  OHMHIP_CHECK(hipStreamSynchronize(m->copy_stream));  // (evictions and re-admissions write and read the records)
  const size_t spare = m->store.free_records.size();
  ohmhip_map_s::HostStore old = std::move(m->store);
  m->store = ohmhip_map_s::HostStore();
  layoutStoreRecord(m);
  const int err = reserveStoreRecords(m, m->spilled.size());
  if (err)
  {
    m->store = std::move(old);
    return err;
  }
  const SlotArrays after = slotArrays(m->mc, m->pool);
  for (auto &entry : m->spilled)
  {
    char *record = takeStoreRecord(m);  // (reserved above)
    for (const SlotArray &a : after)
    {
      if (a.travel != SlotArray::kInRecord)
      {
        continue;
      }
      const SlotArray *from = nullptr;
      for (const SlotArray &b : before)
      {
        from = (b.travel == SlotArray::kInRecord && b.base == a.base) ? &b : from;
      }
      if (from)
      {
        std::memcpy(record + a.record_offset, entry.second.record + from->record_offset, a.stride);
      }
      else
      {
        std::fill_n(reinterpret_cast<uint32_t *>(record + a.record_offset), a.stride / sizeof(uint32_t), a.clear_word);
      }
    }
    entry.second.record = record;  // (dirty bits and use stamp stay)
  }
  old = ohmhip_map_s::HostStore();
  if (m->spill_enabled)
  {
    // what ohmhip_map_set_spill_to_host had pinned ahead of the batches, in records of the new size (best effort: the
    // store grows on demand)
    (void)reserveStoreRecords(m, spare);
  }
  return OHMHIP_OK;
}

int updateLayers(ohmhip_map_t m, unsigned layers, unsigned flags, ohmhip_layer_change_stats *stats)
{
  const unsigned before = m->config.layers;
  if (layers == before && !(flags & OHMHIP_LAYOUT_DISCARD_MAP))
  {
    if (stats)
    {
      stats->layers_before = stats->layers_after = before;
      stats->regions_resident = m->slots_committed;
      stats->regions_in_store = m->spilled.size();
      stats->bytes_per_region_before = stats->bytes_per_region_after = poolBudget(m).per_region;
    }
    return OHMHIP_OK;  // U8: nothing to do
  }
  if ((requiredLayers(m->config.mode) & ~layers) != 0u || m->mc.owner_world > 1u || !m->partition.table_host.empty() ||
      m->pool.d_merge_base)
  {
    return OHMHIP_ERR_UNSUPPORTED;  // U7
  }
  const bool discard = (flags & OHMHIP_LAYOUT_DISCARD_MAP) != 0u;
  hipStream_t s = m->stream;
  // Nothing reads or writes the pool or the store from here on: the batches are done, the write-back's copies are void.
  OHMHIP_CHECK(hipStreamSynchronize(m->front_stream));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  OHMHIP_CHECK(hipStreamSynchronize(m->copy_stream));
  dropPrecleaned(m);
  OHMHIP_CHECK(refreshHostRegionTable(m));

  // U5: what the resident regions may number under the new set.
  const PoolBudget budget_before = poolBudget(m);
  m->config.layers = layers;
  const PoolBudget budget_after = poolBudget(m);
  m->config.layers = before;
  uint32_t to_evict = 0;
  if (!discard && m->memory_limit && m->slots_committed > budget_after.regions)
  {
    if (!m->spill_enabled || budget_after.regions == 0)
    {
      return OHMHIP_ERR_CAPACITY;
    }
    to_evict = uint32_t(m->slots_committed - budget_after.regions);
  }

  // U3: everything new first.  (The stage releases itself on every way out.)
  const unsigned added = layers & ~before;
  StagedLayers stage;
  stage.layers = layers;
  {
    int err = allocLayerArrays(m, stage.blocks, m->pool.slot_capacity, added);
    if (!err && (added & OHMHIP_LAYER_BIT(OHMHIP_LID_TRAVERSAL)))
    {
      err = allocTraversalAcc(m, stage.blocks, m->pool.slot_capacity, s);
    }
    if (err)
    {
      (void)hipStreamSynchronize(s);
      (void)hipGetLastError();
      return (err == int(hipErrorOutOfMemory)) ? int(OHMHIP_ERR_CAPACITY) : err;
    }
  }
  const uint64_t evictions_before = m->evictions;
  if (to_evict)
  {
    // in the old layout: the records are rewritten with all the others below
    OHMHIP_CHECK(evictColdRegions(m, to_evict, to_evict));
  }

  const SlotArrays list_before = slotArrays(m->mc, m->pool);
  stage.exchange(m);
  {
    // U2: the added layers hold their clear value in every slot, assigned or not.
    int err = OHMHIP_OK;
    for (int l = 0; l < OHMHIP_LID_COUNT && !err; ++l)
    {
      if (added & OHMHIP_LAYER_BIT(l))
      {
        err = clearSlots(m, m->pool, 0, m->pool.slot_capacity, s, ~0u, m->pool.layers[l].get());
      }
    }
    err = err ? err : int(hipStreamSynchronize(s));
    err = err ? err : int(hipGetLastError());
    err = err ? err : relayoutStore(m, list_before);
    if (err)
    {
      stage.exchange(m);
      return err;
    }
  }

  // Nothing below fails short of a device error.
  if (discard)
  {
    // U9, as ohmhip_map_clear: no region, no stored region, every slot pristine.
    for (auto &entry : m->spilled)
    {
      releaseStoreRecord(m, entry.second.record);
    }
    m->spilled.clear();
    m->region_slots.clear();
    m->slot_keys_host.clear();
    m->clearance_layer.regions.clear();
    OHMHIP_CHECK(clearSlots(m, m->pool, 0, m->pool.slot_capacity, s));
    OHMHIP_CHECK(hipMemsetAsync(m->pool.d_slot_keys, 0, sizeof(uint64_t) * m->pool.slot_capacity, s));
    OHMHIP_CHECK(commitSlotTable(m, 0));
  }
  if ((before ^ layers) & OHMHIP_LAYER_BIT(OHMHIP_LID_CLEARANCE))
  {
    // U6: a layer just added was never computed, one just removed has nothing to remember
    m->clearance_layer.regions.clear();
    m->clearance_layer.param_sets.clear();
    m->clearance_layer.epoch = 0;
  }
  m->spec_bucket_ok = false;  // (the next batch decides its route from the set in force)
  // U5: the pool keeps its slots; of them the batches use what the limit is worth under the new set
  m->resident_cap = (m->memory_limit && budget_after.regions < m->pool.slot_capacity) ? uint32_t(budget_after.regions) : 0u;
  if (stats)
  {
    stats->layers_before = before;
    stats->layers_after = layers;
    stats->regions_resident = m->slots_committed;
    stats->regions_in_store = m->spilled.size();
    stats->regions_evicted = m->evictions - evictions_before;
    stats->bytes_per_region_before = budget_before.per_region;
    stats->bytes_per_region_after = budget_after.per_region;
  }
  return OHMHIP_OK;
}
}  // namespace

extern "C" {

int ohmhip_map_update_layers(ohmhip_map_t m, unsigned layers, unsigned flags, ohmhip_layer_change_stats *stats)
try
{
  if (stats)
  {
    std::memset(stats, 0, sizeof(*stats));
  }
  if (!m || layers == 0u || (layers >> OHMHIP_LID_COUNT) != 0u || (flags & ~OHMHIP_LAYOUT_DISCARD_MAP) != 0u)
  {
    return OHMHIP_ERR_INVALID_ARG;  // U8
  }
  OHMHIP_SETTLE(m);  // U1: what was presented runs under the set it was presented under
  const int err = updateLayers(m, layers, flags, stats);
  if (err && stats)
  {
    std::memset(stats, 0, sizeof(*stats));
  }
  return err;
}
OHMHIP_ABI_CATCH

int ohmhip_map_layers(ohmhip_map_t m, unsigned *layers)
try
{
  if (!m || !layers)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  *layers = m->config.layers;
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_LAYOUT_IMPL_H
