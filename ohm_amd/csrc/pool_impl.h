// pool_impl.h -- the region pool: per-batch scratch views, pool allocation / growth / roll-back, the host mirror of the
// region table, the pinned host store's records, copy jobs, LDS sizing, value configuration.
//
// Part of ohmhip_map.hip's translation unit (included there, in order): not a stand-alone header.
#ifndef OHMHIP_POOL_IMPL_H
#define OHMHIP_POOL_IMPL_H

namespace
{
BatchScratch batchScratch(ohmhip_map_t m)
{
  // The counters a batch's set-up pass writes exist twice (allocPool makes the arrays twice as long): batch N+1 sets up
  // in the other half while batch N's walk / apply kernels still read theirs.
  const size_t h = size_t(m->parity) * m->pool.hash_capacity;
  const size_t c = size_t(m->parity) * m->pool.slot_capacity;
  BatchScratch bs;
  bs.seg_count = m->pool.d_seg_count + h;
  bs.seg_cursor = m->pool.d_seg_cursor + h;
  bs.seg_offset = m->pool.d_seg_offset + h;
  bs.touched_flag = m->pool.d_touched_flag + h;
  bs.touched = m->pool.d_touched + h;
  bs.hit_count = m->pool.d_hit_count + h;
  // (three lists per parity in one allocation: regions receiving samples, regions whose counts / whose samples the apply
  // kernels still have to process -- k_plan)
  bs.sort_list = m->pool.d_sort_list + 3 * h;
  bs.apply_counts_list = bs.sort_list + m->pool.hash_capacity;
  bs.apply_hits_list = bs.sort_list + 2 * size_t(m->pool.hash_capacity);
  bs.voxel_first_hit = m->pool.d_voxel_first_hit;
  bs.hit_begin = m->pool.d_hit_begin + c;
  bs.hit_end = m->pool.d_hit_end + c;
  bs.dirty = m->pool.d_dirty;
  bs.last_use = m->pool.d_last_use;
  bs.stamp = uint32_t(m->batch_seq + 1u);
  bs.info = m->d_info + m->info_index;
  bs.wg_regions = static_cast<WgRegion *>(m->wg_regions[m->parity].ptr);
  bs.wg_region_count = static_cast<uint32_t *>(m->wg_region_count[m->parity].ptr);
  return bs;
}

inline Chunk *batchChunks(ohmhip_map_t m) { return m->pool.d_chunks + size_t(m->parity) * m->pool.chunk_capacity; }
inline uint32_t *batchEventCount(ohmhip_map_t m) { return m->d_event_count + 4u * m->parity; }
inline DevBuf &batchWalks(ohmhip_map_t m) { return m->walks_buf[m->parity]; }

uint32_t nextPow2(uint32_t v)
{
  uint32_t p = 1;
  while (p < v)
  {
    p <<= 1;
  }
  return p;
}

/// The scratch that goes with the traversal layer, zeroed (queued on `s`): in a pool being built, or beside the layer
/// a live pool is about to gain (layout_impl.h).
int allocTraversalAcc(ohmhip_map_t m, ohmhip_map_s::RegionPool &pool, uint32_t capacity, hipStream_t s)
{
  const size_t bytes = std::max<size_t>(sizeof(unsigned long long) * size_t(m->mc.region_voxels) * capacity, 4);
  OHMHIP_CHECK(pool.d_traversal_acc.alloc(bytes));
  OHMHIP_CHECK(hipMemsetAsync(pool.d_traversal_acc, 0, bytes, s));
  return OHMHIP_OK;
}

/// (Re)allocate the region pool for `capacity` regions, preserving the first `keep` slots' contents.  Everything new is
/// allocated before anything old is released: a failed allocation leaves the map exactly as it was.  `keep` is the
/// committed slot count at every caller (or the count it is about to commit: 0, in ohmhip_map_clear), so the table
/// commit at the end may set slots_committed like every other commit does.
int allocPool(ohmhip_map_t m, uint32_t capacity, uint32_t keep)
{
  const size_t rv = size_t(m->mc.region_voxels);
  hipStream_t s = m->stream;
  if (!m->precleaned.empty() || !m->stale_records.empty())
  {
    OHMHIP_CHECK(drainWriteBack(m));  // background write-back copies read the pool being replaced
  }

  const ohmhip_map_s::RegionPool &old = m->pool;
  ohmhip_map_s::RegionPool fresh;  // releases itself if any step fails
  fresh.slot_capacity = capacity;
  fresh.hash_capacity = nextPow2(std::max<uint32_t>(1024u, capacity * 2u));
  fresh.chunk_capacity = capacity + (1u << 16);
  const size_t hash_cap = fresh.hash_capacity;
  auto zalloc = [&](auto &array, size_t bytes) -> int {
    OHMHIP_CHECK(array.alloc(std::max<size_t>(bytes, 4)));
    OHMHIP_CHECK(hipMemsetAsync(array, 0, std::max<size_t>(bytes, 4), s));
    return OHMHIP_OK;
  };
  auto build = [&]() -> int {
    // The persistent per-slot state (slot_state.h): the kept slots' content, the rest pristine.
    OHMHIP_CHECK(allocSlotArrays(m, fresh, capacity, bool(old.d_merge_base)));
    OHMHIP_CHECK(copySlots(m, old, fresh, keep, s));
    OHMHIP_CHECK(clearSlots(m, fresh, keep, capacity - keep, s));
    // The table: the kept slots' keys (the hash is rebuilt from them below: commitSlotTable clears d_keys).
    OHMHIP_CHECK(zalloc(fresh.d_slot_keys, sizeof(uint64_t) * capacity));
    if (keep && old.d_slot_keys)
    {
      OHMHIP_CHECK(hipMemcpyAsync(fresh.d_slot_keys, old.d_slot_keys, sizeof(uint64_t) * keep, hipMemcpyDeviceToDevice, s));
    }
    OHMHIP_CHECK(fresh.d_keys.alloc(sizeof(unsigned long long) * hash_cap));
    OHMHIP_CHECK(zalloc(fresh.d_vals, sizeof(uint32_t) * hash_cap));
    // The per-batch scratch: zero between batches.
    OHMHIP_CHECK(zalloc(fresh.d_seg_count, sizeof(uint32_t) * 2 * hash_cap));
    OHMHIP_CHECK(zalloc(fresh.d_seg_cursor, sizeof(uint32_t) * 2 * hash_cap));
    OHMHIP_CHECK(zalloc(fresh.d_hit_count, sizeof(uint32_t) * 2 * hash_cap));
    OHMHIP_CHECK(zalloc(fresh.d_sort_list, sizeof(uint32_t) * 6 * hash_cap));  // (3 lists x 2 parities)
    OHMHIP_CHECK(zalloc(fresh.d_seg_offset, sizeof(uint32_t) * 2 * hash_cap));
    OHMHIP_CHECK(zalloc(fresh.d_touched_flag, sizeof(uint32_t) * 2 * hash_cap));
    OHMHIP_CHECK(zalloc(fresh.d_touched, sizeof(uint32_t) * 2 * hash_cap));
    if (m->config.mode == OHMHIP_MODE_OCCUPANCY)
    {
      OHMHIP_CHECK(zalloc(fresh.d_voxel_first_hit, sizeof(uint32_t) * rv * capacity));
    }
    OHMHIP_CHECK(zalloc(fresh.d_hit_begin, sizeof(uint32_t) * 2 * capacity));
    OHMHIP_CHECK(zalloc(fresh.d_hit_end, sizeof(uint32_t) * 2 * capacity));
    OHMHIP_CHECK(zalloc(fresh.d_miss_counts, sizeof(uint32_t) * rv * capacity));
    OHMHIP_CHECK(zalloc(fresh.d_chunks, sizeof(Chunk) * 2 * fresh.chunk_capacity));
    if (m->config.layers & (1u << OHMHIP_LID_TRAVERSAL))
    {
      OHMHIP_CHECK(allocTraversalAcc(m, fresh, capacity, s));
    }
    OHMHIP_CHECK(hipStreamSynchronize(s));
    return OHMHIP_OK;
  };
  const int build_err = build();
  if (build_err)
  {
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    return (build_err == int(hipErrorOutOfMemory)) ? int(OHMHIP_ERR_CAPACITY) : build_err;
  }

  m->pool = std::move(fresh);  // (releases the old pool)
  return commitSlotTable(m, keep);
}

/// Pool capacity for `needed` regions: doubling, clamped to what the sort keys can address.  False when `needed` itself
/// is beyond that (the caller reports OHMHIP_ERR_CAPACITY: a larger slot would be truncated in the keys and alias
/// another region).
bool grownCapacity(uint32_t current, uint32_t needed, uint32_t &capacity)
{
  if (needed > kMaxRegionSlots)
  {
    return false;
  }
  uint64_t cap = std::max<uint32_t>(current, 1u);
  while (cap < needed)
  {
    cap *= 2;
  }
  capacity = uint32_t(std::min<uint64_t>(cap, kMaxRegionSlots));
  return true;
}

/// Forget the regions a failed write_regions / ensure_regions call added to the host table.
void dropHostRegions(ohmhip_map_t m, size_t keep)
{
  for (size_t i = keep; i < m->slot_keys_host.size(); ++i)
  {
    m->region_slots.erase(m->slot_keys_host[i]);
  }
  m->slot_keys_host.resize(keep);
}

/// Forget what a failed batch's set-up pass left in the region table and the per-batch scratch, without touching the
/// pool: the hash is rebuilt from the committed slots.  (Used when the pool may not grow.)
int rollbackTable(ohmhip_map_t m)
{
  hipStream_t s = m->stream;
  const size_t hash_words = m->pool.hash_capacity;
  OHMHIP_CHECK(hipStreamSynchronize(s));
  OHMHIP_CHECK(hipMemsetAsync(m->pool.d_vals, 0, sizeof(uint32_t) * hash_words, s));
  uint32_t *per_hash[] = { m->pool.d_seg_count,  m->pool.d_seg_cursor,   m->pool.d_hit_count, m->pool.d_seg_offset,
                           m->pool.d_touched_flag, m->pool.d_touched };
  for (uint32_t *p : per_hash)
  {
    OHMHIP_CHECK(hipMemsetAsync(p, 0, sizeof(uint32_t) * 2 * hash_words, s));  // (both parities)
  }
  OHMHIP_CHECK(hipMemsetAsync(m->pool.d_sort_list, 0, sizeof(uint32_t) * 6 * hash_words, s));  // (3 lists x 2 parities)
  const uint32_t keep = m->slots_committed;
  if (m->pool.slot_capacity > keep)
  {
    OHMHIP_CHECK(hipMemsetAsync(m->pool.d_slot_keys + keep, 0, sizeof(uint64_t) * (m->pool.slot_capacity - keep), s));
    // the slots the failed batch handed out go back to the pristine state: no modified flags, no use stamp (its set-up
    // pass wrote nothing else of theirs)
    OHMHIP_CHECK(clearSlots(m, m->pool, keep, m->pool.slot_capacity - keep, s, SlotArray::kInSpilledRegion));
  }
  OHMHIP_CHECK(hipMemsetAsync(m->d_info, 0, 3 * sizeof(BatchInfo), s));
  m->info_clean = false;
  m->spec_bucket_ok = false;
  return commitSlotTable(m, keep);
}

/// Grow the pool so that it holds `needed` regions, keeping the first `keep` slots -- and `wish` regions where the
/// budget allows: a batch that overflowed the pool wishes for double the pool (amortised growth), regions created by
/// name for what they need.  Refused, in this order, when `needed` is beyond the slot field of the sort keys, beyond
/// the map's memory limit (the largest pool the limit allows is still tried when the wish overshoots it), or when the
/// new pool does not fit in free device memory.
int growPool(ohmhip_map_t m, uint32_t needed, uint32_t wish, uint32_t keep)
{
  uint32_t cap = 0;
  if (!grownCapacity(m->pool.slot_capacity, needed, cap))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  uint32_t wished_cap = cap;
  if (grownCapacity(m->pool.slot_capacity, std::max(needed, std::min(wish, kMaxRegionSlots)), wished_cap))
  {
    cap = wished_cap;
  }
  const PoolBudget budget = poolBudget(m);
  if (m->memory_limit)
  {
    if (budget.regions < needed)
    {
      return OHMHIP_ERR_CAPACITY;
    }
    cap = uint32_t(std::min<uint64_t>(cap, budget.regions));
  }
  size_t free_b = 0, total_b = 0;
  OHMHIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (budget.per_region * cap > free_b)
  {
    return OHMHIP_ERR_CAPACITY;
  }
  ++m->cache_full;
  return allocPool(m, cap, keep);
}

int refreshHostRegionTable(ohmhip_map_t m)
{
  const uint32_t n = m->slots_committed;
  if (m->slot_keys_host.size() == n)
  {
    return OHMHIP_OK;
  }
  const size_t old = m->slot_keys_host.size();
  m->slot_keys_host.resize(n);
  if (n > old)
  {
    OHMHIP_CHECK(hipMemcpy(m->slot_keys_host.data() + old, m->pool.d_slot_keys + old, sizeof(uint64_t) * (n - old),
                           hipMemcpyDeviceToHost));
    for (size_t i = old; i < n; ++i)
    {
      m->region_slots[m->slot_keys_host[i]] = uint32_t(i);
    }
  }
  return OHMHIP_OK;
}

int ensureStage(ohmhip_map_t m, size_t bytes)
{
  if (bytes <= m->h_stage_bytes)
  {
    return OHMHIP_OK;
  }
  m->h_stage_bytes = 0;
  OHMHIP_CHECK(m->h_stage.alloc(bytes, hipHostMallocDefault));
  m->h_stage_bytes = bytes;
  return OHMHIP_OK;
}

/// Lay out the host store's records for this map's layer set (once) and make sure at least `records` are free.
int reserveStoreRecords(ohmhip_map_t m, size_t records)
{
  ohmhip_map_s::HostStore &st = m->store;
  if (st.record_bytes == 0)
  {
    layoutStoreRecord(m);
  }
  while (st.free_records.size() < records)
  {
    // slabs of about 64 MiB, at least the shortfall (one pinning call for a large reservation)
    const size_t want = std::max<size_t>(records - st.free_records.size(), (size_t(64) << 20) / st.record_bytes + 1);
    PinnedBuf<void> slab;
    if (slab.alloc(want * st.record_bytes, hipHostMallocDefault) != hipSuccess)
    {
      (void)hipGetLastError();
      return OHMHIP_ERR_CAPACITY;
    }
    for (size_t i = 0; i < want; ++i)
    {
      st.free_records.push_back(static_cast<char *>(slab.get()) + i * st.record_bytes);
    }
    st.slabs.push_back(std::move(slab));
    st.records_total += want;
  }
  return OHMHIP_OK;
}

char *takeStoreRecord(ohmhip_map_t m)
{
  if (m->store.free_records.empty() && reserveStoreRecords(m, 1) != OHMHIP_OK)
  {
    return nullptr;
  }
  char *rec = m->store.free_records.back();
  m->store.free_records.pop_back();
  return rec;
}

void releaseStoreRecord(ohmhip_map_t m, char *record)
{
  if (record)
  {
    m->store.free_records.push_back(record);
  }
}

/// Run a list of byte copies as one kernel on `stream` (k_copy_jobs); returns with the launch queued.
int launchCopyJobs(ohmhip_map_t m, const std::vector<CopyJob> &jobs, hipStream_t stream)
{
  if (jobs.empty())
  {
    return OHMHIP_OK;
  }
  OHMHIP_CHECK(m->copy_jobs.ensure(sizeof(CopyJob) * jobs.size(), false, stream));
  OHMHIP_CHECK(hipMemcpy(m->copy_jobs.ptr, jobs.data(), sizeof(CopyJob) * jobs.size(), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_copy_jobs, dim3(uint32_t(jobs.size()) * kCopyBlocksPerJob), dim3(256), 0, stream,
                     static_cast<const CopyJob *>(m->copy_jobs.ptr), uint32_t(jobs.size()));
  return hipGetLastError();
}

/// Highest key bit the sorts need: the slot field only uses log2(slots) + 1 bits (invalid keys are all ones).  `slots`:
/// the pool's capacity when sizing buffers, the slots actually in use when sorting (fewer 8-bit passes for a map that
/// occupies a small part of a large pool).
unsigned sortEndBit(uint32_t slots)
{
  unsigned bits = 1;
  while ((1u << bits) <= slots)
  {
    ++bits;
  }
  return std::min<unsigned>(64u, unsigned(kHitSlotShift) + bits + 1u);
}
unsigned sortEndBit(ohmhip_map_t m) { return sortEndBit(m->pool.slot_capacity); }

/// rocPRIM falls back to a 20-launch merge sort for up to 2^20 keys by default; the one-sweep radix path is several
/// times faster on the 1M-key sample lists of a typical batch.
using SortConfig =
  rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, rocprim::default_config, size_t(1) << 15>;

constexpr size_t kDbgWords = 16 + size_t(kTraceChunks) * kTraceWords;

template <typename G>
size_t walkLdsBytesOf(const MapConst &mc, uint32_t chunk_segments)
{
  // [count tile, padded to 16 B][per-wave queues][staged sample keys][interval counters][cursor + pad]
  // [length histogram][segment order, u16 each]
  const size_t count_words = (size_t((mc.region_voxels + 1) / 2) + 31u) & ~size_t(31);  // whole 32-word rows (tileWord)
  return (count_words + size_t(2 * G::kWaves * G::kQueueCap) + size_t(2 * G::kLdsHits) + size_t(G::kLdsHits / 2) +
          kWalkCursorWords + 64 + (kIndexBuckets + 2) / 2 +
          kLengthClasses + (chunk_segments + 1) / 2) *
         sizeof(uint32_t);
}

size_t walkLdsBytes(const MapConst &mc, uint32_t chunk_segments, bool half = false)
{
  return half ? walkLdsBytesOf<WalkHalf>(mc, chunk_segments) : walkLdsBytesOf<WalkFull>(mc, chunk_segments);
}

__global__ void k_clear_counts(MapConst mc, RegionTable rt, BatchScratch bs, uint32_t *__restrict__ miss_counts)
{
  const uint32_t slot = rt.vals[bs.touched[blockIdx.x]];
  const size_t base = size_t(slot) * size_t(mc.region_voxels);
  for (uint32_t vi = threadIdx.x; vi < uint32_t(mc.region_voxels); vi += blockDim.x)
  {
    miss_counts[base + vi] = 0;
  }
}

/// One ray batch through the pipeline (all map modes).  d_rays: device pointer to 6 doubles per ray.
/// The value half of the configuration (probabilities, clamps, filter, NDT / TSDF parameters): everything a host map can
/// change between batches.  Geometry, mode and the layer set are fixed at creation.
void applyValueConfig(ohmhip_map_t m)
{
  MapConst &mc = m->mc;
  mc.hit_value = m->config.hit_value;
  mc.miss_value = m->config.miss_value;
  mc.threshold_value = m->config.threshold_value;
  mc.min_value = m->config.min_value;
  mc.max_value = m->config.max_value;
  // ohm/RayMapperOccupancy.cpp:92-93
  mc.sat_min = m->config.saturate_at_min ? mc.min_value : std::numeric_limits<float>::lowest();
  mc.sat_max = m->config.saturate_at_max ? mc.max_value : std::numeric_limits<float>::max();
  mc.filter_mode = m->config.ray_filter;
  mc.filter_range = m->config.ray_filter_range;
  mc.sensor_noise = m->config.ndt_sensor_noise;
  mc.sample_threshold = m->config.ndt_sample_threshold;
  mc.adaptation_rate = m->config.ndt_adaptation_rate;
  mc.reinit_threshold = m->config.ndt_reinit_threshold;
  mc.reinit_count = m->config.ndt_reinit_count;
  mc.initial_intensity_cov = m->config.ndt_initial_intensity_cov;
  mc.tsdf_max_weight = m->config.tsdf_max_weight;
  mc.tsdf_trunc = m->config.tsdf_trunc;
  mc.tsdf_dropoff = m->config.tsdf_dropoff;
  mc.tsdf_sparsity = m->config.tsdf_sparsity;

}

}  // namespace

#endif  // OHMHIP_POOL_IMPL_H
