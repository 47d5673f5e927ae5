// slot_state.h -- what a pool slot holds and how the region table is put back together: the one list of the persistent
// per-slot arrays with the movers built on it (pool to pool, slot to slot, slot to store record and back), the table
// commit, the residency budget, the consumers of the dirty bits and the slot index lists.
//
// Part of ohmhip_map.hip's translation unit (included there, in order): not a stand-alone header.
#ifndef OHMHIP_SLOT_STATE_H
#define OHMHIP_SLOT_STATE_H

namespace
{
/// One persistent per-slot array of a region pool.
struct SlotArray
{
  /// Where the slot's part goes when its region is spilled to the host store.
  enum Travel : unsigned
  {
    kInRecord = 1u,         ///< in the store record, at `record_offset`
    kInSpilledRegion = 2u,  ///< as a member of ohmhip_map_s::SpilledRegion (the small words a batch's set-up pass writes)
    kNever = 4u,            ///< merge base: merging maps do not spill
  };
  char *base;
  size_t stride;        ///< bytes per slot
  uint32_t clear_word;  ///< what every 32-bit word of an unassigned slot holds
  Travel travel;
  size_t record_offset;
};

struct SlotArrays
{
  SlotArray a[OHMHIP_LID_COUNT + 4];
  size_t n = 0;
  const SlotArray *begin() const { return a; }
  const SlotArray *end() const { return a + n; }
};

/// Bytes per slot of the replica-merge base (merge_impl.h): a copy of the occupancy layer.
inline size_t mergeBaseStride(const MapConst &mc) { return sizeof(float) * size_t(mc.region_voxels); }

/// THE list of the state that belongs to a slot and persists between batches: every mover below walks it, and nothing
/// else knows the strides and clear values.  Not in it: the slot keys, which are the region table itself
/// (commitSlotTable), and the per-batch scratch -- d_miss_counts, d_voxel_first_hit, d_traversal_acc, the hit ranges,
/// the chunk list and everything sized by the hash -- which is zero between batches and does not move.
/// bytesPerRegionAllLayers counts both kinds.
SlotArrays slotArrays(const MapConst &mc, const ohmhip_map_s::RegionPool &pool)
{
  const size_t rv = size_t(mc.region_voxels);
  SlotArrays list;
  size_t at = 0;  // (records: every part starts on a 256-byte boundary, the mask row follows the layers)
  auto add = [&](void *base, size_t stride, uint32_t clear_word, SlotArray::Travel travel) {
    list.a[list.n++] = SlotArray{ static_cast<char *>(base), stride, clear_word, travel, at };
    at += (travel == SlotArray::kInRecord) ? (stride + 255) & ~size_t(255) : 0;
  };
  for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
  {
    if (pool.layers[l])
    {
      // Occupancy clears to +inf == unobserved (ohm/DefaultLayer.cpp:87-91, ohm/VoxelOccupancy.h:42-45), clearance to
      // -1 (:174-193).
      add(pool.layers[l].get(), rv * kLayerBytes[l], layerClearWord(l), SlotArray::kInRecord);
    }
  }
  // The per-voxel mask is persistent state for NDT / TSDF (voxels that take the ordered replay path).
  add(pool.d_hit_mask.get(), ((rv + 31) / 32) * sizeof(uint32_t), 0u, SlotArray::kInRecord);
  add(pool.d_dirty.get(), sizeof(uint32_t), 0u, SlotArray::kInSpilledRegion);
  add(pool.d_last_use.get(), 2 * sizeof(uint32_t), 0u, SlotArray::kInSpilledRegion);
  if (pool.d_merge_base)
  {
    // replica-merge base (merge_impl.h): a new region's base is "unobserved"
    add(pool.d_merge_base.get(), mergeBaseStride(mc), 0x7f800000u, SlotArray::kNever);
  }
  return list;
}

/// Allocate the blocks of the layers in `layers` (a mask of OHMHIP_LAYER_BIT) in `pool`, `capacity` slots each (contents
/// undefined): a pool being built, or the layers a live pool is about to gain (layout_impl.h).
int allocLayerArrays(ohmhip_map_t m, ohmhip_map_s::RegionPool &pool, uint32_t capacity, unsigned layers)
{
  const size_t rv = size_t(m->mc.region_voxels);
  for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
  {
    if (layers & (1u << l))
    {
      OHMHIP_CHECK(pool.layers[l].alloc(std::max<size_t>(rv * kLayerBytes[l] * capacity, 4)));
    }
  }
  return OHMHIP_OK;
}

/// Allocate the arrays of the list in a pool being built, `capacity` slots each (the list's strides; contents undefined).
int allocSlotArrays(ohmhip_map_t m, ohmhip_map_s::RegionPool &pool, uint32_t capacity, bool merge_base)
{
  const size_t rv = size_t(m->mc.region_voxels);
  OHMHIP_CHECK(allocLayerArrays(m, pool, capacity, m->config.layers));
  OHMHIP_CHECK(pool.d_hit_mask.alloc(std::max<size_t>(((rv + 31) / 32) * sizeof(uint32_t) * capacity, 4)));
  OHMHIP_CHECK(pool.d_dirty.alloc(std::max<size_t>(sizeof(uint32_t) * capacity, 4)));
  OHMHIP_CHECK(pool.d_last_use.alloc(std::max<size_t>(2 * sizeof(uint32_t) * capacity, 4)));
  if (merge_base)
  {
    OHMHIP_CHECK(pool.d_merge_base.alloc(std::max<size_t>(mergeBaseStride(m->mc) * capacity, 4)));
  }
  return OHMHIP_OK;
}

size_t bytesPerRegionAllLayers(const ohmhip_map_config &c, int region_voxels)
{
  size_t b = 0;
  for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
  {
    if (c.layers & (1u << l))
    {
      b += kLayerBytes[l] * size_t(region_voxels);
    }
  }
  // + miss count layer + hit mask
  b += 4 * size_t(region_voxels) + size_t((region_voxels + 31) / 32) * 4;
  // + first-sample table (occupancy mode), traversal accumulator (traversal layer)
  b += (c.mode == OHMHIP_MODE_OCCUPANCY) ? 4 * size_t(region_voxels) : 0;
  b += (c.layers & (1u << OHMHIP_LID_TRAVERSAL)) ? 8 * size_t(region_voxels) : 0;
  return b;
}

/// The first `n` slots of pool `from` into the same slots of pool `to` (a pool being built beside the one in use).
int copySlots(ohmhip_map_t m, const ohmhip_map_s::RegionPool &from, const ohmhip_map_s::RegionPool &to, uint32_t n,
              hipStream_t stream)
{
  if (n == 0)
  {
    return OHMHIP_OK;
  }
  const SlotArrays src = slotArrays(m->mc, from), dst = slotArrays(m->mc, to);
  if (src.n != dst.n)
  {
    return OHMHIP_ERR_INTERNAL;
  }
  for (size_t i = 0; i < dst.n; ++i)
  {
    OHMHIP_CHECK(hipMemcpyAsync(dst.a[i].base, src.a[i].base, dst.a[i].stride * n, hipMemcpyDeviceToDevice, stream));
  }
  return OHMHIP_OK;
}

/// Slots [first, first + count) of `pool` go back to the pristine state every unassigned slot is in -- all of it, or
/// only the arrays whose Travel is in `which`.
/// `only_base`, where not null: only the array that starts there (a layer a live pool has just gained: layout_impl.h).
int clearSlots(ohmhip_map_t m, const ohmhip_map_s::RegionPool &pool, uint32_t first, uint32_t count, hipStream_t stream,
               unsigned which = ~0u, const void *only_base = nullptr)
{
  for (const SlotArray &a : slotArrays(m->mc, pool))
  {
    const size_t bytes = a.stride * count;
    if (bytes == 0 || !(a.travel & which) || (only_base && a.base != only_base))
    {
      continue;
    }
    if (a.clear_word != 0u)
    {
      hipLaunchKernelGGL(k_fill_u32, dim3(2048), dim3(256), 0, stream, reinterpret_cast<uint32_t *>(a.base + a.stride * first),
                         a.clear_word, bytes / 4);
    }
    else
    {
      OHMHIP_CHECK(hipMemsetAsync(a.base + a.stride * first, 0, bytes, stream));
    }
  }
  return OHMHIP_OK;
}

/// Copy jobs that move everything slot `src` holds into slot `dst` of the same pool (compaction).
void appendSlotMoveJobs(ohmhip_map_t m, uint32_t src, uint32_t dst, std::vector<CopyJob> &jobs)
{
  for (const SlotArray &a : slotArrays(m->mc, m->pool))
  {
    jobs.push_back(CopyJob{ a.base + a.stride * src, a.base + a.stride * dst, a.stride });
  }
}

/// The replay mask row is transient in occupancy mode (empty between batches): it is zeroed in a record, not copied,
/// and not copied back.
inline bool transientInRecord(ohmhip_map_t m, const SlotArray &a)
{
  return m->config.mode == OHMHIP_MODE_OCCUPANCY && a.base == reinterpret_cast<char *>(m->pool.d_hit_mask.get());
}

/// Copy jobs that move slot `slot`'s block of every layer (+ its replay mask row where that is persistent state) into
/// store record `record`.
void appendSlotToRecordJobs(ohmhip_map_t m, uint32_t slot, char *record, std::vector<CopyJob> &jobs)
{
  for (const SlotArray &a : slotArrays(m->mc, m->pool))
  {
    if (a.travel != SlotArray::kInRecord)
    {
      continue;
    }
    if (transientInRecord(m, a))
    {
      std::memset(record + a.record_offset, 0, a.stride);
    }
    else
    {
      jobs.push_back(CopyJob{ a.base + a.stride * slot, record + a.record_offset, a.stride });
    }
  }
}

/// ... and back: `record` into slot `slot` (which holds a fresh, unobserved region).
void appendRecordToSlotJobs(ohmhip_map_t m, const char *record, uint32_t slot, std::vector<CopyJob> &jobs)
{
  for (const SlotArray &a : slotArrays(m->mc, m->pool))
  {
    if (a.travel == SlotArray::kInRecord && !transientInRecord(m, a))
    {
      jobs.push_back(CopyJob{ record + a.record_offset, a.base + a.stride * slot, a.stride });
    }
  }
}

/// The host store's record layout for this map's layer set: where read_side.h and region_io.h find a layer's block.
/// (A layer the map does not hold gets the offset of what follows it: nothing reads it.)
void layoutStoreRecord(ohmhip_map_t m)
{
  ohmhip_map_s::HostStore &st = m->store;
  const SlotArrays list = slotArrays(m->mc, m->pool);
  size_t i = 0;
  for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
  {
    st.layer_offset[l] = list.a[i].record_offset;
    i += m->pool.layers[l] ? 1 : 0;
  }
  st.mask_offset = list.a[i].record_offset;  // (the mask row follows the layers in the list)
  st.mask_bytes = list.a[i].stride;
  st.record_bytes = st.mask_offset + ((st.mask_bytes + 255) & ~size_t(255));
}

RegionTable regionTable(ohmhip_map_t m)
{
  RegionTable rt;
  rt.keys = m->pool.d_keys;
  rt.vals = m->pool.d_vals;
  rt.slot_keys = m->pool.d_slot_keys;
  rt.n_slots = m->d_n_slots;
  rt.hash_mask = m->pool.hash_capacity - 1;
  rt.slot_capacity = m->pool.slot_capacity;
  return rt;
}

__global__ void k_rehash(RegionTable rt, uint32_t n)
{
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n)
  {
    return;
  }
  const uint64_t key = rt.slot_keys[slot];
  uint32_t idx = hashRegionKey(key, rt.hash_mask);
  while (true)
  {
    const unsigned long long prev = atomicCAS(&rt.keys[idx], 0ull, (unsigned long long)key);
    if (prev == 0)
    {
      rt.vals[idx] = slot;
      return;
    }
    idx = (idx + 1) & rt.hash_mask;
  }
}

/// The region table becomes the first `n` slot keys: the hash is rebuilt from them (cheap: one lane per region), the
/// device's slot count and the committed count follow.  Returns with the compute stream drained.  Whatever else a
/// caller resets -- d_vals and the batch scratch after a failed batch, the slot keys themselves after a compaction --
/// it queues first.
int commitSlotTable(ohmhip_map_t m, uint32_t n)
{
  hipStream_t s = m->stream;
  OHMHIP_CHECK(hipMemsetAsync(m->pool.d_keys, 0, sizeof(unsigned long long) * m->pool.hash_capacity, s));
  OHMHIP_CHECK(hipMemcpyAsync(m->d_n_slots, &n, sizeof(uint32_t), hipMemcpyHostToDevice, s));
  if (n)
  {
    hipLaunchKernelGGL(k_rehash, dim3((n + 255) / 256), dim3(256), 0, s, regionTable(m), n);
  }
  OHMHIP_CHECK(hipStreamSynchronize(s));
  OHMHIP_CHECK(hipGetLastError());
  m->slots_committed = n;
  return OHMHIP_OK;
}

/// Largest region pool the 20-bit slot field of the sample / event sort keys can address.
constexpr uint32_t kMaxRegionSlots = (1u << 20) - 2u;

/// What a region costs and how many the pool may hold: the memory limit's worth (at most what the sort keys can
/// address), or the pool's capacity when there is no limit.
struct PoolBudget
{
  uint64_t per_region;
  uint64_t regions;
};
PoolBudget poolBudget(ohmhip_map_t m)
{
  const uint64_t per_region = bytesPerRegionAllLayers(m->config, m->mc.region_voxels);
  return { per_region,
           m->memory_limit ? std::min<uint64_t>(m->memory_limit / per_region, kMaxRegionSlots) : m->pool.slot_capacity };
}

/// fn(packed key) for every region whose dirty word has `bit` set (0: every region), the resident regions in slot
/// order and then the ones in the host store: one download of the committed slots' flags.  The caller has drained the
/// compute stream and refreshed the host mirror of the region table.
template <typename Fn>
int forEachDirtyRegion(ohmhip_map_t m, uint32_t bit, Fn fn)
{
  std::vector<uint32_t> dirty(bit ? m->slots_committed : 0u);
  if (!dirty.empty())
  {
    OHMHIP_CHECK(hipMemcpy(dirty.data(), m->pool.d_dirty, sizeof(uint32_t) * dirty.size(), hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < m->slot_keys_host.size(); ++i)
  {
    if (!bit || (dirty[i] & bit))
    {
      fn(m->slot_keys_host[i]);
    }
  }
  for (const auto &entry : m->spilled)
  {
    if (!bit || (entry.second.dirty & bit))
    {
      fn(entry.first);
    }
  }
  return OHMHIP_OK;
}

/// Clear `bit` in every region's dirty word, in the pool (queued on the compute stream) and in the host store.
void clearDirtyBit(ohmhip_map_t m, uint32_t bit)
{
  hipLaunchKernelGGL(k_and_u32, dim3(256), dim3(256), 0, m->stream, m->pool.d_dirty, ~bit, size_t(m->pool.slot_capacity));
  for (auto &entry : m->spilled)
  {
    entry.second.dirty &= ~bit;
  }
}

/// A list of slot indices goes into the map's index scratch (merge_slots) for one of the small kernels below, which the
/// caller queues on `stream`.  `blocking`: the list may go out of scope before the stream gets to the copy.
int uploadSlotIndex(ohmhip_map_t m, const uint32_t *slots, size_t count, hipStream_t stream, bool blocking,
                    const uint32_t *&d_index)
{
  OHMHIP_CHECK(m->merge_slots.ensure(sizeof(uint32_t) * count, false, stream));
  if (blocking)
  {
    OHMHIP_CHECK(hipMemcpy(m->merge_slots.ptr, slots, sizeof(uint32_t) * count, hipMemcpyHostToDevice));
  }
  else
  {
    OHMHIP_CHECK(hipMemcpyAsync(m->merge_slots.ptr, slots, sizeof(uint32_t) * count, hipMemcpyHostToDevice, stream));
  }
  d_index = static_cast<const uint32_t *>(m->merge_slots.ptr);
  return OHMHIP_OK;
}

/// The listed slots are in use now: the stamp of the batch being attempted.
inline void stampSlotsUsedNow(ohmhip_map_t m, const uint32_t *d_index, size_t count, hipStream_t stream)
{
  hipLaunchKernelGGL(k_touch_use_at, dim3(64), dim3(256), 0, stream, m->pool.d_last_use, d_index, count, uint32_t(m->batch_seq + 1u));
}

/// OR `bits` into the listed slots' dirty words (atomically: k_plan may be OR-ing a batch's bits into the same words).
inline void orSlotBits(ohmhip_map_t m, const uint32_t *d_index, size_t count, uint32_t bits, hipStream_t stream)
{
  hipLaunchKernelGGL(k_or_at_u32, dim3(64), dim3(256), 0, stream, m->pool.d_dirty, d_index, count, bits);
}
}  // namespace

#endif  // OHMHIP_SLOT_STATE_H
