// clearance_update.h -- the clearance layer (OHMHIP_LID_CLEARANCE) kept current: ClearanceProcess::update / updateRegion
// (ohmgpu/ClearanceProcess.cpp:418-470, 519-623) over the exact kernels of clearance_kernels.h.  Included at the end of
// ohmhip_map.hip.
//
// One update is four steps, each its own launch on the map's stream:
//  1. fold: the kDirtyClearance bit of every slot (set by k_plan, ohmhip_map_mark_dirty and the replica merge) and of
//     every host-store record becomes a change stamp of the region at a new epoch, and is cleared.  Host uploads and
//     removals stamp their regions when they happen (map_state.h: clearanceMarkChanged).
//  2. selection (k_clearance_stale): one lane per present region probes its neighbourhood -- every region key within
//     D_a = ceil(h / region_dim_a) on each axis, int16-wrapped as moveKey wraps -- in a table of change stamps.  The
//     region is stale when one of them is newer than its own last write, or when it was never written with these
//     parameters.  Lanes are in ascending (z, y, x) key order, the reference's cursor order, so the flags are the list.
//  3. compute: k_clearance_regions_lds / _global into staging, for the first `max_regions` stale regions.
//  4. scatter (k_copy_jobs): each present tile's part of a region's result into its layer block -- the pool slot, or the
//     pinned host-store record of a spilled tile (device visible: nothing is re-admitted; read_side.h: tileHome) --
//     then the sync mark.
// Tiles of a tiled region that hold no data yet are not created: they read -1 like any cleared block.
#ifndef OHMHIP_CLEARANCE_UPDATE_H
#define OHMHIP_CLEARANCE_UPDATE_H

struct ClearanceStaleArgs
{
  const unsigned long long *keys;  ///< open-addressing table of the regions with a change stamp (0: empty)
  const uint32_t *changed;         ///< their change stamps
  uint32_t mask;                   ///< table capacity - 1
  const unsigned long long *present;  ///< [n] the present regions, ascending (z, y, x)
  const uint32_t *written;         ///< [n] epoch each was computed at with the current parameters (0: never)
  uint32_t n;
  int reach[3];                    ///< D per axis
  uint8_t *stale;                  ///< [n] out
};

__global__ void __launch_bounds__(256) k_clearance_stale(ClearanceStaleArgs a)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n)
  {
    return;
  }
  const uint32_t written = a.written[i];
  bool stale = written == 0u;
  int16_t r[3];
  unpackRegionKey(a.present[i], r);
  for (int dz = -a.reach[2]; dz <= a.reach[2] && !stale; ++dz)
  {
    for (int dy = -a.reach[1]; dy <= a.reach[1] && !stale; ++dy)
    {
      for (int dx = -a.reach[0]; dx <= a.reach[0] && !stale; ++dx)
      {
        // (packRegionKey keeps the low 16 bits of each component: the int16 wrap of moveKey)
        const unsigned long long key = packRegionKey(int(r[0]) + dx, int(r[1]) + dy, int(r[2]) + dz);
        uint32_t idx = hashRegionKey(key, a.mask);
        for (;;)
        {
          const unsigned long long k = a.keys[idx];
          if (k == key)
          {
            stale = a.changed[idx] > written;
            break;
          }
          if (k == 0ull)
          {
            break;
          }
          idx = (idx + 1u) & a.mask;
        }
      }
    }
  }
  a.stale[i] = stale ? 1u : 0u;
}

namespace
{
/// 1 + the index of parameter set `p` among those the layer was ever computed with (the flags that do not change a
/// result are ignored).
uint32_t clearanceParamSet(ohmhip_map_t m, const ohmhip_clearance_params &p)
{
  auto &sets = m->clearance_layer.param_sets;
  const unsigned flags = p.flags & (OHMHIP_QF_UNKNOWN_AS_OCCUPIED | OHMHIP_QF_REPORT_UNSCALED);
  for (size_t i = 0; i < sets.size(); ++i)
  {
    const ohmhip_clearance_params &q = sets[i];
    if (q.search_radius == p.search_radius && q.axis_scaling[0] == p.axis_scaling[0] &&
        q.axis_scaling[1] == p.axis_scaling[1] && q.axis_scaling[2] == p.axis_scaling[2] && q.flags == flags)
    {
      return uint32_t(i + 1);
    }
  }
  sets.push_back(p);
  sets.back().flags = flags;
  return uint32_t(sets.size());
}

/// Step 1: the kDirtyClearance bits become change stamps at a new epoch.
int clearanceFold(ohmhip_map_t m)
{
  auto &cl = m->clearance_layer;
  OHMHIP_CHECK(hipStreamSynchronize(m->stream));
  OHMHIP_CHECK(refreshHostRegionTable(m));
  const uint32_t epoch = ++cl.epoch;
  bool any = false;
  OHMHIP_CHECK(forEachDirtyRegion(m, kDirtyClearance, [&](uint64_t key) {
    cl.regions[callerRegionKey(m, key)].changed = epoch;
    any = true;
  }));
  if (any)
  {
    clearDirtyBit(m, kDirtyClearance);
    OHMHIP_CHECK(hipGetLastError());
  }
  return OHMHIP_OK;
}

/// Steps 1 and 2: `present` the caller's regions present in the map (resident or in the host store), ascending
/// (z, y, x) as signed int16; `stale` their flags for parameter set `params`.
int clearanceSelect(ohmhip_map_t m, uint32_t params, int h, std::vector<uint64_t> &present, std::vector<uint8_t> &stale)
{
  OHMHIP_CHECK(clearanceFold(m));
  auto &cl = m->clearance_layer;
  hipStream_t s = m->stream;
  presentRegionOrders(m, present);  // (clearanceFold refreshed the host mirror of the region table)
  for (uint64_t &key : present)
  {
    int16_t r[3];
    regionOfOrder(key, r);
    key = packRegionKey(r);
  }
  const uint32_t n = uint32_t(present.size());
  stale.assign(n, 0);
  if (n == 0)
  {
    return OHMHIP_OK;
  }
  std::vector<uint32_t> written(n, 0u);
  for (uint32_t i = 0; i < n; ++i)
  {
    const auto it = cl.regions.find(present[i]);
    if (it != cl.regions.end() && it->second.params == params)
    {
      written[i] = it->second.written;
    }
  }
  uint32_t cap = 16;
  while (cap < 2 * cl.regions.size())
  {
    cap <<= 1;
  }
  std::vector<unsigned long long> keys(cap, 0ull);
  std::vector<uint32_t> changed(cap, 0u);
  for (const auto &entry : cl.regions)
  {
    if (entry.second.changed == 0)
    {
      continue;
    }
    uint32_t idx = hashRegionKey(entry.first, cap - 1);
    while (keys[idx] != 0)
    {
      idx = (idx + 1) & (cap - 1);
    }
    keys[idx] = entry.first;
    changed[idx] = entry.second.changed;
  }
  OHMHIP_CHECK(cl.table_keys.ensure(sizeof(unsigned long long) * cap, false, s));
  OHMHIP_CHECK(cl.table_changed.ensure(sizeof(uint32_t) * cap, false, s));
  OHMHIP_CHECK(cl.present.ensure(sizeof(unsigned long long) * n, false, s));
  OHMHIP_CHECK(cl.written.ensure(sizeof(uint32_t) * n, false, s));
  OHMHIP_CHECK(cl.stale.ensure(n, false, s));
  OHMHIP_CHECK(hipMemcpyAsync(cl.table_keys.ptr, keys.data(), sizeof(unsigned long long) * cap, hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(hipMemcpyAsync(cl.table_changed.ptr, changed.data(), sizeof(uint32_t) * cap, hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(hipMemcpyAsync(cl.present.ptr, present.data(), sizeof(unsigned long long) * n, hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(hipMemcpyAsync(cl.written.ptr, written.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
  ClearanceStaleArgs a;
  a.keys = static_cast<const unsigned long long *>(cl.table_keys.ptr);
  a.changed = static_cast<const uint32_t *>(cl.table_changed.ptr);
  a.mask = cap - 1;
  a.present = static_cast<const unsigned long long *>(cl.present.ptr);
  a.written = static_cast<const uint32_t *>(cl.written.ptr);
  a.n = n;
  for (int c = 0; c < 3; ++c)
  {
    a.reach[c] = (h + m->mc.kdim[c] - 1) / m->mc.kdim[c];
  }
  a.stale = static_cast<uint8_t *>(cl.stale.ptr);
  hipLaunchKernelGGL(k_clearance_stale, dim3((n + 255) / 256), dim3(256), 0, s, a);
  OHMHIP_CHECK(hipGetLastError());
  OHMHIP_CHECK(hipMemcpyAsync(stale.data(), cl.stale.ptr, n, hipMemcpyDeviceToHost, s));
  return hipStreamSynchronize(s);
}

/// Steps 3 and 4 for `keys` (caller regions present in the map): computed, written where each tile lives, marked for
/// syncVoxels, and recorded as up to date for parameter set `params` at the current epoch.
int clearanceProcess(ohmhip_map_t m, ClearanceArgs &a, const std::vector<uint64_t> &keys, uint32_t params)
{
  if (keys.empty())
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  const MapConst &mc = m->mc;
  const size_t kvox = size_t(mc.kdim[0]) * size_t(mc.kdim[1]) * size_t(mc.kdim[2]);
  const size_t tile_bytes = sizeof(float) * size_t(mc.region_voxels);
  const uint32_t count = uint32_t(keys.size());
  // (staging of at most 256 MiB per pass)
  const uint32_t batch = uint32_t(std::max<size_t>(1, std::min<size_t>(count, (size_t(256) << 20) / (sizeof(float) * kvox))));
  OHMHIP_CHECK(m->query.clear_out.ensure(sizeof(float) * kvox * batch, false, s));
  const float *d_out = static_cast<const float *>(m->query.clear_out.ptr);
  std::vector<int16_t> keys_xyz(3 * size_t(count));
  for (uint32_t i = 0; i < count; ++i)
  {
    unpackRegionKey(keys[i], &keys_xyz[3 * size_t(i)]);
  }
  std::vector<TileRef> tiles;
  std::vector<CopyJob> jobs;
  std::vector<uint32_t> slots;
  for (uint32_t r0 = 0; r0 < count; r0 += batch)
  {
    const uint32_t nb = std::min(batch, count - r0);
    OHMHIP_CHECK(clearanceRegionsDevice(m, a, &keys_xyz[3 * size_t(r0)], nb, static_cast<float *>(m->query.clear_out.ptr)));
    jobs.clear();
    for (uint32_t i = 0; i < nb; ++i)
    {
      tilesOfRegion(mc, &keys_xyz[3 * size_t(r0 + i)], tiles);
      for (const TileRef &t : tiles)
      {
        const uint64_t tile_key = packRegionKey(t.key);
        const char *src = reinterpret_cast<const char *>(d_out + size_t(i) * kvox + t.voxel_offset);
        const TileHome home = tileHome(m, tile_key);
        char *dst = tileLayerBlock(m, home, OHMHIP_LID_CLEARANCE);
        if (!dst)
        {
          continue;
        }
        jobs.push_back(CopyJob{ src, dst, tile_bytes });
        if (home.stored)
        {
          home.stored->dirty |= kDirtySync;
          continue;
        }
        if (!m->precleaned.empty())
        {
          dropPrecleanedKey(m, tile_key);  // (the write-back's copy of the region is void)
        }
        slots.push_back(home.slot);
      }
    }
    OHMHIP_CHECK(launchCopyJobs(m, jobs, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));  // (the next pass reuses the staging)
  }
  if (!slots.empty())
  {
    const uint32_t *d_index = nullptr;
    OHMHIP_CHECK(uploadSlotIndex(m, slots.data(), slots.size(), s, false, d_index));
    orSlotBits(m, d_index, slots.size(), kDirtySync, s);
    OHMHIP_CHECK(hipGetLastError());
  }
  auto &cl = m->clearance_layer;
  for (uint64_t key : keys)
  {
    auto &st = cl.regions[key];
    st.written = cl.epoch;
    st.params = params;
  }
  return hipStreamSynchronize(s);
}

/// What the three entry points check before any device work, then the search parameters (clearanceSetup) and the
/// parameter set.
int clearanceUpdateSetup(ohmhip_map_t m, const ohmhip_clearance_params *p, size_t count, const void *keys,
                         ClearanceArgs &a)
{
  static const char kAny = 0;
  OHMHIP_CHECK(clearanceSetup(m, keys, count, p, &kAny, a));
  if (!m->pool.layers[OHMHIP_LID_CLEARANCE])
  {
    return OHMHIP_ERR_UNSUPPORTED;
  }
  return OHMHIP_OK;
}
}  // namespace

extern "C" {

int ohmhip_map_clearance_stale_regions(ohmhip_map_t m, const ohmhip_clearance_params *params, int16_t *keys_xyz,
                                       size_t capacity, size_t *count)
try
{
  if (!m || !count || (capacity && !keys_xyz))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  *count = 0;
  ClearanceArgs a;
  OHMHIP_CHECK(clearanceUpdateSetup(m, params, 0, nullptr, a));
  OHMHIP_SETTLE(m);
  std::vector<uint64_t> present;
  std::vector<uint8_t> stale;
  OHMHIP_CHECK(clearanceSelect(m, clearanceParamSet(m, *params), a.h, present, stale));
  size_t n = 0;
  for (size_t i = 0; i < present.size(); ++i)
  {
    if (stale[i])
    {
      if (n < capacity)
      {
        unpackRegionKey(present[i], keys_xyz + 3 * n);
      }
      ++n;
    }
  }
  *count = n;
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

int ohmhip_map_clearance_update(ohmhip_map_t m, const ohmhip_clearance_params *params, size_t max_regions,
                                size_t *processed, size_t *remaining)
try
{
  if (processed)
  {
    *processed = 0;
  }
  if (remaining)
  {
    *remaining = 0;
  }
  ClearanceArgs a;
  OHMHIP_CHECK(clearanceUpdateSetup(m, params, 0, nullptr, a));
  OHMHIP_SETTLE(m);
  const uint32_t set = clearanceParamSet(m, *params);
  std::vector<uint64_t> present;
  std::vector<uint8_t> stale;
  OHMHIP_CHECK(clearanceSelect(m, set, a.h, present, stale));
  std::vector<uint64_t> todo;
  size_t total = 0;
  for (size_t i = 0; i < present.size(); ++i)
  {
    if (stale[i])
    {
      if (max_regions == 0 || todo.size() < max_regions)
      {
        todo.push_back(present[i]);
      }
      ++total;
    }
  }
  OHMHIP_CHECK(clearanceProcess(m, a, todo, set));
  if (processed)
  {
    *processed = todo.size();
  }
  if (remaining)
  {
    *remaining = total - todo.size();
  }
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

int ohmhip_map_clearance_update_regions(ohmhip_map_t m, const int16_t *keys_xyz, size_t count,
                                        const ohmhip_clearance_params *params, int force, size_t *processed)
try
{
  if (processed)
  {
    *processed = 0;
  }
  ClearanceArgs a;
  OHMHIP_CHECK(clearanceUpdateSetup(m, params, count, keys_xyz, a));
  OHMHIP_SETTLE(m);
  const uint32_t set = clearanceParamSet(m, *params);
  std::vector<uint64_t> present;
  std::vector<uint8_t> stale;
  OHMHIP_CHECK(clearanceSelect(m, set, a.h, present, stale));
  std::unordered_map<uint64_t, char> listed;
  for (size_t i = 0; i < count; ++i)
  {
    listed.emplace(packRegionKey(keys_xyz + 3 * i), 1);
  }
  std::vector<uint64_t> todo;
  for (size_t i = 0; i < present.size(); ++i)
  {
    if ((force || stale[i]) && listed.count(present[i]))
    {
      todo.push_back(present[i]);
    }
  }
  OHMHIP_CHECK(clearanceProcess(m, a, todo, set));
  if (processed)
  {
    *processed = todo.size();
  }
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_CLEARANCE_UPDATE_H
