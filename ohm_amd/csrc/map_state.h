// map_state.h -- the resident map object of libohmhip.so: device buffers, the staging thread pool, `struct ohmhip_map_s`
// and the forward declarations the parts of the translation unit share.
//
// Part of ohmhip_map.hip's translation unit (included there, in order): not a stand-alone header.
#ifndef OHMHIP_MAP_STATE_H
#define OHMHIP_MAP_STATE_H

namespace
{
const size_t kLayerBytes[OHMHIP_LID_COUNT] = { 4, 8, 24, 4, 4, 4, 8, 8, 8, 4 };

/// The 32-bit word a cleared voxel of layer l holds (ohm/DefaultLayer.cpp: occupancy +inf, clearance -1.0f), or 0 when
/// the layer clears to zero bytes.
inline uint32_t layerClearWord(int l)
{
  return (l == OHMHIP_LID_OCCUPANCY) ? 0x7f800000u : (l == OHMHIP_LID_CLEARANCE) ? 0xbf800000u : 0u;
}

// Owning types: every device buffer, pinned block, stream and event of the map is a member of one of these, so that
// releasing it is a property of the member.  All are movable and not copyable.

/// A device buffer that grows on demand (per-batch scratch, query staging).
struct DevBuf
{
  void *ptr = nullptr;
  size_t bytes = 0;

  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr, o.bytes = 0; }
  DevBuf &operator=(DevBuf &&o) noexcept
  {
    if (this != &o)
    {
      release();
      ptr = o.ptr, bytes = o.bytes;
      o.ptr = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }

  int ensure(size_t want, bool zero, hipStream_t stream)
  {
    if (want <= bytes)
    {
      return OHMHIP_OK;
    }
    if (ptr)
    {
      OHMHIP_CHECK(hipStreamSynchronize(stream));
      OHMHIP_CHECK(hipFree(ptr));
      ptr = nullptr;
      bytes = 0;
    }
    // Grow geometrically so steady-state batches never reallocate.
    size_t alloc = std::max(want, size_t(1) << 16);
    alloc = (alloc + (alloc >> 2) + 255) & ~size_t(255);
    OHMHIP_CHECK(hipMalloc(&ptr, alloc));
    bytes = alloc;
    if (zero)
    {
      OHMHIP_CHECK(hipMemsetAsync(ptr, 0, alloc, stream));
    }
    return OHMHIP_OK;
  }

  void release()
  {
    if (ptr)
    {
      (void)hipFree(ptr);
    }
    ptr = nullptr;
    bytes = 0;
  }
};

/// One handle with one owner: `Free` releases it when the owner dies or is given another.
template <typename H, hipError_t (*Free)(H)>
struct Owned
{
  H handle = nullptr;

  Owned() = default;
  Owned(Owned &&o) noexcept : handle(o.handle) { o.handle = nullptr; }
  Owned &operator=(Owned &&o) noexcept
  {
    if (this != &o)
    {
      reset();
      handle = o.handle;
      o.handle = nullptr;
    }
    return *this;
  }
  ~Owned() { reset(); }

  void reset()
  {
    if (handle)
    {
      (void)Free(handle);
    }
    handle = nullptr;
  }
};

/// A device allocation of fixed size, read where a `T *` is expected.
template <typename T>
struct DevArray : Owned<void *, hipFree>
{
  hipError_t alloc(size_t bytes)
  {
    reset();
    return hipMalloc(&handle, bytes);
  }
  T *get() const { return static_cast<T *>(handle); }
  operator T *() const { return get(); }
};

/// A stream of the map's own.
struct Stream : Owned<hipStream_t, hipStreamDestroy>
{
  hipError_t create()
  {
    reset();
    return hipStreamCreateWithFlags(&handle, hipStreamNonBlocking);
  }
  operator hipStream_t() const { return handle; }
};

/// An event of the map's own.
struct Event : Owned<hipEvent_t, hipEventDestroy>
{
  hipError_t create(unsigned flags = hipEventDefault)
  {
    reset();
    return hipEventCreateWithFlags(&handle, flags);
  }
  operator hipEvent_t() const { return handle; }
};

/// A pinned host block, read where a `T *` is expected.  `dev` is the block's device address when it was allocated
/// hipHostMallocMapped: an alias of the same memory, not owned.
template <typename T>
struct PinnedBuf
{
  T *ptr = nullptr;
  T *dev = nullptr;

  PinnedBuf() = default;
  PinnedBuf(PinnedBuf &&o) noexcept : ptr(o.ptr), dev(o.dev) { o.ptr = o.dev = nullptr; }
  PinnedBuf &operator=(PinnedBuf &&o) noexcept
  {
    if (this != &o)
    {
      reset();
      ptr = o.ptr, dev = o.dev;
      o.ptr = o.dev = nullptr;
    }
    return *this;
  }
  ~PinnedBuf() { reset(); }

  hipError_t alloc(size_t bytes, unsigned flags)
  {
    reset();
    hipError_t err = hipHostMalloc(reinterpret_cast<void **>(&ptr), bytes, flags);
    if (err == hipSuccess && (flags & hipHostMallocMapped))
    {
      err = hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), ptr, 0);
    }
    return err;
  }
  void reset()
  {
    if (ptr)
    {
      (void)hipHostFree(ptr);
    }
    ptr = dev = nullptr;
  }
  T *get() const { return ptr; }
  operator T *() const { return ptr; }
};

template <typename T>
constexpr bool kMoveOnly = std::is_nothrow_move_constructible<T>::value && std::is_nothrow_move_assignable<T>::value &&
                           !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value;
/// The buffers of one count-and-scan (read_side.h: countAndScan): a count per part and a zero behind them, their
/// exclusive scan in 64 bit, rocPRIM's scratch.
struct ScanScratch
{
  DevBuf counts, offsets, temp;
};

static_assert(kMoveOnly<DevBuf> && kMoveOnly<DevArray<uint32_t>> && kMoveOnly<PinnedBuf<uint32_t>> && kMoveOnly<Stream> &&
                kMoveOnly<Event>,
              "the owning types move and do not copy");
}  // namespace

constexpr uint32_t kTimingRing = 32;
constexpr uint32_t kDirtySync = 1u;   ///< d_dirty bit: modified since the last syncVoxels() (ohmhip_map_clear_dirty)
constexpr uint32_t kDirtyMerge = 2u;  ///< d_dirty bit: modified since the last replica merge (merge_impl.h)
constexpr uint32_t kDirtyClearance = 4u;  ///< d_dirty bit: occupancy modified since the last clearance fold (clearance_update.h)

/// A few host threads that stay around for the life of a map: staging a large host ray block into pinned memory is a
/// memcpy one core cannot do at PCIe speed, and starting threads per call costs as much as the copy of a small batch.
class StagePool
{
public:
  explicit StagePool(unsigned n_threads)
  {
    for (unsigned i = 0; i < n_threads; ++i)
    {
      threads_.emplace_back([this, i] { loop(i); });
    }
  }
  ~StagePool()
  {
    {
      std::lock_guard<std::mutex> lock(mu_);
      stop_ = true;
    }
    cv_work_.notify_all();
    for (auto &t : threads_)
    {
      t.join();
    }
  }
  unsigned size() const { return unsigned(threads_.size()); }
  /// Start job(worker index) on the first `n_workers` threads; returns at once.
  void start(unsigned n_workers, std::function<void(unsigned)> job)
  {
    std::lock_guard<std::mutex> lock(mu_);
    job_ = std::move(job);
    active_ = std::min<unsigned>(n_workers, size());
    running_ = active_;
    ++generation_;
    cv_work_.notify_all();
  }
  /// Block until every worker of the last start() has returned.
  void wait()
  {
    std::unique_lock<std::mutex> lock(mu_);
    cv_done_.wait(lock, [this] { return running_ == 0; });
  }

private:
  void loop(unsigned index)
  {
    uint64_t seen = 0;
    for (;;)
    {
      std::function<void(unsigned)> job;
      {
        std::unique_lock<std::mutex> lock(mu_);
        cv_work_.wait(lock, [&] { return stop_ || generation_ != seen; });
        if (stop_)
        {
          return;
        }
        seen = generation_;
        if (index >= active_)
        {
          continue;
        }
        job = job_;
      }
      job(index);
      {
        std::lock_guard<std::mutex> lock(mu_);
        if (--running_ == 0)
        {
          cv_done_.notify_all();
        }
      }
    }
  }
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_done_;
  std::function<void(unsigned)> job_;
  uint64_t generation_ = 0;
  unsigned active_ = 0, running_ = 0;
  bool stop_ = false;
};

struct ohmhip_map_s
{
  /// Settles what is in flight (the launch thread, every stream), joins the map's threads; then the members release
  /// themselves in reverse order of declaration -- the streams, declared first, last.
  ~ohmhip_map_s();

  ohmhip_map_config config;
  MapConst mc;
  int device = 0;
  Stream stream;       ///< compute stream
  Stream copy_stream;  ///< side stream for region upload/download
  Stream wb_stream;    ///< background write-back of the spill path (created on first use): its device-to-host
                                      ///< copies must not delay the re-admissions queued on copy_stream
  /// Stream of a batch's set-up pass (k_ray_setup, k_plan).  It reads the rays and the region table only, and writes
  /// per-batch scratch that exists twice (see `parity`), so the set-up of batch N+1 runs beside the sample sort of batch
  /// N and in the CUs its walk kernel vacates.  Every call waits for its own plan summary, so between calls the stream
  /// holds at most the call's early binning pass (early_bin_event below), which the compute stream waits for: whatever
  /// is ordered behind the compute stream is ordered behind the front stream too.
  Stream front_stream;
  /// Cross-stream ordering uses the STOP EVENTS of the kernels themselves (hipExtLaunchKernelGGL binds an event to the
  /// kernel's own completion signal: free), never a hipEventRecord behind a kernel -- on gfx950 / ROCm 7.2 a record is a
  /// barrier packet that idles the queue for 3-7 us before the next kernel starts (scripts/probes/event_probe.hip,
  /// profiles/r05_event_probe.txt; round 4 paid eight of them per batch).  The events live in the timing ring below.
  /// (batch_done_event and bin_done_event name events of the timing ring `tev`: aliases, not owned)
  hipEvent_t batch_done_event[2] = { nullptr, nullptr };  ///< per parity: stop event of the last kernel of the batch that last used this scratch copy
  hipEvent_t bin_done_event = nullptr;  ///< stop event of the latest k_ray_bin (early route: of the marker behind it)
  /// What a batch's EARLY binning pass waits for on the front stream (BatchRun::frontHalf, where the hazards are listed):
  /// the previous batch's walk-phase end, tev[3], when that was a plain occupancy batch -- its apply kernels then run
  /// beside the pass --, else that batch's end, tev[4]; null before the first batch.  An alias like the two above.
  hipEvent_t early_bin_event = nullptr;
  /// OHMHIP_EARLY_BIN=1 (read at map creation): a speculatively launched k_ray_bin goes to the front stream, behind
  /// early_bin_event, and the compute stream waits for it ahead of the sample sort.  0, the default: it is launched on
  /// the compute stream, behind the previous batch's last kernel.  (Off by default: 11-16 us of 848 per C1 batch, every
  /// run below every run without it, but not three times the run-to-run spread in three jobs of four --
  /// profiles/r08_notes.md.)
  bool early_bin = false;
  uint64_t count_batches = 0, count_binned_early = 0;  ///< ohmhip_map_pipeline_counts
  uint32_t parity = 0;  ///< which copy of the doubled per-batch scratch (RayWalk array, per-hash / per-slot counters,
                        ///< chunk list, event counters) the current batch uses
  Event ev[8];
  /// Events of the last kTimingRing batches: [1] binned, [2] samples ordered (the kernel before the walk), [3] walked,
  /// [4] batch done, [5] plan done, [7] the marker behind an early binning pass (BatchRun::frontHalf) -- all stop events
  /// of kernels --, and with `phase_timing` [0] set-up pass starts, [6] binning starts (on the stream the pass runs on;
  /// records: they cost the batch a few microseconds each).  tev_mask: which of [0] .. [6] the batch recorded;
  /// tev_pre_walk: the event that marks the start of the batch's walk phase ([2], or [1] when nothing ran in between).
  Event tev[kTimingRing][8];
  uint8_t tev_mask[kTimingRing] = {};
  uint8_t tev_pre_walk[kTimingRing] = {};
  bool phase_timing = false;  ///< ohmhip_map_set_phase_timing / OHMHIP_PHASE_TIMING=1 / OHMHIP_DEBUG_FLAGS & 256
  uint64_t batch_seq = 0;

  uint32_t slots_committed = 0;  ///< slots in use after the last successful batch / upload

  /// The region pool: every array allocPool (pool_impl.h) sizes by the pool's capacity.  One value: a pool is built
  /// beside the one in use and takes its place whole, or is dropped whole.
  struct RegionPool
  {
    uint32_t slot_capacity = 0;
    uint32_t hash_capacity = 0;
    uint32_t chunk_capacity = 0;
    DevArray<void> layers[OHMHIP_LID_COUNT];
    DevArray<unsigned long long> d_keys;
    DevArray<uint32_t> d_vals;
    DevArray<uint64_t> d_slot_keys;
    // scratch
    DevArray<uint32_t> d_hit_count, d_sort_list;
    DevArray<uint32_t> d_seg_count, d_seg_cursor, d_seg_offset, d_touched_flag, d_touched;
    DevArray<uint32_t> d_voxel_first_hit, d_hit_begin, d_hit_end, d_dirty;
    /// [2 x slot_capacity] per slot: the stamp of the batch that used the region last, and the stamp of the last use
    /// before the current run of consecutive batches (0: none) -- what the spill policy predicts a region's next use
    /// from (touchRegionUse, evictColdRegions); moves with the slot
    DevArray<uint32_t> d_last_use;
    DevArray<uint32_t> d_miss_counts;
    DevArray<uint32_t> d_hit_mask;
    DevArray<Chunk> d_chunks;
    /// Replica merge (merge_impl.h): base copy of the occupancy layer (null until ohmhip_map_enable_merge).
    DevArray<float> d_merge_base;
    /// Traversal layer only: per-voxel fixed-point sum of a batch's ray lengths (zero between batches).
    DevArray<unsigned long long> d_traversal_acc;
  } pool;
  DevArray<uint32_t> d_n_slots;
  DevArray<BatchInfo> d_info;   ///< three summaries used in turn: k_plan of one batch zeroes the next batch's
  PinnedBuf<BatchInfo> h_info;  ///< device visible: [0] batch summary (written by k_plan), [1] event count
  uint32_t info_index = 0;
  bool info_clean = false;       ///< d_info[next index] was zeroed by the previous batch's k_plan

  DevBuf walks_buf[2], hit_keys_a, hit_keys_b, interval_counts, segments, sort_temp, events;
  DevBuf wg_regions[2], wg_region_count[2], group_heads;  // (workgroup region lists: per parity)
  int merge_mode = 0;  ///< OHMHIP_MERGE_SHARED_ONLY / OHMHIP_MERGE_FULL_UNION
  DevBuf merge_slots, merge_keys_dev, merge_delta, merge_observers;
  /// Regions cut into tiles (tiling_impl.h): > 0 while the translation layer calls back into the entry points with tile
  /// keys.
  int tile_passthrough = 0;
  /// Partitioned map (partition_impl.h): the owner table of ohmhip_map_set_region_partition (host copy for
  /// ohmhip_map_region_owners, device copy behind MapConst::owner_table) and the scratch of ohmhip_map_route_rays.
  struct PartitionState
  {
    Stream route_stream;  ///< routing runs beside the batches in flight: it reads no map state
    std::vector<unsigned char> table_host;
    DevBuf table_dev, masks, block_counts, totals;
    PinnedBuf<uint32_t> h_totals;  ///< device visible: rays per destination of the last routing
  } partition;
  DevBuf use_scratch;  ///< (slot, stamp) pairs of re-admitted regions (queueReadmission)
  /// After how many batches the regions re-admitted lately came back (ring of the last 256): their median stands in as
  /// the period of regions that have no history of their own yet (evictColdRegions).
  std::vector<uint32_t> readmit_periods;
  size_t readmit_period_at = 0;
  DevBuf copy_jobs;  ///< job list of k_copy_jobs (spill to host, compaction)
  DevBuf stop_a, stop_b;  ///< kRfStopOnFirstOccupied: per-ray stop positions (current / candidate)
  /// ohmhip_map_rays_query (query_kernels.h) and the clearance queries (clearance_kernels.h): buffers of their own, so a
  /// query never touches a batch's staging.
  struct QueryState
  {
    DevBuf rays, ranges, volumes, types, keys;   ///< host-pointer calls: device copies of the caller's arrays
    DevBuf walked, last_walked, scan_temp;
    DevBuf spill_keys, spill_blocks;             ///< table of the host store's regions (spill to host)
    DevBuf clear_regions, clear_keys, clear_out, clear_mask;  ///< clearance queries (clearance_kernels.h)
    /// heightmap (heightmap_kernels.h): per-cell winner, per-column records, counters; device copies of the host arrays
    DevBuf hm_winner, hm_rec_occ, hm_rec_vox, hm_rec_mean, hm_counts, hm_out_occ, hm_out_vox, hm_out_mean, hm_out_col;
    /// the generation walk of the fill and layered heightmaps (heightmap_walk_impl.h): the queue of every visit, per key
    /// of a generation its ground height and heightmap cell, the events unsorted / sorted, the accept flags and their
    /// scan, sort and scan scratch, the log's device copy; the pinned pair read back per generation: [0] the next
    /// generation's size, [1] the build's own
    struct HeightmapWalk
    {
      DevBuf queue, ground, rec_cell, keys_a, keys_b, accept, accept_at, temp, log;
      PinnedBuf<uint32_t> next;
    } hm_walk;
    DevBuf hmf_grid;  ///< flood-fill heightmap (heightmap_fill_kernels.h): the visit grid
    /// layered heightmaps (heightmap_layered_kernels.h): per key of a generation its flags and src_height; the touched
    /// lists' heads, nodes and the two device words; per heightmap cell the slot count, the applied stamp and the
    /// multi-layer note; the slot planes; the sorted ground keys; layer_count's device copy
    DevBuf hml_flags, hml_height, hml_head, hml_nodes, hml_words, hml_cell_state, hml_occ, hml_vox, hml_mean, hml_visit,
      hml_ground, hml_ground_sorted, hml_out_count;
    /// point clouds (cloud_kernels.h): the work list, per-wave counts and their scan; device copies of the host arrays
    DevBuf cloud_chunks, cloud_pos, cloud_keys, cloud_values;
    ScanScratch cloud_scan;
    /// NearestNeighbours (neighbours_kernels.h): the work list, the near points, per-wave counts / closest voxels and
    /// their scan, per-query counts / closest voxels and the scan of the queries that found one (both scans' results
    /// are read by the emit pass, so each has its buffers); device copies of the host arrays
    DevBuf nn_chunks, nn_chunk_begin, nn_near, nn_best, nn_query_counts, nn_query_best, nn_keys, nn_ranges;
    ScanScratch nn_scan, nn_query_scan;
    DevBuf rv_keys, rv_values, rv_present;  ///< voxels read by key: device copies of the host arrays
    /// covariance decomposition by key (covariance_kernels.h): the voxels read and their present flags; device copies
    /// of the host variant's result arrays
    DevBuf cov_voxels, cov_present, cov_values, cov_vectors, cov_status;
    /// point filter (point_filter_kernels.h): per-wave kept counts and their scan; one piece of the host variant's
    /// arrays on the device, and the pinned block its points are staged through (two pieces + the piece's kept count)
    DevBuf pf_points, pf_status, pf_values, pf_keys, pf_kept;
    ScanScratch pf_scan;
    PinnedBuf<char> pf_staging;
    /// map compare (compare_kernels.h), on the REFERENCE map: the work list, a record per chunk, per-wave failed
    /// counts and their scan; device copies of the host variant's lists and result
    DevBuf compare_chunks, compare_records, compare_keys, compare_missing, compare_result;
    ScanScratch compare_scan;
  } query;
  /// Voxel edits by key (voxel_edit_impl.h): device copies of the host forms' arrays; per element the tile key, then
  /// the sort pair, each before and after its sort; the distinct tiles; rocPRIM's scratch; the counters of the stats.
  struct EditState
  {
    DevBuf keys, points, ops, values;
    DevBuf keys_a, keys_b, vals_a, vals_b, tiles, temp, counters;
  } edit;
  /// The clearance layer's bookkeeping (clearance_update.h), by the caller's region key -- so it needs no care when a
  /// region changes slot, leaves the pool or comes back.  An update folds the kDirtyClearance bits into `changed` at a
  /// new epoch; a region is up to date for parameter set P when it was written with P (`params`, 1 + index into
  /// `param_sets`; 0: never, or its layer was written by the host) at an epoch no change in its neighbourhood exceeds.
  /// Changes the host makes between updates (uploads, removals) take the epoch of the next fold.
  struct ClearanceLayerState
  {
    struct Region
    {
      uint32_t changed = 0;  ///< epoch of the last occupancy change or removal
      uint32_t written = 0;  ///< epoch the layer was last computed at
      uint32_t params = 0;
    };
    std::unordered_map<uint64_t, Region> regions;
    uint32_t epoch = 0;
    std::vector<ohmhip_clearance_params> param_sets;
    DevBuf table_keys, table_changed, present, written, stale;
  } clearance_layer;
  DevArray<uint32_t> d_event_count;  ///< per parity: [0] deferred event count, [1] walk kernel chunk cursor, [2] replay group count, [3] stop iteration flag
  uint32_t walk_workgroups = 256;     ///< persistent walk workgroups: one per CU
  /// Regions / tiles of at most 4 096 voxels (16^3) are walked by the WalkHalf shape of k_region_walk: 512-thread workgroups with
  /// half of everything, two per CU (walk_kernel.h; OHMHIP_WALK_HALF=0 keeps the full shape for A/B runs).
  bool walk_half = false;
  uint32_t walkSlots() const { return walk_workgroups * (walk_half ? 2u : 1u); }  ///< persistent walk workgroups of a launch
  DevArray<unsigned long long> d_dbg;  ///< 8 debug counters (OHMHIP_DEBUG_FLAGS & 64)
  DevArray<unsigned long long> d_order_counts;  ///< regions k_sort_region_hits ordered by rank [0], by the network [1]
  uint32_t sort_workgroups = 0;  ///< OHMHIP_SORT_WORKGROUPS (tests): cap of the grids of k_sort_region_hits, 0 = none
  double first_ray_time = -1.0;  ///< OccupancyMap::firstRayTime() (ohm/OccupancyMap.cpp:343-347)
  uint32_t event_demand = 0;
  uint32_t event_limit = 0;  ///< OHMHIP_EVENT_LIMIT (tests): cap of the NDT / TSDF event list's first sizing
  bool spec_bucket_ok = false;  ///< the previous occupancy batch used the per-region sample sort: bin speculatively
  uint32_t spec_max_region_hits = 0;  ///< ... and its densest region held this many samples (which sort kernels to launch)
  double segments_per_ray = 10.0;            ///< running estimate (previous batch) used to size the next batch's chunks
  uint32_t bin_rays_per_block = kBinRaysPerBlock;  ///< tunable (OHMHIP_BIN_RAYS): rays per binning workgroup, large batches
  uint32_t min_chunk_segments = 2048;  ///< tunable (OHMHIP_MIN_CHUNK_SEGMENTS): floor of the small-batch chunk size (two rounds of the walk workgroup's 1024 lanes)
  uint32_t chunk_segments = kChunkSegments;  ///< tunable (OHMHIP_CHUNK_SEGMENTS), <= kMaxChunkSegments (15-bit LDS counters)
  /// OHMHIP_DEBUG_FLAGS (development only): 16 = walk kernel refills lanes but does not walk (timing experiments,
  /// breaks results); 64 = per-chunk timing trace of the walk kernel (OHMHIP_DEBUG_TRACE=<file>, scripts/
  /// analyse_trace.py); 128 = iteration / visit / refill counters (hot-address atomics: distorts timing); 256 = phase
  /// timeline of the last three batches printed by ohmhip_map_sync; 512 = spill path timers; 2048 = where a host batch's
  /// call spends its time; 4096 = one line per batch: segments, chunks, regions, densest region.
  unsigned debug_flags = 0;
  int refill_min_idle = kRefillMinIdle;      ///< tunable (OHMHIP_REFILL_MIN_IDLE)  ///< events the previous batch produced (sizes the next batch's list)
  PinnedBuf<void> h_stage;  ///< staging for region copies
  size_t h_stage_bytes = 0;

  /// Host-pointer ray batches go through one of two staging slots (pinned host block + device copies), so the host
  /// copy and the H2D transfer of batch N+1 overlap the device work of batch N.  With coalescing on, consecutive small
  /// batches with the same flags accumulate in the filling slot and run as one device batch.
  struct RaySlot
  {
    PinnedBuf<char> h;            ///< capacity x 48 B rays, x 8 B timestamps, x 4 B intensities, x 1 B filter flags
    size_t capacity = 0;          ///< rays
    DevBuf d_rays, d_times, d_intens, d_fflags;
    Event uploaded;  ///< H2D copies done (copy stream)
    Event done;      ///< the batch reading the device copies has finished (compute stream)
    bool in_flight = false;
    bool rays_uploaded = false;     ///< the rays' H2D copies were queued piece by piece while the block was staged
  } ray_slots[2];
  std::unique_ptr<StagePool> stage_pool;  ///< created by the first large host batch
  /// ohmhip_map_set_async_launch: a host batch's device launch sequence (with its host round trip for the plan) runs on
  /// this one thread while the caller returns and stages its next block.
  bool async_launch = false;
  std::unique_ptr<StagePool> launch_thread;
  bool launch_busy = false;
  int launch_result = OHMHIP_OK;
  int fill_slot = 0;
  size_t pending_rays = 0;
  size_t pending_calls = 0;
  unsigned pending_flags = 0;
  bool pending_intens = false, pending_times = false, pending_fflags = false;
  /// The pending rays were presented through the device-pointer entry point: they sit in the filling slot's DEVICE
  /// buffers already (copied there device to device), the pinned block is not used.
  bool pending_on_device = false;
  PinnedBuf<uint32_t> h_passed;  ///< device visible: per-call filter count of a deferred device-pointer batch
  Event ev_passed;
  /// Host-pointer batches smaller than this are collected and run as one device batch (0: every host batch is launched
  /// by the call that presents it).  On by default: the reference tools present 4096 rays per call.
  size_t coalesce_min_rays = size_t(1) << 16;
  /// The ray-filter chain (ohmhip_map_set_ray_filter_stages; ray_filter_chain.h, ray_filter_kernels.h): while count > 0 it
  /// stands in place of the built-in filter for every batch the caller has not filtered.  It does not ride in MapConst:
  /// k_ray_filter and k_count_passed get the device copy through arguments of their own.
  struct RayFilterChain
  {
    ohmhip_ray_filter_stage stages[OHMHIP_MAX_RAY_FILTER_STAGES] = {};  ///< host copy: the staging threads' count
    uint32_t count = 0;
    DevBuf d_stages;  ///< device copy, rewritten only with nothing pending or in flight on the front / copy streams
    /// Per batch parity: the rays as the chain leaves them and their flag bytes.  Readers are the batch's set-up pass and
    /// its apply / replay kernels (sample points), so a copy is free again when the batch after the next starts -- the
    /// rule of the other doubled per-batch scratch (BatchRun::frontHalf waits for batch_done_event[parity]).
    DevBuf rays[2], flags[2];
    DevBuf q_rays, q_out, q_flags, q_passed;  ///< ohmhip_map_apply_ray_filter: its own buffers, like the other queries
  } ray_chain;

  // host mirror of the region table
  std::unordered_map<uint64_t, uint32_t> region_slots;
  std::vector<uint64_t> slot_keys_host;

  ohmhip_batch_stats stats = {};
  bool stats_pending = false;
  uint64_t cache_hits = 0, cache_misses = 0, cache_full = 0;  ///< ohmhip_map_cache_stats
  uint64_t rays_beyond_tiles = 0;  ///< ohmhip_map_rays_beyond_tiles (tiled maps: rays cut for key-range reasons)
  uint64_t memory_limit = 0;                                   ///< ohmhip_map_set_memory_limit
  /// A layer change under a memory limit (layout_impl.h) keeps the pool's slots -- the layers that stay do not move --
  /// though the limit may be worth fewer regions of the new set than the pool has slots: the batches then use this many
  /// (0: all of them; the limit bounds the pool's growth only, as without a layer change).
  uint32_t resident_cap = 0;
  /// Spill to host (ohmhip_map_set_spill_to_host): regions evicted from the pool when the memory limit is reached, by
  /// packed key.  A spilled region is still part of the map: it is listed, read and synced from here, and moves back
  /// into the pool when a batch (or an upload) touches it.
  struct SpilledRegion
  {
    /// One record of the pinned host store: the region's block of every enabled layer, in layer-id order, followed by
    /// its row of the NDT / TSDF replay mask (layerOffset / maskOffset below).  Pinned, so evictions and re-admissions
    /// are single asynchronous copies straight between the pool and the record -- no staging pass on either side.
    char *record = nullptr;
    uint32_t dirty = 0;
    uint32_t last_use = 0;  ///< stamp of the last batch that used the region before it left the pool
  };
  /// Pinned host store: slabs of fixed-size records, handed out from a free list.
  struct HostStore
  {
    size_t record_bytes = 0;
    size_t layer_offset[OHMHIP_LID_COUNT] = {};
    size_t mask_offset = 0;
    size_t mask_bytes = 0;
    std::vector<PinnedBuf<void>> slabs;
    std::vector<char *> free_records;
    size_t records_total = 0;
  } store;
  std::unordered_map<uint64_t, SpilledRegion> spilled;
  /// Background write-back (writeback_impl.h): resident regions whose content already sits in a store record, valid
  /// while the region's use stamp is the one the copy was taken at.
  struct Precleaned
  {
    char *record = nullptr;
    uint32_t last_use = 0;
  };
  std::unordered_map<uint64_t, Precleaned> precleaned;
  std::vector<char *> stale_records;  ///< records of discarded copies, recycled once the copy stream has passed them
  static constexpr uint32_t kWritebackRing = 4;
  struct WritebackRing
  {
    PinnedBuf<void> jobs;  ///< device visible: the kernel reads its job list straight from here (no copy call: a
                           ///< blocking hipMemcpy from pageable memory would stall the batch pipeline)
    size_t capacity = 0;   ///< bytes
    Event done;
    bool used = false;
  } wb_ring[kWritebackRing];
  uint32_t wb_next = 0;
  PinnedBuf<uint32_t> h_use;     ///< the resident regions' use stamps as of the latest plan (queueUseStamps)
  size_t h_use_capacity = 0;
  uint32_t h_use_slots = 0;      ///< slots the copy covers
  uint32_t evicted_per_call = 0; ///< regions the latest eviction moved out (sizes the write-back's lead)
  bool writeback_off = true;     ///< ohmhip_map_set_spill_writeback (off by default; OHMHIP_WRITEBACK=0 / 1 overrides)
  uint64_t writebacks = 0, writeback_hits = 0, writeback_stale = 0;
  uint32_t writeback_workgroups = 32;  ///< grid of the background copy kernel (OHMHIP_WRITEBACK_WGS): the CUs it may hold
  bool spill_enabled = false;
  /// The last batch failed with OHMHIP_ERR_CAPACITY because it alone touches more regions than the residency limit
  /// holds (not: hash full, device memory, slot field) -- the cause integrateRaysDevice answers by splitting the batch.
  bool batch_exceeds_limit = false;
  uint64_t evictions = 0, readmissions = 0;
  double wb_host_ms = 0;  ///< OHMHIP_DEBUG_FLAGS & 512: host time spent scheduling write-backs
  double spill_ms[6] = { 0, 0, 0, 0, 0, 0 };  ///< OHMHIP_DEBUG_FLAGS & 512: evict select / copy / compact, readmit copy, failed attempts, store growth
};

/// The caller's region key of a pool key (a tile key of a tiled map: tiling_impl.h).
inline uint64_t callerRegionKey(const ohmhip_map_s *m, uint64_t key)
{
  if (m->mc.tile_split[1] <= 1 && m->mc.tile_split[2] <= 1)
  {
    return key;
  }
  int16_t k[3];
  unpackRegionKey(key, k);
  return packRegionKey(k[0], floorDiv(k[1], m->mc.tile_split[1]), floorDiv(k[2], m->mc.tile_split[2]));
}

/// The host changed the occupancy of (or removed) the region of pool key `key`: its neighbourhood's clearance is stale.
inline void clearanceMarkChanged(ohmhip_map_s *m, uint64_t key)
{
  if (m->pool.layers[OHMHIP_LID_CLEARANCE])
  {
    m->clearance_layer.regions[callerRegionKey(m, key)].changed = m->clearance_layer.epoch + 1u;
  }
}

/// The host wrote the clearance layer of (or removed) the region of pool key `key`: it is no longer a computed result.
inline void clearanceMarkUnwritten(ohmhip_map_s *m, uint64_t key)
{
  if (m->pool.layers[OHMHIP_LID_CLEARANCE])
  {
    const auto it = m->clearance_layer.regions.find(callerRegionKey(m, key));
    if (it != m->clearance_layer.regions.end())
    {
      it->second.params = 0;
    }
  }
}

// Background write-back of the spill path (writeback_impl.h).
namespace
{
int queueUseStamps(ohmhip_map_t m, hipStream_t stream);
void scheduleWriteBack(ohmhip_map_t m, uint32_t now);
void dropPrecleaned(ohmhip_map_t m);
int drainWriteBack(ohmhip_map_t m);
void dropPrecleanedKey(ohmhip_map_t m, uint64_t key);
}  // namespace

// Regions larger than one tile (tiling_impl.h): the entry points that name or list regions translate.
inline bool tiledBoundary(ohmhip_map_t m)
{
  return m && (m->mc.tile_split[1] > 1 || m->mc.tile_split[2] > 1) && m->tile_passthrough == 0;
}
namespace
{
void chooseTileDims(const int dims[3], int limit, int tile[3]);
int tiledListRegions(ohmhip_map_t m, bool dirty_only, int16_t *keys_xyz, size_t capacity, size_t *count);
int tiledReadRegions(ohmhip_map_t m, int layer_id, const int16_t *keys_xyz, size_t count, void *const *dsts);
int tiledWriteRegions(ohmhip_map_t m, int layer_id, const int16_t *keys_xyz, size_t count, const void *const *srcs);
int tiledRemoveRegions(ohmhip_map_t m, const int16_t *keys_xyz, size_t count, size_t *removed);
}  // namespace

// Defined further down (they use the region read / remove machinery of the C ABI section).  Internal linkage: the
// shared library exports the C ABI of include/ohmhip.h and nothing else (tests/test_cabi.py).
static int removeResidentRegions(ohmhip_map_t m, const int16_t *keys_xyz, size_t count, size_t *removed);
static int evictColdRegions(ohmhip_map_t m, uint32_t want_free, uint32_t max_evict = 0xffffffffu);
static int makeRoomForNamedRegions(ohmhip_map_t m, const int16_t *keys_xyz, size_t count);
static int appendNamedRegions(ohmhip_map_t m, const int16_t *keys_xyz, size_t count, uint32_t *slots);
static int readmitSpilledSlots(ohmhip_map_t m, uint32_t first_slot, uint32_t end_slot);
static int readmitSpilledKeys(ohmhip_map_t m, const int16_t *keys_xyz, size_t count);


#endif  // OHMHIP_MAP_STATE_H
