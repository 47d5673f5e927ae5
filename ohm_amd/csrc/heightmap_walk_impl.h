// heightmap_walk_impl.h -- host side of the generation walk (heightmap_walk_kernels.h) that the flood-fill and the
// layered heightmaps share: the queue seeded and grown, one round of kernels per generation with the next
// generation's size read back through a pinned word (its scan is 32 bit: not read_side.h's countAndScan), then the
// finish kernel with the visit log, and the tail of a host-array entry point.
//
// A walking build supplies a struct with
//   f                                       its kernel arguments, derived from HeightmapWalkArgs
//   id_bits                                 bits of its largest event id: the sort's end bit above the key index
//   columns                                 its columns kernel
//   generation(qs, begin, count, number, s) its own reservations and bindings for one generation
//   events(count, s)                        its event kernels, on the sorted events
//   settle(qs, next, count, s)              after the read of the next size is queued: returns with the stream idle
// Included after heightmap_impl.h and before the builds in ohmhip_map.hip's translation unit.
#ifndef OHMHIP_HEIGHTMAP_WALK_IMPL_H
#define OHMHIP_HEIGHTMAP_WALK_IMPL_H

namespace
{
unsigned bitsFor(unsigned long long count)  ///< bits that hold 0 .. count - 1
{
  unsigned bits = 0;
  while (bits < 64u && (1ull << bits) < count)
  {
    ++bits;
  }
  return bits;
}

/// `count` entries of T in `buf`, grown when it holds fewer (the old contents are not kept), as `to`.
template <typename T>
int ensureAs(DevBuf &buf, size_t count, hipStream_t s, T *&to)
{
  OHMHIP_CHECK(buf.ensure(sizeof(T) * count, false, s));
  to = static_cast<T *>(buf.ptr);
  return OHMHIP_OK;
}

/// A buffer that must survive growing: a new block of `want` bytes, or of `floor` when that is more, with the first
/// `used` bytes copied.
int growAndKeep(DevBuf &buf, size_t want, size_t used, size_t floor, hipStream_t s)
{
  if (want <= buf.bytes)
  {
    return OHMHIP_OK;
  }
  DevBuf grown;
  OHMHIP_CHECK(grown.ensure(std::max(want, floor), false, s));
  if (used)
  {
    OHMHIP_CHECK(hipMemcpyAsync(grown.ptr, buf.ptr, used, hipMemcpyDeviceToDevice, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));
  }
  buf = std::move(grown);
  return OHMHIP_OK;
}

/// The queue and what grows beside it, an entry per visit: to at least twice the size.
int walkQueueReserve(DevBuf &queue, size_t entries, size_t used, hipStream_t s)
{
  return growAndKeep(queue, sizeof(uint2) * entries, sizeof(uint2) * used, 2 * queue.bytes, s);
}

int heightmapSort(DevBuf &temp, unsigned long long *in, unsigned long long *out, size_t count, unsigned end_bit,
                  hipStream_t s)
{
  size_t sort_bytes = 0;
  OHMHIP_CHECK(rocprim::radix_sort_keys<SortConfig>(nullptr, sort_bytes, in, out, count, 0, end_bit, s));
  OHMHIP_CHECK(temp.ensure(sort_bytes, false, s));
  size_t temp_bytes = temp.bytes;
  return rocprim::radix_sort_keys<SortConfig>(temp.ptr, temp_bytes, in, out, count, 0, end_bit, s);
}

/// The generations, from the seed -- heightmapGeometry's clamped key of reference_pos (F2, L1) -- until one accepts
/// nothing; returns with the stream idle and generations, largest_generation and visits in `stats`.
template <typename Build, typename Stats>
int heightmapWalk(ohmhip_map_t m, Build &build, const int seed[3], Stats &stats)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  ohmhip_map_s::QueryState::HeightmapWalk &w = qs.hm_walk;
  HeightmapWalkArgs &f = build.f;
  if (!w.next.ptr)
  {
    OHMHIP_CHECK(w.next.alloc(sizeof(uint32_t) * 2, hipHostMallocDefault));
  }
  OHMHIP_CHECK(walkQueueReserve(w.queue, 1 << 14, 0, s));
  const uint2 first = make_uint2(uint32_t(seed[f.b] - f.min_g[f.b]) * uint32_t(f.na) + uint32_t(seed[f.a] - f.min_g[f.a]),
                                 uint32_t(seed[f.up] - f.min_g[f.up]));
  OHMHIP_CHECK(hipMemcpyAsync(w.queue.ptr, &first, sizeof(first), hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));  // `first` is pageable

  size_t begin = 0, count = 1;
  stats = Stats{};
  while (count)
  {
    if (begin + count > 0xffffffffull || 9 * count >= (1ull << 31))
    {
      return OHMHIP_ERR_CAPACITY;
    }
    ++stats.generations;
    stats.largest_generation = std::max(stats.largest_generation, uint32_t(count));
    // every key may be accepted by all 8 neighbours
    OHMHIP_CHECK(walkQueueReserve(w.queue, begin + 9 * count, begin + count, s));
    OHMHIP_CHECK(build.generation(qs, begin, count, stats.generations, s));
    unsigned long long *sorted = nullptr;
    uint32_t *accept_at = nullptr;
    OHMHIP_CHECK(ensureAs(qs.hm_rec_occ, count, s, f.rec_occ));
    OHMHIP_CHECK(ensureAs(qs.hm_rec_vox, kHmVoxelWords * count, s, f.rec_vox));
    OHMHIP_CHECK(ensureAs(qs.hm_rec_mean, count, s, f.rec_mean));
    OHMHIP_CHECK(ensureAs(w.ground, count, s, f.ground_h));
    OHMHIP_CHECK(ensureAs(w.rec_cell, count, s, f.rec_cell));
    OHMHIP_CHECK(ensureAs(w.keys_a, 9 * count, s, f.keys));
    OHMHIP_CHECK(ensureAs(w.keys_b, 9 * count, s, sorted));
    OHMHIP_CHECK(ensureAs(w.accept, 8 * count + 1, s, f.accept));
    OHMHIP_CHECK(ensureAs(w.accept_at, 8 * count + 1, s, accept_at));
    f.queue = static_cast<uint2 *>(w.queue.ptr);
    f.gen_begin = uint32_t(begin);
    f.gen_count = uint32_t(count);
    f.seed_generation = (begin == 0) ? 1 : 0;
    f.index_bits = bitsFor(count);
    f.sorted = sorted;
    f.accept_at = accept_at;

    hipLaunchKernelGGL(Build::columns, dim3(uint32_t((count + 63) / 64)), dim3(64), 0, s, build.f);
    OHMHIP_CHECK(hipGetLastError());
    OHMHIP_CHECK(heightmapSort(w.temp, f.keys, sorted, 9 * count, f.index_bits + build.id_bits, s));
    OHMHIP_CHECK(build.events(count, s));
    size_t scan_bytes = 0;
    OHMHIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, f.accept, accept_at, 0u, 8 * count + 1,
                                         rocprim::plus<uint32_t>(), s));
    OHMHIP_CHECK(w.temp.ensure(scan_bytes, false, s));
    scan_bytes = w.temp.bytes;
    OHMHIP_CHECK(rocprim::exclusive_scan(w.temp.ptr, scan_bytes, f.accept, accept_at, 0u, 8 * count + 1,
                                         rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_hmwalk_append, dim3(uint32_t((8 * count + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    OHMHIP_CHECK(hipMemcpyAsync(w.next.ptr, accept_at + 8 * count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OHMHIP_CHECK(build.settle(qs, w.next.ptr, count, s));
    begin += count;
    count = w.next.ptr[0];
  }
  stats.visits = begin;
  return OHMHIP_OK;
}

/// After the walk: the build's finish kernel, 1 lane / heightmap cell and / logged visit, and the device counts read
/// back; returns with the stream idle.  The log, 3 uint32 per visit for the first log_capacity visits, goes to
/// f.out_log, or to log_staging grown to what the walk produced (the host-array call, whose capacity may be
/// "everything").
template <typename Args, typename Stats, size_t N>
int heightmapWalkFinish(ohmhip_map_t m, Args &f, void (*finish)(Args), const char *name, DevBuf *log_staging,
                        uint64_t log_capacity, const Stats &stats, unsigned long long (&counts)[N])
{
  hipStream_t s = m->stream;
  const uint64_t logged = std::min<uint64_t>(log_capacity, stats.visits);
  if (log_staging && logged)
  {
    OHMHIP_CHECK(log_staging->ensure(sizeof(uint32_t) * 3 * logged, false, s));
    f.out_log = static_cast<uint32_t *>(log_staging->ptr);
  }
  f.log_count = f.out_log ? uint32_t(logged) : 0u;
  const size_t lanes = std::max(size_t(f.ma) * size_t(f.mb), size_t(f.log_count));
  hipLaunchKernelGGL(finish, dim3(uint32_t((lanes + 255) / 256)), dim3(256), 0, s, f);
  OHMHIP_CHECK(hipGetLastError());
  OHMHIP_CHECK(hipMemcpyAsync(counts, f.counts, sizeof(counts), hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  if (f.count_inspected)
  {
    std::fprintf(stderr, "ohmhip heightmap %s: %llu voxels inspected, %llu visits, %u generations\n", name, counts[3],
                 (unsigned long long)stats.visits, stats.generations);
  }
  return counts[2] ? OHMHIP_ERR_INTERNAL : OHMHIP_OK;  // (a visit's cell outside the grid: cannot happen)
}

/// The tail of a host-array entry point: the device copies of the result arrays of `n` entries, `device(staged, log,
/// log capacity)` -- the build's walk into them, which fills `stats` --, the log and the results copied back, the
/// stream idle.
template <typename Stats, typename Device>
int heightmapWalkToHost(ohmhip_map_t m, float *occupancy, void *voxels24, void *mean8, uint32_t *source_visit, size_t n,
                        uint32_t *visit_log, uint64_t visit_log_capacity, const Stats &stats, Device device)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  if (!visit_log)
  {
    visit_log_capacity = 0;
  }
  HeightmapStaged d;
  OHMHIP_CHECK(d.stage(qs, occupancy, voxels24, mean8, source_visit, n, s));
  OHMHIP_CHECK(device(d, &qs.hm_walk.log, visit_log_capacity));
  const uint64_t logged = std::min<uint64_t>(visit_log_capacity, stats.visits);
  if (logged)
  {
    OHMHIP_CHECK(hipMemcpyAsync(visit_log, qs.hm_walk.log.ptr, sizeof(uint32_t) * 3 * logged, hipMemcpyDeviceToHost, s));
  }
  OHMHIP_CHECK(d.copyBack(occupancy, voxels24, mean8, source_visit, n, s));
  return hipStreamSynchronize(s);
}
}  // namespace

#endif  // OHMHIP_HEIGHTMAP_WALK_IMPL_H
