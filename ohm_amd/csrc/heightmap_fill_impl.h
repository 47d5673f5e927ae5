// heightmap_fill_impl.h -- host side of the flood-fill heightmap (heightmap_fill_kernels.h): the planar call's
// prologue, source view and staged outputs (heightmap_impl.h), then one round of kernels per generation of the
// reference's queue with the next generation's size read back through a pinned word (its scan is 32 bit: not
// read_side.h's countAndScan).
// Included after heightmap_impl.h in ohmhip_map.hip's translation unit.
#ifndef OHMHIP_HEIGHTMAP_FILL_IMPL_H
#define OHMHIP_HEIGHTMAP_FILL_IMPL_H

namespace
{
static_assert(sizeof(HeightmapFillArgs) <= 4096, "kernel arguments are passed by value");

unsigned bitsFor(unsigned long long count)  ///< bits that hold 0 .. count - 1
{
  unsigned bits = 0;
  while (bits < 64u && (1ull << bits) < count)
  {
    ++bits;
  }
  return bits;
}

/// The queue holds every visit so far and must survive growing: a new block of at least twice the size, the old
/// entries copied.
int fillQueueReserve(DevBuf &queue, size_t entries, size_t used, hipStream_t s)
{
  const size_t want = sizeof(uint2) * entries;
  if (want <= queue.bytes)
  {
    return OHMHIP_OK;
  }
  DevBuf grown;
  OHMHIP_CHECK(grown.ensure(std::max(want, 2 * queue.bytes), false, s));
  if (used)
  {
    OHMHIP_CHECK(hipMemcpyAsync(grown.ptr, queue.ptr, sizeof(uint2) * used, hipMemcpyDeviceToDevice, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));
  }
  queue = std::move(grown);
  return OHMHIP_OK;
}

/// The walk, results into device arrays; returns with the stream idle.  The log, 3 uint32 per visit for the first
/// log_capacity visits, goes to d_log, or to log_staging grown to what the walk produced (the host-array call, whose
/// capacity may be "everything").
int heightmapFillDevice(ohmhip_map_t m, const HeightmapArgs &geometry, const int seed[3], float *d_occ, void *d_vox,
                        void *d_mean, uint32_t *d_visit, uint32_t *d_log, DevBuf *log_staging, uint64_t log_capacity,
                        ohmhip_heightmap_fill_stats &stats)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  HeightmapFillArgs f{};
  static_cast<HeightmapArgs &>(f) = geometry;
  OHMHIP_CHECK(heightmapSourceView(m, f));
  const size_t cells = size_t(f.ma) * size_t(f.mb);
  const size_t grid_cells = size_t(f.na) * size_t(f.nb);
  f.grid_cells = uint32_t(grid_cells);
  OHMHIP_CHECK(qs.hm_winner.ensure(sizeof(uint32_t) * cells, false, s));
  OHMHIP_CHECK(qs.hm_counts.ensure(sizeof(unsigned long long) * 8, false, s));
  OHMHIP_CHECK(qs.hmf_grid.ensure(sizeof(int) * grid_cells, false, s));
  if (!qs.hmf_next.ptr)
  {
    OHMHIP_CHECK(qs.hmf_next.alloc(sizeof(uint32_t), hipHostMallocDefault));
  }
  f.cell_visit = static_cast<uint32_t *>(qs.hm_winner.ptr);
  f.counts = static_cast<unsigned long long *>(qs.hm_counts.ptr);
  f.grid = static_cast<int *>(qs.hmf_grid.ptr);
  f.out_occ = d_occ;
  f.out_vox = static_cast<uint32_t *>(d_vox);
  f.out_mean = static_cast<uint2 *>(d_mean);
  f.out_visit = d_visit;
  f.out_log = d_log;
  OHMHIP_CHECK(hipMemsetAsync(f.grid, 0xff, sizeof(int) * grid_cells, s));
  OHMHIP_CHECK(hipMemsetAsync(f.counts, 0, sizeof(unsigned long long) * 8, s));
  hipLaunchKernelGGL(k_hmfill_clear, dim3(uint32_t((cells + 255) / 256)), dim3(256), 0, s, f);
  OHMHIP_CHECK(hipGetLastError());

  OHMHIP_CHECK(fillQueueReserve(qs.hmf_queue, 1 << 14, 0, s));
  // F2: the seed is heightmapGeometry's clamped key of reference_pos
  const uint2 first = make_uint2(uint32_t(seed[f.b] - f.min_g[f.b]) * uint32_t(f.na) + uint32_t(seed[f.a] - f.min_g[f.a]),
                                 uint32_t(seed[f.up] - f.min_g[f.up]));
  OHMHIP_CHECK(hipMemcpyAsync(qs.hmf_queue.ptr, &first, sizeof(first), hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));  // `first` is pageable

  const unsigned cell_bits = bitsFor((unsigned long long)grid_cells + 1ull);
  size_t begin = 0, count = 1;
  stats = ohmhip_heightmap_fill_stats{};
  while (count)
  {
    if (begin + count > 0xffffffffull || 9 * count >= (1ull << 31))
    {
      return OHMHIP_ERR_CAPACITY;
    }
    ++stats.generations;
    stats.largest_generation = std::max(stats.largest_generation, uint32_t(count));
    // every key may be accepted by all 8 neighbours
    OHMHIP_CHECK(fillQueueReserve(qs.hmf_queue, begin + 9 * count, begin + count, s));
    OHMHIP_CHECK(qs.hm_rec_occ.ensure(sizeof(float) * count, false, s));
    OHMHIP_CHECK(qs.hm_rec_vox.ensure(sizeof(uint32_t) * kHmVoxelWords * count, false, s));
    OHMHIP_CHECK(qs.hm_rec_mean.ensure(sizeof(uint2) * count, false, s));
    OHMHIP_CHECK(qs.hmf_ground.ensure(sizeof(uint32_t) * count, false, s));
    OHMHIP_CHECK(qs.hmf_rec_cell.ensure(sizeof(uint32_t) * count, false, s));
    OHMHIP_CHECK(qs.hmf_keys_a.ensure(sizeof(unsigned long long) * 9 * count, false, s));
    OHMHIP_CHECK(qs.hmf_keys_b.ensure(sizeof(unsigned long long) * 9 * count, false, s));
    OHMHIP_CHECK(qs.hmf_accept.ensure(sizeof(uint32_t) * (8 * count + 1), false, s));
    OHMHIP_CHECK(qs.hmf_accept_at.ensure(sizeof(uint32_t) * (8 * count + 1), false, s));
    f.queue = static_cast<uint2 *>(qs.hmf_queue.ptr);
    f.gen_begin = uint32_t(begin);
    f.gen_count = uint32_t(count);
    f.seed_generation = (begin == 0) ? 1 : 0;
    f.index_bits = bitsFor(count);
    f.rec_occ = static_cast<float *>(qs.hm_rec_occ.ptr);
    f.rec_vox = static_cast<uint32_t *>(qs.hm_rec_vox.ptr);
    f.rec_mean = static_cast<uint2 *>(qs.hm_rec_mean.ptr);
    f.ground_h = static_cast<uint32_t *>(qs.hmf_ground.ptr);
    f.rec_cell = static_cast<uint32_t *>(qs.hmf_rec_cell.ptr);
    f.keys = static_cast<unsigned long long *>(qs.hmf_keys_a.ptr);
    f.sorted = static_cast<const unsigned long long *>(qs.hmf_keys_b.ptr);
    f.accept = static_cast<uint32_t *>(qs.hmf_accept.ptr);
    f.accept_at = static_cast<const uint32_t *>(qs.hmf_accept_at.ptr);
    uint32_t *accept_at = static_cast<uint32_t *>(qs.hmf_accept_at.ptr);

    hipLaunchKernelGGL(k_hmfill_columns, dim3(uint32_t((count + 63) / 64)), dim3(64), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    size_t sort_bytes = 0;
    const unsigned end_bit = f.index_bits + cell_bits;
    OHMHIP_CHECK(rocprim::radix_sort_keys<SortConfig>(nullptr, sort_bytes, f.keys,
                                                      static_cast<unsigned long long *>(qs.hmf_keys_b.ptr), 9 * count, 0,
                                                      end_bit, s));
    OHMHIP_CHECK(qs.hmf_temp.ensure(sort_bytes, false, s));
    size_t temp_bytes = qs.hmf_temp.bytes;
    OHMHIP_CHECK(rocprim::radix_sort_keys<SortConfig>(qs.hmf_temp.ptr, temp_bytes, f.keys,
                                                      static_cast<unsigned long long *>(qs.hmf_keys_b.ptr), 9 * count, 0,
                                                      end_bit, s));
    hipLaunchKernelGGL(k_hmfill_replay, dim3(uint32_t((9 * count + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    size_t scan_bytes = 0;
    OHMHIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, f.accept, accept_at, 0u, 8 * count + 1,
                                         rocprim::plus<uint32_t>(), s));
    OHMHIP_CHECK(qs.hmf_temp.ensure(scan_bytes, false, s));
    scan_bytes = qs.hmf_temp.bytes;
    OHMHIP_CHECK(rocprim::exclusive_scan(qs.hmf_temp.ptr, scan_bytes, f.accept, accept_at, 0u, 8 * count + 1,
                                         rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_hmfill_append, dim3(uint32_t((8 * count + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    OHMHIP_CHECK(hipMemcpyAsync(qs.hmf_next.ptr, accept_at + 8 * count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));
    begin += count;
    count = *qs.hmf_next.ptr;
  }
  const uint64_t logged = std::min<uint64_t>(log_capacity, begin);
  if (log_staging && logged)
  {
    OHMHIP_CHECK(log_staging->ensure(sizeof(uint32_t) * 3 * logged, false, s));
    f.out_log = static_cast<uint32_t *>(log_staging->ptr);
  }
  f.log_count = f.out_log ? uint32_t(logged) : 0u;
  const size_t finish = std::max(cells, size_t(f.log_count));
  hipLaunchKernelGGL(k_hmfill_finish, dim3(uint32_t((finish + 255) / 256)), dim3(256), 0, s, f);
  OHMHIP_CHECK(hipGetLastError());
  unsigned long long counts[8] = {};
  OHMHIP_CHECK(hipMemcpyAsync(counts, f.counts, sizeof(counts), hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  stats.visits = begin;
  stats.populated = counts[0];
  stats.cells = counts[1];
  stats.revisits = counts[4];
  if (f.count_inspected)
  {
    std::fprintf(stderr, "ohmhip heightmap fill: %llu voxels inspected, %zu visits, %u generations\n", counts[3], begin,
                 stats.generations);
  }
  return counts[2] ? OHMHIP_ERR_INTERNAL : OHMHIP_OK;  // (a visit's cell outside the grid: cannot happen)
}
}  // namespace

extern "C" {

int ohmhip_map_heightmap_fill_extents(ohmhip_map_t m, const ohmhip_heightmap_params *params,
                                      ohmhip_heightmap_extents *extents)
try
{
  if (!extents)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  return heightmapBegin(m, params, kHmBuildFill, a, *extents);
}
OHMHIP_ABI_CATCH

int ohmhip_map_heightmap_fill(ohmhip_map_t m, const ohmhip_heightmap_params *params, float *occupancy, void *voxels24,
                              void *mean8, uint32_t *source_visit, uint32_t *visit_log, uint64_t visit_log_capacity,
                              ohmhip_heightmap_fill_stats *stats)
try
{
  if (!occupancy || !voxels24 || !stats)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  ohmhip_heightmap_extents e;
  int seed[3];
  OHMHIP_CHECK(heightmapBegin(m, params, kHmBuildFill, a, e, seed));
  *stats = ohmhip_heightmap_fill_stats{};
  if (!e.populated)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  const size_t n = size_t(a.ma) * size_t(a.mb);
  if (!visit_log)
  {
    visit_log_capacity = 0;
  }
  HeightmapStaged d;
  OHMHIP_CHECK(d.stage(qs, occupancy, voxels24, mean8, source_visit, n, s));
  OHMHIP_CHECK(heightmapFillDevice(m, a, seed, d.occ, d.vox, d.mean, d.source, nullptr, &qs.hmf_log, visit_log_capacity,
                                   *stats));
  const uint64_t logged = std::min<uint64_t>(visit_log_capacity, stats->visits);
  if (logged)
  {
    OHMHIP_CHECK(hipMemcpyAsync(visit_log, qs.hmf_log.ptr, sizeof(uint32_t) * 3 * logged, hipMemcpyDeviceToHost, s));
  }
  OHMHIP_CHECK(d.copyBack(occupancy, voxels24, mean8, source_visit, n, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_heightmap_fill_device(ohmhip_map_t m, const ohmhip_heightmap_params *params, float *d_occupancy,
                                     void *d_voxels24, void *d_mean8, uint32_t *d_source_visit, uint32_t *d_visit_log,
                                     uint64_t visit_log_capacity, ohmhip_heightmap_fill_stats *stats)
try
{
  if (!d_occupancy || !d_voxels24 || !stats)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  ohmhip_heightmap_extents e;
  int seed[3];
  OHMHIP_CHECK(heightmapBegin(m, params, kHmBuildFill, a, e, seed));
  *stats = ohmhip_heightmap_fill_stats{};
  if (!e.populated)
  {
    return OHMHIP_OK;
  }
  return heightmapFillDevice(m, a, seed, d_occupancy, d_voxels24, d_mean8, d_source_visit, d_visit_log, nullptr,
                             d_visit_log ? visit_log_capacity : 0, *stats);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_HEIGHTMAP_FILL_IMPL_H
