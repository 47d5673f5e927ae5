// heightmap_layered_impl.h -- host side of the layered heightmaps (heightmap_layered_kernels.h): the fill call's
// prologue, source view, queue and generation loop (heightmap_fill_impl.h) with the touched lists' node pool growing
// beside the queue and the slot planes growing by doubling when a column asks for more; then L6, L7 and the results.
// Included after heightmap_fill_impl.h in ohmhip_map.hip's translation unit.
#ifndef OHMHIP_HEIGHTMAP_LAYERED_IMPL_H
#define OHMHIP_HEIGHTMAP_LAYERED_IMPL_H

namespace
{
static_assert(sizeof(HeightmapLayeredArgs) <= 4096, "kernel arguments are passed by value");

constexpr uint32_t kHmlInitialSlots = 2;
constexpr uint32_t kHmlMostSlots = 255;  ///< of one column: beyond it OHMHIP_ERR_CAPACITY

/// What the three layered entry points check before any device work, after their own pointers.
int heightmapLayeredRefusal(ohmhip_map_t m, const ohmhip_heightmap_layered_params *p)
{
  if (!p || p->reserved != 0)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return heightmapRefusal(m, &p->base, kHmBuildLayered);
}

int heightmapLayeredBegin(ohmhip_map_t m, const ohmhip_heightmap_layered_params *p, HeightmapArgs &a,
                          ohmhip_heightmap_extents &e, int *reference = nullptr)
{
  OHMHIP_CHECK(heightmapLayeredRefusal(m, p));
  OHMHIP_SETTLE(m);
  return heightmapGeometry(m, &p->base, a, e, reference);
}

/// The slot planes [slots][cells] of `bytes_per_cell` each: a new block for `slots`, the first `used` planes copied.
int layeredPlaneReserve(DevBuf &plane, size_t bytes_per_cell, size_t cells, uint32_t slots, uint32_t used, hipStream_t s)
{
  const size_t want = bytes_per_cell * cells * slots;
  if (want <= plane.bytes)
  {
    return OHMHIP_OK;
  }
  DevBuf grown;
  OHMHIP_CHECK(grown.ensure(want, false, s));
  if (used)
  {
    OHMHIP_CHECK(hipMemcpyAsync(grown.ptr, plane.ptr, bytes_per_cell * cells * used, hipMemcpyDeviceToDevice, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));
  }
  plane = std::move(grown);
  return OHMHIP_OK;
}

int layeredPlanes(ohmhip_map_s::QueryState &qs, HeightmapLayeredArgs &f, uint32_t slots, uint32_t used, hipStream_t s)
{
  const size_t cells = f.hm_cells;
  if (size_t(slots) * cells > (size_t(1) << 31))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  OHMHIP_CHECK(layeredPlaneReserve(qs.hml_occ, sizeof(float), cells, slots, used, s));
  OHMHIP_CHECK(layeredPlaneReserve(qs.hml_vox, sizeof(uint32_t) * kHmVoxelWords, cells, slots, used, s));
  OHMHIP_CHECK(layeredPlaneReserve(qs.hml_mean, sizeof(uint2), cells, slots, used, s));
  OHMHIP_CHECK(layeredPlaneReserve(qs.hml_visit, sizeof(uint32_t), cells, slots, used, s));
  OHMHIP_CHECK(layeredPlaneReserve(qs.hml_ground, sizeof(unsigned long long), cells, slots, used, s));
  f.slot_capacity = slots;
  f.sl_occ = static_cast<float *>(qs.hml_occ.ptr);
  f.sl_vox = static_cast<uint32_t *>(qs.hml_vox.ptr);
  f.sl_mean = static_cast<uint2 *>(qs.hml_mean.ptr);
  f.sl_visit = static_cast<uint32_t *>(qs.hml_visit.ptr);
  f.sl_ground = static_cast<unsigned long long *>(qs.hml_ground.ptr);
  return OHMHIP_OK;
}

int layeredSort(ohmhip_map_s::QueryState &qs, unsigned long long *in, unsigned long long *out, size_t count,
                unsigned end_bit, hipStream_t s)
{
  size_t sort_bytes = 0;
  OHMHIP_CHECK(rocprim::radix_sort_keys<SortConfig>(nullptr, sort_bytes, in, out, count, 0, end_bit, s));
  OHMHIP_CHECK(qs.hmf_temp.ensure(sort_bytes, false, s));
  size_t temp_bytes = qs.hmf_temp.bytes;
  return rocprim::radix_sort_keys<SortConfig>(qs.hmf_temp.ptr, temp_bytes, in, out, count, 0, end_bit, s);
}

/// The walk and what follows it, results into device arrays of layer_capacity planes; returns with the stream idle.
/// The log as in heightmapFillDevice.
int heightmapLayeredDevice(ohmhip_map_t m, const ohmhip_heightmap_layered_params &params, const HeightmapArgs &geometry,
                           const int seed[3], uint32_t layer_capacity, float *d_occ, void *d_vox, void *d_mean,
                           uint32_t *d_visit, uint8_t *d_count, uint32_t *d_log, DevBuf *log_staging,
                           uint64_t log_capacity, ohmhip_heightmap_layered_stats &stats)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  HeightmapLayeredArgs f{};
  static_cast<HeightmapArgs &>(f) = geometry;
  OHMHIP_CHECK(heightmapSourceView(m, f));
  const size_t cells = size_t(f.ma) * size_t(f.mb);
  const size_t grid_cells = size_t(f.na) * size_t(f.nb);
  if (cells + grid_cells + 1 > 0xffffffffull || size_t(layer_capacity) * cells > (size_t(1) << 31))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  f.grid_cells = uint32_t(grid_cells);
  f.hm_cells = uint32_t(cells);
  f.ordered = (params.base.mode == 3) ? 1 : 0;
  f.filter_threshold = f.ordered ? params.virtual_surface_filter_threshold : 0u;
  f.epsilon = 1e-3 * params.base.grid_resolution;
  {
    double up_vec[3] = { 0.0, 0.0, 0.0 };
    up_vec[f.up] = f.up_positive ? 1.0 : -1.0;
    const double *r = params.base.reference_pos;
    f.seed_height = (up_vec[0] * r[0] + up_vec[1] * r[1]) + up_vec[2] * r[2];  // glm::dot(up, reference_pos)
  }
  f.layer_capacity = layer_capacity;
  OHMHIP_CHECK(qs.hm_counts.ensure(sizeof(unsigned long long) * kHmlCountWords, false, s));
  OHMHIP_CHECK(qs.hml_head.ensure(sizeof(uint32_t) * grid_cells, false, s));
  OHMHIP_CHECK(qs.hml_cell_state.ensure(sizeof(uint32_t) * 3 * cells, false, s));
  OHMHIP_CHECK(qs.hml_words.ensure(sizeof(uint32_t) * 2, false, s));
  if (!qs.hml_next.ptr)
  {
    OHMHIP_CHECK(qs.hml_next.alloc(sizeof(uint32_t) * 2, hipHostMallocDefault));
  }
  f.counts = static_cast<unsigned long long *>(qs.hm_counts.ptr);
  f.touched_head = static_cast<uint32_t *>(qs.hml_head.ptr);
  f.slot_count = static_cast<uint32_t *>(qs.hml_cell_state.ptr);
  f.applied = f.slot_count + cells;
  f.multi = f.applied + cells;
  f.words = static_cast<uint32_t *>(qs.hml_words.ptr);
  f.out_occ = d_occ;
  f.out_vox = static_cast<uint32_t *>(d_vox);
  f.out_mean = static_cast<uint2 *>(d_mean);
  f.out_source = d_visit;
  f.out_count = d_count;
  f.out_log = d_log;
  OHMHIP_CHECK(layeredPlanes(qs, f, kHmlInitialSlots, 0, s));
  hipLaunchKernelGGL(k_hml_clear, dim3(uint32_t((std::max(std::max(cells, grid_cells), size_t(kHmlCountWords)) + 255) / 256)),
                     dim3(256), 0, s, f);
  OHMHIP_CHECK(hipGetLastError());

  OHMHIP_CHECK(fillQueueReserve(qs.hmf_queue, 1 << 14, 0, s));
  OHMHIP_CHECK(fillQueueReserve(qs.hml_nodes, 1 << 14, 0, s));
  // L1: the seed is heightmapGeometry's clamped key of reference_pos
  const uint2 first = make_uint2(uint32_t(seed[f.b] - f.min_g[f.b]) * uint32_t(f.na) + uint32_t(seed[f.a] - f.min_g[f.a]),
                                 uint32_t(seed[f.up] - f.min_g[f.up]));
  OHMHIP_CHECK(hipMemcpyAsync(qs.hmf_queue.ptr, &first, sizeof(first), hipMemcpyHostToDevice, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));  // `first` is pageable

  const unsigned id_bits = bitsFor((unsigned long long)grid_cells + cells + 1ull);
  size_t begin = 0, count = 1;
  stats = ohmhip_heightmap_layered_stats{};
  while (count)
  {
    if (begin + count > 0xffffffffull || 9 * count >= (1ull << 31))
    {
      return OHMHIP_ERR_CAPACITY;
    }
    ++stats.generations;
    stats.largest_generation = std::max(stats.largest_generation, uint32_t(count));
    // every key may be accepted by all 8 neighbours; an accepted offer takes one node
    OHMHIP_CHECK(fillQueueReserve(qs.hmf_queue, begin + 9 * count, begin + count, s));
    OHMHIP_CHECK(fillQueueReserve(qs.hml_nodes, begin + 9 * count, begin + count, s));
    OHMHIP_CHECK(qs.hm_rec_occ.ensure(sizeof(float) * count, false, s));
    OHMHIP_CHECK(qs.hm_rec_vox.ensure(sizeof(uint32_t) * kHmVoxelWords * count, false, s));
    OHMHIP_CHECK(qs.hm_rec_mean.ensure(sizeof(uint2) * count, false, s));
    OHMHIP_CHECK(qs.hmf_ground.ensure(sizeof(uint32_t) * count, false, s));
    OHMHIP_CHECK(qs.hmf_rec_cell.ensure(sizeof(uint32_t) * count, false, s));
    OHMHIP_CHECK(qs.hml_flags.ensure(sizeof(uint32_t) * count, false, s));
    OHMHIP_CHECK(qs.hml_height.ensure(sizeof(double) * count, false, s));
    OHMHIP_CHECK(qs.hmf_keys_a.ensure(sizeof(unsigned long long) * 9 * count, false, s));
    OHMHIP_CHECK(qs.hmf_keys_b.ensure(sizeof(unsigned long long) * 9 * count, false, s));
    OHMHIP_CHECK(qs.hmf_accept.ensure(sizeof(uint32_t) * (8 * count + 1), false, s));
    OHMHIP_CHECK(qs.hmf_accept_at.ensure(sizeof(uint32_t) * (8 * count + 1), false, s));
    f.queue = static_cast<uint2 *>(qs.hmf_queue.ptr);
    f.nodes = static_cast<uint2 *>(qs.hml_nodes.ptr);
    f.node_capacity = uint32_t(std::min<size_t>(qs.hml_nodes.bytes / sizeof(uint2), 0xffffffffu));
    f.gen_begin = uint32_t(begin);
    f.gen_count = uint32_t(count);
    f.seed_generation = (begin == 0) ? 1 : 0;
    f.stamp = stats.generations;
    f.index_bits = bitsFor(count);
    f.rec_occ = static_cast<float *>(qs.hm_rec_occ.ptr);
    f.rec_vox = static_cast<uint32_t *>(qs.hm_rec_vox.ptr);
    f.rec_mean = static_cast<uint2 *>(qs.hm_rec_mean.ptr);
    f.ground_h = static_cast<uint32_t *>(qs.hmf_ground.ptr);
    f.rec_cell = static_cast<uint32_t *>(qs.hmf_rec_cell.ptr);
    f.key_flags = static_cast<uint32_t *>(qs.hml_flags.ptr);
    f.src_height = static_cast<double *>(qs.hml_height.ptr);
    f.keys = static_cast<unsigned long long *>(qs.hmf_keys_a.ptr);
    f.sorted = static_cast<const unsigned long long *>(qs.hmf_keys_b.ptr);
    f.accept = static_cast<uint32_t *>(qs.hmf_accept.ptr);
    f.accept_at = static_cast<const uint32_t *>(qs.hmf_accept_at.ptr);
    uint32_t *accept_at = static_cast<uint32_t *>(qs.hmf_accept_at.ptr);

    hipLaunchKernelGGL(k_hml_columns, dim3(uint32_t((count + 63) / 64)), dim3(64), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    OHMHIP_CHECK(layeredSort(qs, f.keys, static_cast<unsigned long long *>(qs.hmf_keys_b.ptr), 9 * count,
                             f.index_bits + id_bits, s));
    const dim3 event_blocks(uint32_t((9 * count + 255) / 256));
    hipLaunchKernelGGL(k_hml_offers, event_blocks, dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_hml_adds, event_blocks, dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    size_t scan_bytes = 0;
    OHMHIP_CHECK(rocprim::exclusive_scan(nullptr, scan_bytes, f.accept, accept_at, 0u, 8 * count + 1,
                                         rocprim::plus<uint32_t>(), s));
    OHMHIP_CHECK(qs.hmf_temp.ensure(scan_bytes, false, s));
    scan_bytes = qs.hmf_temp.bytes;
    OHMHIP_CHECK(rocprim::exclusive_scan(qs.hmf_temp.ptr, scan_bytes, f.accept, accept_at, 0u, 8 * count + 1,
                                         rocprim::plus<uint32_t>(), s));
    hipLaunchKernelGGL(k_hmfill_append, dim3(uint32_t((8 * count + 255) / 256)), dim3(256), 0, s,
                       static_cast<const HeightmapFillArgs &>(f));
    OHMHIP_CHECK(hipGetLastError());
    OHMHIP_CHECK(hipMemcpyAsync(qs.hml_next.ptr, accept_at + 8 * count, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OHMHIP_CHECK(hipMemcpyAsync(qs.hml_next.ptr + 1, f.words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));
    while (qs.hml_next.ptr[1] > f.slot_capacity)
    {
      // a column asked for more slots: its adds are not applied yet, every other cell's are
      const uint32_t asked = qs.hml_next.ptr[1];
      OHMHIP_CHECK(layeredPlanes(qs, f, std::max(asked, 2 * f.slot_capacity), f.slot_capacity, s));
      OHMHIP_CHECK(hipMemsetAsync(f.words + 1, 0, sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_hml_adds, event_blocks, dim3(256), 0, s, f);
      OHMHIP_CHECK(hipGetLastError());
      OHMHIP_CHECK(hipMemcpyAsync(qs.hml_next.ptr + 1, f.words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      OHMHIP_CHECK(hipStreamSynchronize(s));
    }
    begin += count;
    count = qs.hml_next.ptr[0];
  }
  if (f.filter_threshold)
  {
    // L6
    const size_t slots = size_t(f.slot_capacity) * cells;
    OHMHIP_CHECK(qs.hmf_keys_a.ensure(sizeof(unsigned long long) * slots, false, s));
    OHMHIP_CHECK(qs.hml_ground_sorted.ensure(sizeof(unsigned long long) * slots, false, s));
    f.keys = static_cast<unsigned long long *>(qs.hmf_keys_a.ptr);
    f.ground_sorted = static_cast<const unsigned long long *>(qs.hml_ground_sorted.ptr);
    hipLaunchKernelGGL(k_hml_keys, dim3(uint32_t((slots + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    OHMHIP_CHECK(layeredSort(qs, f.keys, static_cast<unsigned long long *>(qs.hml_ground_sorted.ptr), slots, 64, s));
    hipLaunchKernelGGL(k_hml_filter, dim3(uint32_t((slots + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
  }
  const uint64_t logged = std::min<uint64_t>(log_capacity, begin);
  if (log_staging && logged)
  {
    OHMHIP_CHECK(log_staging->ensure(sizeof(uint32_t) * 3 * logged, false, s));
    f.out_log = static_cast<uint32_t *>(log_staging->ptr);
  }
  f.log_count = f.out_log ? uint32_t(logged) : 0u;
  const size_t finish = std::max(cells, size_t(f.log_count));
  hipLaunchKernelGGL(k_hml_finish, dim3(uint32_t((finish + 255) / 256)), dim3(256), 0, s, f);
  OHMHIP_CHECK(hipGetLastError());
  unsigned long long counts[kHmlCountWords] = {};
  OHMHIP_CHECK(hipMemcpyAsync(counts, f.counts, sizeof(counts), hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  stats.visits = begin;
  stats.populated = counts[0];
  stats.cells = counts[kHmlCells];
  stats.voxels = counts[kHmlVoxels];
  stats.repeats = counts[kHmlRepeats];
  stats.too_close = counts[kHmlTooClose];
  stats.filtered = counts[kHmlFiltered];
  stats.multi_layer_columns = counts[kHmlMultiColumns];
  stats.layers = uint32_t(counts[kHmlLayers]);
  if (f.count_inspected)
  {
    std::fprintf(stderr, "ohmhip heightmap layered: %llu voxels inspected, %zu visits, %u generations\n", counts[3],
                 begin, stats.generations);
  }
  if (counts[2])
  {
    return OHMHIP_ERR_INTERNAL;  // (a visit's cell outside the grid, a node beyond the pool: cannot happen)
  }
  return (stats.layers > kHmlMostSlots) ? OHMHIP_ERR_CAPACITY : OHMHIP_OK;
}
}  // namespace

extern "C" {

int ohmhip_map_heightmap_layered_extents(ohmhip_map_t m, const ohmhip_heightmap_layered_params *params,
                                         ohmhip_heightmap_extents *extents)
try
{
  if (!extents)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  return heightmapLayeredBegin(m, params, a, *extents);
}
OHMHIP_ABI_CATCH

int ohmhip_map_heightmap_layered(ohmhip_map_t m, const ohmhip_heightmap_layered_params *params, uint32_t layer_capacity,
                                 float *occupancy, void *voxels24, void *mean8, uint32_t *source_visit,
                                 uint8_t *layer_count, uint32_t *visit_log, uint64_t visit_log_capacity,
                                 ohmhip_heightmap_layered_stats *stats)
try
{
  if (!occupancy || !voxels24 || !stats || layer_capacity == 0)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  ohmhip_heightmap_extents e;
  int seed[3];
  OHMHIP_CHECK(heightmapLayeredBegin(m, params, a, e, seed));
  *stats = ohmhip_heightmap_layered_stats{};
  if (!e.populated)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  const size_t cells = size_t(a.ma) * size_t(a.mb);
  if (size_t(layer_capacity) * cells > (size_t(1) << 31))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  const size_t n = size_t(layer_capacity) * cells;
  if (!visit_log)
  {
    visit_log_capacity = 0;
  }
  HeightmapStaged d;
  OHMHIP_CHECK(d.stage(qs, occupancy, voxels24, mean8, source_visit, n, s));
  uint8_t *d_count = nullptr;
  OHMHIP_CHECK(stageOut(qs.hml_out_count, layer_count, cells, s, d_count));
  OHMHIP_CHECK(heightmapLayeredDevice(m, *params, a, seed, layer_capacity, d.occ, d.vox, d.mean, d.source, d_count,
                                      nullptr, &qs.hmf_log, visit_log_capacity, *stats));
  const uint64_t logged = std::min<uint64_t>(visit_log_capacity, stats->visits);
  if (logged)
  {
    OHMHIP_CHECK(hipMemcpyAsync(visit_log, qs.hmf_log.ptr, sizeof(uint32_t) * 3 * logged, hipMemcpyDeviceToHost, s));
  }
  OHMHIP_CHECK(d.copyBack(occupancy, voxels24, mean8, source_visit, n, s));
  OHMHIP_CHECK(copyOut(layer_count, d_count, cells, s));
  return hipStreamSynchronize(s);
}
OHMHIP_ABI_CATCH

int ohmhip_map_heightmap_layered_device(ohmhip_map_t m, const ohmhip_heightmap_layered_params *params,
                                        uint32_t layer_capacity, float *d_occupancy, void *d_voxels24, void *d_mean8,
                                        uint32_t *d_source_visit, uint8_t *d_layer_count, uint32_t *d_visit_log,
                                        uint64_t visit_log_capacity, ohmhip_heightmap_layered_stats *stats)
try
{
  if (!d_occupancy || !d_voxels24 || !stats || layer_capacity == 0)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  ohmhip_heightmap_extents e;
  int seed[3];
  OHMHIP_CHECK(heightmapLayeredBegin(m, params, a, e, seed));
  *stats = ohmhip_heightmap_layered_stats{};
  if (!e.populated)
  {
    return OHMHIP_OK;
  }
  return heightmapLayeredDevice(m, *params, a, seed, layer_capacity, d_occupancy, d_voxels24, d_mean8, d_source_visit,
                                d_layer_count, d_visit_log, nullptr, d_visit_log ? visit_log_capacity : 0, *stats);
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_HEIGHTMAP_LAYERED_IMPL_H
