// heightmap_layered_impl.h -- host side of the layered heightmaps (heightmap_layered_kernels.h): the fill call's
// prologue and source view, the generation walk (heightmap_walk_impl.h) with the touched lists' node pool growing
// beside the queue and the slot planes growing by doubling when a column asks for more; then L6, L7 and the results.
// Included after heightmap_walk_impl.h in ohmhip_map.hip's translation unit.
#ifndef OHMHIP_HEIGHTMAP_LAYERED_IMPL_H
#define OHMHIP_HEIGHTMAP_LAYERED_IMPL_H

namespace
{
static_assert(sizeof(HeightmapLayeredArgs) <= 4096, "kernel arguments are passed by value");

constexpr uint32_t kHmlInitialSlots = 2;
constexpr uint32_t kHmlMostSlots = 255;  ///< of one column: beyond it OHMHIP_ERR_CAPACITY

/// What the three layered entry points do after their own pointer checks: the layered parameters' own check, then
/// heightmapBegin.
int heightmapLayeredBegin(ohmhip_map_t m, const ohmhip_heightmap_layered_params *p, HeightmapArgs &a,
                          ohmhip_heightmap_extents &e, int *reference = nullptr)
{
  if (!p || p->reserved != 0)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return heightmapBegin(m, &p->base, kHmBuildLayered, a, e, reference);
}

/// The slot planes [slots][cells]: new blocks for exactly `slots`, the first `used` planes copied.
int layeredPlanes(ohmhip_map_s::QueryState &qs, HeightmapLayeredArgs &f, uint32_t slots, uint32_t used, hipStream_t s)
{
  const size_t cells = f.hm_cells;
  if (size_t(slots) * cells > (size_t(1) << 31))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  const auto reserve = [&](DevBuf &plane, size_t bytes_per_cell) {
    return growAndKeep(plane, bytes_per_cell * cells * slots, bytes_per_cell * cells * used, 0, s);
  };
  OHMHIP_CHECK(reserve(qs.hml_occ, sizeof(float)));
  OHMHIP_CHECK(reserve(qs.hml_vox, sizeof(uint32_t) * kHmVoxelWords));
  OHMHIP_CHECK(reserve(qs.hml_mean, sizeof(uint2)));
  OHMHIP_CHECK(reserve(qs.hml_visit, sizeof(uint32_t)));
  OHMHIP_CHECK(reserve(qs.hml_ground, sizeof(unsigned long long)));
  f.slot_capacity = slots;
  f.sl_occ = static_cast<float *>(qs.hml_occ.ptr);
  f.sl_vox = static_cast<uint32_t *>(qs.hml_vox.ptr);
  f.sl_mean = static_cast<uint2 *>(qs.hml_mean.ptr);
  f.sl_visit = static_cast<uint32_t *>(qs.hml_visit.ptr);
  f.sl_ground = static_cast<unsigned long long *>(qs.hml_ground.ptr);
  return OHMHIP_OK;
}

/// The layered builds' steps of the walk: the node pool, flags and heights per generation, two event kernels, and
/// after the synchronise the planes regrown and the adds run again while a column asks for more.
struct HeightmapLayeredBuild
{
  HeightmapLayeredArgs f{};
  unsigned id_bits = 0;
  static constexpr auto columns = k_hml_columns;

  int generation(ohmhip_map_s::QueryState &qs, size_t begin, size_t count, uint32_t number, hipStream_t s)
  {
    // an accepted offer takes one node
    OHMHIP_CHECK(walkQueueReserve(qs.hml_nodes, begin + 9 * count, begin + count, s));
    OHMHIP_CHECK(ensureAs(qs.hml_flags, count, s, f.key_flags));
    OHMHIP_CHECK(ensureAs(qs.hml_height, count, s, f.src_height));
    f.nodes = static_cast<uint2 *>(qs.hml_nodes.ptr);
    f.node_capacity = uint32_t(std::min<size_t>(qs.hml_nodes.bytes / sizeof(uint2), 0xffffffffu));
    f.stamp = number;
    return OHMHIP_OK;
  }

  int adds(size_t count, hipStream_t s)
  {
    hipLaunchKernelGGL(k_hml_adds, dim3(uint32_t((9 * count + 255) / 256)), dim3(256), 0, s, f);
    return hipGetLastError();
  }

  int events(size_t count, hipStream_t s)
  {
    hipLaunchKernelGGL(k_hml_offers, dim3(uint32_t((9 * count + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    return adds(count, s);
  }

  int settle(ohmhip_map_s::QueryState &qs, uint32_t *next, size_t count, hipStream_t s)
  {
    OHMHIP_CHECK(hipMemcpyAsync(next + 1, f.words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OHMHIP_CHECK(hipStreamSynchronize(s));
    while (next[1] > f.slot_capacity)
    {
      // a column asked for more slots: its adds are not applied yet, every other cell's are
      OHMHIP_CHECK(layeredPlanes(qs, f, std::max(next[1], 2 * f.slot_capacity), f.slot_capacity, s));
      OHMHIP_CHECK(hipMemsetAsync(f.words + 1, 0, sizeof(uint32_t), s));
      OHMHIP_CHECK(adds(count, s));
      OHMHIP_CHECK(hipMemcpyAsync(next + 1, f.words + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      OHMHIP_CHECK(hipStreamSynchronize(s));
    }
    return OHMHIP_OK;
  }
};

/// The walk and what follows it, results into device arrays of layer_capacity planes; returns with the stream idle.
/// The log as in heightmapWalkFinish.
int heightmapLayeredDevice(ohmhip_map_t m, const ohmhip_heightmap_layered_params &params, const HeightmapArgs &geometry,
                           const int seed[3], uint32_t layer_capacity, float *d_occ, void *d_vox, void *d_mean,
                           uint32_t *d_visit, uint8_t *d_count, uint32_t *d_log, DevBuf *log_staging,
                           uint64_t log_capacity, ohmhip_heightmap_layered_stats &stats)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  HeightmapLayeredBuild build;
  HeightmapLayeredArgs &f = build.f;
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
  build.id_bits = bitsFor((unsigned long long)grid_cells + cells + 1ull);
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
  OHMHIP_CHECK(ensureAs(qs.hm_counts, kHmlCountWords, s, f.counts));
  OHMHIP_CHECK(ensureAs(qs.hml_head, grid_cells, s, f.touched_head));
  OHMHIP_CHECK(ensureAs(qs.hml_cell_state, 3 * cells, s, f.slot_count));
  OHMHIP_CHECK(ensureAs(qs.hml_words, 2, s, f.words));
  f.applied = f.slot_count + cells;
  f.multi = f.applied + cells;
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
  OHMHIP_CHECK(walkQueueReserve(qs.hml_nodes, 1 << 14, 0, s));

  OHMHIP_CHECK(heightmapWalk(m, build, seed, stats));
  if (f.filter_threshold)
  {
    // L6
    const size_t slots = size_t(f.slot_capacity) * cells;
    unsigned long long *ground_sorted = nullptr;
    OHMHIP_CHECK(ensureAs(qs.hm_walk.keys_a, slots, s, f.keys));
    OHMHIP_CHECK(ensureAs(qs.hml_ground_sorted, slots, s, ground_sorted));
    f.ground_sorted = ground_sorted;
    hipLaunchKernelGGL(k_hml_keys, dim3(uint32_t((slots + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
    OHMHIP_CHECK(heightmapSort(qs.hm_walk.temp, f.keys, ground_sorted, slots, 64, s));
    hipLaunchKernelGGL(k_hml_filter, dim3(uint32_t((slots + 255) / 256)), dim3(256), 0, s, f);
    OHMHIP_CHECK(hipGetLastError());
  }
  unsigned long long counts[kHmlCountWords] = {};
  // (also INTERNAL: a node beyond the pool, which holds one per queue entry)
  const int status = heightmapWalkFinish(m, f, k_hml_finish, "layered", log_staging, log_capacity, stats, counts);
  stats.populated = counts[0];
  stats.cells = counts[kHmlCells];
  stats.voxels = counts[kHmlVoxels];
  stats.repeats = counts[kHmlRepeats];
  stats.too_close = counts[kHmlTooClose];
  stats.filtered = counts[kHmlFiltered];
  stats.multi_layer_columns = counts[kHmlMultiColumns];
  stats.layers = uint32_t(counts[kHmlLayers]);
  return (status == OHMHIP_OK && stats.layers > kHmlMostSlots) ? OHMHIP_ERR_CAPACITY : status;
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
  return heightmapWalkToHost(m, occupancy, voxels24, mean8, source_visit, size_t(layer_capacity) * cells, visit_log,
                             visit_log_capacity, *stats, [&](const HeightmapStaged &d, DevBuf *log, uint64_t capacity) {
                               uint8_t *d_count = nullptr;
                               OHMHIP_CHECK(stageOut(qs.hml_out_count, layer_count, cells, s, d_count));
                               OHMHIP_CHECK(heightmapLayeredDevice(m, *params, a, seed, layer_capacity, d.occ, d.vox,
                                                                   d.mean, d.source, d_count, nullptr, log, capacity,
                                                                   *stats));
                               return copyOut(layer_count, d_count, cells, s);
                             });
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
