// heightmap_fill_impl.h -- host side of the flood-fill heightmap (heightmap_fill_kernels.h): the planar call's
// prologue, source view and staged outputs (heightmap_impl.h), then the generation walk (heightmap_walk_impl.h) with
// the fill's visit grid and replay kernel.
// Included after heightmap_walk_impl.h in ohmhip_map.hip's translation unit.
#ifndef OHMHIP_HEIGHTMAP_FILL_IMPL_H
#define OHMHIP_HEIGHTMAP_FILL_IMPL_H

namespace
{
static_assert(sizeof(HeightmapFillArgs) <= 4096, "kernel arguments are passed by value");

/// The fill's steps of the walk: nothing of its own per generation, one event kernel, one synchronise.
struct HeightmapFillBuild
{
  HeightmapFillArgs f{};
  unsigned id_bits = 0;
  static constexpr auto columns = k_hmfill_columns;

  int generation(ohmhip_map_s::QueryState &, size_t, size_t, uint32_t, hipStream_t) { return OHMHIP_OK; }

  int events(size_t count, hipStream_t s)
  {
    hipLaunchKernelGGL(k_hmfill_replay, dim3(uint32_t((9 * count + 255) / 256)), dim3(256), 0, s, f);
    return hipGetLastError();
  }

  int settle(ohmhip_map_s::QueryState &, const uint32_t *, size_t, hipStream_t s) { return hipStreamSynchronize(s); }
};

/// The walk, results into device arrays; returns with the stream idle.  The log as in heightmapWalkFinish.
int heightmapFillDevice(ohmhip_map_t m, const HeightmapArgs &geometry, const int seed[3], float *d_occ, void *d_vox,
                        void *d_mean, uint32_t *d_visit, uint32_t *d_log, DevBuf *log_staging, uint64_t log_capacity,
                        ohmhip_heightmap_fill_stats &stats)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  HeightmapFillBuild build;
  HeightmapFillArgs &f = build.f;
  static_cast<HeightmapArgs &>(f) = geometry;
  OHMHIP_CHECK(heightmapSourceView(m, f));
  const size_t cells = size_t(f.ma) * size_t(f.mb);
  const size_t grid_cells = size_t(f.na) * size_t(f.nb);
  f.grid_cells = uint32_t(grid_cells);
  build.id_bits = bitsFor((unsigned long long)grid_cells + 1ull);
  OHMHIP_CHECK(ensureAs(qs.hm_winner, cells, s, f.cell_visit));
  OHMHIP_CHECK(ensureAs(qs.hm_counts, 8, s, f.counts));
  OHMHIP_CHECK(ensureAs(qs.hmf_grid, grid_cells, s, f.grid));
  f.out_occ = d_occ;
  f.out_vox = static_cast<uint32_t *>(d_vox);
  f.out_mean = static_cast<uint2 *>(d_mean);
  f.out_visit = d_visit;
  f.out_log = d_log;
  OHMHIP_CHECK(hipMemsetAsync(f.grid, 0xff, sizeof(int) * grid_cells, s));
  OHMHIP_CHECK(hipMemsetAsync(f.counts, 0, sizeof(unsigned long long) * 8, s));
  hipLaunchKernelGGL(k_hmfill_clear, dim3(uint32_t((cells + 255) / 256)), dim3(256), 0, s, f);
  OHMHIP_CHECK(hipGetLastError());

  OHMHIP_CHECK(heightmapWalk(m, build, seed, stats));
  unsigned long long counts[8] = {};
  const int status = heightmapWalkFinish(m, f, k_hmfill_finish, "fill", log_staging, log_capacity, stats, counts);
  stats.populated = counts[0];
  stats.cells = counts[1];
  stats.revisits = counts[4];
  return status;
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
  return heightmapWalkToHost(m, occupancy, voxels24, mean8, source_visit, size_t(a.ma) * size_t(a.mb), visit_log,
                             visit_log_capacity, *stats, [&](const HeightmapStaged &d, DevBuf *log, uint64_t capacity) {
                               return heightmapFillDevice(m, a, seed, d.occ, d.vox, d.mean, d.source, nullptr, log,
                                                          capacity, *stats);
                             });
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
