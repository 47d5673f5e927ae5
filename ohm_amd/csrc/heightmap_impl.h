// heightmap_impl.h -- host side of the planar heightmap (heightmap_kernels.h): argument checks, rule 1 (extents) and
// the dense result grid in fp64 on the host, then the two kernels on the map's stream.  Included at the end of
// ohmhip_map.hip's translation unit, after read_side.h (mapReadView, the refusal, the optional outputs).
#ifndef OHMHIP_HEIGHTMAP_IMPL_H
#define OHMHIP_HEIGHTMAP_IMPL_H

namespace
{
/// Which build an entry point belongs to: the value is the first ohm::HeightmapMode it builds.
enum HeightmapBuild
{
  kHmBuildPlanar = 0,
  kHmBuildFill = 1,    ///< heightmap_fill_impl.h
  kHmBuildLayered = 2  ///< heightmap_layered_impl.h: modes 2 and 3
};

/// What every heightmap entry point checks before any device work.  A mode that has entry points of its own before
/// these is an invalid argument here; any other mode the build does not cover is not supported.
int heightmapRefusal(ohmhip_map_t m, const ohmhip_heightmap_params *p, HeightmapBuild build = kHmBuildPlanar)
{
  if (!p)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (!std::isfinite(p->grid_resolution) || !(p->grid_resolution > 0.0) || p->up_axis < -3 || p->up_axis > 2)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  for (const double v : { p->floor, p->ceiling, p->min_clearance })
  {
    if (!std::isfinite(v) || v < 0.0)
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
  }
  if (int(p->mode) < int(build))
  {
    return OHMHIP_ERR_INVALID_ARG;  // planar: ohmhip_map_heightmap; simple fill: ohmhip_map_heightmap_fill
  }
  if (int(p->mode) != int(build) && !(build == kHmBuildLayered && p->mode == 3))
  {
    return OHMHIP_ERR_UNSUPPORTED;
  }
  if (!m)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  return readSideRefusal(m, OHMHIP_LID_OCCUPANCY);
}

/// Rules 1 and 2 and the dense grid, on the host in fp64: fills the geometry fields of `a` and `e`.  The map is settled
/// by the caller.  e.populated == 0: nothing to build.  `reference`, when asked for and there is something to build:
/// voxelKey(reference_pos) as global voxel coordinates, clamped into the extents on all three axes (the fill's seed,
/// F2; its up coordinate is a.plane).
int heightmapGeometry(ohmhip_map_t m, const ohmhip_heightmap_params *p, HeightmapArgs &a, ohmhip_heightmap_extents &e,
                      int *reference = nullptr)
{
  std::memset(&e, 0, sizeof(e));
  a = HeightmapArgs{};
  const MapConst &mc = m->mc;
  a.mc = mc;
  const int up_axis = int(p->up_axis);
  const int up = (up_axis >= 0) ? up_axis : -up_axis - 1;
  a.up = up;
  a.a = (up == 0) ? 1 : 0;
  a.b = (up == 2) ? 1 : 2;
  a.up_positive = up_axis >= 0;
  a.use_mean = m->pool.layers[OHMHIP_LID_MEAN] && !(p->flags & OHMHIP_HM_IGNORE_VOXEL_MEAN);
  e.use_mean = uint8_t(a.use_mean);
  a.surface_normals = ((p->flags & OHMHIP_HM_SURFACE_NORMALS) && m->pool.layers[OHMHIP_LID_COVARIANCE]) ? 1 : 0;
  a.generate_virtual = (p->flags & OHMHIP_HM_GENERATE_VIRTUAL_SURFACE) ? 1 : 0;
  a.flags = (a.generate_virtual ? kHmVirtualSurfaces : 0u) |
            ((p->flags & OHMHIP_HM_PROMOTE_VIRTUAL_BELOW) ? kHmPromoteVirtualBelow : 0u);
  a.voxel_floor = pointToRegionCoord(p->floor, mc.resolution);
  a.voxel_ceiling = pointToRegionCoord(p->ceiling, mc.resolution);
  a.clearance_permissive = std::max(1, pointToRegionCoord(p->min_clearance, mc.resolution) - 1);
  a.min_clearance = p->min_clearance;

  // rule 1: the regions present, in the caller's coordinates (resident and host store)
  size_t n_regions = 0;
  OHMHIP_CHECK(ohmhip_map_region_count(m, &n_regions));
  if (n_regions == 0)
  {
    return OHMHIP_OK;
  }
  std::vector<int16_t> keys(3 * n_regions);
  size_t listed = 0;
  OHMHIP_CHECK(ohmhip_map_regions(m, keys.data(), n_regions, &listed));
  n_regions = std::min(n_regions, listed);
  double lo[3], hi[3];
  for (int c = 0; c < 3; ++c)
  {
    lo[c] = std::numeric_limits<double>::max();
    hi[c] = -std::numeric_limits<double>::max();
  }
  for (size_t i = 0; i < n_regions; ++i)
  {
    for (int c = 0; c < 3; ++c)
    {
      const double centre = int(keys[3 * i + c]) * mc.region_dim[c];  // MapRegion::centre: no origin
      lo[c] = std::min(lo[c], centre - 0.5 * mc.region_dim[c]);
      hi[c] = std::max(hi[c], centre + 0.5 * mc.region_dim[c]);
    }
  }
  for (int c = 0; c < 3; ++c)
  {
    if (p->cull_max[c] - p->cull_min[c] > 0)
    {
      lo[c] = p->cull_min[c];
      hi[c] = p->cull_max[c];
    }
  }
  // OccupancyMap::voxelKey, the reference's key maths with no tile range: the keys are the caller's
  MapConst kc = mc;
  kc.tile_split[0] = kc.tile_split[1] = kc.tile_split[2] = 1;
  int rmin[3], lmin[3], rmax[3], lmax[3], rref[3], lref[3];
  if (!voxelKey(kc, lo, rmin, lmin) || !voxelKey(kc, hi, rmax, lmax) || !voxelKey(kc, p->reference_pos, rref, lref))
  {
    return OHMHIP_OK;  // a null key: the reference walks nothing
  }
  for (int c = 0; c < 3; ++c)
  {
    a.min_g[c] = rmin[c] * mc.kdim[c] + lmin[c];
    a.max_g[c] = rmax[c] * mc.kdim[c] + lmax[c];
    e.min_region[c] = int16_t(rmin[c]);
    e.min_local[c] = uint8_t(lmin[c]);
    e.max_region[c] = int16_t(rmax[c]);
    e.max_local[c] = uint8_t(lmax[c]);
    const int ref = std::min(std::max(rref[c] * mc.kdim[c] + lref[c], a.min_g[c]), a.max_g[c]);
    if (c == up)
    {
      a.plane = ref;  // rule 2
    }
    if (reference)
    {
      reference[c] = ref;
    }
  }
  const long long na = (long long)a.max_g[a.a] - a.min_g[a.a] + 1;
  const long long nb = (long long)a.max_g[a.b] - a.min_g[a.b] + 1;
  if (na <= 0 || nb <= 0)
  {
    return OHMHIP_OK;
  }
  if (na * nb > (1ll << 31))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  // the heightmap's own geometry (Heightmap.cpp:124-142)
  const int region_size = p->region_size ? int(p->region_size) : 128;
  a.hm = MapConst{};
  a.hm.resolution = p->grid_resolution;
  for (int c = 0; c < 3; ++c)
  {
    a.hm.kdim[c] = a.hm.dim[c] = (c == up) ? 1 : region_size;
    a.hm.region_dim[c] = a.hm.kdim[c] * p->grid_resolution;  // ohm/OccupancyMap.cpp:200-202
    a.hm.origin[c] = p->origin[c];
    a.hm.tile_split[c] = 1;
  }
  a.hm.region_voxels = a.hm.dim[0] * a.hm.dim[1] * a.hm.dim[2];
  double c_lo[3], c_hi[3];
  for (int c = 0; c < 3; ++c)
  {
    c_lo[c] = voxelCentreAxis(mc, c, rmin[c], lmin[c]) - 0.5 * mc.resolution;
    c_hi[c] = voxelCentreAxis(mc, c, rmax[c], lmax[c]) + 0.5 * mc.resolution;
  }
  c_lo[up] = c_hi[up] = 0.0;
  int hr0[3], hl0[3], hr1[3], hl1[3];
  if (!voxelKey(a.hm, c_lo, hr0, hl0) || !voxelKey(a.hm, c_hi, hr1, hl1))
  {
    return OHMHIP_ERR_CAPACITY;  // the heightmap's keys cannot address the source's extents
  }
  a.cell0_a = hr0[a.a] * region_size + hl0[a.a];
  a.cell0_b = hr0[a.b] * region_size + hl0[a.b];
  const long long ma = (long long)(hr1[a.a] * region_size + hl1[a.a]) - a.cell0_a + 1;
  const long long mb = (long long)(hr1[a.b] * region_size + hl1[a.b]) - a.cell0_b + 1;
  if (ma <= 0 || mb <= 0 || ma * mb > (1ll << 31))
  {
    return OHMHIP_ERR_CAPACITY;
  }
  a.na = int(na);
  a.nb = int(nb);
  a.ma = int(ma);
  a.mb = int(mb);
  e.na = uint32_t(na);
  e.nb = uint32_t(nb);
  e.ma = uint32_t(ma);
  e.mb = uint32_t(mb);
  e.first_region[0] = int16_t(hr0[a.a]);
  e.first_region[1] = int16_t(hr0[a.b]);
  e.first_local[0] = uint8_t(hl0[a.a]);
  e.first_local[1] = uint8_t(hl0[a.b]);
  e.populated = 1;
  return OHMHIP_OK;
}

/// What the planar and the fill entry points do after their own pointer checks: the refusal, the map settled, the
/// geometry (the layered ones: heightmapLayeredBegin).
/// OHMHIP_OK with e.populated == 0: nothing to build -- the caller zeroes its outputs and answers OHMHIP_OK.
int heightmapBegin(ohmhip_map_t m, const ohmhip_heightmap_params *p, HeightmapBuild build, HeightmapArgs &a,
                   ohmhip_heightmap_extents &e, int *reference = nullptr)
{
  OHMHIP_CHECK(heightmapRefusal(m, p, build));
  OHMHIP_SETTLE(m);
  return heightmapGeometry(m, p, a, e, reference);
}

/// The source map as the column kernels of both builds see it (a.use_mean and a.surface_normals from
/// heightmapGeometry): the read view, the mean and covariance layers where in use, the development counter.
int heightmapSourceView(ohmhip_map_t m, HeightmapArgs &a)
{
  OHMHIP_CHECK(mapReadView(m, a));
  a.mean = layerView(m, OHMHIP_LID_MEAN, a.use_mean);
  a.covariance = layerView(m, OHMHIP_LID_COVARIANCE, a.surface_normals);
  const char *env = std::getenv("OHMHIP_HEIGHTMAP_COUNT");  // development: count the voxels inspected (counts[3])
  a.count_inspected = (env && std::atoi(env) != 0) ? 1 : 0;
  return OHMHIP_OK;
}

/// The device copies of the four result arrays of a host-array call (QueryState::hm_out_*): null where the caller
/// passed none.  `source` is source_column or source_visit.
struct HeightmapStaged
{
  float *occ = nullptr;
  char *vox = nullptr, *mean = nullptr;
  uint32_t *source = nullptr;

  int stage(ohmhip_map_s::QueryState &qs, const float *occupancy, const void *voxels24, const void *mean8,
            const uint32_t *source_host, size_t n, hipStream_t s)
  {
    OHMHIP_CHECK(stageOut(qs.hm_out_occ, occupancy, n, s, occ));
    OHMHIP_CHECK(stageOut(qs.hm_out_vox, voxels24, 24 * n, s, vox));
    OHMHIP_CHECK(stageOut(qs.hm_out_mean, mean8, 8 * n, s, mean));
    return stageOut(qs.hm_out_col, source_host, n, s, source);
  }

  int copyBack(float *occupancy, void *voxels24, void *mean8, uint32_t *source_host, size_t n, hipStream_t s) const
  {
    OHMHIP_CHECK(copyOut(occupancy, occ, n, s));
    OHMHIP_CHECK(copyOut(voxels24, vox, 24 * n, s));
    OHMHIP_CHECK(copyOut(mean8, mean, 8 * n, s));
    return copyOut(source_host, source, n, s);
  }
};

/// The two kernels on the map's stream, results into device arrays.  d_counts: 4 uint64 of the query's own.
int heightmapDevice(ohmhip_map_t m, HeightmapArgs &a, float *d_occ, void *d_vox, void *d_mean, uint32_t *d_col)
{
  hipStream_t s = m->stream;
  ohmhip_map_s::QueryState &qs = m->query;
  OHMHIP_CHECK(heightmapSourceView(m, a));
  const size_t columns = size_t(a.na) * size_t(a.nb);
  const size_t cells = size_t(a.ma) * size_t(a.mb);
  OHMHIP_CHECK(qs.hm_winner.ensure(sizeof(int) * cells, false, s));
  OHMHIP_CHECK(qs.hm_rec_occ.ensure(sizeof(float) * columns, false, s));
  OHMHIP_CHECK(qs.hm_rec_vox.ensure(sizeof(uint32_t) * kHmVoxelWords * columns, false, s));
  OHMHIP_CHECK(qs.hm_rec_mean.ensure(sizeof(uint2) * columns, false, s));
  OHMHIP_CHECK(qs.hm_counts.ensure(sizeof(unsigned long long) * 4, false, s));
  a.winner = static_cast<int *>(qs.hm_winner.ptr);
  a.rec_occ = static_cast<float *>(qs.hm_rec_occ.ptr);
  a.rec_vox = static_cast<uint32_t *>(qs.hm_rec_vox.ptr);
  a.rec_mean = static_cast<uint2 *>(qs.hm_rec_mean.ptr);
  a.counts = static_cast<unsigned long long *>(qs.hm_counts.ptr);
  a.out_occ = d_occ;
  a.out_vox = static_cast<uint32_t *>(d_vox);
  a.out_mean = static_cast<uint2 *>(d_mean);
  a.out_col = d_col;
  OHMHIP_CHECK(hipMemsetAsync(a.winner, 0xff, sizeof(int) * cells, s));
  OHMHIP_CHECK(hipMemsetAsync(a.counts, 0, sizeof(unsigned long long) * 4, s));
  hipLaunchKernelGGL(k_heightmap_columns, dim3(uint32_t((a.na + 63) / 64), uint32_t((a.nb + 3) / 4)), dim3(256), 0, s,
                     a);
  OHMHIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_heightmap_cells, dim3(uint32_t((cells + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
}  // namespace

extern "C" {

int ohmhip_map_heightmap_extents(ohmhip_map_t m, const ohmhip_heightmap_params *params, ohmhip_heightmap_extents *extents)
try
{
  if (!extents)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  return heightmapBegin(m, params, kHmBuildPlanar, a, *extents);
}
OHMHIP_ABI_CATCH

int ohmhip_map_heightmap(ohmhip_map_t m, const ohmhip_heightmap_params *params, float *occupancy, void *voxels24,
                         void *mean8, uint32_t *source_column, uint64_t *populated, uint64_t *cells)
try
{
  if (!occupancy || !voxels24 || !populated || !cells)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  ohmhip_heightmap_extents e;
  OHMHIP_CHECK(heightmapBegin(m, params, kHmBuildPlanar, a, e));
  *populated = 0;
  *cells = 0;
  if (!e.populated)
  {
    return OHMHIP_OK;
  }
  hipStream_t s = m->stream;
  const size_t n = size_t(a.ma) * size_t(a.mb);
  HeightmapStaged d;
  OHMHIP_CHECK(d.stage(m->query, occupancy, voxels24, mean8, source_column, n, s));
  OHMHIP_CHECK(heightmapDevice(m, a, d.occ, d.vox, d.mean, d.source));
  OHMHIP_CHECK(d.copyBack(occupancy, voxels24, mean8, source_column, n, s));
  unsigned long long counts[4] = { 0, 0, 0, 0 };
  OHMHIP_CHECK(hipMemcpyAsync(counts, a.counts, sizeof(counts), hipMemcpyDeviceToHost, s));
  OHMHIP_CHECK(hipStreamSynchronize(s));
  *populated = counts[0];
  *cells = counts[1];
  if (a.count_inspected)
  {
    std::fprintf(stderr, "ohmhip heightmap: %llu voxels inspected, %d x %d columns\n", counts[3], a.na, a.nb);
  }
  return counts[2] ? OHMHIP_ERR_INTERNAL : OHMHIP_OK;  // (a column's cell outside the grid: cannot happen)
}
OHMHIP_ABI_CATCH

int ohmhip_map_heightmap_device(ohmhip_map_t m, const ohmhip_heightmap_params *params, float *d_occupancy,
                                void *d_voxels24, void *d_mean8, uint32_t *d_source_column, uint64_t *d_counts)
try
{
  if (!d_occupancy || !d_voxels24)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  HeightmapArgs a;
  ohmhip_heightmap_extents e;
  OHMHIP_CHECK(heightmapBegin(m, params, kHmBuildPlanar, a, e));
  if (!e.populated)
  {
    return d_counts ? int(hipMemsetAsync(d_counts, 0, 2 * sizeof(uint64_t), m->stream)) : OHMHIP_OK;
  }
  OHMHIP_CHECK(heightmapDevice(m, a, d_occupancy, d_voxels24, d_mean8, d_source_column));
  if (d_counts)
  {
    OHMHIP_CHECK(hipMemcpyAsync(d_counts, a.counts, 2 * sizeof(uint64_t), hipMemcpyDeviceToDevice, m->stream));
  }
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

}  // extern "C"

#endif  // OHMHIP_HEIGHTMAP_IMPL_H
