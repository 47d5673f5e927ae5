// heightmap_kernels.h -- the planar heightmap (ohm::Heightmap::buildHeightmap, HeightmapMode::kPlanar) built on the
// device from the resident map, read only.
//
//   k_heightmap_columns  1 lane / source column   rules 2-5 of include/ohmhip.h ("HEIGHTMAP"): supporting voxel, ground,
//                                                 the cell value; atomicMax of the walk index per heightmap cell
//   k_heightmap_cells    1 lane / heightmap cell  rule 6: the column with the largest walk index writes the cell; cells
//                                                 nobody wrote get the cleared values
//
// The integer state machines are findNearestSupportingVoxel2 / findNearestSupportingVoxel / findGround of
// ohmheightmap/private/HeightmapOperations.cpp:186-512 as written (tests/heightmap_ref.py is the same restatement on
// the CPU, from the same rule list); heights are fp64 in the reference's order (no FMA: -ffp-contract=off).  Rules 3-5
// are stated once, here -- hmSupportingVoxel, hmGround, hmCellRecord -- for this kernel and for hmWalkColumn of the fill
// and the layered builds (heightmap_walk_kernels.h), which differ in the walk key, the ladder's two flags and what they
// do with the cell.
//
// Shape.  A column is a run of voxels at the stride of one z slice (Z up), of one row (Y up) or of one float (X up).
// Columns are dealt to lanes in walk order, `a` innermost, 64 x 4 columns per workgroup: with Z or Y up `a` is the
// map's x, so the 64 lanes of a wave sit on 64 neighbouring floats and every step of the three scans (down, up, ground)
// is two whole 128-byte rows of a region block for the wave.  All lanes start at the same plane and step in lockstep;
// they differ in where they stop, not in what they load, so the loads stay coalesced until lanes retire.  The tile
// (region) of a voxel is resolved through the device hash only when a lane crosses a tile boundary and the block
// address stays in registers, like k_rays_query; the probes of a wave hit the same one or two table lines at the same
// step.  A workgroup-wide LDS table of the column's regions was not built: the probe is once per 32 steps per lane and
// the measured kernel time is a small part of the call.  With X up a column is a memory row and the
// lanes of a wave are a row apart: each load instruction touches 64 lines, but a lane then reads ITS line for the next
// 31 steps out of L1 / L2, so every line is still fetched from HBM once; correct on all six axes, fast on Z (and Y).
//
// A voxel of a region the map does not hold reads +inf and "no chunk" (resident tile through the region hash, else the
// host store's pinned record, else none).  For regions cut into tiles the chunk exists when any of its tiles does.
#ifndef OHMHIP_HEIGHTMAP_KERNELS_H
#define OHMHIP_HEIGHTMAP_KERNELS_H

#include "covariance_eigen_device.h"
#include "ndt_tsdf_device.h"
#include "query_kernels.h"

namespace ohmhip
{
enum : unsigned
{
  kHmVirtualSurfaces = 1u << 0,     ///< heightmap::kVirtualSurfaces (private/HeightmapOperations.h:45-63)
  kHmPromoteVirtualBelow = 1u << 2  ///< heightmap::kPromoteVirtualBelow
  // kBiasAbove and kIgnoreVirtualAbove are hmSupportingVoxel's parameters: each build passes its own
};

constexpr int kHmNoCell = -1;
constexpr uint32_t kHmVoxelWords = 6;  ///< HeightmapVoxel: 24 bytes

struct HeightmapArgs : MapReadView  ///< the source map
{
  MapConst hm;  ///< heightmap geometry: resolution, region_dim, origin, kdim (1 on the up axis), tile_split 1
  LayerView mean;             ///< no layer unless use_mean
  int use_mean;               ///< source has the mean layer and ignore_voxel_mean is off
  LayerView covariance;       ///< no layer unless surface_normals
  int surface_normals;        ///< OHMHIP_HM_SURFACE_NORMALS and the source has the covariance layer
  int min_g[3], max_g[3];     ///< rule 1: min_ext_key / max_ext_key as global voxel coordinates
  int plane;                  ///< rule 2: the plane key's up coordinate, clamped
  int a, b, up;               ///< heightmapAxisIndices
  int up_positive;            ///< up_axis >= 0
  int na, nb;                 ///< columns
  int cell0_a, cell0_b, ma, mb;  ///< dense result grid: first cell (global heightmap voxel coordinates), size
  int voxel_floor, voxel_ceiling, clearance_permissive;
  double min_clearance;
  unsigned flags;             ///< kHm*
  int generate_virtual;
  // per column records (k_heightmap_columns -> k_heightmap_cells)
  int *winner;                ///< [ma * mb] largest walk index that wrote the cell, -1: none
  float *rec_occ;             ///< [na * nb]
  uint32_t *rec_vox;          ///< [na * nb][6]
  uint2 *rec_mean;            ///< [na * nb]
  unsigned long long *counts; ///< [0] populated [1] cells written [2] columns whose cell left the grid [3] voxels inspected
  int count_inspected;
  // results, dense [mb][ma]
  float *out_occ;
  uint32_t *out_vox;
  uint2 *out_mean;            ///< null: not requested / not in use
  uint32_t *out_col;          ///< null: not requested
};

/// One lane's view of the source map: the tile it last touched.
struct HmCursor
{
  int tx, ty, tz;
  const float *occ;
  const uint2 *mean;
  int rx, ry, rz;  ///< tiled maps: the region whose existence is cached
  bool region_exists;
  uint32_t inspected;
};

/// A cursor that sits on no tile: the first hmSeek resolves.
__device__ inline HmCursor hmCursorStart()
{
  HmCursor c;
  c.tx = 0x7fffffff;
  c.ty = c.tz = 0;
  c.occ = nullptr;
  c.mean = nullptr;
  c.rx = 0x7fffffff;
  c.ry = c.rz = 0;
  c.region_exists = false;
  c.inspected = 0;
  return c;
}

/// The occupancy and mean blocks of tile (tx, ty, tz); false (and nulls) when the map has no such tile.
__device__ inline bool hmTile(const HeightmapArgs &a, int tx, int ty, int tz, const float *&occ, const uint2 *&mean)
{
  const FoundTile t = mapFindTile(a, tx, ty, tz);
  occ = (t.slot != kSlotUnassigned) ? a.occupancy + size_t(t.slot) * size_t(a.mc.region_voxels) : t.stored;
  mean = foundTileLayer<uint2>(t, a.mean, size_t(a.mc.region_voxels));
  return occ != nullptr;
}

/// Writing component `idx` of a 3-vector with selects (reading it: sel3): a run-time index into a local array would put
/// the array into scratch memory.
template <typename T>
__device__ inline void hmPut(T v[3], int idx, T value)
{
  v[0] = (idx == 0) ? value : v[0];
  v[1] = (idx == 1) ? value : v[1];
  v[2] = (idx == 2) ? value : v[2];
}

/// Moves the cursor to the tile of global voxel g and returns the voxel's index in it.
__device__ inline int hmSeek(const HeightmapArgs &a, HmCursor &c, const int g[3])
{
  int t[3], l[3];
#pragma unroll
  for (int axis = 0; axis < 3; ++axis)
  {
    splitGlobal(g[axis], a.mc.dim[axis], t[axis], l[axis]);
  }
  if (t[0] != c.tx || t[1] != c.ty || t[2] != c.tz)
  {
    c.tx = t[0];
    c.ty = t[1];
    c.tz = t[2];
    hmTile(a, t[0], t[1], t[2], c.occ, c.mean);
  }
  return l[0] + a.mc.dim[0] * (l[1] + a.mc.dim[1] * l[2]);
}

/// voxel.occupancy.chunk() != null for the voxel the cursor sits on (hmSeek first).
__device__ inline bool hmHasChunk(const HeightmapArgs &a, HmCursor &c)
{
  if (c.occ)
  {
    return true;
  }
  if (a.mc.tile_split[1] <= 1 && a.mc.tile_split[2] <= 1)
  {
    return false;
  }
  // a region cut into tiles: it exists when any of its tiles does (tiles without data are not created)
  const int ry = floorDiv(c.ty, a.mc.tile_split[1]);
  const int rz = floorDiv(c.tz, a.mc.tile_split[2]);
  if (c.rx != c.tx || c.ry != ry || c.rz != rz)
  {
    c.rx = c.tx;
    c.ry = ry;
    c.rz = rz;
    c.region_exists = false;
    for (int j = 0; j < a.mc.tile_split[2] && !c.region_exists; ++j)
    {
      for (int i = 0; i < a.mc.tile_split[1] && !c.region_exists; ++i)
      {
        const float *occ;
        const uint2 *mean;
        c.region_exists = hmTile(a, c.tx, ry * a.mc.tile_split[1] + i, rz * a.mc.tile_split[2] + j, occ, mean);
      }
    }
  }
  return c.region_exists;
}

/// The occupancy of global voxel g (+inf where the map holds nothing) and whether its region exists.
__device__ inline float hmRead(const HeightmapArgs &a, HmCursor &c, const int g[3], bool &has_chunk)
{
  const int vi = hmSeek(a, c, g);
  ++c.inspected;
  has_chunk = hmHasChunk(a, c);
  return c.occ ? c.occ[vi] : __int_as_float(0x7f800000);
}

/// SrcVoxel::occupancyType (private/HeightmapOperations.h:94-108).
__device__ inline int hmType(const HeightmapArgs &a, HmCursor &c, const int g[3])
{
  bool has;
  const float v = hmRead(a, c, g, has);
  if (!has)
  {
    return kOtNull;
  }
  if (v == __int_as_float(0x7f800000))
  {
    return kOtUnobserved;
  }
  return (v >= a.mc.threshold_value) ? kOtOccupied : kOtFree;
}

/// Rule 3, findNearestSupportingVoxel2 (private/HeightmapOperations.cpp:186-343) in the column of `seed`: the up
/// coordinate of the voxel found in `found` (valid when the returned offset >= 0).
__device__ inline int hmSearch(const HeightmapArgs &a, HmCursor &c, const int seed[3], int to_up, int step_limit,
                               bool search_up, int &found, bool &is_virtual)
{
  const bool allow_virtual = (a.flags & kHmVirtualSurfaces) != 0;
  const int up = a.up;
  const float inf = __int_as_float(0x7f800000);
  const int seed_up = sel3(up, seed);
  int vertical_range = (to_up - seed_up) + 1;  // rangeBetween(from, to)[up] + 1
  const int step = (vertical_range >= 0) ? 1 : -1;
  vertical_range = (vertical_range >= 0) ? vertical_range : -vertical_range;
  if (step_limit > 0)
  {
    vertical_range = min(vertical_range, step_limit);
  }
  bool have_virtual = false;
  int best_virtual = 0;
  bool last_unobserved = false;
  bool last_free = false;
  int last_key = seed_up;
  int cur[3] = { seed[0], seed[1], seed[2] };
  int cur_up = seed_up;
  if (search_up)
  {
    bool has;
    last_unobserved = hmRead(a, c, seed, has) == inf;  // isUnobservedOrNull
    cur_up += step;
  }
  else
  {
    ++vertical_range;
  }
  int offset = 0;
  const int dim_up = (up == 0) ? a.mc.kdim[0] : ((up == 1) ? a.mc.kdim[1] : a.mc.kdim[2]);
  for (int i = 0; i < vertical_range; ++i)
  {
    offset = (i > 0) ? i + 1 : (search_up ? 0 : 1);
    bool has;
    hmPut(cur, up, cur_up);
    const float v = hmRead(a, c, cur, has);
    const bool occupied = v >= a.mc.threshold_value && v != inf;
    const bool free = v < a.mc.threshold_value;
    const bool unobserved = !occupied && !free;
    if (occupied)
    {
      is_virtual = false;
      found = cur_up;
      return offset;
    }
    if (allow_virtual && search_up && free && last_unobserved && !have_virtual)
    {
      have_virtual = true;
      best_virtual = last_key;
    }
    if (allow_virtual && !search_up && unobserved && last_free)
    {
      have_virtual = true;
      best_virtual = cur_up;
    }
    last_unobserved = unobserved;
    last_free = free;
    last_key = cur_up;
    int next_step = step;
    if (!has)
    {
      // :321-328 a region that does not exist: jump out of it, so that the transition on its far side is still seen
      const int local = localCoord(cur_up, dim_up);
      next_step = (step > 0) ? dim_up - local : -(1 + local);
      i += abs(next_step) - 1;
    }
    cur_up += next_step;
  }
  is_virtual = have_virtual;
  found = best_virtual;
  return have_virtual ? offset : -1;
}

/// Rule 3, the selection ladder of findNearestSupportingVoxel (:346-419), rows in the order of
/// tests/heightmap_ref.py::supporting_voxel.  The planar build walks without kBiasAbove and with kIgnoreVirtualAbove
/// (Heightmap.cpp:375); the fill with kBiasAbove on every visit but the first and never kIgnoreVirtualAbove.  Returns
/// false when there is no candidate.
__device__ inline bool hmSupportingVoxel(const HeightmapArgs &a, HmCursor &c, const int seed[3], bool bias_above,
                                         bool ignore_virtual_above, int &candidate)
{
  const int min_up = sel3(a.up, a.min_g), max_up = sel3(a.up, a.max_g);
  const int down_to = a.up_positive ? min_up : max_up;
  const int up_to = a.up_positive ? max_up : min_up;
  int below = 0, above = 0;
  bool virtual_below = false, virtual_above = false;
  const int offset_below = hmSearch(a, c, seed, down_to, a.voxel_floor, false, below, virtual_below);
  const int offset_above = hmSearch(a, c, seed, up_to, a.voxel_ceiling, true, above, virtual_above);
  const bool have_below = offset_below >= 0;
  const bool have_above = offset_above >= 0;
  virtual_below = have_below && virtual_below && !(a.flags & kHmPromoteVirtualBelow);
  bool take_below;
  if (bias_above && have_below && have_above)
  {
    take_below = offset_below < offset_above;  // :367-373 the closer one, the one above on a tie
  }
  else if (have_below && virtual_above && !virtual_below)
  {
    take_below = true;
  }
  else if (have_above && !virtual_above && virtual_below)
  {
    take_below = false;
  }
  else if (ignore_virtual_above && have_below && virtual_above && virtual_below)
  {
    take_below = true;
  }
  else
  {
    take_below = have_below && (!have_above || offset_below <= offset_above ||
                                (!virtual_above && offset_below + offset_above >= a.clearance_permissive));
  }
  candidate = take_below ? below : above;
  return take_below ? have_below : have_above;
}

/// SrcVoxel::position / centre of global voxel g (private/HeightmapOperations.h:111-128): the centre, plus the decoded
/// mean when asked for and in use.  The cursor must sit on g's tile (hmSeek).
__device__ inline void hmPosition(const HeightmapArgs &a, const HmCursor &c, const int g[3], int vi, bool with_mean,
                                  double pos[3])
{
#pragma unroll
  for (int axis = 0; axis < 3; ++axis)
  {
    pos[axis] = globalVoxelCentreAxis(a.mc, axis, g[axis]);
  }
  if (with_mean && c.mean)
  {
    const D3 off = subVoxelToLocal(c.mean[vi].x, a.mc.resolution);
    pos[0] += off.x;
    pos[1] += off.y;
    pos[2] += off.z;
  }
}

__device__ inline double hmDot(const double p[3], const double up[3])
{
  return (p[0] * up[0] + p[1] * up[1]) + p[2] * up[2];  // glm::dot
}

/// subVoxelCoord (ohm/VoxelMeanCompute.h:69-92).
__device__ inline uint32_t hmSubVoxelCoord(const double v[3], double resolution)
{
  const int mean_positions = (1 << 10) - 1;
  const double mean_resolution = resolution / double(mean_positions);
  const double offset = double(0.5f) * resolution;
  uint32_t pattern = 0;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis)
  {
    int pos = pointToRegionCoord(v[axis] + offset, mean_resolution);
    pos = (pos >= 0 ? (pos < (1 << 10) ? pos : mean_positions) : 0);
    pattern |= uint32_t(pos) << (10 * axis);
  }
  return pattern | (1u << 31);
}

/// Words 2-4 of a cell's HeightmapVoxel (Heightmap.cpp:808-826): zeros, or -- with surface normals on, for an OCCUPIED
/// ground voxel -- the primary normal of its covariance turned towards up (D6 of include/ohmhip.h).  The cursor sits on
/// the ground voxel's tile and vi is the voxel's index in it.  The covariance is read here, once per cell written: the
/// cursor keeps a tile's occupancy block, not where the tile lives, so the tile is looked up once more.
__device__ inline void hmSurfaceNormal(const HeightmapArgs &a, const HmCursor &c, int vi, bool occupied,
                                       const double up_vec[3], uint32_t *vox)
{
  vox[2] = 0u;
  vox[3] = 0u;
  vox[4] = 0u;
  if (!a.surface_normals || !occupied)
  {
    return;
  }
  const float *cov =
    foundTileLayer<float>(mapFindTile(a, c.tx, c.ty, c.tz), a.covariance, size_t(a.mc.region_voxels) * 6u);
  if (!cov)
  {
    return;
  }
  float p[6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
  {
    p[i] = cov[size_t(vi) * 6u + i];
  }
  const CovEigen e = covarianceEigen(p);
  float normal[3];
  covarianceSurfaceNormal(e, up_vec, normal);
  vox[2] = __float_as_uint(normal[0]);
  vox[3] = __float_as_uint(normal[1]);
  vox[4] = __float_as_uint(normal[2]);
}

/// Rule 4, findGround (:422-512) from `candidate` up the column of `walk`.  False when the column has no ground.
__device__ inline bool hmGround(const HeightmapArgs &a, HmCursor &c, const int walk[3], int candidate,
                                const double up_vec[3], int &ground_up, double &clearance, bool &ground_observed_above)
{
  const int up = a.up;
  const int min_up = sel3(up, a.min_g), max_up = sel3(up, a.max_g);
  const int step_dir = a.up_positive ? 1 : -1;
  bool observed_above = false;
  double column_height = 1.7976931348623157e308;
  double column_clearance_height = column_height;
  int candidate_type = kOtNull;
  int last_type = kOtNull;
  int key[3] = { walk[0], walk[1], walk[2] };
  for (int key_up = candidate; key_up >= min_up && key_up <= max_up; key_up += step_dir)
  {
    hmPut(key, up, key_up);
    const int voxel_type = hmType(a, c, key);
    const bool last_is_unobserved = last_type == kOtUnobserved || last_type == kOtNull;
    observed_above = observed_above || (voxel_type != kOtNull && voxel_type != kOtUnobserved);
    if (voxel_type == kOtOccupied ||
        (a.generate_virtual && last_is_unobserved && voxel_type == kOtFree && candidate_type == kOtNull))
    {
      // sourceVoxelHeight (:167-184): the mean position for occupied voxels, the centre otherwise
      double pos[3];
      hmPosition(a, c, key, hmSeek(a, c, key), voxel_type == kOtOccupied, pos);
      const double height = hmDot(pos, up_vec);
      if (candidate_type != kOtNull)
      {
        column_clearance_height = height;
        if (column_clearance_height - column_height >= a.min_clearance)
        {
          break;
        }
      }
      column_height = column_clearance_height = height;
      ground_up = key_up;
      candidate_type = voxel_type;
      observed_above = false;
    }
    last_type = voxel_type;
  }
  if (candidate_type == kOtNull)
  {
    return false;
  }
  clearance = column_clearance_height - column_height;
  ground_observed_above = observed_above;
  return true;
}

constexpr long long kHmCellOutside = -2;  ///< hmCellRecord: the cell is not in the dense grid (cannot happen)

/// Rule 5 (Heightmap.cpp:619-671, addSurfaceVoxel :703-835) for ground voxel `ground`: writes the cell's value into
/// record `rec` of rec_occ / rec_vox / rec_mean and returns the dense index of the heightmap cell; kHmNoCell when the
/// voxel writes nothing.
__device__ inline long long hmCellRecord(const HeightmapArgs &a, HmCursor &c, const int ground[3], bool have_candidate,
                                         bool have_ground, double clearance, bool ground_observed_above,
                                         const double up_vec[3], size_t rec)
{
  const int up = a.up;
  const int voxel_type = have_candidate ? hmType(a, c, ground) : int(kOtNull);
  if (!(voxel_type == kOtOccupied || (voxel_type == kOtFree && a.generate_virtual)))
  {
    return kHmNoCell;
  }
  const int vi = hmSeek(a, c, ground);
  double pos[3];
  hmPosition(a, c, ground, vi, voxel_type == kOtOccupied, pos);
  const double src_height = hmDot(up_vec, pos);
  hmPut(pos, up, 0.0);
  int hr[3], hl[3];
  const bool ok = voxelKey(a.hm, pos, hr, hl);
  hmPut(hr, up, 0);
  hmPut(hl, up, 0);
  const int ca = sel3(a.a, hr) * sel3(a.a, a.hm.kdim) + sel3(a.a, hl) - a.cell0_a;
  const int cb = sel3(a.b, hr) * sel3(a.b, a.hm.kdim) + sel3(a.b, hl) - a.cell0_b;
  if (!(ok && ca >= 0 && ca < a.ma && cb >= 0 && cb < a.mb))
  {
    return kHmCellOutside;
  }
  double centre[3];
#pragma unroll
  for (int axis = 0; axis < 3; ++axis)
  {
    centre[axis] = voxelCentreAxis(a.hm, axis, hr[axis], hl[axis]);
  }
  const float height = float(src_height - hmDot(centre, up_vec));
  uint32_t samples = 0;
  if (c.mean)
  {
    samples = min(c.mean[vi].y, 0xffffu);
    const double rel[3] = { pos[0] - centre[0], pos[1] - centre[1], pos[2] - centre[2] };
    a.rec_mean[rec] = make_uint2(hmSubVoxelCoord(rel, a.hm.resolution), 1u);
  }
  a.rec_occ[rec] = (voxel_type == kOtOccupied) ? 1.0f : -1.0f;
  uint32_t *vox = a.rec_vox + rec * kHmVoxelWords;
  vox[0] = __float_as_uint(height);
  vox[1] = __float_as_uint(float(clearance));
  hmSurfaceNormal(a, c, vi, voxel_type == kOtOccupied, up_vec, vox);
  // layer kHvlBaseLayer (0) | flags << 8 | contributing_samples << 16
  vox[5] = ((have_ground && ground_observed_above) ? 0x100u : 0u) | (samples << 16);
  return (long long)(size_t(cb) * size_t(a.ma) + size_t(ca));
}

/// What a column kernel ends on, every lane of the wave present: the wave's count of lanes that wrote a cell into
/// counts[0], and under OHMHIP_HEIGHTMAP_COUNT the voxels the lane inspected into counts[3].
__device__ inline void hmColumnTail(const HeightmapArgs &a, const HmCursor &c, bool wrote)
{
  const unsigned long long wrote_mask = __ballot(wrote);
  if ((threadIdx.x & 63u) == 0u && wrote_mask)
  {
    atomicAdd(&a.counts[0], (unsigned long long)__popcll(wrote_mask));
  }
  if (a.count_inspected && c.inspected)
  {
    atomicAdd(&a.counts[3], (unsigned long long)c.inspected);
  }
}

__global__ void __launch_bounds__(256) k_heightmap_columns(HeightmapArgs a)
{
  const int ia = int(blockIdx.x) * 64 + int(threadIdx.x & 63u);
  const int ib = int(blockIdx.y) * 4 + int(threadIdx.x >> 6);
  bool wrote = false;
  HmCursor c = hmCursorStart();
  if (ia < a.na && ib < a.nb)
  {
    const int up = a.up;
    double up_vec[3] = { 0.0, 0.0, 0.0 };
    hmPut(up_vec, up, a.up_positive ? 1.0 : -1.0);
    int walk[3] = { 0, 0, 0 };
    hmPut(walk, a.a, sel3(a.a, a.min_g) + ia);
    hmPut(walk, a.b, sel3(a.b, a.min_g) + ib);
    hmPut(walk, up, a.plane);
    int candidate = 0;
    const bool have_candidate = hmSupportingVoxel(a, c, walk, false, true, candidate);
    double clearance = 0.0;
    int ground_up = 0;
    bool ground_observed_above = false;
    const bool have_ground =
      have_candidate && hmGround(a, c, walk, candidate, up_vec, ground_up, clearance, ground_observed_above);
    int ground[3] = { walk[0], walk[1], walk[2] };
    if (have_ground)
    {
      hmPut(ground, up, ground_up);
    }
    const size_t col = size_t(ib) * size_t(a.na) + size_t(ia);
    const long long cell =
      hmCellRecord(a, c, ground, have_candidate, have_ground, clearance, ground_observed_above, up_vec, col);
    if (cell >= 0)
    {
      atomicMax(&a.winner[cell], int(col));
      wrote = true;
    }
    else if (cell == kHmCellOutside)
    {
      atomicAdd(&a.counts[2], 1ull);
    }
  }
  hmColumnTail(a, c, wrote);
}

/// Rule 6: the winners write; every other cell is cleared (occupancy +inf, zeros).
__global__ void __launch_bounds__(256) k_heightmap_cells(HeightmapArgs a)
{
  const size_t cell = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t cells = size_t(a.ma) * size_t(a.mb);
  bool written = false;
  if (cell < cells)
  {
    const int w = a.winner[cell];
    written = w >= 0;
    a.out_occ[cell] = written ? a.rec_occ[w] : __int_as_float(0x7f800000);
    uint32_t *vox = a.out_vox + cell * kHmVoxelWords;
#pragma unroll
    for (uint32_t i = 0; i < kHmVoxelWords; ++i)
    {
      vox[i] = written ? a.rec_vox[size_t(w) * kHmVoxelWords + i] : 0u;
    }
    if (a.out_mean)
    {
      a.out_mean[cell] = (written && a.use_mean) ? a.rec_mean[w] : make_uint2(0u, 0u);
    }
    if (a.out_col)
    {
      a.out_col[cell] = uint32_t(w);
    }
  }
  const unsigned long long mask = __ballot(written);
  if ((threadIdx.x & 63u) == 0u && mask)
  {
    atomicAdd(&a.counts[1], (unsigned long long)__popcll(mask));
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_HEIGHTMAP_KERNELS_H
