// ray_front_kernels.h -- the front of the occupancy ray-integration path: from the caller's rays to per-region segment
// records and sample keys (gfx950).
//
// Pipeline per ray batch (all on one HIP stream; see DESIGN.md for the full picture):
//   k_ray_setup         1 lane / ray       filter, keys, fp64 line-walk set-up; enumerate the regions the ray crosses;
//                                          segment and sample counts per region in a workgroup-level LDS table
//   k_plan              1 workgroup        scans over the touched regions: segment / sample offsets, equal-size chunks
//                                          (largest first), sample-sort order
//   k_ray_bin           1 lane / ray       scatter segment records (resume state + voxel count) and sample keys into
//                                          the per-region ranges; set the sample bitmask
//   ... then the stages of sample_sort_kernels.h, walk_kernel.h and apply_kernels.h
//
// Also here because they share the per-ray code: k_count_passed (the ray filter alone) and k_rekey_samples (the sample
// keys of a batch again, after the NDT / TSDF key buffer had to grow).
#ifndef OHMHIP_RAY_FRONT_KERNELS_H
#define OHMHIP_RAY_FRONT_KERNELS_H

#include "batch_scratch.h"
#include "ray_filter_chain.h"
#include "region_table.h"
#include "walk_device.h"

namespace ohmhip
{
// ---------------------------------------------------------------------------------------------------------------------
// Region enumeration for one ray: a 3-way merge of the per-axis region-crossing steps in walk order.
// ---------------------------------------------------------------------------------------------------------------------
struct RegionCursor
{
  int region[3];  ///< current region
  int next_j[3];  ///< step index (1-based) of the next region crossing per axis; > total => none left
  int dir[3];
};

__device__ inline void regionCursorInit(const MapConst &mc, const RayWalk &rw, RegionCursor &rc)
{
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    int local;
    splitGlobal(rw.g0[a], mc.dim[a], rc.region[a], local);
    rc.dir[a] = rwDir(rw, a);
    // Steps needed to leave the start region along this axis.
    rc.next_j[a] = (rc.dir[a] > 0) ? (mc.dim[a] - local) : (local + 1);
  }
}

/// Advance to the next region crossing.  Returns false when the ray crosses no further region boundary.
/// On success `axis`/`j` identify the step which enters the new region, `t_entry` is that step's time -- stepTime() of the
/// winning axis, the value the merge has just compared -- and rc.region is updated.
__device__ inline bool regionCursorNext(const MapConst &mc, const RayWalk &rw, RegionCursor &rc, int &axis, int &j,
                                        double &t_entry)
{
  int best = -1;
  double best_t = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    if (rc.next_j[a] <= rw.total[a])
    {
      const double t = stepTime(rw.init[a], rw.delta[a], rc.next_j[a]);
      if (best < 0 || stepPrecedes(t, a, best_t, best))
      {
        best = a;
        best_t = t;
      }
    }
  }
  if (best < 0)
  {
    return false;
  }
  axis = best;
  t_entry = best_t;
  j = sel3(best, rc.next_j[0], rc.next_j[1], rc.next_j[2]);
  // Per-axis updates spelled out: a run-time index here would push the cursor into scratch memory.
  if (best == 0)
  {
    rc.region[0] += rc.dir[0];
    rc.next_j[0] += mc.dim[0];
  }
  else if (best == 1)
  {
    rc.region[1] += rc.dir[1];
    rc.next_j[1] += mc.dim[1];
  }
  else
  {
    rc.region[2] += rc.dir[2];
    rc.next_j[2] += mc.dim[2];
  }
  return true;
}

/// Is the voxel reached by step (axis, j) the ray's end voxel?  (All three axes exhausted.)  True only when j is the
/// last step on its axis and every step of the other axes precedes it.  `ta` is the step's time.
__device__ inline bool stepReachesEnd(const RayWalk &rw, int axis, int j, double ta)
{
  if (j != sel3(axis, rw.total[0], rw.total[1], rw.total[2]))
  {
    return false;
  }
  bool all_before = true;
#pragma unroll
  for (int b = 0; b < 3; ++b)
  {
    if (rw.total[b] > 0)
    {
      const double tb = stepTime(rw.init[b], rw.delta[b], rw.total[b]);
      all_before = all_before && (b == axis || stepPrecedes(tb, b, ta, axis));
    }
  }
  return all_before;
}

/// ... for a caller that has not got the step's time at hand: computed only where the step is its axis' last.  (The
/// counting passes: with the time handed through their loop k_ray_setup's and k_route_mask's register allocation moves,
/// k_route_mask's across an occupancy step.)
__device__ inline bool stepReachesEnd(const RayWalk &rw, int axis, int j)
{
  if (j != sel3(axis, rw.total[0], rw.total[1], rw.total[2]))
  {
    return false;
  }
  return stepReachesEnd(rw, axis, j, stepTime(sel3(axis, rw.init[0], rw.init[1], rw.init[2]),
                                              sel3(axis, rw.delta[0], rw.delta[1], rw.delta[2]), j));
}

/// Walk the regions a ray crosses and call emit(region key) for every ray-region segment which produces at least one
/// voxel visit: what the counting passes need (k_ray_bin enumerates the same segments with forEachBinSegment, which
/// also builds their records).  Segments in regions another replica owns (MapConst::owner_world > 1) are skipped.
template <typename F>
__device__ inline void forEachSegment(const MapConst &mc, const RayWalk &rw, F emit)
{
  auto f = [&](uint64_t key) {
    if (ownsRegion(mc, key))
    {
      emit(key);
    }
  };
  if (!(rw.flags & kRwValid) || !(rw.flags & kRwWalk))
  {
    return;
  }
  const int manhattan = rw.total[0] + rw.total[1] + rw.total[2];
  const bool include_end = (rw.flags & kRwIncludeEnd) != 0;
  RegionCursor rc;
  regionCursorInit(mc, rw, rc);
  if (manhattan > 0 || include_end)
  {
    f(packRegionKey(rc.region[0], rc.region[1], rc.region[2]));
  }
  int axis, j;
  double ta;
  while (regionCursorNext(mc, rw, rc, axis, j, ta))
  {
    // Entering a region at the ray's end voxel only produces work when the end voxel is part of the ray.
    if (stepReachesEnd(rw, axis, j) && !include_end)
    {
      continue;
    }
    f(packRegionKey(rc.region[0], rc.region[1], rc.region[2]));
  }
}

/// Per-ray part of the fixed-point walk predictor (see Segment): the step deltas in fixed point, with the step direction
/// in the top bit, and whether the ray has to be walked exactly throughout.
struct RayFix
{
  uint32_t e0, e1, e2;
  bool poison;
};

__device__ inline RayFix rayFix(const MapConst &mc, const RayWalk &rw)
{
  RayFix rf;
  rf.poison = false;
  double t_last = 0;       // time of the ray's last real step
  double t_phantom = dInf();  // earliest step the predictor would take beyond an axis' last real one
  uint32_t e[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    e[a] = 0;
    if (rw.total[a] > 0)
    {
      const double ex = rw.delta[a] * mc.fix_scale;
      // (negated comparisons: NaN fails them and poisons the ray)
      rf.poison = rf.poison || !(ex >= 1.0);
      e[a] = !(ex >= 1.0) ? 0u : ((ex >= double(kFixMaxDelta)) ? kFixMaxDelta : uint32_t(ex));
      const double tl = stepTime(rw.init[a], rw.delta[a], rw.total[a]);
      const double tp = rw.init[a] + rw.delta[a] * double(rw.total[a]);
      // (a start point ON a voxel face -- every ray of a sensor standing on the voxel lattice -- can give a first
      // crossing time that rounds to -1e-18 instead of 0: anything above minus one predictor unit quantises to 0 within
      // the predictor's one-unit error per value, so only times below that poison the ray)
      rf.poison = rf.poison || !(tl * mc.fix_scale > -1.0) || !(tp >= tl);
      t_last = (tl > t_last) ? tl : t_last;
      t_phantom = (tp < t_phantom) ? tp : t_phantom;
    }
    e[a] |= rwSign(rw, a) ? kSegNegative : 0u;
  }
  // An axis which has taken its last step keeps stepping in the predictor.  That is harmless when every such phantom
  // step lies at or beyond the last real step of the ray (it then never leads a step the walk still needs by the trust
  // margin); where the end point's key and the geometry disagree (end points within the 1e-6 quantisation slack of a
  // region face) that can fail, and the ray is walked exactly.
  rf.poison = rf.poison || !(t_phantom >= t_last);
  rf.e0 = e[0];
  rf.e1 = e[1];
  rf.e2 = e[2];
  return rf;
}

/// Fixed-point time of the next step along one axis at a region entry (see Segment): the axis has taken k steps and the
/// region is entered at t_base.  An axis without steps left gives kFixFar -- time_next = inf
/// (ohm/LineWalkCompute.h:299-301) -- and `live` false.  `ok` is cleared when the value cannot be represented safely
/// (negative or non-finite): the segment is then poisoned.
__device__ inline uint32_t fixTime(const MapConst &mc, double init, double delta, int total, uint32_t k, double t_base,
                                   bool &live, bool &ok)
{
  live = int(k) < total;
  const double t = (k == 0) ? init : init + delta * double(k);
  const double x = (t - t_base) * mc.fix_scale;
  ok = ok && (!live || x > -1.0);  // (false for NaN; (-1, 0) quantises to 0, still within one unit of the true time)
  const uint32_t f = !(x >= 1.0) ? 0u : ((x >= double(kFixFar)) ? kFixFar : uint32_t(x));
  return live ? f : kFixFar;
}

/// The walk kernel's record of the ray-region segment a ray starts when it has taken k0, k1, k2 steps along the axes at
/// time t_base: everything but the voxel count and the ray word.  kPlain: every region edge is a power of two (see
/// k_ray_bin).
template <bool kPlain>
__device__ inline void segmentHead(const MapConst &mc, const RayWalk &rw, const RayFix &rf, const RegionCursor &rc,
                                   uint32_t k0, uint32_t k1, uint32_t k2, double t_base, Segment &sg)
{
  bool ok = !rf.poison;
  bool live0, live1, live2;
  const uint32_t f0 = fixTime(mc, rw.init[0], rw.delta[0], rw.total[0], k0, t_base, live0, ok);
  const uint32_t f1 = fixTime(mc, rw.init[1], rw.delta[1], rw.total[1], k1, t_base, live1, ok);
  const uint32_t f2 = fixTime(mc, rw.init[2], rw.delta[2], rw.total[2], k2, t_base, live2, ok);
  // A poisoned record is all zeros but for the directions.  An axis without steps left never moves: its delta is
  // irrelevant, zero keeps the candidate at kFixFar.
  sg.f[0] = ok ? f0 : 0u;
  sg.f[1] = ok ? f1 : 0u;
  sg.f[2] = ok ? f2 : 0u;
  sg.e[0] = (ok && live0) ? rf.e0 : (rf.e0 & kSegNegative);
  sg.e[1] = (ok && live1) ? rf.e1 : (rf.e1 & kSegNegative);
  sg.e[2] = (ok && live2) ? rf.e2 : (rf.e2 & kSegNegative);
  // The voxel the segment starts in: k steps from the ray's first along the axis' direction (dir = +-1, so g0 + dir * k
  // without the multiplication: dir >> 1 is 0 or -1, and (k ^ -1) - -1 = -k).
  auto local = [&](int g0, int dir, uint32_t k, int dim) {
    const int g = g0 + ((int(k) ^ (dir >> 1)) - (dir >> 1));
    return kPlain ? (g & (dim - 1)) : localCoord(g, dim);
  };
  const int l0 = local(rw.g0[0], rc.dir[0], k0, mc.dim[0]);
  const int l1 = local(rw.g0[1], rc.dir[1], k1, mc.dim[1]);
  const int l2 = local(rw.g0[2], rc.dir[2], k2, mc.dim[2]);
  sg.vox = uint32_t(l0 + l1 * mc.dim[0] + l2 * mc.dim[0] * mc.dim[1]);
}

/// stepsBefore()'s arithmetic route for the binning pass, which asks for the two other axes at every region crossing.
/// `fast` holds the tests of that route which depend on the ray and the axis alone -- total != 0, a positive finite
/// delta, |init| <= 4 delta: forEachBinSegment evaluates them once per ray -- so that only the tests on x are left per
/// crossing.  Returns false when the count has to come from stepsBefore() itself.  x < 0 <=> floor(x) + 1 <= 0, so one
/// clamp to [0, total] is stepsBefore's  (x < 0) ? 0 : min(count, total); it also gives the 0 of an axis without steps,
/// whatever x is there.
__device__ inline bool stepsBeforeQuick(double init, double rdelta, int total, bool fast, double ta, int &n)
{
  const double x = (ta - init) * rdelta;
  const double whole = floor(x);
  const double frac = x - whole;
  n = min(max(int(whole) + 1, 0), total);
  return fast && frac > 1e-5 && frac < 1.0 - 1e-5 && fabs(x) < 1048576.0;
}

/// Walk the regions a ray crosses as forEachSegment does and call emit(region key, record) with the walk kernel's
/// record of every ray-region segment: the fixed-point predictor at the moment the region is entered, the first voxel,
/// the number of voxels visited in the region and the ray word with its first / end flags.  Every segment carries its
/// own resume state, so dropping the segments of regions another replica owns does not change what the others do.
///
/// A record is built when its region is entered and emitted when the NEXT entry tells how many voxels it holds:
/// emission trails the enumeration by one.  kPlain: the map is not partitioned and its region edges are powers of two
/// (see k_ray_bin).
template <bool kPlain, typename F>
__device__ inline void forEachBinSegment(const MapConst &mc, const RayWalk &rw, const RayFix &rf, uint32_t ray, F emit)
{
  if (!(rw.flags & kRwValid) || !(rw.flags & kRwWalk))
  {
    return;
  }
  const int manhattan = rw.total[0] + rw.total[1] + rw.total[2];
  const bool include_end = (rw.flags & kRwIncludeEnd) != 0;
  if (manhattan == 0 && !include_end)
  {
    return;  // no voxel visited, and no region crossing either
  }
  const bool all_mine = kPlain || mc.owner_world <= 1u;  // (a map that is not partitioned: no test per segment)
  auto f = [&](uint64_t key, const Segment &sg) {
    if (all_mine || ownsRegion(mc, key))
    {
      emit(key, sg);
    }
  };
  RegionCursor rc;
  regionCursorInit(mc, rw, rc);
  // Reciprocals of the step deltas for the step-count estimates (one division per axis per ray, not per crossing), and
  // per axis whether stepsBefore's arithmetic route is open to the ray at all.
  const double r0 = 1.0 / rw.delta[0];
  const double r1 = 1.0 / rw.delta[1];
  const double r2 = 1.0 / rw.delta[2];
  bool fast[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    fast[a] = rw.total[a] != 0 && rw.delta[a] > 0 && rw.delta[a] < dInf() && fabs(rw.init[a]) <= 4.0 * rw.delta[a];
  }
  // The ray's first segment starts in its origin voxel at time 0.
  uint64_t p_key = packRegionKey(rc.region[0], rc.region[1], rc.region[2]);
  Segment p;
  segmentHead<kPlain>(mc, rw, rf, rc, 0u, 0u, 0u, 0.0, p);
  p.ray = ray | ((rw.flags & kRwExcludeStart) ? kSegSkipFirst : 0u);
  int p_sum = 0;
  int axis, j;
  double ta;
    while (regionCursorNext(mc, rw, rc, axis, j, ta))
  {
    // Entering a region at the ray's end voxel only produces work when the end voxel is part of the ray.
    if (stepReachesEnd(rw, axis, j, ta) && !include_end)
    {
      continue;
    }
    const uint64_t key = packRegionKey(rc.region[0], rc.region[1], rc.region[2]);
    // Steps taken along each axis when the region is entered: j on the entering axis, stepsBefore() on the others.  All
    // three quick estimates run in straight-line code (the lanes of a wave enter on different axes); the few counts they
    // cannot vouch for -- x within 1e-5 of a whole number, degenerate deltas -- come from stepsBefore() itself.
    int n0, n1, n2;
    const bool exact0 = !stepsBeforeQuick(rw.init[0], r0, rw.total[0], fast[0], ta, n0) && rw.total[0] != 0 && axis != 0;
    const bool exact1 = !stepsBeforeQuick(rw.init[1], r1, rw.total[1], fast[1], ta, n1) && rw.total[1] != 0 && axis != 1;
    const bool exact2 = !stepsBeforeQuick(rw.init[2], r2, rw.total[2], fast[2], ta, n2) && rw.total[2] != 0 && axis != 2;
    if (exact0 || exact1 || exact2)
    {
#pragma unroll 1
      for (int b = 0; b < 3; ++b)
      {
        if (sel3(b, exact0, exact1, exact2))
        {
          const int n = stepsBefore(sel3(b, rw.init[0], rw.init[1], rw.init[2]), sel3(b, rw.delta[0], rw.delta[1], rw.delta[2]),
                                    sel3(b, r0, r1, r2), sel3(b, rw.total[0], rw.total[1], rw.total[2]), b, axis, ta);
          n0 = (b == 0) ? n : n0;
          n1 = (b == 1) ? n : n1;
          n2 = (b == 2) ? n : n2;
        }
      }
    }
    n0 = (axis == 0) ? j : n0;
    n1 = (axis == 1) ? j : n1;
    n2 = (axis == 2) ? j : n2;
    const int sum = n0 + n1 + n2;
    p.vox |= uint32_t(sum - p_sum) << kSegVoxelBits;
    f(p_key, p);
    p_key = key;
    segmentHead<kPlain>(mc, rw, rf, rc, uint32_t(n0), uint32_t(n1), uint32_t(n2), ta, p);
    p.ray = ray;
    p_sum = sum;
  }
  p.vox |= (uint32_t(manhattan - p_sum) + (include_end ? 1u : 0u)) << kSegVoxelBits;
  p.ray |= include_end ? kSegEnd : 0u;
  f(p_key, p);
}

/// Region / voxel of the ray's sample (end) voxel.
__device__ inline void sampleVoxel(const MapConst &mc, const RayWalk &rw, uint64_t &region_key, uint32_t &vi)
{
  int r1[3], l1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    splitGlobal(rw.g0[a] + rwDir(rw, a) * rw.total[a], mc.dim[a], r1[a], l1[a]);
  }
  region_key = packRegionKey(r1[0], r1[1], r1[2]);
  vi = uint32_t(l1[0] + l1[1] * mc.dim[0] + l1[2] * mc.dim[0] * mc.dim[1]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Ray order inside a binning workgroup.  A lane enumerates its ray's region crossings one after the other, so a wave
// runs as long as its longest ray: with rays in arrival order (a lidar's beams have unrelated ranges) a third of the
// lane slots idle.  The workgroup therefore visits its rays by descending extent (counting sort on the ray's Manhattan
// extent in regions, 64 bins, positions in LDS): the rays of one wave then cross about the same number of regions.
// The order is irrelevant to the result -- segment records and sample keys carry the ray index.  (The bins are read out
// of the RayWalk records, a strided pass over all of them ahead of the loop that loads them whole.  A byte per ray
// written by k_ray_setup instead was measured: the binning pass got 5 us SLOWER -- profiles/r07_notes.md.)
// ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kRayOrderBins = 64;

struct RayOrder
{
  uint32_t bins[kRayOrderBins];
  uint16_t perm[kBinRaysPerBlock];
};

__device__ inline uint32_t rayExtentBin(const MapConst &mc, unsigned flags, const int total[3])
{
  if (!(flags & kRwValid) || !(flags & kRwWalk))
  {
    return 0;
  }
  const int max_dim = max(mc.dim[0], max(mc.dim[1], mc.dim[2]));
  const uint32_t manhattan = uint32_t(total[0] + total[1] + total[2]);
  return min(manhattan >> (31 - __clz(max_dim)), kRayOrderBins - 1u);
}

/// Build the order of the workgroup's `n_local` rays from their extent bins (bin_of(k) = bin of the thread's k-th ray,
/// local index threadIdx.x + k * blockDim.x; at most 8 rays per thread).  Ends with a barrier.
template <typename BinOf>
__device__ inline void buildRayOrder(RayOrder &order, uint32_t n_local, BinOf bin_of)
{
  if (threadIdx.x < kRayOrderBins)
  {
    order.bins[threadIdx.x] = 0;
  }
  __syncthreads();
  uint32_t my_bins[8];
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
  {
    const uint32_t idx = threadIdx.x + k * blockDim.x;
    my_bins[k] = 0;
    if (idx < n_local)
    {
      my_bins[k] = kRayOrderBins - 1u - bin_of(k, idx);  // descending extent
      atomicAdd(&order.bins[my_bins[k]], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < kRayOrderBins)
  {
    const uint32_t count = order.bins[threadIdx.x];
    uint32_t incl = count;
#pragma unroll
    for (int d = 1; d < int(kRayOrderBins); d <<= 1)
    {
      const uint32_t up = __shfl_up(incl, d);
      incl += (int(threadIdx.x) >= d) ? up : 0u;
    }
    order.bins[threadIdx.x] = incl - count;
  }
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k)
  {
    const uint32_t idx = threadIdx.x + k * blockDim.x;
    if (idx < n_local)
    {
      order.perm[atomicAdd(&order.bins[my_bins[k]], 1u)] = uint16_t(idx);
    }
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ray_setup: per-ray line-walk set-up + per-region segment counts.
// ---------------------------------------------------------------------------------------------------------------------
// (6 waves per SIMD: the kernel sits at 80-odd VGPRs, right at an allocation step -- 80 registers give a wave per SIMD
// more than 88 do, and the kernel is latency bound)
template <uint32_t kTab>
__global__ void __launch_bounds__(kBinThreads) __attribute__((amdgpu_waves_per_eu(6, 8)))
  k_ray_setup(MapConst mc, RegionTable rt, BatchScratch bs, const double *__restrict__ rays, uint32_t n_rays,
              unsigned ray_flags, RayWalk *__restrict__ walks, uint32_t rays_per_block, uint32_t tab_mask)
{
  __shared__ LdsRegionTableT<kTab> tab;
  __shared__ unsigned long long s_visits;
  __shared__ uint32_t s_rays_ok;
  __shared__ uint32_t s_list_n;
  for (uint32_t i = threadIdx.x; i <= tab_mask; i += blockDim.x)
  {
    tab.keys[i] = 0;
    tab.count[i] = 0;
    tab.cursor[i] = 0;
  }
  if (threadIdx.x == 0)
  {
    s_visits = 0;
    s_rays_ok = 0;
    s_list_n = 0;
  }
  __syncthreads();

  const uint32_t first = blockIdx.x * rays_per_block;
  const uint32_t last = min(first + rays_per_block, n_rays);
  unsigned long long my_visits = 0;
  uint32_t my_ok = 0;
  for (uint32_t ray = first + threadIdx.x; ray < last; ray += blockDim.x)
  {
    RayWalk rw;
    double start[3], end[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      start[a] = rays[size_t(ray) * 6 + a];
      end[a] = rays[size_t(ray) * 6 + 3 + a];
    }
    setupRay(mc, start, end, ray_flags, rw, ray);
    if (mc.owner_world > 1u && (rw.flags & kRwApplySample))
    {
      // A sample in a region another replica owns is that replica's to apply.
      uint64_t sample_key;
      uint32_t sample_vi;
      sampleVoxel(mc, rw, sample_key, sample_vi);
      rw.flags &= ownsRegion(mc, sample_key) ? ~0u : ~unsigned(kRwApplySample);
    }
    walks[ray] = rw;
    my_ok += (rw.flags & kRwPassed) ? 1u : 0u;
    if (rw.flags & kRwBeyondTiles)
    {
      atomicAdd(&bs.info->n_beyond_tiles, 1u);  // (rare by construction: no LDS stage, no register kept for it)
    }
    if (!(rw.flags & kRwValid))
    {
      continue;
    }
    // Visit accounting: Manhattan extent == number of voxels the walk reports before the end voxel.
    const int manhattan = rw.total[0] + rw.total[1] + rw.total[2];
    if (rw.flags & kRwWalk)
    {
      my_visits += (unsigned long long)manhattan;
      my_visits -= ((rw.flags & kRwExcludeStart) && manhattan > 0) ? 1u : 0u;
      my_visits += (rw.flags & kRwIncludeEnd) ? 1u : 0u;
    }
    my_visits += (rw.flags & kRwApplySample) ? 1u : 0u;

    forEachSegment(mc, rw, [&](uint64_t key) {
      const uint32_t e = ltabFindOrInsert(tab, key, tab_mask);
      if (e < kLtabSize)
      {
        atomicAdd(&tab.count[e], 1u);
      }
      else
      {
        // LDS table full (very long rays): count straight in the global table.
        const uint32_t h = regionInsert(rt, key, &bs.info->error);
        atomicAdd(&bs.seg_count[h], 1u);
        markTouched(bs, h);
      }
    });
    if (rw.flags & kRwApplySample)
    {
      // The sample's region must exist (and be listed as touched) even when no segment enters it.
      uint64_t key;
      uint32_t vi;
      sampleVoxel(mc, rw, key, vi);
      const uint32_t e = ltabFindOrInsert(tab, key, tab_mask);
      if (e < kLtabSize)
      {
        atomicAdd(&tab.cursor[e], 1u);
      }
      else
      {
        const uint32_t h = regionInsert(rt, key, &bs.info->error);
        atomicAdd(&bs.hit_count[h], 1u);
        markTouched(bs, h);
      }
    }
  }
  atomicAdd(&s_visits, my_visits);
  atomicAdd(&s_rays_ok, my_ok);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    atomicAdd(&bs.info->visits, s_visits);
    atomicAdd(&bs.info->rays_ok, (unsigned long long)s_rays_ok);
  }
  // One global insert + one counter atomic per (workgroup, region).
  for (uint32_t e = threadIdx.x; e <= tab_mask; e += blockDim.x)
  {
    const unsigned long long key = tab.keys[e];
    if (key)
    {
      const uint32_t h = regionInsert(rt, key, &bs.info->error);
      const uint32_t c = tab.count[e];
      if (c)
      {
        atomicAdd(&bs.seg_count[h], c);
      }
      markTouched(bs, h);
      const uint32_t hits = tab.cursor[e];
      if (hits)
      {
        atomicAdd(&bs.hit_count[h], hits);
      }
      WgRegion wr;
      wr.key = key;
      wr.count = c;
      wr.entry = e;
      wr.hash = h;
      wr.hits = hits;
      bs.wg_regions[size_t(blockIdx.x) * kLtabSize + atomicAdd(&s_list_n, 1u)] = wr;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0)
  {
    bs.wg_region_count[blockIdx.x] = s_list_n;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_plan: one block.  Exclusive scan of per-region segment counts over the touched list; build chunk list.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024)
  k_plan(RegionTable rt, BatchScratch bs, Chunk *__restrict__ chunks, uint32_t chunk_capacity,
         uint32_t chunk_segments, BatchInfo *__restrict__ host_info, BatchInfo *__restrict__ next_info,
         uint32_t *__restrict__ event_count, uint32_t inline_max_hits)
{
  constexpr uint32_t kSizeClasses = 32;  // chunk size classes for the largest-first order (class = 32 * size / max)
  constexpr int kRounds = 4;             // touched regions held in registers between the two passes: 4 x 1024
  constexpr uint32_t kBigQueue = 256;
  __shared__ uint32_t s_seg[16];
  __shared__ uint32_t s_chk[16];
  __shared__ uint32_t s_hit[16];
  __shared__ uint32_t s_seg_base;
  __shared__ uint32_t s_chk_base;
  __shared__ uint32_t s_hit_base;
  __shared__ uint32_t s_hit_max;
  __shared__ uint32_t s_class[kSizeClasses + 1];
  __shared__ uint32_t s_hclass[33];  // regions per sample-count class (class = bits of count - 1)
  __shared__ uint32_t s_big_n;
  __shared__ uint32_t s_big[kBigQueue][4];  // hash index, slot, segment offset, segment count
  __shared__ uint32_t s_n_apply_counts, s_n_apply_hits;
  const uint32_t n = bs.info->n_touched;
  const uint32_t tid = threadIdx.x;
  if (tid == 0)
  {
    s_seg_base = 0;
    s_chk_base = 0;
    s_hit_base = 0;
    s_hit_max = 0;
    s_big_n = 0;
    s_n_apply_counts = 0;
    s_n_apply_hits = 0;
  }
  if (tid <= kSizeClasses)
  {
    s_class[tid] = 0;
    s_hclass[tid] = 0;
  }
  __syncthreads();
  auto hitClass = [](uint32_t hits) { return uint32_t(32 - __clz(int(hits - 1u))) & 31u; };
  auto sizeClass = [&](uint32_t size) { return min(size * kSizeClasses / chunk_segments, kSizeClasses); };
  auto emit = [&](uint32_t h, uint32_t slot, uint32_t seg_excl, uint32_t cnt, uint32_t nchk, uint32_t per, uint32_t c) {
    const uint32_t begin = c * per;
    const uint32_t end = min(cnt, (c + 1) * per);
    const uint32_t pos = atomicAdd(&s_class[sizeClass(end - begin)], 1u);
    if (pos < chunk_capacity)
    {
      Chunk ch;
      ch.slot = slot;
      ch.seg_begin = seg_excl + begin;
      ch.seg_end = seg_excl + end;
      ch.hash_index = h | ((nchk == 1) ? 0x80000000u : 0u);
      chunks[pos] = ch;
    }
  };

  // Pass 1: segment offsets per region (prefix sum in touched order) and the chunk size histogram.  A region with
  // more than chunk_segments segments is split into equal chunks: nchk - 1 of `per` segments and a last one with the
  // rest.  The first kRounds x 1024 regions stay in registers for pass 2.
  uint32_t r_h[kRounds], r_cnt[kRounds], r_slot[kRounds], r_off[kRounds], r_hits[kRounds];
  for (uint32_t base = 0, round = 0; base < n; base += 1024, ++round)
  {
    const uint32_t i = base + tid;
    uint32_t h = 0, cnt = 0, nchk = 0, slot = 0, hits = 0;
    if (i < n)
    {
      h = bs.touched[i];
      cnt = bs.seg_count[h];
      hits = bs.hit_count[h];
      slot = rt.vals[h];
      nchk = (cnt + chunk_segments - 1) / chunk_segments;
      if (hits)
      {
        atomicMax(&s_hit_max, hits);
        atomicAdd(&s_hclass[hitClass(hits)], 1u);
      }
      // What the walk kernel leaves to the apply kernels (inline_max_hits: the most samples the walk replays for a
      // region it holds in one chunk; 0: it replays none): the counts of regions cut into several chunks, and the samples
      // of regions that are not held by exactly one chunk or are too dense.
      if (nchk > 1)
      {
        bs.apply_counts_list[atomicAdd(&s_n_apply_counts, 1u)] = h;
      }
      if (hits && (nchk != 1 || hits > inline_max_hits))
      {
        bs.apply_hits_list[atomicAdd(&s_n_apply_hits, 1u)] = h;
      }
    }
    // Inclusive scan of (segments, chunks, samples) over the 1024 threads: shuffles inside a wave, wave totals
    // through LDS.
    uint32_t inc_seg = cnt, inc_chk = nchk, inc_hit = hits;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
      const uint32_t a = __shfl_up(inc_seg, d);
      const uint32_t b = __shfl_up(inc_chk, d);
      const uint32_t c = __shfl_up(inc_hit, d);
      if (int(tid & 63u) >= d)
      {
        inc_seg += a;
        inc_chk += b;
        inc_hit += c;
      }
    }
    if ((tid & 63u) == 63u)
    {
      s_seg[tid >> 6] = inc_seg;
      s_chk[tid >> 6] = inc_chk;
      s_hit[tid >> 6] = inc_hit;
    }
    __syncthreads();
    uint32_t wave_seg = 0, wave_hit = 0, all_seg = 0, all_chk = 0, all_hit = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w)
    {
      const uint32_t a = s_seg[w];
      const uint32_t c = s_hit[w];
      wave_seg += (w < (tid >> 6)) ? a : 0u;
      wave_hit += (w < (tid >> 6)) ? c : 0u;
      all_seg += a;
      all_chk += s_chk[w];
      all_hit += c;
    }
    const uint32_t seg_excl = s_seg_base + wave_seg + inc_seg - cnt;
    const uint32_t hit_excl = s_hit_base + wave_hit + inc_hit - hits;
    if (i < n)
    {
      bs.seg_offset[h] = seg_excl;
      bs.seg_cursor[h] = 0;
      if (slot < rt.slot_capacity)
      {
        // The region's range in the sample list; hit_end doubles as the scatter cursor of k_ray_bin and ends up at
        // hit_begin + samples.
        bs.hit_begin[slot] = hit_excl;
        bs.hit_end[slot] = hit_excl;
        // use history (spill to host): also stamped by an attempt the host goes on to reject -- that is what makes
        // the eviction which follows spare the regions the repeated batch needs
        touchRegionUse(bs.last_use, slot, bs.stamp);
      }
      if (nchk)
      {
        const uint32_t per = (cnt + nchk - 1) / nchk;
        if (nchk > 1)
        {
          atomicAdd(&s_class[sizeClass(per)], nchk - 1);
        }
        atomicAdd(&s_class[sizeClass(cnt - (nchk - 1) * per)], 1u);
      }
    }
#pragma unroll
    for (int k = 0; k < kRounds; ++k)
    {
      if (uint32_t(k) == round)
      {
        r_h[k] = h;
        r_cnt[k] = cnt;
        r_slot[k] = slot;
        r_off[k] = seg_excl;
        r_hits[k] = hits;
      }
    }
    __syncthreads();
    if (tid == 1023)
    {
      s_seg_base += all_seg;
      s_chk_base += all_chk;
      s_hit_base += all_hit;
    }
    __syncthreads();
  }
  // Chunks are emitted largest class first: the persistent walk workgroups take them in this order, so the launch
  // ends on its smallest chunks.
  if (tid == 0)
  {
    uint32_t run = 0;
    for (int c = int(kSizeClasses); c >= 0; --c)
    {
      const uint32_t count = s_class[c];
      s_class[c] = run;
      run += count;
    }
  }
  if (tid == 64)
  {
    uint32_t run = 0;
    for (int c = 31; c >= 0; --c)
    {
      const uint32_t count = s_hclass[c];
      s_hclass[c] = run;
      run += count;
    }
    s_hclass[32] = run;
  }
  __syncthreads();
  // Pass 2: emit the chunk records.  Regions with a few chunks are written by their own thread; the big ones (the
  // regions around the sensor split into hundreds of chunks) are queued and written by the whole workgroup.
  for (uint32_t base = 0, round = 0; base < n; base += 1024, ++round)
  {
    const uint32_t i = base + tid;
    uint32_t h = 0, cnt = 0, slot = 0, seg_excl = 0, hits = 0;
#pragma unroll
    for (int k = 0; k < kRounds; ++k)
    {
      if (uint32_t(k) == round)
      {
        h = r_h[k];
        cnt = r_cnt[k];
        slot = r_slot[k];
        seg_excl = r_off[k];
        hits = r_hits[k];
      }
    }
    if (round >= uint32_t(kRounds) && i < n)
    {
      h = bs.touched[i];
      cnt = bs.seg_count[h];
      slot = rt.vals[h];
      seg_excl = bs.seg_offset[h];
      hits = bs.hit_count[h];
    }
    if (i < n && hits)
    {
      bs.hit_count[h] = 0;
      bs.sort_list[atomicAdd(&s_hclass[hitClass(hits)], 1u)] = h;
    }
    const uint32_t nchk = (i < n) ? (cnt + chunk_segments - 1) / chunk_segments : 0u;
    if (nchk)
    {
      const uint32_t per = (cnt + nchk - 1) / nchk;
      uint32_t q = kBigQueue;
      if (nchk > 4)
      {
        q = atomicAdd(&s_big_n, 1u);
      }
      if (q < kBigQueue)
      {
        s_big[q][0] = h;
        s_big[q][1] = slot;
        s_big[q][2] = seg_excl;
        s_big[q][3] = cnt;
      }
      else
      {
        for (uint32_t c = 0; c < nchk; ++c)
        {
          emit(h, slot, seg_excl, cnt, nchk, per, c);
        }
      }
    }
  }
  __syncthreads();
  const uint32_t n_big = min(s_big_n, kBigQueue);
  // One wave per queued region, one lane per chunk.
  for (uint32_t q = tid >> 6; q < n_big; q += 16)
  {
    const uint32_t cnt = s_big[q][3];
    const uint32_t nchk = (cnt + chunk_segments - 1) / chunk_segments;
    const uint32_t per = (cnt + nchk - 1) / nchk;
    for (uint32_t c = tid & 63u; c < nchk; c += 64)
    {
      emit(s_big[q][0], s_big[q][1], s_big[q][2], cnt, nchk, per, c);
    }
  }
  // "Modified" flags (bit 0: since the last syncVoxels(), bit 1: since the last replica merge, bit 2: since the last
  // clearance fold): only by a batch the host is going to run -- one it rejects (pool / chunk list exhausted) is rolled
  // back and must leave no trace here (the header promises a failing batch leaves the map as it was).
  if (!(bs.info->error & (kErrSlotsFull | kErrHashFull)) && *rt.n_slots <= rt.slot_capacity && s_chk_base <= chunk_capacity)
  {
    for (uint32_t i = tid; i < n; i += 1024)
    {
      const uint32_t slot = rt.vals[bs.touched[i]];
      if (slot < rt.slot_capacity)
      {
        bs.dirty[slot] |= 7u;  // kDirtySync | kDirtyMerge | kDirtyClearance (map_state.h)
      }
    }
  }
  if (tid == 0)
  {
    BatchInfo out = *bs.info;  // visits, rays, touched regions, errors: accumulated by k_ray_setup
    out.n_segments = s_seg_base;
    out.n_chunks = s_chk_base;
    out.n_slots = *rt.n_slots;
    out.n_hits = s_hit_base;
    out.max_region_hits = s_hit_max;
    out.n_hit_regions = s_hclass[32];
    out.n_apply_counts = s_n_apply_counts;
    out.n_apply_hits = s_n_apply_hits;
    *bs.info = out;
    // Housekeeping that would otherwise be separate copy / fill launches on the batch's critical path: the host's copy
    // of the summary goes straight to pinned memory, the next batch's summary and the walk's counters start at zero.
    *host_info = out;
    *next_info = BatchInfo{};
    event_count[0] = 0;  // deferred events
    event_count[1] = 0;  // walk chunk cursor
    event_count[3] = 0;  // traversal pass' chunk cursor (the stop-flag replay clears the word again before it uses it)
    __threadfence_system();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_ray_bin: scatter segments to region buckets, emit sample sort keys, set the per-region sample bitmask.
// Three steps per workgroup: count its segments per region in LDS, reserve one contiguous range per region with a
// single returning atomic, then re-enumerate and scatter through LDS cursors.
//
// hit_mask: null for a plain occupancy batch.  There the step that orders the sample keys sets the mask
// (k_sort_region_hits / k_hit_bounds: one atomic per voxel that receives samples instead of one per ray), and the pass
// writes nothing the previous batch's apply kernels still use -- which is what lets BatchRun::frontHalf launch it beside
// them.  NDT, TSDF and stop-flag batches order their samples with their events and keep the mask update here.
//
// kPlain: the instantiation for a map that is not partitioned (owner_world <= 1) and whose region edges are all powers
// of two -- the default map.  Both are known when the batch is launched (BatchRun::launchBin); the kernel then carries
// neither the ownership test nor the floor-modulo alternative of the local voxel coordinates through its
// per-segment loop.  The other instantiation takes every map.
// ---------------------------------------------------------------------------------------------------------------------
template <uint32_t kTab, bool kPlain>
__global__ void __launch_bounds__(kBinThreads)
  k_ray_bin(MapConst mc, RegionTable rt, BatchScratch bs, const RayWalk *__restrict__ walks, uint32_t n_rays,
            Segment *__restrict__ segments, uint32_t segment_capacity, unsigned long long *__restrict__ hit_keys,
            uint32_t *__restrict__ hit_mask, int ray_shift, int bucket_hits, uint32_t rays_per_block,
            uint32_t tab_mask)
{
  __shared__ LdsRegionTableT<kTab> tab;
  __shared__ uint32_t s_slot[kTab];  // region slot per table entry (kSlotUnassigned: not handed over by the set-up)
  if (bs.info->error & (kErrHashFull | kErrSlotsFull))
  {
    return;  // the batch's set-up overflowed the pool: the host grows it and repeats the batch
  }
  for (uint32_t i = threadIdx.x; i <= tab_mask; i += blockDim.x)
  {
    tab.keys[i] = 0;
    tab.count[i] = 0;
    tab.cursor[i] = 0;
    s_slot[i] = kSlotUnassigned;
  }
  __syncthreads();

  const uint32_t first = blockIdx.x * rays_per_block;
  const uint32_t last = min(first + rays_per_block, n_rays);
  const uint32_t mask_words = uint32_t(mc.region_voxels + 31) >> 5;

  // Step 1: the workgroup's regions with their segment and sample counts come from k_ray_setup (same rays, same LDS
  // table layout); reserve one contiguous range in every region bucket it feeds.
  const uint32_t n_wg_regions = bs.wg_region_count[blockIdx.x];
  for (uint32_t i = threadIdx.x; i < n_wg_regions; i += blockDim.x)
  {
    const WgRegion wr = bs.wg_regions[size_t(blockIdx.x) * kLtabSize + i];
    tab.keys[wr.entry] = wr.key;
    if (wr.count)
    {
      tab.cursor[wr.entry] = bs.seg_offset[wr.hash] + atomicAdd(&bs.seg_cursor[wr.hash], wr.count);
    }
    if (wr.hits)
    {
      // The samples' keys need the region's slot: looked up once per (workgroup, region) here, not once per ray.
      const uint32_t slot = rt.vals[wr.hash];
      s_slot[wr.entry] = slot;
      if (bucket_hits && slot < rt.slot_capacity)  // (a speculatively launched pass may see a batch whose slots ran out)
      {
        tab.count[wr.entry] = atomicAdd(&bs.hit_end[slot], wr.hits);
      }
    }
  }
  __syncthreads();
  // Step 2: sample keys and mask bits.  bucket_hits: the keys go straight into their region's range of the sample
  // list (k_sort_region_hits orders each range); otherwise they are written in ray order for a device-wide sort.
  auto emitSample = [&](uint32_t ray, const RayWalk &rw) {
    unsigned long long hk = kHitInvalid;
    uint32_t pos = ray;
    if ((rw.flags & kRwValid) && (rw.flags & kRwApplySample))
    {
      uint64_t key;
      uint32_t vi;
      sampleVoxel(mc, rw, key, vi);
      const uint32_t e = ltabFind(tab, key, tab_mask);
      uint32_t slot;
      if (e < kLtabSize)
      {
        // (A speculatively launched pass may run on a batch whose region inserts failed -- hash table full: the slot is
        // then unassigned, the host repeats the batch after growing the pool, nothing may be written here.)
        slot = s_slot[e];
        if (bucket_hits)
        {
          pos = atomicAdd(&tab.count[e], 1u);
        }
      }
      else
      {
        const uint32_t h = regionFind(rt, key);
        slot = (h != 0xffffffffu) ? rt.vals[h] : kSlotUnassigned;
        if (bucket_hits && slot < rt.slot_capacity)
        {
          pos = atomicAdd(&bs.hit_end[slot], 1u);  // LDS table overflow in k_ray_setup: counted globally there too
        }
      }
      if (slot < rt.slot_capacity)
      {
        hk = packHitKey(slot, vi, ray, ray_shift);
        if (hit_mask)
        {
          atomicOr(&hit_mask[size_t(slot) * mask_words + (vi >> 5)], 1u << (vi & 31));
        }
      }
    }
    if (!bucket_hits || hk != kHitInvalid)
    {
      hit_keys[pos] = hk;
    }
  };
  // Step 3: scatter, rays visited by descending extent (see RayOrder).
  __shared__ RayOrder order;
  const uint32_t n_local = last - first;
  buildRayOrder(order, n_local, [&](uint32_t, uint32_t idx) {
    const RayWalk *w = walks + first + idx;
    const int total[3] = { w->total[0], w->total[1], w->total[2] };
    return rayExtentBin(mc, w->flags, total);
  });
  for (uint32_t idx = threadIdx.x; idx < n_local; idx += blockDim.x)
  {
    const uint32_t ray = first + order.perm[idx];
    const RayWalk rw = walks[ray];
    emitSample(ray, rw);  // (the ray's record is loaded once for both its sample key and its segments)
    const RayFix rf = rayFix(mc, rw);
    forEachBinSegment<kPlain>(mc, rw, rf, ray, [&](uint64_t key, const Segment &sg) {
      const uint32_t e = ltabFind(tab, key, tab_mask);
      uint32_t pos;
      if (e < kLtabSize)
      {
        pos = atomicAdd(&tab.cursor[e], 1u);
      }
      else
      {
        const uint32_t h = regionFind(rt, key);  // table overflow: straight to the global cursor
        if (h == 0xffffffffu)
        {
          return;  // (failed insert of a speculated batch, see above)
        }
        pos = bs.seg_offset[h] + atomicAdd(&bs.seg_cursor[h], 1u);
      }
      if (pos < segment_capacity)
      {
        segments[pos] = sg;
      }
    });
  }
}

/// The number of rays of [rays, rays + n) the map's ray filter passes: what an integrate call reports for its own
/// rays when they only run later, with a collected batch (one workgroup; the count goes straight to pinned memory).
/// With a ray-filter chain set (n_stages > 0) the verdict is the chain's (ray_filter_chain.h), as k_ray_filter will
/// give it when the batch runs.
__global__ void __launch_bounds__(1024)
  k_count_passed(MapConst mc, const double *__restrict__ rays, uint32_t n_rays, unsigned ray_flags,
                 uint32_t *__restrict__ host_count, const ohmhip_ray_filter_stage *__restrict__ stages, uint32_t n_stages)
{
  __shared__ uint32_t s_ok;
  if (threadIdx.x == 0)
  {
    s_ok = 0;
  }
  __syncthreads();
  uint32_t my_ok = 0;
  for (uint32_t ray = threadIdx.x; ray < n_rays; ray += blockDim.x)
  {
    RayWalk rw;
    double start[3], end[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      start[a] = rays[size_t(ray) * 6 + a];
      end[a] = rays[size_t(ray) * 6 + 3 + a];
    }
    if (n_stages)
    {
      unsigned filter_flags;
      my_ok += rayFilterChain(stages, n_stages, start, end, &filter_flags) ? 1u : 0u;
      continue;
    }
    setupRay(mc, start, end, ray_flags, rw, ray);
    my_ok += (rw.flags & kRwPassed) ? 1u : 0u;
  }
  atomicAdd(&s_ok, my_ok);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    *host_count = s_ok;
  }
}

/// Rewrite only the sample (hit) keys of a batch (used when the NDT / TSDF key buffer had to be re-allocated).
__global__ void __launch_bounds__(256)
  k_rekey_samples(MapConst mc, RegionTable rt, const RayWalk *__restrict__ walks, uint32_t n_rays,
                  unsigned long long *__restrict__ hit_keys, int ray_shift)
{
  const uint32_t ray = blockIdx.x * blockDim.x + threadIdx.x;
  if (ray >= n_rays)
  {
    return;
  }
  const RayWalk rw = walks[ray];
  unsigned long long hk = kHitInvalid;
  if ((rw.flags & kRwValid) && (rw.flags & kRwApplySample))
  {
    uint64_t key;
    uint32_t vi;
    sampleVoxel(mc, rw, key, vi);
    const uint32_t h = regionFind(rt, key);
    const uint32_t slot = (h != 0xffffffffu) ? rt.vals[h] : kSlotUnassigned;
    if (slot < rt.slot_capacity)
    {
      hk = packHitKey(slot, vi, ray, ray_shift);
    }
  }
  hit_keys[ray] = hk;
}
}  // namespace ohmhip

#endif  // OHMHIP_RAY_FRONT_KERNELS_H
