// compare_kernels.h -- ohm::compare::compareVoxels (ohm/CompareMaps.cpp:58-75, 193-386) between two resident maps, read
// only: a member-by-member comparison of one layer over the regions of the reference map, in a fixed order.
//
//   k_compare_count   1 workgroup / chunk   every member of every voxel judged; one failed count per wave (for the scan)
//                                           and one CompareRecord per chunk
//   (exclusive scan of the per-wave counts, 64 bit: rocPRIM, compare_impl.h -- only when a mismatch list is wanted)
//   k_compare_emit    1 workgroup / chunk   the same test; a failing voxel writes its key at offset of its wave + rank
//                                           among the failing voxels before it; waves without a failure leave at once
//   k_compare_finish  1 workgroup           the records reduced into ohmhip_compare_result; the first failure resolved
//
// The rules are those of include/ohmhip.h ("MAP COMPARE", K1 - K7); tests/compare_ref.py is the restatement on the CPU.
//
// Shape.  The host lists the work (compare_impl.h): the regions of the reference map the evaluated map also holds, in
// (rz, ry, rx) order, tile by tile, each tile cut into chunks of kCloudChunkVoxels consecutive voxels of the region's
// MapChunk block, with the two layer blocks' addresses -- pool slot or pinned store record -- resolved once per tile; a
// null address reads as the layer's clear word.  A chunk is one workgroup of four waves, wave w owning the chunk's
// voxels [w * 1024, (w + 1) * 1024): the per-wave counts are in voxel order and their exclusive scan is every wave's
// first slot in the mismatch list.  Loads: a layer of 4-byte voxels takes four voxels a lane with one 16-byte load per
// side where both blocks allow it (64-voxel runs of dwords otherwise); 8-byte and 24-byte voxels are loaded whole per
// lane, in 8-byte pieces where both blocks are 8-byte aligned.  Counting is __popcll(__ballot(fail)); the per-member
// maxima are kept per lane and folded across the wave once, at the end.  No atomics anywhere: every output is written
// by exactly one thread with a plain vector store, so two calls return identical bytes.
#ifndef OHMHIP_COMPARE_KERNELS_H
#define OHMHIP_COMPARE_KERNELS_H

#include "cloud_kernels.h"

namespace ohmhip
{
constexpr uint32_t kCompareMaxMembers = OHMHIP_CMP_MAX_MEMBERS;
constexpr uint32_t kCompareNoFailure = 0xffffffffu;

/// Consecutive voxels of one tile in both maps.  Block addresses are those of the chunk's FIRST voxel.
struct CompareChunk
{
  const void *eval;                 ///< evaluated map's block; null: the tile holds no data there, reads cleared
  const void *ref;                  ///< reference map's block; null likewise
  unsigned long long voxels_before; ///< voxels of compared regions ahead of this chunk in the order
  uint32_t first;                   ///< index of the first voxel in the REGION's block
  uint32_t count;                   ///< voxels, <= kCloudChunkVoxels
  int16_t region[3];                ///< the caller's region key
  uint16_t wide;                    ///< both blocks allow the wide loads (16-byte aligned for 4-byte voxels, else 8)
  uint32_t pad_[2];
};
static_assert(sizeof(CompareChunk) == 48, "work list records are three 16-byte words");

/// What k_compare_count leaves per chunk.
struct CompareRecord
{
  uint32_t failed;      ///< voxels with a failing member
  uint32_t first_fail;  ///< offset in the chunk of the first of them, kCompareNoFailure without one
  uint32_t first_mask;  ///< its mask of failing members
  uint32_t pad_;
  uint32_t member_failed[kCompareMaxMembers];  ///< voxels whose member i failed
  uint32_t member_max[kCompareMaxMembers];     ///< largest hi - lo of member i (a float's bits; ordered as unsigned)
};
static_assert(sizeof(CompareRecord) == 64, "one record is four 16-byte words");

struct CompareArgs
{
  const CompareChunk *chunks;
  CompareRecord *records;
  uint32_t *counts;                   ///< [chunks * kCloudWaves (+ 1: a zero)]
  const unsigned long long *offsets;  ///< exclusive scan of counts (emit)
  unsigned long long capacity;        ///< keys the mismatch list holds (emit)
  GpuKeyOut *out_keys;
  uint32_t words;       ///< members = dwords per voxel: 1, 2 or 6
  uint32_t float_mask;  ///< bit i: member i is an f32 (else u32)
  uint32_t tol_mask;    ///< bit i: member i is judged with a tolerance
  uint32_t clear_word;
  uint32_t eps[kCompareMaxMembers];  ///< the tolerance's low 4 bytes, read as the member's type
  int kdim[3];                       ///< region voxel dimensions
};

/// compareDatum<T> (CompareMaps.cpp:58-75) for T = float or uint32_t, or the byte comparison (:313-318) without a
/// tolerance.  diff: hi - lo as an unsigned-ordered word -- a float difference's bits when it is > 0 (an inf among them),
/// 0 for a zero of either sign and for a NaN (a NaN operand, or inf against itself).
__device__ inline bool compareMember(uint32_t val, uint32_t ref, bool is_float, bool has_tol, uint32_t eps, uint32_t &diff)
{
  bool within;
  if (is_float)
  {
    const float v = __uint_as_float(val), r = __uint_as_float(ref);
    const bool swap = r > v;
    const float hi = swap ? r : v;
    const float lo = swap ? v : r;
    const float d = hi - lo;
    within = hi == lo || d <= __uint_as_float(eps);
    diff = (d > 0.0f) ? __float_as_uint(d) : 0u;
  }
  else
  {
    const bool swap = ref > val;
    const uint32_t hi = swap ? ref : val;
    const uint32_t lo = swap ? val : ref;
    const uint32_t d = hi - lo;
    within = hi == lo || d <= eps;
    diff = d;
  }
  return has_tol ? within : val == ref;
}

/// One voxel: the mask of failing members; maxima[] raised to this voxel's differences.
template <int W>
__device__ inline uint32_t compareVoxelWords(const CompareArgs &a, const uint32_t (&e)[W], const uint32_t (&r)[W],
                                             uint32_t (&maxima)[W])
{
  uint32_t mask = 0;
#pragma unroll
  for (int i = 0; i < W; ++i)
  {
    uint32_t diff;
    const bool pass = compareMember(e[i], r[i], (a.float_mask >> i) & 1u, (a.tol_mask >> i) & 1u, a.eps[i], diff);
    mask |= pass ? 0u : (1u << i);
    maxima[i] = max(maxima[i], diff);
  }
  return mask;
}

/// Voxel i of a block as W dwords; a null block reads the clear word.
template <int W>
__device__ inline void compareLoad(const void *block, uint32_t i, bool wide, uint32_t clear_word, uint32_t (&w)[W])
{
  if (!block)
  {
#pragma unroll
    for (int k = 0; k < W; ++k)
    {
      w[k] = clear_word;
    }
    return;
  }
  if (W > 1 && wide)
  {
    const uint2 *p = static_cast<const uint2 *>(block) + size_t(i) * (W / 2);
#pragma unroll
    for (int k = 0; k < W / 2; ++k)
    {
      const uint2 q = p[k];
      w[2 * k] = q.x;
      w[2 * k + 1] = q.y;
    }
    return;
  }
  const uint32_t *p = static_cast<const uint32_t *>(block) + size_t(i) * W;
#pragma unroll
  for (int k = 0; k < W; ++k)
  {
    w[k] = p[k];
  }
}

/// What a wave found in its share of a chunk.
template <int W>
struct CompareWaveSum
{
  uint32_t failed;
  uint32_t first;  ///< (offset in the chunk << 8) | mask of the first failing voxel; kCompareNoFailure: none
  uint32_t member_failed[W];
  uint32_t maxima[W];
};

template <int W>
__device__ inline void compareTally(uint32_t mask, uint32_t index, CompareWaveSum<W> &sum, uint32_t &lane_first)
{
  const unsigned long long any = __ballot(mask != 0u);
  if (any == 0ull)
  {
    return;  // (wave uniform)
  }
  sum.failed += uint32_t(__popcll(any));
#pragma unroll
  for (int i = 0; i < W; ++i)
  {
    sum.member_failed[i] += uint32_t(__popcll(__ballot(((mask >> i) & 1u) != 0u)));
  }
  if (mask != 0u)
  {
    lane_first = min(lane_first, (index << 8) | mask);
  }
}

/// Wave `wave` of the workgroup over its share of chunk c; every lane returns the wave's sums.
template <int W>
__device__ inline CompareWaveSum<W> compareWalkWave(const CompareArgs &a, const CompareChunk &c, uint32_t wave)
{
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t at = wave * kCloudWaveVoxels;
  const uint32_t end = min(at + kCloudWaveVoxels, c.count);
  CompareWaveSum<W> sum{};
  uint32_t lane_first = kCompareNoFailure;
  uint32_t maxima[W] = {};
  if (W == 1 && c.wide)
  {
    const uint32_t cw = a.clear_word;
    for (; at + 256u <= end; at += 256u)
    {
      const uint32_t i4 = (at >> 2) + lane;
      const uint4 e = c.eval ? static_cast<const uint4 *>(c.eval)[i4] : make_uint4(cw, cw, cw, cw);
      const uint4 r = c.ref ? static_cast<const uint4 *>(c.ref)[i4] : make_uint4(cw, cw, cw, cw);
      const uint32_t ev[4] = { e.x, e.y, e.z, e.w };
      const uint32_t rv[4] = { r.x, r.y, r.z, r.w };
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k)
      {
        uint32_t e1[W], r1[W];
        e1[0] = ev[k];
        r1[0] = rv[k];
        const uint32_t mask = compareVoxelWords<W>(a, e1, r1, maxima);
        compareTally<W>(mask, at + 4u * lane + k, sum, lane_first);
      }
    }
  }
  for (; at < end; at += 64u)
  {
    const uint32_t i = at + lane;
    uint32_t mask = 0;
    if (i < end)
    {
      uint32_t e[W], r[W];
      compareLoad<W>(c.eval, i, c.wide != 0, a.clear_word, e);
      compareLoad<W>(c.ref, i, c.wide != 0, a.clear_word, r);
      mask = compareVoxelWords<W>(a, e, r, maxima);
    }
    compareTally<W>(mask, i, sum, lane_first);
  }
  // fold the lanes: the smallest (index, mask) word, the largest difference per member
  for (uint32_t step = 32u; step > 0u; step >>= 1)
  {
    lane_first = min(lane_first, uint32_t(__shfl_xor(int(lane_first), int(step))));
#pragma unroll
    for (int i = 0; i < W; ++i)
    {
      maxima[i] = max(maxima[i], uint32_t(__shfl_xor(int(maxima[i]), int(step))));
    }
  }
  sum.first = lane_first;
#pragma unroll
  for (int i = 0; i < W; ++i)
  {
    sum.maxima[i] = maxima[i];
  }
  return sum;
}

template <int W>
__device__ inline void compareCountChunk(const CompareArgs &a, uint32_t (&lds)[kCloudWaves][2 + 2 * kCompareMaxMembers])
{
  const CompareChunk c = a.chunks[blockIdx.x];
  const uint32_t wave = threadIdx.x >> 6;
  const CompareWaveSum<W> sum = compareWalkWave<W>(a, c, wave);
  if ((threadIdx.x & 63u) == 0u)
  {
    a.counts[size_t(blockIdx.x) * kCloudWaves + wave] = sum.failed;
    lds[wave][0] = sum.failed;
    lds[wave][1] = sum.first;
#pragma unroll
    for (int i = 0; i < W; ++i)
    {
      lds[wave][2 + i] = sum.member_failed[i];
      lds[wave][2 + kCompareMaxMembers + i] = sum.maxima[i];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0u)
  {
    CompareRecord rec{};
    uint32_t first = kCompareNoFailure;
    for (uint32_t w = 0; w < kCloudWaves; ++w)
    {
      rec.failed += lds[w][0];
      first = min(first, lds[w][1]);
#pragma unroll
      for (int i = 0; i < W; ++i)
      {
        rec.member_failed[i] += lds[w][2 + i];
        rec.member_max[i] = max(rec.member_max[i], lds[w][2 + kCompareMaxMembers + i]);
      }
    }
    rec.first_fail = (first == kCompareNoFailure) ? kCompareNoFailure : (first >> 8);
    rec.first_mask = (first == kCompareNoFailure) ? 0u : (first & 0xffu);
    a.records[blockIdx.x] = rec;
  }
}

__global__ void __launch_bounds__(256) k_compare_count(CompareArgs a)
{
  __shared__ uint32_t lds[kCloudWaves][2 + 2 * kCompareMaxMembers];
  switch (a.words)
  {
  case 1u:
    compareCountChunk<1>(a, lds);
    break;
  case 2u:
    compareCountChunk<2>(a, lds);
    break;
  default:
    compareCountChunk<6>(a, lds);
    break;
  }
}

/// The caller's key of voxel `index` of region block `region`, byte 9 the mask of failing members.
__device__ inline GpuKeyOut compareKey(const int kdim[3], const int16_t region[3], uint32_t index, uint32_t mask)
{
  const uint32_t dx = uint32_t(kdim[0]), dy = uint32_t(kdim[1]);
  const uint32_t row = index / dx;
  const uint32_t lz = row / dy;
  GpuKeyOut k;
  k.region[0] = region[0];
  k.region[1] = region[1];
  k.region[2] = region[2];
  k.voxel[0] = uint8_t(index - row * dx);
  k.voxel[1] = uint8_t(row - lz * dy);
  k.voxel[2] = uint8_t(lz);
  k.voxel[3] = uint8_t(mask);
  return k;
}

template <int W>
__device__ inline void compareEmitWave(const CompareArgs &a, const CompareChunk &c, uint32_t wave, unsigned long long base)
{
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long below = cloudLanesBelow();
  const uint32_t end = min((wave + 1u) * kCloudWaveVoxels, c.count);
  uint32_t maxima[W] = {};
  unsigned long long slot = base;
  for (uint32_t at = wave * kCloudWaveVoxels; at < end && slot < a.capacity; at += 64u)
  {
    const uint32_t i = at + lane;
    uint32_t mask = 0;
    if (i < end)
    {
      uint32_t e[W], r[W];
      compareLoad<W>(c.eval, i, c.wide != 0, a.clear_word, e);
      compareLoad<W>(c.ref, i, c.wide != 0, a.clear_word, r);
      mask = compareVoxelWords<W>(a, e, r, maxima);
    }
    const unsigned long long b = __ballot(mask != 0u);
    const unsigned long long mine = slot + uint32_t(__popcll(b & below));
    if (mask != 0u && mine < a.capacity)
    {
      a.out_keys[mine] = compareKey(a.kdim, c.region, c.first + i, mask);
    }
    slot += uint32_t(__popcll(b));
  }
}

__global__ void __launch_bounds__(256) k_compare_emit(CompareArgs a)
{
  const uint32_t wave = threadIdx.x >> 6;
  const size_t part = size_t(blockIdx.x) * kCloudWaves + wave;
  const unsigned long long base = a.offsets[part];
  if (a.counts[part] == 0u || base >= a.capacity)
  {
    return;  // no failure in this wave's share, or all of them lie beyond the list
  }
  const CompareChunk c = a.chunks[blockIdx.x];
  switch (a.words)
  {
  case 1u:
    compareEmitWave<1>(a, c, wave, base);
    break;
  case 2u:
    compareEmitWave<2>(a, c, wave, base);
    break;
  default:
    compareEmitWave<6>(a, c, wave, base);
    break;
  }
}

/// What the host knows before the kernels run, and where the result goes.
struct CompareFinishArgs
{
  const CompareChunk *chunks;
  const CompareRecord *records;
  ohmhip_compare_result *result;
  GpuKeyOut *out_keys;   ///< the mismatch list (stop-at-first: its one entry is written here)
  int16_t *out_missing;  ///< the missing list (stop-at-first only; otherwise the host has written it)
  unsigned long long mismatch_capacity, missing_capacity;
  unsigned long long compared_voxels;  ///< voxels of all chunks
  unsigned long long missing_voxels;   ///< voxels of the regions the evaluated map lacks
  unsigned long long regions_compared, regions_missing, keys_absent;
  uint32_t n_chunks;
  uint32_t first_missing_chunk;  ///< chunks ahead of the first missing region (n_chunks when it follows them all)
  uint32_t member_count;
  int layout_match;
  int keep_going;  ///< OHMHIP_CMP_CONTINUE
  int kdim[3];
  int16_t first_missing[3];
};

/// One workgroup.  Sums in 64 bit; the first failing chunk is the smallest index with a failure.
__global__ void __launch_bounds__(256) k_compare_finish(CompareFinishArgs a)
{
  __shared__ unsigned long long s_sum[256][1 + kCompareMaxMembers];
  __shared__ uint32_t s_word[256][1 + kCompareMaxMembers];
  unsigned long long sums[1 + kCompareMaxMembers] = {};
  uint32_t maxima[kCompareMaxMembers] = {};
  uint32_t first_chunk = a.n_chunks;
  for (uint32_t i = threadIdx.x; i < a.n_chunks; i += 256u)
  {
    const CompareRecord rec = a.records[i];
    sums[0] += rec.failed;
    first_chunk = (rec.failed != 0u) ? min(first_chunk, i) : first_chunk;
#pragma unroll
    for (uint32_t k = 0; k < kCompareMaxMembers; ++k)
    {
      sums[1 + k] += rec.member_failed[k];
      maxima[k] = max(maxima[k], rec.member_max[k]);
    }
  }
  s_word[threadIdx.x][0] = first_chunk;
  s_sum[threadIdx.x][0] = sums[0];
  for (uint32_t k = 0; k < kCompareMaxMembers; ++k)
  {
    s_sum[threadIdx.x][1 + k] = sums[1 + k];
    s_word[threadIdx.x][1 + k] = maxima[k];
  }
  __syncthreads();
  if (threadIdx.x != 0u)
  {
    return;
  }
  for (uint32_t t = 1; t < 256u; ++t)
  {
    first_chunk = min(first_chunk, s_word[t][0]);
    sums[0] += s_sum[t][0];
    for (uint32_t k = 0; k < kCompareMaxMembers; ++k)
    {
      sums[1 + k] += s_sum[t][1 + k];
      maxima[k] = max(maxima[k], s_word[t][1 + k]);
    }
  }
  ohmhip_compare_result res{};
  res.layout_match = a.layout_match;
  res.member_count = a.member_count;
  res.regions_compared = a.regions_compared;
  res.regions_missing = a.regions_missing;
  res.keys_absent = a.keys_absent;
  if (a.keep_going)
  {
    res.voxels_failed = sums[0] + a.missing_voxels;
    res.voxels_passed = a.compared_voxels - sums[0];
    res.mismatch_count = sums[0];
    res.missing_count = a.regions_missing;
    for (uint32_t k = 0; k < kCompareMaxMembers; ++k)
    {
      res.member_failed[k] = sums[1 + k];
      res.member_max_diff[k] = maxima[k];
    }
  }
  else if (first_chunk < a.first_missing_chunk)
  {
    // K5: the walk ends at a value mismatch
    const CompareChunk c = a.chunks[first_chunk];
    const CompareRecord rec = a.records[first_chunk];
    res.voxels_failed = 1;
    res.voxels_passed = c.voxels_before + rec.first_fail;
    res.mismatch_count = 1;
    for (uint32_t k = 0; k < kCompareMaxMembers; ++k)
    {
      res.member_failed[k] = (rec.first_mask >> k) & 1u;
    }
    if (a.mismatch_capacity > 0ull)
    {
      a.out_keys[0] = compareKey(a.kdim, c.region, c.first + rec.first_fail, rec.first_mask);
    }
  }
  else if (a.regions_missing > 0ull)
  {
    // ... or at the first voxel of a region the evaluated map lacks
    res.voxels_failed = 1;
    res.voxels_passed = (a.first_missing_chunk < a.n_chunks) ? a.chunks[a.first_missing_chunk].voxels_before : a.compared_voxels;
    res.missing_count = 1;
    if (a.missing_capacity > 0ull)
    {
      a.out_missing[0] = a.first_missing[0];
      a.out_missing[1] = a.first_missing[1];
      a.out_missing[2] = a.first_missing[2];
    }
  }
  else
  {
    res.voxels_passed = a.compared_voxels;
  }
  *a.result = res;
}
}  // namespace ohmhip

#endif  // OHMHIP_COMPARE_KERNELS_H
