// walk_kernel.h -- the walk stage of the occupancy ray-integration path (gfx950).
//
//   k_region_walk       persistent, 1 workgroup / CU   THE hot kernel: chunks from a device-wide cursor; region
//                                          miss-count tile in LDS, 1 lane / segment resumes the fp64 walk inside the
//                                          region; LDS atomics; single-chunk regions applied straight from LDS
//   k_flagged_events    grid-stride        order the deferred misses the walk could not resolve in LDS
//
// k_region_walk is register bound and fragile.  Cross-compiled for gfx950 at -O3, its six instantiations sit at
// 128 VGPRs and spill (VGPR spills / scratch bytes; <kSpecial, kTrace, geometry>):
//   <0,0,Full> 11 / 48   <0,0,Half> 8 / 32   <1,0,Full> 11 / 48   <1,0,Half> 16 / 48
//   <0,1,Full> 17 / 48   <0,1,Half> 16 / 48
// (36 / 128, 40 / 144, 37 / 128, 41 / 144, 38 / 128, 51 / 144 before round 16, whose tile initialisation for a region
// that fills the tile is a function -- initFullTile -- and whose general form no longer starts at a mask word the
// compiler knows to be the thread's own: the lane-dependent addresses and predicates it used to hoist out of the chunk
// loop, spill, and reload in every chunk are gone; profiles/r16_notes.md.  37 / 148, 43 / 148, 38 / 152, 45 / 152,
// 45 / 156, 56 / 156 before round 14.)
// Moving the prologue's count-tile initialisation loop, unchanged, into a __device__ inline function took the production
// <0,0,Full> instantiation from 37 to 90 spilled VGPRs.  So the body of the kernel is left as one piece of text, and ANY
// edit to it, or to a function it inlines, is checked with scripts/kernel_fingerprint.py against the parent commit
// before it goes near a GPU: the figures above must not get worse.  Code that is new to the kernel and runs once per
// chunk goes into a __noinline__ function (scanOrderBins, applyFullTile, flushFullTile, initFullTile below): written
// into the body, the three of round 14 gave 98 spilled VGPRs, the ordering's scan alone 51 (profiles/r14_notes.md).
#ifndef OHMHIP_WALK_KERNEL_H
#define OHMHIP_WALK_KERNEL_H

#include "batch_scratch.h"
#include "occupancy_math.h"
#include "region_table.h"
#include "walk_device.h"

namespace ohmhip
{
// ---------------------------------------------------------------------------------------------------------------------
// k_region_walk: the hot kernel.
//
// One workgroup (16 waves) per chunk of <= kChunkSegments ray-region segments of ONE region.  The region's miss-count
// tile lives in LDS: one u16 per voxel, 15 bits of count and the top bit holding the voxel's mask flag ("also receives
// samples"), so ONE returning LDS atomic per visit both counts the miss and fetches the flag.  Every lane resumes one
// ray's fp64 walk at the step that enters the region and visits the segment's voxels.  Idle lanes are refilled in
// batches from a workgroup-wide LDS cursor so waves stay mostly full although segments differ in length.
//
// A miss on a masked voxel must be ordered against that voxel's samples.  Such visits are appended to a per-wave LDS
// queue (no atomics: the queue cursor is wave-uniform) and resolved in bursts: against the region's sorted sample keys
// staged in LDS when they fit, otherwise through a global event list (k_flagged_events).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kWalkThreads = 1024;
constexpr int kWalkWaves = kWalkThreads / 64;
constexpr int kQueueCap = 128;     ///< deferred events per wave (8 B each)
#ifndef OHMHIP_LDS_HITS
#define OHMHIP_LDS_HITS 6144
#endif
constexpr int kLdsHits = OHMHIP_LDS_HITS;     ///< a region's sample list is staged in LDS when it has at most this many samples
constexpr uint32_t kIndexShift = 5;  ///< staged samples are indexed by voxel index >> kIndexShift ...
constexpr uint32_t kIndexBuckets = (1u << kHitVoxelBits) >> kIndexShift;  ///< ... in this many buckets (+ 1 end entry)
constexpr int kRefillMinIdle = 20; ///< refill a wave once this many lanes are idle
constexpr uint32_t kTileFlag = 0x8000u;       ///< mask flag inside a u16 tile entry
constexpr uint32_t kTileCountMask = 0x7fffu;  ///< count bits of a u16 tile entry (a chunk adds <= kMaxChunkSegments)
#ifndef OHMHIP_MAX_CHUNK_SEGMENTS
#define OHMHIP_MAX_CHUNK_SEGMENTS 8192
#endif
constexpr uint32_t kMaxChunkSegments = OHMHIP_MAX_CHUNK_SEGMENTS;  ///< bounded by the 15-bit counters and by the LDS order array
constexpr uint32_t kTraceChunks = 4096;  ///< debug trace: records kept per launch
constexpr uint32_t kTraceWords = 32;     ///< debug trace: u64 words per record
constexpr uint32_t kLengthClasses = 128;      ///< segment length histogram bins (lengths above the last bin share it)
/// Copies of every length class's counter, chosen by lane index: the segments of a chunk fall into a few dozen classes,
/// and the lanes of a wave that add to ONE counter are served one after the other.
constexpr uint32_t kOrderCopies = 8;
constexpr uint32_t kOrderBins = kLengthClasses * kOrderCopies;

/// Physical position of the count tile's logical word `w` (two voxels per word, voxel order).  A word's LDS bank is its
/// index modulo 32, which in voxel order is (x / 2, y & 1): lanes whose rays advance in step through a region -- a
/// lidar's vertical fan of beams has the same x and y in every lane -- would all hit one or two banks.  The tile is
/// therefore stored with the bank bits XOR-ed with the y / z bits of the index (a permutation inside every 32-word row).
__device__ inline uint32_t tileWord(uint32_t w)
{
  return w ^ (((w >> 5) ^ (w >> 10)) & 31u);
}

/// Byte address of the tile word holding the u16 entry at byte offset `va` (= 2 x voxel index).
__device__ inline uint32_t tileAddress(uint32_t va)
{
  return (va & ~3u) ^ ((((va >> 5) ^ (va >> 10)) & (31u << 2)));
}

/// Resolve one deferred miss event: find the first sample of the same voxel with a larger ray index; the miss counts
/// towards the interval before that sample, or towards the voxel's trailing count if there is none.
__device__ inline void resolveFlaggedMiss(unsigned long long key, const BatchScratch &bs,
                                          const unsigned long long *__restrict__ sorted_hits,
                                          uint32_t *__restrict__ miss_counts, uint32_t *__restrict__ interval_counts,
                                          int region_voxels)
{
  const uint32_t slot = hitSlot(key);
  const uint32_t vi = hitVoxel(key);
  const uint32_t he = bs.info->n_hits;
  // Start at the voxel's first sample and step over the (few) samples with a smaller ray index.
  uint32_t lo = bs.voxel_first_hit[size_t(slot) * size_t(region_voxels) + vi];
  while (lo < he && hitGroup(sorted_hits[lo]) == hitGroup(key) && sorted_hits[lo] < key)
  {
    ++lo;
  }
  if (lo < he && hitGroup(sorted_hits[lo]) == hitGroup(key))
  {
    // The visit was counted in the voxel's miss count by the walk; move it to the interval before that sample.
    // (Integer add / sub commute, so the transient order against the tile flush does not matter.)
    atomicAdd(&interval_counts[lo], 1u);
    atomicSub(&miss_counts[size_t(slot) * size_t(region_voxels) + vi], 1u);
  }
}

/// Drain one wave's deferred-miss queue of (voxel, ray) pairs.  Preferred: order each miss against the region's samples
/// in LDS (binary search over the staged sorted keys, LDS atomics on the interval / trailing counters).  Otherwise
/// append the events to the global list in one coalesced burst (resolved by k_flagged_events, or sorted and replayed
/// for NDT / TSDF).
__device__ inline void flushQueue(const uint2 *queue, uint32_t qcount, unsigned lane, unsigned long long slot_bits,
                                  int ray_shift, bool lds_resolve, const unsigned long long *l_hits,
                                  const uint16_t *l_index, uint32_t n_region_hits, uint32_t *l_intervals,
                                  uint32_t *l_counts,
                                  unsigned long long *__restrict__ events, uint32_t event_capacity,
                                  uint32_t *__restrict__ event_count, int defer_all, const BatchScratch &bs,
                                  const unsigned long long *__restrict__ sorted_hits,
                                  uint32_t *__restrict__ miss_counts, uint32_t *__restrict__ interval_counts,
                                  int region_voxels)
{
  if (lds_resolve)
  {
    for (uint32_t q = lane; q < qcount; q += 64)
    {
      const uint2 e = queue[q];
      const unsigned long long ev =
        slot_bits | ((unsigned long long)e.x << kHitRayBits) | ((unsigned long long)e.y << ray_shift);
      // First staged sample with key > ev: the bucket index narrows the search to the samples of the event's 32
      // voxels (a handful), a binary search finishes it.
      uint32_t lo = l_index[e.x >> kIndexShift], hi = l_index[(e.x >> kIndexShift) + 1u];
      while (lo < hi)
      {
        const uint32_t mid = (lo + hi) >> 1;
        if (l_hits[mid] > ev)
        {
          hi = mid;
        }
        else
        {
          lo = mid + 1;
        }
      }
      // (lo may be the first sample of the next bucket: the voxel test below rejects it)
      if (lo < n_region_hits && hitGroup(l_hits[lo]) == hitGroup(ev))
      {
        // Belongs before a later sample of the voxel: move it from the voxel's count to that sample's interval.
        atomicAdd(&l_intervals[lo >> 1], 1u << ((lo & 1u) * 16u));
        atomicSub(&l_counts[tileWord(e.x >> 1)], 1u << ((e.x & 1u) * 16u));
      }
    }
    return;
  }
  uint32_t gbase = 0;
  if (lane == 0)
  {
    gbase = atomicAdd(event_count, qcount);
  }
  gbase = __shfl(gbase, 0);
  for (uint32_t q = lane; q < qcount; q += 64)
  {
    const uint2 e = queue[q];
    const unsigned long long ev =
      slot_bits | ((unsigned long long)e.x << kHitRayBits) | ((unsigned long long)e.y << ray_shift);
    if (gbase + q < event_capacity)
    {
      events[gbase + q] = ev;
    }
    else if (!defer_all)
    {
      resolveFlaggedMiss(ev, bs, sorted_hits, miss_counts, interval_counts, region_voxels);
    }
  }
}

// Explicit lane-mask selects for the walk step (see k_region_walk): `mask` is a wave-wide 64-bit lane mask in SGPRs.
constexpr int kFcmpOlt = 4;   ///< llvm::CmpInst::FCMP_OLT
constexpr int kIcmpSlt = 40;  ///< llvm::CmpInst::ICMP_SLT

__device__ inline int selectI(unsigned long long mask, int if_set, int if_clear)
{
  int r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(mask));
  return r;
}

__device__ inline double selectD(unsigned long long mask, double if_set, double if_clear)
{
  const int lo = selectI(mask, __double2loint(if_set), __double2loint(if_clear));
  const int hi = selectI(mask, __double2hiint(if_set), __double2hiint(if_clear));
  return __hiloint2double(hi, lo);
}

/// value + (lane's mask bit): one add-with-carry-in.
__device__ inline int addMask(int value, unsigned long long mask)
{
  asm("v_addc_co_u32_e64 %0, vcc, 0, %0, %1" : "+v"(value) : "s"(mask) : "vcc");
  return value;
}

constexpr int kIcmpEq = 32;   ///< llvm::CmpInst::ICMP_EQ
constexpr int kIcmpUlt = 36;  ///< llvm::CmpInst::ICMP_ULT

/// mask ? if_set : 0
__device__ inline uint32_t selectOrZero(unsigned long long mask, uint32_t if_set)
{
  uint32_t r;
  asm("v_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(if_set), "s"(mask));
  return r;
}

__device__ inline uint32_t umin3(uint32_t a, uint32_t b, uint32_t c)
{
  uint32_t r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

__device__ inline uint32_t umed3(uint32_t a, uint32_t b, uint32_t c)
{
  uint32_t r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

/// a + b, saturating at 2^32 - 1 (the predictor's candidates never wrap into small values).
__device__ inline uint32_t addSat(uint32_t a, uint32_t b)
{
  uint32_t r;
  asm("v_add_u32_e64 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

/// The same with a wave-uniform second operand (kept in an SGPR).
__device__ inline uint32_t addSatUniform(uint32_t a, uint32_t b)
{
  uint32_t r;
  asm("v_add_u32_e64 %0, %1, %2 clamp" : "=v"(r) : "v"(a), "s"(b));
  return r;
}

/// Returning LDS add on the count tile.  Issued as inline assembly so that (a) the tile's address needs no base add (it
/// sits at LDS offset 0: the kernel has no static LDS, checked by the parity tests on every run) and (b) the wait for
/// the returned value is placed by hand, after the walk step (waitTile).
__device__ inline uint32_t tileAdd(uint32_t byte_address, uint32_t value)
{
  uint32_t old;
  asm volatile("ds_add_rtn_u32 %0, %1, %2" : "=v"(old) : "v"(byte_address), "v"(value) : "memory");
  return old;
}

/// 1 << (shift & 31): the hardware shift only reads the low five bits of its shift operand.
__device__ inline uint32_t shiftOne(uint32_t shift)
{
  uint32_t r;
  asm("v_lshlrev_b32_e64 %0, %1, 1" : "=v"(r) : "v"(shift));
  return r;
}

__device__ inline uint32_t waitTile(uint32_t old)
{
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(old) : : "memory");
  return old;
}

/// Kernel parameters of k_region_walk (one struct keeps the template instantiations readable).
struct WalkArgs
{
  MapConst mc;
  BatchScratch bs;
  const Chunk *chunks;
  const Segment *segments;
  const RayWalk *walks;
  const uint64_t *slot_keys;  ///< region key per slot (exact decisions need the region's coordinates)
  const unsigned long long *sorted_hits;
  const uint32_t *hit_mask;
  uint32_t *miss_counts;
  uint32_t *interval_counts;
  unsigned long long *events;
  uint32_t event_capacity;
  uint32_t *event_count;
  int refill_min_idle;
  unsigned dbg;
  int ray_shift;
  int defer_all;     ///< NDT / TSDF: every visit to a masked voxel becomes an event; masked voxels are not counted
  float *occupancy;  ///< non-null: single-chunk regions are applied straight from LDS
  unsigned ray_flags;
  unsigned long long *dbg_counters;
  float *tsdf;       ///< non-null (TSDF mode): single-chunk regions are applied straight from LDS
  uint32_t *chunk_cursor;  ///< device-wide next-chunk cursor (zeroed before the launch)
  uint32_t n_chunks;
  /// NDT / TSDF: this launch repeats a walk whose event list overflowed.  Regions held by a single chunk had their plain
  /// counts applied to the layers by the first launch already: the repeat only regenerates their events.
  int rewalk;
  /// TSDF with weight drop-off: a free-space visit changes the weight by a value that depends on the voxel and the
  /// ray, so no voxel can be counted -- every visit of the batch is an event for the ordered replay.
  int flag_all;
  /// Occupancy maps without mean / secondary layers: a region held by a single chunk whose samples are all staged in
  /// LDS has its samples replayed by the walk's epilogue itself (the ordered sample list, the interval counters and the
  /// trailing counts are all in LDS at that point); the region is marked kSamplesApplied for k_apply_hits.
  int inline_hits;
};

constexpr uint32_t kWalkCursorWords = 24;  ///< l_cursor[]: see k_region_walk
#ifndef OHMHIP_WALK_UNROLL
#define OHMHIP_WALK_UNROLL 2
#endif
constexpr int kWalkUnroll = OHMHIP_WALK_UNROLL;  ///< walk steps per loop trip (see the loop)

/// Shape of a walk workgroup.  WalkFull is the one the design was tuned on: 1024 threads own a CU with a 32 768-voxel
/// tile.  WalkHalf (round 6) can serve regions / tiles of up to 16 384 voxels with everything halved -- threads, tile,
/// staged samples, segments per chunk -- so that TWO workgroups share a CU (at most 80.7 of 81.9 KB of LDS each, 8 waves of
/// 128 VGPRs each): one's prologue and epilogue run under the other's walk loop.  The per-thread shares (segments and
/// samples prefetched per thread, tile words per thread in the epilogue) are the same in both.  The host picks it for
/// regions of at most 4 096 voxels (16^3: -10 % per batch), where it was measured to pay (ohmhip_map.hip).
template <int kThreadsT, int kTileVoxelsT, int kLdsHitsT, uint32_t kSegmentsT, int kQueueCapT, int kMinWavesPerEuT>
struct WalkGeometry
{
  static constexpr int kMinWavesPerEu = kMinWavesPerEuT;  ///< __launch_bounds__: 4 keeps WalkHalf at 128 VGPRs (two workgroups per CU)
  static constexpr int kThreads = kThreadsT;
  static constexpr int kWaves = kThreadsT / 64;
  static constexpr int kTileVoxels = kTileVoxelsT;  ///< largest region / tile the shape serves
  static constexpr int kLdsHits = kLdsHitsT;        ///< samples of a region staged in LDS
  static constexpr uint32_t kSegments = kSegmentsT; ///< segments per chunk (LDS order array)
  static constexpr int kQueueCap = kQueueCapT;      ///< deferred events per wave
};
using WalkFull = WalkGeometry<kWalkThreads, 1 << kHitVoxelBits, kLdsHits, kMaxChunkSegments, kQueueCap, 1>;
using WalkHalf = WalkGeometry<kWalkThreads / 2, (1 << kHitVoxelBits) / 2, kLdsHits / 2, kMaxChunkSegments / 2, 96, 4>;
/// The parts of a chunk's fixed cost that are written for the common shape -- a region that fills the tile -- live in
/// functions of their own which the kernel CALLS: inlined, each of them took the kernel's register allocation from 37
/// spilled VGPRs to 50 .. 120 (see the head of this file), and a call per chunk costs a few hundred cycles.  They reach
/// LDS through pointers that keep its address space, and make their wave-uniform arguments scalar again, which the
/// calling convention hands over in vector registers.
using LdsWord = __attribute__((address_space(3))) uint32_t;
using GlobalWord = __attribute__((address_space(1))) uint32_t;
using GlobalByte = __attribute__((address_space(1))) char;
using GlobalFloat = __attribute__((address_space(1))) float;
// (the compiler's own vector types: float2 / uint4 are classes whose assignment wants the generic address space)
typedef float Float2 __attribute__((ext_vector_type(2)));
typedef uint32_t Quad __attribute__((ext_vector_type(4)));
using GlobalFloat2 = __attribute__((address_space(1))) Float2;
using LdsQuad = __attribute__((address_space(3))) Quad;

/// atomicAdd(), result unused, on a pointer that says it is global memory.
__device__ inline void addGlobal(GlobalWord *address, uint32_t value)
{
  __hip_atomic_fetch_add(address, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename T>
__device__ inline T *uniformPointer(T *p)
{
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
  return reinterpret_cast<T *>(((unsigned long long)hi << 32) | lo);
}

__device__ inline float uniformFloat(float v)
{
  return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

/// Exclusive scan over the segment ordering's counters (one wave): lane l owns kOrderBins / 64 consecutive ones.
__device__ __noinline__ void scanOrderBins(LdsWord *bins, uint32_t lane)
{
  constexpr uint32_t kQuads = kOrderBins / 256u;
  LdsQuad *mine = reinterpret_cast<LdsQuad *>(bins) + lane * kQuads;
  Quad c[kQuads];
  uint32_t total = 0;
#pragma unroll
  for (uint32_t q = 0; q < kQuads; ++q)
  {
    c[q] = mine[q];
    total += c[q].x + c[q].y + c[q].z + c[q].w;
  }
  uint32_t incl = total;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint32_t up = __shfl_up(incl, d);
    incl += (int(lane) >= d) ? up : 0u;
  }
  uint32_t run = incl - total;
#pragma unroll
  for (uint32_t q = 0; q < kQuads; ++q)
  {
    Quad e;
    e.x = run;
    e.y = e.x + c[q].x;
    e.z = e.y + c[q].y;
    e.w = e.z + c[q].z;
    run = e.w + c[q].w;
    mine[q] = e;
  }
}

/// The direct apply of a single-chunk region in the common case: a plain occupancy batch without exclusion flags on a
/// region that fills the tile (an even voxel count, every thread's words exist).  The passes are bound by instruction
/// issue -- 16 waves run their whole instruction stream whichever lanes need it -- and the general form in the kernel
/// spends most of its stream on conditions that are the same for every word.  Same loads, same arithmetic, same stores.
/// `g_counts`: where voxels which also receive samples hand their count to k_apply_hits; null when the kernel replays
/// the samples itself.  `stamps`: null, or the trace record's two words for the ends of the passes.
template <typename G>
__device__ __noinline__ void applyFullTile(const LdsWord *tile, float *occupancy, uint32_t *g_counts, MissConst mc,
                                           unsigned long long *stamps)
{
  constexpr uint32_t kWordsPerThread = uint32_t(G::kTileVoxels) / 2u / uint32_t(G::kThreads) / 2u;
  // (byte offsets from the region's first voxel: a word's two voxels are one float2)
  GlobalByte *occ_bytes = (GlobalByte *)uniformPointer(occupancy);
  GlobalWord *counts = (GlobalWord *)uniformPointer(g_counts);
  stamps = uniformPointer(stamps);
  mc.miss_value = uniformFloat(mc.miss_value);
  mc.min_value = uniformFloat(mc.min_value);
  mc.sat_min = uniformFloat(mc.sat_min);
  mc.sat_max = uniformFloat(mc.sat_max);
  for (uint32_t half = 0; half < 2u; ++half)
  {
    const uint32_t first = threadIdx.x + half * kWordsPerThread * uint32_t(G::kThreads);
    uint32_t words[kWordsPerThread];
    Float2 values[kWordsPerThread];
    // The LDS reads of the pass in one burst, one wait.
#pragma unroll
    for (uint32_t j = 0; j < kWordsPerThread; ++j)
    {
      words[j] = tile[tileWord(first + j * uint32_t(G::kThreads))];
    }
#pragma unroll
    for (uint32_t j = 0; j < kWordsPerThread; ++j)
    {
      const uint32_t i = first + j * uint32_t(G::kThreads);
      // 0xffff over every entry whose voxel also receives samples: those keep their count for the ordered replay
      // (k_apply_hits, or the kernel's own); the others are applied here.
      const uint32_t sampled = ((words[j] >> 15) & 0x00010001u) * 0xffffu;
      const uint32_t kept = words[j] & sampled & (kTileCountMask | (kTileCountMask << 16));
      words[j] &= ~sampled;
      if (counts && __ballot(kept != 0u))
      {
        if (kept & 0xffffu)
        {
          addGlobal(&counts[2 * i], kept & 0xffffu);
        }
        if (kept >> 16)
        {
          addGlobal(&counts[2 * i + 1], kept >> 16);
        }
      }
      values[j] = Float2(0.0f);
      if (words[j])
      {
        values[j] = *(const GlobalFloat2 *)(occ_bytes + i * 8u);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < kWordsPerThread; ++j)
    {
      const uint32_t i = first + j * uint32_t(G::kThreads);
      if (__ballot(words[j] != 0u))
      {
        // (a voxel at its clamp -- most of a settled map's free space -- does not move: nothing to write; neither does
        // one without a count, which gets its own value back)
        const float v0 = occMissNPlainWave(mc, values[j].x, words[j] & 0xffffu);
        if (!sameValue(v0, values[j].x))
        {
          *(GlobalFloat *)(occ_bytes + i * 8u) = v0;
        }
        const float v1 = occMissNPlainWave(mc, values[j].y, words[j] >> 16);
        if (!sameValue(v1, values[j].y))
        {
          *(GlobalFloat *)(occ_bytes + i * 8u + 4u) = v1;
        }
      }
    }
    if (stamps && threadIdx.x == 0)
    {
      stamps[half] = wall_clock64();
    }
  }
}

/// The tile flush of a multi-chunk region that fills the tile: every thread's words exist, so their LDS reads go out in
/// bursts with one wait each, and a word in which no lane of the wave holds a count is passed over on the wave's ballot.
/// `skip_masked` (NDT / TSDF): entries of masked voxels are not flushed.
template <typename G>
__device__ __noinline__ void flushFullTile(const LdsWord *tile, uint32_t *g_counts, uint32_t skip_masked)
{
  constexpr uint32_t kBurst = 8;
  constexpr uint32_t kWords = uint32_t(G::kTileVoxels) / 2u / uint32_t(G::kThreads);
  static_assert(kWords % kBurst == 0u, "the tile flush reads whole bursts");
  GlobalWord *counts = (GlobalWord *)uniformPointer(g_counts);
  skip_masked = __builtin_amdgcn_readfirstlane(skip_masked);
  for (uint32_t burst = 0; burst < kWords / kBurst; ++burst)
  {
    const uint32_t first = threadIdx.x + burst * kBurst * uint32_t(G::kThreads);
    uint32_t words[kBurst];
#pragma unroll
    for (uint32_t j = 0; j < kBurst; ++j)
    {
      words[j] = tile[tileWord(first + j * uint32_t(G::kThreads))];
    }
#pragma unroll
    for (uint32_t j = 0; j < kBurst; ++j)
    {
      const uint32_t i = first + j * uint32_t(G::kThreads);
      const uint32_t masked = skip_masked ? ((words[j] >> 15) & 0x00010001u) * 0xffffu : 0u;
      const uint32_t n = words[j] & ~masked & (kTileCountMask | (kTileCountMask << 16));
      if (__ballot(n != 0u))
      {
        if (n & 0xffffu)
        {
          addGlobal(&counts[2 * i], n & 0xffffu);
        }
        if (n >> 16)
        {
          addGlobal(&counts[2 * i + 1], n >> 16);
        }
      }
    }
  }
}

/// The count tile's initialisation for a region that fills the tile, without flag_all: every thread owns whole mask
/// words (one in both shapes), every 4-word group of its 16 tile words exists, and the mask word is the one the thread
/// prefetched.  Entries start at zero count with the voxel's mask flag in the top bit, at the positions tileWord() gives
/// them, exactly as the general form in the kernel writes them.  Everything that depends on the lane -- the store
/// addresses, the row's swizzle -- is computed here from `tid`, so the kernel keeps nothing of it alive across its chunk
/// loop.  The swizzle's low two bits permute the words inside a 4-word group: physical word r holds logical word
/// r ^ (swizzle & 3).  That is a swap of neighbouring 2-bit fields (bit 0) and of neighbouring 4-bit groups (bit 1) of
/// the mask word, applied to the word once; sixteen fixed-shift decodes follow (field to the top, arithmetic shift down
/// to bits 16 / 15, one mask).
template <typename G>
__device__ __noinline__ void initFullTile(LdsWord *tile, uint32_t mask_word, uint32_t tid)
{
  static_assert(uint32_t(G::kTileVoxels) == 32u * uint32_t(G::kThreads), "one mask word per thread");
  const uint32_t w = tid;
  const uint32_t swizzle = ((w >> 1) ^ (w >> 6)) & 31u;  // tileWord(w * 16) ^ (w * 16)
  uint32_t m = mask_word;
  uint32_t d = (m ^ (m >> 2)) & 0x33333333u & (0u - (swizzle & 1u));
  m ^= d ^ (d << 2);
  d = (m ^ (m >> 4)) & 0x0f0f0f0fu & (0u - ((swizzle >> 1) & 1u));
  m ^= d ^ (d << 4);
  // The swizzle's high bits permute the 4-word groups of the row: logical group g lies at g ^ (swizzle >> 2).
  LdsQuad *groups = reinterpret_cast<LdsQuad *>(tile);
  const uint32_t group = swizzle >> 2;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q)
  {
    Quad v;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r)
    {
      // field q * 4 + r: its low bit to bit 15, its high bit to bit 31
      const uint32_t top = m << (30u - (q * 4u + r) * 2u);
      v[r] = uint32_t(int32_t(top) >> 15) & 0x80008000u;
    }
    groups[(w * 4u + q) ^ group] = v;
  }
}

/// kSpecial: the batch contains rays whose end voxel is part of the walk (clipped / kRfEndPointAsFree / TSDF) or
/// kRfExcludeOrigin.  The common case (kSpecial == false) keeps those predicates out of the hot loop: every iteration
/// of an active lane is a miss.
/// kTrace: development instrumentation (OHMHIP_DEBUG_FLAGS 64 / 128): per-chunk time stamps and loop counters.  Compiled
/// out of the production instantiations.
template <bool kSpecial, bool kTrace, typename G = WalkFull>
__global__ void __launch_bounds__(G::kThreads, G::kMinWavesPerEu) k_region_walk(WalkArgs args)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const MapConst &mc = args.mc;
  // Layout: [count tile: ceil(region_voxels / 2) words][queues][staged sample keys][interval counters][cursor]
  // [kLengthClasses reserved words][idle words][bucket index][segment order: u16 per segment].  The tile sits at
  // offset 0 so the per-visit atomic needs no base add.
  const uint32_t count_words = uint32_t(mc.region_voxels + 1) >> 1;
  const uint32_t mask_words = uint32_t(mc.region_voxels + 31) >> 5;
  uint32_t *l_counts = lds;
  uint2 *l_queues = reinterpret_cast<uint2 *>(lds + ((count_words + 31u) & ~31u));  // (whole rows: see tileWord)
  unsigned long long *l_hits = reinterpret_cast<unsigned long long *>(l_queues + G::kWaves * G::kQueueCap);
  uint32_t *l_intervals = reinterpret_cast<uint32_t *>(l_hits + G::kLdsHits);  // [G::kLdsHits] u16 interval counters
  // l_cursor[0]: segment cursor, [1]: a fetched chunk's index, [2..5]: its record, [6..7]: its samples, [8..9]: its
  // region key; [12..21]: a second record (start-up only)
  uint32_t *l_cursor = l_intervals + G::kLdsHits / 2;
  // (kLengthClasses words behind the cursor are reserved and unused: the class counters live in l_bins)
  uint32_t *l_idle = l_cursor + kWalkCursorWords + kLengthClasses;  // [64] scratch words: where a lane with nothing to visit aims its LDS add
  uint16_t *l_index = reinterpret_cast<uint16_t *>(l_idle + 64);  // [kIndexBuckets + 2] first staged sample per bucket
  uint16_t *l_order = l_index + kIndexBuckets + 2;
  // The segment ordering's counters, [kLengthClasses descending][kOrderCopies], share the queues' words: no wave touches
  // its queue between the barrier behind a chunk's final queue flush and the barrier in front of the next walk loop.
  uint32_t *l_bins = reinterpret_cast<uint32_t *>(l_queues);
  static_assert(kOrderBins <= 2u * uint32_t(G::kWaves) * uint32_t(G::kQueueCap), "the class counters alias the queues");
  static_assert(kOrderBins % 256u == 0u, "the scan gives each of 64 lanes whole uint4s");

  // Persistent workgroups: the launch has one workgroup per CU and each takes chunks from a device-wide cursor until
  // none are left.  A static blockIdx -> chunk binding leaves the hardware's round-robin of workgroups over the 8 XCDs
  // in charge of the balance, and chunk costs vary enough that some XCDs then finish in half the time of others.
  // The chunk record (and the region's range in the sample list) travels with the index through LDS: thread 0 fetches
  // the next one while the other waves are still finishing their loop, so a trip does not start with a chain of
  // dependent global loads.
  const int defer_all = args.defer_all;
  // A workgroup's first chunk is the one with its own index (the list is ordered largest first, so the launch starts on
  // the gridDim.x largest chunks, one per workgroup, whatever order the workgroups arrive in); the shared cursor hands
  // out the chunks behind those.
  auto fetchNextChunk = [&](uint32_t *record, bool first = false) {
    const uint32_t next = first ? blockIdx.x : gridDim.x + atomicAdd(args.chunk_cursor, 1u);
    record[1] = next;
    if (next < args.n_chunks)
    {
      const Chunk c = args.chunks[next];
      record[2] = c.slot;
      record[3] = c.seg_begin;
      record[4] = c.seg_end;
      record[5] = c.hash_index;
      record[6] = defer_all ? 0u : args.bs.hit_begin[c.slot];
      record[7] = defer_all ? 0u : args.bs.hit_end[c.slot];
      const uint64_t key = args.slot_keys[c.slot];
      record[8] = uint32_t(key);
      record[9] = uint32_t(key >> 32);
    }
  };
  // A workgroup holds two chunk records: the chunk it works on and the next one.  While it walks chunk N every thread
  // loads its share of chunk N + 1's prologue inputs (segment lengths, the region's sample keys and mask words) into
  // registers -- issued behind the first lane refill of chunk N, so the loads complete under the walk and the next
  // prologue starts without a memory round trip -- and thread 0 claims chunk N + 2 while the other waves finish their
  // loop.
  constexpr int kSegPerThread = int(G::kSegments) / G::kThreads;
  constexpr int kHitsPerThread = G::kLdsHits / uint32_t(G::kThreads);
  struct ChunkRecord
  {
    uint32_t index, slot, seg_begin, seg_end, hash_index, hb, he, key_lo, key_hi;
  };
  auto readRecord = [&](const uint32_t *record) {
    // (readfirstlane: the values are wave-uniform, so the chunk loop's condition is a scalar branch and the barriers
    // inside the loop are not restructured as if threads could leave at different trips.)
    ChunkRecord r;
    r.index = __builtin_amdgcn_readfirstlane(record[1]);
    r.slot = __builtin_amdgcn_readfirstlane(record[2]);
    r.seg_begin = __builtin_amdgcn_readfirstlane(record[3]);
    r.seg_end = __builtin_amdgcn_readfirstlane(record[4]);
    r.hash_index = __builtin_amdgcn_readfirstlane(record[5]);
    r.hb = __builtin_amdgcn_readfirstlane(record[6]);
    r.he = __builtin_amdgcn_readfirstlane(record[7]);
    r.key_lo = __builtin_amdgcn_readfirstlane(record[8]);
    r.key_hi = __builtin_amdgcn_readfirstlane(record[9]);
    return r;
  };
  unsigned long long pf_hits[kHitsPerThread] = {};
  uint32_t pf_vox[kSegPerThread] = {};
  uint32_t pf_mask = 0;
  // Every global load of a chunk's prologue that depends only on the chunk record, issued back to back: clamped instead
  // of predicated so the loads share one basic block.
  auto prefetchChunk = [&](const ChunkRecord &r) {
    const uint32_t n_hits = r.he - r.hb;
    if (!defer_all && n_hits && n_hits <= uint32_t(G::kLdsHits))
    {
#pragma unroll
      for (int j = 0; j < kHitsPerThread; ++j)
      {
        pf_hits[j] = args.sorted_hits[r.hb + min(threadIdx.x + uint32_t(j) * uint32_t(G::kThreads), n_hits - 1u)];
      }
    }
    pf_mask = args.hit_mask[size_t(r.slot) * mask_words + min(threadIdx.x, mask_words - 1u)];
    const uint32_t n = r.seg_end - r.seg_begin;
#pragma unroll
    for (int j = 0; j < kSegPerThread; ++j)
    {
      pf_vox[j] = args.segments[r.seg_begin + min(threadIdx.x + uint32_t(j) * uint32_t(G::kThreads), n - 1u)].vox;
    }
  };
  // The first two records, fetched by two waves at once.
  if (threadIdx.x == 0 || threadIdx.x == 64)
  {
    fetchNextChunk(l_cursor + (threadIdx.x ? kWalkCursorWords / 2 : 0), threadIdx.x == 0);
  }
  __syncthreads();
  ChunkRecord cur = readRecord(l_cursor);
  ChunkRecord next = readRecord(l_cursor + kWalkCursorWords / 2);
  if (next.index < cur.index)
  {
    const ChunkRecord swap = cur;
    cur = next;
    next = swap;
  }
  if (cur.index < args.n_chunks)
  {
    prefetchChunk(cur);
  }
  __syncthreads();  // (everyone has read the records: thread 0 may overwrite the first one)
  while (cur.index < args.n_chunks)
  {
    unsigned long long clk_start = 0;
    if (kTrace)
    {
      clk_start = wall_clock64();
    }
    const uint32_t chunk_index = cur.index;
    Chunk chunk;
    chunk.slot = cur.slot;
    chunk.seg_begin = cur.seg_begin;
    chunk.seg_end = cur.seg_end;
    chunk.hash_index = cur.hash_index;
    const uint32_t hb = cur.hb;
    const uint32_t he = cur.he;
    // Region coordinates (packRegionKey): only the exact decisions use them.
    const int region_x = int(int16_t(cur.key_lo & 0xffffu));
    const int region_y = int(int16_t(cur.key_lo >> 16));
    const int region_z = int(int16_t(cur.key_hi & 0xffffu));
    const uint32_t n_seg = chunk.seg_end - chunk.seg_begin;
    const Segment *chunk_segments = args.segments + chunk.seg_begin;

    // ---- prologue.  One workgroup owns the CU (the tile takes most of its LDS), so nothing overlaps this phase; its
    // ---- inputs are in registers already (prefetchChunk).
    // The region's sorted sample keys are staged in LDS so deferred misses can be ordered against them at LDS latency.
    const uint32_t n_region_hits = he - hb;
    const bool lds_resolve = !defer_all && n_region_hits <= uint32_t(G::kLdsHits);
    unsigned long long my_hits[kHitsPerThread];
#pragma unroll
    for (int j = 0; j < kHitsPerThread; ++j)
    {
      my_hits[j] = pf_hits[j];
    }
    const uint32_t *g_mask = args.hit_mask + size_t(chunk.slot) * mask_words;
    const uint32_t my_mask = pf_mask;
    uint32_t bins[kSegPerThread];  // the segment's counter: its length class, longest first, and the lane's copy
#pragma unroll
    for (int j = 0; j < kSegPerThread; ++j)
    {
      bins[j] = (kLengthClasses - 1u - min(pf_vox[j] >> kSegVoxelBits, kLengthClasses - 1u)) * kOrderCopies +
                (threadIdx.x & (kOrderCopies - 1u));
    }
    for (uint32_t b = threadIdx.x; b < kOrderBins; b += uint32_t(G::kThreads))
    {
      l_bins[b] = 0;
    }
    if (threadIdx.x == 0)
    {
      l_cursor[0] = 0;
    }
    if (threadIdx.x < 64)
    {
      l_idle[threadIdx.x] = 0;
    }
    const bool stamp = kTrace && threadIdx.x == 0;
    unsigned long long clk_p[6] = { 0, 0, 0, 0, 0, 0 };
    if (stamp)
    {
      clk_p[0] = wall_clock64();
    }
    // Tile entries start at zero count with the voxel's mask flag in the top bit: one mask word covers 16 tile words,
    // half a row of the tile, which tileWord() maps onto half a row again: the 4-word groups permuted by the high bits
    // of the row's XOR constant, the words inside a group by its low two bits.  The common case has a body of its own
    // (initFullTile).
    // (The general form starts behind the last mask word when initFullTile served the region.  Written as an else
    // branch around the unchanged loop, the call took five of the six instantiations above the parent's spill counts.)
    const bool full_init = !args.flag_all && mc.region_voxels == G::kTileVoxels;
    if (full_init)
    {
      initFullTile<G>((LdsWord *)l_counts, my_mask, threadIdx.x);
    }
    for (uint32_t w = full_init ? mask_words : threadIdx.x; w < mask_words; w += uint32_t(G::kThreads))
    {
      const uint32_t mword = args.flag_all ? 0xffffffffu : ((w == threadIdx.x) ? my_mask : g_mask[w]);
      const uint32_t swizzle = tileWord(w * 16u) ^ (w * 16u);
#pragma unroll
      for (uint32_t q = 0; q < 4; ++q)
      {
        const uint32_t logical = w * 16u + q * 4u;
        if (logical + 3u < count_words)
        {
          uint32_t v[4];
#pragma unroll
          for (uint32_t r = 0; r < 4; ++r)
          {
            // physical word r of the group holds logical word r ^ (swizzle & 3)
            const uint32_t two = (mword >> ((q * 4u + (r ^ (swizzle & 3u))) * 2u)) & 3u;
            v[r] = ((two & 1u) << 15) | ((two & 2u) << 30);
          }
          *reinterpret_cast<uint4 *>(&l_counts[logical ^ (swizzle & ~3u)]) = make_uint4(v[0], v[1], v[2], v[3]);
        }
        else
        {
          for (uint32_t r = 0; r < 4; ++r)
          {
            if (logical + r < count_words)
            {
              const uint32_t two = (mword >> ((q * 4u + r) * 2u)) & 3u;
              l_counts[tileWord(logical + r)] = ((two & 1u) << 15) | ((two & 2u) << 30);
            }
          }
        }
      }
    }
    if (stamp)
    {
      clk_p[1] = wall_clock64();
    }
    __syncthreads();
    bool prefetched = false;  // wave-uniform: the next chunk's prologue loads have been issued
    if (stamp)
    {
      clk_p[2] = wall_clock64();
    }
    // Longest segments first (counting sort on the voxel count, indices in LDS): lanes refilled together get segments
    // of similar length and so retire together, and the workgroup drains on its SHORTEST segments instead of waiting
    // for a few long stragglers.  The order inside a length class is arbitrary; integer counting does not care.
    // Every class has kOrderCopies counters and a lane adds to the copy of its own index, in the count and in the
    // placement alike, so at most 64 / kOrderCopies lanes of a wave meet on one address.
#pragma unroll
    for (int j = 0; j < kSegPerThread; ++j)
    {
      if (threadIdx.x + uint32_t(j) * uint32_t(G::kThreads) < n_seg)
      {
        atomicAdd(&l_bins[bins[j]], 1u);
      }
    }
    if (lds_resolve && n_region_hits)
    {
#pragma unroll
      for (int j = 0; j < kHitsPerThread; ++j)
      {
        const uint32_t i = threadIdx.x + uint32_t(j) * uint32_t(G::kThreads);
        if (i < n_region_hits)
        {
          l_hits[i] = my_hits[j];
        }
        if (i < (n_region_hits + 1) / 2)
        {
          l_intervals[i] = 0;  // two u16 counters per word (a chunk adds at most kMaxChunkSegments to one counter)
        }
      }
    }
    __syncthreads();
    if (stamp)
    {
      clk_p[3] = wall_clock64();
    }
    if (lds_resolve && n_region_hits)
    {
      // Bucket index over the staged samples (sorted by voxel): l_index[b] = first sample of a voxel in bucket >= b.
#pragma unroll
      for (int j = 0; j < kHitsPerThread; ++j)
      {
        const uint32_t i = threadIdx.x + uint32_t(j) * uint32_t(G::kThreads);
        if (i < n_region_hits)
        {
          auto bucketOf = [](unsigned long long key) {
            return (uint32_t(key >> kHitRayBits) & ((1u << kHitVoxelBits) - 1u)) >> kIndexShift;
          };
          const uint32_t b = bucketOf(my_hits[j]);
          const uint32_t first = (i == 0) ? 0u : bucketOf(l_hits[i - 1]) + 1u;
          for (uint32_t k = first; k <= b; ++k)
          {
            l_index[k] = uint16_t(i);
          }
          if (i + 1 == n_region_hits)
          {
            for (uint32_t k = b + 1u; k <= kIndexBuckets; ++k)
            {
              l_index[k] = uint16_t(n_region_hits);
            }
          }
        }
      }
    }
    if (threadIdx.x < 64)
    {
      // Exclusive scan over the counters, which lie in DESCENDING length order: longest first.
      scanOrderBins((LdsWord *)l_bins, threadIdx.x);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kSegPerThread; ++j)
    {
      const uint32_t i = threadIdx.x + uint32_t(j) * uint32_t(G::kThreads);
      if (i < n_seg)
      {
        l_order[atomicAdd(&l_bins[bins[j]], 1u)] = uint16_t(i);
      }
    }
    __syncthreads();
    if (stamp)
    {
      clk_p[4] = wall_clock64();
      if (chunk_index < kTraceChunks)
      {
        unsigned long long *rec = args.dbg_counters + 16 + size_t(chunk_index) * kTraceWords;
        rec[20] = clk_p[0];
        rec[21] = clk_p[1];
        rec[22] = clk_p[2];
        rec[23] = clk_p[3];
      }
    }

    const unsigned lane = laneId();
    const unsigned wave = threadIdx.x >> 6;
    uint2 *queue = l_queues + wave * G::kQueueCap;
    const int dimx = mc.dim[0];
    const int dimxy = mc.dim[0] * mc.dim[1];
    const unsigned long long slot_bits = (unsigned long long)chunk.slot << kHitSlotShift;
    const int ray_shift = args.ray_shift;
    const int refill_min_idle = args.refill_min_idle;
    const bool refill_only = kTrace && (args.dbg & 16u) != 0;
    const uint32_t fix_margin = mc.fix_margin;
    const uint32_t idle_address = uint32_t(reinterpret_cast<char *>(l_idle + lane) - reinterpret_cast<char *>(lds));

    // Per-lane walk state (all named scalars: no run-time indexed arrays).
    int left = 0;  // voxels this lane still has to visit in its segment (<= 0: idle)
    uint32_t f0 = 0, f1 = 0, f2 = 0, d0 = 0, d1 = 0, d2 = 0;  // predictor: next step time / step delta per axis
    int sx = 0, sy = 0, sz = 0;  // change of `va` per step along each axis
    uint32_t va = 0;             // byte offset of the current voxel's u16 tile entry (2 x voxel index)
    uint32_t ray = 0;
    uint32_t skip = 0;      // kSpecial only: first voxel is not visited (kRfExcludeOrigin)
    uint32_t end_last = 0;  // kSpecial only: the segment's last voxel is the ray's end voxel
    uint32_t qcount = 0;     // wave-uniform
    bool exhausted = false;  // wave-uniform
    uint32_t dbg_iters = 0, dbg_active = 0, dbg_refills = 0, dbg_fm = 0, dbg_slow = 0;  // wave-uniform (kTrace)
    uint32_t dbg_s2 = 0, dbg_s3 = 0, dbg_sl = 0, dbg_sp = 0;
    unsigned long long clk_loop = 0;
    if (kTrace)
    {
      clk_loop = wall_clock64();
    }

    // The walk loop.  A wave's trip is a chain of dependent hops (LDS round trip, mask algebra on the scalar unit,
    // branches), and with four waves per SIMD the chain, not instruction issue, sets the pace.  So one trip takes
    // kWalkUnroll steps per lane: one refill / exit test per trip, the steps' LDS adds in flight together, their
    // returned flags tested after the last step.  A lane whose segment ends inside a trip idles for the rest of it.
    int refill_threshold = refill_min_idle;  // idle lanes that trigger a refill; 64 once the chunk has no segments left
    while (true)
    {
      // ---- refill idle lanes (wave-uniform decision) ------------------------------------------------------------------
      const unsigned long long am = __ballot(left > 0);
      const int n_idle = 64 - __popcll(am);
      if (__builtin_expect(n_idle >= refill_threshold, 0))
      {
        if (exhausted)
        {
          break;  // every lane idle and nothing left to hand out
        }
        if (kTrace)
        {
          ++dbg_refills;
        }
        uint32_t base = 0;
        if (lane == 0)
        {
          base = atomicAdd(l_cursor, uint32_t(n_idle));
        }
        base = __builtin_amdgcn_readfirstlane(base);
        exhausted = base + uint32_t(n_idle) >= n_seg;
        refill_threshold = exhausted ? 64 : refill_threshold;
        const unsigned long long idle = ~am;
        const uint32_t mine =
          base + __builtin_amdgcn_mbcnt_hi(uint32_t(idle >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(idle), 0u));
        if (left <= 0 && mine < n_seg)
        {
          const uint4 *rec = reinterpret_cast<const uint4 *>(chunk_segments + l_order[mine]);
          const uint4 ra = rec[0];
          const uint4 rb = rec[1];
          f0 = ra.x;
          f1 = ra.y;
          f2 = ra.z;
          va = (ra.w & ((1u << kSegVoxelBits) - 1u)) << 1;
          left = int(ra.w >> kSegVoxelBits);
          d0 = rb.x & ~kSegNegative;
          d1 = rb.y & ~kSegNegative;
          d2 = rb.z & ~kSegNegative;
          sx = (rb.x & kSegNegative) ? -2 : 2;
          sy = (rb.y & kSegNegative) ? -2 * dimx : 2 * dimx;
          sz = (rb.z & kSegNegative) ? -2 * dimxy : 2 * dimxy;
          ray = rb.w & kSegRayMask;
          if (kSpecial)
          {
            skip = (rb.w & kSegSkipFirst) ? 1u : 0u;
            end_last = (rb.w & kSegEnd) ? 1u : 0u;
          }
          left = refill_only ? 0 : left;
        }
        if (!prefetched)
        {
          // First refill of the chunk: the lanes' records are on their way, now queue the next chunk's prologue loads
          // behind them (loads return in order, so nothing in this chunk ever waits for these).
          prefetched = true;
          if (next.index < args.n_chunks)
          {
            prefetchChunk(next);
          }
        }
      }

      uint32_t olds[kWalkUnroll];     // tile word returned by each step's LDS add
      uint32_t visited[kWalkUnroll];  // `va` of each step's voxel
#pragma unroll
      for (int u = 0; u < kWalkUnroll; ++u)
      {
        // ---- visit: count the miss and fetch the voxel's mask flag with one returning LDS atomic.  Masked voxels
        // ---- (which also receive samples) are counted too; the ordering pass moves such a miss to an interval counter
        // ---- when a later sample of the voxel exists.  `va` is the byte offset of the voxel's u16 tile entry
        // ---- (2 x voxel index): word address = va & ~3, and the shifts only read the low five bits of their shift
        // ---- operand, so (va << 3) selects bit 0 or 16 of the word for the count and (.. | 15) bit 15 or 31 for the
        // ---- flag.  A lane with nothing to visit adds to its own scratch word instead (no exec-mask juggling; the
        // ---- scratch words start every chunk at zero and a lane idles for far fewer than 2^15 steps of a chunk, so
        // ---- their flag bits stay clear).
        // kSpecial: the ray's end voxel (last voxel of a kSegEnd segment) is always visited; kRfExcludeOrigin drops
        // the first voxel of the ray otherwise.
        const bool at_end = kSpecial && end_last && left == 1;
        const bool visit = kSpecial ? (left > 0 && (at_end || !skip)) : (left > 0);
        visited[u] = va;
        olds[u] = tileAdd(visit ? tileAddress(va) : idle_address, shiftOne(va << 3));
        if (kSpecial)
        {
          skip = 0;
        }
        if (kTrace)
        {
          ++dbg_iters;
          dbg_active += uint32_t(__popcll(__ballot(visit)));
        }

        int stride;
        {
          // ---- one walk step from the fixed-point predictor (see Segment), taken by every lane.  The smallest
          // ---- candidate is trusted when it lies inside the region's range (below kFixMaxDelta) and leads the second
          // ---- smallest by more than the accumulated truncation error; a visiting lane that cannot trust it asks the
          // ---- reference's fp64 arithmetic (rare: near-ties, ray ends that disagree with their keys, degenerate rays).
          const uint32_t fmin = umin3(f0, f1, f2);
          const uint32_t fmed = umed3(f0, f1, f2);
          const uint32_t limit = min(fmed, kFixMaxDelta);
          const uint32_t lead = addSatUniform(fmin, fix_margin);
          const unsigned long long certain = __builtin_amdgcn_uicmp(lead, limit, kIcmpUlt);
          unsigned long long a0 = __builtin_amdgcn_uicmp(f0, fmin, kIcmpEq);
          unsigned long long a2 = __builtin_amdgcn_uicmp(f2, fmin, kIcmpEq);
          // (a lane on its segment's LAST voxel takes a step nobody uses -- its predictors are parked when the ray ends
          // there, which would send every ray of a TSDF / end-point-as-free batch through the exact path once for nothing)
          const unsigned long long slow = __ballot(left > 1) & ~certain;
          if (__builtin_expect(slow != 0, 0))
          {
            int axis = 1;
            if ((slow >> lane) & 1ull)
            {
              uint32_t r = ray;
              asm volatile("" : "+v"(r));  // keeps the record's address arithmetic inside this (rare) block
              axis = exactNextAxis(mc, args.walks[r], region_x, region_y, region_z, va >> 1);
            }
            a0 = (a0 & ~slow) | (slow & __ballot(axis == 0));
            a2 = (a2 & ~slow) | (slow & __ballot(axis == 2));
            if (kTrace)
            {
              ++dbg_slow;
              dbg_s2 += uint32_t(__popcll(slow & __ballot(left == 2)));
              dbg_s3 += uint32_t(__popcll(slow & __ballot(left == 3)));
              dbg_sl += uint32_t(__popcll(slow));
              dbg_sp += uint32_t(__popcll(slow & __ballot((d0 | d1 | d2) == 0u)));
            }
          }
          const unsigned long long a1 = ~(a0 | a2);
          f0 = addSat(f0, selectOrZero(a0, d0));
          f1 = addSat(f1, selectOrZero(a1, d1));
          f2 = addSat(f2, selectOrZero(a2, d2));
          stride = selectI(a2, sz, selectI(a0, sx, sy));
        }
        va += uint32_t(stride);
        left -= 1;
      }

      // ---- deferred ordering of misses on masked voxels.  The returned tile words are consumed after the trip's last
      // ---- step, so the LDS round trips are covered by the step arithmetic (waitTile carries the s_waitcnt).
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < kWalkUnroll; ++u)
      {
        olds[u] = waitTile(olds[u]);  // (the first one waits; LDS operations return in order)
      }
#pragma unroll
      for (int u = 0; u < kWalkUnroll; ++u)
      {
        // (a lane that did not visit holds its scratch word, whose flag bits are clear)
        const bool flagged = __builtin_amdgcn_ubfe(olds[u], (visited[u] << 3) | 15u, 1u) != 0;
        const unsigned long long fm = __ballot(flagged);
        if (kTrace)
        {
          dbg_fm += fm ? 1u : 0u;
        }
        if (fm)
        {
          if (flagged)
          {
            const uint32_t pos =
              qcount + __builtin_amdgcn_mbcnt_hi(uint32_t(fm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(fm), 0u));
            queue[pos] = make_uint2(visited[u] >> 1, ray);
          }
          qcount += uint32_t(__popcll(fm));
          if (qcount > uint32_t(G::kQueueCap - 64))
          {
            flushQueue(queue, qcount, lane, slot_bits, ray_shift, lds_resolve, l_hits, l_index, n_region_hits,
                       l_intervals, l_counts, args.events, args.event_capacity, args.event_count, defer_all, args.bs,
                       args.sorted_hits, args.miss_counts, args.interval_counts, mc.region_voxels);
            qcount = 0;
          }
        }
      }
    }

    if (kTrace && lane == 0)
    {
      const unsigned long long clk_end_loop = wall_clock64();
      if (chunk_index < kTraceChunks)
      {
        unsigned long long *rec = args.dbg_counters + 16 + size_t(chunk_index) * kTraceWords;
        if (wave < 15)
        {
          rec[2 + wave] = clk_end_loop;
        }
        if (wave == 0)
        {
          rec[0] = n_seg | ((unsigned long long)((chunk.hash_index >> 31) & 1u) << 32);
          rec[1] = clk_loop;
          rec[18] = clk_start;
          rec[17] = (unsigned long long)__builtin_amdgcn_s_getreg(63492) |
                    ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32);  // HW_ID | XCC_ID
        }
      }
      if (args.dbg & 128u)
      {
        atomicAdd(&args.dbg_counters[0], (unsigned long long)dbg_iters);
        atomicAdd(&args.dbg_counters[1], (unsigned long long)dbg_active);
        atomicAdd(&args.dbg_counters[2], (unsigned long long)dbg_refills);
        atomicAdd(&args.dbg_counters[3], (unsigned long long)dbg_fm);
        atomicAdd(&args.dbg_counters[4], (unsigned long long)dbg_slow);
        atomicAdd(&args.dbg_counters[5], (unsigned long long)dbg_s2);
        atomicAdd(&args.dbg_counters[6], (unsigned long long)dbg_s3);
        atomicAdd(&args.dbg_counters[7], (unsigned long long)dbg_sl);
        atomicAdd(&args.dbg_counters[8], (unsigned long long)dbg_sp);
      }
    }
    // Final queue flush.
    if (qcount)
    {
      flushQueue(queue, qcount, lane, slot_bits, ray_shift, lds_resolve, l_hits, l_index, n_region_hits, l_intervals,
                 l_counts, args.events, args.event_capacity, args.event_count, defer_all, args.bs, args.sorted_hits,
                 args.miss_counts, args.interval_counts, mc.region_voxels);
    }
    if (threadIdx.x == 0)
    {
      fetchNextChunk(l_cursor);  // the chunk after the next one; overlaps with the other waves finishing their loop
    }
    __syncthreads();
    const ChunkRecord after_next = readRecord(l_cursor);
    if (stamp && chunk_index < kTraceChunks)
    {
      args.dbg_counters[16 + size_t(chunk_index) * kTraceWords + 24] = wall_clock64();  // epilogue start
    }

    const bool inline_hits = args.inline_hits && lds_resolve && n_region_hits > 0u && args.occupancy && !args.rewalk &&
                             (chunk.hash_index & 0x80000000u);
    if (lds_resolve && !inline_hits)
    {
      for (uint32_t i = threadIdx.x; i < n_region_hits; i += uint32_t(G::kThreads))
      {
        const uint32_t c = (l_intervals[i >> 1] >> ((i & 1u) * 16u)) & 0xffffu;
        if (c)
        {
          atomicAdd(&args.interval_counts[hb + i], c);
        }
      }
    }
    uint32_t *g_counts = args.miss_counts + size_t(chunk.slot) * size_t(mc.region_voxels);
    if (args.rewalk && (chunk.hash_index & 0x80000000u))
    {
      __syncthreads();
      cur = next;
      next = after_next;
      continue;
    }
    if (args.occupancy && (chunk.hash_index & 0x80000000u))
    {
      // This chunk holds ALL of the region's segments for the batch: apply the miss counts to the log-odds layer
      // straight from LDS (no count round trip through HBM).  Voxels which also receive samples keep their count for
      // the ordered replay (occupancy: k_apply_hits; NDT: their visits are events, the tile entry is not used).
      float *g_occ = args.occupancy + size_t(chunk.slot) * size_t(mc.region_voxels);
      // Load pass / update pass, so the loads of the voxels a thread updates are in flight together (a load -> update ->
      // store loop would pay the memory latency once per touched word, and nothing else runs on this CU to hide it);
      // in two halves, which keeps the kernel's register peak below the walk loop's budget.
      constexpr uint32_t kWordsPerThread = uint32_t(G::kTileVoxels) / 2u / uint32_t(G::kThreads) / 2u;
      const bool even_voxels = (mc.region_voxels & 1) == 0;
      // The common case has a body of its own (applyFullTile).
      constexpr unsigned kExcludeFlags =
        OHMHIP_RF_EXCLUDE_UNOBSERVED | OHMHIP_RF_EXCLUDE_FREE | OHMHIP_RF_EXCLUDE_OCCUPIED;
      if (!defer_all && !(args.ray_flags & kExcludeFlags) && mc.region_voxels == G::kTileVoxels)
      {
        const MissConst miss = { mc.miss_value, mc.min_value, mc.sat_min, mc.sat_max };
        applyFullTile<G>((const LdsWord *)l_counts, g_occ, inline_hits ? nullptr : g_counts, miss,
                         (kTrace && chunk_index < kTraceChunks) ?
                           args.dbg_counters + 16 + size_t(chunk_index) * kTraceWords + 25 :
                           nullptr);
      }
      else
      {
      for (uint32_t half = 0; half < 2u; ++half)
      {
      uint32_t words[kWordsPerThread];
      float2 values[kWordsPerThread];
#pragma unroll
      for (uint32_t j = 0; j < kWordsPerThread; ++j)
      {
        const uint32_t i = threadIdx.x + (half * kWordsPerThread + j) * uint32_t(G::kThreads);
        const uint32_t flagged_w = (i < count_words) ? l_counts[tileWord(i)] : 0u;
        uint32_t w = flagged_w;
        // Keep only the entries applied here: unflagged voxels with a count.
        w = (w & kTileFlag) ? (w & 0xffff0000u) : w;
        w = (w & (kTileFlag << 16)) ? (w & 0x0000ffffu) : w;
        if (!defer_all && !inline_hits)
        {
          // Voxels which also receive samples keep their count for the ordered replay (k_apply_hits).
          if ((flagged_w & kTileFlag) && (flagged_w & kTileCountMask))
          {
            atomicAdd(&g_counts[2 * i], flagged_w & kTileCountMask);
          }
          if ((flagged_w & (kTileFlag << 16)) && ((flagged_w >> 16) & kTileCountMask))
          {
            atomicAdd(&g_counts[2 * i + 1], (flagged_w >> 16) & kTileCountMask);
          }
        }
        words[j] = w;
        values[j] = make_float2(0.0f, 0.0f);
        if (w)
        {
          if (even_voxels)
          {
            values[j] = *reinterpret_cast<const float2 *>(&g_occ[2 * i]);
          }
          else
          {
            values[j].x = g_occ[2 * i];
            values[j].y = (2 * i + 1 < uint32_t(mc.region_voxels)) ? g_occ[2 * i + 1] : 0.0f;
          }
        }
      }
#pragma unroll
      for (uint32_t j = 0; j < kWordsPerThread; ++j)
      {
        const uint32_t i = threadIdx.x + (half * kWordsPerThread + j) * uint32_t(G::kThreads);
        const uint32_t w = words[j];
        if (w)
        {
          const uint32_t n0 = w & kTileCountMask;
          const uint32_t n1 = (w >> 16) & kTileCountMask;
          // (a voxel at its clamp -- most of a settled map's free space -- does not move: nothing to write)
          if (n0)
          {
            const float v = occMissN(mc, args.ray_flags, values[j].x, n0);
            if (!sameValue(v, values[j].x))
            {
              g_occ[2 * i] = v;
            }
          }
          if (n1)
          {
            const float v = occMissN(mc, args.ray_flags, values[j].y, n1);
            if (!sameValue(v, values[j].y))
            {
              g_occ[2 * i + 1] = v;
            }
          }
        }
      }
      if (stamp && chunk_index < kTraceChunks)
      {
        args.dbg_counters[16 + size_t(chunk_index) * kTraceWords + 25 + half] = wall_clock64();
      }
      }  // halves
      }  // general form
      if (inline_hits)
      {
        // Ordered replay of the region's samples, one lane per voxel with samples (the head of its run in the sorted
        // list): misses before each sample from the interval counters, the sample, the trailing misses from the tile.
        // These voxels are disjoint from the ones the passes above wrote.
        for (uint32_t i = threadIdx.x; i < n_region_hits; i += uint32_t(G::kThreads))
        {
          const unsigned long long key = l_hits[i];
          const unsigned long long group = key >> kHitRayBits;
          if (i > 0u && (l_hits[i - 1u] >> kHitRayBits) == group)
          {
            continue;
          }
          const uint32_t vi = uint32_t(group) & ((1u << kHitVoxelBits) - 1u);
          float x = g_occ[vi];
          for (uint32_t j = i; j < n_region_hits && (l_hits[j] >> kHitRayBits) == group; ++j)
          {
            x = occMissN(mc, args.ray_flags, x, (l_intervals[j >> 1] >> ((j & 1u) * 16u)) & 0xffffu);
            x = occHit(mc, args.ray_flags, x);
          }
          const uint32_t w = l_counts[tileWord(vi >> 1)];
          x = occMissN(mc, args.ray_flags, x, (w >> ((vi & 1u) * 16u)) & kTileCountMask);
          g_occ[vi] = x;
        }
        if (stamp && chunk_index < kTraceChunks)
        {
          args.dbg_counters[16 + size_t(chunk_index) * kTraceWords + 27] = wall_clock64();
        }
        if (threadIdx.x == 0)
        {
          atomicOr(&args.bs.hit_begin[chunk.slot], kSamplesApplied);
        }
      }
      if (stamp && chunk_index < kTraceChunks)
      {
        args.dbg_counters[16 + size_t(chunk_index) * kTraceWords + 19] = wall_clock64();
      }
      __syncthreads();
      cur = next;
      next = after_next;
      continue;
    }
    if (args.tsdf && (chunk.hash_index & 0x80000000u))
    {
      // TSDF, region held by this one chunk: voxels that only saw free-space visits (count n, not flagged) end at
      // weight = min(weight + n, max_weight), distance = truncation distance (see k_apply_counts_tsdf) -- applied here
      // straight from LDS; flagged voxels are replayed from their events.
      float2 *g_tsdf = reinterpret_cast<float2 *>(args.tsdf) + size_t(chunk.slot) * size_t(mc.region_voxels);
      constexpr uint32_t kTsdfBatch = 4;
      for (uint32_t first = threadIdx.x; first < count_words; first += kTsdfBatch * uint32_t(G::kThreads))
      {
        uint32_t words[kTsdfBatch];
        float2 values[2 * kTsdfBatch];
#pragma unroll
        for (uint32_t j = 0; j < kTsdfBatch; ++j)
        {
          const uint32_t i = first + j * uint32_t(G::kThreads);
          uint32_t w = (i < count_words) ? l_counts[tileWord(i)] : 0u;
          w = (w & kTileFlag) ? (w & 0xffff0000u) : w;
          w = (w & (kTileFlag << 16)) ? (w & 0x0000ffffu) : w;
          words[j] = w;
          values[2 * j] = make_float2(0.0f, 0.0f);
          values[2 * j + 1] = make_float2(0.0f, 0.0f);
          if (w & kTileCountMask)
          {
            values[2 * j] = g_tsdf[2 * i];
          }
          if ((w >> 16) & kTileCountMask)
          {
            values[2 * j + 1] = g_tsdf[2 * i + 1];
          }
        }
#pragma unroll
        for (uint32_t j = 0; j < kTsdfBatch; ++j)
        {
          const uint32_t i = first + j * uint32_t(G::kThreads);
          const uint32_t n0 = words[j] & kTileCountMask;
          const uint32_t n1 = (words[j] >> 16) & kTileCountMask;
          if (n0)
          {
            const float wn = values[2 * j].x + float(n0);
            g_tsdf[2 * i] = make_float2((mc.tsdf_max_weight < wn) ? mc.tsdf_max_weight : wn, mc.tsdf_trunc);
          }
          if (n1)
          {
            const float wn = values[2 * j + 1].x + float(n1);
            g_tsdf[2 * i + 1] = make_float2((mc.tsdf_max_weight < wn) ? mc.tsdf_max_weight : wn, mc.tsdf_trunc);
          }
        }
      }
      if (stamp && chunk_index < kTraceChunks)
      {
        args.dbg_counters[16 + size_t(chunk_index) * kTraceWords + 19] = wall_clock64();
      }
      __syncthreads();
      cur = next;
      next = after_next;
      continue;
    }
    // Flush the tile: integer adds, so the merge across chunks of one region is order independent.  (NDT / TSDF:
    // entries of masked voxels are skipped -- their visits travel as events.)
    const bool full_tile = mc.region_voxels == G::kTileVoxels;
    if (full_tile)
    {
      flushFullTile<G>((const LdsWord *)l_counts, g_counts, uint32_t(defer_all));
    }
    for (uint32_t i = threadIdx.x; !full_tile && i < count_words; i += uint32_t(G::kThreads))
    {
      const uint32_t w = l_counts[tileWord(i)];
      if (w & (kTileCountMask | (kTileCountMask << 16)))
      {
#pragma unroll
        for (uint32_t half = 0; half < 2; ++half)
        {
          const uint32_t entry = (w >> (16u * half)) & 0xffffu;
          const uint32_t n = entry & kTileCountMask;
          if (n && !(defer_all && (entry & kTileFlag)))
          {
            atomicAdd(&g_counts[2 * i + half], n);
          }
        }
      }
    }
    if (stamp && chunk_index < kTraceChunks)
    {
      args.dbg_counters[16 + size_t(chunk_index) * kTraceWords + 19] = wall_clock64();
    }
    // The tile is reused by the next trip: everyone must be done reading it.
    __syncthreads();
    cur = next;
    next = after_next;
  }  // chunk loop
}

/// Resolve the deferred miss events (grid-stride; the event count lives in device memory).
__global__ void __launch_bounds__(256)
  k_flagged_events(BatchScratch bs, const unsigned long long *__restrict__ events, uint32_t event_capacity,
                   const uint32_t *__restrict__ event_count, const unsigned long long *__restrict__ sorted_hits,
                   uint32_t *__restrict__ miss_counts, uint32_t *__restrict__ interval_counts, int region_voxels,
                   uint32_t *__restrict__ host_event_count)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    *host_event_count = *event_count;  // pinned: sizes the next batch's event list
  }
  const uint32_t n = min(*event_count, event_capacity);
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
  {
    resolveFlaggedMiss(events[i], bs, sorted_hits, miss_counts, interval_counts, region_voxels);
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_WALK_KERNEL_H
