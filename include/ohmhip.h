/*
 * ohmhip.h -- C ABI of libohmhip.so: the MI355X (gfx950) replacement for the part of ohm's `gputil` + `ohmgpu`
 * that sits under ohm::GpuMap::integrateRays / GpuNdtMap / GpuTsdfMap.
 *
 * Plain C: opaque handles, POD structs, pointers and sizes.  No C++/torch types cross this boundary and no
 * exception does either: every function returns an int status (0 == OHMHIP_OK, negative == ohmhip error,
 * positive == hipError_t value); ohmhip_error_string() renders it.
 *
 * Citations are file:line in the reference checkout (csiro-robotics/ohm).  Two groups:
 *   1. device plumbing  -- what ohmgpu's hot path uses of gputil::Device/Queue/Event/Buffer/PinnedBuffer;
 *   2. the typed hot path -- one resident voxel map per handle, ray batches in, region layers out.  This replaces
 *      the generic `gputil::Kernel` variadic launch of regionRayUpdateOccupancy, regionRayUpdateNdt, covarianceHitNdt and tsdfRayUpdate
 *      (ohmgpu/GpuMap.cpp:1130-1164, ohmgpu/GpuNdtMap.cpp:383-486, ohmgpu/GpuTsdfMap.cpp:262-263) and the
 *      GpuLayerCache upload/download protocol (ohmgpu/GpuLayerCache.cpp:172-182, 300-321, 429-633).
 */
#ifndef OHMHIP_H
#define OHMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* CORE ABI.  The header has grown to 91 entry points over six rounds; a reference-side binding of ohm::GpuMap /
 * GpuNdtMap / GpuTsdfMap / GpuCache needs FIFTEEN of them.  The list below is exact: it is every ohmhip_* call made by
 * ohm_amd/host/ref_adaptor/private/HipBindingCore.cpp, the compiled and GPU-tested logic of the Level-2 adaptor
 * (INTEGRATION.md), and tests/test_cabi.py keeps the two in step.
 *   OHMHIP_CORE_ABI: ohmhip_error_string ohmhip_map_config_default ohmhip_map_create ohmhip_map_destroy
 *   OHMHIP_CORE_ABI: ohmhip_map_update_config ohmhip_map_integrate_rays ohmhip_map_integrate_rays_filtered ohmhip_map_sync
 *   OHMHIP_CORE_ABI: ohmhip_map_write_regions ohmhip_map_dirty_regions ohmhip_map_read_regions ohmhip_map_clear_dirty
 *   OHMHIP_CORE_ABI: ohmhip_map_clear ohmhip_map_remove_regions ohmhip_map_cache_stats
 * (the gputil::Device / Queue / Event / Buffer backend adds group 1 below; ohmhip_map_integrate_rays_device and
 * ohmhip_transform_samples serve GpuTransformSamples callers.)  Everything else is optional: residency limit and spill,
 * region listings and zero-copy views, LineKeysQueryGpu, multi-GPU (group 3).  Entry points that only tune or measure
 * -- knobs found useful while optimising, nothing a binding has to know -- carry OHMHIP_EXPERIMENTAL: they may change
 * or go without notice. */
#define OHMHIP_EXPERIMENTAL

#define OHMHIP_OK 0
#define OHMHIP_ERR_INVALID_ARG (-1)
#define OHMHIP_ERR_NO_DEVICE (-2)
#define OHMHIP_ERR_CAPACITY (-3)    /* region pool exhausted and could not grow */
#define OHMHIP_ERR_UNSUPPORTED (-4) /* flag / layout not supported by the HIP path */
#define OHMHIP_ERR_NOT_FOUND (-5)
#define OHMHIP_ERR_INTERNAL (-6)
#define OHMHIP_ERR_PEER (-7)        /* a collective call was abandoned because ANOTHER rank failed in it */

const char *ohmhip_error_string(int status);
/* Identifies the build: 16 hex digits over the library's sources (set by __graft_entry__.build()), "unversioned" for
 * other builds.  Recorded with profiles so a counter profile of another build is not quoted for this one. */
const char *ohmhip_build_id(void);

/* ------------------------------------------------------------------------------------------------------------------ */
/* 1. Device plumbing (replaces gputil)                                                                               */
/* ------------------------------------------------------------------------------------------------------------------ */
typedef struct ohmhip_stream_s *ohmhip_stream_t; /* gputil::Queue  (gputil/gpuQueue.h:39)  */
typedef struct ohmhip_event_s *ohmhip_event_t;   /* gputil::Event  (gputil/gpuEvent.h:23)  */
typedef struct ohmhip_buffer_s *ohmhip_buffer_t; /* gputil::Buffer (gputil/gpuBuffer.h:73) */

typedef struct ohmhip_device_info
{
  char name[256];
  char arch[64];
  uint64_t total_memory;      /* gputil::Device::deviceMemory()       gputil/gpuDevice.h:163-171 */
  uint64_t max_allocation;    /* gputil::Device::maxAllocationSize()  */
  int compute_units;
  int lds_bytes_per_block;
  int unified_memory;         /* gputil::Device::unifiedMemory()      */
} ohmhip_device_info;

int ohmhip_device_count(int *count);                            /* gputil/cuda/gpuDevice.cpp:108-115 */
int ohmhip_device_select(int device);                           /* gputil/cuda/gpuKernel.cpp:33 (cudaSetDevice) */
int ohmhip_device_get_info(int device, ohmhip_device_info *info);
int ohmhip_device_synchronize(void);                            /* cudaDeviceSynchronize, gputil/cuda/gpuBuffer.cpp (pin) */

int ohmhip_stream_create(ohmhip_stream_t *stream);              /* gputil/cuda/gpuDevice.cpp:156 */
int ohmhip_stream_destroy(ohmhip_stream_t stream);              /* gputil/cuda/gpuQueue.cpp:22  */
int ohmhip_stream_finish(ohmhip_stream_t stream);               /* Queue::finish   gputil/cuda/gpuQueue.cpp:114 */
int ohmhip_stream_wait_event(ohmhip_stream_t stream, ohmhip_event_t event); /* gputil/cuda/gpuKernel.cpp:91 */

int ohmhip_event_create(ohmhip_event_t *event);                 /* gputil/cuda/gpuEvent.cpp:150 (blocking sync) */
int ohmhip_event_destroy(ohmhip_event_t event);                 /* gputil/cuda/gpuEvent.cpp:22  */
int ohmhip_event_record(ohmhip_event_t event, ohmhip_stream_t stream); /* Queue::mark gputil/gpuQueue.h:68-96 */
int ohmhip_event_wait(ohmhip_event_t event);                    /* Event::wait      gputil/cuda/gpuEvent.cpp:95 */
int ohmhip_event_is_complete(ohmhip_event_t event, int *complete); /* Event::isComplete gputil/cuda/gpuEvent.cpp:76 */
int ohmhip_event_elapsed_ms(ohmhip_event_t start, ohmhip_event_t stop, float *ms);

/* Buffer flags: gputil/gpuBuffer.h:24-45 */
#define OHMHIP_BF_READ (1u << 0)
#define OHMHIP_BF_WRITE (1u << 1)
#define OHMHIP_BF_HOST_ACCESS (1u << 2) /* pinned host allocation (cudaHostAlloc, gputil/cuda/gpuBuffer.cpp:249) */

int ohmhip_buffer_create(ohmhip_buffer_t *buffer, size_t bytes, unsigned flags); /* gputil/cuda/gpuBuffer.cpp:240 */
int ohmhip_buffer_destroy(ohmhip_buffer_t buffer);                               /* :273-276 */
int ohmhip_buffer_resize(ohmhip_buffer_t buffer, size_t bytes, size_t *actual);  /* grow-only, gpuBuffer.h:161 */
int ohmhip_buffer_size(ohmhip_buffer_t buffer, size_t *bytes);
int ohmhip_buffer_ptr(ohmhip_buffer_t buffer, void **device_ptr);                /* Buffer::argPtr */
/* stream == NULL => synchronous (gputil/cuda/gpuBuffer.cpp:78); otherwise async + optional completion event (:58-67) */
int ohmhip_buffer_write(ohmhip_buffer_t buffer, const void *src, size_t bytes, size_t dst_offset,
                        ohmhip_stream_t stream, ohmhip_event_t block_on, ohmhip_event_t completion);
int ohmhip_buffer_read(ohmhip_buffer_t buffer, void *dst, size_t bytes, size_t src_offset, ohmhip_stream_t stream,
                       ohmhip_event_t block_on, ohmhip_event_t completion);
int ohmhip_buffer_fill(ohmhip_buffer_t buffer, int byte_value, size_t bytes, size_t offset,
                       ohmhip_stream_t stream);                                  /* gputil/cuda/gpuBuffer.cpp:206 */
/* Buffer::fill / fillPartial with an arbitrary pattern (gputil/gpuBuffer.h:199-236): `bytes` from `offset` are filled
 * with repetitions of the pattern, the last one cut short if it does not fit.  Asynchronous when `stream` is given. */
int ohmhip_buffer_fill_pattern(ohmhip_buffer_t buffer, const void *pattern, size_t pattern_size, size_t bytes,
                               size_t offset, ohmhip_stream_t stream, ohmhip_event_t block_on,
                               ohmhip_event_t completion);
/* gputil::copyBuffer (gputil/gpuBuffer.h:459-510): device-side copy between two buffers. */
int ohmhip_buffer_copy(ohmhip_buffer_t dst, size_t dst_offset, ohmhip_buffer_t src, size_t src_offset, size_t bytes,
                       ohmhip_stream_t stream, ohmhip_event_t block_on, ohmhip_event_t completion);
int ohmhip_buffer_flags(ohmhip_buffer_t buffer, unsigned *flags);                /* Buffer::flags */
/* Pinned host staging memory (gputil::PinnedBuffer, gputil/cuda/gpuPinnedBuffer.cpp:66-131). */
int ohmhip_host_alloc(void **ptr, size_t bytes);
int ohmhip_host_free(void *ptr);

/* ------------------------------------------------------------------------------------------------------------------ */
/* 2. The hot path: a device-resident voxel map                                                                       */
/* ------------------------------------------------------------------------------------------------------------------ */

/* Voxel layers (ohm/DefaultLayer.cpp:76-311).  Bit i <=> layer id i. */
enum ohmhip_layer_id
{
  OHMHIP_LID_OCCUPANCY = 0,  /* float, clear +inf                        */
  OHMHIP_LID_MEAN = 1,       /* VoxelMean {u32 coord, u32 count}         ohm/VoxelMeanCompute.h:29-33 */
  OHMHIP_LID_COVARIANCE = 2, /* CovarianceVoxel float[6]                 ohm/CovarianceVoxelCompute.h:56-66 */
  OHMHIP_LID_TRAVERSAL = 3,  /* float                                    */
  OHMHIP_LID_TOUCH_TIME = 4, /* u32 ms since first ray                   */
  OHMHIP_LID_INCIDENT = 5,   /* u32 packed normal                        */
  OHMHIP_LID_INTENSITY = 6,  /* IntensityMeanCov {float, float}          */
  OHMHIP_LID_HIT_MISS = 7,   /* HitMissCount {u32, u32}                  */
  OHMHIP_LID_TSDF = 8,       /* VoxelTsdf {float weight, float distance} ohm/VoxelTsdfCompute.h:20-24 */
  OHMHIP_LID_CLEARANCE = 9,  /* float, clear -1; written by ohmhip_map_clearance_update* ohm/DefaultLayer.cpp:174-193 */
  OHMHIP_LID_COUNT = 10
};
#define OHMHIP_LAYER_BIT(id) (1u << (id))

/* Which update rule integrateRays applies: GpuMap / GpuNdtMap / GpuTsdfMap. */
enum ohmhip_map_mode
{
  OHMHIP_MODE_OCCUPANCY = 0, /* ohmgpu/GpuMap.h:143     (CPU semantics: ohm/RayMapperOccupancy.cpp:68-339) */
  OHMHIP_MODE_NDT_OM = 1,    /* ohmgpu/GpuNdtMap.h:63   (ohm/RayMapperNdt.cpp:84-407, NdtMode::kOccupancy)  */
  OHMHIP_MODE_NDT_TM = 2,    /* NdtMode::kTraversability                                                   */
  OHMHIP_MODE_TSDF = 3       /* ohmgpu/GpuTsdfMap.h:37  (ohm/RayMapperTsdf.cpp:87-182)                      */
};

/* Ray flags, bit-compatible with ohm::RayFlag (ohm/RayFlag.h:16-60). */
#define OHMHIP_RF_DEFAULT 0u
#define OHMHIP_RF_END_POINT_AS_FREE (1u << 0)
#define OHMHIP_RF_STOP_ON_FIRST_OCCUPIED (1u << 1) /* exact, via per-ray stop iteration over the sorted visits of the
                                                      batch (slow path); also with a traversal layer */
#define OHMHIP_RF_EXCLUDE_ORIGIN (1u << 2)
#define OHMHIP_RF_EXCLUDE_SAMPLE (1u << 3)
#define OHMHIP_RF_EXCLUDE_RAY (1u << 4)
#define OHMHIP_RF_EXCLUDE_UNOBSERVED (1u << 5)
#define OHMHIP_RF_EXCLUDE_FREE (1u << 6)
#define OHMHIP_RF_EXCLUDE_OCCUPIED (1u << 7)
#define OHMHIP_RF_REVERSE_WALK (1u << 8) /* accepted and ignored: results follow the CPU forward walk */

/* Ray filter applied on device before integration (ohm/RayFilter.cpp:12-58; map default = good rays <= 1e10,
 * ohm/OccupancyMap.cpp:215-218). */
enum ohmhip_ray_filter
{
  OHMHIP_FILTER_NONE = 0,
  OHMHIP_FILTER_GOOD = 1,
  OHMHIP_FILTER_CLIP = 2
};

typedef struct ohmhip_map_config
{
  double resolution;          /* OccupancyMap::resolution()                              */
  int region_dim[3];          /* OccupancyMap::regionVoxelDimensions(); 0 => 32          */
  double origin[3];           /* OccupancyMap::origin()                                  */
  unsigned layers;            /* OHMHIP_LAYER_BIT mask                                   */
  int mode;                   /* ohmhip_map_mode                                         */
  float hit_value;            /* OccupancyMap::hitValue()   (log odds)                   */
  float miss_value;           /* OccupancyMap::missValue()                               */
  float threshold_value;      /* OccupancyMap::occupancyThresholdValue()                 */
  float min_value, max_value; /* OccupancyMap::min/maxVoxelValue()                       */
  int saturate_at_min, saturate_at_max;
  int ray_filter;             /* ohmhip_ray_filter                                       */
  double ray_filter_range;
  /* NDT (ohm/private/NdtMapDetail.h:20-45) */
  float ndt_sensor_noise;
  unsigned ndt_sample_threshold;
  float ndt_adaptation_rate;
  float ndt_reinit_threshold;
  unsigned ndt_reinit_count;
  float ndt_initial_intensity_cov;
  /* TSDF (ohm/VoxelTsdf.h:27-37) */
  float tsdf_max_weight, tsdf_trunc, tsdf_dropoff, tsdf_sparsity;
  /* Residency: the whole map lives in HBM.  region_capacity regions are preallocated per layer (0 => derived from
   * gpu_mem_size, itself defaulting to 4 GiB; cf. GpuCache default 1 GiB, ohmgpu/GpuCache.h:90). The pool grows by
   * doubling when exhausted. */
  uint64_t gpu_mem_size;
  uint32_t region_capacity;
} ohmhip_map_config;

typedef struct ohmhip_map_s *ohmhip_map_t;

/* Timing / accounting of the most recent integrate call (device side measured with hipEvents on the map's stream). */
typedef struct ohmhip_batch_stats
{
  uint64_t rays_in;          /* rays submitted                                                           */
  uint64_t rays_integrated;  /* rays that passed the filter                                              */
  uint64_t voxel_visits;     /* exact count of miss visits + sample updates (== CPU walk visit count)    */
  uint64_t ray_region_segments;
  uint32_t regions_touched;
  uint32_t regions_resident;
  float ms_total;            /* first kernel start -> last kernel end                                    */
  float ms_setup;            /* ray setup + region binning                                               */
  float ms_walk;             /* the region line-walk kernel (dominant)                                   */
  float ms_apply;            /* hit sort + ordered apply                                                 */
} ohmhip_batch_stats;

/* LARGE REGIONS.  region_dim takes what the reference takes: any 1..255 voxels per axis (ohm/OccupancyMap.h:287,
 * glm::u8vec3; default 32^3, :24-26).  A region of up to 32768 voxels is one LDS tile of the walk kernel.  A larger one
 * is cut, inside the library, into equal tiles that each are one contiguous piece of the region's MapChunk block -- z
 * slabs of whole x-y layers (64^3 -> 8 tiles of 64 x 64 x 8), or, when one layer alone exceeds a tile, y strips of single
 * layers (255 x 255 x n -> 255 x 85 x 1) -- and everything internal works per tile.  The ABI keeps speaking REGIONS:
 * keys, listings, dirty sets and the blocks of read_regions / write_regions are the caller's regions (a tile no ray has
 * reached reads as cleared), results are those of the CPU mappers run with the same region size.  What counts tiles
 * instead: ohmhip_batch_stats::regions_touched / regions_resident, ohmhip_cache_stats, the memory limit's granule.
 * Not available for such maps (OHMHIP_ERR_UNSUPPORTED): the slot-level plumbing ohmhip_map_region_slot /
 * _ensure_regions / the replica merge -- the partitioned map works.  One limit: tile coordinates (region coordinate x
 * tiles per region on that axis) share the packed key's 16-bit fields, so with t tiles per region along an axis only
 * region coordinates within +-32767 / t are addressable there (64^3 at 0.1 m: +-26 km in z); rays beyond are rejected by
 * the key test like rays beyond the reference's own int16 region range. */
void ohmhip_map_config_default(ohmhip_map_config *config); /* reference defaults, ohm/OccupancyMap.cpp:192-223 */
int ohmhip_map_create(ohmhip_map_t *map, const ohmhip_map_config *config); /* GpuMap ctor + gpumap::enableGpu,
                                                                              ohmgpu/GpuMap.cpp:272, 106-122 */
int ohmhip_map_destroy(ohmhip_map_t map);
/* The reference GpuMap reads the OccupancyMap's probabilities, clamps and NDT / TSDF parameters at every launch
 * (ohmgpu/GpuMap.cpp:1036-1191, GpuNdtMap.cpp:289-503), so setters called on the map after the GpuMap exists take
 * effect from the next batch.  Same here: pass the configuration again; resolution, region dimensions, origin, mode and
 * layer set must equal those of creation (OHMHIP_ERR_INVALID_ARG otherwise), everything else applies to batches
 * presented afterwards.  One exception: the TSDF truncation distance of a map that already holds regions cannot
 * change (OHMHIP_ERR_UNSUPPORTED; free-space TSDF updates are exact only against one truncation distance).  A change of
 * the TSDF max_weight or dropoff_epsilon is accepted, as in the reference, and costs one pass over the map's TSDF layer:
 * which voxels may take free-space visits as counts is re-derived from what the earlier options left in them. */
int ohmhip_map_update_config(ohmhip_map_t map, const ohmhip_map_config *config);

/* GpuMap::integrateRays (ohmgpu/GpuMap.cpp:416, 540-875): rays = element_count dvec3 (origin, sample pairs).
 * Host-pointer form stages through one of two pinned blocks and uploads on a side stream, so batch N+1 is copied while
 * batch N runs; returns after enqueue (like the reference the call is asynchronous; ohmhip_map_sync / any read is
 * the fence).  *integrated = points accepted (2 per ray). */
int ohmhip_map_integrate_rays(ohmhip_map_t map, const double *rays, size_t element_count, const float *intensities,
                              const double *timestamps, unsigned ray_flags, size_t *integrated);
/* GpuMap::setRayFilter with an arbitrary RayFilterFunction (ohm/RayFilter.h:45, ohmgpu/GpuMap.cpp:348-369; applied
 * per ray on the host at GpuMap.cpp:736-746).  The filter is host code, so the host mirror runs it and hands over what
 * passed: `rays` holds the accepted (possibly moved) origin / sample pairs and filter_flags[ray] the RayFilterFlag bits
 * the filter set (ohm/RayFilter.h:21-29: 1 invalid, 2 clipped start, 4 clipped end).  The map's built-in filter is not applied to
 * such a batch; a clipped end makes the end voxel part of the ray and suppresses the sample, as in the CPU mappers
 * (ohm/RayMapperOccupancy.cpp:209-223, ohm/RayMapperNdt.cpp:251-269).  Hand over accepted rays only: a ray whose flags
 * carry kRffInvalid is neither integrated nor counted in *integrated. */
int ohmhip_map_integrate_rays_filtered(ohmhip_map_t map, const double *rays, size_t element_count,
                                       const float *intensities, const double *timestamps, unsigned ray_flags,
                                       const unsigned char *filter_flags, size_t *integrated);
/* GpuMap::setRayFilter with the STOCK filters of ohm/RayFilter.cpp, evaluated on the device: a chain of up to
 * OHMHIP_MAX_RAY_FILTER_STAGES stages the map owns.  While a chain is set it stands in place of the built-in filter
 * (ohmhip_map_config::ray_filter) for every batch the map integrates -- host pointers, device pointers, collected calls,
 * ohmhip_map_apply_pattern -- as GpuMap::effectiveRayFilter does (ohmgpu/GpuMap.cpp:348-369, 736-746); batches of
 * ohmhip_map_integrate_rays_filtered are the caller's and are not filtered again; ohmhip_map_rays_query and
 * ohmhip_map_line_keys keep the built-in filter (the reference reads OccupancyMap::rayFilter() there).
 *   GOOD            goodRayFilter(range)   RayFilter.cpp:12-34     range <= 0: no range test
 *   CLIP            clipRayFilter(range)   RayFilter.cpp:37-57
 *   CLIP_BOUNDED    clipBounded(box)       RayFilter.cpp:60-77, Aabb::clipLine / rayIntersect / contains (ohm/Aabb.h)
 *   CLIP_TO_BOUNDS  clipToBounds(box)      RayFilter.cpp:80-86
 * Stage i sees the ray as stage i - 1 left it, RayFilterFlag bits are OR-ed, the first stage that returns false ends the
 * chain (`a(...) && b(...)` in a lambda).  A rejected ray counts as not integrated; kRffClippedEnd makes the end voxel
 * part of the ray and suppresses the sample, as for a caller-filtered batch.  Aabb::contains is the reference's
 * `!any(max < p) && !any(min > p)`: a NaN coordinate counts as contained.  NaN in `range` or a box is accepted (the
 * reference has no check; its comparisons decide).  The time base of the touch-time layer still comes from the first
 * stamp of the call as submitted.  The caller's arrays are never written: moved rays live in scratch of the map's.
 * set: count == 0 clears the chain.  OHMHIP_ERR_INVALID_ARG for a kind outside 1..4, count above the maximum, NULL
 * stages with count > 0, a non-zero `reserved`.  Rays waiting in the coalescing buffer are launched first, so calls that
 * reported a count were filtered by the chain that counted them.  Not available on a partitioned / owner-computes map
 * (OHMHIP_ERR_UNSUPPORTED, whichever is set second): routed rays would be filtered twice. */
enum ohmhip_ray_filter_stage_kind
{
  OHMHIP_RFS_GOOD = 1,
  OHMHIP_RFS_CLIP = 2,
  OHMHIP_RFS_CLIP_BOUNDED = 3,
  OHMHIP_RFS_CLIP_TO_BOUNDS = 4
};
#define OHMHIP_MAX_RAY_FILTER_STAGES 4
typedef struct ohmhip_ray_filter_stage
{
  int kind;          /* ohmhip_ray_filter_stage_kind */
  int reserved;      /* 0 */
  double range;      /* GOOD, CLIP */
  double box_min[3]; /* CLIP_BOUNDED, CLIP_TO_BOUNDS */
  double box_max[3];
} ohmhip_ray_filter_stage;
int ohmhip_map_set_ray_filter_stages(ohmhip_map_t map, const ohmhip_ray_filter_stage *stages, unsigned count);
/* The chain as set: *count stages (0: none), the first min(*count, capacity) of them in `out` (may be NULL). */
int ohmhip_map_ray_filter_stages(ohmhip_map_t map, ohmhip_ray_filter_stage *out, unsigned capacity, unsigned *count);
/* What the chain does to a batch, without touching the map: for EVERY input ray the ray as the chain leaves it
 * (rays_out, element_count dvec3) and its RayFilterFlag byte (flags_out, one per ray; a rejected ray carries
 * kRffInvalid = 1 and the points as the rejecting stage left them); *passed = rays kept.  Runs the device pass.  With no
 * chain set rays come back as given, flags 0.  Outputs may be NULL.  The _device form takes device pointers. */
int ohmhip_map_apply_ray_filter(ohmhip_map_t map, const double *rays, size_t element_count, double *rays_out,
                                unsigned char *flags_out, size_t *passed);
int ohmhip_map_apply_ray_filter_device(ohmhip_map_t map, const double *d_rays, size_t element_count, double *d_rays_out,
                                       unsigned char *d_flags_out, size_t *passed);
/* Small host batches (the reference tools present 4096 rays per call, ohmapp/OhmAppGpu.cpp:187-207) would cost a full
 * pipeline pass each.  Consecutive host-pointer batches with the same flags and the same optional arrays are therefore
 * collected in the pinned staging block and run as ONE device batch once min_rays have accumulated -- or as soon as
 * anything observes the map (sync, stats, region reads, a device-pointer batch ...).  The result is the one the
 * separate calls give: the CPU mappers integrate ray by ray, so call boundaries carry no meaning, except for the
 * traversal layer (its exit range is carried within a call): maps with that layer never merge batches.  Every call
 * still reports its own *integrated: the ray filter's verdict is evaluated on the host while the rays are staged, with
 * the arithmetic the device uses.  An error of a deferred batch (pool exhausted ...) surfaces at the call that launches
 * it.  Default min_rays: 65536; 0 launches every call's batch in that call. */
OHMHIP_EXPERIMENTAL int ohmhip_map_set_batch_coalescing(ohmhip_map_t map, size_t min_rays);
/* Large host batches, opt-in: with enable != 0 a host-pointer call that is a device batch on its own returns as soon
 * as its rays are staged and their upload is queued; the device launch sequence -- which waits for the batch's plan
 * summary in its middle -- runs on a thread the map owns, so the caller stages its next block, and the link carries it,
 * beside that wait (1 M-ray calls: 1.4 -> ~1.1 ms).  The reference's GpuMap::integrateRays returns with
 * its GPU work in flight in the same way (ohmgpu/GpuMap.cpp:874).  What changes for the caller: *integrated is the
 * host's evaluation of the ray filter (the same verdict), and an error of the batch (OHMHIP_ERR_CAPACITY ...) is
 * returned by the NEXT call on the map that settles it -- any entry point but the staging part of integrate_rays; the
 * rays of the call that reports it stay queued.  Everything that observes the map waits for the launch first, so
 * results do not depend on the setting.  Default: off. */
OHMHIP_EXPERIMENTAL int ohmhip_map_set_async_launch(ohmhip_map_t map, int enable);
/* Same with rays (and optional intensities/timestamps) already resident in device memory.  The arrays must be COMPLETE
 * when the call is made (not merely enqueued on some stream): the map reads them on streams of its own.  Calls below
 * the coalescing threshold are collected like small host batches (round 3): their arrays are copied device to device
 * behind the rays already waiting and run as one batch once min_rays have accumulated or anything observes the map.
 * With `integrated` non-NULL the call waits for that copy (it reports its own count from a filter pass over the copy),
 * so the caller's arrays are free when it returns; with NULL they must stay valid until the next ohmhip_map_sync.
 * A call at or above the threshold is a device batch of its own and returns with that batch IN FLIGHT (its kernels read
 * the arrays until it ends).  At most two batches are in flight: when any integrate call returns, every batch but the
 * two launched last has completed (the map double-buffers its per-batch scratch and the set-up pass of a batch waits for
 * the one before the previous).  So the arrays of a batch may be reused once two further batches have been LAUNCHED and
 * the call that launched the second has returned -- three buffers used in turn, advanced per launch
 * (ohmhip_map_batches_launched; a call that launches nothing must not advance the turn), never need a sync
 * (ohm_amd/distributed.py, PartitionedIntegrator) -- or after ohmhip_map_sync. */
int ohmhip_map_integrate_rays_device(ohmhip_map_t map, const double *d_rays, size_t element_count,
                                     const float *d_intensities, const double *d_timestamps, unsigned ray_flags,
                                     size_t *integrated);
/* Residency accounting, the counterpart of ohm::GpuCacheStats (ohmgpu/GpuCacheStats.h, GpuLayerCache::queryStats,
 * ohmgpu/GpuLayerCache.h:334-339).  The whole map is resident, so the figures read: hits = regions a batch touched that
 * were resident already, misses = regions a batch (or an upload) created, full = times the pool was exhausted and had to
 * be re-allocated at twice the size (the reference evicts its least recently used region instead,
 * ohmgpu/GpuLayerCache.cpp:530-584).  Cumulative since creation or the last reset. */
typedef struct ohmhip_cache_stats
{
  uint64_t hits;
  uint64_t misses;
  uint64_t full;
  uint32_t regions_resident;
  uint32_t region_capacity;   /* regions the pool holds without growing                                   */
  uint64_t bytes_per_region;  /* all enabled layers + per-region scratch                                    */
  uint64_t memory_limit;      /* see ohmhip_map_set_memory_limit (0 = device memory is the limit)           */
  uint64_t evictions;         /* regions moved to the host store (ohmhip_map_set_spill_to_host)             */
  uint64_t readmissions;      /* regions brought back from it                                               */
  uint32_t regions_spilled;   /* regions in the host store right now                                        */
  uint32_t spill_enabled;
  uint64_t writebacks;        /* regions copied to the store in the background, ahead of their eviction     */
  uint64_t writeback_hits;    /* evictions that found their region clean (no copy-out on the batch's path)   */
  uint64_t writeback_stale;   /* background copies discarded because a batch touched the region afterwards  */
} ohmhip_cache_stats;
int ohmhip_map_cache_stats(ohmhip_map_t map, ohmhip_cache_stats *stats, int reset);
/* RESIDENCY LIMIT.  Without spilling (below) a map that outgrows what it may allocate fails the batch that needs the
 * extra regions with OHMHIP_ERR_CAPACITY and stays exactly as it was before that batch (the batch's region inserts are
 * rolled back; this holds for pool / chunk-list EXHAUSTION, the failure a caller can act on -- a batch that dies later
 * of a device error or a failed buffer allocation may leave regions it touched flagged as modified, which costs a
 * redundant copy at the next syncVoxels(), never a wrong value), so the caller can cull regions (ohmhip_map_remove_regions after reading them back) and present the
 * batch again -- or turn on ohmhip_map_set_spill_to_host and let the library move cold regions to host memory.  The
 * limit is free device memory -- 288 GB of HBM3E hold about 1 million 32^3 occupancy-only regions (8.1 B per voxel
 * with scratch) -- or, when set, `bytes` for this map's region pool (the reference's gpu_mem_size,
 * ohmgpu/GpuCache.h:90, bounds its cache the same way).  0 removes the limit. */
int ohmhip_map_set_memory_limit(ohmhip_map_t map, uint64_t bytes);
/* SPILL TO HOST (off by default).  With it on, a batch that needs more regions than the memory limit (or the device)
 * allows no longer fails: resident regions -- a quarter of the pool at a time; those not expected back soon: least
 * recently used first, but a region that has been coming back every N batches is kept while its next use is near (a
 * sweep over a map larger than the pool would otherwise lose every region once per revolution); the counterpart of
 * the reference's LRU slot reuse, ohmgpu/GpuLayerCache.cpp:530-584 -- are copied to a host store inside the
 * library and dropped from the pool, and the batch is repeated.  A stored region stays part of the map: it is listed by
 * ohmhip_map_regions / _region_count / _dirty_regions, ohmhip_map_read_regions serves it from the store, and it returns
 * to the pool with its content when a later batch reaches it or an upload / ohmhip_map_ensure_regions names it.  Results
 * are those of an unbounded pool.  WRITE-BACK: once the pool is under pressure the regions the policy would evict next
 * are copied to the store in the background, on the copy stream while batches run, so that an eviction finds them
 * clean and only drops them (the reference overlaps the download of the cache slot it reuses with queued work the same
 * way, ohmgpu/GpuLayerCache.cpp:550-584); a copy is discarded if a batch touches its region afterwards
 * (ohmhip_cache_stats::writebacks / writeback_hits / writeback_stale).  What does not combine with it: replica merge (OHMHIP_ERR_UNSUPPORTED either way
 * round) and the zero-copy views (ohmhip_map_region_slot reports OHMHIP_ERR_NOT_FOUND for a stored region).  A batch
 * that alone touches more regions than the limit allows is integrated as two halves in ray order (and those again, down
 * to single rays: the reference finalises what it has enqueued when its cache fills in the middle of a batch and carries
 * on, ohmgpu/GpuMap.cpp:900-996; results are those of the whole batch -- except on maps with a traversal layer, whose
 * exit range is carried within a call: there the call fails with OHMHIP_ERR_CAPACITY and changes nothing.  When a LATER
 * half -- in the end a single ray -- still does not fit, the call returns OHMHIP_ERR_CAPACITY with the halves before it
 * applied: `*integrated` then counts the leading elements that were integrated and must not be presented again; the
 * host mirrors put that count into the exception they raise).  Only this cause splits a batch: a full hash, a refused
 * allocation or the end of the slot field fail at once and change nothing.  Turning spilling on sets the batch coalescing threshold to 0 (a collected
 * batch touches the regions of all its calls at once). */
int ohmhip_map_set_spill_to_host(ohmhip_map_t map, int enable);
/* The background write-back of the spill path (see WRITE-BACK above), opt-in: off by default. */
OHMHIP_EXPERIMENTAL int ohmhip_map_set_spill_writeback(ohmhip_map_t map, int enable);
/* Wait for all queued work (GpuMap::syncVoxels fence half, ohmgpu/GpuMap.cpp:308-324). */
int ohmhip_map_sync(ohmhip_map_t map);
int ohmhip_map_last_stats(ohmhip_map_t map, ohmhip_batch_stats *stats);

/* Device phase times of one of the last 32 batches (batches_back = 0: the latest): ms[0] the device time the batch cost
 * -- first kernel start -> last kernel end, or, for batches that overlapped (this batch's plan had ended before the
 * previous batch's last kernel did), the interval between the previous batch's last kernel and this one's (a batch's
 * set-up pass runs on a second stream under the previous batch's last kernels); a batch presented after the device went
 * idle keeps its own span, host idle time between batches is never counted --, ms[1] ray setup + binning (the set-up pass is timed from the moment it may start: queued behind a running
 * walk kernel it mostly waits for CUs), ms[2] the region walk kernel, ms[3] sample ordering + ordered apply.
 * hipEvents on the map's streams (the gputil::Event / Queue::mark() bookkeeping of ohmgpu/GpuMap.cpp:1036-1191 serves
 * the same purpose); waits for that batch only.  Lets a caller time a run of batches without synchronising after each. */
OHMHIP_EXPERIMENTAL int ohmhip_map_batch_timings(ohmhip_map_t map, uint32_t batches_back, float ms[4]);
/* What the phase times are read from (round 5).  The end of a batch's binning, sample ordering, walk and apply phases and
 * of its plan are the STOP EVENTS of the kernels themselves (hipExtLaunchKernelGGL: bound to the kernel's completion
 * signal, free), so ms[0] (as the interval between consecutive batches' ends; for a batch on its own: plan end -> batch
 * end), ms[2] (end of the kernel before the walk -> end of the walk kernel, on the stream it runs on) and ms[3] are
 * always available.  The START of the set-up pass and of the binning pass have no kernel in front of them to carry an
 * event: they are hipEventRecord markers, and a marker idles the queue for 3-7 us before the next kernel
 * (scripts/probes/event_probe.hip) -- round 4 paid eight of them per batch, 5 % of a C1 batch.  They are therefore
 * recorded only with phase timing on (this call, OHMHIP_PHASE_TIMING=1): ms[1], and ms[0] of a batch on its own as first
 * kernel start -> last kernel end, need it and read 0 / the shorter span otherwise.  Default: off. */
OHMHIP_EXPERIMENTAL int ohmhip_map_set_phase_timing(ohmhip_map_t map, int enable);
/* The per-batch device buffers (ray set-up records, ray-region segments, sample keys, sort scratch) are grown by the
 * batch that first needs them -- a few hipMalloc calls, each a device synchronisation, inside that call.  The reference's
 * GpuMap constructor sizes its key / ray buffers for `expected_element_count` up front (ohmgpu/GpuMap.cpp:429-470); this is
 * the counterpart: size everything a batch of `ray_count` rays needs now (the deferred-event list: 16 per ray, at most
 * 2^27 events).  Optional; batches of any size still work, and the host mirrors treat a failing reservation as "grow on
 * demand", not as an error. */
OHMHIP_EXPERIMENTAL int ohmhip_map_reserve_rays(ohmhip_map_t map, size_t ray_count);
/* OccupancyMap::firstRayTime / setFirstRayTime (ohm/OccupancyMap.h:342-351): the time base the touch-time layer is
 * encoded against (milliseconds since it, ohm/VoxelTouchTimeCompute.h:24-37).  Like the reference the map takes it from
 * the first time stamp it is ever given; set it explicitly where that is not the map's to decide -- the ranks of a
 * partitioned map must share ONE base (the first stamp of the whole job), not each the first stamp that happens to be
 * routed to it.  A negative value means "not set yet".
 * CONTRACT for stamps outside [base, base + 2^32 ms): the touch time is (stamp - base) / 0.001 truncated toward zero to
 * a 64-bit integer, of which the low 32 bits are kept -- 5 s before the base reads 4294962296, 5e6 s after it 705032704.
 * That is what the reference's x86-64 build yields for a cast C leaves undefined; a quotient that does not fit 64 bits,
 * or NaN, gives 0.  A map whose first stamp is not its earliest therefore holds wrapped, not clamped, touch times.
 * A host mirror that filters rays before the library sees them (GpuMap::setRayFilter) sets the base from the first stamp
 * of the call as submitted, as the reference does, not from the first ray that survives the filter. */
int ohmhip_map_set_first_ray_time(ohmhip_map_t map, double time);
int ohmhip_map_first_ray_time(ohmhip_map_t map, double *time);
/* Device batches the map has launched since it was created.  An integrate call that only collects its rays (batch
 * coalescing) or is rejected launches none: callers that recycle device ray buffers by the "two batches in flight" rule
 * of ohmhip_map_integrate_rays_device count LAUNCHES with this, not calls -- a buffer handed to the call that made the
 * count L is free once the count has reached L + 2 and a later integrate call has returned (or after ohmhip_map_sync).
 * Does not flush collected rays. */
OHMHIP_EXPERIMENTAL int ohmhip_map_batches_launched(ohmhip_map_t map, uint64_t *count);
/* Which route the map's device batches took through the launch pipeline, since the map was created: *batches = batches
 * completed, *binned_early = those whose binning pass ran on the front stream beside the previous batch's apply kernels
 * and stood (a plain occupancy batch that follows one, with OHMHIP_EARLY_BIN=1 in the environment at map creation -- off by default; a pass repeated after a wrong guess does
 * not count).  Read only: it changes nothing and does not flush collected rays.  For tests and measurements, so that a
 * fallback to the compute stream cannot pass for the early route. */
OHMHIP_EXPERIMENTAL int ohmhip_map_pipeline_counts(ohmhip_map_t map, uint64_t *batches, uint64_t *binned_early);
/* How the per-region ordering step of plain occupancy batches ordered its regions, since the map was created:
 * *regions_ranked = regions placed by bucket and ranked inside their buckets, *regions_network = regions whose buckets
 * were too crowded for that and that ran the bitonic network.  One count per region and launch that ordered it: a
 * speculated pass that is dropped and repeated counts twice; regions that go through the device-wide sort (more than
 * 8192 samples in one region) are not counted.  Counted on the device: waits for the batches launched so far, does not
 * flush collected rays.  For tests and measurements, so that one path cannot pass for the other. */
OHMHIP_EXPERIMENTAL int ohmhip_map_order_counts(ohmhip_map_t map, uint64_t *regions_ranked, uint64_t *regions_network);
/* Maps whose regions are cut into tiles (LARGE REGIONS above): rays, among those that passed the filter, with an end in
 * a region the reference still addresses (|region| <= 32767) but whose tile coordinates leave the key's 16-bit fields.
 * Such a ray is not walked and, when it is the sample that lies out there, its sample is dropped -- the one place results
 * differ from the CPU mappers run with the same region size; this count (since the map was created, rejected batches
 * excluded) lets a caller see that it happened.  Always 0 for regions of up to 32768 voxels.  Flushes collected rays. */
OHMHIP_EXPERIMENTAL int ohmhip_map_rays_beyond_tiles(ohmhip_map_t map, uint64_t *count);

/* Region table (replaces GpuLayerCache::lookup, ohmgpu/GpuLayerCache.cpp:104-119). keys = int16 xyz triples. */
int ohmhip_map_region_count(ohmhip_map_t map, size_t *count);
int ohmhip_map_regions(ohmhip_map_t map, int16_t *keys_xyz, size_t capacity, size_t *count);
/* Regions modified on device since the last ohmhip_map_clear_dirty (dirty-region tracking for syncVoxels). */
int ohmhip_map_dirty_regions(ohmhip_map_t map, int16_t *keys_xyz, size_t capacity, size_t *count);
int ohmhip_map_clear_dirty(ohmhip_map_t map);
size_t ohmhip_layer_voxel_bytes(int layer_id);

/* GpuLayerCache::syncToMainMemory (ohmgpu/GpuLayerCache.cpp:300-321, 670-696): copy `count` regions' layer blocks
 * into dsts[i] (each region_voxels * voxel_bytes, MapChunk layout x + y*dx + z*dx*dy, ohm/MapChunk.h:33-50).
 * Pinned staging + hipMemcpyAsync on the copy stream. */
int ohmhip_map_read_regions(ohmhip_map_t map, int layer_id, const int16_t *keys_xyz, size_t count, void *const *dsts);
/* GpuLayerCache::upload (ohmgpu/GpuLayerCache.cpp:172-182): make CPU-side voxel blocks resident (creates regions). */
int ohmhip_map_write_regions(ohmhip_map_t map, int layer_id, const int16_t *keys_xyz, size_t count,
                             const void *const *srcs);
/* GpuCache::clear (ohmgpu/GpuCache.cpp, ohm/MapRegionCache.h): drop all regions. */
int ohmhip_map_clear(ohmhip_map_t map);
/* MapRegionCache::remove as the core map calls it when it drops regions (OccupancyMap::cullRegions ->
 * gpu_cache->remove, ohm/OccupancyMap.cpp:1202-1234; GpuLayerCache::remove, ohmgpu/GpuLayerCache.cpp): the listed
 * regions leave the device map (their voxels are discarded, modified or not -- sync first to keep them); unknown keys
 * are ignored.  *removed = regions actually dropped. */
int ohmhip_map_remove_regions(ohmhip_map_t map, const int16_t *keys_xyz, size_t count, size_t *removed);

/* LineKeysQueryGpu / `calculateLines` (ohmgpu/LineKeysQueryGpu.cpp, ohmgpu/gpu/LineKeys.cl:66-100): the voxel keys on
 * `line_count` query lines (6 doubles each: start, end), in walk order, with the CPU walk's fp64 semantics.  keys_out is
 * line_count * max_keys_per_line records in the reference's GpuKey layout (short region[3]; uchar voxel[4], 10 bytes,
 * ohmgpu/GpuKey.h:37-46); counts_out[i] is the line's total voxel count.  Host pointers; synchronous. */
int ohmhip_map_line_keys(ohmhip_map_t map, const double *lines, size_t line_count, uint32_t max_keys_per_line,
                         void *keys_out, uint32_t *counts_out);

/* RaysQuery / RaysQueryGpu (ohm/RaysQuery.{h,cpp}, ohmgpu/RaysQueryGpu.{h,cpp}; reference kernel raysQuery,
 * ohmgpu/gpu/RaysQuery.cl:193): for each ray (origin, end point: 6 doubles) of `element_count` points -- an odd trailing
 * point is not a ray, as in ohmhip_map_integrate_rays -- the CPU query of ohm/RaysQuery.cpp:102-203 as written, bit for
 * bit: the map's own ray filter (OHMHIP_FILTER_*, map->rayFilter(), :118), then walkSegmentKeys with flags 0 (start and
 * end voxel visited, fp64, ohm/LineWalk.h:112-129), stopping after the first voxel whose value is > threshold_value
 * (strict: the reference's GPU kernel uses >=, RaysQuery.cl:111).  Per ray: ranges[i] = float(exit range) of the last
 * voxel that is not occupied, widened to double (RaysQuery::ranges()); unobserved_volumes[i] = the sum of
 * volume_coefficient * (exit^3 - enter^3) over the unobserved (+inf) voxels, in walk order; terminal_types[i] =
 * ohm::OccupancyType of the last visited voxel (kNull -2, kUnobserved -1, kFree 0, kOccupied 1); terminal_keys (nullable)
 * = its key (Query::intersectedVoxels()) in the 10-byte GpuKey layout of ohmhip_map_line_keys, in the caller's region
 * coordinates.  A filtered ray reports 0, 0, kNull, Key::kNull.  Reference behaviour kept: the CPU declares the terminal
 * type and key outside its ray loop (:116-117), so a ray that passes the filter but visits no voxel (a null start or end
 * key) repeats the type and key of the last preceding ray that did (kNull / Key::kNull before any).
 * The query observes the map as ohmhip_map_read_regions would -- collected rays launched, an asynchronous launch settled,
 * regions of the host store (spill to host) included -- and changes nothing of it: voxels, dirty set, residency, use
 * stamps, ohmhip_map_cache_stats; it uses buffers of its own.  OHMHIP_ERR_UNSUPPORTED for a map without the occupancy
 * layer (the CPU query refuses it: valid_layers) and for a map with region ownership / a partition (a rank holds only its
 * territory); OHMHIP_ERR_INVALID_ARG for null arrays, checked before any device work.  Host pointers; synchronous. */
int ohmhip_map_rays_query(ohmhip_map_t map, const double *rays, size_t element_count, double volume_coefficient,
                          double *ranges, double *unobserved_volumes, int8_t *terminal_types, void *terminal_keys);
/* ohmhip_map_rays_query on DEVICE arrays (e.g. the output of ohmhip_transform_samples): enqueued on the map's stream,
 * ohmhip_map_sync is the fence.  The rays must stay valid, and the outputs unread, until then. */
OHMHIP_EXPERIMENTAL int ohmhip_map_rays_query_device(ohmhip_map_t map, const double *d_rays, size_t element_count,
                                                     double volume_coefficient, double *d_ranges,
                                                     double *d_unobserved_volumes, int8_t *d_terminal_types,
                                                     void *d_terminal_keys);

/* ClearanceProcess / LineQueryGpu (ohmgpu/ClearanceProcess.{h,cpp}, ohmgpu/LineQueryGpu.{h,cpp}): the clearance of a voxel
 * v is the CPU's calculateNearestNeighbour(v, map, h, unknown_as_occupied, ignore_self = false, search_radius,
 * axis_scaling, report_unscaled) (ohm/private/VoxelAlgorithms.cpp:22-98) as written, bit for bit -- not the
 * reference's approximate GPU flood fill (gpu/RoiRangeFill.cl).  h = int(ceil(double(search_radius) / resolution)) on
 * every axis (calculateVoxelSearchHalfExtents, :16).  A voxel is a candidate when its region exists and value != +inf
 * && value >= threshold_value (isOccupied, ohm/VoxelOccupancy.h:161: `>=`, unlike the rays query's `>`), or, with
 * OHMHIP_QF_UNKNOWN_AS_OCCUPIED, when it is unobserved (+inf) or in no region (isUnobservedOrNull).  v itself a
 * candidate: 0.  Otherwise the neighbours moveKey(v, x, y, z) for x, y, z in [-h, h] (the region key adds in int16 and
 * wraps, ohm/private/OccupancyMapDetail.cpp:27-93), all fp32 with rounding after every operation:
 * c(k) = float(voxelCentreLocal(k)) (fp64 in the order of OccupancyMap::voxelCentre, ohm/OccupancyMap.h:757-777);
 * sep = c(n) - c(v); r2 = (sep.x*sep.x + sep.y*sep.y) + sep.z*sep.z; s = sep * axis_scaling per component; s2 the same
 * dot product of s; r2 = s2 unless OHMHIP_QF_REPORT_UNSCALED; a candidate counts when search_radius == 0 ||
 * r2 <= search_radius * search_radius and is taken when s2 is smaller than the best so far -- strictly, so ties go to
 * the earliest in the CPU's scan order (z outermost, x innermost; the device selects by (s2, scan index)).  Result:
 * sqrtf(r2 of the one taken), -1 when none.
 * The map is observed as ohmhip_map_rays_query observes it -- collected rays launched, an asynchronous launch settled,
 * resident tiles through the region hash, regions of the host store from their pinned records without re-admission,
 * tiled regions in the caller's region coordinates -- and nothing of it changes: voxels, dirty set, residency, use
 * stamps, ohmhip_map_cache_stats.  Results go to the caller's memory, as the reference's RoiRangeFill::finishRegion
 * downloads each region's block (ohmhip_map_clearance_update below keeps the map's own clearance layer).
 * OHMHIP_ERR_UNSUPPORTED for a map without the occupancy layer, a map with region ownership or a partition, and h > 127;
 * OHMHIP_ERR_INVALID_ARG, before any device work, for null arrays, a negative or non-finite search_radius and a zero or
 * non-finite axis_scaling component. */
#define OHMHIP_QF_UNKNOWN_AS_OCCUPIED (1u << 0) /* ohm::kQfUnknownAsOccupied (ohm/QueryFlag.h:38) */
#define OHMHIP_QF_REPORT_UNSCALED (1u << 4)     /* ohm::kQfReportUnscaledResults (:50); other QueryFlag bits ignored */
typedef struct ohmhip_clearance_params
{
  float search_radius;
  float axis_scaling[3];
  unsigned flags; /* OHMHIP_QF_* */
} ohmhip_clearance_params;

/* ClearanceProcess::calculateForExtents per region: every voxel of each listed region (present in the map or not),
 * MapChunk order x + y*dx + z*dx*dy, one float per voxel -- dsts[i] as in ohmhip_map_read_regions.  Host pointers;
 * synchronous. */
int ohmhip_map_clearance_regions(ohmhip_map_t map, const int16_t *keys_xyz, size_t count,
                                 const ohmhip_clearance_params *params, float *const *dsts);
/* The same into one device array of count * region_voxels floats, enqueued on the map's stream (keys_xyz is a host
 * array of count regions); ohmhip_map_sync is the fence. */
OHMHIP_EXPERIMENTAL int ohmhip_map_clearance_regions_device(ohmhip_map_t map, const int16_t *keys_xyz, size_t count,
                                                            const ohmhip_clearance_params *params, float *d_out);
/* Clearance of arbitrary voxels given as 10-byte GpuKey records (the layout ohmhip_map_line_keys writes), one float
 * each.  A key whose local coordinates lie outside the region dimensions: OHMHIP_ERR_INVALID_ARG.  Host pointers;
 * synchronous. */
int ohmhip_map_clearance_keys(ohmhip_map_t map, const void *keys, size_t count, const ohmhip_clearance_params *params,
                              float *out);

/* The clearance layer (OHMHIP_LID_CLEARANCE: a map gets it only with OHMHIP_LAYER_BIT(9) at ohmhip_map_create; float,
 * cleared to -1; integration never writes it) kept current, as ClearanceProcess::update keeps it in the reference
 * (ohmgpu/ClearanceProcess.cpp:418-470, 519-623).  Values are those of ohmhip_map_clearance_regions, bit for bit.
 * h = ceil(search_radius / resolution); D_a = ceil(h / region_dim_a).  A region present in the map (resident or in the
 * host store) is STALE for params when it was never written with them (new, last written with other parameters, or
 * its clearance layer written by the host), or when the occupancy of a region within D_a of it on every axis (keys
 * wrap in int16) changed, or such a region was removed (ohmhip_map_remove_regions), after it was last written.
 * Occupancy changes: integrated batches, ohmhip_map_write_regions of the occupancy layer, ohmhip_map_mark_dirty and the
 * replica merge -- conservatively: a batch that touches a region changes it.  Eviction and re-admission are not
 * changes.  (The reference pads by one region, the same as D = 1 while h <= region_dim, and misses dependencies beyond;
 * this does not.)  Stale regions are processed in ascending (z, y, x) signed key order.  The map is observed as the
 * clearance queries observe it; an update re-admits and evicts nothing, changes no use stamp or cache counter, writes
 * the new values of host-store regions into their records and gives each processed region the sync mark (not the merge
 * mark).  Tiles of a tiled region that hold no data are not created: they keep reading -1.  OHMHIP_ERR_UNSUPPORTED as
 * for the clearance queries, and for a map without the clearance layer; OHMHIP_ERR_INVALID_ARG, before any device
 * work, for null arrays and the parameters ohmhip_map_clearance_regions refuses.  Host pointers; synchronous. */
/* Stale regions for params, in processing order. *count = total; at most capacity written. */
int ohmhip_map_clearance_stale_regions(ohmhip_map_t map, const ohmhip_clearance_params *params, int16_t *keys_xyz,
                                       size_t capacity, size_t *count);
/* ClearanceProcess::update: bring up to max_regions (0 = all) stale regions up to date, the first in processing order.
 * processed / remaining (optional): regions written, stale regions left. */
int ohmhip_map_clearance_update(ohmhip_map_t map, const ohmhip_clearance_params *params, size_t max_regions,
                                size_t *processed, size_t *remaining);
/* calculateForExtents / updateRegion(force): the listed regions present in the map (absent ones are skipped, never
 * created); force = 0 skips up-to-date ones.  processed (optional): regions written. */
int ohmhip_map_clearance_update_regions(ohmhip_map_t map, const int16_t *keys_xyz, size_t count,
                                        const ohmhip_clearance_params *params, int force, size_t *processed);

/* HEIGHTMAP.  The planar heightmap of ohm::Heightmap::buildHeightmap (ohmheightmap/Heightmap.cpp:335-412, HeightmapMode::
 * kPlanar, the class default: private/HeightmapDetail.h:68) computed on the device against the resident map, equal to
 * the CPU algorithm as written for every cell and every field.  The reference is CPU only.  In its order:
 *  1 EXTENTS (Heightmap.cpp:349-365).  calculateExtents of the source map (ohm/OccupancyMap.cpp:397-459): over the regions
 *    present -- resident or in the host store -- region.centre -+ 0.5 * regionSpatialResolution per axis in fp64, where
 *    region.centre = coord * regionSpatialResolution WITHOUT the map origin (ohm/MapRegion.cpp:32-43); an axis with
 *    cull_max - cull_min > 0 takes the cull box's min / max instead; min_ext_key / max_ext_key = voxelKey(min / max).
 *    The upper corner of the last region is a point of the next region: the walked range is one voxel wider than the
 *    data.  An empty map (or a null extents / reference key) builds nothing: *populated = 0, the arrays untouched.
 *  2 WALK (PlaneWalker.cpp:24-52).  (a, b, up) = heightmapAxisIndices(up_axis) (HeightmapUtil.cpp:86-116: X up (1, 2, 0),
 *    Y up (0, 2, 1), Z up (0, 1, 2); the negative axes the same indices with up = -e).  The plane is voxelKey(
 *    reference_pos)'s up coordinate clamped into [min_ext_key, max_ext_key].  Columns are visited with a innermost: the
 *    WALK INDEX of a column is ib * na + ia.
 *  3 SUPPORTING VOXEL (private/HeightmapOperations.cpp:186-419).  findNearestSupportingVoxel with kIgnoreVirtualAbove, plus
 *    kVirtualSurfaces / kPromoteVirtualBelow from the flags, never kBiasAbove; voxel_floor / voxel_ceiling =
 *    pointToRegionCoord(floor / ceiling, resolution) (0: unlimited); clearance_voxel_count_permissive = max(1,
 *    pointToRegionCoord(min_clearance, resolution) - 1).  findNearestSupportingVoxel2 as written: vertical_range =
 *    rangeBetween(seed, limit)[up] + 1, the step direction from ITS sign, the limit applied, then ++vertical_range for
 *    the downward search only; offsets 0 (up) / 1 (down) at i = 0 and i + 1 after; the upward search reads the seed only
 *    for last_unobserved and starts one voxel on; a voxel of a region that does not exist reads +inf and the walk then
 *    leaves that region in one step (:321-328: to local 0 of the next region going up the key, to the last voxel of the
 *    previous one going down), i advancing by as much; occupied is value >= threshold && value != +inf, free is value <
 *    threshold; upward the first unobserved -> free transition records the unobserved voxel, downward every free ->
 *    unobserved transition records the unobserved voxel (the last stands).  Then the selection ladder of :367-418.
 *  4 GROUND (findGround, :422-512).  From the candidate in the direction of up while the key is within [min_ext_key,
 *    max_ext_key] on the up axis; kNull (no region) and kUnobserved are both "unobserved" for the virtual transition and
 *    neither sets observed_above; heights are fp64 dot(position, up), position = voxelCentreGlobal(key), plus
 *    subVoxelToLocalCoord(mean.coord, resolution) for OCCUPIED voxels when the source has the mean layer and
 *    OHMHIP_HM_IGNORE_VOXEL_MEAN is off (a never written coord of 0 decodes too: ohm/VoxelMeanCompute.h:112 tests a
 *    constant); clearance test column_clearance_height - column_height >= min_clearance in fp64.  clearance and
 *    observed_above are reported as they stand when the loop ends, also when it runs out of range.
 *  5 CELL (Heightmap.cpp:619-671, addSurfaceVoxel :703-835).  ground_key = the ground found, else the walk key; its type is
 *    forced to kNull when there was no candidate; a cell is written for kOccupied, and for kFree with virtual surfaces
 *    on.  Position: the mean position for occupied, the centre for free.  src_height = dot(up, pos); pos[up] = 0; hm_key
 *    = voxelKey(pos) IN THE HEIGHTMAP'S OWN GEOMETRY (grid_resolution, regions of region_size voxels with 1 on the up
 *    axis, origin) with the up axis' region and local zeroed.  Occupancy +1.0f (surface) / -1.0f (virtual surface);
 *    HeightmapVoxel (24 bytes, ohmheightmap/HeightmapVoxel.h:68-97): height = float(src_height - dot(voxelCentreGlobal(
 *    hm_key), up)), clearance = float(ground clearance), normal 0 (or SURFACE NORMALS below), layer 0 (kHvlBaseLayer),
 *    flags = 1 (kHvfObservedAbove) or 0, contributing_samples = min(mean.count, 0xffff) of the ground voxel -- free ones too -- when the source's mean
 *    layer is in use, else 0; heightmap mean (when in use): coord = subVoxelCoord(pos - voxelCentreGlobal(hm_key),
 *    grid_resolution), count = 1.
 *  6 COLLISIONS.  Planar mode overwrites: of the source columns landing in one heightmap cell the one with the LARGEST
 *    walk index stands.  *populated counts every write, overwritten or not; *cells the cells that hold a value.
 * Results: the heightmap's three layers as dense mb x ma arrays (a fastest) over the cell range extents.first_cell ..:
 * voxelKey of the heightmap for voxelCentreGlobal(min_ext_key) - resolution / 2 and voxelCentreGlobal(max_ext_key) +
 * resolution / 2 on a and b.  Cells nobody wrote hold +inf / zeros, as a cleared chunk does.  source_column (optional):
 * the walk index of the column that wrote the cell, 0xffffffff for none.
 * NOT PROVIDED: blur, mesh, serialisation.  kSimpleFill and the layered fill modes (kLayeredFill*: multi-layer sorting,
 * the virtual-surface filter) are calls of their own (the next two blocks); here mode != 0: OHMHIP_ERR_UNSUPPORTED.
 * SURFACE NORMALS.  normal_x / y / z are 0 unless OHMHIP_HM_SURFACE_NORMALS is set and the source map has the covariance
 * layer: then the cell of a kOccupied ground voxel carries covarianceEstimatePrimaryNormal of that voxel's covariance
 * turned towards up (Heightmap.cpp:815-826), by the rule D1-D6 of COVARIANCE DECOMPOSITION below -- the reference
 * derives it with an eigen solver chosen at compile time (Eigen, or 20 rounds of glm::qr_decompose, ohm/CovarianceVoxel.
 * cpp:49-144), so the answer held to is the rule's, not either build's last bits.  Cells of free (virtual) ground
 * voxels keep zeros; no other field or array changes with the flag; it applies to the flood fill alike.  The covariance
 * is read once per cell written, not per step of the search.
 * The map is observed as the clearance queries observe it -- collected rays launched, an asynchronous launch settled,
 * regions of the host store from their pinned records, tiled regions in the caller's coordinates -- and nothing of it
 * changes.  OHMHIP_ERR_UNSUPPORTED also for a map without the occupancy layer and for a map with region ownership or a
 * partition; OHMHIP_ERR_INVALID_ARG, before any device work, for null arrays, a non-finite or non-positive
 * grid_resolution, negative or non-finite floor / ceiling / min_clearance and up_axis outside -3 .. 2;
 * OHMHIP_ERR_CAPACITY when ma * mb or na * nb exceeds 2^31. */
#define OHMHIP_HM_GENERATE_VIRTUAL_SURFACE (1u << 0) /* Heightmap::setGenerateVirtualSurface */
#define OHMHIP_HM_PROMOTE_VIRTUAL_BELOW (1u << 1)    /* Heightmap::setPromoteVirtualBelow */
#define OHMHIP_HM_IGNORE_VOXEL_MEAN (1u << 2)        /* Heightmap::setIgnoreVoxelMean */
#define OHMHIP_HM_SURFACE_NORMALS (1u << 3)          /* normals from the covariance layer (SURFACE NORMALS above) */
typedef struct ohmhip_heightmap_params
{
  double reference_pos[3];
  double cull_min[3], cull_max[3]; /* an axis with max - min <= 0 is not culled */
  double grid_resolution;          /* heightmap geometry */
  double origin[3];
  uint8_t region_size;             /* 0 = 128 (Heightmap::kDefaultRegionSize) */
  int8_t up_axis;                  /* ohm::UpAxis: -3 (kNegZ) .. 2 (kZ) */
  uint8_t mode;                    /* ohm::HeightmapMode: 0 planar, 1 simple fill (ohmhip_map_heightmap_fill); 2, 3 layered (ohmhip_map_heightmap_layered) */
  double floor, ceiling, min_clearance;
  unsigned flags;                  /* OHMHIP_HM_* */
} ohmhip_heightmap_params;
typedef struct ohmhip_heightmap_extents
{
  int16_t min_region[3]; /* min_ext_key, 10-byte GpuKey layout */
  uint8_t min_local[4];
  int16_t max_region[3]; /* max_ext_key */
  uint8_t max_local[4];
  uint32_t na, nb;       /* source columns walked */
  int16_t first_region[2]; /* first heightmap cell: region and local index on a and b */
  uint8_t first_local[2];
  uint8_t use_mean;      /* the heightmap carries a mean layer (source has one and it is not ignored) */
  uint8_t populated;     /* 0: empty map, nothing to build (every count 0) */
  uint32_t ma, mb;       /* cells of the dense result grid */
} ohmhip_heightmap_extents;
int ohmhip_map_heightmap_extents(ohmhip_map_t map, const ohmhip_heightmap_params *params,
                                 ohmhip_heightmap_extents *extents);
/* Builds the heightmap into host arrays of ma * mb cells (sizes from ohmhip_map_heightmap_extents of the same map state):
 * occupancy float, voxels24 24-byte HeightmapVoxel, mean8 (nullable) VoxelMean {u32 coord, u32 count} -- zeros when the
 * heightmap has no mean layer --, source_column (nullable).  Synchronous. */
int ohmhip_map_heightmap(ohmhip_map_t map, const ohmhip_heightmap_params *params, float *occupancy, void *voxels24,
                         void *mean8, uint32_t *source_column, uint64_t *populated, uint64_t *cells);
/* The same into DEVICE arrays, enqueued on the map's stream; ohmhip_map_sync is the fence.  d_counts (nullable): two
 * uint64 on the device, populated and cells. */
OHMHIP_EXPERIMENTAL int ohmhip_map_heightmap_device(ohmhip_map_t map, const ohmhip_heightmap_params *params,
                                                    float *d_occupancy, void *d_voxels24, void *d_mean8,
                                                    uint32_t *d_source_column, uint64_t *d_counts);

/* HEIGHTMAP, FLOOD FILL.  ohm::Heightmap::buildHeightmap in HeightmapMode::kSimpleFill, the default of the reference's
 * ohmheightmap tool (utils/ohmheightmap/ohmheightmap.cpp:158): buildHeightmapT<PlaneFillWalker> (ohmheightmap/Heightmap.
 * cpp:381-389, 522-700; PlaneFillWalker.cpp/.h).  Every column is searched from the height of the ground found next to
 * it, so the surface is followed up a ramp or onto a second storey.  Equal to the CPU algorithm for every cell and every
 * field, and the order of the visits is returned so that it can be held to the reference's FIFO.  Rules 1, 3, 4 and 5
 * are those of the block above; new or different:
 *  F1 EXTENTS.  Rule 1.  The visit grid is na x nb over [min_ext_key, max_ext_key]; (a, b, up) as in rule 2.
 *  F2 SEED.  walk_key = voxelKey(reference_pos); a null key builds nothing.  isBounded / clampToAxis (Heightmap.cpp:552-
 *    556) and PlaneFillWalker::begin (PlaneFillWalker.cpp:27-41) together clamp it into [min_ext_key, max_ext_key] on all
 *    three axes.  begin only clears the grid: the seed's cell is not marked visited and the seed is never popped.
 *  F3 A VISIT of queued key (cell, h), h = the key's offset from min_ext_key on the up index (keyHeight, PlaneFillWalker.
 *    cpp:153-156: the raw key axis whatever the sign of up_axis): candidate = findNearestSupportingVoxel (rule 3) with
 *    kVirtualSurfaces / kPromoteVirtualBelow only on the first visit and kBiasAbove added on every later one (Heightmap.
 *    cpp:385-388, :674) -- with a voxel found below and one above the closer is taken, the one above on a tie -- and
 *    never kIgnoreVirtualAbove; then findGround (rule 4).  ground_key = the ground found, else the walk key; hg its
 *    height offset.
 *  F4 NEIGHBOURS (PlaneFillWalker::visit, PlaneFillWalker.cpp:65-122; the visit mode is ignored except kIgnoreNeighbours,
 *    which is never passed).  row_delta -1 .. 1 on b (outer), col_delta -1 .. 1 on a (inner), self and cells off the
 *    grid skipped.  Neighbour n is offered hg and accepts when grid[n] < 0 || hg < grid[n] (Revisit::kLower, the
 *    constructor default: PlaneFillWalker.h:95-96); an accepted offer appends (n, hg) to the FIFO and sets grid[n] = hg.
 *    The visiting cell's own entry is not touched.
 *  F5 POP (walkNext, PlaneFillWalker.cpp:44-62).  The front key is taken and grid[cell] = h of the popped key -- which
 *    can RAISE the value after a lower offer was accepted in between, so that a later offer gets in again.
 *  F6 CELL.  Rule 5 with layer 0.  The mode is not multi-layered: a write overwrites, and of all visits that write one
 *    heightmap cell the one with the LARGEST VISIT SEQUENCE NUMBER stands.  populated counts every write.  No
 *    virtual-surface filter (ordered layers only).  The walk ends when the FIFO is empty.
 * Visits are numbered in FIFO order from 0 (the seed).  The device walks one GENERATION of the queue per round --
 * generation 0 is the seed, generation t + 1 the keys accepted while generation t is visited -- and replays the grid
 * events of a generation per cell in the reference's order, so the calls below make one host round trip
 * per generation, the _device variant too.
 * Results as for the planar call, with source_visit (nullable) in place of source_column: the sequence number of the
 * visit that wrote the cell, 0xffffffff for none; visit_log (nullable): per visit in sequence order three uint32 ia, ib,
 * h, the first visit_log_capacity visits (a smaller capacity is not an error; stats.visits is the full count).
 * stats.revisits: accepted offers to a cell that already held a height.
 * mode 1 builds; mode 0 is OHMHIP_ERR_INVALID_ARG (the planar call); modes 2 and 3 (kLayeredFillUnordered, kLayeredFill:
 * the next block, ohmhip_map_heightmap_layered) are OHMHIP_ERR_UNSUPPORTED here.  Every other refusal, and
 * how the map is observed, is the planar call's; OHMHIP_ERR_CAPACITY also when the visits exceed 2^32 - 1 or one
 * generation 2^31 / 9 keys.  Nothing of the map changes. */
typedef struct ohmhip_heightmap_fill_stats
{
  uint64_t visits;     /* keys visited, the seed included */
  uint64_t populated;  /* cell writes, overwritten or not */
  uint64_t cells;      /* cells that hold a value */
  uint64_t revisits;
  uint32_t generations, largest_generation;
} ohmhip_heightmap_fill_stats;
int ohmhip_map_heightmap_fill_extents(ohmhip_map_t map, const ohmhip_heightmap_params *params,
                                      ohmhip_heightmap_extents *extents);
int ohmhip_map_heightmap_fill(ohmhip_map_t map, const ohmhip_heightmap_params *params, float *occupancy, void *voxels24,
                              void *mean8, uint32_t *source_visit, uint32_t *visit_log, uint64_t visit_log_capacity,
                              ohmhip_heightmap_fill_stats *stats);
/* The same into DEVICE arrays (d_visit_log: 3 * visit_log_capacity uint32); the results stay in device memory, stats is
 * a host struct.  The call still makes the generation loop's host round trips and returns with the map's stream idle. */
OHMHIP_EXPERIMENTAL int ohmhip_map_heightmap_fill_device(ohmhip_map_t map, const ohmhip_heightmap_params *params,
                                                         float *d_occupancy, void *d_voxels24, void *d_mean8,
                                                         uint32_t *d_source_visit, uint32_t *d_visit_log,
                                                         uint64_t visit_log_capacity, ohmhip_heightmap_fill_stats *stats);

/* HEIGHTMAP, LAYERED.  ohm::Heightmap::buildHeightmap in HeightmapMode::kLayeredFillUnordered (2) and kLayeredFill (3):
 * buildHeightmapT<PlaneFillLayeredWalker> (ohmheightmap/Heightmap.cpp:391-402, 522-700; PlaneFillLayeredWalker.cpp),
 * addSurfaceVoxel's multi-layer branch (Heightmap.cpp:703-835) and filterVirtualVoxels / finaliseLayeredHeightmap /
 * BaseLayerCandidate::isOtherCandidateBetter / DstVoxel::haveRecordedHeight (private/HeightmapOperations.cpp:32-62,
 * 135-165, 515-773).  A column of the heightmap holds every surface found over its cell -- the floor under a platform
 * and the platform -- stacked along the RAW up axis of the heightmap's own key space: slot k of a column is the voxel at
 * the cell's key moved k steps along that axis.  Equal to the CPU algorithm for every slot and every field.  Rules 1, 3,
 * 4 and 5 are those of HEIGHTMAP, F1-F3 those of the flood fill; new or different:
 *  L1 EXTENTS, SEED.  F1 and F2.  PlaneFillLayeredWalker::begin (PlaneFillLayeredWalker.cpp:27-51) clamps the seed into
 *    the range on all axes and touches nothing: the seed is never "touched", so a neighbour may queue its column again.
 *  L2 A VISIT.  F3 unchanged: kVirtualSurfaces / kPromoteVirtualBelow only on the first visit, kBiasAbove added on every
 *    later one, never kIgnoreVirtualAbove (Heightmap.cpp:397-400, :674); then findGround.  ground_key = the ground
 *    found, else the walk key; hg its height offset.
 *  L3 NEIGHBOURS (onVisitWalker, Heightmap.cpp:60-70; visit, PlaneFillLayeredWalker.cpp:68-102).  F4's loop order.  A
 *    neighbour's key is ground_key moved sideways, so it is offered hg.  With a candidate (kAddUnvisitedNeighbours) the
 *    offer is accepted when (cell, hg) has never been touched; with a null candidate (kAddUnvisitedColumnNeighbours)
 *    when the cell has never been touched at any height.  An accepted offer touches (cell, hg) -- a node (height, next)
 *    at the head of the cell's list, :129-158 -- and is appended to the FIFO.  A pop changes nothing; there is no
 *    "lower" rule.
 *  L4 BASE CANDIDATE (Heightmap.cpp:623-624).  ground.isValid() && (ground.clearance > 0 || ground.observed_above).
 *  L5 ADDING TO A COLUMN (addSurfaceVoxel, :731-831), in visit order.  The cell key, position, occupancy value and voxel
 *    fields are rule 5's.  Slot 0 empty: write there.  Else haveRecordedHeight (HeightmapOperations.cpp:32-62) walks the
 *    slots in use from 0: |double(float height_k) + dot(centre_k, up) - src_height| < 1e-3 * grid_resolution for any slot
 *    makes the add a REPEAT, dropped.  Else all slots in use are walked keeping the nearest height difference below and
 *    above exactly as written (:754-776); the insert slot is the first empty one; the add is dropped as TOO CLOSE when
 *    either nearest difference is in (0, min_clearance] -- as written for real and virtual voxels alike.  Else height =
 *    float(src_height - dot(centre(slot), up)), layer = base candidate ? kHvlBaseLayer (0) : kHvlExtended (1), the mean
 *    coord taken against the slot's centre (DstVoxel::setPosition), and in ordered mode the column is noted as
 *    multi-layered.  populated counts the adds that stood.
 *  L6 VIRTUAL-SURFACE FILTER (kLayeredFill with virtual_surface_filter_threshold > 0; Heightmap.cpp:665-683,
 *    filterVirtualVoxels :515-600).  A map from each ground_key that added a voxel to its slot and type; the first entry
 *    for a key stands.  A virtual entry with fewer than threshold of its 26 neighbours IN THE SOURCE MAP'S KEY SPACE in
 *    that map, any type counting, becomes layer kHvlInvalid (2) with occupancy -inf
 *    (kHeightmapVirtualSurfaceFilteredValue).  The count depends on the set alone, not on the hash map's order.
 *  L7 FINALISE (kLayeredFill only; finaliseLayeredHeightmap :603-773).  A column not noted as multi-layered: an invalid
 *    voxel is cleared, anything else becomes kHvlBaseLayer.  A multi-layered column is sorted by (absolute height, slot)
 *    ascending, invalid voxels at +inf; the absolute height is getVoxelHeight of the slot the voxel sat in (dot(up,
 *    centre) + double(height)).  The sorted voxels are rewritten from slot 0, each height made relative to its new
 *    slot's centre in one float rounding, every layer kHvlExtended, invalid entries cleared.  The best base candidate
 *    (layer kHvlBaseLayer before the sort) then becomes kHvlBaseLayer by isOtherCandidateBetter (:135-165) walked in
 *    sorted order: first clearance > 0 or kHvfObservedAbove, then the distance of the absolute height to seed_height =
 *    dot(up, reference_pos), strict <, so the earlier candidate wins a tie.  kLayeredFillUnordered skips L6 and L7: its
 *    columns keep insertion order and may hold several base-layer voxels.
 * The reference's own tests run these modes with min_clearance = -1; a negative min_clearance stays an invalid argument
 * here and 0 builds the same heightmap (tests/test_heightmap_layered_ref.py).
 * Results: layer_capacity dense planes of mb x ma cells, slot-major [slot][ib][ia], a fastest.  Empty slots hold +inf /
 * zeros / 0xffffffff, as a cleared chunk does.  layer_count (nullable): slots in use per cell.  source_visit
 * (nullable): the sequence number of the visit that added the slot's voxel.  A column that needs more slots than
 * layer_capacity is not an error: the planes beyond the capacity are not returned and stats.layers says what a complete
 * call needs -- visit_log_capacity's convention.  mean8, source_visit and visit_log as in the fill call.
 * base.mode 2 or 3 builds; 0 and 1 are OHMHIP_ERR_INVALID_ARG (they have calls of their own); any other mode is
 * OHMHIP_ERR_UNSUPPORTED; layer_capacity 0, reserved != 0, a null occupancy, voxels24 or stats OHMHIP_ERR_INVALID_ARG.
 * Every other refusal, and how the map is observed, is the fill call's; OHMHIP_ERR_CAPACITY also for more than 255
 * slots in one column.  One host round trip per generation, as for the fill.  Nothing of the map changes. */
typedef struct ohmhip_heightmap_layered_params
{
  ohmhip_heightmap_params base;               /* base.mode: 2 kLayeredFillUnordered, 3 kLayeredFill */
  uint32_t virtual_surface_filter_threshold;  /* Heightmap::setVirtualSurfaceFilterThreshold; 0 = off; ordered mode only */
  uint32_t reserved;                          /* 0 */
} ohmhip_heightmap_layered_params;
typedef struct ohmhip_heightmap_layered_stats
{
  uint64_t visits;               /* keys visited, the seed included */
  uint64_t populated;            /* adds that stood (L5) */
  uint64_t cells;                /* columns holding >= 1 voxel at the end */
  uint64_t voxels;               /* voxels at the end */
  uint64_t repeats, too_close;   /* adds refused as a repeat / as too near */
  uint64_t filtered;             /* virtual voxels removed by L6 */
  uint64_t multi_layer_columns;  /* columns L5 noted as multi-layered (ordered mode) */
  uint32_t layers;               /* largest slot count of any column, before removal */
  uint32_t generations, largest_generation;
} ohmhip_heightmap_layered_stats;
int ohmhip_map_heightmap_layered_extents(ohmhip_map_t map, const ohmhip_heightmap_layered_params *params,
                                         ohmhip_heightmap_extents *extents);
int ohmhip_map_heightmap_layered(ohmhip_map_t map, const ohmhip_heightmap_layered_params *params, uint32_t layer_capacity,
                                 float *occupancy, void *voxels24, void *mean8, uint32_t *source_visit,
                                 uint8_t *layer_count, uint32_t *visit_log, uint64_t visit_log_capacity,
                                 ohmhip_heightmap_layered_stats *stats);
/* The same into DEVICE arrays; stats is a host struct.  Returns with the map's stream idle. */
OHMHIP_EXPERIMENTAL int ohmhip_map_heightmap_layered_device(ohmhip_map_t map,
                                                            const ohmhip_heightmap_layered_params *params,
                                                            uint32_t layer_capacity, float *d_occupancy,
                                                            void *d_voxels24, void *d_mean8, uint32_t *d_source_visit,
                                                            uint8_t *d_layer_count, uint32_t *d_visit_log,
                                                            uint64_t visit_log_capacity,
                                                            ohmhip_heightmap_layered_stats *stats);

/* POINT CLOUDS.  The voxels of the map that pass a test, as points, compacted on the device: what ohmtools::saveCloud,
 * saveDensityCloud, saveTsdfCloud and saveClearanceCloud (ohmtools/OhmCloud.cpp, driven by ohm2ply) collect on the host
 * after downloading every layer they read.  Only the points cross to the host.  A point is a position (3 doubles), the
 * caller's voxel key (10-byte GpuKey layout: int16 region[3], uint8 voxel[4], voxel[3] = 0) and one float value.
 *  OCCUPANCY (saveCloud, OhmCloud.cpp:453-493).  Passes: isOccupied, v != +inf && v >= threshold (ohm/VoxelOccupancy.h:
 *    161-164); with OHMHIP_CLOUD_EXPORT_FREE also isFree, v != +inf && v < threshold.  A NaN passes neither.  Position:
 *    the mean position when the map has the mean layer and OHMHIP_CLOUD_IGNORE_VOXEL_MEAN is off, else voxelCentreGlobal.
 *    The mean position is positionSafe (ohm/VoxelMean.h:47-54): voxelCentreGlobal(key) + subVoxelToLocalCoord(mean.coord,
 *    resolution), which decodes a coord of 0 like any other (ohm/VoxelMeanCompute.h:112 tests a constant) -- a free voxel
 *    exported with the mean layer lands on the decoded position of coord 0, half a voxel below its centre on every axis.  Value: the
 *    occupancy value.
 *  DENSITY (the rule saveDensityCloud is documented to apply: ohm/Density.h:34-55, SaveDensityCloudOptions; the function
 *    as written never sets the key of the voxels it reads, OhmCloud.cpp:524-538, so its output specifies nothing).
 *    density = count > 0 ? (traversal > 0 ? float(count) / traversal : +inf) : 0 with count the mean layer's sample
 *    count.  Passes: density >= density_threshold -- with a threshold of 0 every voxel of every region.  Needs the
 *    traversal and mean layers.  Position: the mean position, or voxelCentreGlobal with IGNORE_VOXEL_MEAN.  Value: the
 *    density.
 *  TSDF (saveTsdfCloud, :950-987).  Passes: weight > 0 && fabsf(distance) < surface_distance.  Position: voxelCentreLocal,
 *    the centre with a map origin of zero (ohm/OccupancyMap.h:757-778, OccupancyMap.cpp:849-852).  Value: the distance.
 *  CLEARANCE (saveClearanceCloud, :879-947).  Needs the occupancy and clearance layers.  Passes: occupancyType(v) >=
 *    export_type with unobserved -1, free 0, occupied 1 (ohm/VoxelOccupancy.h:116-128: a NaN is unobserved), and then
 *    range >= 0, where range is the clearance value, replaced by colour_range when negative.  Position:
 *    voxelCentreLocal.  Value: the range after the replacement.
 *  EXTENTS.  With OHMHIP_CLOUD_USE_EXTENTS, in any mode, only regions whose key lies per axis within [regionKey(
 *    min_extents), regionKey(max_extents)] take part (ohm/OccupancyMap.cpp:746-750, MapRegion.cpp:32-38), with every
 *    voxel of theirs, as saveClearanceCloud does.
 *  A map without a layer its mode needs yields 0 points and OHMHIP_OK (the reference returns 0).
 *  ORDER.  The reference iterates a hash map; this library fixes the order: regions ascending by (rz, ry, rx), voxels
 *    of a region ascending by MapChunk index x + y * dx + z * dx * dy -- for a region cut into tiles too.  Two calls on
 *    the same map state return identical bytes.
 * The map is observed as the heightmap observes it -- collected rays launched, an asynchronous launch settled, regions
 * of the host store from their pinned records, keys and positions in the caller's region coordinates -- and nothing of
 * it changes: no voxel, dirty bit, residency, use stamp or cache counter.
 * *count is always the number of ALL matching voxels; the arrays receive the first min(count, capacity) points.
 * capacity == 0 (null arrays) only counts.  OHMHIP_ERR_INVALID_ARG, before any device work, for null params, a null
 * map, a null count, mode > 3, unknown flag bits, a NaN density_threshold / surface_distance / colour_range, non-finite
 * extents under USE_EXTENTS and capacity > 0 with null positions; OHMHIP_ERR_UNSUPPORTED for a map with region ownership
 * or a partition (a rank holds only its territory). */
#define OHMHIP_CLOUD_OCCUPANCY 0
#define OHMHIP_CLOUD_DENSITY 1
#define OHMHIP_CLOUD_TSDF 2
#define OHMHIP_CLOUD_CLEARANCE 3
#define OHMHIP_CLOUD_EXPORT_FREE (1u << 0)       /* SaveCloudOptions::export_free */
#define OHMHIP_CLOUD_IGNORE_VOXEL_MEAN (1u << 1) /* SaveCloudOptions::ignore_voxel_mean */
#define OHMHIP_CLOUD_USE_EXTENTS (1u << 2)
/* Voxels per unit of device work: a region's block is cut into chunks of this many consecutive voxels (tests place
 * voxels on its edges). */
#define OHMHIP_CLOUD_CHUNK_VOXELS 4096
typedef struct ohmhip_cloud_params
{
  double min_extents[3], max_extents[3]; /* USE_EXTENTS */
  float density_threshold;               /* DENSITY */
  float surface_distance;                /* TSDF */
  float colour_range;                    /* CLEARANCE */
  int32_t export_type;                   /* CLEARANCE: -1 unobserved and up, 0 free and up, 1 occupied */
  uint32_t flags;                        /* OHMHIP_CLOUD_* flag bits */
  uint8_t mode;                          /* OHMHIP_CLOUD_OCCUPANCY .. OHMHIP_CLOUD_CLEARANCE */
} ohmhip_cloud_params;
/* The number of matching voxels. */
int ohmhip_map_cloud_count(ohmhip_map_t map, const ohmhip_cloud_params *params, uint64_t *count);
/* The cloud into host arrays of `capacity` points: positions_xyz 3 doubles each, keys10 (nullable) 10 bytes each,
 * values (nullable).  Synchronous. */
int ohmhip_map_cloud(ohmhip_map_t map, const ohmhip_cloud_params *params, uint64_t capacity, double *positions_xyz,
                     void *keys10, float *values, uint64_t *count);
/* The same into DEVICE arrays, enqueued on the map's stream; ohmhip_map_sync is the fence.  d_count: one uint64 on the
 * device. */
OHMHIP_EXPERIMENTAL int ohmhip_map_cloud_device(ohmhip_map_t map, const ohmhip_cloud_params *params, uint64_t capacity,
                                                double *d_positions_xyz, void *d_keys10, float *d_values,
                                                uint64_t *d_count);

/* POINT QUERIES.  ohm::NearestNeighbours (ohm/NearestNeighbours.cpp:35-181, 240-284) and voxels read by key or by world
 * point (ohm::Voxel<T>, OccupancyMap::voxelKey) against the resident map: only the answers cross to the host, where
 * ohmhip_map_read_regions moves whole region blocks.
 *  NEAREST NEIGHBOURS.  The CPU query, operation for operation, for query_count near points at once; every obstructing
 *    voxel within search_radius of a point, or only the closest.  Flags honoured: OHMHIP_QF_UNKNOWN_AS_OCCUPIED and
 *    OHMHIP_QF_NEAREST_RESULT (ohm/QueryFlag.h:36-42).
 *    Regions: those with regionKey(near - r) <= key <= regionKey(near + r) per axis (:251-263; regionKey as for the
 *    cloud's extents, stored in an int16), r the float radius widened to double; visited ascending z, then y, then x
 *    (ohm/private/OccupancyQueryAlg.h:47-58), their voxels in MapChunk index order x + y * dx + z * dx * dy.
 *    A voxel obstructs when v != +inf && v >= threshold, or when v == +inf and UNKNOWN_AS_OCCUPIED is set; a NaN never
 *    obstructs (:78-85).  A region the map does not hold contributes nothing without the flag and all of its voxels
 *    with it (:54-69); a tile of a tiled region that holds no data reads +inf.
 *    Range test, fp32 as written (:108-114): q = vec3(near - origin), a double subtract, then narrowed; d = vec3(
 *    voxelCentreLocal(key)) - q, the centre narrowed first; r2 = (d.x * d.x + d.y * d.y) + d.z * d.z; the voxel passes
 *    when r2 <= search_radius * search_radius; its range is sqrtf(r2).
 *    With NEAREST_RESULT the single result of a query is the first voxel in visiting order whose r2 is strictly smaller
 *    than that of every earlier one (:116-120; ClosestResult, ohm/private/QueryDetail.h:39-43): counts[q] is 0 or 1.
 *    Results: those of query q start at sum(counts[0 .. q)).  counts and *total are always the full numbers; the
 *    arrays receive the first min(total, capacity) results -- keys10 in the 10-byte GpuKey layout, ranges (nullable)
 *    one float each.  capacity == 0 with null arrays only counts.  Two calls on the same map state return identical
 *    bytes.
 *    The map is observed as the cloud observes it -- collected rays launched, an asynchronous launch settled, regions of
 *    the host store from their pinned records, tiled regions in the caller's coordinates -- and nothing of it changes:
 *    no voxel, dirty bit, residency, use stamp or cache counter.
 *    OHMHIP_ERR_INVALID_ARG, before any device work, for a null map, params, points (when query_count > 0), counts or
 *    total, a non-finite point, a negative or non-finite radius, unknown flag bits and capacity > 0 with null keys;
 *    OHMHIP_ERR_UNSUPPORTED for a map without the occupancy layer and for a map with region ownership or a partition;
 *    OHMHIP_ERR_CAPACITY, before any kernel runs, when the work list -- one entry per query and OHMHIP_CLOUD_CHUNK_VOXELS
 *    voxels that may lie in reach -- would exceed 2^24 entries.  query_count == 0 is OK and does nothing.
 *  VOXEL KEYS.  ohmhip_map_voxel_keys is OccupancyMap::voxelKey(point) (ohm/OccupancyMap.cpp:859-886) of the map's
 *    geometry: the caller's key in the GpuKey layout, Key::kNull (region lowest() x 3, voxel 0) where the reference
 *    yields it.  Host arithmetic only.
 *  VOXEL READS.  ohmhip_map_read_voxels copies, for each key, the ohmhip_layer_voxel_bytes(layer_id) bytes of that voxel
 *    into values, and sets present[i] = 1 when the map holds the key's region (ohmhip_map_regions lists it).  An absent
 *    region or a null key: the layer's clear value (occupancy +inf, clearance -1, zeros otherwise) and present 0.  A
 *    tile of a present tiled region that holds no data: the clear value and present 1.  Resident regions and regions of
 *    the host store alike; duplicate keys are fine; the map is observed as above and not changed.
 *    OHMHIP_ERR_INVALID_ARG for a key whose local coordinates lie outside the region dimensions (host arrays only: the
 *    device variant reads such a key as a null key), a layer id out of range and null arrays with count > 0;
 *    OHMHIP_ERR_UNSUPPORTED for a layer the map lacks and for a map with region ownership or a partition. */
#define OHMHIP_QF_NEAREST_RESULT (1u << 1) /* ohm::kQfNearestResult (ohm/QueryFlag.h:40) */
typedef struct ohmhip_neighbours_params
{
  float search_radius;
  unsigned query_flags; /* OHMHIP_QF_UNKNOWN_AS_OCCUPIED | OHMHIP_QF_NEAREST_RESULT */
} ohmhip_neighbours_params;
/* Host pointers; synchronous.  points_xyz: 3 doubles per query. */
int ohmhip_map_nearest_neighbours(ohmhip_map_t map, const double *points_xyz, size_t query_count,
                                  const ohmhip_neighbours_params *params, uint64_t capacity, uint64_t *counts,
                                  void *keys10, float *ranges, uint64_t *total);
/* The same into DEVICE arrays (d_counts query_count uint64, d_total one uint64), enqueued on the map's stream;
 * ohmhip_map_sync is the fence.  points_xyz stays a host array: the work list is laid out on the host. */
OHMHIP_EXPERIMENTAL int ohmhip_map_nearest_neighbours_device(ohmhip_map_t map, const double *points_xyz,
                                                             size_t query_count,
                                                             const ohmhip_neighbours_params *params, uint64_t capacity,
                                                             uint64_t *d_counts, void *d_keys10, float *d_ranges,
                                                             uint64_t *d_total);
int ohmhip_map_voxel_keys(ohmhip_map_t map, const double *points_xyz, size_t count, void *keys10);
int ohmhip_map_read_voxels(ohmhip_map_t map, int layer_id, const void *keys10, size_t count, void *values,
                           uint8_t *present);
/* The same on DEVICE arrays, enqueued on the map's stream; ohmhip_map_sync is the fence. */
OHMHIP_EXPERIMENTAL int ohmhip_map_read_voxels_device(ohmhip_map_t map, int layer_id, const void *d_keys10, size_t count,
                                                      void *d_values, uint8_t *d_present);

/* COVARIANCE DECOMPOSITION.  What ohm derives from an NDT voxel's covariance -- covarianceEigenDecomposition,
 * covarianceEstimatePrimaryNormal, covarianceUnitSphereTransformation (ohm/CovarianceVoxel.cpp:147-206) -- computed
 * where the covariance lies.  The reference picks its eigen solver at compile time (Eigen, or 20 rounds of
 * glm::qr_decompose), and the two agree only to a perturbation bound around the mathematical object: the spectrum of
 * C = S S^T.  This library holds to that object by ONE deterministic fp64 rule, the same text compiled for the device
 * and the host, which tests/covariance_eigen_ref.py restates operation by operation and equals bit for bit (DESIGN.md
 * 4.14 has its measured distance from an arbitrary-precision decomposition):
 *  D1 MATRIX.  The six floats p0 .. p5 of CovarianceVoxel widened to fp64; S lower triangular with rows (p0, 0, 0),
 *     (p1, p2, 0), (p3, p4, p5) (ohm/CovarianceVoxel.h:71-99); C = S S^T with c00 = p0 p0, c01 = p0 p1, c02 = p0 p3,
 *     c11 = p1 p1 + p2 p2, c12 = p1 p3 + p2 p4, c22 = (p3 p3 + p4 p4) + p5 p5; no fused multiply-add anywhere.
 *  D2 NON-FINITE.  Any entry of C NaN or +-inf: eigenvalues (1, 1, 1), identity eigenvectors, status
 *     OHMHIP_COV_NON_FINITE -- the Eigen build when its solver does not report success (CovarianceVoxel.cpp:58-65).
 *     Only a non-finite float brings it about: FLT_MAX squared is 1.2e77, finite in fp64.
 *  D3 SOLVER.  Cyclic Jacobi on the upper triangle with V = I, pairs (0,1), (0,2), (1,2) per sweep, at most 16 sweeps
 *     (no known input rotates in more than 6); a sweep starts only while (|a01| + |a02|) + |a12| != 0.  Per pair
 *     with apq != 0: g = 100 |apq|; from the fourth sweep on, |app| + g == |app| and |aqq| + g == |aqq| set apq = 0
 *     and skip; h = aqq - app; t = apq / h when |h| + g == |h|, else theta = (0.5 h) / apq, t = 1 / (|theta| +
 *     sqrt(theta theta + 1)) negated for theta < 0; c = 1 / sqrt(t t + 1), s = t c, tau = s / (1 + c); app -= t apq,
 *     aqq += t apq, apq = 0; the third index' two entries and the three rows of V's columns p and q go (x, y) ->
 *     (x - s (y + x tau), y + s (x - y tau)).  Eigenvalues ascending (the Eigen build's order) by the strict swaps
 *     (0,1), (1,2), (0,1), so equal values keep the order of their diagonal positions; V's columns move with them.
 *  D4 ROTATION.  det = (V00 m0 - V01 m1) + V02 m2 with m0 = V11 V22 - V12 V21, m1 = V10 V22 - V12 V20, m2 = V10 V21
 *     - V11 V20 (Vrc: row r, column c).  det < 0 negates column 0 (a -0.0 that makes is kept), det == 0 gives the
 *     identity (:66-74, :187-195).
 *  D5 SCALE.  scale_i = |lambda_i| > 1e-9 ? sqrt(|lambda_i|) : |lambda_i| (:198-203).
 *  D6 NORMAL.  index = 0; for i = 0 .. 2: lambda_i < lambda_index takes i (preferred_axis 0); column `index` after D4,
 *     divided by sqrt(length2) when length2 = (x x + y y) + z z > 0.  A heightmap then multiplies it by flip =
 *     ((nx ux + ny uy) + nz uz) >= 0 ? 1.0 : -1.0 for the up axis normal u, in fp64, and narrows each component to
 *     float (ohmheightmap/Heightmap.cpp:820-825).
 * ohmhip_covariance_decompose runs the rule on the host for covariances the caller holds (6 floats each): eigenvalues 3
 * doubles, eigenvectors 9 doubles column-major after D4, scales 3 (D5), normals 3 (D6, not flipped), status 1 byte;
 * every output array is optional.  No device is needed.
 * ohmhip_map_covariance_eigen decomposes the voxels at `count` keys (10-byte GpuKeys, as ohmhip_map_read_voxels takes
 * them) on the device: per key 3 + 9 doubles and a status byte -- OHMHIP_COV_ABSENT where ohmhip_map_read_voxels would
 * report present 0 (no such region, a null key; the doubles are zeros then), else OHMHIP_COV_DECOMPOSED or
 * OHMHIP_COV_NON_FINITE.  A never written voxel of a present region is the zero matrix and decomposes.  Only the results
 * cross to the host, not the 24-byte covariance layer.  A missing region is never created; the map is observed exactly
 * as ohmhip_map_read_voxels observes it and nothing of it changes; that call's refusals, with OHMHIP_ERR_UNSUPPORTED for
 * a map without the covariance layer. */
#define OHMHIP_COV_ABSENT 0
#define OHMHIP_COV_DECOMPOSED 1
#define OHMHIP_COV_NON_FINITE 2
int ohmhip_covariance_decompose(const float *covariance6, size_t count, double *eigenvalues, double *eigenvectors,
                                double *scales, double *normals, uint8_t *status);
int ohmhip_map_covariance_eigen(ohmhip_map_t map, const void *keys10, size_t count, double *eigenvalues,
                                double *eigenvectors, uint8_t *status);
/* The same on DEVICE arrays, enqueued on the map's stream; ohmhip_map_sync is the fence. */
OHMHIP_EXPERIMENTAL int ohmhip_map_covariance_eigen_device(ohmhip_map_t map, const void *d_keys10, size_t count,
                                                           double *d_eigenvalues, double *d_eigenvectors,
                                                           uint8_t *d_status);
/* COVARIANCE ELLIPSOIDS.  ohm2ply --mode covariance (utils/ohm2ply/ohm2ply.cpp:845-1018) without the download: for every
 * voxel the OHMHIP_CLOUD_OCCUPANCY cloud of the same params selects -- isOccupied only, OHMHIP_CLOUD_USE_EXTENTS
 * honoured --, in that cloud's fixed order (row i describes the voxel of row i of ohmhip_map_cloud), the position
 * positionSafe(mean), the rotation axes9 (9 doubles column-major, D4) and scales3 (D5) of covarianceUnitSphereTransformation
 * -- WITHOUT ohm2ply's display factor sqrt(3) --, the key and the occupancy value.  The selection, count, scan and emit
 * are the cloud call's own; the decomposition then reads the covariance at the emitted keys.  *count = all matching
 * voxels; at most capacity rows are written; keys10 and values are optional (the device variant needs d_keys10, zeroes
 * it past the count, and refuses a capacity above 2^31 - 1 with OHMHIP_ERR_CAPACITY).  The device variant does not
 * learn the count on the host, so its work and its scratch (25 B a row) grow with capacity, not with the count: rows
 * past the count are read at the zeroed key and not written.  Pass a capacity near the count
 * (ohmhip_map_covariance_ellipsoids_count).  OHMHIP_ERR_INVALID_ARG for
 * OHMHIP_CLOUD_EXPORT_FREE, OHMHIP_CLOUD_IGNORE_VOXEL_MEAN, a mode other than OHMHIP_CLOUD_OCCUPANCY and null positions /
 * axes / scales with capacity > 0; OHMHIP_ERR_UNSUPPORTED for a map without the occupancy, mean or covariance layer
 * (ohm2ply refuses such a map, :863-873); every other refusal as for ohmhip_map_cloud.  Nothing of the map changes. */
int ohmhip_map_covariance_ellipsoids_count(ohmhip_map_t map, const ohmhip_cloud_params *params, uint64_t *count);
int ohmhip_map_covariance_ellipsoids(ohmhip_map_t map, const ohmhip_cloud_params *params, uint64_t capacity,
                                     double *positions_xyz, double *axes9, double *scales3, void *keys10, float *values,
                                     uint64_t *count);
/* The same into DEVICE arrays (d_count one uint64), enqueued on the map's stream; ohmhip_map_sync is the fence. */
OHMHIP_EXPERIMENTAL int ohmhip_map_covariance_ellipsoids_device(ohmhip_map_t map, const ohmhip_cloud_params *params,
                                                                uint64_t capacity, double *d_positions_xyz,
                                                                double *d_axes9, double *d_scales3, void *d_keys10,
                                                                float *d_values, uint64_t *d_count);

/* POINT FILTER.  ohmfilter's filterCloud (utils/ohmfilter/ohmfilter.cpp:150-279): of a point cloud, the points that fall
 * in an occupied voxel of the resident map and -- on a map with the NDT layers -- inside that voxel's Gaussian
 * (filterPointByCovariance, :67-91); how a map strips transient objects from a scan.  Per point, only the answers cross
 * to the host.  For each point p (three doubles):
 *  1. KEY.  key = OccupancyMap::voxelKey(p) (ohm/OccupancyMap.cpp:859-886), as ohmhip_map_voxel_keys evaluates it.  A
 *     null key (Key::isNull, ohm/Key.h:206) gives status 0.
 *  2. OCCUPANCY.  v = the voxel's occupancy; +inf for a region the map does not hold and for a tile of a present tiled
 *     region that holds no data.  The point is occupied iff v != +inf && v >= threshold (isOccupied, ohm/
 *     VoxelOccupancy.h:161-164); a NaN is not occupied.  Not occupied: status 0.
 *  3. COVARIANCE TEST.  It runs iff OHMHIP_PF_OCCUPANCY_ONLY is not set, the map carries both the mean and the covariance
 *     layer, and expected_value_tolerance >= 0; otherwise an occupied point has status 1 (ohmfilter.cpp:187-221: layer
 *     availability selects the filter, and a negative tolerance keeps every occupied point).  The test (:67-91,
 *     :197-203), fp64 throughout with contraction off:
 *       mean = voxelCentreGlobal(key) + subVoxelToLocalCoord(mean.coord, resolution) -- positionUnsafe, ohm/VoxelMean.h:
 *         47-54, per axis the centre (ohm/OccupancyMap.h:757-778) and then the decoded offset added; a coord of 0
 *         decodes like any other, as for the POINT CLOUDS;
 *       d = p - mean;
 *       S = covarianceSqrtMatrix (ohm/CovarianceVoxel.h:71-91): the six floats c0..c5 widened to double, the lower
 *         triangular [[c0,0,0],[c1,c2,0],[c3,c4,c5]], stored by columns m[column][row]: m[0] = (c0, c1, c3), m[1] =
 *         (0, c2, c4), m[2] = (0, 0, c5);
 *       v = inverse(S) * d, the inverse as glm writes it, the adjugate times 1 / determinant over the full 3 x 3 matrix,
 *         zeros included.  glm is not installed beside this library, so the operation order inside inverse is not
 *         pinned to the reference bit for bit; THIS is the order used:
 *           r = 1 / (m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02) + m20 * (m01 * m12 - m11 * m02))
 *           i00 =  (m11 * m22 - m21 * m12) * r   i10 = -(m10 * m22 - m20 * m12) * r   i20 =  (m10 * m21 - m20 * m11) * r
 *           i01 = -(m01 * m22 - m21 * m02) * r   i11 =  (m00 * m22 - m20 * m02) * r   i21 = -(m00 * m21 - m20 * m01) * r
 *           i02 =  (m01 * m12 - m11 * m02) * r   i12 = -(m00 * m12 - m10 * m02) * r   i22 =  (m00 * m11 - m10 * m01) * r
 *         with mCR = m[C][R] and the sum in r taken left to right; v.x = (i00 * d.x + i10 * d.y) + i20 * d.z, v.y =
 *         (i01 * d.x + i11 * d.y) + i21 * d.z, v.z = (i02 * d.x + i12 * d.y) + i22 * d.z;
 *       a = (v.x * v.x + v.y * v.y) + v.z * v.z;
 *       kept iff fabs(a) < 3.0 + expected_value_tolerance, that sum in fp64.  Status 1 when kept, 2 when removed by this
 *         test.
 *     The adjugate form is deliberate: a zero on the diagonal gives a determinant of 0, NaNs in v, and the point is
 *     removed -- as are points of a voxel with a NaN or infinite entry.  The reference behaves the same way.
 *  OUTPUTS.  status [count] (nullable): 0 / 1 / 2.  kept_indices [capacity] (null only with capacity == 0): the indices
 *    of the status-1 points, ascending; it receives the first min(*kept, capacity).  values [count] (nullable): a where
 *    the covariance test ran, a quiet NaN (0x7ff8000000000000) elsewhere.  keys10 [count] (nullable): each point's key in
 *    the 10-byte GpuKey layout, Key::kNull as ohmhip_map_voxel_keys writes it.  *kept: always the full number of kept
 *    points.  Two calls on the same map state return identical bytes: nothing that determines an output uses an atomic.
 *  The map is observed as the other read-side calls observe it -- collected rays launched, an asynchronous launch
 *  settled, regions of the host store from their pinned records, tiled regions in the caller's coordinates -- and
 *  nothing of it changes: no voxel, dirty bit, residency, use stamp or cache counter.
 *  OHMHIP_ERR_INVALID_ARG, before any device work, for a null map, params or kept, null points with count > 0, unknown
 *  flag bits, a NaN tolerance, stride_doubles < 3, capacity > 0 with null kept_indices and -- host variant -- a
 *  non-finite point (the device variant gives such a point status 0 and a null key); OHMHIP_ERR_UNSUPPORTED for a map
 *  without the occupancy layer and for a map with region ownership or a partition.  count == 0 is OK and writes *kept
 *  = 0. */
#define OHMHIP_PF_OCCUPANCY_ONLY (1u << 0) /* ohmfilter --occupancy-only */
#define OHMHIP_PF_PIECE_POINTS (1u << 18)  /* points per staged piece of the host variant; tests straddle it */
typedef struct ohmhip_point_filter_params
{
  double expected_value_tolerance; /* ohmfilter --tolerance: < 0 turns the covariance test off */
  uint32_t flags;                  /* OHMHIP_PF_* */
} ohmhip_point_filter_params;
/* Host pointers; synchronous.  points_xyz: 3 doubles per point, staged through pinned memory in pieces of
 * OHMHIP_PF_PIECE_POINTS; indices continue across pieces. */
int ohmhip_map_filter_points(ohmhip_map_t map, const double *points_xyz, uint64_t count,
                             const ohmhip_point_filter_params *params, uint64_t capacity, uint8_t *status,
                             uint64_t *kept_indices, double *values, void *keys10, uint64_t *kept);
/* The same on DEVICE arrays, enqueued on the map's stream; ohmhip_map_sync is the fence.  Point i is read at d_points +
 * i * stride_doubles, stride_doubles >= 3: the sample ends of a ray buffer (ohmhip_transform_samples' output: stride 6,
 * the pointer advanced by 3) are read where they lie.  d_kept: one uint64 on the device.  OHMHIP_ERR_CAPACITY for more
 * than 2^36 points in one call. */
OHMHIP_EXPERIMENTAL int ohmhip_map_filter_points_device(ohmhip_map_t map, const double *d_points, uint64_t stride_doubles,
                                                        uint64_t count, const ohmhip_point_filter_params *params,
                                                        uint64_t capacity, uint8_t *d_status, uint64_t *d_kept_indices,
                                                        double *d_values, void *d_keys10, uint64_t *d_kept);

/* GpuTransformSamples::transform (ohmgpu/GpuTransformSamples.h:75-79, .cpp:97-210; kernel transformTimestampedPoints,
 * ohmgpu/gpu/TransformSamples.cl:94-228): sensor-frame samples with time stamps + a timestamped trajectory (translations
 * xyz, rotations as quaternions x,y,z,w) -> world-frame ray pairs (sensor origin, sample), 6 doubles per valid sample,
 * compacted in input order into `output` (resized), ready for ohmhip_map_integrate_rays_device().  Same rules as the
 * reference: samples with a NaN component or dot(s, s) > max_range are skipped; pose = lerp of the bracketing
 * translations and rot[from] * slerp(rot[from], rot[to], f); fp64 throughout (the reference kernel is fp32).  Host
 * pointers in; *ray_elements = 2 x valid samples (the reference's return value).  Synchronous on `stream` (NULL: the
 * default stream). */
int ohmhip_transform_samples(const double *transform_times, const double *transform_translations,
                             const double *transform_rotations_xyzw, uint32_t transform_count,
                             const double *sample_times, const double *local_samples, uint32_t point_count,
                             double max_range, ohmhip_stream_t stream, ohmhip_buffer_t output, uint32_t *ray_elements);

/* RAY PATTERNS.  ohm::RayPattern / RayPatternConical / ClearingPattern (ohm/RayPattern.{h,cpp}, ohm/RayPatternConical.cpp,
 * ohm/ClearingPattern.{h,cpp}) with the pattern resident in device memory: a fixed fan of rays in the sensor frame, moved
 * to a pose and integrated -- per application only the pose crosses the link.  A pattern is ray_count (start, end) pairs
 * of 3 doubles; the host mirrors build it (addPoints / addRays, the conical constructor) and hand it over once.
 *   POSES.  pose_kind OHMHIP_POSE_QUAT: 7 doubles per pose, translation xyz then rotation x, y, z, w (the layout of
 *   ohmhip_transform_samples); OHMHIP_POSE_MAT4: 16 doubles per pose, a column-major 4 x 4 matrix m[c][r] = m[4c + r].
 *   ARITHMETIC (fp64, one rounding per operation, no contraction; tests/ray_pattern_ref.py is the model the device is held
 *   to bit for bit).  Every pattern point p becomes s = scaling * p per component, then
 *     QUAT (RayPattern.cpp:58-70, glm's quaternion * vector): u = (q.x, q.y, q.z); uv = cross(u, s); uuv = cross(u, uv);
 *       out = (s + ((uv * q.w) + uuv) * 2) + translation, cross(a, b) = (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x,
 *       a.x*b.y - b.x*a.y); the quaternion is used as given, not normalised;
 *     MAT4 (RayPattern.cpp:72-84, glm's mat4 * vec4): out[r] = (m[0][r]*s.x + m[1][r]*s.y) + (m[2][r]*s.z + m[3][r]).
 *   (The reference's matrix overload has no scaling argument: scaling == 1 is that overload.)
 *   OUTPUT: pose major, in pattern order, 6 doubles per ray: a call with K poses yields exactly the K ray sets of K
 *   single-pose calls, one behind the other. */
typedef struct ohmhip_pattern_s *ohmhip_pattern_t;
#define OHMHIP_POSE_QUAT 0
#define OHMHIP_POSE_MAT4 1
/* Copies ray_count ray pairs (6 doubles each, host memory) to the device.  ray_count == 0 (ray_pairs may be NULL then)
 * makes an empty pattern: every use of it succeeds and does nothing. */
int ohmhip_pattern_create(const double *ray_pairs, size_t ray_count, ohmhip_pattern_t *pattern);
/* The pattern's output buffers may be read by batches in flight: destroy it after ohmhip_map_sync of the maps it was
 * applied to (the call itself waits for the device). */
int ohmhip_pattern_destroy(ohmhip_pattern_t pattern);
int ohmhip_pattern_ray_count(ohmhip_pattern_t pattern, size_t *ray_count);
/* RayPattern::buildRays for pose_count poses at once: the rays are built on the device into a buffer of the pattern's
 * and, with host_out non-NULL, copied to it (pose_count * ray_count * 6 doubles).  Synchronous.  OHMHIP_ERR_CAPACITY when
 * pose_count * ray_count reaches 2^28 (what one batch takes). */
int ohmhip_pattern_build_rays(ohmhip_pattern_t pattern, const double *poses, size_t pose_count, int pose_kind,
                              double scaling, double *host_out);
/* ClearingPattern::lastRaySet: the rays of the latest ohmhip_pattern_build_rays / ohmhip_map_apply_pattern call on this
 * pattern, read back from the device.  *elements = number of points (2 per ray; 0 before any call); host_out may be
 * NULL to ask for the size only.  Waits for the kernel that built them, not for the batch that integrates them. */
int ohmhip_pattern_last_rays(ohmhip_pattern_t pattern, double *host_out, size_t *elements);
/* ClearingPattern::apply (ohm/ClearingPattern.h:109-130) for pose_count poses in one device batch, in this order:
 *  1 rays collected from earlier integrate calls (batch coalescing) are launched: they belong to the unscaled miss value;
 *  2 this batch's miss value is the fp32 product miss_value * probability_scaling;
 *  3 the rays are built on the map's stream into one of three buffers the pattern owns, used in turn by
 *    ohmhip_map_batches_launched -- the rule of ohmhip_map_integrate_rays_device for arrays of batches in flight;
 *  4 that buffer is a device batch of its own with ray_flags & ~OHMHIP_RF_REVERSE_WALK (ClearingPattern.cpp:40-44),
 *    ordered behind the kernel by the streams alone: no host synchronisation, nothing staged, never merged with the
 *    calls that follow;
 *  5 the miss value is restored, also when the batch fails.
 * The batch replays its rays one by one in order (OHMHIP_RF_STOP_ON_FIRST_OCCUPIED included), so K poses in one call give
 * the map K calls with one pose each give -- a later pose's rays see what an earlier pose cleared.  *integrated (optional)
 * = points of the rays the map's ray filter passed (a NaN pose yields NaN rays, which it drops).  pose_count == 0 or an
 * empty pattern: OHMHIP_OK, nothing integrated, nothing launched.  OHMHIP_ERR_INVALID_ARG for NULL arguments and an
 * unknown pose_kind, OHMHIP_ERR_CAPACITY when pose_count * ray_count reaches 2^28.  Flags, map modes and partitioned maps
 * are served as ohmhip_map_integrate_rays_device serves them. */
int ohmhip_map_apply_pattern(ohmhip_map_t map, ohmhip_pattern_t pattern, const double *poses, size_t pose_count,
                             int pose_kind, double scaling, float probability_scaling, unsigned ray_flags,
                             size_t *integrated);

/* MAP COPY.  ohm::copyMap (ohm/CopyUtil.h:148, ohm/CopyUtil.cpp:58-165) and the rule OccupancyMap::clone is built on
 * (ohm/OccupancyMap.cpp:953-1004) between two device maps, device to device: one kernel launch per call (k_copy_map),
 * nothing crosses the host link.  tests/copy_ref.py restates C2 / C3 on the CPU.
 *  C1 canCopy (CopyUtil.cpp:52-56): dst != src and equal resolution, region voxel dimensions and origin, each compared
 *     with ==; anything else is OHMHIP_ERR_INVALID_ARG.  The modes may differ (an NDT map's occupancy into a plain map).
 *  C2 layers: the layers both maps hold (calculateOverlappingLayerSet), narrowed by params->layers (CopyLayerFilter,
 *     judged on the source layer; 0 = every common layer).  No layer in common before the mask: nothing happens,
 *     OHMHIP_ERR_NOT_FOUND (the reference returns false, :78-82).  The mask removes every common layer: the regions are
 *     created in dst, nothing is copied, OHMHIP_OK (:86-100, 117-126).
 *  C3 regions: a region of src is copied when it passes every filter given.
 *     (a) keys_xyz: only the listed regions (how the mirrors run arbitrary host CopyChunkFilters); a key src does not
 *         hold is skipped and counted in keys_absent, a repeated key counts once.
 *     (b) OHMHIP_COPY_USE_EXTENTS: copyFilterExtents (CopyUtil.cpp:37-45) in its operation order, in double, on the host:
 *         half = 0.5 * region_spatial_dimensions; lo = centre - half; hi = centre + half; pass = no axis with
 *         hi < min_extents and no axis with lo > max_extents (touching passes).  centre is MapChunk::region.centre =
 *         coord * region_dimension WITHOUT the map origin (ohm/MapRegion.cpp:40-42, ohm/MapCoord.h:37-40): on a map
 *         whose origin is not zero the box is relative to the origin.  Kept as the reference has it.
 *     (c) OHMHIP_COPY_DIRTY_ONLY, in the place of copyFilterStamp (CopyUtil.cpp:47-50): the regions
 *         ohmhip_map_dirty_regions lists -- changed since the caller's last ohmhip_map_clear_dirty / syncVoxels.  The
 *         device map keeps dirty bits, not stamps.  The copy never clears the bit.
 *  C4 what lands: in every copied region each copied layer of dst equals src's block byte for byte, whether dst held the
 *     region or not, voxels src holds no data for included.  A tile of a tiled region (LARGE REGIONS) that src lacks reads
 *     as cleared in dst afterwards, even where dst had data.  Layers only dst has keep what they held; in a region the
 *     copy creates they read as cleared.
 *  C5 dst behaves through every entry point like a dst that received the same regions and layers by
 *     ohmhip_map_read_regions(src) + ohmhip_map_write_regions(dst): the write-back's pre-cleaned copies of the regions
 *     are void; the NDT replay mask is re-derived from the mean layer, the TSDF replay mask from the TSDF layer with
 *     DST's truncation distance; a copied occupancy layer marks the region's clearance changed, a copied clearance layer
 *     marks it unwritten.  Copied regions carry all three dirty bits, as after ohmhip_map_mark_dirty.
 *  C6 src is read only: it is settled first (rays collected from earlier calls are launched, as every observer does);
 *     after that no voxel, dirty bit, residency, use stamp or cache counter of it changes.  Regions in its host store
 *     (SPILL TO HOST) are read where they lie, nothing is re-admitted.
 *  C7 dst is written: settled, its stream idle; regions it keeps in its host store come back as for
 *     ohmhip_map_write_regions; its memory limit and spill setting apply exactly as for an ohmhip_map_write_regions of the
 *     same keys, with the same errors (OHMHIP_ERR_CAPACITY: dst holds what it held, stats->regions_created and
 *     bytes_copied are 0, regions_passed says what the copy would have moved).
 *  C8 OHMHIP_ERR_UNSUPPORTED when either map has region ownership or a partition, or dst has replica merge enabled.
 *     OHMHIP_ERR_INVALID_ARG, before any device work, for null maps, unknown flag bits, a layer mask with bits >=
 *     OHMHIP_LID_COUNT, keys_xyz non-null with key_count 0 or the reverse, and NaN extents under USE_EXTENTS.
 *  C9 blocking: the call returns with the copy complete and both maps free to use. */
#define OHMHIP_COPY_DIRTY_ONLY (1u << 0)
#define OHMHIP_COPY_USE_EXTENTS (1u << 1)
typedef struct ohmhip_copy_params
{
  unsigned flags;
  unsigned layers; /* OHMHIP_LAYER_BIT mask of source layers allowed; 0 => every common layer */
  double min_extents[3], max_extents[3];
  const int16_t *keys_xyz; /* optional; NULL => every region of src */
  size_t key_count;
} ohmhip_copy_params;
typedef struct ohmhip_copy_stats
{
  uint64_t regions_passed;  /* regions of src that passed the filters    */
  uint64_t regions_created; /* of those, regions dst did not hold before */
  uint64_t keys_absent;
  uint64_t bytes_copied;
  unsigned layers_copied; /* OHMHIP_LAYER_BIT mask */
} ohmhip_copy_stats;
/* OHMHIP_OK when C1 holds, OHMHIP_ERR_INVALID_ARG otherwise (null maps included).  No device work. */
int ohmhip_map_can_copy(ohmhip_map_t dst, ohmhip_map_t src);
int ohmhip_map_copy(ohmhip_map_t dst, ohmhip_map_t src, const ohmhip_copy_params *params /* NULL: everything */,
                    ohmhip_copy_stats *stats /* optional */);

/* MAP COMPARE.  ohm::compare::compareVoxels (ohm/CompareMaps.h:139, ohm/CompareMaps.cpp:334-386), the rule ohmcmp is
 * built on (utils/ohmcmp/ohmcmp.cpp:356-386), between two device maps: one layer of `eval` held against the same layer
 * of `ref`, member by member, on the device -- only the result and the two lists cross the host link.
 * tests/compare_ref.py restates K3 - K5 on the CPU.
 *  K1 compatibility: both maps must have equal region voxel dimensions, else OHMHIP_ERR_INVALID_ARG (the reference would
 *     index one map's block with the other's key, CompareMaps.cpp:364-373).  Resolution, origin and mode are not looked
 *     at, as in compareVoxels.  eval == ref is allowed.  Region ownership or a partition on either map:
 *     OHMHIP_ERR_UNSUPPORTED (a rank holds only its territory).
 *  K2 layout (compareLayoutLayer, CompareMaps.cpp:78-144): a layer id has one layout here, so the layouts match exactly
 *     when both maps hold layer_id.  Without a match result->layout_match = 0, every count is 0 and the call returns
 *     OHMHIP_OK (:339-344: a result, not an error); member_count is the layer's in either case.  The members, all 4
 *     bytes and of one type per layer (ohm/DefaultLayer.cpp:85-303): occupancy {occupancy f32}; mean {coord, count u32};
 *     covariance {P00, P01, P11, P02, P12, P22 f32}; traversal {traversal f32}; touch_time {touch u32}; incident_normal
 *     {packed_normal u32}; intensity {mean, cov f32}; hit_miss_count {hit_count, miss_count u32}; tsdf {weight,
 *     distance f32}; clearance {clearance f32}.  A tolerance_members bit at or above the layer's member count:
 *     OHMHIP_ERR_INVALID_ARG.
 *  K3 what is visited (CompareMaps.cpp:359-383): every voxel of every region of ref, narrowed by keys_xyz to the listed
 *     regions; a key ref does not hold is skipped and counted in keys_absent, a repeated key counts once.  Regions only
 *     eval holds are ignored.  A region eval lacks fails every one of its dx * dy * dz voxels: it counts in
 *     regions_missing, is listed in missing_regions_xyz, and adds nothing to the mismatch list, member_failed or
 *     member_max_diff (compareVoxel returns before it logs, :197-205).  A tile of a tiled region (LARGE REGIONS) that one
 *     map lacks, inside a region that map does hold, reads as the layer's clear word (occupancy +inf, clearance -1,
 *     zeros otherwise).  regions_compared, regions_missing and keys_absent describe the selection, with or without
 *     OHMHIP_CMP_CONTINUE.
 *  K4 one voxel (compareVoxel :207-331, compareDatum :58-75): every member is judged; a voxel passes when all its
 *     members pass.  Member i without its tolerance_members bit passes when its 4 bytes are equal (:313-318).  With the
 *     bit: eps = the low 4 bytes of tolerance_bits[i] read as the member's type T; hi, lo = the two values, exchanged
 *     only when ref > val (:69-72); the member passes when hi == lo || (hi - lo) <= eps (:74), for f32 the subtraction
 *     and both comparisons in fp32 with subnormals kept, for u32 unsigned.  Hence: a NaN on either side fails under any
 *     tolerance (eps = +inf and identical NaN bits included) and passes the byte comparison when the bits are equal;
 *     +0 against -0 passes with a tolerance and fails without; +-inf against itself passes; inf against FLT_MAX fails for
 *     every finite eps; a NaN or negative eps passes equal values only; a subnormal difference is not zero; FLT_MAX
 *     against -FLT_MAX overflows to inf.
 *  K5 order and stopping.  The reference iterates a hash map; this library fixes the order of POINT CLOUDS' ORDER rule:
 *     regions ascending by (rz, ry, rx), voxels by MapChunk index x + y * dx + z * dx * dy, for tiled regions too.
 *     With OHMHIP_CMP_CONTINUE everything is compared: mismatch_keys10 receives the first min(mismatch_count,
 *     mismatch_capacity) failing voxels of the regions both maps hold, in order, as 10-byte key records (int16
 *     region[3], uint8 voxel[3], and in byte 9 the mask of failing members); missing_regions_xyz the first
 *     min(missing_count, missing_capacity) regions eval lacks, in order; member_failed[i] counts the voxels whose member
 *     i failed; member_max_diff[i] is the largest hi - lo of member i over the visited voxels of regions both maps hold
 *     where neither side is a NaN -- a float's bits in the low word, possibly inf -- and 0 when there is none (a
 *     difference that is itself a NaN, inf against itself, does not count; a zero of either sign is +0).
 *     Without the flag (the reference's default, OHM_CMP_FAIL, CompareMaps.h:18-22) the result is the one a sequential
 *     walk in that order returns at its first failure: voxels_failed 1 or 0, voxels_passed the voxels ahead of it,
 *     mismatch_count + missing_count <= 1 with that one entry in its list, member_failed the failing voxel's mask as
 *     0 / 1 (all zero when the failure is a region eval lacks), member_max_diff all zero.
 *  K6 both maps are only read: each is settled first (collected rays launched, an asynchronous launch finished); after
 *     that no voxel, dirty bit, residency, use stamp or cache counter of either changes.  Regions in a host store (SPILL
 *     TO HOST) are read where they lie.  Nothing that determines an output uses an atomic: two calls return identical
 *     bytes.
 *  K7 capacities: a capacity of 0 (its array may be NULL) only counts; the totals are always complete.
 *     OHMHIP_ERR_INVALID_ARG, before any device work, for a null map, params or result, unknown flag bits, layer_id
 *     outside 0 .. OHMHIP_LID_COUNT - 1, a non-zero capacity with a null array, keys_xyz non-null with key_count 0 or the
 *     reverse, and the refusals of K1 / K2.  ohmhip_map_compare is blocking. */
#define OHMHIP_CMP_CONTINUE (1u << 0) /* ohm::compare::kContinue (CompareMaps.h:44) */
#define OHMHIP_CMP_MAX_MEMBERS 6
typedef struct ohmhip_compare_params
{
  unsigned flags;
  int layer_id;
  unsigned tolerance_members;                      /* bit i: member i is compared with a tolerance */
  uint64_t tolerance_bits[OHMHIP_CMP_MAX_MEMBERS]; /* memberClearValue of the reference's tolerance object */
  const int16_t *keys_xyz;                         /* optional; NULL => every region of ref */
  size_t key_count;
} ohmhip_compare_params;
typedef struct ohmhip_compare_result
{
  uint64_t voxels_passed, voxels_failed; /* VoxelsResult (CompareMaps.h:48-56) */
  int32_t layout_match;
  uint32_t member_count;
  uint64_t regions_compared, regions_missing, keys_absent;
  uint64_t mismatch_count, missing_count; /* totals, whatever the capacities */
  uint64_t member_failed[OHMHIP_CMP_MAX_MEMBERS];
  uint64_t member_max_diff[OHMHIP_CMP_MAX_MEMBERS]; /* float members: the float's bits in the low word */
} ohmhip_compare_result;
int ohmhip_map_compare(ohmhip_map_t eval, ohmhip_map_t ref, const ohmhip_compare_params *params,
                       uint64_t mismatch_capacity, void *mismatch_keys10, uint64_t missing_capacity,
                       int16_t *missing_regions_xyz, ohmhip_compare_result *result);
/* The same with the two lists and the result in DEVICE memory, enqueued on ref's stream; ohmhip_map_sync(ref) is the
 * fence.  params and its key list stay host memory: the work list is laid out on the host. */
OHMHIP_EXPERIMENTAL int ohmhip_map_compare_device(ohmhip_map_t eval, ohmhip_map_t ref,
                                                  const ohmhip_compare_params *params, uint64_t mismatch_capacity,
                                                  void *d_mismatch_keys10, uint64_t missing_capacity,
                                                  int16_t *d_missing_regions_xyz, ohmhip_compare_result *d_result);

/* VOXEL EDITS.  The Voxel API's writes for many voxels at once, on the device: Voxel<T>::write (ohmhip_map_write_voxels),
 * ohm::integrateHit(map, key) / ohm::integrateMiss(map, key) (ohm/VoxelOccupancy.h:57-108) and ohm::integrateHit(map,
 * sample) (ohm/VoxelMean.h:196-203) (ohmhip_map_integrate_voxels).  Keys are 10-byte GpuKey records as
 * ohmhip_map_read_voxels takes them, in the caller's region coordinates; with points_xyz in their place the key is
 * OccupancyMap::voxelKey(point), computed on the device.  tests/voxel_edit_ref.py restates E1 - E4 on the CPU.
 *  E1 order: for every voxel the result is the one obtained by applying that voxel's elements one at a time, in input
 *     order, with the reference functions; different voxels are independent; two calls are ordered as called.  The map
 *     is settled first (rays collected from earlier calls are launched, an asynchronous launch is finished, as every
 *     observer does): an edit between two ohmhip_map_integrate_rays calls lands between them.
 *  E2 SET (ohmhip_map_write_voxels): the voxel's ohmhip_layer_voxel_bytes(layer_id) bytes become values[i], for any
 *     layer the map holds; among duplicate keys the last in input order wins.  The bytes are stored as given: no clamp,
 *     no validation (NaN, -0.0, +-inf and out-of-clamp values are the caller's business, as with
 *     ohmhip_map_write_regions).
 *  E3 HIT is occupancyAdjustHit(&v, v, hit_value, +inf, max_value, saturate_at_min ? min_value : lowest(),
 *     saturate_at_max ? max_value : FLT_MAX, false), MISS is occupancyAdjustMiss with miss_value and min_value in the
 *     places of hit_value and max_value: the argument lists of VoxelOccupancy.h:63-65 and :94-96, with the values of
 *     the map's current configuration.  No ray flag and no ray filter applies and no other layer is touched.
 *  E4 HIT_SAMPLE requires points (with keys: OHMHIP_ERR_INVALID_ARG).  E3's HIT on voxelKey(point); then, on a map with
 *     the mean layer, updatePosition (VoxelMean.h:158-163): coord' = subVoxelUpdate(coord, count, point -
 *     voxelCentreGlobal(key), resolution), count' = min(count, 0xfffffffe) + 1 -- the count saturates; it is not the ray
 *     mapper's wrapping ++count.  Without the mean layer only the occupancy changes (updatePositionSafe).  Covariance,
 *     intensity, hit / miss count, touch time, incident, traversal and TSDF layers are never touched, on NDT maps too.
 *  E5 regions: a key whose region the map does not hold creates it, cleared (of a tiled region, LARGE REGIONS, the
 *     tiles the edit writes to).  Regions in the host store (SPILL TO HOST) come back as for ohmhip_map_write_regions
 *     of the same keys; the memory limit and the spill setting apply as there, with the same errors.  All regions an
 *     edit needs are named before the first voxel is written: on OHMHIP_ERR_CAPACITY the map holds exactly what it
 *     held and the stats are zero.
 *  E6 bookkeeping: afterwards the map behaves through every entry point like one that received the same voxels by
 *     ohmhip_map_read_regions, a host edit, ohmhip_map_write_regions and ohmhip_map_mark_dirty.  Every touched region
 *     carries all three dirty bits; the write-back's pre-cleaned copy of it is void.  On an NDT map a voxel whose mean
 *     count the edit makes or leaves > 0 has its ordered-replay mask bit set, one whose count becomes 0 has it cleared;
 *     on a TSDF map a SET on the TSDF layer re-derives the voxel's bit from the map's truncation distance.  The bit is
 *     updated per voxel, not by a pass over the region.  An occupancy edit marks the region's clearance changed, a SET
 *     on the clearance layer marks it unwritten.
 *  E7 a null key (region -32768 x 3) or a point voxelKey() maps to Key::kNull is skipped and counted in null_keys (the
 *     reference requires isValid() and specifies nothing).  Host arrays: a key with local coordinates outside the
 *     region dimensions, or a non-finite point, is OHMHIP_ERR_INVALID_ARG before any device work; in _device arrays
 *     such an element, and one whose op is not 1 .. 3 or is HIT_SAMPLE beside keys, is treated as a null key.
 *  E8 OHMHIP_ERR_INVALID_ARG, before any device work, for a null map, count > 0x7fffffff, null arrays with count > 0,
 *     both of keys10 / points_xyz (or neither with count > 0), an op -- with ops == NULL -- or, for host arrays, any
 *     ops[i] outside 1 .. 3, and a layer_id out of range.  OHMHIP_ERR_UNSUPPORTED for a layer the map lacks, HIT / MISS /
 *     HIT_SAMPLE on a map without the occupancy layer, a map with region ownership or a partition, and a map with
 *     replica merge enabled.  count == 0 is OHMHIP_OK and does nothing.
 *  E9 blocking: every form returns with the edit complete and the stats final.  The _device forms read arrays that must
 *     be complete when the call is made; all forms make one read-back of the distinct regions the edit names (the
 *     region table is the host's). */
#define OHMHIP_EDIT_HIT 1        /* ohm::integrateHit(map, key)     ohm/VoxelOccupancy.h:57-77   */
#define OHMHIP_EDIT_MISS 2       /* ohm::integrateMiss(map, key)    ohm/VoxelOccupancy.h:88-108  */
#define OHMHIP_EDIT_HIT_SAMPLE 3 /* ohm::integrateHit(map, sample)  ohm/VoxelMean.h:196-203; points only */
typedef struct ohmhip_voxel_edit_stats
{
  uint64_t applied;         /* elements applied                                                         */
  uint64_t null_keys;       /* elements skipped: null key, or a point voxelKey() maps to Key::kNull      */
  uint64_t distinct_voxels; /* voxels written                                                           */
  uint64_t regions_touched; /* caller's regions holding at least one written voxel                      */
  uint64_t regions_created; /* of those, regions the map did not hold before                            */
} ohmhip_voxel_edit_stats;
int ohmhip_map_write_voxels(ohmhip_map_t map, int layer_id, const void *keys10, size_t count, const void *values,
                            ohmhip_voxel_edit_stats *stats /* optional */);
OHMHIP_EXPERIMENTAL int ohmhip_map_write_voxels_device(ohmhip_map_t map, int layer_id, const void *d_keys10, size_t count,
                                                       const void *d_values, ohmhip_voxel_edit_stats *stats);
int ohmhip_map_integrate_voxels(ohmhip_map_t map, const uint8_t *ops /* NULL: every element is `op` */, int op,
                                const void *keys10 /* or NULL */, const double *points_xyz /* or NULL */, size_t count,
                                ohmhip_voxel_edit_stats *stats /* optional */);
OHMHIP_EXPERIMENTAL int ohmhip_map_integrate_voxels_device(ohmhip_map_t map, const uint8_t *d_ops, int op,
                                                           const void *d_keys10, const double *d_points_xyz,
                                                           size_t count, ohmhip_voxel_edit_stats *stats);

/* LAYER CHANGES.  OccupancyMap::updateLayout(new_layout, preserve_map) and the add*Layer calls built on it
 * (ohm/OccupancyMap.cpp:521-682, MapChunk::updateLayout ohm/MapChunk.cpp:93-143) on a live device map: the layer set
 * given to ohmhip_map_create changes, the voxels of the layers in both sets stay where they are.  `layers` is a mask of
 * OHMHIP_LAYER_BIT values; the map's mode never changes here.  tests/layout_ref.py restates the chunk and the store
 * record rules on the CPU.
 *  U1 order: the map is settled first, as every observer does it: rays collected from earlier calls are launched --
 *     under the OLD layer set -- and an asynchronous launch is finished.  The call is blocking.  Batches presented
 *     afterwards see the new set.
 *  U2 content: every region the map holds -- resident, in the host store (SPILL TO HOST), every tile of a tiled region
 *     (LARGE REGIONS) -- keeps, byte for byte, its block of every layer in both sets.  Every added layer holds its clear
 *     value in every region (+inf for occupancy, -1 for clearance, 0 otherwise), and in every unassigned slot, so a
 *     region created later starts cleared.  A removed layer's memory is released: removing a layer and adding it again
 *     yields a cleared layer, never the old bytes.  Afterwards the map behaves through every entry point like a map
 *     created with the new set that received the common layers' blocks through ohmhip_map_write_regions -- the
 *     ordered-replay mask of an NDT or TSDF map included, which is untouched.
 *  U3 no copy of what stays: for every retained layer ohmhip_map_device_layer_ptr returns the same pointer and stride
 *     before and after.  Beyond the added layers and the scratch tied to them (the traversal layer's accumulator) the
 *     call takes no device memory proportional to the map.  Everything new is allocated before anything old is
 *     released: a failed allocation leaves the map exactly as it was, OHMHIP_ERR_CAPACITY with all of *stats zero.
 *  U4 host store: the record layout follows the set.  Every record in use is rewritten into the new layout -- common
 *     layers and the mask row copied, added layers cleared, the region's dirty bits and use stamp kept; the
 *     write-back's pre-cleaned copies are void; free records of the old size are not handed out again.
 *  U5 memory limit: the cost of a region (ohmhip_cache_stats::bytes_per_region) follows the new set.  If the resident
 *     regions no longer fit the limit and spilling is on, the regions the spill policy would evict next move to the
 *     store first (counted in regions_evicted); with spilling off: OHMHIP_ERR_CAPACITY, map unchanged.  The pool keeps
 *     its slots (U3); the batches that follow keep no more regions resident than the limit is worth under the new set,
 *     until ohmhip_map_set_memory_limit sets a limit anew.
 *  U6 bookkeeping: dirty bits are unchanged.  Adding the clearance layer leaves every region unwritten: all regions are
 *     stale for ohmhip_map_clearance_stale_regions; removing it forgets that bookkeeping.  Adding the traversal layer
 *     allocates its accumulator, zeroed; removing the layer frees it.
 *  U7 required layers, OHMHIP_ERR_UNSUPPORTED if any would go: OHMHIP_MODE_OCCUPANCY occupancy; OHMHIP_MODE_NDT_OM
 *     occupancy, mean, covariance; OHMHIP_MODE_NDT_TM those and intensity, hit / miss; OHMHIP_MODE_TSDF TSDF.  Also
 *     OHMHIP_ERR_UNSUPPORTED: a map with region ownership or a partition, and a map with replica merge enabled.
 *  U8 OHMHIP_ERR_INVALID_ARG, before any device work, for a null map, a bit at or above OHMHIP_LID_COUNT, layers == 0,
 *     an unknown flag, and a null `layers` pointer in the getter.  The mask the map has already is OHMHIP_OK and does
 *     nothing beyond U1: the pointers are unchanged.
 *  U9 OHMHIP_LAYOUT_DISCARD_MAP: the map is cleared as ohmhip_map_clear does it and takes the new set: the result of
 *     updateLayout(..., false).
 *  U10 a failed call of any kind leaves the layers, regions, dirty bits, store and statistics as they were (under U5 a
 *     call that fails after its evictions leaves those regions in the store: they are still the map's). */
#define OHMHIP_LAYOUT_DISCARD_MAP 1u /* updateLayout(..., preserve_map = false) */
typedef struct ohmhip_layer_change_stats
{
  unsigned layers_before, layers_after;        /* OHMHIP_LAYER_BIT masks */
  uint64_t regions_resident, regions_in_store; /* after the call */
  uint64_t regions_evicted;                    /* moved to the host store to stay inside the memory limit */
  uint64_t bytes_per_region_before, bytes_per_region_after; /* what a resident region costs against the limit */
} ohmhip_layer_change_stats;
OHMHIP_EXPERIMENTAL int ohmhip_map_update_layers(ohmhip_map_t map, unsigned layers, unsigned flags,
                                                 ohmhip_layer_change_stats *stats /* optional */);
OHMHIP_EXPERIMENTAL int ohmhip_map_layers(ohmhip_map_t map, unsigned *layers);

/* Multi-GPU merge support (no reference equivalent -- ohm is single device).  The resident layer of a
 * map is one allocation of region_stride_bytes per slot: ohm_amd/distributed.py wraps it as a device tensor and runs
 * the RCCL all-reduce of touched-region occupancy deltas on it.  ensure_regions makes regions resident (cleared)
 * without touching their data and returns their slots; mark_dirty flags slots for the next syncVoxels(). */
int ohmhip_map_device_layer_ptr(ohmhip_map_t map, int layer_id, void **device_ptr, size_t *region_stride_bytes);
int ohmhip_map_region_slot(ohmhip_map_t map, const int16_t key_xyz[3], uint32_t *slot);
int ohmhip_map_ensure_regions(ohmhip_map_t map, const int16_t *keys_xyz, size_t count, uint32_t *slots);
int ohmhip_map_mark_dirty(ohmhip_map_t map, const uint32_t *slots, size_t count);

/* Exact multi-GPU integration, "owner computes" (SURVEY 8e mode 2: map partitioned by region; no reference equivalent).
 * With world_size > 1 the map integrates only what falls in regions ohmhip_region_owner() assigns to `rank`: the ray
 * segments crossing those regions and the samples landing in them.  Every voxel's update sequence depends only on the
 * rays that reach it, in order, so when each of world_size maps is given the SAME ray stream the union of their
 * regions is bit-identical to one map integrating that stream (tests/test_gpu_owner_computes.py); what the ranks
 * exchange is rays (an all-gather), never voxels.  Regions are dealt to ranks by a hash of their block of
 * 2^block_shift regions per axis.  Set before the first integrate call; world_size <= 1 turns the filter off.
 * ohmhip_batch_stats::visits keeps counting the voxels of the presented rays, owned or not. */
int ohmhip_map_set_region_ownership(ohmhip_map_t map, uint32_t world_size, uint32_t rank, int block_shift);
int ohmhip_region_owner(const int16_t *keys_xyz, size_t count, int block_shift, uint32_t world_size,
                        uint32_t *owners);

/* ------------------------------------------------------------------------------------------------------------------
 * Partitioned map (north_star: "ray batches shard by sensor-origin region across GPUs"; no reference
 * equivalent -- ohm is single device).  The exact multi-GPU mode, and what `bench.py --gpus N` runs: every rank owns a
 * TERRITORY of region blocks and holds only those regions; rays travel to the owners of the regions they cross (48 B
 * per routed ray over RCCL -- voxels never cross a link), and every rank integrates the rays addressed to it in
 * (source rank, ray) order.  The union of the ranks' regions is bit-identical to one map integrating rank 0's batch,
 * then rank 1's, ... -- for every map type, clamps included (tests/test_gpu_partitioned.py).  One RayFlag is refused on
 * a partitioned map (OHMHIP_ERR_UNSUPPORTED): OHMHIP_RF_STOP_ON_FIRST_OCCUPIED, whose effect on a voxel depends on voxels
 * other ranks own.
 *
 * ohmhip_map_set_region_partition: like ohmhip_map_set_region_ownership, but the blocks of 2^block_shift regions per
 * axis are dealt by a TABLE (x fastest) over [grid_origin, grid_origin + grid_dims) in block coordinates (region
 * coordinate >> block_shift); blocks outside the grid belong to the owner of the nearest cell, so territories that reach
 * the table's edge extend outwards without limit.  grid_dims = {0,0,0} / owners = NULL: the block hash of
 * ohmhip_region_owner.  The table is copied.  Only on an empty map.  world_size <= 64.
 * ohmhip_map_region_owners: owners under the map's current partition (host evaluation).
 * ohmhip_map_route_rays: for `ray_count` rays in DEVICE memory (6 doubles each) find, per ray, the ranks owning a
 * region its walk touches or its sample lands in -- exactly, with the functions the integration itself runs (rays the
 * map's ray filter rejects go nowhere) -- and compact the rays per destination, in ray order, into d_routed
 * (destination d's block starts at counts[0] + .. + counts[d-1]); d_routed_index (may be NULL) receives each routed
 * ray's index in the input, for callers that route side arrays (time stamps, intensities) themselves.  counts (host,
 * world_size entries) = rays per destination; *visits (may be NULL) = voxel visits of the input rays.  Returns
 * OHMHIP_ERR_CAPACITY -- with counts valid -- when d_routed holds fewer than sum(counts) rays: grow and repeat.
 * Synchronous, on a stream of its own: it reads nothing a batch writes, so it runs beside the batches in flight (the
 * next batch is routed and exchanged while the previous one integrates).
 * ohmhip_comm_exchange_counts / _rays: the all-to-all of the routed rays over RCCL (both collective).  First the counts
 * (recv_counts[s] = rays rank s addressed to this rank), then, with d_recv holding sum(recv_counts) rays, the blocks:
 * on return (stream order) d_recv holds the rays addressed to this rank in source-rank order, ready for
 * ohmhip_map_integrate_rays_device.  A torch.distributed all_to_all_single does the same job for Python hosts
 * (ohm_amd/distributed.py: PartitionedIntegrator). */
typedef struct ohmhip_partition
{
  uint32_t world_size;
  uint32_t rank;
  int32_t block_shift;
  int32_t grid_origin[3];
  uint32_t grid_dims[3];
  const uint8_t *owners;
} ohmhip_partition;
int ohmhip_map_set_region_partition(ohmhip_map_t map, const ohmhip_partition *partition);
int ohmhip_map_region_owners(ohmhip_map_t map, const int16_t *keys_xyz, size_t count, uint32_t *owners);
/* The same rule for a partition description alone (no map, no device): what hosts use to plan and check a table. */
int ohmhip_partition_owners(const ohmhip_partition *partition, const int16_t *keys_xyz, size_t count, uint32_t *owners);
int ohmhip_map_route_rays(ohmhip_map_t map, const double *d_rays, size_t ray_count, unsigned ray_flags, double *d_routed,
                          uint32_t *d_routed_index, size_t capacity, uint32_t *counts, uint64_t *visits);

/* ------------------------------------------------------------------------------------------------------------------
 * Replica merge (SURVEY 8e mode 1: every GPU integrates the rays of its own sensor origins into its own resident map;
 * regions touched by more than one GPU are reconciled on demand).  No reference equivalent -- ohm is single device.
 *
 * Rule, per voxel of the occupancy layer, relative to the state `base` all replicas shared after the previous merge:
 *     merged = clamp(base + sum over ranks of (value_r - base), min, max)
 * (+inf == unobserved counts as 0 and stays unobserved only if no rank observed the voxel).  That equals integrating the
 * ranks' rays one rank after the other wherever no min / max clamp engaged in between -- log-odds updates commute until
 * they saturate -- and is the usual order-free map-merge value where one did.  Exact multi-GPU integration is the
 * region-ownership mode above.  Other layers are not additive and stay per replica.
 *
 * ohmhip_map_enable_merge() gives the map a base copy of its occupancy layer (current content == base) and starts
 * tracking the regions modified since.  INVARIANT: `base` of a region is the same on every rank (a rank that does not
 * hold the region == base unobserved).  It changes only when the region is EXCHANGED, and then on every rank (a rank
 * that never touched the region creates it and receives the merged tile).  A region that only one rank modified is
 * not exchanged in OHMHIP_MERGE_SHARED_ONLY mode (the default): it stays PENDING on that rank -- listed by
 * merge_keys in every later round, its base untouched -- until a second rank lists it too; then the owner's whole
 * pending delta travels.  (Round 2 rebased such regions locally, which made `base` rank-private and later exchanges
 * wrong on the peers.)  So after a merge: an exchanged region is bit-identical on all ranks; a pending region is
 * exact on its one rank and absent / at its last exchanged value elsewhere.  OHMHIP_MERGE_FULL_UNION exchanges every
 * pending region of any rank: all replicas are then bit-identical maps after every merge, at the price of moving
 * the tiles only one rank needed.
 *
 * The merge itself is either one call over RCCL (ohmhip_map_merge_replicas: region key lists are all-gathered, the
 * delta tiles of the agreed region list are all-reduced -- 5 bytes per voxel: float delta summed + observer flag by
 * max --, everything on the map's stream; the ranks agree on the outcome of their local steps with a one-word
 * all-reduce BEFORE the tile all-reduce, so a rank-local failure makes every rank return together: the failing rank its
 * own error, the others OHMHIP_ERR_PEER, nothing applied, all regions still pending) or, for any other transport, the
 * steps it is made of: ohmhip_map_merge_keys -> (exchange keys, agree on the ordered region list) ->
 * ohmhip_map_merge_pack -> (sum the deltas / max the observer flags across ranks) -> ohmhip_map_merge_apply. */
#define OHMHIP_MERGE_SHARED_ONLY 0
#define OHMHIP_MERGE_FULL_UNION 1
typedef struct ohmhip_comm_s *ohmhip_comm_t;
#define OHMHIP_COMM_ID_BYTES 128
int ohmhip_comm_unique_id(unsigned char id[OHMHIP_COMM_ID_BYTES]);  /* ncclGetUniqueId; hand it to every rank */
/* ncclCommInitRank on the calling thread's current device (collective: every rank calls it with the same id). */
int ohmhip_comm_init_rank(ohmhip_comm_t *comm, const unsigned char id[OHMHIP_COMM_ID_BYTES], int world_size, int rank);
int ohmhip_comm_destroy(ohmhip_comm_t comm);
/* Partitioned map: the all-to-all of routed rays (see "Partitioned map" above). */
/* FAILURE AGREEMENT: a rank that cannot take part in the step (its routing failed, it is out of memory ...) still calls
 * ohmhip_comm_exchange_counts, with OHMHIP_COUNT_FAILED in every send count: the call then returns OHMHIP_ERR_PEER on
 * EVERY rank (recv_counts zeroed) and no rank enters the payload exchange -- all ranks leave the step together.  A failure
 * after the exchange (the integration of what arrived) is local: the failing rank's caller has to end the group's run. */
#define OHMHIP_COUNT_FAILED 0xffffffffu
int ohmhip_comm_exchange_counts(ohmhip_comm_t comm, const uint32_t *send_counts, uint32_t *recv_counts,
                                ohmhip_stream_t stream);
int ohmhip_comm_exchange_rays(ohmhip_comm_t comm, const double *d_send, const uint32_t *send_counts, double *d_recv,
                              const uint32_t *recv_counts, ohmhip_stream_t stream);
/* The routed rays' SIDE ARRAYS (round 5) -- the time stamps and intensities the reference passes with every batch
 * (ohmgpu/GpuMap.cpp:416; GpuNdtMap.cpp:433-486: NDT-TM needs the intensities, a touch-time layer the stamps) travel the
 * same way: ohmhip_gather_rows puts an array into routed order with the index list ohmhip_map_route_rays returns
 * (d_dst[i] = d_src[d_index[i]], rows of bytes_per_row bytes, device pointers, stream order), and
 * ohmhip_comm_exchange_side is the all-to-all of ohmhip_comm_exchange_rays for bytes_per_ray bytes per ray with the
 * same counts.  Both exchange calls validate their arguments before the collective starts: an invalid call returns
 * OHMHIP_ERR_INVALID_ARG without having taken part in it. */
int ohmhip_comm_exchange_side(ohmhip_comm_t comm, const void *d_send, const uint32_t *send_counts, void *d_recv,
                              const uint32_t *recv_counts, uint32_t bytes_per_ray, ohmhip_stream_t stream);
int ohmhip_gather_rows(const void *d_src, const uint32_t *d_index, size_t count, uint32_t bytes_per_row, void *d_dst,
                       ohmhip_stream_t stream);

typedef struct ohmhip_merge_stats
{
  uint32_t regions_local;   /* regions pending on this rank (modified since they were last exchanged)  */
  uint32_t regions_union;   /* ... any rank did                                                       */
  uint32_t regions_shared;  /* the ones whose tiles travel (pending on > 1 rank; all in FULL_UNION)    */
  uint64_t payload_bytes;   /* bytes this rank contributed to the tile all-reduce (5 per shared voxel) */
  uint64_t key_bytes;       /* bytes it contributed to the key all-gather                              */
  float ms_total;           /* host wall time of the call                                              */
} ohmhip_merge_stats;

int ohmhip_map_enable_merge(ohmhip_map_t map);
int ohmhip_map_set_merge_mode(ohmhip_map_t map, int mode);
/* Collective over `comm`.  On return every rank holds the merged values of the exchanged regions, which become the new
 * base on every rank. */
int ohmhip_map_merge_replicas(ohmhip_map_t map, ohmhip_comm_t comm, ohmhip_merge_stats *stats);
/* The steps, for other transports.  merge_keys: keys (int16 x 3 each) of the PENDING regions -- modified since they were
 * last exchanged --, at most `capacity` written, *count = how many there are.  merge_pack: for `count` regions in the
 * given order (made resident if they are not) write count x region_voxels float deltas and uint8 observer flags to the
 * DEVICE buffers.  merge_apply: the same regions with the deltas summed / flags max-ed (or summed) over all ranks; EVERY
 * rank applies every exchanged region.  merge_finish: kept for ABI compatibility, nothing left to do. */
int ohmhip_map_merge_keys(ohmhip_map_t map, int16_t *keys_xyz, size_t capacity, size_t *count);
int ohmhip_map_merge_pack(ohmhip_map_t map, const int16_t *keys_xyz, size_t count, float *d_delta,
                          unsigned char *d_observers);
int ohmhip_map_merge_apply(ohmhip_map_t map, const int16_t *keys_xyz, size_t count, const float *d_delta_sum,
                           const unsigned char *d_observer_sum);
int ohmhip_map_merge_finish(ohmhip_map_t map);

#ifdef __cplusplus
}
#endif

#endif /* OHMHIP_H */
