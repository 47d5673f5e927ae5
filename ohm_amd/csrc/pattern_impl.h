// pattern_impl.h -- ohmhip_map_apply_pattern: ClearingPattern::apply (ohm/ClearingPattern.h:109-130) with the pattern's
// rays built on the device (k_pattern_rays, ohmhip_transform.hip) and handed to the device-batch path.  Host code only:
// no kernel of this translation unit changes.
//
// Part of ohmhip_map.hip's translation unit (included there, in order): not a stand-alone header.
#ifndef OHMHIP_PATTERN_IMPL_H
#define OHMHIP_PATTERN_IMPL_H

extern "C" int ohmhip_map_apply_pattern(ohmhip_map_t m, ohmhip_pattern_t pattern, const double *poses, size_t pose_count,
                                        int pose_kind, double scaling, float probability_scaling, unsigned ray_flags,
                                        size_t *integrated)
try
{
  if (integrated)
  {
    *integrated = 0;
  }
  if (!m || !pattern || (!poses && pose_count) || (pose_kind != OHMHIP_POSE_QUAT && pose_kind != OHMHIP_POSE_MAT4))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  size_t ray_count = 0;
  OHMHIP_CHECK(ohmhip_pattern_ray_count(pattern, &ray_count));
  if (pose_count == 0 || ray_count == 0)
  {
    return OHMHIP_OK;
  }
  if (pose_count >= kPatternMaxRays || pose_count * ray_count >= kPatternMaxRays)
  {
    return OHMHIP_ERR_CAPACITY;
  }
  // ClearingPattern.cpp:40-44: a clearing ray is traced forwards so that it can stop at the first obstruction.
  ray_flags &= ~unsigned(OHMHIP_RF_REVERSE_WALK);
  OHMHIP_CHECK(validateBatchRequest(m, ray_flags));
  // Rays collected from earlier calls belong to the unscaled miss value: they are launched first (kernels take MapConst
  // by value at launch), and so is a batch still with the map's launch thread.
  OHMHIP_SETTLE(m);
  // The turn is the number of batches launched so far: a call that launches nothing (a failing batch) does not advance
  // it, and every batch but the two launched last has completed (include/ohmhip.h, ohmhip_map_integrate_rays_device).
  const double *d_rays = nullptr;
  hipEvent_t built = nullptr;
  OHMHIP_CHECK(patternBuildOnStream(pattern, m, m->batch_seq, m->stream, poses, pose_count, pose_kind, scaling, &d_rays,
                                    &built));
  OHMHIP_CHECK(hipStreamWaitEvent(m->front_stream, built, 0));  // (the set-up pass reads the rays first)
  struct MissScope
  {
    ohmhip_map_t m;
    float miss_value;
    ~MissScope() { m->mc.miss_value = miss_value; }
  } miss_scope{ m, m->mc.miss_value };
  m->mc.miss_value = miss_scope.miss_value * probability_scaling;  // ClearingPattern.h:114-115, in fp32
  return integrateRaysDevice(m, d_rays, 2 * pose_count * ray_count, nullptr, nullptr, ray_flags, integrated);
}
OHMHIP_ABI_CATCH

#endif  // OHMHIP_PATTERN_IMPL_H
