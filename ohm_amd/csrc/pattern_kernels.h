// pattern_kernels.h -- k_pattern_rays: a resident ray pattern moved to a batch of poses (RayPattern::buildRays,
// ohm/RayPattern.cpp:58-84), fp64 in the operation order include/ohmhip.h states under RAY PATTERNS and
// tests/ray_pattern_ref.py models: one rounding per operation (the build has -ffp-contract=off), no libm call.
//
// Part of ohmhip_transform.hip's translation unit: the integration kernels' translation unit does not see it.
#ifndef OHMHIP_PATTERN_KERNELS_H
#define OHMHIP_PATTERN_KERNELS_H

namespace ohmhip
{
/// glm::cross
__device__ inline void patternCross(const double a[3], const double b[3], double out[3])
{
  out[0] = a[1] * b[2] - b[1] * a[2];
  out[1] = a[2] * b[0] - b[2] * a[0];
  out[2] = a[0] * b[1] - b[0] * a[1];
}

/// One lane per output point (pose, pattern point).  points: 3 doubles per pattern point (2 points per ray); poses: 7
/// (translation xyz, rotation xyzw) or 16 (column-major mat4) doubles per pose; out: pose major in pattern order, so
/// that consecutive lanes write consecutive addresses.  point_count * pose_count < 2^29 (checked by the callers).
__global__ void __launch_bounds__(256)
  k_pattern_rays(const double *__restrict__ points, uint32_t point_count, const double *__restrict__ poses,
                 uint32_t pose_count, int pose_kind, double scaling, double *__restrict__ out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= point_count * pose_count)
  {
    return;
  }
  const uint32_t pose_index = i / point_count;
  const uint32_t point_index = i - pose_index * point_count;
  const double *p = points + 3 * size_t(point_index);
  const double s[3] = { scaling * p[0], scaling * p[1], scaling * p[2] };
  double *o = out + 3 * size_t(i);
  if (pose_kind == OHMHIP_POSE_QUAT)
  {
    const double *pose = poses + 7 * size_t(pose_index);
    const double u[3] = { pose[3], pose[4], pose[5] };
    const double w = pose[6];
    double uv[3], uuv[3];
    patternCross(u, s, uv);
    patternCross(u, uv, uuv);
#pragma unroll
    for (int a = 0; a < 3; ++a)
    {
      o[a] = (s[a] + ((uv[a] * w) + uuv[a]) * 2.0) + pose[a];
    }
  }
  else
  {
    const double *m = poses + 16 * size_t(pose_index);
#pragma unroll
    for (int r = 0; r < 3; ++r)
    {
      o[r] = (m[0 + r] * s[0] + m[4 + r] * s[1]) + (m[8 + r] * s[2] + m[12 + r]);
    }
  }
}
}  // namespace ohmhip

#endif  // OHMHIP_PATTERN_KERNELS_H
