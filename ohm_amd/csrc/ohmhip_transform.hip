// ohmhip_transform.hip -- GpuTransformSamples equivalent: sensor-frame samples + a timestamped trajectory in, world-frame
// ray pairs (sensor origin, sample) out, resident on the device and ready for ohmhip_map_integrate_rays_device().
//
// Semantics follow ohmgpu/GpuTransformSamples.cpp:97-210 (host side: sample filter, compaction) and
// ohmgpu/gpu/TransformSamples.cl:13-228 (kernel: bracketing search, lerp of the translation, the reference's rotation
// rule rot[from] * slerp(rot[from], rot[to], f)), in fp64 throughout -- the reference kernel is fp32 only because it had
// to run on devices without doubles (it rebases the time stamps to keep them representable).
#include "ohmhip_internal.h"

#include <hip/hip_runtime.h>

#include <string.h>

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <memory>

#include "pattern_kernels.h"

namespace ohmhip
{
struct Quat
{
  double x, y, z, w;
};

/// TransformSamples.cl:13-54
__device__ inline Quat slerp(const Quat &from, const Quat &to, double f)
{
  if (from.x == to.x && from.y == to.y && from.z == to.z && from.w == to.w)
  {
    return from;
  }
  double cos_angle = ((from.x * to.x + from.y * to.y) + from.z * to.z) + from.w * to.w;
  Quat temp = to;
  if (!(cos_angle >= 0))
  {
    temp.x = -1.0 * to.x;
    temp.y = -1.0 * to.y;
    temp.z = -1.0 * to.z;
    temp.w = -1.0 * to.w;
    cos_angle = -1.0 * cos_angle;
  }
  double coeff0, coeff1;
  if (1.0 - cos_angle > 1e-12)
  {
    const double angle = acos(cos_angle);
    const double inv_sin = 1.0 / sin(angle);
    coeff0 = sin((1.0 - f) * angle) * inv_sin;
    coeff1 = sin(f * angle) * inv_sin;
  }
  else
  {
    coeff0 = 1.0 - f;
    coeff1 = f;
  }
  Quat r;
  r.x = coeff0 * from.x + coeff1 * temp.x;
  r.y = coeff0 * from.y + coeff1 * temp.y;
  r.z = coeff0 * from.z + coeff1 * temp.z;
  r.w = coeff0 * from.w + coeff1 * temp.w;
  return r;
}

/// TransformSamples.cl:57-65
__device__ inline Quat quatMul(const Quat &a, const Quat &b)
{
  Quat q;
  q.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  q.y = a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x;
  q.z = a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w;
  q.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  return q;
}

/// ohmgpu/GpuTransformSamples.cpp:47-60 (goodSample).  As in the reference the SQUARED length is compared with
/// max_range itself.
__global__ void __launch_bounds__(256)
  k_sample_flags(const double *__restrict__ local, uint32_t n, double max_range, uint32_t *__restrict__ good)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n)
  {
    return;
  }
  const double x = local[3 * size_t(i)], y = local[3 * size_t(i) + 1], z = local[3 * size_t(i) + 2];
  const bool nan = (x != x) || (y != y) || (z != z);
  const bool far = ((x * x + y * y) + z * z) > max_range;
  good[i] = (!nan && !far) ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
  k_transform_samples(const double *__restrict__ times, const double *__restrict__ positions,
                      const double *__restrict__ rotations, uint32_t transform_count,
                      const double *__restrict__ sample_times, const double *__restrict__ local, uint32_t n,
                      const uint32_t *__restrict__ good, const uint32_t *__restrict__ slot, double *__restrict__ out)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !good[i])
  {
    return;
  }
  double sample_time = sample_times[i];
  // TransformSamples.cl:128-196: the pair of transforms bracketing the sample time.
  uint32_t from = 0;
  uint32_t to = transform_count - 1;
  if (transform_count > 2)
  {
    if (times[0] <= sample_time && sample_time <= times[transform_count - 1])
    {
      uint32_t iterations = 0;
      while (from <= to && iterations < 100000u)
      {
        ++iterations;
        const uint32_t mid_low = (from + to) / 2;
        const uint32_t mid_high = min(mid_low + 1, transform_count - 1);
        if (sample_time >= times[mid_low] && sample_time <= times[mid_high])
        {
          from = mid_low;
          to = mid_high;
          break;
        }
        else if (sample_time <= times[mid_low])
        {
          to = mid_low - 1;
        }
        else
        {
          from = mid_low + 1;
        }
      }
    }
    else if (sample_time < times[0])
    {
      sample_time = times[0];
      from = to = 0;
    }
    else
    {
      sample_time = times[transform_count - 1];
      from = to = transform_count - 1;
    }
  }
  // A sample outside the trajectory takes the end pose (the reference divides 0 / 0 there and emits NaN rays).
  const double span = times[to] - times[from];
  const double f = (span != 0) ? (sample_time - times[from]) / span : 0.0;
  double position[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
  {
    position[a] = positions[3 * size_t(from) + a] + f * (positions[3 * size_t(to) + a] - positions[3 * size_t(from) + a]);
  }
  Quat qf, qt;
  qf.x = rotations[4 * size_t(from) + 0];
  qf.y = rotations[4 * size_t(from) + 1];
  qf.z = rotations[4 * size_t(from) + 2];
  qf.w = rotations[4 * size_t(from) + 3];
  qt.x = rotations[4 * size_t(to) + 0];
  qt.y = rotations[4 * size_t(to) + 1];
  qt.z = rotations[4 * size_t(to) + 2];
  qt.w = rotations[4 * size_t(to) + 3];
  const Quat q = quatMul(qf, slerp(qf, qt, f));
  // TransformSamples.cl:68-91
  const double vx = local[3 * size_t(i)], vy = local[3 * size_t(i) + 1], vz = local[3 * size_t(i) + 2];
  const double xx = q.x * q.x, xy = q.x * q.y, xz = q.x * q.z, xw = q.x * q.w;
  const double yy = q.y * q.y, yz = q.y * q.z, yw = q.y * q.w;
  const double zz = q.z * q.z, zw = q.z * q.w;
  const double rx = (1 - 2 * (yy + zz)) * vx + (2 * (xy - zw)) * vy + (2 * (xz + yw)) * vz;
  const double ry = (2 * (xy + zw)) * vx + (1 - 2 * (xx + zz)) * vy + (2 * (yz - xw)) * vz;
  const double rz = (2 * (xz - yw)) * vx + (2 * (yz + xw)) * vy + (1 - 2 * (xx + yy)) * vz;
  double *o = out + 6 * size_t(slot[i]);
  o[0] = position[0];
  o[1] = position[1];
  o[2] = position[2];
  o[3] = position[0] + rx;
  o[4] = position[1] + ry;
  o[5] = position[2] + rz;
}
}  // namespace ohmhip

using namespace ohmhip;

extern "C" int ohmhip_transform_samples(const double *transform_times, const double *transform_translations,
                                        const double *transform_rotations_xyzw, uint32_t transform_count,
                                        const double *sample_times, const double *local_samples, uint32_t point_count,
                                        double max_range, ohmhip_stream_t stream, ohmhip_buffer_t output,
                                        uint32_t *ray_elements)
try
{
  if (ray_elements)
  {
    *ray_elements = 0;
  }
  if (!output || (point_count && (!sample_times || !local_samples)) ||
      (transform_count && (!transform_times || !transform_translations || !transform_rotations_xyzw)))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (point_count == 0 || transform_count == 0)
  {
    return OHMHIP_OK;  // GpuTransformSamples.cpp:103-106
  }
  hipStream_t s = stream ? stream->stream : nullptr;
  size_t actual = 0;
  int status = ohmhip_buffer_resize(output, sizeof(double) * 6 * size_t(point_count), &actual);
  if (status)
  {
    return status;
  }
  const size_t tn = transform_count, pn = point_count;
  const size_t bytes_d = sizeof(double) * (8 * tn + 4 * pn);
  double *d_d = nullptr;
  uint32_t *d_u = nullptr;
  void *d_temp = nullptr;
  auto cleanup = [&]() {
    (void)hipFree(d_d);
    (void)hipFree(d_u);
    (void)hipFree(d_temp);
  };
  if ((status = hipMalloc(reinterpret_cast<void **>(&d_d), bytes_d)) != 0 ||
      (status = hipMalloc(reinterpret_cast<void **>(&d_u), sizeof(uint32_t) * (2 * pn + 1))) != 0)
  {
    cleanup();
    return status;
  }
  double *d_times = d_d, *d_pos = d_times + tn, *d_rot = d_pos + 3 * tn, *d_stimes = d_rot + 4 * tn;
  double *d_local = d_stimes + pn;
  uint32_t *d_good = d_u, *d_slot = d_u + pn;
  auto up = [&](double *dst, const double *src, size_t count) {
    return int(hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyHostToDevice, s));
  };
  status = up(d_times, transform_times, tn);
  status = status ? status : up(d_pos, transform_translations, 3 * tn);
  status = status ? status : up(d_rot, transform_rotations_xyzw, 4 * tn);
  status = status ? status : up(d_stimes, sample_times, pn);
  status = status ? status : up(d_local, local_samples, 3 * pn);
  if (status)
  {
    cleanup();
    return status;
  }
  const dim3 grid(uint32_t((pn + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_sample_flags, grid, block, 0, s, d_local, point_count, max_range, d_good);
  // Stable compaction of the rejected samples (the reference skips them while staging, GpuTransformSamples.cpp:131-142).
  size_t temp_bytes = 0;
  status = int(rocprim::exclusive_scan(nullptr, temp_bytes, d_good, d_slot, 0u, pn, rocprim::plus<uint32_t>(), s));
  if (!status)
  {
    status = int(hipMalloc(&d_temp, temp_bytes));
  }
  if (!status)
  {
    status = int(rocprim::exclusive_scan(d_temp, temp_bytes, d_good, d_slot, 0u, pn, rocprim::plus<uint32_t>(), s));
  }
  if (!status)
  {
    void *out_ptr = nullptr;
    (void)ohmhip_buffer_ptr(output, &out_ptr);
    hipLaunchKernelGGL(k_transform_samples, grid, block, 0, s, d_times, d_pos, d_rot, transform_count, d_stimes, d_local,
                       point_count, d_good, d_slot, static_cast<double *>(out_ptr));
    uint32_t tail[2] = { 0, 0 };
    status = int(hipMemcpyAsync(&tail[0], d_good + (pn - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    status = status ? status : int(hipMemcpyAsync(&tail[1], d_slot + (pn - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    status = status ? status : int(hipStreamSynchronize(s));
    if (!status && ray_elements)
    {
      *ray_elements = 2u * (tail[0] + tail[1]);
    }
  }
  cleanup();
  return status;
}
OHMHIP_ABI_CATCH

// ---- Ray patterns (include/ohmhip.h, RAY PATTERNS) ---------------------------------------------------------------------

/// A ray pattern resident on the device: its points, and the buffers its applications write.
struct ohmhip_pattern_s
{
  /// Where one application's rays go, with the poses that produced them: the pinned block the caller's poses are
  /// copied to and its device copy.
  struct Output
  {
    double *d_rays = nullptr;
    size_t ray_bytes = 0;
    double *d_poses = nullptr;
    double *h_poses = nullptr;
    size_t pose_bytes = 0;
    uint64_t turn = ~uint64_t(0);  ///< the turn that last wrote it
  };
  static constexpr int kTurnOutputs = 3;  ///< [0, 3): taken in turn by the batches of a map; [3]: ohmhip_pattern_build_rays

  size_t ray_count = 0;
  double *d_points = nullptr;
  Output out[kTurnOutputs + 1];
  const void *user = nullptr;
  hipEvent_t built = nullptr;
  const double *last = nullptr;
  size_t last_elements = 0;

  ~ohmhip_pattern_s()
  {
    (void)hipDeviceSynchronize();  // (batches in flight may still read the outputs)
    for (Output &o : out)
    {
      (void)hipFree(o.d_rays);
      (void)hipFree(o.d_poses);
      (void)hipHostFree(o.h_poses);
    }
    (void)hipFree(d_points);
    if (built)
    {
      (void)hipEventDestroy(built);
    }
  }
};

namespace
{
inline size_t poseDoubles(int pose_kind)
{
  return pose_kind == OHMHIP_POSE_QUAT ? 7u : 16u;
}

/// Build into `o` on `stream`.  The caller has made sure nothing reads `o` any more.
int patternBuild(ohmhip_pattern_t p, ohmhip_pattern_s::Output &o, hipStream_t stream, const double *poses,
                 size_t pose_count, int pose_kind, double scaling)
{
  const size_t pose_bytes = sizeof(double) * poseDoubles(pose_kind) * pose_count;
  const size_t ray_bytes = sizeof(double) * 6 * p->ray_count * pose_count;
  if (o.pose_bytes < pose_bytes)
  {
    (void)hipFree(o.d_poses);
    (void)hipHostFree(o.h_poses);
    o.d_poses = o.h_poses = nullptr;
    o.pose_bytes = 0;
    const size_t want = std::max<size_t>(pose_bytes + pose_bytes / 2, 1024);
    OHMHIP_CHECK(hipHostMalloc(reinterpret_cast<void **>(&o.h_poses), want, hipHostMallocDefault));
    OHMHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&o.d_poses), want));
    o.pose_bytes = want;
  }
  if (o.ray_bytes < ray_bytes)
  {
    (void)hipFree(o.d_rays);
    o.d_rays = nullptr;
    o.ray_bytes = 0;
    OHMHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&o.d_rays), ray_bytes));
    o.ray_bytes = ray_bytes;
  }
  memcpy(o.h_poses, poses, pose_bytes);
  OHMHIP_CHECK(hipMemcpyAsync(o.d_poses, o.h_poses, pose_bytes, hipMemcpyHostToDevice, stream));
  const uint32_t points = uint32_t(2 * p->ray_count), n_poses = uint32_t(pose_count);
  const size_t lanes = size_t(points) * n_poses;  // < 2^29
  hipLaunchKernelGGL(k_pattern_rays, dim3(uint32_t((lanes + 255) / 256)), dim3(256), 0, stream, p->d_points, points,
                     o.d_poses, n_poses, pose_kind, scaling, o.d_rays);
  OHMHIP_CHECK(hipGetLastError());
  OHMHIP_CHECK(hipEventRecord(p->built, stream));
  p->last = o.d_rays;
  p->last_elements = lanes;
  return OHMHIP_OK;
}
}  // namespace

int ohmhip::patternBuildOnStream(ohmhip_pattern_t p, const void *user, uint64_t turn, hipStream_t stream,
                                 const double *poses, size_t pose_count, int pose_kind, double scaling,
                                 const double **d_rays, hipEvent_t *built)
{
  ohmhip_pattern_s::Output &o = p->out[turn % ohmhip_pattern_s::kTurnOutputs];
  if (p->user != user)
  {
    // Another map's batches may still read what its turns wrote.
    OHMHIP_CHECK(hipDeviceSynchronize());
    p->user = user;
  }
  else if (o.turn == turn)
  {
    // The turn did not advance: the application that took it launched no batch.  Its pose copy may still be queued.
    OHMHIP_CHECK(hipStreamSynchronize(stream));
  }
  o.turn = turn;
  OHMHIP_CHECK(patternBuild(p, o, stream, poses, pose_count, pose_kind, scaling));
  *d_rays = o.d_rays;
  *built = p->built;
  return OHMHIP_OK;
}

extern "C" int ohmhip_pattern_create(const double *ray_pairs, size_t ray_count, ohmhip_pattern_t *pattern)
try
{
  if (!pattern || (!ray_pairs && ray_count))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  *pattern = nullptr;
  if (ray_count >= kPatternMaxRays)
  {
    return OHMHIP_ERR_CAPACITY;
  }
  int count = 0;
  const int derr = ohmhip_device_count(&count);
  if (derr || count == 0)
  {
    return derr ? derr : OHMHIP_ERR_NO_DEVICE;
  }
  std::unique_ptr<ohmhip_pattern_s> p(new ohmhip_pattern_s);
  p->ray_count = ray_count;
  OHMHIP_CHECK(hipEventCreateWithFlags(&p->built, hipEventDisableTiming));
  if (ray_count)
  {
    OHMHIP_CHECK(hipMalloc(reinterpret_cast<void **>(&p->d_points), sizeof(double) * 6 * ray_count));
    OHMHIP_CHECK(hipMemcpy(p->d_points, ray_pairs, sizeof(double) * 6 * ray_count, hipMemcpyHostToDevice));
  }
  *pattern = p.release();
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

extern "C" int ohmhip_pattern_destroy(ohmhip_pattern_t pattern)
try
{
  delete pattern;
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

extern "C" int ohmhip_pattern_ray_count(ohmhip_pattern_t pattern, size_t *ray_count)
try
{
  if (!pattern || !ray_count)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  *ray_count = pattern->ray_count;
  return OHMHIP_OK;
}
OHMHIP_ABI_CATCH

extern "C" int ohmhip_pattern_build_rays(ohmhip_pattern_t pattern, const double *poses, size_t pose_count, int pose_kind,
                                         double scaling, double *host_out)
try
{
  if (!pattern || (!poses && pose_count) || (pose_kind != OHMHIP_POSE_QUAT && pose_kind != OHMHIP_POSE_MAT4))
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  if (pose_count == 0 || pattern->ray_count == 0)
  {
    return OHMHIP_OK;
  }
  if (pose_count >= kPatternMaxRays || pose_count * pattern->ray_count >= kPatternMaxRays)
  {
    return OHMHIP_ERR_CAPACITY;
  }
  ohmhip_pattern_s::Output &o = pattern->out[ohmhip_pattern_s::kTurnOutputs];
  OHMHIP_CHECK(patternBuild(pattern, o, nullptr, poses, pose_count, pose_kind, scaling));
  if (host_out)
  {
    OHMHIP_CHECK(hipMemcpyAsync(host_out, o.d_rays, sizeof(double) * 3 * pattern->last_elements, hipMemcpyDeviceToHost,
                                nullptr));
  }
  return int(hipStreamSynchronize(nullptr));
}
OHMHIP_ABI_CATCH

extern "C" int ohmhip_pattern_last_rays(ohmhip_pattern_t pattern, double *host_out, size_t *elements)
try
{
  if (elements)
  {
    *elements = 0;
  }
  if (!pattern || !elements)
  {
    return OHMHIP_ERR_INVALID_ARG;
  }
  *elements = pattern->last_elements;
  if (!host_out || pattern->last_elements == 0)
  {
    return OHMHIP_OK;
  }
  OHMHIP_CHECK(hipEventSynchronize(pattern->built));
  return int(hipMemcpy(host_out, pattern->last, sizeof(double) * 3 * pattern->last_elements, hipMemcpyDeviceToHost));
}
OHMHIP_ABI_CATCH
