// ref_shim_incident.cpp -- exports, through a C ABI, the reference's ohm/VoxelIncidentCompute.h compiled WHERE IT LIES
// (-I/root/reference), in its GPUTIL_DEVICE form: the form the reference's own GPU path compiles.  TEST INFRASTRUCTURE
// ONLY.  No reference source is copied: this file only #includes it.
//
// A translation unit of its own because GPUTIL_DEVICE must not reach the headers ref_shim.cpp includes.  The host form
// of the header names glm::vec3, and glm is not installed here; the device form needs only a `float3` with x, y, z and
// operator*=(float), unqualified max / min / sqrt, and the two CUDA-style function attributes.  Those few lines follow;
// none of them is a stand-in for glm.
#include <algorithm>
#include <cmath>

struct float3
{
  float x, y, z;
  float3 &operator*=(float s)
  {
    x *= s;
    y *= s;
    z *= s;
    return *this;
  }
};
using std::max;
using std::min;
inline float sqrt(float v)
{
  return std::sqrt(v);
}
#define __device__
#define __host__
#define GPUTIL_DEVICE 1

#include <ohm/VoxelIncidentCompute.h>  // decodeNormal, encodeNormal, updateIncidentNormal

extern "C" {
void ref_decode_normal(unsigned packed, float out[3])
{
  const float3 n = decodeNormal(packed);
  out[0] = n.x;
  out[1] = n.y;
  out[2] = n.z;
}
unsigned ref_encode_normal(const float normal[3]) { return encodeNormal(float3{ normal[0], normal[1], normal[2] }); }
unsigned ref_update_incident_normal(unsigned packed, const float incident_ray[3], unsigned point_count)
{
  return updateIncidentNormal(packed, float3{ incident_ray[0], incident_ray[1], incident_ray[2] }, point_count);
}
}
