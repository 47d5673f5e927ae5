// ray_filter_chain.h -- the stock ray filters of ohm/RayFilter.cpp as stages of a chain, one ray at a time: what
// ohmhip_map_set_ray_filter_stages installs in place of the map's built-in filter.
//
// ONE definition for host and device: k_ray_filter and k_count_passed call it on the device, hostFilterCount on the
// staging threads, the stand-alone check program (scripts/probes/rayfilter_chain_check.cpp) on the host alone.  fp64,
// written operation by operation like the reference, compiled under -ffp-contract=off: every build gives the same
// bits.  Stand-alone: it needs the public header and <math.h>, nothing of the library.
//
// Reference, statement by statement:
//   GOOD            goodRayFilter   ohm/RayFilter.cpp:12-34
//   CLIP            clipRayFilter   ohm/RayFilter.cpp:37-57
//   CLIP_BOUNDED    clipBounded     ohm/RayFilter.cpp:60-77 over Aabb::clipLine (allow_clamp false), Aabb::rayIntersect
//                                   and Aabb::contains (ohm/Aabb.h:301-312, 330-446)
//   CLIP_TO_BOUNDS  clipToBounds    ohm/RayFilter.cpp:80-86
// A chain is what a user writes in a RayFilterFunction lambda as `a(start, end, flags) && b(start, end, flags)`: stage i
// sees the ray as stage i - 1 left it, the flags are OR-ed, the first stage that returns false ends the chain.
#ifndef OHMHIP_RAY_FILTER_CHAIN_H
#define OHMHIP_RAY_FILTER_CHAIN_H

#include "../../include/ohmhip.h"

#include <math.h>

#if defined(__HIPCC__)
#define OHMHIP_RFC_FN __host__ __device__ inline
#else
#define OHMHIP_RFC_FN inline
#endif

namespace ohmhip
{
/// RayFilterFlag, ohm/RayFilter.h:21-29.
enum : unsigned
{
  kRffInvalid = 1u,
  kRffClippedStart = 2u,
  kRffClippedEnd = 4u
};

/// !any(isnan(v)) && !any(isinf(v))
OHMHIP_RFC_FN bool rfcFinite3(const double v[3])
{
  const bool nan = __builtin_isnan(v[0]) || __builtin_isnan(v[1]) || __builtin_isnan(v[2]);
  const bool inf = __builtin_isinf(v[0]) || __builtin_isinf(v[1]) || __builtin_isinf(v[2]);
  return !nan && !inf;
}

/// glm::dot of a dvec3 with itself: the products, then x + y, then + z.
OHMHIP_RFC_FN double rfcDot3(const double v[3])
{
  return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
}

/// Aabb::contains with epsilon 0, i.e. overlaps() with the point as a box: !any(max < p) && !any(min > p).  A NaN
/// coordinate fails both comparisons and so counts as contained -- the reference's form, kept.
OHMHIP_RFC_FN bool rfcContains(const double box_min[3], const double box_max[3], const double p[3])
{
  const bool max_less = box_max[0] < p[0] || box_max[1] < p[1] || box_max[2] < p[2];
  const bool min_greater = box_min[0] > p[0] || box_min[1] > p[1] || box_min[2] > p[2];
  return !max_less && !min_greater;
}

/// Aabb::rayIntersect (ohm/Aabb.h:330-375) with ray_dir_inv = 1.0 / ray_dir per axis (:381).
OHMHIP_RFC_FN bool rfcRayIntersect(const double box_min[3], const double box_max[3], const double origin[3],
                                   const double dir[3], double hit_times[2])
{
  const double inv[3] = { 1.0 / dir[0], 1.0 / dir[1], 1.0 / dir[2] };
  // corners_[sign[a]] / corners_[1 - sign[a]] with sign[a] = dir[a] < 0
  const double near_x = (dir[0] < 0.0) ? box_max[0] : box_min[0];
  const double far_x = (dir[0] < 0.0) ? box_min[0] : box_max[0];
  const double near_y = (dir[1] < 0.0) ? box_max[1] : box_min[1];
  const double far_y = (dir[1] < 0.0) ? box_min[1] : box_max[1];
  const double near_z = (dir[2] < 0.0) ? box_max[2] : box_min[2];
  const double far_z = (dir[2] < 0.0) ? box_min[2] : box_max[2];

  hit_times[0] = (near_x - origin[0]) * inv[0];
  hit_times[1] = (far_x - origin[0]) * inv[0];
  double tmin = (near_y - origin[1]) * inv[1];
  double tmax = (far_y - origin[1]) * inv[1];

  bool miss = (hit_times[0] > tmax) || (tmin > hit_times[1]);

  hit_times[0] = (tmin > hit_times[0] || __builtin_isnan(hit_times[0])) ? tmin : hit_times[0];
  hit_times[1] = (tmax < hit_times[1] || __builtin_isnan(hit_times[1])) ? tmax : hit_times[1];

  tmin = (near_z - origin[2]) * inv[2];
  tmax = (far_z - origin[2]) * inv[2];

  miss = (hit_times[0] > tmax) || (tmin > hit_times[1]) || miss;

  hit_times[0] = (tmin > hit_times[0] || __builtin_isnan(hit_times[0])) ? tmin : hit_times[0];
  hit_times[1] = (tmax < hit_times[1] || __builtin_isnan(hit_times[1])) ? tmax : hit_times[1];

  return !miss;
}

/// Aabb::clipLine (ohm/Aabb.h:386-446), allow_clamp false.  `clip_flags`: 1 start moved, 2 end moved (Aabb::kClipped*).
OHMHIP_RFC_FN bool rfcClipLine(const double box_min[3], const double box_max[3], double start[3], double end[3],
                               unsigned *clip_flags)
{
  const double origin[3] = { start[0], start[1], start[2] };
  double dir[3] = { end[0] - start[0], end[1] - start[1], end[2] - start[2] };
  *clip_flags = 0;
  const double d2 = rfcDot3(dir);
  if (d2 < 1e-9)
  {
    return false;  // degenerate ray
  }
  const double length = sqrt(d2);
  dir[0] = dir[0] / length;
  dir[1] = dir[1] / length;
  dir[2] = dir[2] / length;

  double hit_times[2] = { 0, 0 };
  if (!rfcRayIntersect(box_min, box_max, origin, dir, hit_times))
  {
    return false;
  }
  int hit_count = 0;
  if (hit_times[0] > 0 && hit_times[0] < length)
  {
    start[0] = origin[0] + dir[0] * hit_times[0];
    start[1] = origin[1] + dir[1] * hit_times[0];
    start[2] = origin[2] + dir[2] * hit_times[0];
    *clip_flags |= 1u;
    ++hit_count;
  }
  if (hit_times[1] > 0 && hit_times[1] < length)
  {
    end[0] = origin[0] + dir[0] * hit_times[1];
    end[1] = origin[1] + dir[1] * hit_times[1];
    end[2] = origin[2] + dir[2] * hit_times[1];
    *clip_flags |= 2u;
    ++hit_count;
  }
  return hit_count > 0;
}

/// One stage on one ray.  May move `start` / `end`, ORs its RayFilterFlag bits into `*flags`, returns the stage's
/// verdict.  `kind` is one of OHMHIP_RFS_* (validated when the chain is set).
OHMHIP_RFC_FN bool rayFilterStage(const ohmhip_ray_filter_stage &st, double start[3], double end[3], unsigned *flags)
{
  switch (st.kind)
  {
  case OHMHIP_RFS_GOOD: {
    bool is_good = rfcFinite3(start) && rfcFinite3(end);
    const double ray[3] = { end[0] - start[0], end[1] - start[1], end[2] - start[2] };
    is_good = is_good && (st.range <= 0 || rfcDot3(ray) <= st.range * st.range);
    if (!is_good)
    {
      *flags |= kRffInvalid;
    }
    return is_good;
  }
  case OHMHIP_RFS_CLIP: {
    const bool is_good = rfcFinite3(start) && rfcFinite3(end);
    double ray[3] = { end[0] - start[0], end[1] - start[1], end[2] - start[2] };
    const double len2 = rfcDot3(ray);
    if (is_good && st.range > 0 && len2 > st.range * st.range)
    {
      const double len = sqrt(len2);
      ray[0] = ray[0] / len;
      ray[1] = ray[1] / len;
      ray[2] = ray[2] / len;
      end[0] = start[0] + ray[0] * st.range;
      end[1] = start[1] + ray[1] * st.range;
      end[2] = start[2] + ray[2] * st.range;
      *flags |= kRffClippedEnd;
    }
    if (!is_good)
    {
      *flags |= kRffInvalid;
    }
    return is_good;
  }
  case OHMHIP_RFS_CLIP_BOUNDED: {
    unsigned line_clip_flags = 0;
    if (rfcClipLine(st.box_min, st.box_max, start, end, &line_clip_flags))
    {
      if (!rfcContains(st.box_min, st.box_max, start) && !rfcContains(st.box_min, st.box_max, end))
      {
        return false;
      }
    }
    *flags |= (line_clip_flags & 1u) ? unsigned(kRffClippedStart) : 0u;
    *flags |= (line_clip_flags & 2u) ? unsigned(kRffClippedEnd) : 0u;
    return true;
  }
  case OHMHIP_RFS_CLIP_TO_BOUNDS:
    *flags |= rfcContains(st.box_min, st.box_max, end) ? unsigned(kRffClippedEnd) : 0u;
    return true;
  default:
    return true;
  }
}

/// The chain on one ray.  Returns whether the ray passes; `*flags_out` are the OR-ed RayFilterFlag bits, with kRffInvalid
/// added for a rejected ray whichever stage rejected it (clipBounded's `return false` sets no bit of its own): that bit
/// is how the rejection travels to the set-up pass.
OHMHIP_RFC_FN bool rayFilterChain(const ohmhip_ray_filter_stage *stages, unsigned count, double start[3], double end[3],
                                  unsigned *flags_out)
{
  unsigned flags = 0;
  bool keep = true;
  for (unsigned i = 0; i < count && keep; ++i)
  {
    keep = rayFilterStage(stages[i], start, end, &flags);
  }
  if (!keep)
  {
    flags |= kRffInvalid;
  }
  *flags_out = flags;
  return keep;
}
}  // namespace ohmhip

#endif  // OHMHIP_RAY_FILTER_CHAIN_H
