// OhmGpuMap.h -- C++14 host mirror of the reference's ray-integration interface over the ohmhip C ABI.
//
//   ohm::OccupancyMap (ohm/OccupancyMap.h:291)  parameters + MapChunk / VoxelBlock layout host storage
//   ohm::RayMapper    (ohm/RayMapper.h:22-65)
//   ohm::GpuMap       (ohmgpu/GpuMap.h:143-384)   ohm::GpuNdtMap (ohmgpu/GpuNdtMap.h:63-132)
//   ohm::GpuTsdfMap   (ohmgpu/GpuTsdfMap.h:37-94)
//
// Same names, argument meaning and error behaviour as the reference for this path: integrateRays() takes
// `element_count` POINTS (2 per ray) and returns the number integrated (0 on failure); construction throws
// gputil::ApiException when device memory cannot be allocated; syncVoxels() is the fence that copies modified regions
// back into MapChunk::voxel_blocks-equivalent host memory (index = x + y*dx + z*dx*dy, ohm/MapChunk.h:33-50).
// Only what the path needs is mirrored: this is not a re-implementation of ohm::OccupancyMap.
//
// glm: callers which have glm pass glm::dvec3 arrays (3 packed doubles); this header does not need glm.
#ifndef OHMHIP_OHMGPUMAP_H
#define OHMHIP_OHMGPUMAP_H

#include "gputil_hip.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace ohm
{
/// ohm/RayFlag.h:16-60
enum RayFlag : unsigned
{
  kRfDefault = 0,
  kRfEndPointAsFree = (1u << 0u),
  kRfStopOnFirstOccupied = (1u << 1u),
  kRfExcludeOrigin = (1u << 2u),
  kRfExcludeSample = (1u << 3u),
  kRfExcludeRay = (1u << 4u),
  kRfExcludeUnobserved = (1u << 5u),
  kRfExcludeFree = (1u << 6u),
  kRfExcludeOccupied = (1u << 7u),
  kRfReverseWalk = (1u << 8u)
};

/// ohm/NdtMode.h
enum class NdtMode
{
  kNone = 0,
  kOccupancy,
  kTraversability
};

/// Plain 3 x double point, layout compatible with glm::dvec3.
struct dvec3
{
  double x, y, z;
};

/// ohm/RayFilter.h:21-29
enum RayFilterFlag : unsigned
{
  kRffInvalid = (1u << 0u),
  kRffClippedStart = (1u << 1u),
  kRffClippedEnd = (1u << 2u)
};

/// ohm/RayFilter.h:45: called per ray before integration; may move the points, set RayFilterFlag bits, or reject (false).
using RayFilterFunction = std::function<bool(dvec3 *, dvec3 *, unsigned *)>;

/// The parts of ohm::Aabb (ohm/Aabb.h) the stock ray filters use.
class Aabb
{
public:
  enum : unsigned
  {
    kClippedStart = 1u,
    kClippedEnd = 2u
  };
  Aabb(const dvec3 &min_ext, const dvec3 &max_ext) : corners_{ min_ext, max_ext } {}
  const dvec3 &minExtents() const { return corners_[0]; }
  const dvec3 &maxExtents() const { return corners_[1]; }
  /// ohm/Aabb.h:301-312 with epsilon 0: closed box.
  bool contains(const dvec3 &p) const
  {
    return !(corners_[1].x < p.x || corners_[1].y < p.y || corners_[1].z < p.z) &&
           !(corners_[0].x > p.x || corners_[0].y > p.y || corners_[0].z > p.z);
  }
  /// ohm/Aabb.h:386-446 (allow_clamp false).
  bool clipLine(dvec3 &start, dvec3 &end, unsigned *clip_flags = nullptr) const
  {
    const dvec3 origin = start;
    dvec3 dir{ end.x - start.x, end.y - start.y, end.z - start.z };
    if (clip_flags)
    {
      *clip_flags = 0;
    }
    const double d2 = (dir.x * dir.x + dir.y * dir.y) + dir.z * dir.z;
    if (d2 < 1e-9)
    {
      return false;
    }
    const double length = std::sqrt(d2);
    dir.x /= length;
    dir.y /= length;
    dir.z /= length;
    double t[2] = { 0, 0 };
    if (!rayIntersect(origin, dir, t))
    {
      return false;
    }
    int hits = 0;
    if (t[0] > 0 && t[0] < length)
    {
      start = dvec3{ origin.x + dir.x * t[0], origin.y + dir.y * t[0], origin.z + dir.z * t[0] };
      if (clip_flags)
      {
        *clip_flags |= kClippedStart;
      }
      ++hits;
    }
    if (t[1] > 0 && t[1] < length)
    {
      end = dvec3{ origin.x + dir.x * t[1], origin.y + dir.y * t[1], origin.z + dir.z * t[1] };
      if (clip_flags)
      {
        *clip_flags |= kClippedEnd;
      }
      ++hits;
    }
    return hits > 0;
  }

private:
  /// ohm/Aabb.h:330-383 (slab test).
  bool rayIntersect(const dvec3 &o, const dvec3 &d, double t[2]) const
  {
    const double oo[3] = { o.x, o.y, o.z };
    const double dd[3] = { d.x, d.y, d.z };
    const double lo[3] = { corners_[0].x, corners_[0].y, corners_[0].z };
    const double hi[3] = { corners_[1].x, corners_[1].y, corners_[1].z };
    bool miss = false;
    for (int a = 0; a < 3; ++a)
    {
      const double inv = 1.0 / dd[a];
      const bool neg = dd[a] < 0.0;
      const double tmin = ((neg ? hi[a] : lo[a]) - oo[a]) * inv;
      const double tmax = ((neg ? lo[a] : hi[a]) - oo[a]) * inv;
      if (a == 0)
      {
        t[0] = tmin;
        t[1] = tmax;
        continue;
      }
      miss = miss || (t[0] > tmax) || (tmin > t[1]);
      t[0] = (tmin > t[0] || std::isnan(t[0])) ? tmin : t[0];
      t[1] = (tmax < t[1] || std::isnan(t[1])) ? tmax : t[1];
    }
    return !miss;
  }
  dvec3 corners_[2];
};

/// ohm/RayFilter.cpp:12-34
inline bool goodRayFilter(dvec3 *start, dvec3 *end, unsigned *filter_flags, double max_range)
{
  const double v[6] = { start->x, start->y, start->z, end->x, end->y, end->z };
  bool good = true;
  for (double c : v)
  {
    good = good && std::isfinite(c);
  }
  const double rx = end->x - start->x, ry = end->y - start->y, rz = end->z - start->z;
  good = good && (max_range <= 0 || (rx * rx + ry * ry) + rz * rz <= max_range * max_range);
  if (!good)
  {
    *filter_flags |= kRffInvalid;
  }
  return good;
}

/// ohm/RayFilter.cpp:37-58
inline bool clipRayFilter(dvec3 *start, dvec3 *end, unsigned *filter_flags, double max_length)
{
  const double v[6] = { start->x, start->y, start->z, end->x, end->y, end->z };
  bool good = true;
  for (double c : v)
  {
    good = good && std::isfinite(c);
  }
  double rx = end->x - start->x, ry = end->y - start->y, rz = end->z - start->z;
  const double len2 = (rx * rx + ry * ry) + rz * rz;
  if (good && max_length > 0 && len2 > max_length * max_length)
  {
    const double len = std::sqrt(len2);
    rx /= len;
    ry /= len;
    rz /= len;
    *end = dvec3{ start->x + rx * max_length, start->y + ry * max_length, start->z + rz * max_length };
    *filter_flags |= kRffClippedEnd;
  }
  *filter_flags |= good ? 0u : unsigned(kRffInvalid);
  return good;
}

/// ohm/RayFilter.cpp:61-78
inline bool clipBounded(dvec3 *start, dvec3 *end, unsigned *filter_flags, const Aabb &clip_box)
{
  unsigned line_clip_flags = 0;
  if (clip_box.clipLine(*start, *end, &line_clip_flags))
  {
    if (!clip_box.contains(*start) && !clip_box.contains(*end))
    {
      return false;
    }
  }
  *filter_flags |= (line_clip_flags & Aabb::kClippedStart) ? unsigned(kRffClippedStart) : 0u;
  *filter_flags |= (line_clip_flags & Aabb::kClippedEnd) ? unsigned(kRffClippedEnd) : 0u;
  return true;
}

/// ohm/RayFilter.cpp:81-93
inline bool clipToBounds(dvec3 * /*start*/, dvec3 *end, unsigned *filter_flags, const Aabb &clip_box)
{
  *filter_flags |= clip_box.contains(*end) ? unsigned(kRffClippedEnd) : 0u;
  return true;
}

/// A chain of up to OHMHIP_MAX_RAY_FILTER_STAGES of the stock filters above for GpuMap::setRayFilter: evaluated on the
/// DEVICE for every batch the map integrates, in place of the map's built-in filter (include/ohmhip.h:
/// ohmhip_map_set_ray_filter_stages).  Stage i sees the ray as stage i - 1 left it, flags are OR-ed, the first stage that
/// rejects ends the chain -- `a(...) && b(...)` in a RayFilterFunction lambda.  Calling it runs the same chain on the
/// host (Aabb::contains above has the reference's form already: a NaN coordinate counts as contained); a rejected ray
/// carries kRffInvalid.
class DeviceRayFilter
{
public:
  DeviceRayFilter &goodRay(double max_range = 0.0) { return add(OHMHIP_RFS_GOOD, max_range, nullptr); }
  DeviceRayFilter &clipRay(double max_length) { return add(OHMHIP_RFS_CLIP, max_length, nullptr); }
  DeviceRayFilter &clipBounded(const Aabb &box) { return add(OHMHIP_RFS_CLIP_BOUNDED, 0.0, &box); }
  DeviceRayFilter &clipToBounds(const Aabb &box) { return add(OHMHIP_RFS_CLIP_TO_BOUNDS, 0.0, &box); }
  /// False once more stages were added than the device takes (setRayFilter then fails).
  bool valid() const { return !overflow_; }
  const std::vector<ohmhip_ray_filter_stage> &stages() const { return stages_; }

  bool operator()(dvec3 *start, dvec3 *end, unsigned *filter_flags) const
  {
    for (const ohmhip_ray_filter_stage &st : stages_)
    {
      const Aabb box(dvec3{ st.box_min[0], st.box_min[1], st.box_min[2] }, dvec3{ st.box_max[0], st.box_max[1], st.box_max[2] });
      bool keep = true;
      switch (st.kind)
      {
      case OHMHIP_RFS_GOOD:
        keep = goodRayFilter(start, end, filter_flags, st.range);
        break;
      case OHMHIP_RFS_CLIP:
        keep = clipRayFilter(start, end, filter_flags, st.range);
        break;
      case OHMHIP_RFS_CLIP_BOUNDED:
        keep = ohm::clipBounded(start, end, filter_flags, box);
        break;
      default:
        keep = ohm::clipToBounds(start, end, filter_flags, box);
        break;
      }
      if (!keep)
      {
        *filter_flags |= kRffInvalid;
        return false;
      }
    }
    return true;
  }

private:
  DeviceRayFilter &add(int kind, double range, const Aabb *box)
  {
    if (stages_.size() >= OHMHIP_MAX_RAY_FILTER_STAGES)
    {
      overflow_ = true;
      return *this;
    }
    ohmhip_ray_filter_stage st = {};
    st.kind = kind;
    st.range = range;
    if (box)
    {
      const dvec3 &lo = box->minExtents(), &hi = box->maxExtents();
      st.box_min[0] = lo.x, st.box_min[1] = lo.y, st.box_min[2] = lo.z;
      st.box_max[0] = hi.x, st.box_max[1] = hi.y, st.box_max[2] = hi.z;
    }
    stages_.push_back(st);
    return *this;
  }
  std::vector<ohmhip_ray_filter_stage> stages_;
  bool overflow_ = false;
};

/// ohm/MapProbability.h:20-36 (float)
inline float probabilityToValue(float probability) { return std::log(probability / (1.0f - probability)); }
inline float valueToProbability(float value)
{
  return (value == -INFINITY) ? 0.0f : 1.0f - (1.0f / (1.0f + std::exp(value)));
}

/// One region's voxel memory: one contiguous block per layer (ohm/MapChunk.h:155, ohm/VoxelBlock.h:48).
struct MapChunk
{
  std::array<int16_t, 3> region{ { 0, 0, 0 } };
  std::vector<std::vector<uint8_t>> voxel_blocks;  ///< indexed by layer id (ohmhip_layer_id); empty when absent
};

/// Host-side map description and chunk store.
class OccupancyMap
{
public:
  explicit OccupancyMap(double resolution = 1.0, int region_dim_x = 32, int region_dim_y = 32, int region_dim_z = 32)
    : resolution_(resolution)
  {
    region_dim_[0] = region_dim_x > 0 ? region_dim_x : 32;  // ohm/OccupancyMap.h:24-26
    region_dim_[1] = region_dim_y > 0 ? region_dim_y : 32;
    region_dim_[2] = region_dim_z > 0 ? region_dim_z : 32;
    // ohm/OccupancyMap.cpp:205-213
    min_voxel_value_ = -2.0f;
    max_voxel_value_ = 3.511f;
    hit_value_ = probabilityToValue(0.9f);
    miss_value_ = probabilityToValue(0.45f);
    threshold_value_ = probabilityToValue(0.5f);
    layers_ = OHMHIP_LAYER_BIT(OHMHIP_LID_OCCUPANCY);
  }

  double resolution() const { return resolution_; }
  const int *regionVoxelDimensions() const { return region_dim_; }
  size_t regionVoxelVolume() const { return size_t(region_dim_[0]) * region_dim_[1] * region_dim_[2]; }
  void setOrigin(double x, double y, double z)
  {
    origin_[0] = x;
    origin_[1] = y;
    origin_[2] = z;
  }
  const double *origin() const { return origin_; }
  void setHitProbability(float p) { hit_value_ = probabilityToValue(p); }
  void setMissProbability(float p) { miss_value_ = probabilityToValue(p); }
  /// ohm/OccupancyMap.h:623: the log-odds adjustments set directly.
  void setHitValue(float value) { hit_value_ = value; }
  void setMissValue(float value) { miss_value_ = value; }
  void setOccupancyThresholdProbability(float p) { threshold_value_ = probabilityToValue(p); }
  float hitValue() const { return hit_value_; }
  float missValue() const { return miss_value_; }
  float missProbability() const { return valueToProbability(miss_value_); }
  float occupancyThresholdValue() const { return threshold_value_; }
  float minVoxelValue() const { return min_voxel_value_; }
  float maxVoxelValue() const { return max_voxel_value_; }
  void setMinVoxelValue(float v) { min_voxel_value_ = v; }
  void setMaxVoxelValue(float v) { max_voxel_value_ = v; }
  bool saturateAtMinValue() const { return saturate_min_; }
  bool saturateAtMaxValue() const { return saturate_max_; }
  void setSaturateAtMinValue(bool s) { saturate_min_ = s; }
  void setSaturateAtMaxValue(bool s) { saturate_max_ = s; }
  /// Ray filter: 0 none, 1 goodRayFilter(range), 2 clipRayFilter(range) (ohm/RayFilter.cpp:12-58).
  void setRayFilter(int mode, double range)
  {
    ray_filter_ = mode;
    ray_filter_range_ = range;
  }
  int rayFilterMode() const { return ray_filter_; }
  double rayFilterRange() const { return ray_filter_range_; }
  unsigned layers() const { return layers_; }
  void addLayer(int layer_id) { layers_ |= OHMHIP_LAYER_BIT(layer_id); }
  bool hasLayer(int layer_id) const { return (layers_ & OHMHIP_LAYER_BIT(layer_id)) != 0; }
  /// The layout without a layer (MapLayout::removeLayer + updateLayout): the chunks lose its blocks.
  void removeLayer(int layer_id) { updateLayout(layers_ & ~OHMHIP_LAYER_BIT(layer_id)); }
  /// OccupancyMap::updateLayout (ohm/OccupancyMap.cpp:670-682) with MapChunk::updateLayout (ohm/MapChunk.cpp:93-143) for
  /// every chunk: the blocks of the layers in both layouts stay, an added layer gets a block of its clear value
  /// (ohm/DefaultLayer.cpp: occupancy +inf, clearance -1, zero bytes otherwise), a removed layer's blocks go.
  /// preserve_map == false drops the chunks instead.
  void updateLayout(unsigned layers, bool preserve_map = true)
  {
    if (!preserve_map)
    {
      chunks_.clear();
    }
    const size_t voxels = regionVoxelVolume();
    for (auto &entry : chunks_)
    {
      std::vector<std::vector<uint8_t>> &blocks = entry.second.voxel_blocks;
      blocks.resize(OHMHIP_LID_COUNT);
      for (int layer = 0; layer < OHMHIP_LID_COUNT; ++layer)
      {
        const bool wanted = (layers & OHMHIP_LAYER_BIT(layer)) != 0;
        if (!wanted)
        {
          std::vector<uint8_t>().swap(blocks[layer]);
        }
        else if (blocks[layer].empty())
        {
          const float clear = (layer == OHMHIP_LID_OCCUPANCY) ? INFINITY : (layer == OHMHIP_LID_CLEARANCE) ? -1.0f : 0.0f;
          blocks[layer].resize(voxels * ohmhip_layer_voxel_bytes(layer));
          for (size_t at = 0; at + sizeof(float) <= blocks[layer].size(); at += sizeof(float))
          {
            std::memcpy(&blocks[layer][at], &clear, sizeof(float));
          }
        }
      }
    }
    layers_ = layers;
  }

  using ChunkMap = std::map<std::array<int16_t, 3>, MapChunk>;
  ChunkMap &chunks() { return chunks_; }
  const ChunkMap &chunks() const { return chunks_; }
  size_t regionCount() const { return chunks_.size(); }

  /// OccupancyMap::region(key, allow_create) restricted to what syncVoxels() needs.
  MapChunk &region(const std::array<int16_t, 3> &key)
  {
    MapChunk &chunk = chunks_[key];
    chunk.region = key;
    if (chunk.voxel_blocks.size() < size_t(OHMHIP_LID_COUNT))
    {
      chunk.voxel_blocks.resize(OHMHIP_LID_COUNT);
    }
    return chunk;
  }

private:
  double resolution_;
  int region_dim_[3];
  double origin_[3] = { 0, 0, 0 };
  float hit_value_, miss_value_, threshold_value_, min_voxel_value_, max_voxel_value_;
  bool saturate_min_ = false, saturate_max_ = false;
  int ray_filter_ = OHMHIP_FILTER_GOOD;  // ohm/OccupancyMap.cpp:215-218
  double ray_filter_range_ = 1e10;
  unsigned layers_;
  ChunkMap chunks_;
};

/// ohm/RayMapper.h:22-65
class RayMapper
{
public:
  virtual ~RayMapper() = default;
  virtual bool valid() const = 0;
  virtual size_t integrateRays(const dvec3 *rays, size_t element_count, const float *intensities,
                               const double *timestamps, unsigned ray_update_flags) = 0;
  size_t integrateRays(const dvec3 *rays, size_t element_count)
  {
    return integrateRays(rays, element_count, nullptr, nullptr, kRfDefault);
  }
};

/// Voxel key: region + local coordinates (ohm/Key.h), in the layout of the 10-byte record the device reads and writes
/// (ohm::GpuKey, ohmgpu/GpuKey.h:37-46), so arrays of keys cross the C ABI as they are.  `voxel` names all four bytes
/// of the record -- the fourth is 0 except where a call documents a use for it -- and `local` its three coordinates;
/// both are byte arrays over the same storage.  Equality is that of the voxel: the fourth byte does not take part.
struct Key
{
  int16_t region[3];
  union
  {
    uint8_t voxel[4];
    uint8_t local[3];
  };
  bool operator==(const Key &o) const
  {
    return region[0] == o.region[0] && region[1] == o.region[1] && region[2] == o.region[2] && local[0] == o.local[0] &&
           local[1] == o.local[1] && local[2] == o.local[2];
  }
};
static_assert(sizeof(Key) == 10, "Key keeps the 10-byte GpuKey layout");
/// The name the map's own calls use for the record.
using CloudKey = Key;

/// The keys of the regions a device map holds (ohmhip_map_regions), or of those modified since the last
/// ohmhip_map_clear_dirty (ohmhip_map_dirty_regions): the count, then the list.  @return the status; `keys` is empty
/// unless it is OHMHIP_OK.
inline int fetchRegions(ohmhip_map_t map, bool dirty_only, std::vector<std::array<int16_t, 3>> &keys)
{
  const auto call = dirty_only ? &ohmhip_map_dirty_regions : &ohmhip_map_regions;
  size_t count = 0;
  keys.clear();
  int status = call(map, nullptr, 0, &count);
  if (status == OHMHIP_OK && count)
  {
    keys.resize(count);
    status = call(map, keys.front().data(), count, &count);
    keys.resize(status == OHMHIP_OK ? count : 0);
  }
  return status;
}

/// ohm::GpuMap (ohmgpu/GpuMap.h:143-384)
class GpuMap : public RayMapper
{
public:
  /// @param expected_element_count points per call the per-batch device buffers are sized for up front (as the reference does, ohmgpu/GpuMap.cpp:429-470); larger batches still work, the buffers then grow on demand.
  /// @param gpu_mem_size device memory budget for the resident map, 0 => default.
  explicit GpuMap(OccupancyMap *map, bool borrowed_map = true, unsigned expected_element_count = 2048,
                  size_t gpu_mem_size = 0)
    : GpuMap(map, borrowed_map, expected_element_count, gpu_mem_size, OHMHIP_MODE_OCCUPANCY, nullptr)
  {}

  ~GpuMap() override
  {
    if (handle_)
    {
      ohmhip_map_destroy(handle_);
    }
    if (!borrowed_map_)
    {
      delete map_;
    }
  }
  GpuMap(const GpuMap &) = delete;
  GpuMap &operator=(const GpuMap &) = delete;

  bool gpuOk() const { return handle_ != nullptr; }
  bool valid() const override { return gpuOk(); }
  OccupancyMap &map() { return *map_; }
  const OccupancyMap &map() const { return *map_; }
  bool borrowedMap() const { return borrowed_map_; }
  float hitValue() const { return map_->hitValue(); }
  float missValue() const { return map_->missValue(); }
  /// Pass-throughs to the map for API compatibility (ohmgpu/GpuMap.h:234-244); the device takes the new values with the
  /// next batch.
  void setHitValue(float value) { map_->setHitValue(value); }
  void setMissValue(float value) { map_->setMissValue(value); }
  /// ohmgpu/GpuMap.h:271, 323: the reference can sort a batch's rays by region before upload.  Here every batch is
  /// binned per region on the device: stored only.
  void setGroupedRays(bool group) { grouped_rays_ = group; }
  bool groupedRays() const { return grouped_rays_; }
  /// ohmgpu/GpuMap.h:246-262.  Stored only: this backend bins rays per region, it does not need segmentation.
  void setRaySegmentLength(double length) { ray_segment_length_ = length; }
  double raySegmentLength() const { return ray_segment_length_; }

  /// ohmgpu/GpuMap.cpp:348-369.  With a filter set, integrateRays() runs it per ray on the host, as the reference does
  /// (GpuMap.cpp:736-746), and hands the surviving rays and their RayFilterFlag bits to the device; without one the
  /// map's built-in filter (OccupancyMap::setRayFilter(mode, range)) runs on the device.
  void setRayFilter(const RayFilterFunction &ray_filter)
  {
    clearDeviceRayFilter();
    ray_filter_ = ray_filter;
  }
  /// A chain of the stock filters, evaluated on the device for every batch -- host pointers, device buffers, collected
  /// calls -- with no host pass (ohmhip_map_set_ray_filter_stages).  Returns false (lastStatus()) when the chain is
  /// refused: too many stages, a partitioned map.  rayFilter() is empty while a device chain is set.
  bool setRayFilter(const DeviceRayFilter &ray_filter)
  {
    if (!gpuOk() || !ray_filter.valid())
    {
      last_status_ = OHMHIP_ERR_INVALID_ARG;
      return false;
    }
    const std::vector<ohmhip_ray_filter_stage> &stages = ray_filter.stages();
    last_status_ = ohmhip_map_set_ray_filter_stages(handle_, stages.data(), unsigned(stages.size()));
    if (last_status_ != OHMHIP_OK)
    {
      return false;
    }
    device_ray_filter_ = ray_filter;
    ray_filter_ = RayFilterFunction();
    return true;
  }
  const RayFilterFunction &rayFilter() const { return ray_filter_; }
  const RayFilterFunction &effectiveRayFilter() const { return ray_filter_; }
  const DeviceRayFilter &deviceRayFilter() const { return device_ray_filter_; }
  void clearRayFilter()
  {
    clearDeviceRayFilter();
    ray_filter_ = RayFilterFunction();
  }
  /// What the device chain does to `rays` without touching the map: every ray as the chain leaves it and its
  /// RayFilterFlag byte (rejected: kRffInvalid); returns the number of rays kept (ohmhip_map_apply_ray_filter).
  size_t applyRayFilter(const dvec3 *rays, size_t element_count, std::vector<dvec3> &rays_out,
                        std::vector<unsigned char> &flags_out)
  {
    rays_out.assign(element_count & ~size_t(1), dvec3{ 0, 0, 0 });
    flags_out.assign(element_count / 2, 0);
    size_t passed = 0;
    last_status_ = gpuOk() ? ohmhip_map_apply_ray_filter(handle_, reinterpret_cast<const double *>(rays), element_count,
                                                         reinterpret_cast<double *>(rays_out.data()), flags_out.data(),
                                                         &passed) :
                             OHMHIP_ERR_INVALID_ARG;
    return (last_status_ == OHMHIP_OK) ? passed : 0;
  }

  using RayMapper::integrateRays;
  /// ohmgpu/GpuMap.cpp:416: returns points integrated, 0 on failure (gpuOk() false, device error).
  size_t integrateRays(const dvec3 *rays, size_t element_count, const float *intensities, const double *timestamps,
                       unsigned ray_update_flags) override
  {
    if (!gpuOk() || !rays || element_count < 2)
    {
      return 0;
    }
    if (!pushConfigIfChanged())
    {
      return 0;
    }
    size_t integrated = 0;
    if (ray_filter_)
    {
      if (timestamps && !time_base_checked_)
      {
        // The reference takes the map's time base from the first stamp of the call BEFORE it filters
        // (ohmgpu/GpuMap.cpp:593 against :736-746): the library only sees the kept rays' stamps, so a base still unset
        // is set here -- also by a call whose rays are all rejected.
        if (firstRayTime() < 0)
        {
          ohmhip_map_set_first_ray_time(handle_, timestamps[0]);
        }
        time_base_checked_ = true;
      }
      std::vector<dvec3> kept;
      std::vector<unsigned char> kept_flags;
      std::vector<float> kept_intensities;
      std::vector<double> kept_timestamps;
      kept.reserve(element_count);
      for (size_t i = 0; i + 1 < element_count; i += 2)
      {
        dvec3 start = rays[i], end = rays[i + 1];
        unsigned filter_flags = 0;
        if (!ray_filter_(&start, &end, &filter_flags))
        {
          continue;
        }
        kept.push_back(start);
        kept.push_back(end);
        kept_flags.push_back(static_cast<unsigned char>(filter_flags));
        if (intensities)
        {
          kept_intensities.push_back(intensities[i >> 1]);
        }
        if (timestamps)
        {
          kept_timestamps.push_back(timestamps[i >> 1]);
        }
      }
      if (kept.empty())
      {
        return 0;
      }
      last_status_ = ohmhip_map_integrate_rays_filtered(
        handle_, reinterpret_cast<const double *>(kept.data()), kept.size(),
        intensities ? kept_intensities.data() : nullptr, timestamps ? kept_timestamps.data() : nullptr,
        ray_update_flags, kept_flags.data(), &integrated);
      return (last_status_ == OHMHIP_OK) ? integrated : 0;
    }
    last_status_ = ohmhip_map_integrate_rays(handle_, reinterpret_cast<const double *>(rays), element_count,
                                             intensities, timestamps, ray_update_flags, &integrated);
    last_partial_ = (last_status_ == OHMHIP_OK) ? 0 : integrated;
    return (last_status_ == OHMHIP_OK) ? integrated : 0;
  }
  /// glm-compatible overload: any 3-double point type.
  template <typename Vec3>
  size_t integrateRays(const Vec3 *rays, size_t element_count, const float *intensities = nullptr,
                       const double *timestamps = nullptr, unsigned ray_update_flags = kRfDefault)
  {
    static_assert(sizeof(Vec3) == 3 * sizeof(double), "rays must be packed double triples (glm::dvec3)");
    return integrateRays(reinterpret_cast<const dvec3 *>(rays), element_count, intensities, timestamps,
                         ray_update_flags);
  }
  /// Rays already resident in device memory (e.g. the output buffer of GpuTransformSamples::transform): the same
  /// integration without the host-to-device staging.  The buffer's content must be complete when the call is made (the
  /// transform is synchronous; wait for any other producer): the map reads it on streams of its own.
  size_t integrateRays(const gputil::Buffer &device_rays, size_t element_count, unsigned ray_update_flags = kRfDefault)
  {
    if (!gpuOk() || !device_rays.isValid() || element_count < 2)
    {
      return 0;
    }
    if (!pushConfigIfChanged())
    {
      return 0;
    }
    void *ptr = nullptr;
    size_t integrated = 0;
    last_status_ = ohmhip_buffer_ptr(device_rays.handle(), &ptr);
    if (last_status_ == OHMHIP_OK)
    {
      last_status_ = ohmhip_map_integrate_rays_device(handle_, static_cast<const double *>(ptr), element_count, nullptr,
                                                      nullptr, ray_update_flags, &integrated);
    }
    return (last_status_ == OHMHIP_OK) ? integrated : 0;
  }
  int lastStatus() const { return last_status_; }
  /// After a failed integrateRays: the leading elements of that call that WERE integrated (non-zero only when a batch over
  /// the residency limit was split and a later part still did not fit, include/ohmhip.h); do not present those again.
  size_t lastPartialCount() const { return last_partial_; }

  /// ohmgpu/GpuMap.cpp:308-324 -> GpuLayerCache::syncToMainMemory: fence, then copy regions modified on the device
  /// into the host chunks (every enabled layer).
  void syncVoxels() { syncLayers(nullptr); }

  /// ohmgpu/GpuMap.cpp:327-345: only the listed layers (OHMHIP_LID_* ids here).  The regions stay marked as modified
  /// -- there is one mark per region, not per layer -- so a later syncVoxels() still brings the other layers over.
  void syncVoxels(const std::vector<int> &layer_indices) { syncLayers(&layer_indices); }

private:
  void syncLayers(const std::vector<int> *only)
  {
    if (!gpuOk())
    {
      return;
    }
    std::vector<std::array<int16_t, 3>> keys;
    OHMHIP_GPUAPICHECK(fetchRegions(handle_, true, keys));
    const size_t count = keys.size();
    const size_t voxels = map_->regionVoxelVolume();
    for (int layer = 0; layer < OHMHIP_LID_COUNT; ++layer)
    {
      if (!map_->hasLayer(layer) || count == 0)
      {
        continue;
      }
      if (only && std::find(only->begin(), only->end(), layer) == only->end())
      {
        continue;
      }
      std::vector<void *> dsts(count);
      for (size_t i = 0; i < count; ++i)
      {
        MapChunk &chunk = map_->region(keys[i]);
        chunk.voxel_blocks[layer].resize(voxels * ohmhip_layer_voxel_bytes(layer));
        dsts[i] = chunk.voxel_blocks[layer].data();
      }
      OHMHIP_GPUAPICHECK(ohmhip_map_read_regions(handle_, layer, keys.front().data(), count, dsts.data()));
    }
    if (!only)
    {
      OHMHIP_GPUAPICHECK(ohmhip_map_clear_dirty(handle_));
    }
    OHMHIP_GPUAPICHECK(ohmhip_map_sync(handle_));
  }

public:

  ohmhip_batch_stats lastBatchStats() const
  {
    ohmhip_batch_stats st{};
    ohmhip_map_last_stats(handle_, &st);
    return st;
  }
  /// Device batches launched so far (a call that only collects its rays, or is rejected, launches none): what a caller
  /// recycling device ray buffers by the "two batches in flight" rule counts (include/ohmhip.h).
  uint64_t batchesLaunched() const
  {
    uint64_t n = 0;
    ohmhip_map_batches_launched(handle_, &n);
    return n;
  }
  /// Regions above 32768 voxels only: rays cut because a tile coordinate left the key range although the reference
  /// addresses the region (include/ohmhip.h: ohmhip_map_rays_beyond_tiles).
  uint64_t raysBeyondTiles() const
  {
    uint64_t n = 0;
    ohmhip_map_rays_beyond_tiles(handle_, &n);
    return n;
  }
  /// OccupancyMap::setFirstRayTime / firstRayTime (ohm/OccupancyMap.h:342-351): the touch-time layer's time base; the
  /// ranks of a partitioned map share one.
  void setFirstRayTime(double time)
  {
    OHMHIP_GPUAPICHECK(ohmhip_map_set_first_ray_time(handle_, time));
    time_base_checked_ = false;
  }
  double firstRayTime() const
  {
    double t = -1.0;
    ohmhip_map_first_ray_time(handle_, &t);
    return t;
  }
  /// Start markers of the set-up and binning passes for lastBatchStats().ms_setup (a few microseconds per batch; off by
  /// default, see ohmhip_map_set_phase_timing).
  void setPhaseTiming(bool enable) { OHMHIP_GPUAPICHECK(ohmhip_map_set_phase_timing(handle_, enable ? 1 : 0)); }
  /// The MapRegionCache face of the reference's GpuCache (ohm/MapRegionCache.h; ohmgpu/GpuCache.h:80): what the core
  /// map and the tests call through gpuCache() -- flush / clear / remove.  There is no separate cache object here (the
  /// whole map is resident), so this is a view of the GpuMap.
  class GpuCache
  {
  public:
    explicit GpuCache(GpuMap *owner) : owner_(owner) {}
    /// GpuCache::flush: bring the host map up to date.
    void flush() { owner_->syncVoxels(); }
    /// GpuCache::clear: drop every resident region (modified or not).
    void clear() { OHMHIP_GPUAPICHECK(ohmhip_map_clear(owner_->handle_)); }
    /// MapRegionCache::remove(region_key)
    void remove(const std::array<int16_t, 3> &region_key) { owner_->removeRegions(region_key.data(), 1); }
    /// GpuCache::reinitialise (ohmgpu/GpuCache.h:103): the reference rebuilds its layer caches after the map's layout
    /// changed, dropping what they held; here the device map keeps its layout for life, so this is clear().
    void reinitialise() { clear(); }
    /// GpuCache::targetGpuAllocSize (ohmgpu/GpuCache.h:139): the byte budget of the device-side voxel storage
    /// (0: bounded by the device's free memory only).
    size_t targetGpuAllocSize() const
    {
      ohmhip_cache_stats st{};
      OHMHIP_GPUAPICHECK(ohmhip_map_cache_stats(owner_->handle_, &st, 0));
      return size_t(st.memory_limit);
    }
    /// GpuCache::layerCount (ohmgpu/GpuCache.h:143): voxel layers held on the device.
    unsigned layerCount() const
    {
      unsigned n = 0;
      for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
      {
        n += owner_->map().hasLayer(l) ? 1u : 0u;
      }
      return n;
    }

  private:
    GpuMap *owner_;
  };
  GpuCache *gpuCache() { return &cache_view_; }

  /// MapRegionCache::remove, as OccupancyMap::cullRegions calls it on the map's GPU cache
  /// (ohm/OccupancyMap.cpp:1202-1234): drop regions (packed int16 x, y, z triples) from the device map.
  size_t removeRegions(const int16_t *keys_xyz, size_t count)
  {
    size_t removed = 0;
    OHMHIP_GPUAPICHECK(ohmhip_map_remove_regions(handle_, keys_xyz, count, &removed));
    return removed;
  }

  /// GpuLayerCache::queryStats (ohmgpu/GpuLayerCache.h:334-339): hits / misses / full of the resident region pool
  /// (ohmhip_cache_stats); @p reset clears the counters as GpuLayerCache::resetStats() does.
  ohmhip_cache_stats queryStats(bool reset = false) const
  {
    ohmhip_cache_stats st{};
    OHMHIP_GPUAPICHECK(ohmhip_map_cache_stats(handle_, &st, reset ? 1 : 0));
    return st;
  }

  /// Bound the region pool in bytes (include/ohmhip.h "RESIDENCY LIMIT"; the reference's gpu_mem_size): a batch that
  /// needs more fails -- integrateRays() returns 0 -- and leaves the map as it was.  0 removes the bound.
  void setMemoryLimit(uint64_t bytes) { OHMHIP_GPUAPICHECK(ohmhip_map_set_memory_limit(handle_, bytes)); }

  /// With a memory limit: spill the least recently used regions to a host store instead of failing the batch
  /// (include/ohmhip.h "SPILL TO HOST"; the reference reuses its least recently used cache slot,
  /// ohmgpu/GpuLayerCache.cpp:530-584).  Stored regions stay part of the map and come back when touched.
  void setSpillToHost(bool enable = true)
  {
    OHMHIP_GPUAPICHECK(ohmhip_map_set_spill_to_host(handle_, enable ? 1 : 0));
  }

  /// Opt-in background write-back of the spill path (include/ohmhip.h "WRITE-BACK"; the reference overlaps the download
  /// of a reused cache slot with queued work, ohmgpu/GpuLayerCache.cpp:550-584).
  void setSpillWriteback(bool enable = true)
  {
    OHMHIP_GPUAPICHECK(ohmhip_map_set_spill_writeback(handle_, enable ? 1 : 0));
  }

  /// Not in the reference: run consecutive small integrateRays() batches as one device batch of at least @p min_rays
  /// rays (see ohmhip_map_set_batch_coalescing; on by default with 65536); 0 turns it off.
  void setBatchCoalescing(size_t min_rays) { OHMHIP_GPUAPICHECK(ohmhip_map_set_batch_coalescing(handle_, min_rays)); }
  /// Large host batches return once staged; the launch sequence runs on a thread of the map (see
  /// ohmhip_map_set_async_launch).  Off by default.
  void setAsyncLaunch(bool enable) { OHMHIP_GPUAPICHECK(ohmhip_map_set_async_launch(handle_, enable ? 1 : 0)); }

  /// OccupancyMap::updateLayout and the add*Layer calls (ohm/OccupancyMap.cpp:521-682) on the live map (include/ohmhip.h
  /// "LAYER CHANGES"): the map holds exactly @p layers (a mask of OHMHIP_LAYER_BIT) from the next batch on -- added
  /// layers start cleared, removed ones are released, the others keep their voxels where they are -- and the host map
  /// follows.  preserve_map == false also drops every region.  Throws, and changes nothing, for a layer the map's mode
  /// needs, a partitioned or merging map, or a memory limit the new set does not fit.
  void updateLayout(unsigned layers, bool preserve_map = true)
  {
    ohmhip_layer_change_stats stats{};
    OHMHIP_GPUAPICHECK(ohmhip_map_update_layers(handle_, layers, preserve_map ? 0u : OHMHIP_LAYOUT_DISCARD_MAP, &stats));
    last_layer_change_ = stats;
    cfg_.layers = layers;
    map_->updateLayout(layers, preserve_map);
  }
  void addLayer(int layer_id) { updateLayout(map_->layers() | OHMHIP_LAYER_BIT(layer_id)); }
  void removeLayer(int layer_id) { updateLayout(map_->layers() & ~OHMHIP_LAYER_BIT(layer_id)); }
  void addVoxelMeanLayer() { addLayer(OHMHIP_LID_MEAN); }
  void addTraversalLayer() { addLayer(OHMHIP_LID_TRAVERSAL); }
  void addTouchTimeLayer() { addLayer(OHMHIP_LID_TOUCH_TIME); }
  void addIncidentNormalLayer() { addLayer(OHMHIP_LID_INCIDENT); }
  bool voxelMeanEnabled() const { return map_->hasLayer(OHMHIP_LID_MEAN); }
  bool traversalEnabled() const { return map_->hasLayer(OHMHIP_LID_TRAVERSAL); }
  bool touchTimeEnabled() const { return map_->hasLayer(OHMHIP_LID_TOUCH_TIME); }
  bool incidentNormalEnabled() const { return map_->hasLayer(OHMHIP_LID_INCIDENT); }
  /// ohmhip_layer_change_stats of the last updateLayout that reached the device (zero before the first).
  const ohmhip_layer_change_stats &lastLayerChangeStats() const { return last_layer_change_; }

  /// Not in the reference (single device): owner-computes multi-GPU mode, see ohmhip_map_set_region_ownership.  The
  /// map integrates only what falls in the regions @p rank owns among @p world_size maps fed the same ray stream.
  void setRegionOwnership(unsigned world_size, unsigned rank, int block_shift = 0)
  {
    OHMHIP_GPUAPICHECK(ohmhip_map_set_region_ownership(handle_, world_size, rank, block_shift));
  }

  /// Not in the reference (single device): the partitioned map (include/ohmhip.h "Partitioned map") -- like
  /// setRegionOwnership(), with the blocks of 2^block_shift regions dealt by a table (x fastest) over
  /// [grid_origin, grid_origin + grid_dims) in block coordinates; an empty table selects the block hash.
  struct RegionPartition
  {
    unsigned world_size = 1;
    unsigned rank = 0;
    int block_shift = 0;
    int grid_origin[3] = { 0, 0, 0 };
    unsigned grid_dims[3] = { 0, 0, 0 };
    std::vector<uint8_t> owners;
  };
  void setRegionPartition(const RegionPartition &partition)
  {
    ohmhip_partition p;
    p.world_size = partition.world_size;
    p.rank = partition.rank;
    p.block_shift = partition.block_shift;
    for (int a = 0; a < 3; ++a)
    {
      p.grid_origin[a] = partition.grid_origin[a];
      p.grid_dims[a] = partition.grid_dims[a];
    }
    p.owners = partition.owners.empty() ? nullptr : partition.owners.data();
    OHMHIP_GPUAPICHECK(ohmhip_map_set_region_partition(handle_, &p));
    partition_world_ = (partition.world_size > 1) ? partition.world_size : 1u;
  }
  /// Route @p element_count / 2 rays resident in @p device_rays to the ranks owning a region they touch
  /// (ohmhip_map_route_rays): @p routed is resized to hold them per destination, blocks back to back in rank order,
  /// rays in order inside a block; @p counts[d] = rays addressed to rank d.  Returns the total number of routed rays.
  size_t routeRays(const gputil::Buffer &device_rays, size_t element_count, unsigned ray_update_flags,
                   gputil::Buffer &routed, std::vector<uint32_t> &counts)
  {
    counts.assign(partition_world_, 0u);
    void *src = nullptr;
    OHMHIP_GPUAPICHECK(ohmhip_buffer_ptr(device_rays.handle(), &src));
    size_t capacity = routed.isValid() ? routed.size() / (6 * sizeof(double)) : 0;
    for (;;)
    {
      void *dst = nullptr;
      if (routed.isValid())
      {
        OHMHIP_GPUAPICHECK(ohmhip_buffer_ptr(routed.handle(), &dst));
      }
      const int status = ohmhip_map_route_rays(handle_, static_cast<const double *>(src), element_count / 2,
                                               ray_update_flags, static_cast<double *>(dst), nullptr, capacity,
                                               counts.data(), nullptr);
      size_t total = 0;
      for (uint32_t c : counts)
      {
        total += c;
      }
      if (status == OHMHIP_OK)
      {
        return total;
      }
      if (status != OHMHIP_ERR_CAPACITY)
      {
        OHMHIP_GPUAPICHECK(status);
      }
      capacity = total + total / 4 + 64;
      if (routed.isValid())
      {
        routed.resize(capacity * 6 * sizeof(double));
      }
      else
      {
        routed.create(capacity * 6 * sizeof(double));
      }
      capacity = routed.size() / (6 * sizeof(double));
    }
  }

  /// ohm::NearestNeighbours for `query_count` near points at once (ohmhip_map_nearest_neighbours): every obstructing voxel
  /// within search_radius of a point in the CPU query's visiting order, or with kQfNearestResult (1 << 1) the closest;
  /// kQfUnknownAsOccupied (1 << 0).  counts: results per query; those of query q start at the sum of the counts before
  /// it.  @return the status (lastStatus() too).
  int nearestNeighbours(const dvec3 *points, size_t query_count, float search_radius, unsigned query_flags,
                        std::vector<uint64_t> &counts, std::vector<CloudKey> &keys, std::vector<float> &ranges)
  {
    static_assert(sizeof(dvec3) == 3 * sizeof(double), "points are read as 3 doubles each");
    counts.assign(query_count, 0);
    keys.clear();
    ranges.clear();
    if (!gpuOk() || !pushConfigIfChanged())
    {
      return last_status_ = OHMHIP_ERR_INVALID_ARG;
    }
    ohmhip_neighbours_params p{};
    p.search_radius = search_radius;
    p.query_flags = query_flags & (OHMHIP_QF_UNKNOWN_AS_OCCUPIED | OHMHIP_QF_NEAREST_RESULT);
    uint64_t total = 0, unused = 0;
    const double *xyz = query_count ? &points[0].x : nullptr;
    last_status_ = ohmhip_map_nearest_neighbours(handle_, xyz, query_count, &p, 0, query_count ? counts.data() : &unused,
                                                 nullptr, nullptr, &total);
    if (last_status_ != OHMHIP_OK || total == 0)
    {
      return last_status_;
    }
    keys.resize(size_t(total));
    ranges.resize(size_t(total));
    const uint64_t capacity = total;
    last_status_ = ohmhip_map_nearest_neighbours(handle_, xyz, query_count, &p, capacity, counts.data(), keys.data(),
                                                 ranges.data(), &total);
    const size_t held = (last_status_ == OHMHIP_OK) ? size_t(std::min(total, capacity)) : 0;
    keys.resize(held);
    ranges.resize(held);
    return last_status_;
  }

  /// OccupancyMap::voxelKey of each point in the map's geometry (ohmhip_map_voxel_keys): Key::kNull -- region lowest()
  /// x 3, voxel 0 -- where the reference yields it.
  std::vector<CloudKey> voxelKeys(const dvec3 *points, size_t count)
  {
    std::vector<CloudKey> keys(count);
    last_status_ = gpuOk() ? ohmhip_map_voxel_keys(handle_, count ? &points[0].x : nullptr, count, keys.data()) :
                             OHMHIP_ERR_INVALID_ARG;
    return keys;
  }

  /// The voxels of layer `layer_id` at `keys` (ohmhip_map_read_voxels): ohmhip_layer_voxel_bytes(layer_id) bytes each into
  /// `values`; present[i] = 1 when the map holds the key's region, else the value is the layer's clear value.
  int readVoxels(int layer_id, const std::vector<CloudKey> &keys, std::vector<uint8_t> &values,
                 std::vector<uint8_t> &present)
  {
    values.assign(keys.size() * ohmhip_layer_voxel_bytes(layer_id), 0);
    present.assign(keys.size(), 0);
    if (!gpuOk() || !pushConfigIfChanged())
    {
      return last_status_ = OHMHIP_ERR_INVALID_ARG;
    }
    return last_status_ = ohmhip_map_read_voxels(handle_, layer_id, keys.data(), keys.size(), values.data(), present.data());
  }

  /// ohm::OccupancyType of the voxels at `keys`: kNull (-2) where the map does not hold the region, else occupancyType
  /// (ohm/VoxelOccupancy.h:116-128: unobserved -1 -- a NaN too --, free 0, occupied 1).
  std::vector<int8_t> occupancyTypes(const std::vector<CloudKey> &keys)
  {
    std::vector<uint8_t> values, present;
    std::vector<int8_t> types(keys.size(), int8_t(-2));
    if (readVoxels(OHMHIP_LID_OCCUPANCY, keys, values, present) != OHMHIP_OK)
    {
      return types;
    }
    const float threshold = map_->occupancyThresholdValue();
    for (size_t i = 0; i < keys.size(); ++i)
    {
      float v;
      std::memcpy(&v, &values[i * sizeof(float)], sizeof(float));
      const int type = (v < std::numeric_limits<float>::infinity()) ? ((v < threshold) ? 0 : 1) : -1;
      types[i] = present[i] ? int8_t(type) : int8_t(-2);
    }
    return types;
  }

  /// ohmfilter's test of `count` points (ohmhip_map_filter_points; utils/ohmfilter/ohmfilter.cpp:150-279): status 0 not
  /// occupied, 1 kept, 2 removed by the covariance test, which runs on a map with the mean and covariance layers unless
  /// occupancy_only is set or expected_value_tolerance is negative; kept_indices: the indices of the kept points,
  /// ascending; values: filterPointByCovariance's value where the test ran, NaN elsewhere; keys: each point's voxel key.
  /// @return the status (lastStatus() too).
  int filterPoints(const dvec3 *points, size_t count, double expected_value_tolerance, bool occupancy_only,
                   std::vector<uint8_t> &status, std::vector<uint64_t> &kept_indices, std::vector<double> &values,
                   std::vector<CloudKey> &keys)
  {
    static_assert(sizeof(dvec3) == 3 * sizeof(double), "points are read as 3 doubles each");
    status.assign(count, 0);
    kept_indices.assign(count, 0);
    values.assign(count, 0.0);
    keys.assign(count, CloudKey{});
    if (!gpuOk() || !pushConfigIfChanged())
    {
      kept_indices.clear();
      return last_status_ = OHMHIP_ERR_INVALID_ARG;
    }
    ohmhip_point_filter_params p{};
    p.expected_value_tolerance = expected_value_tolerance;
    p.flags = occupancy_only ? OHMHIP_PF_OCCUPANCY_ONLY : 0u;
    uint64_t kept = 0;
    last_status_ = ohmhip_map_filter_points(handle_, count ? &points[0].x : nullptr, count, &p, count, status.data(),
                                            kept_indices.data(), values.data(), keys.data(), &kept);
    kept_indices.resize((last_status_ == OHMHIP_OK) ? size_t(kept) : 0);
    return last_status_;
  }

  // -- voxel edits by key (include/ohmhip.h, VOXEL EDITS) ------------------------------------------------------------
  /// What integrateVoxels does to a voxel (OHMHIP_EDIT_*).
  enum class VoxelEdit : uint8_t
  {
    kHit = OHMHIP_EDIT_HIT,              ///< ohm::integrateHit(map, key)
    kMiss = OHMHIP_EDIT_MISS,            ///< ohm::integrateMiss(map, key)
    kHitSample = OHMHIP_EDIT_HIT_SAMPLE  ///< ohm::integrateHit(map, sample): points only
  };

  /// Voxel<T>::write for many voxels (ohmhip_map_write_voxels): the ohmhip_layer_voxel_bytes(layer_id) bytes of every
  /// voxel at `keys` become those of `values`, stored as given; among duplicate keys the last wins, null keys are
  /// skipped, regions the map does not hold are created.  @return the status (lastStatus() too).
  int writeVoxels(int layer_id, const std::vector<CloudKey> &keys, const void *values)
  {
    last_edit_stats_ = ohmhip_voxel_edit_stats{};
    if (!gpuOk() || !pushConfigIfChanged())
    {
      return last_status_ = OHMHIP_ERR_INVALID_ARG;
    }
    return last_status_ = ohmhip_map_write_voxels(handle_, layer_id, keys.empty() ? nullptr : keys.data(), keys.size(),
                                                  values, &last_edit_stats_);
  }

  /// One VoxelEdit per element -- `ops`, or `op` for all of them when ops is null -- at `keys`, or at the voxels of
  /// `points` (exactly one of the two; ohmhip_map_integrate_voxels), per voxel in input order.
  int integrateVoxels(const VoxelEdit *ops, VoxelEdit op, const CloudKey *keys, const dvec3 *points, size_t count)
  {
    static_assert(sizeof(dvec3) == 3 * sizeof(double), "points are read as 3 doubles each");
    static_assert(sizeof(VoxelEdit) == 1, "ops are read as bytes");
    last_edit_stats_ = ohmhip_voxel_edit_stats{};
    if (!gpuOk() || !pushConfigIfChanged())
    {
      return last_status_ = OHMHIP_ERR_INVALID_ARG;
    }
    return last_status_ = ohmhip_map_integrate_voxels(handle_, reinterpret_cast<const uint8_t *>(ops), int(op), keys,
                                                      points ? &points[0].x : nullptr, count, &last_edit_stats_);
  }

  /// ohm::integrateHit(map, key) at every key.
  int integrateHits(const std::vector<CloudKey> &keys)
  {
    return integrateVoxels(nullptr, VoxelEdit::kHit, keys.data(), nullptr, keys.size());
  }
  /// ohm::integrateHit at the voxel of every point; with update_mean ohm::integrateHit(map, sample): the voxel mean
  /// takes the point as well.
  int integrateHits(const std::vector<dvec3> &points, bool update_mean = false)
  {
    return integrateVoxels(nullptr, update_mean ? VoxelEdit::kHitSample : VoxelEdit::kHit, nullptr, points.data(),
                           points.size());
  }
  /// ohm::integrateMiss(map, key) at every key / at the voxel of every point.
  int integrateMisses(const std::vector<CloudKey> &keys)
  {
    return integrateVoxels(nullptr, VoxelEdit::kMiss, keys.data(), nullptr, keys.size());
  }
  int integrateMisses(const std::vector<dvec3> &points)
  {
    return integrateVoxels(nullptr, VoxelEdit::kMiss, nullptr, points.data(), points.size());
  }
  /// The single-voxel conveniences, with the reference's names and meaning (ohm/VoxelOccupancy.h:73-77, 104-108,
  /// ohm/VoxelMean.h:196-203).
  int integrateHit(const CloudKey &key) { return integrateVoxels(nullptr, VoxelEdit::kHit, &key, nullptr, 1); }
  int integrateMiss(const CloudKey &key) { return integrateVoxels(nullptr, VoxelEdit::kMiss, &key, nullptr, 1); }
  int integrateHit(const dvec3 &sample) { return integrateVoxels(nullptr, VoxelEdit::kHitSample, nullptr, &sample, 1); }
  /// ohmhip_voxel_edit_stats of the last edit (all zero after one that failed).
  const ohmhip_voxel_edit_stats &lastEditStats() const { return last_edit_stats_; }

  /// ohm::KeyRange (ohm/KeyRange.h) of the closed box between two keys: its keys x fastest, then y, then z -- the order
  /// KeyRange::walkNext visits them in (ohm/KeyRange.cpp:105-129).  Empty when max lies below min on any axis.
  std::vector<CloudKey> keyRange(const CloudKey &min_key, const CloudKey &max_key) const
  {
    const int *dim = map_->regionVoxelDimensions();
    long lo[3], hi[3];
    for (int a = 0; a < 3; ++a)
    {
      lo[a] = long(min_key.region[a]) * dim[a] + min_key.voxel[a];
      hi[a] = long(max_key.region[a]) * dim[a] + max_key.voxel[a];
      if (hi[a] < lo[a])
      {
        return {};
      }
    }
    std::vector<CloudKey> keys;
    keys.reserve(size_t(hi[0] - lo[0] + 1) * size_t(hi[1] - lo[1] + 1) * size_t(hi[2] - lo[2] + 1));
    for (long z = lo[2]; z <= hi[2]; ++z)
    {
      for (long y = lo[1]; y <= hi[1]; ++y)
      {
        for (long x = lo[0]; x <= hi[0]; ++x)
        {
          const long g[3] = { x, y, z };
          CloudKey k{};
          for (int a = 0; a < 3; ++a)
          {
            long r = g[a] / dim[a];
            r -= (g[a] - r * dim[a] < 0) ? 1 : 0;
            k.region[a] = int16_t(r);
            k.voxel[a] = uint8_t(g[a] - r * dim[a]);
          }
          keys.push_back(k);
        }
      }
    }
    return keys;
  }
  /// ... between the voxels of two points (voxelKeys).
  std::vector<CloudKey> keyRange(const dvec3 &min_point, const dvec3 &max_point)
  {
    const dvec3 ends[2] = { min_point, max_point };
    const std::vector<CloudKey> keys = voxelKeys(ends, 2);
    return (last_status_ == OHMHIP_OK) ? keyRange(keys[0], keys[1]) : std::vector<CloudKey>();
  }

  ohmhip_map_t handle() const { return handle_; }
  /// OccupancyMap::clone (ohm/OccupancyMap.cpp:953-1004) on the device: a new map of the same class, configuration and
  /// layers, which owns its (empty) host map, then the regions that pass the extents rule of copyFilterExtents, copied
  /// device to device (ohmhip_map_copy).  Without extents: every region.  Null when the copy fails (lastStatus()).
  std::unique_ptr<GpuMap> clone() const
  {
    const double inf = std::numeric_limits<double>::infinity();
    return clone(dvec3{ -inf, -inf, -inf }, dvec3{ inf, inf, inf });
  }
  std::unique_ptr<GpuMap> clone(const dvec3 &min_ext, const dvec3 &max_ext) const;
  /// Push the map's current parameters (threshold, built-in ray filter, ...) to the device, as a batch would: what a
  /// query of the map (RaysQueryGpu) calls first.  @return false when the device refuses them.
  bool syncConfig() { return pushConfigIfChanged(); }

protected:
  using ConfigHook = void (*)(ohmhip_map_config &, void *);
  GpuMap(OccupancyMap *map, bool borrowed_map, unsigned expected_element_count, size_t gpu_mem_size, int mode,
         void *hook_data, ConfigHook hook = nullptr)
    : map_(map)
    , borrowed_map_(borrowed_map)
  {
    ohmhip_map_config &cfg = cfg_;
    std::memset(&cfg, 0, sizeof(cfg));
    ohmhip_map_config_default(&cfg);
    cfg.resolution = map->resolution();
    for (int a = 0; a < 3; ++a)
    {
      cfg.region_dim[a] = map->regionVoxelDimensions()[a];
      cfg.origin[a] = map->origin()[a];
    }
    cfg.mode = mode;
    fillMapValues(cfg);
    cfg.gpu_mem_size = gpu_mem_size;
    if (hook)
    {
      hook(cfg, hook_data);
    }
    cfg.layers = map->layers();
    // gputil::Exception on allocation failure from the ctor (ohmgpu/GpuMap.h:53-54,159-160).
    OHMHIP_GPUAPICHECK(ohmhip_map_create(&handle_, &cfg));
    if (expected_element_count > 2048u)
    {
      // the reference sizes its ray / key buffers for expected_element_count points here (ohmgpu/GpuMap.cpp:429-470)
      // (best effort: a reservation the device cannot hold is not an error, the batches grow their buffers on demand)
      (void)ohmhip_map_reserve_rays(handle_, expected_element_count / 2u);
    }
    uploadExisting();
  }

  /// The host map's probabilities, clamps and built-in filter.
  void fillMapValues(ohmhip_map_config &cfg) const
  {
    cfg.hit_value = map_->hitValue();
    cfg.miss_value = map_->missValue();
    cfg.threshold_value = map_->occupancyThresholdValue();
    cfg.min_value = map_->minVoxelValue();
    cfg.max_value = map_->maxVoxelValue();
    cfg.saturate_at_min = map_->saturateAtMinValue();
    cfg.saturate_at_max = map_->saturateAtMaxValue();
    cfg.ray_filter = map_->rayFilterMode();
    cfg.ray_filter_range = map_->rayFilterRange();
  }
  /// Mapper-specific parameters (NDT, TSDF) as they stand now.
  virtual void fillMapperValues(ohmhip_map_config &) const {}
  /// A map of this class and configuration over `map`, which it owns (clone()).
  virtual GpuMap *newLike(OccupancyMap *map) const { return new GpuMap(map, false, 2048, size_t(cfg_.gpu_mem_size)); }

  /// The reference reads the map's parameters at every launch (ohmgpu/GpuMap.cpp:1036-1191): setters called on the
  /// OccupancyMap / mapper after construction apply from the next batch.
  /// @return false when the device refuses the new values (lastStatus() says why); nothing is integrated then.
  bool pushConfigIfChanged()
  {
    ohmhip_map_config now = cfg_;
    fillMapValues(now);
    fillMapperValues(now);
    if (std::memcmp(&now, &cfg_, sizeof(now)) != 0)
    {
      last_status_ = ohmhip_map_update_config(handle_, &now);
      if (last_status_ != OHMHIP_OK)
      {
        return false;
      }
      cfg_ = now;
    }
    return true;
  }

  /// gpumap::enableGpu + GpuLayerCache::upload for chunks the CPU map already holds.
  void uploadExisting() { uploadRegions(nullptr, 0); }

public:
  /// Push host chunks to the device: all of them (keys_xyz == nullptr) or the listed regions -- what
  /// GpuLayerCache::upload does for a region whose CPU copy is newer than the device's
  /// (ohmgpu/GpuLayerCache.cpp:172-182), e.g. after CPU-side integration into the host map.
  void uploadRegions(const int16_t *keys_xyz, size_t count)
  {
    for (int layer = 0; layer < OHMHIP_LID_COUNT; ++layer)
    {
      if (!map_->hasLayer(layer))
      {
        continue;
      }
      std::vector<const void *> srcs;
      std::vector<int16_t> layer_keys;
      auto take = [&](const std::array<int16_t, 3> &key, const MapChunk &chunk) {
        if (chunk.voxel_blocks.size() > size_t(layer) && !chunk.voxel_blocks[layer].empty())
        {
          srcs.push_back(chunk.voxel_blocks[layer].data());
          layer_keys.insert(layer_keys.end(), key.begin(), key.end());
        }
      };
      if (!keys_xyz)
      {
        for (const auto &entry : map_->chunks())
        {
          take(entry.first, entry.second);
        }
      }
      else
      {
        for (size_t i = 0; i < count; ++i)
        {
          const std::array<int16_t, 3> key{ { keys_xyz[3 * i], keys_xyz[3 * i + 1], keys_xyz[3 * i + 2] } };
          const auto found = map_->chunks().find(key);
          if (found != map_->chunks().end())
          {
            take(found->first, found->second);
          }
        }
      }
      if (!srcs.empty())
      {
        OHMHIP_GPUAPICHECK(ohmhip_map_write_regions(handle_, layer, layer_keys.data(), srcs.size(), srcs.data()));
      }
    }
  }

protected:
  OccupancyMap *map_ = nullptr;
  bool borrowed_map_ = true;
  ohmhip_map_t handle_ = nullptr;
  double ray_segment_length_ = 0;
  bool grouped_rays_ = false;
  int last_status_ = OHMHIP_OK;
  ohmhip_voxel_edit_stats last_edit_stats_{};
  size_t last_partial_ = 0;
  unsigned partition_world_ = 1;
  void clearDeviceRayFilter()
  {
    if (!device_ray_filter_.stages().empty() && gpuOk())
    {
      last_status_ = ohmhip_map_set_ray_filter_stages(handle_, nullptr, 0);
    }
    device_ray_filter_ = DeviceRayFilter();
  }
  RayFilterFunction ray_filter_;
  DeviceRayFilter device_ray_filter_;  ///< the chain set on the device (empty: none)
  bool time_base_checked_ = false;  ///< a stamped call under a host filter has seen to the time base
  ohmhip_map_config cfg_;
  ohmhip_layer_change_stats last_layer_change_{};
  GpuCache cache_view_{ this };
};

/// ohm::GpuNdtMap (ohmgpu/GpuNdtMap.h:63-132).  NDT parameters default as in ohm/private/NdtMapDetail.h:20-45 and may
/// be changed BEFORE construction through NdtParams.
struct NdtParams
{
  float sensor_noise = 0.05f;
  unsigned sample_threshold = 3;
  float adaptation_rate = -1.0f;  ///< <= 0: derived from the map's miss probability (ohm/NdtMap.cpp:31-36)
  float reinitialise_covariance_threshold = probabilityToValue(0.2f);
  unsigned reinitialise_covariance_point_count = 100;
  float initial_intensity_covariance = 1.0f;
};

class GpuNdtMap : public GpuMap
{
public:
  GpuNdtMap(OccupancyMap *map, bool borrowed_map = true, unsigned expected_element_count = 2048,
            size_t gpu_mem_size = 0, NdtMode ndt_mode = NdtMode::kOccupancy, const NdtParams &params = NdtParams())
    : GpuMap(prepare(map, ndt_mode), borrowed_map, expected_element_count, gpu_mem_size,
             ndt_mode == NdtMode::kTraversability ? OHMHIP_MODE_NDT_TM : OHMHIP_MODE_NDT_OM,
             const_cast<NdtParams *>(&params), &GpuNdtMap::fill)
    , params_(params)
    , mode_(ndt_mode)
  {}
  NdtMode mode() const { return mode_; }
  float sensorNoise() const { return params_.sensor_noise; }
  /// ohmgpu/GpuNdtMap.h (setSensorNoise) and the NdtMap setters reached through ndtMap() in the reference
  /// (ohm/NdtMap.h:100-160): apply from the next batch.
  void setSensorNoise(float noise) { params_.sensor_noise = noise; }
  void setSampleThreshold(unsigned count) { params_.sample_threshold = count; }
  void setAdaptationRate(float rate) { params_.adaptation_rate = rate; }
  void setReinitialiseCovarianceThreshold(float value) { params_.reinitialise_covariance_threshold = value; }
  void setReinitialiseCovariancePointCount(unsigned count) { params_.reinitialise_covariance_point_count = count; }
  const NdtParams &ndtParams() const { return params_; }

protected:
  void fillMapperValues(ohmhip_map_config &cfg) const override { fill(cfg, const_cast<NdtParams *>(&params_)); }
  GpuMap *newLike(OccupancyMap *map) const override
  {
    return new GpuNdtMap(map, false, 2048, size_t(cfg_.gpu_mem_size), mode_, params_);
  }

public:

  /// ohm/NdtMap.h:146-149
  static float ndtAdaptationRateFromMissProbability(float miss_probability, float scale = 2.0f)
  {
    return std::max(0.0f, std::min(scale * (1.0f - 2.0f * miss_probability), 1.0f));
  }

private:
  static OccupancyMap *prepare(OccupancyMap *map, NdtMode mode)
  {
    // NdtMap::enableNdt (ohm/NdtMap.cpp:194-213): voxel mean + covariance (+ intensity, hit/miss for NDT-TM).
    map->addLayer(OHMHIP_LID_OCCUPANCY);
    map->addLayer(OHMHIP_LID_MEAN);
    map->addLayer(OHMHIP_LID_COVARIANCE);
    if (mode == NdtMode::kTraversability)
    {
      map->addLayer(OHMHIP_LID_INTENSITY);
      map->addLayer(OHMHIP_LID_HIT_MISS);
    }
    return map;
  }
  static void fill(ohmhip_map_config &cfg, void *data)
  {
    const NdtParams &p = *static_cast<const NdtParams *>(data);
    cfg.ndt_sensor_noise = p.sensor_noise;
    cfg.ndt_sample_threshold = p.sample_threshold;
    // cfg.miss_value is already the map's; derive the rate exactly as NdtMap's ctor does.
    cfg.ndt_adaptation_rate = (p.adaptation_rate > 0) ?
                                p.adaptation_rate :
                                ndtAdaptationRateFromMissProbability(valueToProbability(cfg.miss_value));
    cfg.ndt_reinit_threshold = p.reinitialise_covariance_threshold;
    cfg.ndt_reinit_count = p.reinitialise_covariance_point_count;
    cfg.ndt_initial_intensity_cov = p.initial_intensity_covariance;
  }
  NdtParams params_;
  NdtMode mode_;
};

/// ohm/VoxelTsdf.h:27-37
struct TsdfOptions
{
  float max_weight = 1e4f;
  float default_truncation_distance = 0.1f;
  float dropoff_epsilon = 0.0f;
  float sparsity_compensation_factor = 1.0f;
};

/// ohm::GpuTsdfMap (ohmgpu/GpuTsdfMap.h:37-94)
class GpuTsdfMap : public GpuMap
{
public:
  GpuTsdfMap(OccupancyMap *map, bool borrowed_map = true, unsigned expected_element_count = 2048,
             size_t gpu_mem_size = 0, const TsdfOptions &options = TsdfOptions())
    : GpuMap(prepare(map), borrowed_map, expected_element_count, gpu_mem_size, OHMHIP_MODE_TSDF,
             const_cast<TsdfOptions *>(&options), &GpuTsdfMap::fill)
    , options_(options)
  {}
  const TsdfOptions &tsdfOptions() const { return options_; }
  float maxWeight() const { return options_.max_weight; }
  float defaultTruncationDistance() const { return options_.default_truncation_distance; }
  /// ohmgpu/GpuTsdfMap.h:37-94 setters: apply from the next batch.
  void setTsdfOptions(const TsdfOptions &options) { options_ = options; }
  void setMaxWeight(float max_weight) { options_.max_weight = max_weight; }
  void setDefaultTruncationDistance(float distance) { options_.default_truncation_distance = distance; }
  void setSparsityCompensationFactor(float factor) { options_.sparsity_compensation_factor = factor; }
  float sparsityCompensationFactor() const { return options_.sparsity_compensation_factor; }
  void setDropoffEpsilon(float dropoff_epsilon) { options_.dropoff_epsilon = dropoff_epsilon; }
  float dropoffEpsilon() const { return options_.dropoff_epsilon; }

protected:
  void fillMapperValues(ohmhip_map_config &cfg) const override { fill(cfg, const_cast<TsdfOptions *>(&options_)); }
  GpuMap *newLike(OccupancyMap *map) const override
  {
    return new GpuTsdfMap(map, false, 2048, size_t(cfg_.gpu_mem_size), options_);
  }

public:

private:
  static OccupancyMap *prepare(OccupancyMap *map)
  {
    map->addLayer(OHMHIP_LID_TSDF);
    return map;
  }
  static void fill(ohmhip_map_config &cfg, void *data)
  {
    const TsdfOptions &o = *static_cast<const TsdfOptions *>(data);
    cfg.tsdf_max_weight = o.max_weight;
    cfg.tsdf_trunc = o.default_truncation_distance;
    cfg.tsdf_dropoff = o.dropoff_epsilon;
    cfg.tsdf_sparsity = o.sparsity_compensation_factor;
  }
  TsdfOptions options_;
};

// ---------------------------------------------------------------------------------------------------------------------
// ohm/CopyUtil.h over ohmhip_map_copy (include/ohmhip.h, MAP COPY): canCopy, copyMap and the filter helpers on two
// GpuMaps.  The copy runs device to device in one kernel launch.

/// What a CopyChunkFilter sees of a MapChunk: the region coordinate, MapRegion::centre -- coord * region spatial
/// dimensions, WITHOUT the map origin (ohm/MapRegion.cpp:40-42) --, whether the region changed since the last
/// syncVoxels(), and the map's region spatial dimensions.
struct CopyChunk
{
  std::array<int16_t, 3> coord;
  dvec3 centre;
  bool dirty;
  dvec3 region_spatial_dimensions;
};

/// An empty filter is an implied pass (CopyUtil.h:23-28).
using CopyChunkFilter = std::function<bool(const CopyChunk &)>;
using CopyLayerFilter = std::function<bool(const std::string &)>;

/// The layer names of ohm/DefaultLayer.cpp by OHMHIP_LID_*.
inline const char *copyLayerName(int layer_id)
{
  static const char *const names[OHMHIP_LID_COUNT] = { "occupancy", "mean",      "covariance",     "traversal", "touch_time",
                                                       "incident_normal", "intensity", "hit_miss_count", "tsdf",      "clearance" };
  return (layer_id >= 0 && layer_id < OHMHIP_LID_COUNT) ? names[layer_id] : "";
}

/// copyFilterExtents (CopyUtil.cpp:37-45) in its operation order.  Used alone it goes down as OHMHIP_COPY_USE_EXTENTS.
struct CopyFilterExtents
{
  dvec3 min_ext, max_ext;
  bool operator()(const CopyChunk &chunk) const
  {
    const double dims[3] = { chunk.region_spatial_dimensions.x, chunk.region_spatial_dimensions.y, chunk.region_spatial_dimensions.z };
    const double centre[3] = { chunk.centre.x, chunk.centre.y, chunk.centre.z };
    const double mn[3] = { min_ext.x, min_ext.y, min_ext.z }, mx[3] = { max_ext.x, max_ext.y, max_ext.z };
    bool below = false, above = false;
    for (int a = 0; a < 3; ++a)
    {
      const double half = 0.5 * dims[a];
      const double lo = centre[a] - half;
      const double hi = centre[a] + half;
      below = below || hi < mn[a];
      above = above || lo > mx[a];
    }
    return !below && !above;
  }
};

/// In the place of copyFilterStamp (CopyUtil.cpp:47-50): the device map keeps dirty bits, not stamps.  Used alone it
/// goes down as OHMHIP_COPY_DIRTY_ONLY.
struct CopyFilterDirty
{
  bool operator()(const CopyChunk &chunk) const { return chunk.dirty; }
};

inline CopyChunkFilter copyFilterExtents(const dvec3 &min_ext, const dvec3 &max_ext)
{
  return CopyFilterExtents{ min_ext, max_ext };
}
inline CopyChunkFilter copyFilterDirty() { return CopyFilterDirty{}; }

/// CopyUtil.h:50-57
inline CopyChunkFilter copyFilterAnd(const CopyChunkFilter &filter_a, const CopyChunkFilter &filter_b)
{
  if (!filter_a || !filter_b)
  {
    return filter_a ? filter_a : filter_b;
  }
  return [filter_a, filter_b](const CopyChunk &chunk) { return filter_a(chunk) && filter_b(chunk); };
}

/// CopyUtil.h:67-75: an empty operand is an implied pass, so the result is empty.
inline CopyChunkFilter copyFilterOr(const CopyChunkFilter &filter_a, const CopyChunkFilter &filter_b)
{
  if (!filter_a || !filter_b)
  {
    return {};
  }
  return [filter_a, filter_b](const CopyChunk &chunk) { return filter_a(chunk) || filter_b(chunk); };
}

/// CopyUtil.h:81-91: the negation of an empty filter passes nothing.
inline CopyChunkFilter copyFilterNegate(const CopyChunkFilter &filter)
{
  if (filter)
  {
    return [filter](const CopyChunk &chunk) { return !filter(chunk); };
  }
  return [](const CopyChunk &) { return false; };
}

/// CopyUtil.h:96-101
inline CopyLayerFilter copyLayersFilter(const std::vector<std::string> &layers)
{
  return [layers](const std::string &name) { return std::find(layers.begin(), layers.end(), name) != layers.end(); };
}

/// CopyUtil.h:107-117
inline CopyLayerFilter copyFilterNegate(const CopyLayerFilter &filter)
{
  if (filter)
  {
    return [filter](const std::string &name) { return !filter(name); };
  }
  return [](const std::string &) { return false; };
}

/// ohm::canCopy (CopyUtil.cpp:52-56)
inline bool canCopy(const GpuMap &dst, const GpuMap &src)
{
  return ohmhip_map_can_copy(dst.handle(), src.handle()) == OHMHIP_OK;
}

/// ohm::copyMap (CopyUtil.cpp:58-165) from src into dst.  False where the reference returns false (canCopy fails, no
/// layer in common) and when the device call fails (status, when given, says how: OHMHIP_ERR_CAPACITY under dst's
/// memory limit, OHMHIP_ERR_UNSUPPORTED for partitioned or merging maps).  A filter other than copyFilterExtents /
/// copyFilterDirty alone is evaluated over src's regions on the host and the surviving keys are passed.
inline bool copyMap(GpuMap &dst, const GpuMap &src, const CopyChunkFilter &copy_chunk_filter = {},
                    const CopyLayerFilter &copy_layer_filter = {}, ohmhip_copy_stats *stats = nullptr, int *status = nullptr)
{
  int local_status = OHMHIP_OK;
  int &st = status ? *status : local_status;
  st = OHMHIP_ERR_INVALID_ARG;
  if (stats)
  {
    std::memset(stats, 0, sizeof(*stats));
  }
  if (!canCopy(dst, src))
  {
    return false;
  }
  const unsigned common = dst.map().layers() & src.map().layers();
  if (common == 0)
  {
    st = OHMHIP_ERR_NOT_FOUND;
    return false;
  }
  ohmhip_copy_params params;
  std::memset(&params, 0, sizeof(params));
  if (copy_layer_filter)
  {
    for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
    {
      if ((common & OHMHIP_LAYER_BIT(l)) && copy_layer_filter(copyLayerName(l)))
      {
        params.layers |= OHMHIP_LAYER_BIT(l);
      }
    }
    if (params.layers == 0)
    {
      // every common layer is filtered out: the regions are still created (:117-126).  0 means "all" in the C ABI, so
      // the request is spelt with layers that are not common.
      params.layers = (OHMHIP_LAYER_BIT(OHMHIP_LID_COUNT) - 1u) & ~common;
      if (params.layers == 0)
      {
        st = OHMHIP_ERR_UNSUPPORTED;
        return false;
      }
    }
  }
  std::vector<int16_t> keys;
  if (const CopyFilterExtents *extents = copy_chunk_filter.target<CopyFilterExtents>())
  {
    params.flags = OHMHIP_COPY_USE_EXTENTS;
    const double mn[3] = { extents->min_ext.x, extents->min_ext.y, extents->min_ext.z };
    const double mx[3] = { extents->max_ext.x, extents->max_ext.y, extents->max_ext.z };
    std::copy(mn, mn + 3, params.min_extents);
    std::copy(mx, mx + 3, params.max_extents);
  }
  else if (copy_chunk_filter.target<CopyFilterDirty>())
  {
    params.flags = OHMHIP_COPY_DIRTY_ONLY;
  }
  else if (copy_chunk_filter)
  {
    std::vector<std::array<int16_t, 3>> all, dirty;
    if ((st = fetchRegions(src.handle(), false, all)) != OHMHIP_OK ||
        (st = fetchRegions(src.handle(), true, dirty)) != OHMHIP_OK)
    {
      return false;
    }
    std::sort(dirty.begin(), dirty.end());
    const int *dim = src.map().regionVoxelDimensions();
    const dvec3 spatial{ dim[0] * src.map().resolution(), dim[1] * src.map().resolution(), dim[2] * src.map().resolution() };
    for (const std::array<int16_t, 3> &coord : all)
    {
      CopyChunk chunk;
      chunk.coord = coord;
      chunk.centre = dvec3{ double(coord[0]) * spatial.x, double(coord[1]) * spatial.y, double(coord[2]) * spatial.z };
      chunk.dirty = std::binary_search(dirty.begin(), dirty.end(), coord);
      chunk.region_spatial_dimensions = spatial;
      if (copy_chunk_filter(chunk))
      {
        keys.insert(keys.end(), coord.begin(), coord.end());
      }
    }
    if (keys.empty())
    {
      st = OHMHIP_OK;
      return true;  // (every chunk excluded: CopyUtil.cpp:117-123 visits none)
    }
    params.keys_xyz = keys.data();
    params.key_count = keys.size() / 3;
  }
  st = ohmhip_map_copy(dst.handle(), src.handle(), &params, stats);
  return st == OHMHIP_OK;
}

inline std::unique_ptr<GpuMap> GpuMap::clone(const dvec3 &min_ext, const dvec3 &max_ext) const
{
  std::unique_ptr<OccupancyMap> host_map(new OccupancyMap(*map_));
  host_map->chunks().clear();
  std::unique_ptr<GpuMap> other(newLike(host_map.get()));
  host_map.release();  // (owned by `other`: borrowed_map == false)
  if (!copyMap(*other, *this, copyFilterExtents(min_ext, max_ext)))
  {
    return nullptr;
  }
  return other;
}

// ---------------------------------------------------------------------------------------------------------------------
// ohm/CompareMaps.h over ohmhip_map_compare (include/ohmhip.h, MAP COMPARE): compareLayoutLayer, compareVoxels and
// configureTolerance on two GpuMaps.  The comparison runs on the device; the result and the listed mismatches cross over.
namespace compare
{
/// ohm::compare::Severity
enum class Severity
{
  kInfo,
  kWarning,
  kError
};

/// ohm::compare::Flag
enum Flag : unsigned
{
  kZero = 0u,
  kContinue = OHMHIP_CMP_CONTINUE
};

/// ohm::compare::VoxelsResult, and beside it what the device call reports: every field of ohmhip_compare_result, the
/// listed mismatches (voxel[3] = the mask of failing members) and the listed regions the evaluated map lacks.
struct VoxelsResult
{
  size_t voxels_passed = 0;
  size_t voxels_failed = 0;
  bool layout_match = false;
  int status = OHMHIP_OK;
  ohmhip_compare_result detail{};
  std::vector<CloudKey> mismatches;
  std::vector<std::array<int16_t, 3>> missing_regions;
  explicit operator bool() const { return voxels_failed == 0 && layout_match; }
};

using Log = std::function<void(Severity, const std::string &)>;
inline void emptyLog(Severity, const std::string &) {}

/// The members of a layer in voxel order, all 4 bytes (ohm/DefaultLayer.cpp:85-303); is_float[i] says how member i reads.
struct LayerMembers
{
  std::vector<std::string> names;
  unsigned float_mask = 0;
};

inline LayerMembers layerMembers(int layer_id)
{
  switch (layer_id)
  {
  case OHMHIP_LID_OCCUPANCY: return { { "occupancy" }, 0x1u };
  case OHMHIP_LID_MEAN: return { { "coord", "count" }, 0x0u };
  case OHMHIP_LID_COVARIANCE: return { { "P00", "P01", "P11", "P02", "P12", "P22" }, 0x3fu };
  case OHMHIP_LID_TRAVERSAL: return { { "traversal" }, 0x1u };
  case OHMHIP_LID_TOUCH_TIME: return { { "touch" }, 0x0u };
  case OHMHIP_LID_INCIDENT: return { { "packed_normal" }, 0x0u };
  case OHMHIP_LID_INTENSITY: return { { "mean", "cov" }, 0x3u };
  case OHMHIP_LID_HIT_MISS: return { { "hit_count", "miss_count" }, 0x0u };
  case OHMHIP_LID_TSDF: return { { "weight", "distance" }, 0x3u };
  case OHMHIP_LID_CLEARANCE: return { { "clearance" }, 0x1u };
  default: return {};
  }
}

inline int layerIdByName(const std::string &layer_name)
{
  for (int l = 0; l < OHMHIP_LID_COUNT; ++l)
  {
    if (layer_name == copyLayerName(l))
    {
      return l;
    }
  }
  return -1;
}

/// Stands for the reference's dummy MapLayer: member names with the 64-bit clear values that hold the allowed errors.
/// The compared member's own type reads the stored bytes (CompareMaps.cpp:248-304).
struct Tolerance
{
  explicit Tolerance(std::string layer) : layer_name(std::move(layer)) {}
  std::string layer_name;
  std::vector<std::pair<std::string, uint64_t>> members;
  int indexOf(const std::string &member_name) const
  {
    for (size_t i = 0; i < members.size(); ++i)
    {
      if (members[i].first == member_name)
      {
        return int(i);
      }
    }
    return -1;
  }
};

/// ohm::compare::configureTolerance (CompareMaps.cpp:396-469): the absolute value, its typed bytes in the low end.
inline void configureTolerance(Tolerance &layer, const char *member_name, float epsilon)
{
  epsilon = std::fabs(epsilon);
  uint64_t e = 0;
  std::memcpy(&e, &epsilon, sizeof(epsilon));
  layer.members.emplace_back(member_name, e);
}
inline void configureTolerance(Tolerance &layer, const char *member_name, double epsilon)
{
  epsilon = std::fabs(epsilon);
  uint64_t e = 0;
  std::memcpy(&e, &epsilon, sizeof(epsilon));
  layer.members.emplace_back(member_name, e);
}
inline void configureTolerance(Tolerance &layer, const char *member_name, uint8_t epsilon) { layer.members.emplace_back(member_name, uint64_t(epsilon)); }
inline void configureTolerance(Tolerance &layer, const char *member_name, uint16_t epsilon) { layer.members.emplace_back(member_name, uint64_t(epsilon)); }
inline void configureTolerance(Tolerance &layer, const char *member_name, uint32_t epsilon) { layer.members.emplace_back(member_name, uint64_t(epsilon)); }
inline void configureTolerance(Tolerance &layer, const char *member_name, uint64_t epsilon) { layer.members.emplace_back(member_name, epsilon); }
inline void configureTolerance(Tolerance &layer, const char *member_name, int8_t epsilon) { layer.members.emplace_back(member_name, uint64_t(std::abs(int(epsilon)))); }
inline void configureTolerance(Tolerance &layer, const char *member_name, int16_t epsilon) { layer.members.emplace_back(member_name, uint64_t(std::abs(int(epsilon)))); }
inline void configureTolerance(Tolerance &layer, const char *member_name, int32_t epsilon) { layer.members.emplace_back(member_name, uint64_t(std::llabs(int64_t(epsilon)))); }
inline void configureTolerance(Tolerance &layer, const char *member_name, int64_t epsilon) { layer.members.emplace_back(member_name, uint64_t(epsilon < 0 ? -uint64_t(epsilon) : uint64_t(epsilon))); }

/// ohm::compare::compareLayoutLayer (CompareMaps.cpp:78-144): a layer has one layout in this library, so what is left to
/// check is that both maps hold it.
inline bool compareLayoutLayer(const GpuMap &eval_map, const GpuMap &ref_map, const std::string &layer_name, unsigned flags = 0,
                               const Log &log = emptyLog)
{
  (void)flags;
  const int layer = layerIdByName(layer_name);
  bool ok = true;
  if (layer < 0 || !ref_map.map().hasLayer(layer))
  {
    log(Severity::kError, "the reference map holds no layer named " + layer_name);
    ok = false;
  }
  if (layer < 0 || !eval_map.map().hasLayer(layer))
  {
    log(Severity::kError, "the evaluated map holds no layer named " + layer_name);
    ok = false;
  }
  return ok;
}

/// ohm::compare::compareVoxels (CompareMaps.cpp:334-386) on the device.  With a log other than emptyLog the first
/// max_logged failing voxels of regions both maps hold are fetched (readVoxels) and reported member by member at
/// Severity::kError; the two lists of the result hold up to max_logged entries either way.
inline VoxelsResult compareVoxels(GpuMap &eval_map, GpuMap &ref_map, const std::string &layer_name,
                                  const Tolerance *tolerance = nullptr, unsigned flags = 0, const Log &log = emptyLog,
                                  size_t max_logged = 1024)
{
  VoxelsResult result;
  if (!compareLayoutLayer(eval_map, ref_map, layer_name, flags, log))
  {
    return result;
  }
  const int layer = layerIdByName(layer_name);
  const LayerMembers members = layerMembers(layer);
  ohmhip_compare_params params;
  std::memset(&params, 0, sizeof(params));
  params.flags = flags;
  params.layer_id = layer;
  for (size_t i = 0; tolerance && i < members.names.size(); ++i)
  {
    const int at = tolerance->indexOf(members.names[i]);
    if (at != -1)
    {
      params.tolerance_members |= 1u << i;
      params.tolerance_bits[i] = tolerance->members[size_t(at)].second;
    }
  }
  result.mismatches.resize(max_logged);
  std::vector<int16_t> missing(3 * max_logged);
  result.status = ohmhip_map_compare(eval_map.handle(), ref_map.handle(), &params, max_logged,
                                     max_logged ? result.mismatches.data() : nullptr, max_logged,
                                     max_logged ? missing.data() : nullptr, &result.detail);
  if (result.status != OHMHIP_OK)
  {
    result.mismatches.clear();
    return result;
  }
  result.voxels_passed = size_t(result.detail.voxels_passed);
  result.voxels_failed = size_t(result.detail.voxels_failed);
  result.layout_match = result.detail.layout_match != 0;
  result.mismatches.resize(size_t(std::min<uint64_t>(result.detail.mismatch_count, max_logged)));
  for (size_t i = 0; i < size_t(std::min<uint64_t>(result.detail.missing_count, max_logged)); ++i)
  {
    result.missing_regions.push_back({ { missing[3 * i], missing[3 * i + 1], missing[3 * i + 2] } });
  }
  if (log.target<void (*)(Severity, const std::string &)>() &&
      *log.target<void (*)(Severity, const std::string &)>() == &emptyLog)
  {
    return result;
  }
  std::vector<CloudKey> where = result.mismatches;
  for (CloudKey &key : where)
  {
    key.voxel[3] = 0;
  }
  std::vector<uint8_t> have, expect, present;
  if (where.empty() || eval_map.readVoxels(layer, where, have, present) != OHMHIP_OK ||
      ref_map.readVoxels(layer, where, expect, present) != OHMHIP_OK)
  {
    return result;
  }
  const size_t count = members.names.size();
  for (size_t n = 0; n < where.size(); ++n)
  {
    for (size_t i = 0; i < count; ++i)
    {
      if (!((result.mismatches[n].voxel[3] >> i) & 1u))
      {
        continue;
      }
      uint32_t h, e;
      std::memcpy(&h, &have[(n * count + i) * 4], 4);
      std::memcpy(&e, &expect[(n * count + i) * 4], 4);
      std::string text = layer_name + " voxel (" + std::to_string(where[n].region[0]) + "," + std::to_string(where[n].region[1]) +
                         "," + std::to_string(where[n].region[2]) + "):(" + std::to_string(where[n].voxel[0]) + "," +
                         std::to_string(where[n].voxel[1]) + "," + std::to_string(where[n].voxel[2]) + ") differs in " +
                         members.names[i] + ": eval holds ";
      if ((members.float_mask >> i) & 1u)
      {
        float hf, ef;
        std::memcpy(&hf, &h, 4);
        std::memcpy(&ef, &e, 4);
        text += std::to_string(hf) + ", ref holds " + std::to_string(ef);
      }
      else
      {
        text += std::to_string(h) + ", ref holds " + std::to_string(e);
      }
      log(Severity::kError, text);
    }
  }
  return result;
}
}  // namespace compare

/// Quaternion in (x, y, z, w) member order (glm::dquat exposes the same members; its memory order depends on the glm
/// version, ohmgpu/GpuTransformSamples.cpp:169-174).
struct dquat
{
  double x, y, z, w;
};

/// ohm::GpuTransformSamples (ohmgpu/GpuTransformSamples.h:30-83): sensor-frame samples + timestamped trajectory ->
/// world-frame ray pairs in a device buffer.  fp64 on the device (the reference kernel is fp32).
class GpuTransformSamples
{
public:
  explicit GpuTransformSamples(gputil::Device &) {}
  GpuTransformSamples() = default;

  /// @return 2 x the number of valid samples written to @p output_buffer (as the reference), 0 on failure.
  unsigned transform(const double *transform_times, const dvec3 *transform_translations, const dquat *transform_rotations,
                     unsigned transform_count, const double *sample_times, const dvec3 *local_samples,
                     unsigned point_count, gputil::Queue &gpu_queue, gputil::Buffer &output_buffer,
                     double max_range = INFINITY)
  {
    if (!output_buffer.isValid())
    {
      output_buffer.create(sizeof(double) * 6 * (point_count ? point_count : 1u));
    }
    uint32_t elements = 0;
    last_status_ = ohmhip_transform_samples(
      transform_times, reinterpret_cast<const double *>(transform_translations),
      reinterpret_cast<const double *>(transform_rotations), transform_count, sample_times,
      reinterpret_cast<const double *>(local_samples), point_count, max_range, gpu_queue.handle(),
      output_buffer.handle(), &elements);
    return (last_status_ == OHMHIP_OK) ? elements : 0u;
  }
  int lastStatus() const { return last_status_; }

private:
  int last_status_ = OHMHIP_OK;
};

/// ohm::Query (ohm/Query.h:51-121) over a GpuMap: the map, the query flags, the result arrays every query shares and the
/// execute / reset protocol.  A query derives from it and provides onExecute() and, if it holds more than the shared
/// results, onReset(); one that always evaluates on the device names kQfGpuEvaluate in forcedQueryFlags().  The device
/// calls are synchronous, so the asynchronous forms complete at once (ohm/Query.h:103-121).  The accessors here are
/// ohm::Query's; a query whose reference class reports another type declares its own of the same name, which hides
/// them: LineQueryGpu::ranges() are floats kept in an array of its own (through a Query& its ranges() is null), and
/// NearestNeighbours returns the two shared arrays as vectors.
class Query
{
public:
  virtual ~Query() = default;

  void setGpuMap(GpuMap *gpu_map) { gpu_map_ = gpu_map; }
  GpuMap *gpuMap() const { return gpu_map_; }
  unsigned queryFlags() const { return query_flags_ | forcedQueryFlags(); }
  void setQueryFlags(unsigned flags) { query_flags_ = flags; }

  size_t numberOfResults() const { return number_of_results_; }
  const Key *intersectedVoxels() const { return intersected_voxels_.data(); }
  /// Null for a query that reports no ranges.
  const double *ranges() const { return ranges_.empty() ? nullptr : ranges_.data(); }

  /// Synchronous query (ohm/Query.h:93): a soft reset, then onExecute().  @return true on success; false without a
  /// usable map or when the device refuses, and then there are no results.
  bool execute()
  {
    reset(false);
    if (!gpu_map_ || !gpu_map_->gpuOk())
    {
      return false;
    }
    if (!onExecute())
    {
      reset(false);
      return false;
    }
    return true;
  }
  virtual bool executeAsync() { return execute(); }
  bool wait(unsigned /*timeout_ms*/ = ~0u) { return true; }
  /// Drops the results; a hard reset also releases their memory (ohm/Query.h:114) and whatever onReset(true) drops.
  void reset(bool hard_reset = true)
  {
    number_of_results_ = 0;
    intersected_voxels_.clear();
    ranges_.clear();
    if (hard_reset)
    {
      std::vector<Key>().swap(intersected_voxels_);
      std::vector<double>().swap(ranges_);
    }
    onReset(hard_reset);
  }

protected:
  Query(GpuMap *gpu_map, unsigned query_flags)
    : gpu_map_(gpu_map)
    , query_flags_(query_flags)
  {}
  /// Fill the results and set number_of_results_; the map is there and valid.
  virtual bool onExecute() = 0;
  virtual void onReset(bool /*hard_reset*/) {}
  /// Bits queryFlags() always reports.
  virtual unsigned forcedQueryFlags() const { return 0; }

  GpuMap *gpu_map_ = nullptr;
  unsigned query_flags_ = 0;
  size_t number_of_results_ = 0;
  std::vector<Key> intersected_voxels_;
  std::vector<double> ranges_;
};

/// Worst case of the number of voxels on the line from a to b, as the reference sizes its key buffer
/// (ohmgpu/LineKeysQueryGpu.cpp:112-119).
inline uint32_t maxKeysPerLine(const dvec3 &a, const dvec3 &b, double resolution)
{
  const double len = std::sqrt((b.x - a.x) * (b.x - a.x) + (b.y - a.y) * (b.y - a.y) + (b.z - a.z) * (b.z - a.z));
  return uint32_t(std::ceil(len / resolution * std::sqrt(3.0))) + 4u;
}

/// ohm::LineKeysQueryGpu (ohmgpu/LineKeysQueryGpu.h; the interface of ohm/LineKeysQuery.h:47-101): the voxel keys along a
/// set of query lines, walked on the device with the CPU walk's fp64 semantics (ohmhip_map_line_keys).  The query needs
/// the map's geometry only; it is given the GpuMap that holds the device handle.  Results as in the reference: one
/// result per ray, resultIndices() / resultCounts() index intersectedVoxels(); no ranges.  A reset keeps the rays.
class LineKeysQueryGpu : public Query
{
public:
  explicit LineKeysQueryGpu(GpuMap &gpu_map, unsigned query_flags = 0) : Query(&gpu_map, query_flags) {}

  /// Ray start / end point pairs; @p point_count is twice the number of rays.
  void setRays(const dvec3 *rays, size_t point_count) { rays_.assign(rays, rays + (point_count & ~size_t(1))); }
  const dvec3 *rays() const { return rays_.data(); }
  size_t rayPointCount() const { return rays_.size(); }

  const size_t *resultIndices() const { return result_indices_.data(); }
  const size_t *resultCounts() const { return result_counts_.data(); }

protected:
  bool onExecute() override
  {
    const size_t ray_count = rays_.size() / 2;
    if (ray_count == 0)
    {
      return true;
    }
    uint32_t max_keys = 1;
    for (size_t i = 0; i < ray_count; ++i)
    {
      max_keys = std::max(max_keys, maxKeysPerLine(rays_[2 * i], rays_[2 * i + 1], gpu_map_->map().resolution()));
    }
    std::vector<Key> records(ray_count * size_t(max_keys));
    std::vector<uint32_t> counts(ray_count);
    if (ohmhip_map_line_keys(gpu_map_->handle(), &rays_[0].x, ray_count, max_keys, records.data(), counts.data()) !=
        OHMHIP_OK)
    {
      return false;
    }
    result_indices_.resize(ray_count);
    result_counts_.resize(ray_count);
    for (size_t i = 0; i < ray_count; ++i)
    {
      const auto first = records.begin() + i * size_t(max_keys);
      result_indices_[i] = intersected_voxels_.size();
      result_counts_[i] = std::min<size_t>(counts[i], max_keys);
      intersected_voxels_.insert(intersected_voxels_.end(), first, first + result_counts_[i]);
    }
    number_of_results_ = ray_count;
    return true;
  }
  void onReset(bool) override
  {
    result_indices_.clear();
    result_counts_.clear();
  }

private:
  std::vector<dvec3> rays_;
  std::vector<size_t> result_indices_, result_counts_;
};

/// ohm::OccupancyType (ohm/OccupancyType.h:14-24).
enum OccupancyType : int
{
  kNull = -2,
  kUnobserved = -1,
  kFree = 0,
  kOccupied = 1
};

/// ohm::QueryFlag::kQfGpuEvaluate (ohm/QueryFlag.h:42).
constexpr unsigned kQfGpuEvaluate = 1u << 2u;

/// ohm::RaysQueryGpu (ohmgpu/RaysQueryGpu.h; the interface of ohm/RaysQuery.h): for each ray, the range to the first
/// occupied voxel, the unobserved volume crossed, and the state and key of the voxel the ray ends in -- evaluated on the
/// device against the resident map (ohmhip_map_rays_query), bit-identical to the CPU query (ohm/RaysQuery.cpp:102-203).
/// The map's current parameters apply; the map is read, never changed.  A hard reset also drops the rays
/// (ohm/RaysQuery.cpp onReset).
class RaysQueryGpu : public Query
{
public:
  explicit RaysQueryGpu(GpuMap &gpu_map, unsigned query_flags = 0) : Query(&gpu_map, query_flags) {}

  void setVolumeCoefficient(double coefficient) { volume_coefficient_ = coefficient; }
  double volumeCoefficient() const { return volume_coefficient_; }

  /// Origin / end point pairs; @p element_count is twice the number of rays (an odd trailing point is dropped).
  void setRays(const dvec3 *rays, size_t element_count) { rays_.assign(rays, rays + (element_count & ~size_t(1))); }
  void addRays(const dvec3 *rays, size_t element_count)
  {
    rays_.insert(rays_.end(), rays, rays + (element_count & ~size_t(1)));
  }
  void addRay(const dvec3 &origin, const dvec3 &end_point)
  {
    rays_.push_back(origin);
    rays_.push_back(end_point);
  }
  void clearRays() { rays_.clear(); }
  const dvec3 *rays() const { return rays_.data(); }
  size_t numberOfRays() const { return rays_.size() / 2; }

  const double *unobservedVolumes() const { return volumes_.data(); }
  const OccupancyType *terminalOccupancyTypes() const { return types_.data(); }

protected:
  unsigned forcedQueryFlags() const override { return kQfGpuEvaluate; }
  bool onExecute() override
  {
    if (!gpu_map_->syncConfig())
    {
      return false;
    }
    const size_t n = rays_.size() / 2;
    std::vector<int8_t> types(n);
    ranges_.resize(n);
    volumes_.resize(n);
    intersected_voxels_.resize(n);
    if (ohmhip_map_rays_query(gpu_map_->handle(), reinterpret_cast<const double *>(rays_.data()), rays_.size(),
                              volume_coefficient_, ranges_.data(), volumes_.data(), types.data(),
                              intersected_voxels_.data()) != OHMHIP_OK)
    {
      return false;
    }
    types_.resize(n);
    for (size_t i = 0; i < n; ++i)
    {
      types_[i] = OccupancyType(types[i]);
    }
    number_of_results_ = n;
    return true;
  }
  void onReset(bool hard_reset) override
  {
    volumes_.clear();
    types_.clear();
    if (hard_reset)
    {
      rays_.clear();
    }
  }

private:
  double volume_coefficient_ = 1.0;
  std::vector<dvec3> rays_;
  std::vector<double> volumes_;
  std::vector<OccupancyType> types_;
};

/// The other ohm::QueryFlag bits (ohm/QueryFlag.h:35-60).
constexpr unsigned kQfUnknownAsOccupied = 1u << 0u;
constexpr unsigned kQfNearestResult = 1u << 1u;
constexpr unsigned kQfNoCache = 1u << 3u;
constexpr unsigned kQfReportUnscaledResults = 1u << 4u;
constexpr unsigned kQfSpecialised = 1u << 16u;

/// ohm::MappingProcessResult (ohm/MappingProcess.h:18-24).
enum MappingProcessResult : int
{
  kMprUpToDate = 0,
  kMprProgressing = 1
};

/// The parameter block of the clearance calls (ohmhip_map_clearance_*) from a search radius, ohm::QueryFlag bits and the
/// per-axis scaling.
inline ohmhip_clearance_params clearanceParams(float search_radius, unsigned query_flags, const float axis_scaling[3])
{
  ohmhip_clearance_params p{};
  p.search_radius = search_radius;
  for (int a = 0; a < 3; ++a)
  {
    p.axis_scaling[a] = axis_scaling[a];
  }
  p.flags = query_flags;
  return p;
}

/// ohm::ClearanceProcess (ohmgpu/ClearanceProcess.h): the clearance of every voxel of a set of regions -- the distance
/// to the nearest obstructing voxel within the search radius, per calculateNearestNeighbour (ohm/private/
/// VoxelAlgorithms.cpp:22-98), evaluated exactly on the device (ohmhip_map_clearance_regions), not by the reference's
/// approximate flood fill.  calculateForExtents() keeps its results here per region; update() keeps the map's clearance
/// layer current.  Not provided: stamp-based skipping (force = false recomputes), serialisation.
class ClearanceProcess
{
public:
  enum : unsigned
  {
    kQfInstantiateUnknown = kQfSpecialised << 0u
  };
  using RegionKey = std::array<int16_t, 3>;

  ClearanceProcess() = default;
  ClearanceProcess(float search_radius, unsigned query_flags)
    : search_radius_(search_radius)
    , query_flags_(query_flags)
  {}

  float searchRadius() const { return search_radius_; }
  void setSearchRadius(float range) { search_radius_ = range; }
  unsigned queryFlags() const { return query_flags_; }
  void setQueryFlags(unsigned flags) { query_flags_ = flags; }
  const float *axisScaling() const { return axis_scaling_; }
  void setAxisScaling(float x, float y, float z)
  {
    axis_scaling_[0] = x;
    axis_scaling_[1] = y;
    axis_scaling_[2] = z;
  }
  void reset() { results_.clear(); }

  /// ClearanceProcess::ensureClearanceLayer (ohm/DefaultLayer.cpp:174-193): add the clearance layer to the map before
  /// its GpuMap is created (a live device map gains it through GpuMap::addLayer(OHMHIP_LID_CLEARANCE)).
  static void ensureClearanceLayer(OccupancyMap &map) { map.addLayer(OHMHIP_LID_CLEARANCE); }

  /// ClearanceProcess::update (ohmgpu/ClearanceProcess.cpp:418-470): recompute the clearance layer of stale regions in
  /// ascending (z, y, x) key order, max_regions (0: all) per device call, until time_slice seconds have passed or --
  /// time_slice <= 0 -- nothing is stale (ohmhip_map_clearance_update).
  /// @return kMprUpToDate / kMprProgressing, or a negative OHMHIP_ERR_* status.
  int update(GpuMap &gpu_map, double time_slice = 0.0, size_t max_regions = 0)
  {
    if (!gpu_map.gpuOk() || !gpu_map.syncConfig())
    {
      return OHMHIP_ERR_INVALID_ARG;
    }
    const auto start = std::chrono::steady_clock::now();
    const ohmhip_clearance_params p = params();
    for (;;)
    {
      size_t processed = 0, remaining = 0;
      const int status = ohmhip_map_clearance_update(gpu_map.handle(), &p, max_regions, &processed, &remaining);
      if (status != OHMHIP_OK)
      {
        return status;
      }
      if (remaining == 0)
      {
        return kMprUpToDate;
      }
      if (time_slice > 0 &&
          std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count() >= time_slice)
      {
        return kMprProgressing;
      }
    }
  }

  /// ClearanceProcess::calculateForExtents (ohmgpu/ClearanceProcess.cpp:474-510): the regions from regionKey(min) to
  /// regionKey(max) that exist in the map, or all of them with kQfInstantiateUnknown (not created on the device).  On a
  /// map with the clearance layer, the layer of those present is written too: all of them with force, the stale ones
  /// otherwise.
  /// @return false when the device refuses the query.
  bool calculateForExtents(GpuMap &gpu_map, const dvec3 &min_extents, const dvec3 &max_extents, bool force = true)
  {
    if (!gpu_map.gpuOk() || !gpu_map.syncConfig())
    {
      return false;
    }
    const OccupancyMap &m = gpu_map.map();
    const double lo[3] = { min_extents.x, min_extents.y, min_extents.z };
    const double hi[3] = { max_extents.x, max_extents.y, max_extents.z };
    int r0[3], r1[3];
    for (int a = 0; a < 3; ++a)
    {
      const double rdim = m.regionVoxelDimensions()[a] * m.resolution();
      r0[a] = int16_t(int(std::floor((lo[a] - m.origin()[a]) / rdim + 0.5)));  // pointToRegionCoord, ohm/MapCoord.h:85
      r1[a] = int16_t(int(std::floor((hi[a] - m.origin()[a]) / rdim + 0.5)));
    }
    std::vector<RegionKey> present;
    if (!(query_flags_ & kQfInstantiateUnknown))
    {
      if (fetchRegions(gpu_map.handle(), false, present) != OHMHIP_OK)
      {
        return false;
      }
      std::sort(present.begin(), present.end());
    }
    std::vector<int16_t> keys;
    for (int z = r0[2]; z <= r1[2]; ++z)
    {
      for (int y = r0[1]; y <= r1[1]; ++y)
      {
        for (int x = r0[0]; x <= r1[0]; ++x)
        {
          const RegionKey key = { int16_t(x), int16_t(y), int16_t(z) };
          if ((query_flags_ & kQfInstantiateUnknown) || std::binary_search(present.begin(), present.end(), key))
          {
            keys.insert(keys.end(), key.begin(), key.end());
          }
        }
      }
    }
    const size_t count = keys.size() / 3;
    const size_t voxels = m.regionVoxelVolume();
    std::vector<std::vector<float>> blocks(count, std::vector<float>(voxels));
    std::vector<float *> dsts(count);
    for (size_t i = 0; i < count; ++i)
    {
      dsts[i] = blocks[i].data();
    }
    const ohmhip_clearance_params p = params();
    if (ohmhip_map_clearance_regions(gpu_map.handle(), keys.data(), count, &p, dsts.data()) != OHMHIP_OK)
    {
      return false;
    }
    for (size_t i = 0; i < count; ++i)
    {
      results_[RegionKey{ keys[3 * i], keys[3 * i + 1], keys[3 * i + 2] }] = std::move(blocks[i]);
    }
    if (m.hasLayer(OHMHIP_LID_CLEARANCE) &&
        ohmhip_map_clearance_update_regions(gpu_map.handle(), keys.data(), count, &p, force ? 1 : 0, nullptr) !=
          OHMHIP_OK)
    {
      return false;
    }
    return true;
  }

  /// The clearance block of a computed region (MapChunk order), null otherwise.
  const float *regionClearance(const RegionKey &region_key) const
  {
    const auto it = results_.find(region_key);
    return it == results_.end() ? nullptr : it->second.data();
  }
  /// The clearance of one voxel of a computed region.  @return false when its region was not computed.
  bool voxelClearance(const Key &key, const int *region_dim, float *value) const
  {
    const float *block = regionClearance(RegionKey{ key.region[0], key.region[1], key.region[2] });
    if (!block)
    {
      return false;
    }
    *value = block[key.local[0] + key.local[1] * region_dim[0] + key.local[2] * region_dim[0] * region_dim[1]];
    return true;
  }

private:
  ohmhip_clearance_params params() const { return clearanceParams(search_radius_, query_flags_, axis_scaling_); }

  float search_radius_ = 0.0f;
  unsigned query_flags_ = 0;
  float axis_scaling_[3] = { 1.0f, 1.0f, 1.0f };
  std::map<RegionKey, std::vector<float>> results_;
};

/// ohm::Mapper (ohm/Mapper.h): runs its processes (ClearanceProcess) over one GpuMap between integrateRays batches.
class Mapper
{
public:
  explicit Mapper(GpuMap *gpu_map = nullptr)
    : map_(gpu_map)
  {}
  void setMap(GpuMap *gpu_map) { map_ = gpu_map; }
  GpuMap *map() const { return map_; }
  /// Takes ownership, as the reference's Mapper does.
  void addProcess(ClearanceProcess *process) { processes_.emplace_back(process); }
  size_t processCount() const { return processes_.size(); }

  /// Mapper::update: each process in turn shares time_slice seconds (<= 0: each runs until it is up to date).
  /// @return kMprUpToDate when every process is, kMprProgressing, or a negative OHMHIP_ERR_* status.
  int update(double time_slice = 0.0, size_t max_regions = 0)
  {
    if (!map_)
    {
      return kMprUpToDate;
    }
    const auto start = std::chrono::steady_clock::now();
    int result = kMprUpToDate;
    for (auto &process : processes_)
    {
      double left = 0.0;
      if (time_slice > 0)
      {
        left = time_slice - std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        if (left <= 0)
        {
          return kMprProgressing;
        }
      }
      const int status = process->update(*map_, left, max_regions);
      if (status < 0)
      {
        return status;
      }
      result = (status == kMprUpToDate) ? result : int(kMprProgressing);
    }
    return result;
  }

private:
  GpuMap *map_;
  std::vector<std::unique_ptr<ClearanceProcess>> processes_;
};

/// ohm::LineQueryGpu (ohmgpu/LineQueryGpu.{h,cpp}; interface of ohm/LineQuery.h): the voxels a segment passes through
/// (calculateSegmentKeys, device walk: ohmhip_map_line_keys) and the clearance of each (ohmhip_map_clearance_keys),
/// with LineQueryGpu::onExecute's post-processing: a voxel in no region of the map, or unobstructed within the radius
/// (-1), reports defaultRange(); only kQfUnknownAsOccupied is passed to the clearance.  kQfNearestResult keeps the
/// first voxel, then any later one with range >= 0 && (range < closest || closest < 0) -- the GPU query's rule; the CPU
/// LineQuery compares range * range < closest (ohm/LineQuery.cpp:75-84) and is not followed.  ranges() are floats, as
/// the reference reports them.
class LineQueryGpu : public Query
{
public:
  LineQueryGpu(GpuMap &gpu_map, const dvec3 &start_point, const dvec3 &end_point, float search_radius,
               unsigned query_flags = 0)
    : Query(&gpu_map, query_flags)
    , start_(start_point)
    , end_(end_point)
    , search_radius_(search_radius)
  {}

  void setStartPoint(const dvec3 &p) { start_ = p; }
  void setEndPoint(const dvec3 &p) { end_ = p; }
  float searchRadius() const { return search_radius_; }
  void setSearchRadius(float r) { search_radius_ = r; }
  float defaultRange() const { return default_range_; }
  void setDefaultRange(float range) { default_range_ = range; }
  void setAxisScaling(float x, float y, float z)
  {
    axis_scaling_[0] = x;
    axis_scaling_[1] = y;
    axis_scaling_[2] = z;
  }

  const float *ranges() const { return float_ranges_.data(); }

protected:
  unsigned forcedQueryFlags() const override { return kQfGpuEvaluate; }
  bool onExecute() override
  {
    if (!gpu_map_->syncConfig())
    {
      return false;
    }
    const double line[6] = { start_.x, start_.y, start_.z, end_.x, end_.y, end_.z };
    const uint32_t max_keys = maxKeysPerLine(start_, end_, gpu_map_->map().resolution());
    std::vector<Key> &keys = intersected_voxels_;
    keys.resize(max_keys);
    uint32_t count = 0;
    if (ohmhip_map_line_keys(gpu_map_->handle(), line, 1, max_keys, keys.data(), &count) != OHMHIP_OK)
    {
      return false;
    }
    const size_t n = std::min<size_t>(count, max_keys);
    keys.resize(n);
    float_ranges_.resize(n);
    const ohmhip_clearance_params p = clearanceParams(search_radius_, query_flags_ & kQfUnknownAsOccupied, axis_scaling_);
    if (n && ohmhip_map_clearance_keys(gpu_map_->handle(), keys.data(), n, &p, float_ranges_.data()) != OHMHIP_OK)
    {
      return false;
    }
    std::vector<std::array<int16_t, 3>> present;
    if (fetchRegions(gpu_map_->handle(), false, present) != OHMHIP_OK)
    {
      return false;
    }
    std::sort(present.begin(), present.end());
    size_t closest_index = 0;
    float closest = -1.0f;
    for (size_t i = 0; i < n; ++i)
    {
      const std::array<int16_t, 3> rk = { keys[i].region[0], keys[i].region[1], keys[i].region[2] };
      float &range = float_ranges_[i];
      if (!std::binary_search(present.begin(), present.end(), rk) || range < 0)
      {
        range = default_range_;
      }
      if (i == 0 || (range >= 0 && (range < closest || closest < 0)))
      {
        closest_index = i;
        closest = range;
      }
    }
    if ((query_flags_ & kQfNearestResult) && n)
    {
      keys[0] = keys[closest_index];
      float_ranges_[0] = float_ranges_[closest_index];
      keys.resize(1);
      float_ranges_.resize(1);
    }
    number_of_results_ = keys.size();
    return true;
  }
  void onReset(bool) override { float_ranges_.clear(); }

private:
  dvec3 start_, end_;
  float search_radius_ = 0.0f;
  float default_range_ = -1.0f;
  float axis_scaling_[3] = { 1.0f, 1.0f, 1.0f };
  std::vector<float> float_ranges_;
};

/// Not in the reference (ohm is single device): the RCCL communicator the library owns (include/ohmhip.h, ohmhip_comm_*).
/// Rank 0 makes the id (uniqueId) and the host program carries its 128 bytes to the other ranks over whatever it has
/// (MPI, a socket, a file); every rank then constructs its communicator -- a collective call.
class RayCommunicator
{
public:
  static std::array<unsigned char, OHMHIP_COMM_ID_BYTES> uniqueId()
  {
    std::array<unsigned char, OHMHIP_COMM_ID_BYTES> id{};
    OHMHIP_GPUAPICHECK(ohmhip_comm_unique_id(id.data()));
    return id;
  }
  RayCommunicator(const std::array<unsigned char, OHMHIP_COMM_ID_BYTES> &id, int world_size, int rank)
    : world_(world_size)
    , rank_(rank)
  {
    OHMHIP_GPUAPICHECK(ohmhip_comm_init_rank(&handle_, id.data(), world_size, rank));
  }
  RayCommunicator(const RayCommunicator &) = delete;
  RayCommunicator &operator=(const RayCommunicator &) = delete;
  ~RayCommunicator()
  {
    if (handle_)
    {
      ohmhip_comm_destroy(handle_);
    }
  }
  ohmhip_comm_t handle() const { return handle_; }
  int worldSize() const { return world_; }
  int rank() const { return rank_; }

private:
  ohmhip_comm_t handle_ = nullptr;
  int world_ = 1;
  int rank_ = 0;
};

/// Not in the reference: exact multi-GPU integration into a region-partitioned map (include/ohmhip.h "Partitioned map";
/// the C++ face of ohm_amd.distributed.PartitionedIntegrator).  Every rank constructs one around its EMPTY GpuMap with the
/// same territory table and calls integrateRays() with its own rays, all ranks the same number of times: the rays are
/// routed on the device to the owners of the regions they cross, exchanged over RCCL (48 B per routed ray) and what
/// arrives is integrated in (source rank, ray) order.  The union of the ranks' maps is bit-identical to one map
/// integrating rank 0's batch, then rank 1's, ...  The batch a call launches stays in flight; three receive buffers are
/// used in turn because the map keeps at most two batches in flight (ohmhip_map_integrate_rays_device).
class PartitionedIntegrator
{
public:
  PartitionedIntegrator(GpuMap &gpu_map, const GpuMap::RegionPartition &partition, RayCommunicator &comm)
    : map_(gpu_map)
    , comm_(comm)
    , exchange_queue_(gputil::Queue::create())
  {
    map_.setRegionPartition(partition);
  }

  /// Collective.  @p device_rays: this rank's rays (origin, sample pairs; element_count points), complete when the call
  /// is made and free again when it returns.  Returns the points this rank integrated (its own and received rays that
  /// pass the ray filter), 0 on failure (lastStatus()).
  size_t integrateRays(const gputil::Buffer &device_rays, size_t element_count, unsigned ray_update_flags = kRfDefault)
  {
    const int world = comm_.worldSize();
    send_counts_.assign(size_t(world), 0u);
    recv_counts_.assign(size_t(world), 0u);
    if (element_count >= 2 && device_rays.isValid())
    {
      map_.routeRays(device_rays, element_count, ray_update_flags, routed_, send_counts_);
    }
    last_status_ = ohmhip_comm_exchange_counts(comm_.handle(), send_counts_.data(), recv_counts_.data(),
                                               exchange_queue_.handle());
    if (last_status_ != OHMHIP_OK)
    {
      return 0;
    }
    size_t n_in = 0;
    for (uint32_t c : recv_counts_)
    {
      n_in += c;
    }
    // The turn advances per LAUNCH, not per call: a step that launches nothing -- no rays received, or rays
    // the map only collects -- leaves the two batches launched last in flight, possibly both still reading their
    // buffers.  A buffer is free once two more batches were launched after the one that reads it.
    const uint64_t launched = map_.batchesLaunched();
    size_t turn = 0;
    while (turn < 2 && recv_batch_[turn] != 0 && recv_batch_[turn] + 2 > launched)
    {
      ++turn;  // (at most two buffers are held by batches in flight: the third is always free)
    }
    recv_batch_[turn] = 0;
    gputil::Buffer &in = recv_[turn];
    const size_t in_bytes = std::max<size_t>(n_in, 1) * 6 * sizeof(double);
    if (!in.isValid())
    {
      in.create(in_bytes + in_bytes / 4);
    }
    else if (in.size() < in_bytes)
    {
      in.resize(in_bytes + in_bytes / 4);  // (the batch that read it has ended: see above)
    }
    void *d_routed = nullptr, *d_in = nullptr;
    if (routed_.isValid())
    {
      OHMHIP_GPUAPICHECK(ohmhip_buffer_ptr(routed_.handle(), &d_routed));
    }
    OHMHIP_GPUAPICHECK(ohmhip_buffer_ptr(in.handle(), &d_in));
    last_status_ = ohmhip_comm_exchange_rays(comm_.handle(), static_cast<const double *>(d_routed), send_counts_.data(),
                                             static_cast<double *>(d_in), recv_counts_.data(), exchange_queue_.handle());
    if (last_status_ != OHMHIP_OK)
    {
      return 0;
    }
    exchange_queue_.finish();  // the exchange only: the batches in flight stay in flight
    rays_received_ = n_in;
    if (n_in == 0)
    {
      return 0;
    }
    const size_t done = map_.integrateRays(in, 2 * n_in, ray_update_flags);
    last_status_ = map_.lastStatus();
    const uint64_t after = map_.batchesLaunched();
    recv_batch_[turn] = after > launched ? after : 0;  // (no launch: the rays were copied, the buffer is free)
    return done;
  }

  size_t raysReceived() const { return rays_received_; }
  const std::vector<uint32_t> &sendCounts() const { return send_counts_; }
  const std::vector<uint32_t> &receiveCounts() const { return recv_counts_; }
  int lastStatus() const { return last_status_; }

private:
  GpuMap &map_;
  RayCommunicator &comm_;
  gputil::Queue exchange_queue_;
  gputil::Buffer routed_, recv_[3];
  std::vector<uint32_t> send_counts_, recv_counts_;
  uint64_t recv_batch_[3] = { 0, 0, 0 };  ///< launch count of the batch reading each receive buffer (0: none)
  size_t rays_received_ = 0;
  int last_status_ = OHMHIP_OK;
};

/// ohm::UpAxis (ohmheightmap/UpAxis.h)
enum class UpAxis : int
{
  kNegZ = -3,
  kNegY = -2,
  kNegX = -1,
  kX = 0,
  kY = 1,
  kZ = 2
};

/// ohm::HeightmapVoxelType (ohmheightmap/HeightmapVoxelType.h)
enum class HeightmapVoxelType : uint8_t
{
  kUnknown = 0,
  kVacant,
  kSurface,
  kVirtualSurface
};

/// ohm::HeightmapMode (ohmheightmap/HeightmapMode.h); kPlanar and kSimpleFill are built on the device.
enum class HeightmapMode : int
{
  kPlanar = 0,
  kSimpleFill,
  kLayeredFillUnordered,
  kLayeredFill
};

/// ohm::HeightmapVoxel (ohmheightmap/HeightmapVoxel.h:68-97)
struct alignas(8) HeightmapVoxel
{
  float height;
  float clearance;
  float normal_x, normal_y, normal_z;
  uint8_t layer;
  uint8_t flags;  ///< kHvfObservedAbove = 1
  uint16_t contributing_samples;
};
static_assert(sizeof(HeightmapVoxel) == 24, "HeightmapVoxel is 24 bytes");

/// ohm::VoxelMean (ohm/VoxelMean.h)
struct VoxelMean
{
  uint32_t coord;
  uint32_t count;
};

/// ohm::Heightmap (ohmheightmap/Heightmap.h) in planar and simple-fill mode, built on the device from the resident map
/// of a GpuMap (ohmhip_map_heightmap, ohmhip_map_heightmap_fill: include/ohmhip.h, "HEIGHTMAP"), equal to the CPU
/// algorithm for every cell and field; the layered fill modes are refused here (OHMHIP_ERR_UNSUPPORTED): they are
/// LayeredHeightmap's.  Only the results cross to the host: the heightmap's layers as dense arrays of heightmapCellsA()
/// x heightmapCellsB() cells, a fastest, over the cell range the source's extents cover (extents()).
class Heightmap
{
public:
  static constexpr unsigned kDefaultRegionSize = 128;
  virtual ~Heightmap() = default;

  Heightmap(double grid_resolution, double min_clearance, UpAxis up_axis = UpAxis::kZ, unsigned region_size = 0)
    : grid_resolution_(grid_resolution)
    , min_clearance_(min_clearance)
    , up_axis_(up_axis)
    , region_size_(region_size ? region_size : kDefaultRegionSize)
  {}

  void setOccupancyMap(GpuMap *gpu_map) { gpu_map_ = gpu_map; }
  GpuMap *occupancyMap() const { return gpu_map_; }

  void setCeiling(double ceiling) { ceiling_ = ceiling; }
  double ceiling() const { return ceiling_; }
  void setFloor(double floor) { floor_ = floor; }
  double floor() const { return floor_; }
  void setMinClearance(double clearance) { min_clearance_ = clearance; }
  double minClearance() const { return min_clearance_; }
  void setIgnoreVoxelMean(bool ignore) { ignore_voxel_mean_ = ignore; }
  bool ignoreVoxelMean() const { return ignore_voxel_mean_; }
  void setGenerateVirtualSurface(bool enable) { generate_virtual_surface_ = enable; }
  bool generateVirtualSurface() const { return generate_virtual_surface_; }
  void setPromoteVirtualBelow(bool enable) { promote_virtual_below_ = enable; }
  bool promoteVirtualBelow() const { return promote_virtual_below_; }
  void setMode(HeightmapMode mode) { mode_ = mode; }
  HeightmapMode mode() const { return mode_; }
  /// Surface normals of occupied cells from the source's covariance layer (OHMHIP_HM_SURFACE_NORMALS): what the
  /// reference always computes on an NDT map (ohmheightmap/Heightmap.cpp:815-826).  Off -- the default -- normal_x / y /
  /// z stay 0; on a map without the covariance layer the setting changes nothing.
  void setSurfaceNormals(bool enable) { surface_normals_ = enable; }
  bool surfaceNormals() const { return surface_normals_; }
  /// The origin of the heightmap's own OccupancyMap (heightmap().setOrigin() in the reference).
  void setHeightmapOrigin(const dvec3 &origin) { origin_ = origin; }
  const dvec3 &heightmapOrigin() const { return origin_; }
  double gridResolution() const { return grid_resolution_; }
  UpAxis upAxis() const { return up_axis_; }
  int upAxisIndex() const { return int(up_axis_) >= 0 ? int(up_axis_) : -int(up_axis_) - 1; }
  /// heightmapAxisIndices (ohmheightmap/HeightmapUtil.cpp:86-116)
  int surfaceAxisIndexA() const { return upAxisIndex() == 0 ? 1 : 0; }
  int surfaceAxisIndexB() const { return upAxisIndex() == 2 ? 1 : 2; }
  dvec3 upAxisNormal() const
  {
    double n[3] = { 0.0, 0.0, 0.0 };
    n[upAxisIndex()] = int(up_axis_) >= 0 ? 1.0 : -1.0;
    return dvec3{ n[0], n[1], n[2] };
  }

  /// Heightmap::buildHeightmap (ohmheightmap/Heightmap.cpp:335-412).  @return true when any cell was populated.
  virtual bool buildHeightmap(const dvec3 &reference_pos,
                              const Aabb &cull_to = Aabb(dvec3{ 0, 0, 0 }, dvec3{ 0, 0, 0 }))
  {
    clearResults();
    if (!gpu_map_ || !gpu_map_->gpuOk() || !gpu_map_->syncConfig())
    {
      return false;
    }
    const ohmhip_heightmap_params p = params(reference_pos, cull_to);
    const bool fill = mode_ == HeightmapMode::kSimpleFill;  // the layered modes: refused by the planar call
    last_status_ = fill ? ohmhip_map_heightmap_fill_extents(gpu_map_->handle(), &p, &extents_) :
                          ohmhip_map_heightmap_extents(gpu_map_->handle(), &p, &extents_);
    if (last_status_ != OHMHIP_OK || !extents_.populated)
    {
      return false;
    }
    const size_t n = size_t(extents_.ma) * size_t(extents_.mb);
    occupancy_.resize(n);
    voxels_.resize(n);
    if (extents_.use_mean)
    {
      mean_.resize(n);
    }
    if (fill)
    {
      return buildFill(p, n);
    }
    uint64_t populated = 0, cells = 0;
    last_status_ = ohmhip_map_heightmap(gpu_map_->handle(), &p, occupancy_.data(), voxels_.data(),
                                        extents_.use_mean ? mean_.data() : nullptr, nullptr, &populated, &cells);
    if (last_status_ != OHMHIP_OK)
    {
      occupancy_.clear();
      voxels_.clear();
      mean_.clear();
      return false;
    }
    populated_ = populated;
    cells_ = cells;
    return populated != 0;
  }

  /// The settings as the C ABI takes them.
  ohmhip_heightmap_params params(const dvec3 &reference_pos, const Aabb &cull_to) const
  {
    ohmhip_heightmap_params p{};
    const double ref[3] = { reference_pos.x, reference_pos.y, reference_pos.z };
    const double lo[3] = { cull_to.minExtents().x, cull_to.minExtents().y, cull_to.minExtents().z };
    const double hi[3] = { cull_to.maxExtents().x, cull_to.maxExtents().y, cull_to.maxExtents().z };
    const double origin[3] = { origin_.x, origin_.y, origin_.z };
    for (int i = 0; i < 3; ++i)
    {
      p.reference_pos[i] = ref[i];
      p.cull_min[i] = lo[i];
      p.cull_max[i] = hi[i];
      p.origin[i] = origin[i];
    }
    p.grid_resolution = grid_resolution_;
    p.region_size = uint8_t(region_size_ == kDefaultRegionSize ? 0 : region_size_);
    p.up_axis = int8_t(up_axis_);
    p.mode = uint8_t(mode_);
    p.floor = floor_;
    p.ceiling = ceiling_;
    p.min_clearance = min_clearance_;
    p.flags = (generate_virtual_surface_ ? OHMHIP_HM_GENERATE_VIRTUAL_SURFACE : 0u) |
              (promote_virtual_below_ ? OHMHIP_HM_PROMOTE_VIRTUAL_BELOW : 0u) |
              (ignore_voxel_mean_ ? OHMHIP_HM_IGNORE_VOXEL_MEAN : 0u) |
              (surface_normals_ ? OHMHIP_HM_SURFACE_NORMALS : 0u);
    return p;
  }

  int lastStatus() const { return last_status_; }
  const ohmhip_heightmap_extents &extents() const { return extents_; }
  size_t heightmapCellsA() const { return extents_.ma; }
  size_t heightmapCellsB() const { return extents_.mb; }
  uint64_t populatedCount() const { return populated_; }
  uint64_t cellCount() const { return cells_; }
  /// Dense [cellsB][cellsA] layers: occupancy (+1 surface, -1 virtual surface, +inf nothing), HeightmapVoxel, VoxelMean
  /// (empty when the heightmap has no mean layer).
  const std::vector<float> &occupancy() const { return occupancy_; }
  const std::vector<HeightmapVoxel> &heightmapVoxels() const { return voxels_; }
  const std::vector<VoxelMean> &voxelMeans() const { return mean_; }
  /// HeightmapMode::kSimpleFill: per cell the sequence number of the visit that wrote it (0xffffffff: none), the
  /// walk's counts and, after setKeepVisitLog(true), ia, ib, h of every visit in the reference's FIFO order.
  const std::vector<uint32_t> &sourceVisits() const { return source_visit_; }
  const ohmhip_heightmap_fill_stats &fillStats() const { return fill_stats_; }
  void setKeepVisitLog(bool keep) { keep_visit_log_ = keep; }
  bool keepVisitLog() const { return keep_visit_log_; }
  const std::vector<uint32_t> &visitLog() const { return visit_log_; }

  /// voxelCentreGlobal of the heightmap's own OccupancyMap (ohm/OccupancyMap.h:757-778).
  dvec3 voxelCentreGlobal(const Key &key) const
  {
    const double origin[3] = { origin_.x, origin_.y, origin_.z };
    double c[3];
    for (int i = 0; i < 3; ++i)
    {
      const double region_dim = (i == upAxisIndex() ? 1.0 : double(region_size_)) * grid_resolution_;
      double v = double(float(key.region[i]));
      v *= region_dim;
      v -= 0.5 * region_dim;
      v += origin[i];
      v += double(key.local[i]) * grid_resolution_;
      v += 0.5 * grid_resolution_;
      c[i] = v;
    }
    return dvec3{ c[0], c[1], c[2] };
  }

  /// Heightmap::getHeightmapVoxelInfo (ohmheightmap/Heightmap.cpp:415-461) for a key of the heightmap.
  virtual HeightmapVoxelType getHeightmapVoxelInfo(const Key &key, dvec3 *pos,
                                                   HeightmapVoxel *voxel_info = nullptr) const
  {
    return voxelInfoAt(key, 0, pos, voxel_info);
  }

protected:
  /// getHeightmapVoxelInfo for the voxel `slot` steps up the raw up axis from the key's cell: plane `slot` of the
  /// arrays (0 in every mode but the layered ones).
  HeightmapVoxelType voxelInfoAt(const Key &key, size_t slot, dvec3 *pos, HeightmapVoxel *voxel_info) const
  {
    if (!extents_.populated || occupancy_.empty())
    {
      return HeightmapVoxelType::kUnknown;
    }
    const int a = surfaceAxisIndexA(), b = surfaceAxisIndexB();
    const long ca = (long(key.region[a]) - extents_.first_region[0]) * long(region_size_) + key.local[a] - extents_.first_local[0];
    const long cb = (long(key.region[b]) - extents_.first_region[1]) * long(region_size_) + key.local[b] - extents_.first_local[1];
    if (ca < 0 || cb < 0 || ca >= long(extents_.ma) || cb >= long(extents_.mb))
    {
      return HeightmapVoxelType::kUnknown;
    }
    const size_t plane = size_t(extents_.ma) * size_t(extents_.mb);
    if ((slot + 1) * plane > occupancy_.size())
    {
      return HeightmapVoxelType::kUnknown;
    }
    Key flat = key;
    flat.region[upAxisIndex()] = int16_t(slot);
    flat.local[upAxisIndex()] = 0;
    const dvec3 centre = voxelCentreGlobal(flat);
    const size_t cell = slot * plane + size_t(cb) * extents_.ma + size_t(ca);
    const float occupancy = occupancy_[cell];
    if (pos)
    {
      *pos = centre;
    }
    if (occupancy == std::numeric_limits<float>::infinity())
    {
      return HeightmapVoxelType::kUnknown;
    }
    const HeightmapVoxel &info = voxels_[cell];
    if (pos)
    {
      const dvec3 up = upAxisNormal();
      *pos = dvec3{ centre.x + up.x * double(info.height), centre.y + up.y * double(info.height),
                    centre.z + up.z * double(info.height) };
    }
    if (voxel_info)
    {
      *voxel_info = info;
    }
    if (occupancy == 0)
    {
      return HeightmapVoxelType::kVacant;
    }
    return occupancy > 0 ? HeightmapVoxelType::kSurface : HeightmapVoxelType::kVirtualSurface;
  }

  void clearResults()
  {
    occupancy_.clear();
    voxels_.clear();
    mean_.clear();
    source_visit_.clear();
    visit_log_.clear();
    fill_stats_ = ohmhip_heightmap_fill_stats{};
    populated_ = cells_ = 0;
    extents_ = ohmhip_heightmap_extents{};
  }

  /// ohmhip_map_heightmap_fill into the arrays sized by buildHeightmap.  The number of visits is known after the walk:
  /// a log too small for it is fetched by a second build.
  bool buildFill(const ohmhip_heightmap_params &p, size_t n)
  {
    source_visit_.resize(n);
    uint64_t capacity = keep_visit_log_ ? 4ull * extents_.na * extents_.nb : 0;
    for (;;)
    {
      visit_log_.resize(size_t(3 * capacity));
      last_status_ = ohmhip_map_heightmap_fill(gpu_map_->handle(), &p, occupancy_.data(), voxels_.data(),
                                               extents_.use_mean ? mean_.data() : nullptr, source_visit_.data(),
                                               capacity ? visit_log_.data() : nullptr, capacity, &fill_stats_);
      if (last_status_ != OHMHIP_OK)
      {
        occupancy_.clear();
        voxels_.clear();
        mean_.clear();
        source_visit_.clear();
        visit_log_.clear();
        return false;
      }
      if (!capacity || fill_stats_.visits <= capacity)
      {
        break;
      }
      capacity = fill_stats_.visits;
    }
    visit_log_.resize(capacity ? size_t(3 * fill_stats_.visits) : 0);
    populated_ = fill_stats_.populated;
    cells_ = fill_stats_.cells;
    return populated_ != 0;
  }

  GpuMap *gpu_map_ = nullptr;
  double grid_resolution_;
  double min_clearance_;
  UpAxis up_axis_;
  unsigned region_size_;
  double ceiling_ = 0, floor_ = 0;
  bool ignore_voxel_mean_ = false, generate_virtual_surface_ = false, promote_virtual_below_ = false;
  bool surface_normals_ = false;
  HeightmapMode mode_ = HeightmapMode::kPlanar;
  dvec3 origin_{ 0, 0, 0 };
  ohmhip_heightmap_extents extents_{};
  std::vector<float> occupancy_;
  std::vector<HeightmapVoxel> voxels_;
  std::vector<VoxelMean> mean_;
  std::vector<uint32_t> source_visit_, visit_log_;
  ohmhip_heightmap_fill_stats fill_stats_{};
  bool keep_visit_log_ = false;
  uint64_t populated_ = 0, cells_ = 0;
  int last_status_ = OHMHIP_OK;
};

/// ohm::Heightmap in HeightmapMode::kLayeredFill (the default here) and kLayeredFillUnordered, built on the device
/// (ohmhip_map_heightmap_layered: include/ohmhip.h, "HEIGHTMAP, LAYERED", rules L1-L7).  The arrays of the parent gain a
/// leading slot axis: layerSlots() planes of heightmapCellsB() x heightmapCellsA() cells, slot k of a column the
/// heightmap voxel at the cell's key moved k steps along the raw up axis; empty slots hold +inf / zeros / 0xffffffff.
/// kPlanar and kSimpleFill are the parent's builds.
class LayeredHeightmap : public Heightmap
{
public:
  static constexpr uint32_t kInitialLayerCapacity = 4;

  LayeredHeightmap(double grid_resolution, double min_clearance, UpAxis up_axis = UpAxis::kZ, unsigned region_size = 0)
    : Heightmap(grid_resolution, min_clearance, up_axis, region_size)
  {
    setMode(HeightmapMode::kLayeredFill);
  }

  /// Heightmap::setVirtualSurfaceFilterThreshold: 0 is off; applied in kLayeredFill only.
  void setVirtualSurfaceFilterThreshold(unsigned threshold) { filter_threshold_ = threshold; }
  unsigned virtualSurfaceFilterThreshold() const { return filter_threshold_; }

  bool buildHeightmap(const dvec3 &reference_pos,
                      const Aabb &cull_to = Aabb(dvec3{ 0, 0, 0 }, dvec3{ 0, 0, 0 })) override
  {
    if (mode() != HeightmapMode::kLayeredFill && mode() != HeightmapMode::kLayeredFillUnordered)
    {
      layer_count_.clear();
      layered_stats_ = ohmhip_heightmap_layered_stats{};
      return Heightmap::buildHeightmap(reference_pos, cull_to);
    }
    clearResults();
    layer_count_.clear();
    layered_stats_ = ohmhip_heightmap_layered_stats{};
    if (!gpu_map_ || !gpu_map_->gpuOk() || !gpu_map_->syncConfig())
    {
      return false;
    }
    ohmhip_heightmap_layered_params p{};
    p.base = params(reference_pos, cull_to);
    p.virtual_surface_filter_threshold = filter_threshold_;
    last_status_ = ohmhip_map_heightmap_layered_extents(gpu_map_->handle(), &p, &extents_);
    if (last_status_ != OHMHIP_OK || !extents_.populated)
    {
      return false;
    }
    const size_t plane = size_t(extents_.ma) * size_t(extents_.mb);
    layer_count_.resize(plane);
    // the slots and the visits are known after the walk: what was too small is fetched by a second build
    uint32_t slots = kInitialLayerCapacity;
    uint64_t capacity = keep_visit_log_ ? 4ull * extents_.na * extents_.nb : 0;
    for (;;)
    {
      occupancy_.resize(slots * plane);
      voxels_.resize(slots * plane);
      mean_.resize(extents_.use_mean ? slots * plane : 0);
      source_visit_.resize(slots * plane);
      visit_log_.resize(size_t(3 * capacity));
      last_status_ = ohmhip_map_heightmap_layered(gpu_map_->handle(), &p, slots, occupancy_.data(), voxels_.data(),
                                                  extents_.use_mean ? mean_.data() : nullptr, source_visit_.data(),
                                                  layer_count_.data(), capacity ? visit_log_.data() : nullptr,
                                                  capacity, &layered_stats_);
      if (last_status_ != OHMHIP_OK)
      {
        clearResults();
        layer_count_.clear();
        return false;
      }
      if (layered_stats_.layers <= slots && (!capacity || layered_stats_.visits <= capacity))
      {
        break;
      }
      slots = std::max(slots, layered_stats_.layers);
      capacity = capacity ? std::max(capacity, layered_stats_.visits) : 0;
    }
    slots_ = std::max<uint32_t>(1u, layered_stats_.layers);
    occupancy_.resize(slots_ * plane);
    voxels_.resize(slots_ * plane);
    mean_.resize(extents_.use_mean ? slots_ * plane : 0);
    source_visit_.resize(slots_ * plane);
    visit_log_.resize(capacity ? size_t(3 * layered_stats_.visits) : 0);
    populated_ = layered_stats_.populated;
    cells_ = layered_stats_.cells;
    return populated_ != 0;
  }

  /// Planes of the result arrays after a layered build: at least 1, else what the tallest column needed.
  uint32_t layerSlots() const { return slots_; }
  /// Slots in use per cell.
  const std::vector<uint8_t> &layerCounts() const { return layer_count_; }
  const ohmhip_heightmap_layered_stats &layeredStats() const { return layered_stats_; }

  /// The key's up-axis coordinate is the slot.
  HeightmapVoxelType getHeightmapVoxelInfo(const Key &key, dvec3 *pos,
                                           HeightmapVoxel *voxel_info = nullptr) const override
  {
    const long slot = long(key.region[upAxisIndex()]) + long(key.local[upAxisIndex()]);
    const bool layered = mode() == HeightmapMode::kLayeredFill || mode() == HeightmapMode::kLayeredFillUnordered;
    if (layered && slot < 0)
    {
      return HeightmapVoxelType::kUnknown;
    }
    return voxelInfoAt(key, layered ? size_t(slot) : 0, pos, voxel_info);
  }

private:
  unsigned filter_threshold_ = 0;
  uint32_t slots_ = 0;
  std::vector<uint8_t> layer_count_;
  ohmhip_heightmap_layered_stats layered_stats_{};
};

/// What a point cloud is made of (include/ohmhip.h, "POINT CLOUDS").
enum class CloudMode : uint8_t
{
  kOccupancy = OHMHIP_CLOUD_OCCUPANCY,  ///< ohmtools::saveCloud
  kDensity = OHMHIP_CLOUD_DENSITY,      ///< ohmtools::saveDensityCloud, by the rule it documents
  kTsdf = OHMHIP_CLOUD_TSDF,            ///< ohmtools::saveTsdfCloud
  kClearance = OHMHIP_CLOUD_CLEARANCE   ///< ohmtools::saveClearanceCloud
};

/// The options of the reference's exporters (SaveCloudOptions, SaveDensityCloudOptions and the arguments of
/// saveTsdfCloud / saveClearanceCloud) under their names.
struct CloudOptions
{
  CloudMode mode = CloudMode::kOccupancy;
  bool export_free = false;
  bool ignore_voxel_mean = false;
  float density_threshold = 0.0f;
  float surface_distance = std::numeric_limits<float>::infinity();
  float colour_range = 0.0f;
  int export_type = 0;       ///< ohm::OccupancyType: -1 unobserved and up, 0 free and up, 1 occupied
  bool use_extents = false;  ///< only regions from regionKey(min_extents) to regionKey(max_extents)
  dvec3 min_extents{ 0, 0, 0 }, max_extents{ 0, 0, 0 };
};

/// The points of a cloud in the library's fixed order -- regions ascending by (z, y, x), voxels by MapChunk index --
/// and the number of all matching voxels.
struct VoxelCloud
{
  std::vector<dvec3> positions;
  std::vector<CloudKey> keys;
  std::vector<float> values;
  uint64_t count = 0;
  int status = OHMHIP_OK;
};

/// The cloud of `gpu_map`'s device map, compacted on the device: a count call, then arrays of exactly that size.
inline VoxelCloud extractCloud(GpuMap &gpu_map, const CloudOptions &options = CloudOptions())
{
  VoxelCloud cloud;
  if (!gpu_map.gpuOk() || !gpu_map.syncConfig())
  {
    cloud.status = OHMHIP_ERR_INVALID_ARG;
    return cloud;
  }
  ohmhip_cloud_params p{};
  p.mode = uint8_t(options.mode);
  p.flags = (options.export_free ? OHMHIP_CLOUD_EXPORT_FREE : 0u) |
            (options.ignore_voxel_mean ? OHMHIP_CLOUD_IGNORE_VOXEL_MEAN : 0u) |
            (options.use_extents ? OHMHIP_CLOUD_USE_EXTENTS : 0u);
  p.density_threshold = options.density_threshold;
  p.surface_distance = options.surface_distance;
  p.colour_range = options.colour_range;
  p.export_type = int32_t(options.export_type);
  const double lo[3] = { options.min_extents.x, options.min_extents.y, options.min_extents.z };
  const double hi[3] = { options.max_extents.x, options.max_extents.y, options.max_extents.z };
  for (int i = 0; i < 3; ++i)
  {
    p.min_extents[i] = lo[i];
    p.max_extents[i] = hi[i];
  }
  cloud.status = ohmhip_map_cloud_count(gpu_map.handle(), &p, &cloud.count);
  if (cloud.status != OHMHIP_OK || cloud.count == 0)
  {
    return cloud;
  }
  static_assert(sizeof(dvec3) == 3 * sizeof(double), "positions are written as 3 doubles a point");
  const uint64_t capacity = cloud.count;
  cloud.positions.resize(size_t(capacity));
  cloud.keys.resize(size_t(capacity));
  cloud.values.resize(size_t(capacity));
  cloud.status = ohmhip_map_cloud(gpu_map.handle(), &p, capacity, &cloud.positions[0].x, cloud.keys.data(),
                                  cloud.values.data(), &cloud.count);
  const size_t held = (cloud.status == OHMHIP_OK) ? size_t(std::min(cloud.count, capacity)) : 0;
  cloud.positions.resize(held);
  cloud.keys.resize(held);
  cloud.values.resize(held);
  return cloud;
}

/// What ohm derives from an NDT voxel's covariance (ohm/CovarianceVoxel.h:33-67), by the one fp64 rule D1-D6 of
/// include/ohmhip.h ("COVARIANCE DECOMPOSITION") that the device and the host evaluate alike.  Per voxel: eigenvalues
/// ascending, eigenvectors as 9 doubles column-major after D4 (a glm::dmat3's storage), and a status byte
/// (OHMHIP_COV_ABSENT: the map holds no such region or the key is null -- the doubles are zeros --, OHMHIP_COV_DECOMPOSED,
/// OHMHIP_COV_NON_FINITE).
struct CovarianceEigen
{
  std::vector<double> eigenvalues;   ///< 3 a voxel
  std::vector<double> eigenvectors;  ///< 9 a voxel
  std::vector<uint8_t> status;
  int call_status = OHMHIP_OK;
  size_t size() const { return status.size(); }
};

/// covarianceEigenDecomposition (ohm/CovarianceVoxel.cpp:147-154) for covariances the caller holds, 6 floats each
/// (CovarianceVoxel::trianglar_covariance), on the host (ohmhip_covariance_decompose).
inline CovarianceEigen covarianceEigenDecomposition(const float *covariance6, size_t count)
{
  CovarianceEigen e;
  e.eigenvalues.assign(3 * count, 0.0);
  e.eigenvectors.assign(9 * count, 0.0);
  e.status.assign(count, 0);
  e.call_status = ohmhip_covariance_decompose(covariance6, count, e.eigenvalues.data(), e.eigenvectors.data(), nullptr,
                                              nullptr, e.status.data());
  return e;
}

/// ... and for the voxels of `gpu_map`'s device map at `keys`, decomposed on the device (ohmhip_map_covariance_eigen):
/// only the results cross to the host, and the map is read, never changed.
inline CovarianceEigen covarianceEigenDecomposition(GpuMap &gpu_map, const std::vector<Key> &keys)
{
  CovarianceEigen e;
  e.eigenvalues.assign(3 * keys.size(), 0.0);
  e.eigenvectors.assign(9 * keys.size(), 0.0);
  e.status.assign(keys.size(), 0);
  e.call_status = (gpu_map.gpuOk() && gpu_map.syncConfig()) ?
                    ohmhip_map_covariance_eigen(gpu_map.handle(), keys.data(), keys.size(), e.eigenvalues.data(),
                                                e.eigenvectors.data(), e.status.data()) :
                    int(OHMHIP_ERR_INVALID_ARG);
  return e;
}

/// D6 of one decomposition (covarianceEstimatePrimaryNormal with preferred_axis 0, ohm/CovarianceVoxel.cpp:157-177):
/// the column of the first smallest eigenvalue, divided by its length when that is not zero.
inline dvec3 covariancePrimaryNormal(const double *eigenvalues, const double *eigenvectors)
{
  int index = 0;
  for (int i = 0; i < 3; ++i)
  {
    index = (eigenvalues[i] < eigenvalues[index]) ? i : index;
  }
  const double *v = eigenvectors + 3 * index;
  const double length2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  if (!(length2 > 0.0))
  {
    return dvec3{ v[0], v[1], v[2] };
  }
  const double length = std::sqrt(length2);
  return dvec3{ v[0] / length, v[1] / length, v[2] / length };
}

/// covarianceEstimatePrimaryNormal over keys: one normal a key (zeros where the status is OHMHIP_COV_ABSENT), not yet
/// turned towards an up axis.  @return the call's status; `status` (optional) receives the per-voxel bytes.
inline int covarianceEstimatePrimaryNormal(GpuMap &gpu_map, const std::vector<Key> &keys, std::vector<dvec3> &normals,
                                           std::vector<uint8_t> *status = nullptr)
{
  const CovarianceEigen e = covarianceEigenDecomposition(gpu_map, keys);
  normals.assign(keys.size(), dvec3{ 0, 0, 0 });
  for (size_t i = 0; e.call_status == OHMHIP_OK && i < keys.size(); ++i)
  {
    if (e.status[i] != OHMHIP_COV_ABSENT)
    {
      normals[i] = covariancePrimaryNormal(&e.eigenvalues[3 * i], &e.eigenvectors[9 * i]);
    }
  }
  if (status)
  {
    *status = e.status;
  }
  return e.call_status;
}

/// The unit quaternion of a rotation given as 9 doubles column-major, by Shepperd's method: of 1 + m00 + m11 + m22,
/// 1 + m00 - m11 - m22, 1 - m00 + m11 - m22 and 1 - m00 - m11 + m22 (four times w, x, y, z squared) the largest, the
/// first among equals, gives its component as sqrt(.) / 2; the other three are the matching sums or differences of
/// off-diagonal pairs times 0.25 / that component.  The same operations in the same order as ohm_amd.
/// rotation_to_quaternion.
inline dquat covarianceRotationQuaternion(const double *c)
{
  // m(r, c) = c[3 * c + r]
  const double m00 = c[0], m10 = c[1], m20 = c[2], m01 = c[3], m11 = c[4], m21 = c[5], m02 = c[6], m12 = c[7], m22 = c[8];
  const double four[4] = { 1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22 };
  int k = 0;
  for (int i = 1; i < 4; ++i)
  {
    k = (four[i] > four[k]) ? i : k;
  }
  const double big = 0.5 * std::sqrt(four[k] > 0.0 ? four[k] : 0.0);
  const double f = 0.25 / big;
  const double wx = m21 - m12, wy = m02 - m20, wz = m10 - m01;
  const double xy = m01 + m10, xz = m02 + m20, yz = m12 + m21;
  dquat q{};
  switch (k)
  {
  case 0: q.w = big; q.x = wx * f; q.y = wy * f; q.z = wz * f; break;
  case 1: q.w = wx * f; q.x = big; q.y = xy * f; q.z = xz * f; break;
  case 2: q.w = wy * f; q.x = xy * f; q.y = big; q.z = yz * f; break;
  default: q.w = wz * f; q.x = xz * f; q.y = yz * f; q.z = big; break;
  }
  return q;
}

/// covarianceUnitSphereTransformation (ohm/CovarianceVoxel.cpp:180-206) over keys: the rotation (from the D4 matrix)
/// and the scale (D5: |lambda| > 1e-9 ? sqrt(|lambda|) : |lambda|) that deform a unit sphere into each voxel's
/// ellipsoid; zeros where the status is OHMHIP_COV_ABSENT.
inline int covarianceUnitSphereTransformation(GpuMap &gpu_map, const std::vector<Key> &keys, std::vector<dquat> &rotations,
                                              std::vector<dvec3> &scales, std::vector<uint8_t> *status = nullptr)
{
  const CovarianceEigen e = covarianceEigenDecomposition(gpu_map, keys);
  rotations.assign(keys.size(), dquat{ 0, 0, 0, 0 });
  scales.assign(keys.size(), dvec3{ 0, 0, 0 });
  for (size_t i = 0; e.call_status == OHMHIP_OK && i < keys.size(); ++i)
  {
    if (e.status[i] == OHMHIP_COV_ABSENT)
    {
      continue;
    }
    rotations[i] = covarianceRotationQuaternion(&e.eigenvectors[9 * i]);
    double s[3];
    for (int c = 0; c < 3; ++c)
    {
      const double eval = std::abs(e.eigenvalues[3 * i + c]);
      s[c] = (eval > 1e-9) ? std::sqrt(eval) : eval;
    }
    scales[i] = dvec3{ s[0], s[1], s[2] };
  }
  if (status)
  {
    *status = e.status;
  }
  return e.call_status;
}

/// ohm2ply --mode covariance (utils/ohm2ply/ohm2ply.cpp:845-1018) as a query against the device map
/// (ohmhip_map_covariance_ellipsoids): every occupied voxel of an NDT map, in extractCloud's order for the same
/// extents, with its mean position, the rotation (9 doubles column-major, D4) and the scale (D5, without ohm2ply's
/// sqrt(3) display factor) of its covariance's ellipsoid, and its occupancy value.  intersectedVoxels() are the voxels'
/// keys; there are no ranges.
class CovarianceEllipsoids : public Query
{
public:
  explicit CovarianceEllipsoids(GpuMap &gpu_map) : Query(&gpu_map, 0) {}

  /// Only regions from regionKey(min_extents) to regionKey(max_extents) (OHMHIP_CLOUD_USE_EXTENTS).
  void setExtents(const dvec3 &min_extents, const dvec3 &max_extents)
  {
    use_extents_ = true;
    min_extents_ = min_extents;
    max_extents_ = max_extents;
  }
  void clearExtents() { use_extents_ = false; }

  const std::vector<dvec3> &positions() const { return positions_; }
  const std::vector<double> &axes() const { return axes_; }  ///< 9 a voxel
  const std::vector<dvec3> &scales() const { return scales_; }
  const std::vector<float> &values() const { return values_; }
  int lastStatus() const { return last_status_; }

protected:
  bool onExecute() override
  {
    if (!gpu_map_->syncConfig())
    {
      last_status_ = OHMHIP_ERR_INVALID_ARG;
      return false;
    }
    ohmhip_cloud_params p{};
    p.mode = OHMHIP_CLOUD_OCCUPANCY;
    p.flags = use_extents_ ? OHMHIP_CLOUD_USE_EXTENTS : 0u;
    p.surface_distance = std::numeric_limits<float>::infinity();
    const double lo[3] = { min_extents_.x, min_extents_.y, min_extents_.z };
    const double hi[3] = { max_extents_.x, max_extents_.y, max_extents_.z };
    for (int i = 0; i < 3; ++i)
    {
      p.min_extents[i] = lo[i];
      p.max_extents[i] = hi[i];
    }
    uint64_t count = 0;
    last_status_ = ohmhip_map_covariance_ellipsoids_count(gpu_map_->handle(), &p, &count);
    if (last_status_ != OHMHIP_OK)
    {
      return false;
    }
    if (count == 0)
    {
      return true;
    }
    static_assert(sizeof(dvec3) == 3 * sizeof(double), "positions and scales are written as 3 doubles a voxel");
    const uint64_t capacity = count;
    positions_.resize(size_t(capacity));
    axes_.resize(size_t(9 * capacity));
    scales_.resize(size_t(capacity));
    values_.resize(size_t(capacity));
    intersected_voxels_.resize(size_t(capacity));
    last_status_ = ohmhip_map_covariance_ellipsoids(gpu_map_->handle(), &p, capacity, &positions_[0].x, axes_.data(),
                                                    &scales_[0].x, intersected_voxels_.data(), values_.data(), &count);
    if (last_status_ != OHMHIP_OK)
    {
      return false;
    }
    const size_t held = size_t(std::min(count, capacity));
    positions_.resize(held);
    axes_.resize(9 * held);
    scales_.resize(held);
    values_.resize(held);
    intersected_voxels_.resize(held);
    number_of_results_ = held;
    return true;
  }
  void onReset(bool hard_reset) override
  {
    positions_.clear();
    axes_.clear();
    scales_.clear();
    values_.clear();
    if (hard_reset)
    {
      std::vector<dvec3>().swap(positions_);
      std::vector<double>().swap(axes_);
      std::vector<dvec3>().swap(scales_);
      std::vector<float>().swap(values_);
    }
  }

private:
  bool use_extents_ = false;
  dvec3 min_extents_{ 0, 0, 0 }, max_extents_{ 0, 0, 0 };
  std::vector<dvec3> positions_, scales_;
  std::vector<double> axes_;
  std::vector<float> values_;
  int last_status_ = OHMHIP_OK;
};

/// ohm::NearestNeighbours (ohm/NearestNeighbours.h) against the device-resident map: the obstructing voxels within
/// searchRadius() of nearPoint(), in the CPU query's visiting order, or with kQfNearestResult the closest one
/// (GpuMap::nearestNeighbours).  ranges() are float results widened to double, as the reference stores them.  There is
/// no asynchronous form, as for the reference's CPU query (ohm/NearestNeighbours.cpp:287-290).  lastStatus() is that of
/// the last device call: an execute() refused for want of a usable map makes none and leaves it as it was.
class NearestNeighbours : public Query
{
public:
  NearestNeighbours(GpuMap &gpu_map, const dvec3 &near_point, float search_radius, unsigned query_flags)
    : Query(&gpu_map, query_flags)
    , near_point_(near_point)
    , search_radius_(search_radius)
  {}

  dvec3 nearPoint() const { return near_point_; }
  void setNearPoint(const dvec3 &point) { near_point_ = point; }
  float searchRadius() const { return search_radius_; }
  void setSearchRadius(float range) { search_radius_ = range; }

  bool executeAsync() override { return false; }

  const std::vector<Key> &intersectedVoxels() const { return intersected_voxels_; }
  const std::vector<double> &ranges() const { return ranges_; }
  int lastStatus() const { return last_status_; }

protected:
  bool onExecute() override
  {
    std::vector<uint64_t> counts;
    std::vector<float> ranges;
    last_status_ =
      gpu_map_->nearestNeighbours(&near_point_, 1, search_radius_, query_flags_, counts, intersected_voxels_, ranges);
    ranges_.assign(ranges.begin(), ranges.end());
    number_of_results_ = intersected_voxels_.size();
    return last_status_ == OHMHIP_OK;
  }

private:
  dvec3 near_point_{ 0, 0, 0 };
  float search_radius_ = 0.0f;
  int last_status_ = OHMHIP_OK;
};

/// ohm::RayPattern (ohm/RayPattern.h, .cpp): a fixed set of (start, end) ray pairs relative to the sensor.  The host
/// assembles it; it then lives in device memory and moving it to a pose is device work (include/ohmhip.h, RAY PATTERNS).
class RayPattern
{
public:
  RayPattern() = default;
  virtual ~RayPattern() { dropDevicePattern(); }
  RayPattern(const RayPattern &) = delete;
  RayPattern &operator=(const RayPattern &) = delete;

  void addPoints(const dvec3 *points, size_t point_count)
  {
    for (size_t i = 0; i < point_count; ++i)
    {
      addRay(dvec3{ 0.0, 0.0, 0.0 }, points[i]);
    }
  }
  void addPoint(const dvec3 &point) { addPoints(&point, 1); }
  void addRays(const dvec3 *ray_pairs, size_t elements)
  {
    for (size_t i = 0; i + 1 < elements; i += 2)
    {
      addRay(ray_pairs[i], ray_pairs[i + 1]);
    }
  }
  void addRay(const dvec3 &ray_start, const dvec3 &ray_end)
  {
    dropDevicePattern();
    sample_pairs_.push_back(ray_start);
    sample_pairs_.push_back(ray_end);
  }
  size_t rayCount() const { return sample_pairs_.size() / 2; }
  size_t pointCount() const { return sample_pairs_.size(); }
  const dvec3 *rayPoints() const { return sample_pairs_.data(); }

  /// RayPattern::buildRays (RayPattern.cpp:58-70), computed on the device.  @return elements in @p rays.
  size_t buildRays(std::vector<dvec3> *rays, const dvec3 &position, const dquat &rotation, double scaling = 1.0) const
  {
    const double pose[7] = { position.x, position.y, position.z, rotation.x, rotation.y, rotation.z, rotation.w };
    return buildRays(rays, pose, 1, OHMHIP_POSE_QUAT, scaling);
  }
  /// ... with a column-major 4 x 4 matrix (glm::dmat4's memory, RayPattern.cpp:72-84).
  size_t buildRays(std::vector<dvec3> *rays, const double pattern_transform[16]) const
  {
    return buildRays(rays, pattern_transform, 1, OHMHIP_POSE_MAT4, 1.0);
  }
  /// Extension: @p pose_count poses at once, pose major.
  size_t buildRays(std::vector<dvec3> *rays, const double *poses, size_t pose_count, int pose_kind, double scaling) const
  {
    rays->assign(pose_count * pointCount(), dvec3{ 0.0, 0.0, 0.0 });
    OHMHIP_GPUAPICHECK(ohmhip_pattern_build_rays(devicePattern(), poses, pose_count, pose_kind, scaling,
                                                 rays->empty() ? nullptr : &(*rays)[0].x));
    return rays->size();
  }

  /// The device copy, made when first needed and dropped when the pattern changes.
  ohmhip_pattern_t devicePattern() const
  {
    if (!handle_)
    {
      OHMHIP_GPUAPICHECK(ohmhip_pattern_create(sample_pairs_.empty() ? nullptr : &sample_pairs_[0].x, rayCount(), &handle_));
    }
    return handle_;
  }

private:
  void dropDevicePattern()
  {
    if (handle_)
    {
      ohmhip_pattern_destroy(handle_);  // (waits for the device: batches in flight may read its buffers)
      handle_ = nullptr;
    }
  }

  std::vector<dvec3> sample_pairs_;
  mutable ohmhip_pattern_t handle_ = nullptr;
};

/// ohm::RayPatternConical (ohm/RayPatternConical.cpp:20-75), the constructor as written there in glm's operation order:
/// normalise as v * (1 / sqrt(dot)), quaternion * vector as v + ((uv * w) + uuv) * 2, both loop angles accumulated.
class RayPatternConical : public RayPattern
{
public:
  RayPatternConical(const dvec3 &cone_axis, double cone_angle, double range, double angular_resolution,
                    double min_range = 0)
  {
    const double inv = 1.0 / std::sqrt((cone_axis.x * cone_axis.x + cone_axis.y * cone_axis.y) + cone_axis.z * cone_axis.z);
    const dvec3 n{ cone_axis.x * inv, cone_axis.y * inv, cone_axis.z * inv };
    addRay(scaled(n, min_range), scaled(n, range));
    const dvec3 deflection_base{ n.z, n.x, n.y };
    const double two_pi = 2 * 3.14159265358979323846;
    for (double circle_angle = 0; angular_resolution > 0 && circle_angle < two_pi; circle_angle += angular_resolution)
    {
      const dvec3 deflection_axis = rotate(angleAxis(circle_angle, n), deflection_base);
      for (double deflection_angle = angular_resolution; deflection_angle <= 0.5 * cone_angle;
           deflection_angle += angular_resolution)
      {
        const dvec3 ray_dir = rotate(angleAxis(deflection_angle, deflection_axis), n);
        addRay(scaled(ray_dir, min_range), scaled(ray_dir, range));
      }
    }
  }

private:
  static dvec3 scaled(const dvec3 &v, double s) { return dvec3{ v.x * s, v.y * s, v.z * s }; }
  static dvec3 cross(const dvec3 &a, const dvec3 &b)
  {
    return dvec3{ a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y };
  }
  static dquat angleAxis(double angle, const dvec3 &axis)
  {
    const double s = std::sin(angle * 0.5);
    return dquat{ axis.x * s, axis.y * s, axis.z * s, std::cos(angle * 0.5) };
  }
  static dvec3 rotate(const dquat &q, const dvec3 &v)
  {
    const dvec3 u{ q.x, q.y, q.z };
    const dvec3 uv = cross(u, v);
    const dvec3 uuv = cross(u, uv);
    return dvec3{ v.x + ((uv.x * q.w) + uuv.x) * 2.0, v.y + ((uv.y * q.w) + uuv.y) * 2.0,
                  v.z + ((uv.z * q.w) + uuv.z) * 2.0 };
  }
};

/// ohm::ClearingPattern (ohm/ClearingPattern.h, .cpp): applies a RayPattern at a pose so that every ray lowers the first
/// occupied voxel it meets and stops there.  apply() is one library call (ohmhip_map_apply_pattern): rays waiting in the
/// map's coalescing buffer are launched first, the batch runs with the miss value scaled by probability_scaling, and
/// GpuMap::missValue() never changes.  applyMany() is an extension: K poses in one device batch, with the result of K
/// apply() calls.
class ClearingPattern
{
public:
  static const unsigned kDefaultRayFlags = kRfEndPointAsFree | kRfStopOnFirstOccupied | kRfExcludeFree | kRfExcludeUnobserved;

  ClearingPattern(const RayPattern *pattern, bool take_ownership) : pattern_(pattern), has_ownership_(take_ownership) {}
  ~ClearingPattern()
  {
    if (has_ownership_)
    {
      delete pattern_;
    }
  }
  ClearingPattern(const ClearingPattern &) = delete;
  ClearingPattern &operator=(const ClearingPattern &) = delete;

  const RayPattern *pattern() const { return pattern_; }
  bool hasPatternOwnership() const { return has_ownership_; }
  unsigned rayFlags() const { return ray_flags_; }
  /// ClearingPattern.cpp:40-44: kRfReverseWalk is never set.
  void setRayFlags(unsigned ray_flags) { ray_flags_ = ray_flags & ~unsigned(kRfReverseWalk); }

  /// @return points integrated (2 per ray the map's ray filter passed); the reference returns nothing.
  size_t apply(GpuMap *map, const dvec3 &position, const dquat &rotation, float probability_scaling = 1.0f)
  {
    const double pose[7] = { position.x, position.y, position.z, rotation.x, rotation.y, rotation.z, rotation.w };
    return applyMany(map, pose, 1, OHMHIP_POSE_QUAT, probability_scaling);
  }
  /// ... with a column-major 4 x 4 matrix (glm::dmat4's memory).
  size_t apply(GpuMap *map, const double pattern_transform[16], float probability_scaling = 1.0f)
  {
    return applyMany(map, pattern_transform, 1, OHMHIP_POSE_MAT4, probability_scaling);
  }
  size_t applyMany(GpuMap *map, const double *poses, size_t pose_count, int pose_kind = OHMHIP_POSE_QUAT,
                   float probability_scaling = 1.0f)
  {
    if (!map->syncConfig())  // the host map's values, as before every batch
    {
      return 0;
    }
    size_t integrated = 0;
    OHMHIP_GPUAPICHECK(ohmhip_map_apply_pattern(map->handle(), pattern_->devicePattern(), poses, pose_count, pose_kind, 1.0,
                                                probability_scaling, ray_flags_, &integrated));
    have_last_ = pose_count > 0 && pattern_->rayCount() > 0;
    return integrated;
  }

  /// The rays of the last apply() (or of a buildRays() on the pattern since), read back from the device buffer the batch
  /// was given.  Valid until the next call.
  const dvec3 *lastRaySet(size_t *element_count)
  {
    last_ray_set_.clear();
    size_t elements = 0;
    if (have_last_)
    {
      OHMHIP_GPUAPICHECK(ohmhip_pattern_last_rays(pattern_->devicePattern(), nullptr, &elements));
      last_ray_set_.resize(elements);
      if (elements)
      {
        OHMHIP_GPUAPICHECK(ohmhip_pattern_last_rays(pattern_->devicePattern(), &last_ray_set_[0].x, &elements));
      }
    }
    *element_count = elements;
    return last_ray_set_.data();
  }

private:
  const RayPattern *pattern_;
  bool has_ownership_;
  unsigned ray_flags_ = kDefaultRayFlags;
  bool have_last_ = false;
  std::vector<dvec3> last_ray_set_;
};

/// ohm::configureGpu / gpuDevice (ohmgpu/OhmGpu.h:40-66): select the process-wide device.
inline int configureGpu(int device_index = 0)
{
  int count = 0;
  if (ohmhip_device_count(&count) != OHMHIP_OK || device_index >= count)
  {
    return 1;
  }
  return ohmhip_device_select(device_index) == OHMHIP_OK ? 0 : 1;
}
}  // namespace ohm

#endif  // OHMHIP_OHMGPUMAP_H
