// gpumap_driver.cpp -- C++14 test driver for the host mirror (OhmGpuMap.h over the C ABI).  Links libohmhip.so only; built
// with plain g++ (no hipcc, no glm).  The Python side is tests/cpp_driver.py.
//
//   gpumap_driver <mode> <resolution> <batch_rays> <rays.bin> <out.bin> [mode arguments ...]
//
// The modes are the entries of kModes at the end of this file, one function each; the comment at a function gives the
// mode's extra arguments and the layout of what it writes.  Unless a mode says otherwise:
//   rays.bin: u64 n_points, then n_points * 3 doubles (start, end point pairs).
//   a map dump (writeRegionDump): u64 regions, per region i16[3] key, then per enabled layer (ascending id): u32 layer
//   id, u64 bytes, payload.
//   keys are written as i16[3] region, u8[3] local (9 bytes) where a layout says "key", and as the 10-byte record
//   where it says so.
#include "OhmGpuMap.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace
{
enum ExitCode : int
{
  kOk = 0,
  kUsage = 2,            ///< unknown mode, too few arguments
  kNoDevice = 3,
  kInput = 4,            ///< an input file cannot be read
  kMapInvalid = 5,       ///< GpuMap::gpuOk() is false
  kOutput = 6,           ///< the output file cannot be written
  kUnexpected = 7,       ///< a count or a refusal is not what the mode expects (e.g. not every point was integrated)
  kFailedCall = 8,       ///< a call of the mirror failed
  kCacheView = 9,        ///< occcoalesce: the GpuCache view reports the wrong layers or limit
  kApiException = 10,    ///< gputil::ApiException
  kRoutedBlock = 11,     ///< occpart: the routed block was not integrated whole
  kExchange = 12         ///< occpartint: the exchange failed or lost rays
};

/// Ends the mode with an exit code (main returns it).
struct Failure
{
  ExitCode code;
};

void check(bool ok, ExitCode code)
{
  if (!ok)
  {
    throw Failure{ code };
  }
}

/// The five fixed arguments and what follows them.
struct Args
{
  std::string mode;
  double resolution;
  size_t batch_rays;
  const char *input;
  const char *output;
  int extra_count;
  char **extra;

  bool has(int i) const { return i < extra_count; }
  double real(int i, double otherwise) const { return has(i) ? std::atof(extra[i]) : otherwise; }
  long integer(int i, long otherwise) const { return has(i) ? std::strtol(extra[i], nullptr, 0) : otherwise; }
};

/// An input file that closes itself; a short read ends the mode with kInput.
class InFile
{
public:
  explicit InFile(const char *path) : file_(std::fopen(path, "rb")) { check(file_ != nullptr, kInput); }
  ~InFile() { std::fclose(file_); }
  InFile(const InFile &) = delete;
  InFile &operator=(const InFile &) = delete;
  void bytes(void *data, size_t size) { check(size == 0 || std::fread(data, 1, size, file_) == size, kInput); }
  template <typename T>
  T value()
  {
    T v;
    bytes(&v, sizeof(T));
    return v;
  }
  template <typename T>
  std::vector<T> array(size_t count)
  {
    std::vector<T> v(count);
    bytes(v.data(), count * sizeof(T));
    return v;
  }

private:
  FILE *file_;
};

/// The output file: closes itself, and a failed write ends the mode with kOutput.
class OutFile
{
public:
  explicit OutFile(const char *path, ExitCode cannot_open = kOutput) : file_(std::fopen(path, "wb"))
  {
    check(file_ != nullptr, cannot_open);
  }
  ~OutFile() { std::fclose(file_); }
  OutFile(const OutFile &) = delete;
  OutFile &operator=(const OutFile &) = delete;
  void bytes(const void *data, size_t size) { check(size == 0 || std::fwrite(data, 1, size, file_) == size, kOutput); }
  template <typename T>
  void value(const T &v)
  {
    bytes(&v, sizeof(T));
  }
  template <typename T>
  void array(const std::vector<T> &v)
  {
    bytes(v.data(), v.size() * sizeof(T));
  }
  /// i16[3] region, u8[3] local; array() of keys writes the 10-byte records.
  void key(const ohm::Key &k)
  {
    bytes(k.region, sizeof(k.region));
    bytes(k.local, sizeof(k.local));
  }

private:
  FILE *file_;
};

std::vector<ohm::dvec3> readRays(const char *path)
{
  InFile in(path);
  const uint64_t n_points = in.value<uint64_t>();
  return in.array<ohm::dvec3>(size_t(n_points));
}

void writeRegionDump(OutFile &out, const ohm::OccupancyMap &map)
{
  out.value(uint64_t(map.regionCount()));
  for (const auto &entry : map.chunks())
  {
    out.value(entry.first);
    for (uint32_t layer = 0; layer < uint32_t(OHMHIP_LID_COUNT); ++layer)
    {
      if (map.hasLayer(int(layer)))
      {
        const std::vector<uint8_t> &block = entry.second.voxel_blocks[layer];
        out.value(layer);
        out.value(uint64_t(block.size()));
        out.array(block);
      }
    }
  }
}

/// integrateRays in calls of `batch_rays` rays (0: one call), as the reference's gpuMapTest() harness batches
/// (tests/ohmtestgpu/GpuMapTest.cpp:68-205); `after_batch` runs after each call.  @return the points integrated, which
/// the caller holds against rays.size() & ~1.
size_t integrateInBatches(ohm::GpuMap &gpu_map, const std::vector<ohm::dvec3> &rays, size_t batch_rays,
                          const std::function<void()> &after_batch = {})
{
  const size_t points = rays.size() & ~size_t(1);
  const size_t step = batch_rays ? 2 * batch_rays : points;
  size_t total = 0;
  for (size_t at = 0; at < points; at += step)
  {
    total += gpu_map.integrateRays(rays.data() + at, std::min(step, points - at), nullptr, nullptr, ohm::kRfDefault);
    if (after_batch)
    {
      after_batch();
    }
  }
  return total;
}

ohm::OccupancyMap hostMap(double resolution, bool with_mean, int region_dim = 32)
{
  ohm::OccupancyMap map(resolution, region_dim, region_dim, region_dim);
  if (with_mean)
  {
    map.addLayer(OHMHIP_LID_MEAN);
  }
  return map;
}

/// A host map and its GpuMap.
struct ResidentMap
{
  ohm::OccupancyMap map;
  ohm::GpuMap gpu;
  ResidentMap(double resolution, bool with_mean) : map(hostMap(resolution, with_mean)), gpu(&map, true) {}
};

/// ... with the rays of the input file integrated in batches -- still collected by batch coalescing when the mode asks
/// its question.
struct BuiltMap : ResidentMap
{
  std::vector<ohm::dvec3> rays;
  BuiltMap(const Args &args, bool with_mean) : ResidentMap(args.resolution, with_mean), rays(readRays(args.input))
  {
    check(integrateInBatches(gpu, rays, args.batch_rays) == (rays.size() & ~size_t(1)), kFailedCall);
  }
};

// -- the integration modes: the rays into a map in batches, syncVoxels(), the map dump -----------------------------------

/// What every integration mode ends with.  Prints "integrated <n> of <points> points, <regions> regions".
int finishIntegration(const Args &args, ohm::OccupancyMap &map, ohm::GpuMap &gpu_map, size_t total, size_t points)
{
  gpu_map.syncVoxels();
  std::printf("integrated %zu of %llu points, %zu regions\n", total, (unsigned long long)points, map.regionCount());
  OutFile out(args.output);
  writeRegionDump(out, map);
  return (total == points) ? kOk : kUnexpected;
}

template <typename Map>
std::unique_ptr<ohm::GpuMap> makeGpuMap(ohm::OccupancyMap &map, const Args &args)
{
  std::unique_ptr<ohm::GpuMap> gpu_map(new Map(&map, true, unsigned(args.batch_rays * 2)));
  check(gpu_map->gpuOk(), kMapInvalid);
  return gpu_map;
}

/// occ, occmean, ndt, tsdf: ohm::GpuMap (with the mean layer), GpuNdtMap, GpuTsdfMap.
template <typename Map, bool with_mean>
int modeIntegrate(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map = hostMap(args.resolution, with_mean);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<Map>(map, args);
  return finishIntegration(args, map, *gpu_map, integrateInBatches(*gpu_map, rays, args.batch_rays), rays.size());
}

/// occcoalesce: GpuMap::setBatchCoalescing so that every fourth call launches a device batch; the GpuCache view.
int modeCoalesce(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map(args.resolution);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<ohm::GpuMap>(map, args);
  gpu_map->setBatchCoalescing(3 * args.batch_rays + 1);
  const size_t total = integrateInBatches(*gpu_map, rays, args.batch_rays);
  gpu_map->gpuCache()->flush();  // GpuCache::flush == syncVoxels
  // (occupancy only, no memory limit set)
  check(gpu_map->gpuCache()->layerCount() == 1u && gpu_map->gpuCache()->targetGpuAllocSize() == 0u, kCacheView);
  return finishIntegration(args, map, *gpu_map, total, rays.size());
}

/// occowner: GpuMap::setRegionOwnership(2, 1): this map is rank 1 of a two-way region partition.
int modeOwner(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map(args.resolution);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<ohm::GpuMap>(map, args);
  gpu_map->setRegionOwnership(2, 1);
  return finishIntegration(args, map, *gpu_map, integrateInBatches(*gpu_map, rays, args.batch_rays), rays.size());
}

/// occclipbox: GpuMap.ClipBox (tests/ohmtestgpu/GpuMapTest.cpp:633-647): a RayFilterFunction wrapping clipBounded.
int modeClipBox(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map(args.resolution);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<ohm::GpuMap>(map, args);
  const ohm::Aabb clip_box(ohm::dvec3{ -1.0, -1.0, -1.0 }, ohm::dvec3{ 2.0, 2.0, 2.0 });
  gpu_map->setRayFilter([clip_box](ohm::dvec3 *start, ohm::dvec3 *end, unsigned *filter_flags) {
    return ohm::clipBounded(start, end, filter_flags, clip_box);
  });
  return finishIntegration(args, map, *gpu_map, integrateInBatches(*gpu_map, rays, args.batch_rays), rays.size());
}

/// occchain: GpuMap::setRayFilter(DeviceRayFilter) -- goodRay(6) then clipBounded on the box (-1, -1, -0.5)-(2, 1.5, 1),
/// evaluated on the device -- on a map with a mean layer and 16^3 regions; the rays in host-pointer calls of batch_rays.
/// out: u64 points the calls reported, u64 rays applyRayFilter kept, its flag byte per ray, the map dump.  Also checked
/// here: the chain's host form gives applyRayFilter's verdicts, and clearRayFilter empties the device chain.
int modeChain(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map = hostMap(args.resolution, true, 16);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<ohm::GpuMap>(map, args);
  const ohm::Aabb box(ohm::dvec3{ -1.0, -1.0, -0.5 }, ohm::dvec3{ 2.0, 1.5, 1.0 });
  ohm::DeviceRayFilter chain;
  chain.goodRay(6.0).clipBounded(box);
  check(gpu_map->setRayFilter(chain) && !gpu_map->rayFilter() && gpu_map->deviceRayFilter().stages().size() == 2u,
        kFailedCall);
  std::vector<ohm::dvec3> moved;
  std::vector<unsigned char> flags;
  const size_t kept = gpu_map->applyRayFilter(rays.data(), rays.size(), moved, flags);
  check(gpu_map->lastStatus() == OHMHIP_OK, kFailedCall);
  size_t host_kept = 0;
  for (size_t i = 0; i + 1 < rays.size(); i += 2)
  {
    ohm::dvec3 start = rays[i], end = rays[i + 1];
    unsigned host_flags = 0;
    const bool ok = chain(&start, &end, &host_flags);
    host_kept += ok ? 1u : 0u;
    check(host_flags == flags[i / 2] && std::memcmp(&start, &moved[i], sizeof(start)) == 0 &&
            std::memcmp(&end, &moved[i + 1], sizeof(end)) == 0,
          kUnexpected);
  }
  check(host_kept == kept, kUnexpected);
  const size_t total = integrateInBatches(*gpu_map, rays, args.batch_rays);
  gpu_map->syncVoxels();
  gpu_map->clearRayFilter();
  unsigned stages_left = 99;
  check(ohmhip_map_ray_filter_stages(gpu_map->handle(), nullptr, 0, &stages_left) == OHMHIP_OK && stages_left == 0u,
        kUnexpected);
  std::printf("integrated %zu of %llu points, %zu kept by the chain, %zu regions\n", total,
              (unsigned long long)rays.size(), kept, map.regionCount());
  OutFile out(args.output);
  out.value(uint64_t(total));
  out.value(uint64_t(kept));
  out.array(flags);
  writeRegionDump(out, map);
  return (total == 2 * kept) ? kOk : kUnexpected;
}

/// The rays in calls of `batch_rays` rays (0: one call), each written to the start of `device_rays`, which grows to hold
/// it; each(points in the call).
void forEachDeviceBatch(const std::vector<ohm::dvec3> &rays, size_t batch_rays, gputil::Buffer &device_rays,
                        const std::function<void(size_t)> &each)
{
  const size_t step = batch_rays ? batch_rays * 2 : rays.size();
  for (size_t i = 0; i < rays.size(); i += step)
  {
    const size_t count = std::min(step, rays.size() - i);
    if (!device_rays.isValid())
    {
      device_rays.create(step * sizeof(ohm::dvec3));
    }
    device_rays.write(rays.data() + i, count * sizeof(ohm::dvec3));
    each(count);
  }
}

/// occdev: the sample points (odd entries) go through ohm::GpuTransformSamples with a static identity trajectory and
/// are integrated straight from the device buffer (all rays then start at the origin).
int modeDeviceRays(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map(args.resolution);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<ohm::GpuMap>(map, args);
  gputil::Device device;
  gputil::Queue queue = device.defaultQueue();
  ohm::GpuTransformSamples transform(device);
  gputil::Buffer device_rays;
  const double times[2] = { 0.0, 1.0 };
  const ohm::dvec3 translations[2] = { { 0, 0, 0 }, { 0, 0, 0 } };
  const ohm::dquat rotations[2] = { { 0, 0, 0, 1 }, { 0, 0, 0, 1 } };
  const size_t step = args.batch_rays ? args.batch_rays * 2 : rays.size();
  std::vector<ohm::dvec3> samples;
  std::vector<double> sample_times;
  size_t total = 0;
  for (size_t i = 0; i < rays.size(); i += step)
  {
    const size_t count = std::min(step, rays.size() - i);
    samples.clear();
    sample_times.clear();
    for (size_t k = 1; k < count; k += 2)
    {
      samples.push_back(rays[i + k]);
      sample_times.push_back(0.25 + 0.5 * double(k) / double(count));
    }
    const unsigned elements = transform.transform(times, translations, rotations, 2, sample_times.data(), samples.data(),
                                                  unsigned(samples.size()), queue, device_rays);
    total += gpu_map->integrateRays(device_rays, elements, ohm::kRfDefault);
  }
  return finishIntegration(args, map, *gpu_map, total, rays.size());
}

/// occpart: rank 1 of a two-way partition by a table -- region blocks (2 x 2 x 2 regions) with block x >= 1 belong to
/// rank 1.  Every batch is routed on the device and the block addressed to this rank integrated (what the all-to-all
/// would deliver from a single source rank); the points of rays that never reach rank 1's territory count as done.
int modePartition(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map(args.resolution);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<ohm::GpuMap>(map, args);
  ohm::GpuMap::RegionPartition part;
  part.world_size = 2;
  part.rank = 1;
  part.block_shift = 1;
  part.grid_origin[0] = 0;
  part.grid_dims[0] = 2;
  part.grid_dims[1] = part.grid_dims[2] = 1;
  part.owners = { 0, 1 };
  gpu_map->setRegionPartition(part);
  gputil::Buffer device_rays, routed;
  std::vector<uint32_t> counts;
  size_t total = 0;
  forEachDeviceBatch(rays, args.batch_rays, device_rays, [&](size_t count) {
    gpu_map->routeRays(device_rays, count, ohm::kRfDefault, routed, counts);
    if (counts[1])
    {
      std::vector<ohm::dvec3> block(size_t(counts[1]) * 2);
      routed.read(block.data(), block.size() * sizeof(ohm::dvec3), size_t(counts[0]) * 2 * sizeof(ohm::dvec3));
      gputil::Buffer mine;
      mine.create(block.size() * sizeof(ohm::dvec3));
      mine.write(block.data(), block.size() * sizeof(ohm::dvec3));
      check(gpu_map->integrateRays(mine, block.size(), ohm::kRfDefault) == block.size(), kRoutedBlock);
      gpu_map->syncVoxels();  // (the block buffer goes out of scope: the batch must have read it)
    }
    total += count;
  });
  return finishIntegration(args, map, *gpu_map, total, rays.size());
}

/// occpartint: ohm::PartitionedIntegrator at world size 1 over the library's own RCCL communicator: every batch is
/// routed on the device, exchanged (count all-gather + the block a rank addresses to itself) and integrated with the
/// previous batches still in flight -- each batch from the one device buffer, rewritten without any wait in between
/// (it is free again when integrateRays returned).
int modePartitionedIntegrator(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map(args.resolution);
  const std::unique_ptr<ohm::GpuMap> gpu_map = makeGpuMap<ohm::GpuMap>(map, args);
  const auto id = ohm::RayCommunicator::uniqueId();
  ohm::RayCommunicator comm(id, 1, 0);
  ohm::GpuMap::RegionPartition whole;  // world size 1: everything belongs to rank 0
  ohm::PartitionedIntegrator integrator(*gpu_map, whole, comm);
  gputil::Buffer device_rays;
  size_t total = 0;
  forEachDeviceBatch(rays, args.batch_rays, device_rays, [&](size_t count) {
    total += integrator.integrateRays(device_rays, count, ohm::kRfDefault);
    check(integrator.lastStatus() == OHMHIP_OK && integrator.raysReceived() == integrator.sendCounts()[0], kExchange);
  });
  return finishIntegration(args, map, *gpu_map, total, rays.size());
}

// -- host only ------------------------------------------------------------------------------------------------------------

/// filter:<clipbounded|cliptobounds|clipray|goodray>: one of the stock ray filters of the mirror over the rays; per ray
/// accepted (1 byte), filter flags (1 byte), start and end (6 doubles).  Box (-1,-1,-1)..(2,2,2), length = resolution.
int modeRayFilter(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  const ohm::Aabb box(ohm::dvec3{ -1.0, -1.0, -1.0 }, ohm::dvec3{ 2.0, 2.0, 2.0 });
  const double length = args.resolution;
  ohm::RayFilterFunction filter;
  if (args.mode == "filter:clipbounded")
  {
    filter = [&box](ohm::dvec3 *s, ohm::dvec3 *e, unsigned *f) { return ohm::clipBounded(s, e, f, box); };
  }
  else if (args.mode == "filter:cliptobounds")
  {
    filter = [&box](ohm::dvec3 *s, ohm::dvec3 *e, unsigned *f) { return ohm::clipToBounds(s, e, f, box); };
  }
  else if (args.mode == "filter:clipray")
  {
    filter = [length](ohm::dvec3 *s, ohm::dvec3 *e, unsigned *f) { return ohm::clipRayFilter(s, e, f, length); };
  }
  else
  {
    filter = [length](ohm::dvec3 *s, ohm::dvec3 *e, unsigned *f) { return ohm::goodRayFilter(s, e, f, length); };
  }
  OutFile out(args.output, kInput);  // (this mode has always answered 4 here)
  for (size_t i = 0; i + 1 < rays.size(); i += 2)
  {
    ohm::dvec3 start = rays[i], end = rays[i + 1];
    unsigned flags = 0;
    const bool ok = filter(&start, &end, &flags);
    const unsigned char head[2] = { static_cast<unsigned char>(ok), static_cast<unsigned char>(flags) };
    out.value(head);
    out.value(start);
    out.value(end);
  }
  return kOk;
}

// -- one feature each -------------------------------------------------------------------------------------------------------

/// transform: ohm::GpuTransformSamples::transform on a trajectory and samples from the input file, the output buffer to
/// the output file (resolution and batch size are not used).  in: u64 transforms, u64 points, f64 max_range, then
/// times[transforms], translations (dvec3 each), rotations (dquat x, y, z, w each), sample times[points], local samples
/// (dvec3 each).  out: u64 elements (2 x valid samples), then elements x (x, y, z) read back from the buffer.
int modeTransform(const Args &args)
{
  InFile in(args.input);
  const size_t transform_count = size_t(in.value<uint64_t>()), point_count = size_t(in.value<uint64_t>());
  const double max_range = in.value<double>();
  // The file is read as plain doubles and every struct is filled member by member, so that the order in which dvec3
  // and dquat declare their members matters: the mirror casts these arrays back to double pointers.
  const std::vector<double> times = in.array<double>(transform_count);
  const std::vector<double> raw_translations = in.array<double>(3 * transform_count);
  const std::vector<double> raw_rotations = in.array<double>(4 * transform_count);
  const std::vector<double> sample_times = in.array<double>(point_count);
  const std::vector<double> raw_samples = in.array<double>(3 * point_count);
  std::vector<ohm::dvec3> translations(transform_count), samples(point_count);
  std::vector<ohm::dquat> rotations(transform_count);
  for (size_t i = 0; i < transform_count; ++i)
  {
    translations[i].x = raw_translations[3 * i + 0];
    translations[i].y = raw_translations[3 * i + 1];
    translations[i].z = raw_translations[3 * i + 2];
    rotations[i].x = raw_rotations[4 * i + 0];
    rotations[i].y = raw_rotations[4 * i + 1];
    rotations[i].z = raw_rotations[4 * i + 2];
    rotations[i].w = raw_rotations[4 * i + 3];
  }
  for (size_t i = 0; i < point_count; ++i)
  {
    samples[i].x = raw_samples[3 * i + 0];
    samples[i].y = raw_samples[3 * i + 1];
    samples[i].z = raw_samples[3 * i + 2];
  }
  gputil::Device device;
  gputil::Queue queue = device.defaultQueue();
  ohm::GpuTransformSamples transform(device);
  gputil::Buffer device_rays;
  const uint64_t elements =
    transform.transform(times.data(), translations.data(), rotations.data(), unsigned(transform_count),
                        sample_times.data(), samples.data(), unsigned(point_count), queue, device_rays, max_range);
  check(transform.lastStatus() == OHMHIP_OK, kFailedCall);
  std::vector<ohm::dvec3> world(elements);
  if (elements)
  {
    device_rays.read(world.data(), sizeof(ohm::dvec3) * elements);
  }
  OutFile out(args.output);
  out.value(elements);
  for (const ohm::dvec3 &p : world)
  {
    const double xyz[3] = { p.x, p.y, p.z };
    out.value(xyz);
  }
  return kOk;
}

/// clearing <tx> <ty> <tz>: RayPattern.Clearing as the reference writes it (tests/ohmtestgpu/GpuRayPatternTests.cpp:28-85):
/// a line of 20 occupied voxels along x written directly, hit probability 0.51, miss probability 0; a one-ray pattern
/// along y, rotated onto x by angleAxis(-pi/2, z) and moved to (tx, ty, tz) (the centre of voxel 0), applied 20 times
/// through ohm::ClearingPattern.  <batch_rays> and <rays.bin> are not used.  out: per application the 2 points of
/// lastRaySet() (6 doubles), u64 points integrated and the occupancy words of the voxels (0..31, 0, 0) after
/// syncVoxels(); then the whole occupancy block of region (0, 0, 0) and the map's miss value (float).
int modeClearing(const Args &args)
{
  check(args.has(2), kUsage);
  const unsigned voxel_count = 20;
  ohm::OccupancyMap line_map(args.resolution);
  line_map.setHitProbability(0.51f);
  line_map.setMissProbability(0.0f);
  std::vector<uint8_t> &block = line_map.region({ { 0, 0, 0 } }).voxel_blocks[OHMHIP_LID_OCCUPANCY];
  {
    std::vector<float> values(line_map.regionVoxelVolume(), std::numeric_limits<float>::infinity());
    std::fill(values.begin(), values.begin() + voxel_count, line_map.hitValue());
    block.resize(sizeof(float) * values.size());
    std::memcpy(block.data(), values.data(), block.size());
  }
  ohm::GpuMap line_gpu_map(&line_map, true);
  line_gpu_map.uploadRegions(nullptr, 0);
  ohm::RayPattern line_pattern;
  line_pattern.addPoint(ohm::dvec3{ 0, line_map.resolution() * voxel_count, 0 });
  ohm::ClearingPattern clearing(&line_pattern, false);
  const ohm::dvec3 pattern_translate{ args.real(0, 0), args.real(1, 0), args.real(2, 0) };
  const double half_angle = (-0.5 * 3.14159265358979323846) * 0.5;  // glm::angleAxis(-0.5 * M_PI, (0, 0, 1))
  const ohm::dquat rotation{ 0 * std::sin(half_angle), 0 * std::sin(half_angle), 1 * std::sin(half_angle),
                             std::cos(half_angle) };
  OutFile out(args.output);
  for (unsigned i = 0; i < voxel_count; ++i)
  {
    const uint64_t integrated = clearing.apply(&line_gpu_map, pattern_translate, rotation);
    line_gpu_map.syncVoxels();
    size_t elements = 0;
    const ohm::dvec3 *ray_set = clearing.lastRaySet(&elements);
    check(elements == 2, kUnexpected);
    out.bytes(ray_set, 2 * sizeof(ohm::dvec3));
    out.value(integrated);
    out.bytes(block.data(), 32 * sizeof(float));
  }
  out.array(block);
  out.value(line_gpu_map.missValue());
  return kOk;
}

/// heightmapfill: ohm::Heightmap in HeightmapMode::kSimpleFill over a map whose voxels are written directly; <rays.bin>
/// is a scene file instead (<batch_rays> is not used).  in: i32 region dims[3], f64 reference[3], f64 floor, ceiling,
/// min_clearance, i32 up axis, u32 flags (1 virtual surfaces, 2 promote below), u64 regions, then per region i16[3]
/// key and its occupancy block.  out: u32 ma, u32 mb, the ohmhip_heightmap_fill_stats, u64 surface and u64 virtual
/// cells as getHeightmapVoxelInfo names them, then the occupancy, HeightmapVoxel, source visit arrays and the log.
int modeHeightmapFill(const Args &args)
{
  InFile in(args.input);
  const std::vector<int32_t> dims = in.array<int32_t>(3);
  const std::vector<double> numbers = in.array<double>(6);
  const int32_t up_axis = in.value<int32_t>();
  const uint32_t flags = in.value<uint32_t>();
  const uint64_t regions = in.value<uint64_t>();
  ohm::OccupancyMap fill_map(args.resolution, dims[0], dims[1], dims[2]);
  for (uint64_t i = 0; i < regions; ++i)
  {
    const auto key = in.value<std::array<int16_t, 3>>();
    std::vector<uint8_t> &block = fill_map.region(key).voxel_blocks[OHMHIP_LID_OCCUPANCY];
    block.resize(sizeof(float) * fill_map.regionVoxelVolume());
    in.bytes(block.data(), block.size());
  }
  ohm::GpuMap fill_gpu_map(&fill_map, true);
  fill_gpu_map.uploadRegions(nullptr, 0);
  ohm::Heightmap heightmap(args.resolution, numbers[5], ohm::UpAxis(up_axis));
  heightmap.setOccupancyMap(&fill_gpu_map);
  heightmap.setFloor(numbers[3]);
  heightmap.setCeiling(numbers[4]);
  heightmap.setGenerateVirtualSurface((flags & 1u) != 0);
  heightmap.setPromoteVirtualBelow((flags & 2u) != 0);
  heightmap.setKeepVisitLog(true);
  const ohm::dvec3 reference{ numbers[0], numbers[1], numbers[2] };
  heightmap.setMode(ohm::HeightmapMode::kLayeredFill);  // the layered modes stay refused
  check(!heightmap.buildHeightmap(reference) && heightmap.lastStatus() == OHMHIP_ERR_UNSUPPORTED, kUnexpected);
  heightmap.setMode(ohm::HeightmapMode::kSimpleFill);
  check(heightmap.buildHeightmap(reference), kFailedCall);
  uint64_t types[2] = { 0, 0 };
  const ohmhip_heightmap_extents &e = heightmap.extents();
  const int axis_a = heightmap.surfaceAxisIndexA(), axis_b = heightmap.surfaceAxisIndexB();
  const long region_size = long(ohm::Heightmap::kDefaultRegionSize);
  for (uint32_t cb = 0; cb < e.mb; ++cb)
  {
    for (uint32_t ca = 0; ca < e.ma; ++ca)
    {
      ohm::Key key{};
      const long ga = long(e.first_region[0]) * region_size + e.first_local[0] + long(ca);
      const long gb = long(e.first_region[1]) * region_size + e.first_local[1] + long(cb);
      key.region[axis_a] = int16_t(ga >= 0 ? ga / region_size : -((-ga + region_size - 1) / region_size));
      key.local[axis_a] = uint8_t(ga - long(key.region[axis_a]) * region_size);
      key.region[axis_b] = int16_t(gb >= 0 ? gb / region_size : -((-gb + region_size - 1) / region_size));
      key.local[axis_b] = uint8_t(gb - long(key.region[axis_b]) * region_size);
      ohm::dvec3 pos{};
      const ohm::HeightmapVoxelType type = heightmap.getHeightmapVoxelInfo(key, &pos);
      types[0] += type == ohm::HeightmapVoxelType::kSurface;
      types[1] += type == ohm::HeightmapVoxelType::kVirtualSurface;
    }
  }
  OutFile out(args.output);
  out.value(uint32_t(heightmap.heightmapCellsA()));
  out.value(uint32_t(heightmap.heightmapCellsB()));
  out.value(heightmap.fillStats());
  out.value(types);
  out.array(heightmap.occupancy());
  out.array(heightmap.heightmapVoxels());
  out.array(heightmap.sourceVisits());
  out.array(heightmap.visitLog());
  return kOk;
}

/// heightmaplayered: ohm::LayeredHeightmap over a map whose voxels are written directly; <rays.bin> is a scene file
/// (<batch_rays> is not used).  in: heightmapfill's header, then u32 mode (2, 3) and u32 virtual-surface filter
/// threshold before the u64 region count and the regions.  out: u32 ma, u32 mb, u32 slots, u32 0, the
/// ohmhip_heightmap_layered_stats, u64 surface and u64 virtual voxels as getHeightmapVoxelInfo names them over every
/// slot, then the occupancy, HeightmapVoxel and source visit planes, the layer counts and the log.
int modeHeightmapLayered(const Args &args)
{
  InFile in(args.input);
  const std::vector<int32_t> dims = in.array<int32_t>(3);
  const std::vector<double> numbers = in.array<double>(6);
  const int32_t up_axis = in.value<int32_t>();
  const uint32_t flags = in.value<uint32_t>();
  const uint32_t mode = in.value<uint32_t>();
  const uint32_t threshold = in.value<uint32_t>();
  const uint64_t regions = in.value<uint64_t>();
  ohm::OccupancyMap source_map(args.resolution, dims[0], dims[1], dims[2]);
  for (uint64_t i = 0; i < regions; ++i)
  {
    const auto key = in.value<std::array<int16_t, 3>>();
    std::vector<uint8_t> &block = source_map.region(key).voxel_blocks[OHMHIP_LID_OCCUPANCY];
    block.resize(sizeof(float) * source_map.regionVoxelVolume());
    in.bytes(block.data(), block.size());
  }
  ohm::GpuMap gpu_map(&source_map, true);
  gpu_map.uploadRegions(nullptr, 0);
  ohm::LayeredHeightmap layered(args.resolution, numbers[5], ohm::UpAxis(up_axis));
  check(layered.mode() == ohm::HeightmapMode::kLayeredFill, kUnexpected);
  layered.setMode(ohm::HeightmapMode(mode));
  layered.setVirtualSurfaceFilterThreshold(threshold);
  ohm::Heightmap &heightmap = layered;  // built through the base class
  heightmap.setOccupancyMap(&gpu_map);
  heightmap.setFloor(numbers[3]);
  heightmap.setCeiling(numbers[4]);
  heightmap.setGenerateVirtualSurface((flags & 1u) != 0);
  heightmap.setPromoteVirtualBelow((flags & 2u) != 0);
  heightmap.setKeepVisitLog(true);
  const ohm::dvec3 reference{ numbers[0], numbers[1], numbers[2] };
  check(heightmap.buildHeightmap(reference), kFailedCall);
  uint64_t types[2] = { 0, 0 };
  const ohmhip_heightmap_extents &e = heightmap.extents();
  const int axis_a = heightmap.surfaceAxisIndexA(), axis_b = heightmap.surfaceAxisIndexB();
  const long region_size = long(ohm::Heightmap::kDefaultRegionSize);
  for (uint32_t slot = 0; slot <= layered.layerSlots(); ++slot)  // one past the last plane: kUnknown
  {
    for (uint32_t cb = 0; cb < e.mb; ++cb)
    {
      for (uint32_t ca = 0; ca < e.ma; ++ca)
      {
        ohm::Key key{};
        const long ga = long(e.first_region[0]) * region_size + e.first_local[0] + long(ca);
        const long gb = long(e.first_region[1]) * region_size + e.first_local[1] + long(cb);
        key.region[axis_a] = int16_t(ga >= 0 ? ga / region_size : -((-ga + region_size - 1) / region_size));
        key.local[axis_a] = uint8_t(ga - long(key.region[axis_a]) * region_size);
        key.region[axis_b] = int16_t(gb >= 0 ? gb / region_size : -((-gb + region_size - 1) / region_size));
        key.local[axis_b] = uint8_t(gb - long(key.region[axis_b]) * region_size);
        key.region[heightmap.upAxisIndex()] = int16_t(slot);
        ohm::dvec3 pos{};
        const ohm::HeightmapVoxelType type = heightmap.getHeightmapVoxelInfo(key, &pos);
        check(slot < layered.layerSlots() || type == ohm::HeightmapVoxelType::kUnknown, kUnexpected);
        types[0] += type == ohm::HeightmapVoxelType::kSurface;
        types[1] += type == ohm::HeightmapVoxelType::kVirtualSurface;
      }
    }
  }
  OutFile out(args.output);
  out.value(uint32_t(heightmap.heightmapCellsA()));
  out.value(uint32_t(heightmap.heightmapCellsB()));
  out.value(uint32_t(layered.layerSlots()));
  out.value(uint32_t(0));
  out.value(layered.layeredStats());
  out.value(types);
  out.array(heightmap.occupancy());
  out.array(heightmap.heightmapVoxels());
  out.array(heightmap.sourceVisits());
  out.array(layered.layerCounts());
  out.array(heightmap.visitLog());
  return kOk;
}

/// heightmap [min clearance] [flags: bit 0 turns virtual surfaces on]: ohm::Heightmap over a map with occupancy + mean.
/// Reference position (0, 0, 0), +Z up, grid resolution = the map's.  out: u32 ma, u32 mb, u64 populated, u64 cells, u8
/// has mean, then the occupancy, HeightmapVoxel and (if any) VoxelMean arrays.
int modeHeightmap(const Args &args)
{
  BuiltMap built(args, true);
  ohm::Heightmap heightmap(args.resolution, args.real(0, 0.0), ohm::UpAxis::kZ);
  heightmap.setOccupancyMap(&built.gpu);
  heightmap.setGenerateVirtualSurface((args.integer(1, 0) & 1) != 0);
  check(heightmap.buildHeightmap(ohm::dvec3{ 0.0, 0.0, 0.0 }), kFailedCall);
  OutFile out(args.output);
  out.value(uint32_t(heightmap.heightmapCellsA()));
  out.value(uint32_t(heightmap.heightmapCellsB()));
  out.value(uint64_t(heightmap.populatedCount()));
  out.value(uint64_t(heightmap.cellCount()));
  out.value(uint8_t(heightmap.voxelMeans().empty() ? 0 : 1));
  out.array(heightmap.occupancy());
  out.array(heightmap.heightmapVoxels());
  out.array(heightmap.voxelMeans());
  return kOk;
}

/// cloud [export free: != 0]: ohm::extractCloud over a map with occupancy + mean.  out: u64 count, u64 points, then the
/// positions (3 f64 each), the keys (10-byte records) and the values (f32).
int modeCloud(const Args &args)
{
  BuiltMap built(args, true);
  ohm::CloudOptions options;
  options.export_free = args.real(0, 0.0) != 0.0;
  const ohm::VoxelCloud cloud = ohm::extractCloud(built.gpu, options);
  check(cloud.status == OHMHIP_OK, kFailedCall);
  OutFile out(args.output);
  out.value(cloud.count);
  out.value(uint64_t(cloud.positions.size()));
  out.array(cloud.positions);
  out.array(cloud.keys);
  out.array(cloud.values);
  return kOk;
}

/// The query points of `neighbours` and `voxels`: the end points of every 97th ray.
std::vector<ohm::dvec3> everyNinetySeventhEnd(const std::vector<ohm::dvec3> &rays)
{
  std::vector<ohm::dvec3> points;
  for (size_t i = 1; i < rays.size(); i += 2 * 97)
  {
    points.push_back(rays[i]);
  }
  return points;
}

/// neighbours [search radius: 0.25] [query flags]: GpuMap::nearestNeighbours over a map with occupancy + mean.  out: u64
/// queries, u64 results, the counts (u64 each), the keys (10-byte records), the ranges (f32), then what an
/// ohm::NearestNeighbours object reports for the first point: u64 results, per result key, f64 range.
int modeNeighbours(const Args &args)
{
  BuiltMap built(args, true);
  const std::vector<ohm::dvec3> points = everyNinetySeventhEnd(built.rays);
  const float radius = float(args.real(0, 0.25));
  const unsigned flags = unsigned(args.has(1) ? std::atoi(args.extra[1]) : 0);
  std::vector<uint64_t> counts;
  std::vector<ohm::CloudKey> keys;
  std::vector<float> ranges;
  check(built.gpu.nearestNeighbours(points.data(), points.size(), radius, flags, counts, keys, ranges) == OHMHIP_OK,
        kFailedCall);
  ohm::NearestNeighbours query(built.gpu, points.empty() ? ohm::dvec3{ 0, 0, 0 } : points[0], radius, flags);
  check(query.execute(), kFailedCall);
  OutFile out(args.output);
  out.value(uint64_t(points.size()));
  out.value(uint64_t(keys.size()));
  out.array(counts);
  out.array(keys);
  out.array(ranges);
  out.value(uint64_t(query.numberOfResults()));
  for (size_t i = 0; i < query.numberOfResults(); ++i)
  {
    out.key(query.intersectedVoxels()[i]);
    out.value(query.ranges()[i]);
  }
  return kOk;
}

/// voxels: GpuMap::voxelKeys, readVoxels and occupancyTypes over a map with occupancy + mean.  out: u64 keys, the keys
/// (10-byte records), the occupancy values (f32), the mean voxels (8 bytes each), present (u8 each), the occupancy types
/// (i8 each).
int modeVoxels(const Args &args)
{
  BuiltMap built(args, true);
  const std::vector<ohm::dvec3> points = everyNinetySeventhEnd(built.rays);
  const std::vector<ohm::CloudKey> keys = built.gpu.voxelKeys(points.data(), points.size());
  std::vector<uint8_t> occupancy, mean, present, present_mean;
  check(built.gpu.lastStatus() == OHMHIP_OK &&
          built.gpu.readVoxels(OHMHIP_LID_OCCUPANCY, keys, occupancy, present) == OHMHIP_OK &&
          built.gpu.readVoxels(OHMHIP_LID_MEAN, keys, mean, present_mean) == OHMHIP_OK && present == present_mean,
        kFailedCall);
  OutFile out(args.output);
  out.value(uint64_t(points.size()));
  out.array(keys);
  out.array(occupancy);
  out.array(mean);
  out.array(present);
  out.array(built.gpu.occupancyTypes(keys));
  return kOk;
}

/// covariance: the covariance calls of the mirror over a GpuNdtMap (occupancy + mean + covariance) built from the rays
/// in batches.  The keys are those of every 97th ray's end point, then a key of a region the map does not hold and a
/// null key.  out: u64 keys, the keys (10-byte records), the covariance voxels readVoxels gives for them (6 f32 each);
/// of covarianceEigenDecomposition the eigenvalues (3 f64 each), eigenvectors (9 f64 each) and status (u8 each); of
/// covarianceEstimatePrimaryNormal the normals (3 f64 each); of covarianceUnitSphereTransformation the rotations (x, y, z, w f64 each) and scales (3 f64 each); then what a
/// CovarianceEllipsoids query reports: u64 results, positions (3 f64 each), axes (9 f64 each), scales (3 f64 each),
/// keys (10-byte records), values (f32 each); then a planar heightmap with surface normals and virtual surfaces on,
/// reference position (0, 0, 0), +Z up: u32 ma, u32 mb, the occupancy and HeightmapVoxel arrays.
int modeCovariance(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map = hostMap(args.resolution, true);
  ohm::GpuNdtMap gpu(&map, true);
  check(gpu.gpuOk(), kMapInvalid);
  check(integrateInBatches(gpu, rays, args.batch_rays) == (rays.size() & ~size_t(1)), kFailedCall);
  const std::vector<ohm::dvec3> points = everyNinetySeventhEnd(rays);
  std::vector<ohm::Key> keys = gpu.voxelKeys(points.data(), points.size());
  check(gpu.lastStatus() == OHMHIP_OK, kFailedCall);
  ohm::Key absent{};
  absent.region[0] = absent.region[1] = absent.region[2] = 300;
  keys.push_back(absent);
  ohm::Key null_key{};
  null_key.region[0] = null_key.region[1] = null_key.region[2] = int16_t(-32768);
  keys.push_back(null_key);
  std::vector<uint8_t> covariance, present;
  check(gpu.readVoxels(OHMHIP_LID_COVARIANCE, keys, covariance, present) == OHMHIP_OK, kFailedCall);
  const ohm::CovarianceEigen eigen = ohm::covarianceEigenDecomposition(gpu, keys);
  std::vector<ohm::dvec3> normals, scales;
  std::vector<ohm::dquat> rotations;
  std::vector<uint8_t> normal_status, sphere_status;
  check(eigen.call_status == OHMHIP_OK &&
          ohm::covarianceEstimatePrimaryNormal(gpu, keys, normals, &normal_status) == OHMHIP_OK &&
          ohm::covarianceUnitSphereTransformation(gpu, keys, rotations, scales, &sphere_status) == OHMHIP_OK &&
          normal_status == eigen.status && sphere_status == eigen.status,
        kFailedCall);
  ohm::CovarianceEllipsoids ellipsoids(gpu);
  check(ellipsoids.execute() && ellipsoids.lastStatus() == OHMHIP_OK, kFailedCall);
  ohm::Heightmap heightmap(args.resolution, 0.0, ohm::UpAxis::kZ);
  heightmap.setOccupancyMap(&gpu);
  heightmap.setGenerateVirtualSurface(true);
  check(!heightmap.surfaceNormals(), kUnexpected);
  heightmap.setSurfaceNormals(true);
  check(heightmap.buildHeightmap(ohm::dvec3{ 0.0, 0.0, 0.0 }), kFailedCall);
  OutFile out(args.output);
  out.value(uint64_t(keys.size()));
  out.array(keys);
  out.array(covariance);
  out.array(eigen.eigenvalues);
  out.array(eigen.eigenvectors);
  out.array(eigen.status);
  out.array(normals);
  out.array(rotations);
  out.array(scales);
  out.value(uint64_t(ellipsoids.numberOfResults()));
  out.array(ellipsoids.positions());
  out.array(ellipsoids.axes());
  out.array(ellipsoids.scales());
  out.bytes(ellipsoids.intersectedVoxels(), ellipsoids.numberOfResults() * sizeof(ohm::Key));
  out.array(ellipsoids.values());
  out.value(uint32_t(heightmap.heightmapCellsA()));
  out.value(uint32_t(heightmap.heightmapCellsB()));
  out.array(heightmap.occupancy());
  out.array(heightmap.heightmapVoxels());
  return kOk;
}

/// filter [tolerance: -1] [occupancy only] [offset: 0.35]: GpuMap::filterPoints over a map with occupancy + mean; the
/// points are every ray's end point and, displaced by offset along x, the same again.  out: u64 points, u64 kept, the
/// status (u8 each), the kept indices (u64 each), the values (f64 each), the keys (10-byte records).
int modeFilterPoints(const Args &args)
{
  BuiltMap built(args, true);
  const double offset = args.real(2, 0.35);
  std::vector<ohm::dvec3> points;
  for (int pass = 0; pass < 2; ++pass)
  {
    for (size_t i = 1; i < built.rays.size(); i += 2)
    {
      ohm::dvec3 p = built.rays[i];
      p.x += pass * offset;
      points.push_back(p);
    }
  }
  std::vector<uint8_t> status;
  std::vector<uint64_t> kept;
  std::vector<double> values;
  std::vector<ohm::CloudKey> keys;
  check(built.gpu.filterPoints(points.data(), points.size(), args.real(0, -1.0), args.integer(1, 0) != 0, status, kept,
                               values, keys) == OHMHIP_OK,
        kFailedCall);
  OutFile out(args.output);
  out.value(uint64_t(points.size()));
  out.value(uint64_t(kept.size()));
  out.array(status);
  out.array(kept);
  out.array(values);
  out.array(keys);
  return kOk;
}

/// voxeledit <ops file>: voxel edits by key.  <rays.bin> holds the points of an edit script, the ops file one op byte
/// per point (1 HIT, 2 MISS, 3 HIT_SAMPLE); <batch_rays> is not used.  On an occupancy + mean map:
/// GpuMap::integrateVoxels of the script; then the single-voxel conveniences on the first point -- integrateHit(sample),
/// integrateMiss(key), integrateHit(key) --; then integrateMisses(keyRange(p, q)) with p and q the script's last two
/// points.  out: the map dump, then the five counters of lastEditStats() after the script (u64 each), u64 range keys
/// and the keys of keyRange (10-byte records).
int modeVoxelEdit(const Args &args)
{
  const std::vector<ohm::dvec3> points = readRays(args.input);
  check(args.has(0) && points.size() >= 2, kUsage);
  const std::vector<ohm::GpuMap::VoxelEdit> ops = InFile(args.extra[0]).array<ohm::GpuMap::VoxelEdit>(points.size());
  ResidentMap edit(args.resolution, true);
  check(edit.gpu.integrateVoxels(ops.data(), ohm::GpuMap::VoxelEdit::kHit, nullptr, points.data(), points.size()) ==
          OHMHIP_OK,
        kFailedCall);
  const ohmhip_voxel_edit_stats script_stats = edit.gpu.lastEditStats();
  const std::vector<ohm::CloudKey> first = edit.gpu.voxelKeys(points.data(), 1);
  check(edit.gpu.lastStatus() == OHMHIP_OK && edit.gpu.integrateHit(points[0]) == OHMHIP_OK &&
          edit.gpu.integrateMiss(first[0]) == OHMHIP_OK && edit.gpu.integrateHit(first[0]) == OHMHIP_OK,
        kFailedCall);
  const std::vector<ohm::CloudKey> range = edit.gpu.keyRange(points[points.size() - 2], points[points.size() - 1]);
  check(edit.gpu.lastStatus() == OHMHIP_OK && edit.gpu.integrateMisses(range) == OHMHIP_OK, kFailedCall);
  edit.gpu.syncVoxels();
  OutFile out(args.output);
  writeRegionDump(out, edit.map);
  const uint64_t counters[6] = { script_stats.applied,         script_stats.null_keys,       script_stats.distinct_voxels,
                                 script_stats.regions_touched, script_stats.regions_created, range.size() };
  out.value(counters);
  out.array(range);
  return kOk;
}

/// copy [box minimum: 0] [box maximum on every axis: 4.5]: Copy.CopySubmapFromGpu (tests/ohmtestgpu/GpuCopyTests.cpp:
/// 112-150): the rays into a GpuMap, then -- without a sync of the source -- ohm::copyMap into a second map with
/// copyFilterExtents, and a clone() of the same box.  out: the map dumps of the source, the copy and the clone.
/// Prints "copied <n> of <regions> regions, <bytes> bytes".
int modeCopy(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ResidentMap src(args.resolution, false), dst(args.resolution, false), again(args.resolution, false);
  check(ohm::canCopy(dst.gpu, src.gpu) && !ohm::canCopy(src.gpu, src.gpu), kFailedCall);
  check(integrateInBatches(src.gpu, rays, args.batch_rays) == (rays.size() & ~size_t(1)), kUnexpected);
  const double box_min = args.real(0, 0.0), box_max = args.real(1, 4.5);
  const ohm::dvec3 copy_min{ box_min, box_min, box_min }, copy_max{ box_max, box_max, box_max };
  const ohm::CopyChunkFilter box = ohm::copyFilterExtents(copy_min, copy_max);
  ohmhip_copy_stats stats, again_stats;
  check(ohm::copyMap(dst.gpu, src.gpu, box, {}, &stats) && stats.regions_passed == stats.regions_created &&
          stats.layers_copied == OHMHIP_LAYER_BIT(OHMHIP_LID_OCCUPANCY),
        kFailedCall);
  // the same box by a host lambda (the keys go down), a filter that passes nothing, and every layer filtered out
  check(ohm::copyMap(again.gpu, src.gpu, [&box](const ohm::CopyChunk &chunk) { return box(chunk); }, {}, &again_stats) &&
          again_stats.regions_passed == stats.regions_passed && again_stats.bytes_copied == stats.bytes_copied &&
          ohm::copyMap(again.gpu, src.gpu, ohm::copyFilterNegate(ohm::CopyChunkFilter())) &&
          ohm::copyMap(again.gpu, src.gpu, {}, ohm::copyFilterNegate(ohm::copyLayersFilter({ "occupancy" }))),
        kFailedCall);
  const std::unique_ptr<ohm::GpuMap> clone = src.gpu.clone(copy_min, copy_max);
  check(clone != nullptr, kFailedCall);
  src.gpu.syncVoxels();
  dst.gpu.syncVoxels();
  clone->syncVoxels();
  std::printf("copied %llu of %zu regions, %llu bytes\n", (unsigned long long)stats.regions_passed, src.map.regionCount(),
              (unsigned long long)stats.bytes_copied);
  OutFile out(args.output);
  writeRegionDump(out, src.map);
  writeRegionDump(out, dst.map);
  writeRegionDump(out, clone->map());
  return kOk;
}

/// compare: ohm::compare::compareVoxels between two GpuMaps: every ray but the last into the reference map, every ray
/// into the evaluated one.  out: three comparisons of the occupancy layer -- kContinue, stop-at-first, kContinue with
/// ohmcmp's tolerance --, each as: the ohmhip_compare_result, u64 listed mismatches + their 10-byte records, u64 listed
/// missing regions + their i16[3] keys, u64 messages logged.  Prints "compare flags <f>: passed <n> failed <n>" for each.
int modeCompare(const Args &args)
{
  namespace cmp = ohm::compare;
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ResidentMap ref(args.resolution, false), eval(args.resolution, false);
  check(rays.size() >= 4 && ref.gpu.integrateRays(rays.data(), rays.size() - 2) == rays.size() - 2 &&
          eval.gpu.integrateRays(rays.data(), rays.size()) == rays.size(),
        kUnexpected);
  check(cmp::compareLayoutLayer(eval.gpu, ref.gpu, "occupancy") && !cmp::compareLayoutLayer(eval.gpu, ref.gpu, "mean") &&
          !cmp::compareVoxels(eval.gpu, ref.gpu, "mean").layout_match && cmp::compareVoxels(ref.gpu, ref.gpu, "occupancy"),
        kFailedCall);
  // ohmcmp's occupancy tolerance: it forgives one more ray where both maps had observed the voxel
  cmp::Tolerance loose("occupancy");
  cmp::configureTolerance(loose, "occupancy", 1e2f);
  cmp::configureTolerance(loose, "count", uint32_t(1));  // (a name the layer lacks is ignored)
  OutFile out(args.output);
  for (int pass = 0; pass < 3; ++pass)
  {
    const unsigned flags = (pass == 1) ? unsigned(cmp::kZero) : unsigned(cmp::kContinue);
    uint64_t logged = 0;
    const cmp::VoxelsResult res = cmp::compareVoxels(eval.gpu, ref.gpu, "occupancy", pass == 2 ? &loose : nullptr, flags,
                                                     [&logged](cmp::Severity severity, const std::string &) {
                                                       logged += severity == cmp::Severity::kError ? 1u : 0u;
                                                     });
    check(res.status == OHMHIP_OK && !(pass < 2 && bool(res)), kFailedCall);
    out.value(res.detail);
    out.value(uint64_t(res.mismatches.size()));
    out.array(res.mismatches);
    out.value(uint64_t(res.missing_regions.size()));
    out.array(res.missing_regions);
    out.value(logged);
    std::printf("compare flags %u: passed %zu failed %zu\n", flags, res.voxels_passed, res.voxels_failed);
  }
  return kOk;
}

/// linekeys: ohm::LineKeysQueryGpu over the rays.  out: u64 rays, then per ray u64 index, u64 count, and after them all
/// keys in intersectedVoxels() order.
int modeLineKeys(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ResidentMap resident(args.resolution, false);
  ohm::LineKeysQueryGpu query(resident.gpu);
  query.setRays(rays.data(), rays.size());
  check(query.executeAsync() && query.wait() && query.numberOfResults() == rays.size() / 2, kFailedCall);
  OutFile out(args.output);
  const uint64_t n = query.numberOfResults();
  out.value(n);
  uint64_t total_keys = 0;
  for (uint64_t i = 0; i < n; ++i)
  {
    const uint64_t index = query.resultIndices()[i], count = query.resultCounts()[i];
    out.value(index);
    out.value(count);
    total_keys = index + count;
  }
  for (uint64_t k = 0; k < total_keys; ++k)
  {
    out.key(query.intersectedVoxels()[k]);
  }
  return kOk;
}

/// raysquery: ohm::RaysQueryGpu: the first half of the rays builds the map (ohm::GpuMap::integrateRays), the second
/// half is the query (addRay / executeAsync / wait).  out: u64 rays, then per ray f64 range, f64 unobserved volume, i32
/// terminal type, key.
int modeRaysQuery(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ResidentMap resident(args.resolution, false);
  const size_t build_points = (rays.size() / 2) & ~size_t(1);
  check(!build_points || resident.gpu.integrateRays(rays.data(), build_points) == build_points, kFailedCall);
  ohm::RaysQueryGpu query(resident.gpu);
  for (size_t i = build_points; i + 1 < rays.size(); i += 2)
  {
    query.addRay(rays[i], rays[i + 1]);
  }
  check((query.queryFlags() & ohm::kQfGpuEvaluate) && query.executeAsync() && query.wait() &&
          query.numberOfResults() == query.numberOfRays(),
        kFailedCall);
  OutFile out(args.output);
  const uint64_t n = query.numberOfResults();
  out.value(n);
  for (uint64_t i = 0; i < n; ++i)
  {
    out.value(query.ranges()[i]);
    out.value(query.unobservedVolumes()[i]);
    out.value(int32_t(query.terminalOccupancyTypes()[i]));
    out.key(query.intersectedVoxels()[i]);
  }
  return kOk;
}

/// Per region in ascending key order: i16[3] key and the region's voxels as f32, after a u64 count.
void writeClearanceBlocks(OutFile &out, std::vector<std::array<int16_t, 3>> keys, size_t voxels,
                          const std::function<const void *(const std::array<int16_t, 3> &)> &block_of)
{
  std::sort(keys.begin(), keys.end());
  out.value(uint64_t(keys.size()));
  for (const auto &key : keys)
  {
    const void *block = block_of(key);
    check(block != nullptr, kFailedCall);
    out.value(key);
    out.bytes(block, voxels * sizeof(float));
  }
}

/// clearance [search radius: 0.5] [query flags: 0]: every ray builds the map; ohm::ClearanceProcess over the extents of
/// all the rays' points.  out: the clearance blocks (writeClearanceBlocks) of every region of the map.
int modeClearance(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ResidentMap resident(args.resolution, false);
  const size_t build_points = rays.size() & ~size_t(1);
  check(!build_points || resident.gpu.integrateRays(rays.data(), build_points) == build_points, kFailedCall);
  ohm::dvec3 lo = rays[0], hi = rays[0];
  for (size_t i = 1; i < build_points; ++i)
  {
    lo = ohm::dvec3{ std::min(lo.x, rays[i].x), std::min(lo.y, rays[i].y), std::min(lo.z, rays[i].z) };
    hi = ohm::dvec3{ std::max(hi.x, rays[i].x), std::max(hi.y, rays[i].y), std::max(hi.z, rays[i].z) };
  }
  ohm::ClearanceProcess clearance(float(args.real(0, 0.5)), unsigned(args.integer(1, 0)) | ohm::kQfGpuEvaluate);
  check(clearance.calculateForExtents(resident.gpu, lo, hi), kFailedCall);
  std::vector<std::array<int16_t, 3>> keys;
  check(ohm::fetchRegions(resident.gpu.handle(), false, keys) == OHMHIP_OK, kFailedCall);
  OutFile out(args.output);
  writeClearanceBlocks(out, keys, resident.map.regionVoxelVolume(),
                       [&](const std::array<int16_t, 3> &key) { return clearance.regionClearance(key); });
  return kOk;
}

/// clearanceupdate [search radius: 0.5] [query flags: 0] [region budget of the updates between batches: 2] [region
/// dimension: 32]: ohm::Mapper with an ohm::ClearanceProcess: batches of <batch_rays> rays, a budgeted update after
/// each, a full update at the end.  out: the clearance layer (writeClearanceBlocks) of every region of the host map.
int modeClearanceUpdate(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  const size_t budget = size_t(args.integer(2, 2));
  ohm::OccupancyMap update_map = hostMap(args.resolution, false, int(args.integer(3, 32)));
  ohm::ClearanceProcess::ensureClearanceLayer(update_map);
  ohm::GpuMap update_gpu_map(&update_map, true);
  ohm::Mapper mapper(&update_gpu_map);
  mapper.addProcess(new ohm::ClearanceProcess(float(args.real(0, 0.5)), unsigned(args.integer(1, 0)) | ohm::kQfGpuEvaluate));
  bool updates_ok = true;
  const size_t done = integrateInBatches(update_gpu_map, rays, std::max<size_t>(1, args.batch_rays),
                                         [&] { updates_ok = updates_ok && mapper.update(1e-9, budget) >= 0; });
  check(done == (rays.size() & ~size_t(1)) && updates_ok && mapper.update(0.0) == ohm::kMprUpToDate, kFailedCall);
  update_gpu_map.syncVoxels();
  std::vector<std::array<int16_t, 3>> keys;
  for (const auto &entry : update_map.chunks())
  {
    keys.push_back(entry.first);
  }
  OutFile out(args.output);
  writeClearanceBlocks(out, keys, update_map.regionVoxelVolume(), [&](const std::array<int16_t, 3> &key) {
    return update_map.chunks().find(key)->second.voxel_blocks[OHMHIP_LID_CLEARANCE].data();
  });
  return kOk;
}

/// linequery [search radius: 0.5] [query flags: 0]: the last <batch_rays> rays are query lines, each an
/// ohm::LineQueryGpu; the rays before them build the map.  out: u64 lines, then per line u32 results and per result
/// key, f32 range.
int modeLineQuery(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ResidentMap resident(args.resolution, false);
  const size_t query_points = std::min(2 * args.batch_rays, rays.size() & ~size_t(1));
  const size_t build_points = (rays.size() & ~size_t(1)) - query_points;
  check(!build_points || resident.gpu.integrateRays(rays.data(), build_points) == build_points, kFailedCall);
  const float radius = float(args.real(0, 0.5));
  const unsigned flags = unsigned(args.integer(1, 0));
  OutFile out(args.output);
  out.value(uint64_t((rays.size() - build_points) / 2));
  for (size_t i = build_points; i + 1 < rays.size(); i += 2)
  {
    ohm::LineQueryGpu query(resident.gpu, rays[i], rays[i + 1], radius, flags);
    check((query.queryFlags() & ohm::kQfGpuEvaluate) && query.executeAsync() && query.wait(), kFailedCall);
    const uint32_t n = uint32_t(query.numberOfResults());
    out.value(n);
    for (uint32_t k = 0; k < n; ++k)
    {
      out.key(query.intersectedVoxels()[k]);
      out.value(query.ranges()[k]);
    }
  }
  return kOk;
}

/// The ohm::Query surface of one query, as u32 each: queryFlags() as constructed (with flags 0) and after
/// setQueryFlags(0); execute(), executeAsync(), wait(); numberOfResults() after the execute(), after reset(false),
/// after another execute() and after reset(true).
template <typename Q>
void recordQuerySurface(Q &query, std::vector<uint32_t> &rec)
{
  rec.push_back(query.queryFlags());
  query.setQueryFlags(0);
  rec.push_back(query.queryFlags());
  rec.push_back(query.execute());
  const uint32_t n = uint32_t(query.numberOfResults());
  rec.push_back(query.executeAsync());
  rec.push_back(query.wait());
  rec.push_back(n);
  query.reset(false);
  rec.push_back(uint32_t(query.numberOfResults()));
  query.execute();
  rec.push_back(uint32_t(query.numberOfResults()));
  query.reset(true);
  rec.push_back(uint32_t(query.numberOfResults()));
}

/// queryapi: what the four queries share and where they differ.  The rays build the map in one call and are the rays of
/// LineKeysQueryGpu and RaysQueryGpu; LineQueryGpu runs from the first point 4 voxels along x (radius 2 voxels),
/// NearestNeighbours at the second point (radius 2.5 voxels).  out, all u32: recordQuerySurface of LineKeysQueryGpu,
/// RaysQueryGpu, LineQueryGpu, NearestNeighbours; then RaysQueryGpu::numberOfRays() after reset(false) and after
/// reset(true), LineKeysQueryGpu::rayPointCount() after reset(true), LineKeysQueryGpu::ranges() == nullptr, and
/// execute() of LineKeysQueryGpu and of RaysQueryGpu without a map.
int modeQueryApi(const Args &args)
{
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  check(rays.size() >= 2, kUsage);
  ResidentMap resident(args.resolution, false);
  const size_t points = rays.size() & ~size_t(1);
  check(resident.gpu.integrateRays(rays.data(), points) == points, kFailedCall);
  std::vector<uint32_t> rec;
  ohm::LineKeysQueryGpu line_keys(resident.gpu, 0);
  line_keys.setRays(rays.data(), points);
  recordQuerySurface(line_keys, rec);
  ohm::RaysQueryGpu rays_query(resident.gpu, 0);
  rays_query.setRays(rays.data(), points);
  recordQuerySurface(rays_query, rec);
  const uint32_t rays_after_hard = uint32_t(rays_query.numberOfRays());
  rays_query.setRays(rays.data(), points);
  rays_query.reset(false);
  const uint32_t rays_after_soft = uint32_t(rays_query.numberOfRays());
  const ohm::dvec3 line_end{ rays[0].x + 4 * args.resolution, rays[0].y, rays[0].z };
  ohm::LineQueryGpu line_query(resident.gpu, rays[0], line_end, float(2 * args.resolution), 0);
  recordQuerySurface(line_query, rec);
  ohm::NearestNeighbours neighbours(resident.gpu, rays[1], float(2.5 * args.resolution), 0);
  recordQuerySurface(neighbours, rec);
  rec.push_back(rays_after_soft);
  rec.push_back(rays_after_hard);
  rec.push_back(uint32_t(line_keys.rayPointCount()));
  rec.push_back(line_keys.ranges() == nullptr);
  line_keys.setGpuMap(nullptr);
  rec.push_back(line_keys.execute());
  rays_query.setGpuMap(nullptr);
  rec.push_back(rays_query.execute());
  OutFile out(args.output);
  out.array(rec);
  return kOk;
}

/// layout toggle <mean pattern>: VoxelMean.LayoutToggle (tests/ohmtestgpu/GpuVoxelMeanTests.cpp:143-244) on a map of
/// 32^3 regions: integrateHit at (1.1, 1.1, 1.1); addVoxelMeanLayer; the mean voxel written as {pattern, 1};
/// updateLayout back to the first layout.  out, per stage (created, mean added, mean written, layout restored): u32
/// host layers, u32 device layers (ohmhip_map_layers), f32 occupancy of the voxel, u64 cloud points, f64[3] position of
/// the first; then u32[2] the mean voxel as added, i32 the status of reading it once the layer is gone.
/// layout added: the first <batch_rays> rays, stamped 100 + 0.01 i, into an occupancy map of 16^3 regions; the mean,
/// traversal, touch-time and incident-normal layers added; the other rays, stamped 200 + 0.01 i; syncVoxels.  out: a
/// map dump.
int modeLayout(const Args &args)
{
  check(args.has(0), kUsage);
  const std::string which = args.extra[0];
  OutFile out(args.output);
  if (which == "toggle")
  {
    ohm::OccupancyMap map(args.resolution, 32, 32, 32);
    ohm::GpuMap gpu(&map, true);
    check(gpu.gpuOk(), kMapInvalid);
    const unsigned cached_layout = map.layers();
    const ohm::dvec3 sample{ 1.1, 1.1, 1.1 };
    check(gpu.integrateHit(sample) == OHMHIP_OK, kFailedCall);
    const std::vector<ohm::CloudKey> key = gpu.voxelKeys(&sample, 1);
    std::vector<uint8_t> value, present;
    auto stage = [&]() {
      unsigned device_layers = 0;
      check(ohmhip_map_layers(gpu.handle(), &device_layers) == OHMHIP_OK, kFailedCall);
      check(gpu.readVoxels(OHMHIP_LID_OCCUPANCY, key, value, present) == OHMHIP_OK && present[0] == 1, kFailedCall);
      const ohm::VoxelCloud cloud = ohm::extractCloud(gpu);
      check(cloud.status == OHMHIP_OK && !cloud.positions.empty(), kFailedCall);
      out.value(uint32_t(map.layers()));
      out.value(uint32_t(device_layers));
      out.bytes(value.data(), sizeof(float));
      out.value(uint64_t(cloud.count));
      out.value(cloud.positions[0]);
    };
    stage();
    gpu.addVoxelMeanLayer();
    check(gpu.voxelMeanEnabled(), kUnexpected);
    stage();
    std::vector<uint8_t> mean_added;
    check(gpu.readVoxels(OHMHIP_LID_MEAN, key, mean_added, present) == OHMHIP_OK && present[0] == 1, kFailedCall);
    const uint32_t mean[2] = { uint32_t(args.integer(1, 0)), 1u };
    check(gpu.writeVoxels(OHMHIP_LID_MEAN, key, mean) == OHMHIP_OK, kFailedCall);
    stage();
    gpu.updateLayout(cached_layout);
    check(!gpu.voxelMeanEnabled(), kUnexpected);
    stage();
    out.array(mean_added);
    std::vector<uint8_t> gone;
    out.value(int32_t(gpu.readVoxels(OHMHIP_LID_MEAN, key, gone, present)));
    return kOk;
  }
  check(which == "added", kUsage);
  const std::vector<ohm::dvec3> rays = readRays(args.input);
  ohm::OccupancyMap map(args.resolution, 16, 16, 16);
  ohm::GpuMap gpu(&map, true);
  check(gpu.gpuOk(), kMapInvalid);
  const size_t points = rays.size() & ~size_t(1);
  const size_t first = std::min(2 * args.batch_rays, points);
  auto integrate = [&](size_t begin, size_t end, double start) {
    std::vector<double> stamps((end - begin) / 2);
    for (size_t i = 0; i < stamps.size(); ++i)
    {
      stamps[i] = start + 0.01 * double(i);
    }
    check(end == begin || gpu.integrateRays(rays.data() + begin, end - begin, nullptr, stamps.data(), ohm::kRfDefault) ==
                            end - begin,
          kFailedCall);
  };
  integrate(0, first, 100.0);
  gpu.addVoxelMeanLayer();
  gpu.addTraversalLayer();
  gpu.addTouchTimeLayer();
  gpu.addIncidentNormalLayer();
  check(gpu.voxelMeanEnabled() && gpu.traversalEnabled() && gpu.touchTimeEnabled() && gpu.incidentNormalEnabled(),
        kUnexpected);
  integrate(first, points, 200.0);
  gpu.syncVoxels();
  writeRegionDump(out, map);
  return kOk;
}

struct Mode
{
  const char *name;
  int (*run)(const Args &);
  bool needs_device;
};

const Mode kModes[] = {
  { "occ", &modeIntegrate<ohm::GpuMap, false>, true },
  { "occmean", &modeIntegrate<ohm::GpuMap, true>, true },
  { "ndt", &modeIntegrate<ohm::GpuNdtMap, false>, true },
  { "tsdf", &modeIntegrate<ohm::GpuTsdfMap, false>, true },
  { "occdev", &modeDeviceRays, true },
  { "occcoalesce", &modeCoalesce, true },
  { "occowner", &modeOwner, true },
  { "occclipbox", &modeClipBox, true },
  { "occchain", &modeChain, true },
  { "occpart", &modePartition, true },
  { "occpartint", &modePartitionedIntegrator, true },
  { "transform", &modeTransform, true },
  { "clearing", &modeClearing, true },
  { "copy", &modeCopy, true },
  { "compare", &modeCompare, true },
  { "linekeys", &modeLineKeys, true },
  { "raysquery", &modeRaysQuery, true },
  { "linequery", &modeLineQuery, true },
  { "queryapi", &modeQueryApi, true },
  { "clearance", &modeClearance, true },
  { "clearanceupdate", &modeClearanceUpdate, true },
  { "heightmap", &modeHeightmap, true },
  { "heightmapfill", &modeHeightmapFill, true },
  { "heightmaplayered", &modeHeightmapLayered, true },
  { "cloud", &modeCloud, true },
  { "neighbours", &modeNeighbours, true },
  { "voxels", &modeVoxels, true },
  { "covariance", &modeCovariance, true },
  { "filter", &modeFilterPoints, true },
  { "voxeledit", &modeVoxelEdit, true },
  { "layout", &modeLayout, true },
  { "filter:clipbounded", &modeRayFilter, false },
  { "filter:cliptobounds", &modeRayFilter, false },
  { "filter:clipray", &modeRayFilter, false },
  { "filter:goodray", &modeRayFilter, false },
};
}  // namespace

int main(int argc, char **argv)
{
  const Mode *mode = nullptr;
  for (const Mode &m : kModes)
  {
    mode = (argc >= 6 && m.name == std::string(argv[1])) ? &m : mode;
  }
  if (!mode)
  {
    std::fprintf(stderr, "usage: %s <mode> <resolution> <batch_rays> <rays.bin | other input> <out.bin> [mode arguments]\n  modes:",
                 argv[0]);
    for (const Mode &m : kModes)
    {
      std::fprintf(stderr, " %s", m.name);
    }
    std::fprintf(stderr, "\n");
    return kUsage;
  }
  const Args args{ argv[1], std::atof(argv[2]), size_t(std::atoll(argv[3])), argv[4], argv[5], argc - 6, argv + 6 };
  try
  {
    if (mode->needs_device && ohm::configureGpu(0) != 0)
    {
      std::fprintf(stderr, "no HIP device\n");
      return kNoDevice;
    }
    return mode->run(args);
  }
  catch (const Failure &failure)
  {
    return failure.code;
  }
  catch (const gputil::ApiException &e)
  {
    std::fprintf(stderr, "gputil::ApiException: %s\n", e.what());
    return kApiException;
  }
}
