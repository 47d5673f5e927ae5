// gpumap_driver.cpp -- C++14 test driver for the host mirror (ohm::GpuMap / GpuNdtMap / GpuTsdfMap over the C ABI).
// Reads a binary ray file, integrates it in batches exactly like the reference's gpuMapTest() harness
// (tests/ohmtestgpu/GpuMapTest.cpp:68-205), syncs, and dumps every region layer for the Python parity test to check
// against the CPU oracle.  Links libohmhip.so only; built with plain g++ (no hipcc, no glm).
//
//   gpumap_driver <mode: occ|occmean|occdev|ndt|tsdf|linekeys|raysquery|clearance|clearanceupdate|linequery|heightmap|cloud|neighbours|voxels|filter|transform|...> <resolution> <batch_rays>
//                 <rays.bin> <out.bin> [search radius] [query flags]
//   occdev: the sample points (odd entries) go through ohm::GpuTransformSamples with a static identity trajectory and
//   are integrated straight from the device buffer (all rays then start at the origin).
//   transform: <rays.bin> is a trajectory-and-samples file instead and <out.bin> receives the ray buffer of
//   ohm::GpuTransformSamples::transform (layouts at the mode below); <resolution> and <batch_rays> are not used.
//   clearing: RayPattern.Clearing through ohm::ClearingPattern; <batch_rays> and <rays.bin> are not used, three more
//   arguments give the translation (layout at the mode below).
//   filter:<clipbounded|cliptobounds|clipray|goodray>: host only, one record per ray (layout at the mode below).
//   heightmapfill: <rays.bin> is a scene file (voxels written directly) and <out.bin> receives the flood-fill
//   heightmap of ohm::Heightmap in HeightmapMode::kSimpleFill (layouts at the mode below); <batch_rays> is not used.
//   rays.bin: u64 n_points, then n_points * 3 doubles.  out.bin: u64 regions, per region i16[3] key, then per enabled
//   layer (ascending id): u32 layer id, u64 bytes, payload.
#include "OhmGpuMap.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

int main(int argc, char **argv)
{
  if (argc < 6)
  {
    std::fprintf(stderr, "usage: %s <occ|occmean|occdev|occcoalesce|occowner|occclipbox|ndt|tsdf|transform|...> <resolution> <batch_rays> <rays.bin | transform input> <out.bin>\n", argv[0]);
    return 2;
  }
  const std::string mode = argv[1];
  const double resolution = std::atof(argv[2]);
  const size_t batch_rays = size_t(std::atoll(argv[3]));
  if (mode.compare(0, 7, "filter:") == 0)
  {
    // Host only (no device): run one of the stock ray filters of OhmGpuMap.h over the rays and write, per ray,
    // accepted (1 byte), filter flags (1 byte), start and end (6 doubles).  Box (-1,-1,-1)..(2,2,2), length = resolution.
    FILE *in = std::fopen(argv[4], "rb");
    if (!in)
    {
      return 4;
    }
    uint64_t n_points = 0;
    std::vector<ohm::dvec3> rays;
    bool read_ok = std::fread(&n_points, sizeof(n_points), 1, in) == 1;
    if (read_ok)
    {
      rays.resize(n_points);
      read_ok = std::fread(rays.data(), sizeof(ohm::dvec3), n_points, in) == n_points;
    }
    std::fclose(in);
    if (!read_ok)
    {
      return 4;
    }
    const ohm::Aabb box(ohm::dvec3{ -1.0, -1.0, -1.0 }, ohm::dvec3{ 2.0, 2.0, 2.0 });
    FILE *out = std::fopen(argv[5], "wb");
    if (!out)
    {
      return 4;
    }
    for (uint64_t i = 0; i + 1 < n_points; i += 2)
    {
      ohm::dvec3 start = rays[i], end = rays[i + 1];
      unsigned flags = 0;
      bool ok = false;
      if (mode == "filter:clipbounded")
      {
        ok = ohm::clipBounded(&start, &end, &flags, box);
      }
      else if (mode == "filter:cliptobounds")
      {
        ok = ohm::clipToBounds(&start, &end, &flags, box);
      }
      else if (mode == "filter:clipray")
      {
        ok = ohm::clipRayFilter(&start, &end, &flags, resolution);
      }
      else if (mode == "filter:goodray")
      {
        ok = ohm::goodRayFilter(&start, &end, &flags, resolution);
      }
      else
      {
        return 2;
      }
      const unsigned char head[2] = { static_cast<unsigned char>(ok), static_cast<unsigned char>(flags) };
      std::fwrite(head, 1, 2, out);
      std::fwrite(&start, sizeof(start), 1, out);
      std::fwrite(&end, sizeof(end), 1, out);
    }
    std::fclose(out);
    return 0;
  }
  try
  {
    if (ohm::configureGpu(0) != 0)
    {
      std::fprintf(stderr, "no HIP device\n");
      return 3;
    }
    if (mode == "transform")
    {
      // ohm::GpuTransformSamples::transform on a trajectory and samples from the input file, the output buffer to the
      // output file (resolution and batch size are not used).  in: u64 transforms, u64 points, f64 max_range, then
      // times[transforms], translations (dvec3 each), rotations (dquat x, y, z, w each), sample times[points], local
      // samples (dvec3 each).  out: u64 elements (2 x valid samples), then elements x (x, y, z) read back from the buffer.
      FILE *tin = std::fopen(argv[4], "rb");
      if (!tin)
      {
        return 4;
      }
      uint64_t counts[2] = { 0, 0 };
      double max_range = 0;
      if (std::fread(counts, sizeof(uint64_t), 2, tin) != 2 || std::fread(&max_range, sizeof(double), 1, tin) != 1)
      {
        std::fclose(tin);
        return 4;
      }
      const size_t transform_count = size_t(counts[0]), point_count = size_t(counts[1]);
      // The file is read as plain doubles and every struct is filled member by member, so that the order in which dvec3
      // and dquat declare their members matters: the mirror casts these arrays back to double pointers.
      std::vector<double> times(transform_count), sample_times(point_count);
      std::vector<double> raw_translations(3 * transform_count), raw_rotations(4 * transform_count);
      std::vector<double> raw_samples(3 * point_count);
      const auto read_doubles = [tin](std::vector<double> &to) {
        return std::fread(to.data(), sizeof(double), to.size(), tin) == to.size();
      };
      const bool read_ok = read_doubles(times) && read_doubles(raw_translations) && read_doubles(raw_rotations) &&
                           read_doubles(sample_times) && read_doubles(raw_samples);
      std::fclose(tin);
      if (!read_ok)
      {
        return 4;
      }
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
      if (transform.lastStatus() != OHMHIP_OK)
      {
        return 8;
      }
      std::vector<ohm::dvec3> world(elements);
      if (elements)
      {
        device_rays.read(world.data(), sizeof(ohm::dvec3) * elements);
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      std::fwrite(&elements, sizeof(elements), 1, out);
      for (uint64_t i = 0; i < elements; ++i)
      {
        const double xyz[3] = { world[i].x, world[i].y, world[i].z };
        std::fwrite(xyz, sizeof(double), 3, out);
      }
      std::fclose(out);
      return 0;
    }

    if (mode == "clearing")
    {
      // RayPattern.Clearing as the reference writes it (tests/ohmtestgpu/GpuRayPatternTests.cpp:28-85): a line of 20 occupied
      // voxels along x written directly, hit probability 0.51, miss probability 0; a one-ray pattern along y, rotated onto
      // x by angleAxis(-pi/2, z) and moved to argv 6-8 (the centre of voxel 0), applied 20 times through
      // ohm::ClearingPattern.  <batch_rays> and <rays.bin> are not used.  out: per application the 2 points of
      // lastRaySet() (6 doubles), u64 points integrated and the occupancy words of the voxels (0..31, 0, 0) after
      // syncVoxels(); then the whole occupancy block of region (0, 0, 0) and the map's miss value (float).
      if (argc < 9)
      {
        return 2;
      }
      const unsigned voxel_count = 20;
      ohm::OccupancyMap line_map(resolution);
      line_map.setHitProbability(0.51f);
      line_map.setMissProbability(0.0f);
      const std::array<int16_t, 3> key{ { 0, 0, 0 } };
      {
        std::vector<uint8_t> &block = line_map.region(key).voxel_blocks[OHMHIP_LID_OCCUPANCY];
        std::vector<float> values(line_map.regionVoxelVolume(), std::numeric_limits<float>::infinity());
        for (unsigned i = 0; i < voxel_count; ++i)
        {
          values[i] = line_map.hitValue();
        }
        block.resize(sizeof(float) * values.size());
        std::memcpy(block.data(), values.data(), block.size());
      }
      ohm::GpuMap line_gpu_map(&line_map, true);
      line_gpu_map.uploadRegions(nullptr, 0);
      ohm::RayPattern line_pattern;
      line_pattern.addPoint(ohm::dvec3{ 0, line_map.resolution() * voxel_count, 0 });
      ohm::ClearingPattern clearing(&line_pattern, false);
      const ohm::dvec3 pattern_translate{ std::atof(argv[6]), std::atof(argv[7]), std::atof(argv[8]) };
      const double half_angle = (-0.5 * 3.14159265358979323846) * 0.5;  // glm::angleAxis(-0.5 * M_PI, (0, 0, 1))
      const ohm::dquat rotation{ 0 * std::sin(half_angle), 0 * std::sin(half_angle), 1 * std::sin(half_angle),
                                 std::cos(half_angle) };
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      for (unsigned i = 0; i < voxel_count; ++i)
      {
        const uint64_t integrated = clearing.apply(&line_gpu_map, pattern_translate, rotation);
        line_gpu_map.syncVoxels();
        size_t elements = 0;
        const ohm::dvec3 *ray_set = clearing.lastRaySet(&elements);
        if (elements != 2)
        {
          std::fclose(out);
          return 7;
        }
        std::fwrite(ray_set, sizeof(ohm::dvec3), 2, out);
        std::fwrite(&integrated, sizeof(integrated), 1, out);
        std::fwrite(line_map.region(key).voxel_blocks[OHMHIP_LID_OCCUPANCY].data(), sizeof(float), 32, out);
      }
      const std::vector<uint8_t> &block = line_map.region(key).voxel_blocks[OHMHIP_LID_OCCUPANCY];
      std::fwrite(block.data(), 1, block.size(), out);
      const float miss_value = line_gpu_map.missValue();
      std::fwrite(&miss_value, sizeof(miss_value), 1, out);
      std::fclose(out);
      return 0;
    }
    if (mode == "heightmapfill")
    {
      // ohm::Heightmap in HeightmapMode::kSimpleFill over a map whose voxels are written directly; <rays.bin> is a scene
      // file instead (<batch_rays> is not used).  in: i32 region dims[3], f64 reference[3], f64 floor, ceiling,
      // min_clearance, i32 up axis, u32 flags (1 virtual surfaces, 2 promote below), u64 regions, then per region i16[3]
      // key and its occupancy block.  out: u32 ma, u32 mb, the ohmhip_heightmap_fill_stats, u64 surface and u64 virtual
      // cells as getHeightmapVoxelInfo names them, then the occupancy, HeightmapVoxel, source visit arrays and the log.
      FILE *sin = std::fopen(argv[4], "rb");
      if (!sin)
      {
        return 4;
      }
      int32_t dims[3] = { 0, 0, 0 }, up_axis = 2;
      double numbers[6] = {};
      uint32_t flags = 0;
      uint64_t regions = 0;
      bool read_ok = std::fread(dims, sizeof(int32_t), 3, sin) == 3 && std::fread(numbers, sizeof(double), 6, sin) == 6 &&
                     std::fread(&up_axis, sizeof(up_axis), 1, sin) == 1 && std::fread(&flags, sizeof(flags), 1, sin) == 1 &&
                     std::fread(&regions, sizeof(regions), 1, sin) == 1;
      ohm::OccupancyMap fill_map(resolution, dims[0], dims[1], dims[2]);
      for (uint64_t i = 0; read_ok && i < regions; ++i)
      {
        std::array<int16_t, 3> key{};
        read_ok = std::fread(key.data(), sizeof(int16_t), 3, sin) == 3;
        if (read_ok)
        {
          std::vector<uint8_t> &block = fill_map.region(key).voxel_blocks[OHMHIP_LID_OCCUPANCY];
          block.resize(sizeof(float) * fill_map.regionVoxelVolume());
          read_ok = std::fread(block.data(), 1, block.size(), sin) == block.size();
        }
      }
      std::fclose(sin);
      if (!read_ok)
      {
        return 4;
      }
      ohm::GpuMap fill_gpu_map(&fill_map, true);
      fill_gpu_map.uploadRegions(nullptr, 0);
      ohm::Heightmap heightmap(resolution, numbers[5], ohm::UpAxis(up_axis));
      heightmap.setOccupancyMap(&fill_gpu_map);
      heightmap.setFloor(numbers[3]);
      heightmap.setCeiling(numbers[4]);
      heightmap.setGenerateVirtualSurface((flags & 1u) != 0);
      heightmap.setPromoteVirtualBelow((flags & 2u) != 0);
      heightmap.setKeepVisitLog(true);
      heightmap.setMode(ohm::HeightmapMode::kLayeredFill);
      if (heightmap.buildHeightmap(ohm::dvec3{ numbers[0], numbers[1], numbers[2] }) ||
          heightmap.lastStatus() != OHMHIP_ERR_UNSUPPORTED)
      {
        return 7;  // the layered modes stay refused
      }
      heightmap.setMode(ohm::HeightmapMode::kSimpleFill);
      if (!heightmap.buildHeightmap(ohm::dvec3{ numbers[0], numbers[1], numbers[2] }))
      {
        return 8;
      }
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
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint32_t ma = uint32_t(heightmap.heightmapCellsA()), mb = uint32_t(heightmap.heightmapCellsB());
      std::fwrite(&ma, sizeof(ma), 1, out);
      std::fwrite(&mb, sizeof(mb), 1, out);
      std::fwrite(&heightmap.fillStats(), sizeof(ohmhip_heightmap_fill_stats), 1, out);
      std::fwrite(types, sizeof(uint64_t), 2, out);
      std::fwrite(heightmap.occupancy().data(), sizeof(float), heightmap.occupancy().size(), out);
      std::fwrite(heightmap.heightmapVoxels().data(), sizeof(ohm::HeightmapVoxel), heightmap.heightmapVoxels().size(), out);
      std::fwrite(heightmap.sourceVisits().data(), sizeof(uint32_t), heightmap.sourceVisits().size(), out);
      std::fwrite(heightmap.visitLog().data(), sizeof(uint32_t), heightmap.visitLog().size(), out);
      std::fclose(out);
      return 0;
    }

    FILE *in = std::fopen(argv[4], "rb");
    if (!in)
    {
      return 4;
    }
    uint64_t n_points = 0;
    if (std::fread(&n_points, sizeof(n_points), 1, in) != 1)
    {
      return 4;
    }
    std::vector<ohm::dvec3> rays(n_points);
    if (std::fread(rays.data(), sizeof(ohm::dvec3), n_points, in) != n_points)
    {
      return 4;
    }
    std::fclose(in);

    if (mode == "voxeledit")
    {
      // Voxel edits by key through the host mirror.  <rays.bin> holds the points of an edit script, argv 6 names a raw
      // file with one op byte per point (1 HIT, 2 MISS, 3 HIT_SAMPLE); <batch_rays> is not used.  On an occupancy + mean
      // map: GpuMap::integrateVoxels of the script; then the single-voxel conveniences on the first point --
      // integrateHit(sample), integrateMiss(key), integrateHit(key) --; then integrateMisses(keyRange(p, q)) with p and
      // q the script's last two points.  out.bin: the map's regions (layout at the top), then the five counters of
      // lastEditStats() after the script (u64 each), u64 range keys and the keys of keyRange (10 bytes each).
      if (argc < 7 || rays.size() < 2)
      {
        return 2;
      }
      std::vector<ohm::GpuMap::VoxelEdit> ops(rays.size());
      FILE *oin = std::fopen(argv[6], "rb");
      if (!oin || std::fread(ops.data(), 1, ops.size(), oin) != ops.size())
      {
        return 4;
      }
      std::fclose(oin);
      ohm::OccupancyMap edit_map(resolution);
      edit_map.addLayer(OHMHIP_LID_MEAN);
      ohm::GpuMap edit_gpu_map(&edit_map, true);
      if (edit_gpu_map.integrateVoxels(ops.data(), ohm::GpuMap::VoxelEdit::kHit, nullptr, rays.data(), rays.size()) != OHMHIP_OK)
      {
        return 8;
      }
      const ohmhip_voxel_edit_stats script_stats = edit_gpu_map.lastEditStats();
      const std::vector<ohm::CloudKey> first = edit_gpu_map.voxelKeys(rays.data(), 1);
      if (edit_gpu_map.lastStatus() != OHMHIP_OK || edit_gpu_map.integrateHit(rays[0]) != OHMHIP_OK ||
          edit_gpu_map.integrateMiss(first[0]) != OHMHIP_OK || edit_gpu_map.integrateHit(first[0]) != OHMHIP_OK)
      {
        return 8;
      }
      const std::vector<ohm::CloudKey> range = edit_gpu_map.keyRange(rays[rays.size() - 2], rays[rays.size() - 1]);
      if (edit_gpu_map.lastStatus() != OHMHIP_OK || edit_gpu_map.integrateMisses(range) != OHMHIP_OK)
      {
        return 8;
      }
      edit_gpu_map.syncVoxels();
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint64_t regions = edit_map.regionCount();
      std::fwrite(&regions, sizeof(regions), 1, out);
      for (const auto &entry : edit_map.chunks())
      {
        std::fwrite(entry.first.data(), sizeof(int16_t), 3, out);
        for (uint32_t layer = 0; layer < uint32_t(OHMHIP_LID_COUNT); ++layer)
        {
          if (!edit_map.hasLayer(int(layer)))
          {
            continue;
          }
          const auto &block = entry.second.voxel_blocks[layer];
          const uint64_t bytes = block.size();
          std::fwrite(&layer, sizeof(layer), 1, out);
          std::fwrite(&bytes, sizeof(bytes), 1, out);
          std::fwrite(block.data(), 1, bytes, out);
        }
      }
      const uint64_t counters[6] = { script_stats.applied,         script_stats.null_keys,       script_stats.distinct_voxels,
                                     script_stats.regions_touched, script_stats.regions_created, range.size() };
      std::fwrite(counters, sizeof(uint64_t), 6, out);
      std::fwrite(range.data(), sizeof(ohm::CloudKey), range.size(), out);
      std::fclose(out);
      return 0;
    }

    if (mode == "copy")
    {
      // Copy.CopySubmapFromGpu (tests/ohmtestgpu/GpuCopyTests.cpp:112-150): the rays into a GpuMap, then -- without a
      // sync of the source -- ohm::copyMap into a second map with copyFilterExtents [argv 6: box minimum, argv 7: box
      // maximum on every axis, default 0 and 4.5], and a clone() of the same box.  out.bin = the source's chunks, then
      // the copy's, then the clone's, each in the layout of the integration modes below.
      const double box_min = argc > 6 ? std::atof(argv[6]) : 0.0;
      const double box_max = argc > 7 ? std::atof(argv[7]) : 4.5;
      ohm::OccupancyMap src_map(resolution), dst_map(resolution);
      ohm::GpuMap src(&src_map, true), dst(&dst_map, true);
      if (!ohm::canCopy(dst, src) || ohm::canCopy(src, src))
      {
        return 8;
      }
      const size_t step = batch_rays ? 2 * batch_rays : rays.size();
      for (size_t i = 0; i < rays.size(); i += step)
      {
        const size_t n = std::min(step, rays.size() - i);
        if (src.integrateRays(rays.data() + i, n) != n)
        {
          return 7;
        }
      }
      const ohm::dvec3 copy_min{ box_min, box_min, box_min }, copy_max{ box_max, box_max, box_max };
      ohmhip_copy_stats stats;
      if (!ohm::copyMap(dst, src, ohm::copyFilterExtents(copy_min, copy_max), {}, &stats) ||
          stats.regions_passed != stats.regions_created || stats.layers_copied != OHMHIP_LAYER_BIT(OHMHIP_LID_OCCUPANCY))
      {
        return 8;
      }
      // the same box by a host lambda (the keys go down), and a filter that passes nothing
      ohm::OccupancyMap again_map(resolution);
      ohm::GpuMap again(&again_map, true);
      const ohm::CopyChunkFilter box = ohm::copyFilterExtents(copy_min, copy_max);
      ohmhip_copy_stats again_stats;
      if (!ohm::copyMap(again, src, [&box](const ohm::CopyChunk &chunk) { return box(chunk); }, {}, &again_stats) ||
          again_stats.regions_passed != stats.regions_passed || again_stats.bytes_copied != stats.bytes_copied ||
          !ohm::copyMap(again, src, ohm::copyFilterNegate(ohm::CopyChunkFilter())) ||
          ohm::copyMap(again, src, {}, ohm::copyFilterNegate(ohm::copyLayersFilter({ "occupancy" }))) != true)
      {
        return 8;
      }
      std::unique_ptr<ohm::GpuMap> clone = src.clone(copy_min, copy_max);
      if (!clone)
      {
        return 8;
      }
      src.syncVoxels();
      dst.syncVoxels();
      clone->syncVoxels();
      std::printf("copied %llu of %zu regions, %llu bytes\n", (unsigned long long)stats.regions_passed, src_map.regionCount(),
                  (unsigned long long)stats.bytes_copied);
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      for (const ohm::OccupancyMap *m : { &src_map, &dst_map, &clone->map() })
      {
        const uint64_t regions = m->regionCount();
        std::fwrite(&regions, sizeof(regions), 1, out);
        for (const auto &entry : m->chunks())
        {
          std::fwrite(entry.first.data(), sizeof(int16_t), 3, out);
          const uint32_t layer = OHMHIP_LID_OCCUPANCY;
          const auto &block = entry.second.voxel_blocks[layer];
          const uint64_t bytes = block.size();
          std::fwrite(&layer, sizeof(layer), 1, out);
          std::fwrite(&bytes, sizeof(bytes), 1, out);
          std::fwrite(block.data(), 1, bytes, out);
        }
      }
      std::fclose(out);
      return 0;
    }

    if (mode == "compare")
    {
      // ohm::compare::compareVoxels between two GpuMaps: every ray but the last into the reference map, every ray into
      // the evaluated one.  out.bin = three comparisons of the occupancy layer -- kContinue, stop-at-first, kContinue with
      // ohmcmp's tolerance --, each as: the ohmhip_compare_result, u64 listed mismatches + their 10-byte keys, u64
      // listed missing regions + their keys, u64 messages logged.
      ohm::OccupancyMap ref_map(resolution), eval_map(resolution);
      ohm::GpuMap ref(&ref_map, true), eval(&eval_map, true);
      if (rays.size() < 4 || ref.integrateRays(rays.data(), rays.size() - 2) != rays.size() - 2 ||
          eval.integrateRays(rays.data(), rays.size()) != rays.size())
      {
        return 7;
      }
      if (!ohm::compare::compareLayoutLayer(eval, ref, "occupancy") || ohm::compare::compareLayoutLayer(eval, ref, "mean") ||
          ohm::compare::compareVoxels(eval, ref, "mean").layout_match)
      {
        return 8;
      }
      // ohmcmp's occupancy tolerance: it forgives one more ray where both maps had observed the voxel
      ohm::compare::Tolerance loose("occupancy");
      ohm::compare::configureTolerance(loose, "occupancy", 1e2f);
      ohm::compare::configureTolerance(loose, "count", uint32_t(1));  // (a name the layer lacks is ignored)
      if (!ohm::compare::compareVoxels(ref, ref, "occupancy"))
      {
        return 8;
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      for (int pass = 0; pass < 3; ++pass)
      {
        const unsigned flags = (pass == 1) ? unsigned(ohm::compare::kZero) : unsigned(ohm::compare::kContinue);
        uint64_t logged = 0;
        const ohm::compare::VoxelsResult res =
          ohm::compare::compareVoxels(eval, ref, "occupancy", pass == 2 ? &loose : nullptr, flags,
                                      [&logged](ohm::compare::Severity severity, const std::string &) {
                                        logged += severity == ohm::compare::Severity::kError ? 1u : 0u;
                                      });
        if (res.status != OHMHIP_OK || (pass < 2 && bool(res)))
        {
          std::fclose(out);
          return 8;
        }
        std::fwrite(&res.detail, sizeof(res.detail), 1, out);
        const uint64_t n_keys = res.mismatches.size(), n_missing = res.missing_regions.size();
        std::fwrite(&n_keys, sizeof(n_keys), 1, out);
        std::fwrite(res.mismatches.data(), sizeof(ohm::CloudKey), n_keys, out);
        std::fwrite(&n_missing, sizeof(n_missing), 1, out);
        for (const auto &region : res.missing_regions)
        {
          std::fwrite(region.data(), sizeof(int16_t), 3, out);
        }
        std::fwrite(&logged, sizeof(logged), 1, out);
        std::printf("compare flags %u: passed %zu failed %zu\n", flags, res.voxels_passed, res.voxels_failed);
      }
      std::fclose(out);
      return 0;
    }

    if (mode == "linekeys")
    {
      // ohm::LineKeysQueryGpu over the rays: out.bin = u64 rays, then per ray u64 index, u64 count, and after them all
      // keys (i16[3] region, u8[3] local each) in intersectedVoxels() order.
      ohm::OccupancyMap query_map(resolution);
      ohm::GpuMap query_gpu_map(&query_map, true);
      ohm::LineKeysQueryGpu query(query_gpu_map);
      query.setRays(rays.data(), rays.size());
      if (!query.executeAsync() || !query.wait() || query.numberOfResults() != rays.size() / 2)
      {
        return 8;
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint64_t n = query.numberOfResults();
      std::fwrite(&n, sizeof(n), 1, out);
      uint64_t total_keys = 0;
      for (uint64_t i = 0; i < n; ++i)
      {
        const uint64_t index = query.resultIndices()[i], count = query.resultCounts()[i];
        std::fwrite(&index, sizeof(index), 1, out);
        std::fwrite(&count, sizeof(count), 1, out);
        total_keys = index + count;
      }
      for (uint64_t k = 0; k < total_keys; ++k)
      {
        std::fwrite(query.intersectedVoxels()[k].region, sizeof(int16_t), 3, out);
        std::fwrite(query.intersectedVoxels()[k].local, sizeof(uint8_t), 3, out);
      }
      std::fclose(out);
      return 0;
    }

    if (mode == "clearanceupdate")
    {
      // [argv 6: search radius, argv 7: query flags, argv 8: region budget of the updates between batches (default 2),
      //  argv 9: region dimension (default 32)]
      // ohm::Mapper with an ohm::ClearanceProcess: batches of <batch_rays> rays, a budgeted update after each, a full
      // update at the end.  out.bin = u64 regions, then per region i16[3] key and the clearance layer (region voxels
      // f32), in ascending key order.
      const float radius = argc > 6 ? float(std::atof(argv[6])) : 0.5f;
      const unsigned flags = argc > 7 ? unsigned(std::strtoul(argv[7], nullptr, 0)) : 0u;
      const size_t budget = argc > 8 ? size_t(std::atoll(argv[8])) : 2u;
      const int dim = argc > 9 ? std::atoi(argv[9]) : 32;
      ohm::OccupancyMap update_map(resolution, dim, dim, dim);
      ohm::ClearanceProcess::ensureClearanceLayer(update_map);
      ohm::GpuMap update_gpu_map(&update_map, true);
      ohm::Mapper mapper(&update_gpu_map);
      mapper.addProcess(new ohm::ClearanceProcess(radius, flags | ohm::kQfGpuEvaluate));
      const size_t points = rays.size() & ~size_t(1);
      const size_t step = std::max<size_t>(2, 2 * batch_rays);
      for (size_t i = 0; i < points; i += step)
      {
        const size_t n = std::min(step, points - i);
        if (update_gpu_map.integrateRays(rays.data() + i, n) != n || mapper.update(1e-9, budget) < 0)
        {
          return 8;
        }
      }
      if (mapper.update(0.0) != ohm::kMprUpToDate)
      {
        return 8;
      }
      update_gpu_map.syncVoxels();
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      std::vector<std::array<int16_t, 3>> keys;
      for (const auto &entry : update_map.chunks())
      {
        keys.push_back(entry.second.region);
      }
      std::sort(keys.begin(), keys.end());
      const uint64_t count = keys.size();
      std::fwrite(&count, sizeof(count), 1, out);
      for (const auto &key : keys)
      {
        const auto &block = update_map.chunks().find(key)->second.voxel_blocks[OHMHIP_LID_CLEARANCE];
        std::fwrite(key.data(), sizeof(int16_t), 3, out);
        std::fwrite(block.data(), 1, block.size(), out);
      }
      std::fclose(out);
      return 0;
    }

    if (mode == "clearance" || mode == "linequery")
    {
      // [argv 6: search radius (default 0.5), argv 7: query flags (default 0)]
      // clearance: every ray builds the map; ohm::ClearanceProcess over the extents of all the rays' points.
      //   out.bin = u64 regions, then per region i16[3] key and region voxels f32, in ascending key order.
      // linequery: the last <batch_rays> rays are query lines, each an ohm::LineQueryGpu; the rays before them build
      //   the map.  out.bin = u64 lines, then per line u32 results and per result i16[3] region, u8[3]
      //   local, f32 range.
      const float radius = argc > 6 ? float(std::atof(argv[6])) : 0.5f;
      const unsigned flags = argc > 7 ? unsigned(std::strtoul(argv[7], nullptr, 0)) : 0u;
      ohm::OccupancyMap query_map(resolution);
      ohm::GpuMap query_gpu_map(&query_map, true);
      const size_t query_points = mode == "clearance" ? 0 : std::min(2 * batch_rays, rays.size() & ~size_t(1));
      const size_t build_points = (rays.size() & ~size_t(1)) - query_points;
      if (build_points && query_gpu_map.integrateRays(rays.data(), build_points) != build_points)
      {
        return 8;
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      if (mode == "clearance")
      {
        ohm::dvec3 lo = rays[0], hi = rays[0];
        for (size_t i = 1; i < build_points; ++i)
        {
          lo.x = std::min(lo.x, rays[i].x);
          lo.y = std::min(lo.y, rays[i].y);
          lo.z = std::min(lo.z, rays[i].z);
          hi.x = std::max(hi.x, rays[i].x);
          hi.y = std::max(hi.y, rays[i].y);
          hi.z = std::max(hi.z, rays[i].z);
        }
        ohm::ClearanceProcess clearance(radius, flags | ohm::kQfGpuEvaluate);
        if (!clearance.calculateForExtents(query_gpu_map, lo, hi))
        {
          std::fclose(out);
          return 8;
        }
        size_t n = 0;
        ohmhip_map_regions(query_gpu_map.handle(), nullptr, 0, &n);
        std::vector<std::array<int16_t, 3>> keys(n);
        if (n)
        {
          ohmhip_map_regions(query_gpu_map.handle(), keys.front().data(), n, &n);
        }
        std::sort(keys.begin(), keys.end());
        const uint64_t count = keys.size();
        std::fwrite(&count, sizeof(count), 1, out);
        for (const auto &key : keys)
        {
          const float *block = clearance.regionClearance(key);
          if (!block)
          {
            std::fclose(out);
            return 8;
          }
          std::fwrite(key.data(), sizeof(int16_t), 3, out);
          std::fwrite(block, sizeof(float), query_map.regionVoxelVolume(), out);
        }
        std::fclose(out);
        return 0;
      }
      const uint64_t lines = (rays.size() - build_points) / 2;
      std::fwrite(&lines, sizeof(lines), 1, out);
      for (size_t i = build_points; i + 1 < rays.size(); i += 2)
      {
        ohm::LineQueryGpu query(query_gpu_map, rays[i], rays[i + 1], radius, flags);
        if (!(query.queryFlags() & ohm::kQfGpuEvaluate) || !query.executeAsync() || !query.wait())
        {
          std::fclose(out);
          return 8;
        }
        const uint32_t n = uint32_t(query.numberOfResults());
        std::fwrite(&n, sizeof(n), 1, out);
        for (uint32_t k = 0; k < n; ++k)
        {
          std::fwrite(query.intersectedVoxels()[k].region, sizeof(int16_t), 3, out);
          std::fwrite(query.intersectedVoxels()[k].local, sizeof(uint8_t), 3, out);
          std::fwrite(&query.ranges()[k], sizeof(float), 1, out);
        }
      }
      std::fclose(out);
      return 0;
    }

    if (mode == "heightmap")
    {
      // ohm::Heightmap: the map (occupancy + mean) is built by ohm::GpuMap::integrateRays in batches, still collected by
      // batch coalescing when the heightmap is asked for; [search radius] is min_clearance, [query flags] bit 0 turns
      // virtual surfaces on.  Reference position (0, 0, 0), +Z up, grid resolution = the map's.  out.bin = u32 ma, u32
      // mb, u64 populated, u64 cells, u8 has mean, then the occupancy, HeightmapVoxel and (if any) VoxelMean arrays.
      ohm::OccupancyMap hm_map(resolution);
      hm_map.addLayer(OHMHIP_LID_MEAN);
      ohm::GpuMap hm_gpu_map(&hm_map, true);
      const size_t step = std::max<size_t>(2, batch_rays * 2);
      for (size_t at = 0; at + 1 < rays.size(); at += step)
      {
        const size_t count = std::min(step, (rays.size() - at) & ~size_t(1));
        if (hm_gpu_map.integrateRays(rays.data() + at, count) != count)
        {
          return 8;
        }
      }
      ohm::Heightmap heightmap(resolution, argc > 6 ? std::atof(argv[6]) : 0.0, ohm::UpAxis::kZ);
      heightmap.setOccupancyMap(&hm_gpu_map);
      heightmap.setGenerateVirtualSurface(argc > 7 && (std::atoi(argv[7]) & 1));
      if (!heightmap.buildHeightmap(ohm::dvec3{ 0.0, 0.0, 0.0 }))
      {
        return 8;
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint32_t ma = uint32_t(heightmap.heightmapCellsA()), mb = uint32_t(heightmap.heightmapCellsB());
      const uint64_t populated = heightmap.populatedCount(), cells = heightmap.cellCount();
      const uint8_t has_mean = heightmap.voxelMeans().empty() ? 0 : 1;
      std::fwrite(&ma, sizeof(ma), 1, out);
      std::fwrite(&mb, sizeof(mb), 1, out);
      std::fwrite(&populated, sizeof(populated), 1, out);
      std::fwrite(&cells, sizeof(cells), 1, out);
      std::fwrite(&has_mean, 1, 1, out);
      std::fwrite(heightmap.occupancy().data(), sizeof(float), heightmap.occupancy().size(), out);
      std::fwrite(heightmap.heightmapVoxels().data(), sizeof(ohm::HeightmapVoxel), heightmap.heightmapVoxels().size(), out);
      std::fwrite(heightmap.voxelMeans().data(), sizeof(ohm::VoxelMean), heightmap.voxelMeans().size(), out);
      std::fclose(out);
      return 0;
    }

    if (mode == "cloud")
    {
      // ohm::extractCloud: the map (occupancy + mean) is built by ohm::GpuMap::integrateRays in batches, still collected
      // by batch coalescing when the cloud is asked for; [search radius] != 0 exports free voxels too.  out.bin = u64
      // count, u64 points, then the positions (3 f64 each), the keys (10 bytes each) and the values (f32).
      ohm::OccupancyMap cloud_map(resolution);
      cloud_map.addLayer(OHMHIP_LID_MEAN);
      ohm::GpuMap cloud_gpu_map(&cloud_map, true);
      const size_t step = std::max<size_t>(2, batch_rays * 2);
      for (size_t at = 0; at + 1 < rays.size(); at += step)
      {
        const size_t count = std::min(step, (rays.size() - at) & ~size_t(1));
        if (cloud_gpu_map.integrateRays(rays.data() + at, count) != count)
        {
          return 8;
        }
      }
      ohm::CloudOptions options;
      options.export_free = argc > 6 && std::atof(argv[6]) != 0.0;
      const ohm::VoxelCloud cloud = ohm::extractCloud(cloud_gpu_map, options);
      if (cloud.status != OHMHIP_OK)
      {
        return 8;
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint64_t points = cloud.positions.size();
      std::fwrite(&cloud.count, sizeof(cloud.count), 1, out);
      std::fwrite(&points, sizeof(points), 1, out);
      std::fwrite(cloud.positions.data(), sizeof(ohm::dvec3), cloud.positions.size(), out);
      std::fwrite(cloud.keys.data(), sizeof(ohm::CloudKey), cloud.keys.size(), out);
      std::fwrite(cloud.values.data(), sizeof(float), cloud.values.size(), out);
      std::fclose(out);
      return 0;
    }

    if (mode == "neighbours" || mode == "voxels")
    {
      // ohm::NearestNeighbours / GpuMap::nearestNeighbours and the voxel reads: the map (occupancy + mean) is built by
      // ohm::GpuMap::integrateRays in batches, still collected by batch coalescing when the first query is asked; the
      // query points are the end points of every 97th ray.
      //   neighbours: [search radius] [query flags]; out.bin = u64 queries, u64 results, the counts (u64 each), the keys
      //   (10 bytes each), the ranges (f32), then what an ohm::NearestNeighbours object reports for the first point: u64
      //   results, per result i16[3] region, u8[3] local, f64 range.
      //   voxels: out.bin = u64 keys, the keys of GpuMap::voxelKeys (10 bytes each), the occupancy values (f32), the mean
      //   voxels (8 bytes each), present (u8 each), the occupancy types (i8 each).
      ohm::OccupancyMap point_map(resolution);
      point_map.addLayer(OHMHIP_LID_MEAN);
      ohm::GpuMap point_gpu_map(&point_map, true);
      const size_t step = std::max<size_t>(2, batch_rays * 2);
      for (size_t at = 0; at + 1 < rays.size(); at += step)
      {
        const size_t count = std::min(step, (rays.size() - at) & ~size_t(1));
        if (point_gpu_map.integrateRays(rays.data() + at, count) != count)
        {
          return 8;
        }
      }
      std::vector<ohm::dvec3> points;
      for (size_t i = 1; i < rays.size(); i += 2 * 97)
      {
        points.push_back(rays[i]);
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint64_t n_points = points.size();
      std::fwrite(&n_points, sizeof(n_points), 1, out);
      if (mode == "neighbours")
      {
        const float radius = (argc > 6) ? float(std::atof(argv[6])) : 0.25f;
        const unsigned flags = (argc > 7) ? unsigned(std::atoi(argv[7])) : 0u;
        std::vector<uint64_t> counts;
        std::vector<ohm::CloudKey> keys;
        std::vector<float> ranges;
        if (point_gpu_map.nearestNeighbours(points.data(), points.size(), radius, flags, counts, keys, ranges) != OHMHIP_OK)
        {
          std::fclose(out);
          return 8;
        }
        const uint64_t n_results = keys.size();
        std::fwrite(&n_results, sizeof(n_results), 1, out);
        std::fwrite(counts.data(), sizeof(uint64_t), counts.size(), out);
        std::fwrite(keys.data(), sizeof(ohm::CloudKey), keys.size(), out);
        std::fwrite(ranges.data(), sizeof(float), ranges.size(), out);
        ohm::NearestNeighbours query(point_gpu_map, points.empty() ? ohm::dvec3{ 0, 0, 0 } : points[0], radius, flags);
        if (!query.execute())
        {
          std::fclose(out);
          return 8;
        }
        const uint64_t n_query = query.numberOfResults();
        std::fwrite(&n_query, sizeof(n_query), 1, out);
        for (size_t i = 0; i < query.numberOfResults(); ++i)
        {
          std::fwrite(query.intersectedVoxels()[i].region, sizeof(int16_t), 3, out);
          std::fwrite(query.intersectedVoxels()[i].local, 1, 3, out);
          std::fwrite(&query.ranges()[i], sizeof(double), 1, out);
        }
      }
      else
      {
        const std::vector<ohm::CloudKey> keys = point_gpu_map.voxelKeys(points.data(), points.size());
        std::vector<uint8_t> occupancy, mean, present, present_mean;
        if (point_gpu_map.lastStatus() != OHMHIP_OK ||
            point_gpu_map.readVoxels(OHMHIP_LID_OCCUPANCY, keys, occupancy, present) != OHMHIP_OK ||
            point_gpu_map.readVoxels(OHMHIP_LID_MEAN, keys, mean, present_mean) != OHMHIP_OK || present != present_mean)
        {
          std::fclose(out);
          return 8;
        }
        const std::vector<int8_t> types = point_gpu_map.occupancyTypes(keys);
        std::fwrite(keys.data(), sizeof(ohm::CloudKey), keys.size(), out);
        std::fwrite(occupancy.data(), 1, occupancy.size(), out);
        std::fwrite(mean.data(), 1, mean.size(), out);
        std::fwrite(present.data(), 1, present.size(), out);
        std::fwrite(types.data(), 1, types.size(), out);
      }
      std::fclose(out);
      return 0;
    }

    if (mode == "filter")
    {
      // GpuMap::filterPoints: the map (occupancy + mean) is built as for `neighbours`; the points are every ray's end
      // point and, displaced by [offset] (default 0.35) along x, the same again.  [tolerance] (default -1) [occupancy only].
      //   out.bin = u64 points, u64 kept, the status (u8 each), the kept indices (u64 each), the values (f64 each), the
      //   keys (10 bytes each).
      ohm::OccupancyMap filter_map(resolution);
      filter_map.addLayer(OHMHIP_LID_MEAN);
      ohm::GpuMap filter_gpu_map(&filter_map, true);
      const size_t step = std::max<size_t>(2, batch_rays * 2);
      for (size_t at = 0; at + 1 < rays.size(); at += step)
      {
        const size_t count = std::min(step, (rays.size() - at) & ~size_t(1));
        if (filter_gpu_map.integrateRays(rays.data() + at, count) != count)
        {
          return 8;
        }
      }
      const double tolerance = (argc > 6) ? std::atof(argv[6]) : -1.0;
      const bool occupancy_only = argc > 7 && std::atoi(argv[7]) != 0;
      const double offset = (argc > 8) ? std::atof(argv[8]) : 0.35;
      std::vector<ohm::dvec3> points;
      for (int pass = 0; pass < 2; ++pass)
      {
        for (size_t i = 1; i < rays.size(); i += 2)
        {
          ohm::dvec3 p = rays[i];
          p.x += pass * offset;
          points.push_back(p);
        }
      }
      std::vector<uint8_t> status;
      std::vector<uint64_t> kept;
      std::vector<double> values;
      std::vector<ohm::CloudKey> keys;
      if (filter_gpu_map.filterPoints(points.data(), points.size(), tolerance, occupancy_only, status, kept, values, keys) !=
          OHMHIP_OK)
      {
        return 8;
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint64_t n_points = points.size(), n_kept = kept.size();
      std::fwrite(&n_points, sizeof(n_points), 1, out);
      std::fwrite(&n_kept, sizeof(n_kept), 1, out);
      std::fwrite(status.data(), 1, status.size(), out);
      std::fwrite(kept.data(), sizeof(uint64_t), kept.size(), out);
      std::fwrite(values.data(), sizeof(double), values.size(), out);
      std::fwrite(keys.data(), sizeof(ohm::CloudKey), keys.size(), out);
      std::fclose(out);
      return 0;
    }

    if (mode == "raysquery")
    {
      // ohm::RaysQueryGpu: the first half of the rays builds the map (ohm::GpuMap::integrateRays), the second half is
      // the query (addRay / executeAsync / wait).  out.bin = u64 rays, then per ray f64 range, f64 unobserved volume,
      // i32 terminal type, i16[3] region, u8[3] local.
      ohm::OccupancyMap query_map(resolution);
      ohm::GpuMap query_gpu_map(&query_map, true);
      const size_t build_points = (rays.size() / 2) & ~size_t(1);
      if (build_points && query_gpu_map.integrateRays(rays.data(), build_points) != build_points)
      {
        return 8;
      }
      ohm::RaysQueryGpu query(query_gpu_map);
      for (size_t i = build_points; i + 1 < rays.size(); i += 2)
      {
        query.addRay(rays[i], rays[i + 1]);
      }
      if (!(query.queryFlags() & ohm::kQfGpuEvaluate) || !query.executeAsync() || !query.wait() ||
          query.numberOfResults() != query.numberOfRays())
      {
        return 8;
      }
      FILE *out = std::fopen(argv[5], "wb");
      if (!out)
      {
        return 6;
      }
      const uint64_t n = query.numberOfResults();
      std::fwrite(&n, sizeof(n), 1, out);
      for (uint64_t i = 0; i < n; ++i)
      {
        const int32_t type = query.terminalOccupancyTypes()[i];
        std::fwrite(&query.ranges()[i], sizeof(double), 1, out);
        std::fwrite(&query.unobservedVolumes()[i], sizeof(double), 1, out);
        std::fwrite(&type, sizeof(type), 1, out);
        std::fwrite(query.intersectedVoxels()[i].region, sizeof(int16_t), 3, out);
        std::fwrite(query.intersectedVoxels()[i].local, sizeof(uint8_t), 3, out);
      }
      std::fclose(out);
      return 0;
    }

    ohm::OccupancyMap map(resolution);
    std::unique_ptr<ohm::GpuMap> gpu_map;
    if (mode == "occ" || mode == "occmean" || mode == "occdev" || mode == "occcoalesce" || mode == "occowner" ||
        mode == "occclipbox" || mode == "occpart" || mode == "occpartint")
    {
      if (mode == "occmean")
      {
        map.addLayer(OHMHIP_LID_MEAN);
      }
      gpu_map.reset(new ohm::GpuMap(&map, true, unsigned(batch_rays * 2)));
      if (mode == "occcoalesce")
      {
        gpu_map->setBatchCoalescing(3 * batch_rays + 1);  // every fourth call launches a device batch
      }
      if (mode == "occclipbox")
      {
        // GpuMap.ClipBox (tests/ohmtestgpu/GpuMapTest.cpp:633-647): a RayFilterFunction wrapping clipBounded
        const ohm::Aabb clip_box(ohm::dvec3{ -1.0, -1.0, -1.0 }, ohm::dvec3{ 2.0, 2.0, 2.0 });
        gpu_map->setRayFilter([clip_box](ohm::dvec3 *start, ohm::dvec3 *end, unsigned *filter_flags) {
          return ohm::clipBounded(start, end, filter_flags, clip_box);
        });
      }
      if (mode == "occpart")
      {
        // rank 1 of a two-way partition by a table: region blocks (2 x 2 x 2 regions) with block x >= 1 belong to rank 1
        ohm::GpuMap::RegionPartition part;
        part.world_size = 2;
        part.rank = 1;
        part.block_shift = 1;
        part.grid_origin[0] = 0;
        part.grid_dims[0] = 2;
        part.grid_dims[1] = part.grid_dims[2] = 1;
        part.owners = { 0, 1 };
        gpu_map->setRegionPartition(part);
      }
      if (mode == "occowner")
      {
        gpu_map->setRegionOwnership(2, 1);  // this map is rank 1 of a two-way region partition
      }
    }
    else if (mode == "ndt")
    {
      gpu_map.reset(new ohm::GpuNdtMap(&map, true, unsigned(batch_rays * 2)));
    }
    else if (mode == "tsdf")
    {
      gpu_map.reset(new ohm::GpuTsdfMap(&map, true, unsigned(batch_rays * 2)));
    }
    else
    {
      return 2;
    }
    if (!gpu_map->gpuOk())
    {
      return 5;
    }
    const size_t batch_points = batch_rays ? batch_rays * 2 : size_t(n_points);
    size_t total = 0;
    if (mode == "occdev")
    {
      gputil::Device device;
      gputil::Queue queue = device.defaultQueue();
      ohm::GpuTransformSamples transform(device);
      gputil::Buffer device_rays;
      const double times[2] = { 0.0, 1.0 };
      const ohm::dvec3 translations[2] = { { 0, 0, 0 }, { 0, 0, 0 } };
      const ohm::dquat rotations[2] = { { 0, 0, 0, 1 }, { 0, 0, 0, 1 } };
      std::vector<ohm::dvec3> samples;
      std::vector<double> sample_times;
      for (size_t i = 0; i < n_points; i += batch_points)
      {
        const size_t count = std::min<size_t>(batch_points, n_points - i);
        samples.clear();
        sample_times.clear();
        for (size_t k = 1; k < count; k += 2)
        {
          samples.push_back(rays[i + k]);
          sample_times.push_back(0.25 + 0.5 * double(k) / double(count));
        }
        const unsigned elements = transform.transform(times, translations, rotations, 2, sample_times.data(),
                                                      samples.data(), unsigned(samples.size()), queue, device_rays);
        total += gpu_map->integrateRays(device_rays, elements, ohm::kRfDefault);
      }
    }
    else if (mode == "occpartint")
    {
      // ohm::PartitionedIntegrator at world size 1 over the library's own RCCL communicator: every batch is routed on
      // the device, exchanged (count all-gather + the block a rank addresses to itself) and integrated with the previous
      // batches still in flight -- each batch from a device buffer of its own, rewritten without any wait in between.
      const auto id = ohm::RayCommunicator::uniqueId();
      ohm::RayCommunicator comm(id, 1, 0);
      ohm::GpuMap::RegionPartition whole;  // world size 1: everything belongs to rank 0
      ohm::PartitionedIntegrator integrator(*gpu_map, whole, comm);
      gputil::Buffer device_rays;
      for (size_t i = 0; i < n_points; i += batch_points)
      {
        const size_t count = std::min<size_t>(batch_points, n_points - i);
        if (!device_rays.isValid())
        {
          device_rays.create(batch_points * sizeof(ohm::dvec3));
        }
        device_rays.write(rays.data() + i, count * sizeof(ohm::dvec3));  // (free again when integrateRays returned)
        const size_t done = integrator.integrateRays(device_rays, count, ohm::kRfDefault);
        if (integrator.lastStatus() != OHMHIP_OK || integrator.raysReceived() * 2 != integrator.sendCounts()[0] * 2)
        {
          return 12;
        }
        total += done;
      }
    }
    else if (mode == "occpart")
    {
      // route every batch on the device and integrate the block addressed to this rank (what the all-to-all would
      // deliver from a single source rank); the points of rays that never reach rank 1's territory count as done
      gputil::Device device;
      gputil::Buffer device_rays, routed;
      std::vector<uint32_t> counts;
      for (size_t i = 0; i < n_points; i += batch_points)
      {
        const size_t count = std::min<size_t>(batch_points, n_points - i);
        if (!device_rays.isValid())
        {
          device_rays.create(count * sizeof(ohm::dvec3));
        }
        device_rays.resize(count * sizeof(ohm::dvec3));
        device_rays.write(rays.data() + i, count * sizeof(ohm::dvec3));
        gpu_map->routeRays(device_rays, count, ohm::kRfDefault, routed, counts);
        gputil::Buffer mine;
        if (counts[1])
        {
          std::vector<ohm::dvec3> block(size_t(counts[1]) * 2);
          routed.read(block.data(), block.size() * sizeof(ohm::dvec3), size_t(counts[0]) * 2 * sizeof(ohm::dvec3));
          mine.create(block.size() * sizeof(ohm::dvec3));
          mine.write(block.data(), block.size() * sizeof(ohm::dvec3));
          const size_t done = gpu_map->integrateRays(mine, block.size(), ohm::kRfDefault);
          if (done != block.size())
          {
            return 11;
          }
          gpu_map->syncVoxels();  // (the block buffer goes out of scope: the batch must have read it)
        }
        total += count;
      }
    }
    else
    {
      for (size_t i = 0; i < n_points; i += batch_points)
      {
        const size_t count = std::min<size_t>(batch_points, n_points - i);
        total += gpu_map->integrateRays(rays.data() + i, count, nullptr, nullptr, ohm::kRfDefault);
      }
    }
    if (mode == "occcoalesce")
    {
      gpu_map->gpuCache()->flush();  // GpuCache::flush == syncVoxels
      if (gpu_map->gpuCache()->layerCount() != 1u || gpu_map->gpuCache()->targetGpuAllocSize() != 0u)
      {
        return 9;  // (occupancy only, no memory limit set)
      }
    }
    gpu_map->syncVoxels();
    std::printf("integrated %zu of %llu points, %zu regions\n", total, (unsigned long long)n_points, map.regionCount());

    FILE *out = std::fopen(argv[5], "wb");
    if (!out)
    {
      return 6;
    }
    const uint64_t regions = map.regionCount();
    std::fwrite(&regions, sizeof(regions), 1, out);
    for (const auto &entry : map.chunks())
    {
      std::fwrite(entry.first.data(), sizeof(int16_t), 3, out);
      for (uint32_t layer = 0; layer < uint32_t(OHMHIP_LID_COUNT); ++layer)
      {
        if (!map.hasLayer(int(layer)))
        {
          continue;
        }
        const auto &block = entry.second.voxel_blocks[layer];
        const uint64_t bytes = block.size();
        std::fwrite(&layer, sizeof(layer), 1, out);
        std::fwrite(&bytes, sizeof(bytes), 1, out);
        std::fwrite(block.data(), 1, bytes, out);
      }
    }
    std::fclose(out);
    return (total == n_points) ? 0 : 7;
  }
  catch (const gputil::ApiException &e)
  {
    std::fprintf(stderr, "gputil::ApiException: %s\n", e.what());
    return 10;
  }
}
