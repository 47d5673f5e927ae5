"""ohm_amd -- MI355X-native GPU ray integration for ohm occupancy maps (GpuMap / GpuNdtMap / GpuTsdfMap path only).

The compute path is libohmhip.so (hand-written HIP for gfx950) behind the C ABI in include/ohmhip.h.  This package
is the thin host-side mirror of the reference's interface used by the tests and the benchmark harness.
"""
from ._lib import OhmHipError, LIB_PATH, EXPORTED_SYMBOLS  # noqa: F401
from .gpumap import (GpuMap, GpuNdtMap, GpuTransformSamples, GpuTsdfMap, LineKeysQueryGpu, NdtMode, OccupancyMap, RayFlag,  # noqa: F401
                     OccupancyType, RaysQueryGpu, RayMapper, LAYERS, QueryFlag, ClearanceProcess, LineQueryGpu,
                     MappingProcessResult, Mapper, NearestNeighbours, VoxelEdit, key_range,
                     device_count, device_info, probability_to_value, value_to_probability)
from .raypattern import ClearingPattern, RayPattern, RayPatternConical  # noqa: F401
from .copyutil import (canCopy, copyMap, copyFilterExtents, copyFilterDirty, copyFilterAnd, copyFilterOr,  # noqa: F401
                       copyFilterNegate, copyLayersFilter)
from .compare import (Severity, kContinue, VoxelsResult, Tolerance, VoxelMismatch, configureTolerance,  # noqa: F401
                      compareLayoutLayer, compareVoxels, occupancy_stats, compare_maps, default_tolerances)
from .heightmap import Heightmap, HeightmapMode, HeightmapVoxelType, UpAxis, HEIGHTMAP_VOXEL_DTYPE  # noqa: F401
from .heightmap import LayeredHeightmap  # noqa: F401
from .cloud import (CloudMode, VoxelCloud, GPU_KEY_DTYPE, CLOUD_CHUNK_VOXELS, cloud_params, count_cloud,  # noqa: F401
                    extract_cloud, write_ply, save_cloud, save_density_cloud, save_tsdf_cloud, save_clearance_cloud,
                    write_filtered_ply, filter_cloud, EllipsoidCloud, extract_covariance_ellipsoids, icosphere,
                    write_ellipsoid_ply, save_covariance_cloud)
from .covariance import (CovarianceDecomposition, covariance_decompose, covariance_estimate_primary_normal,  # noqa: F401
                         covariance_unit_sphere_transformation, rotation_to_quaternion, quaternion_to_rotation)
