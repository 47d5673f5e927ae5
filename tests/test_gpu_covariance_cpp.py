"""-m gpu: the covariance calls of the C++ mirror (ohm_amd/host/OhmGpuMap.h), run by `gpumap_driver covariance` over an
ohm::GpuNdtMap built from rays in batches: covarianceEigenDecomposition, covarianceEstimatePrimaryNormal and
covarianceUnitSphereTransformation over keys, the CovarianceEllipsoids query and a heightmap with setSurfaceNormals.
Every array equals, byte for byte, what the Python mirror gives on a map built by the same calls, and the by-key
results equal the model of tests/covariance_eigen_ref.py on the covariances the driver read back."""
import struct

import numpy as np
import pytest

import covariance_eigen_ref as cov_ref
import cpp_driver
import heightmap_ref as R
import ohm_amd
from heightmap_cases import two_level_scene
from ohm_amd import GPU_KEY_DTYPE, GpuNdtMap, Heightmap, OccupancyMap, extract_covariance_ellipsoids

pytestmark = pytest.mark.gpu

BATCH = 4096


class Reader:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, dtype, count):
        dtype = np.dtype(dtype)
        out = np.frombuffer(self.data, dtype=dtype, count=count, offset=self.at)
        self.at += dtype.itemsize * count
        return out

    def u64(self):
        return int(self.take("<u8", 1)[0])


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def test_cpp_covariance(gpu):
    rays = two_level_scene()
    r = Reader(cpp_driver.run("covariance", 0.1, BATCH, rays))
    n = r.u64()
    keys = r.take(GPU_KEY_DTYPE, n)
    covariance = r.take(np.float32, 6 * n).reshape(n, 6)
    eigenvalues = r.take(np.float64, 3 * n).reshape(n, 3)
    eigenvectors = r.take(np.float64, 9 * n).reshape(n, 9)
    status = r.take(np.uint8, n)
    normals = r.take(np.float64, 3 * n).reshape(n, 3)
    rotations = r.take(np.float64, 4 * n).reshape(n, 4)  # x, y, z, w
    scales = r.take(np.float64, 3 * n).reshape(n, 3)
    m = r.u64()
    e_positions = r.take(np.float64, 3 * m).reshape(m, 3)
    e_axes = r.take(np.float64, 9 * m).reshape(m, 3, 3)
    e_scales = r.take(np.float64, 3 * m).reshape(m, 3)
    e_keys = r.take(GPU_KEY_DTYPE, m)
    e_values = r.take(np.float32, m)
    ma, mb = (int(v) for v in r.take("<u4", 2))
    hm_occupancy = r.take(np.float32, ma * mb).reshape(mb, ma)
    hm_voxels = r.take(R.HEIGHTMAP_VOXEL, ma * mb).reshape(mb, ma)
    assert r.at == len(r.data)

    # the last two keys: a region the map does not hold, a null key
    assert status[-2:].tolist() == [0, 0] and (status[:-2] == 1).all() and n > 100
    for array in (eigenvalues, eigenvectors, normals, rotations, scales):
        assert not array[-2:].any()
    # by key: the model on the covariances the driver read back
    for i in range(n - 2):
        d = cov_ref.decompose(covariance[i])
        assert np.array_equal(eigenvalues[i].view(np.uint64), d.eigenvalues.view(np.uint64)), i
        assert np.array_equal(eigenvectors[i].view(np.uint64), d.eigenvectors.view(np.uint64)), i
        assert np.array_equal(normals[i].view(np.uint64), d.normal.view(np.uint64)), i
        assert np.array_equal(scales[i].view(np.uint64), d.scale.view(np.uint64)), i
    assert len(np.unique(covariance[:-2], axis=0)) > 50  # the mapper's own covariances

    # the Python mirror on a map built by the same calls
    map_ = OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean", "covariance"))
    gm = GpuNdtMap(map_)
    for at in range(0, rays.shape[0], 2 * BATCH):
        part = rays[at:at + 2 * BATCH]
        assert gm.integrateRays(part) == part.shape[0]
    want_covariance, _ = gm.readVoxels(keys, "covariance")
    assert np.array_equal(raw(covariance), raw(want_covariance))
    want = gm.covarianceEigen(keys)
    assert np.array_equal(raw(eigenvalues), raw(want[0])) and np.array_equal(raw(eigenvectors), raw(want[1]))
    assert np.array_equal(status, want[2])
    host = ohm_amd.covariance_decompose(covariance[:-2])
    quaternions, want_scales = ohm_amd.covariance_unit_sphere_transformation(covariance[:-2])  # w, x, y, z
    assert np.array_equal(raw(normals[:-2]), raw(host.normals)) and np.array_equal(raw(scales[:-2]), raw(want_scales))
    assert np.array_equal(raw(rotations[:-2]), raw(quaternions[:, [1, 2, 3, 0]]))

    ellipsoids = extract_covariance_ellipsoids(gm)
    assert m == ellipsoids.count == len(ellipsoids) > 500
    for have, expect in ((e_positions, ellipsoids.positions), (e_axes, ellipsoids.axes), (e_scales, ellipsoids.scales),
                         (e_keys, ellipsoids.keys), (e_values, ellipsoids.values)):
        assert np.array_equal(raw(have), raw(expect))

    hm = Heightmap(0.1, 0.0)
    hm.generate_virtual_surface = True
    hm.surface_normals = True
    hm.set_occupancy_map(gm)
    assert hm.build_heightmap((0.0, 0.0, 0.0))
    assert (ma, mb) == (int(hm.extents.ma), int(hm.extents.mb))
    assert np.array_equal(raw(hm_occupancy), raw(hm.occupancy)) and np.array_equal(raw(hm_voxels), raw(hm.voxels))
    assert np.stack([hm_voxels[name] for name in ("normal_x", "normal_y", "normal_z")])[:, hm_occupancy == 1.0].any()
    gm.close()
