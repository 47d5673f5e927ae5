"""CPU: the covariance entry points of the C ABI (ohmhip_covariance_decompose, ohmhip_map_covariance_eigen / _device,
ohmhip_map_covariance_ellipsoids / _count / _device) and the heightmap's OHMHIP_HM_SURFACE_NORMALS flag are exported,
declared and bound, stay out of the core ABI list, and refuse invalid arguments before any device work; the Python
mirrors exist and the heightmap's flag travels in its params."""
import ctypes as C
import os

import numpy as np

import cpp_driver
import ohm_amd
from ohm_amd import GPU_KEY_DTYPE, GpuMap, Heightmap, cloud_params
from ohm_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ohmhip_covariance_decompose", "ohmhip_map_covariance_eigen", "ohmhip_map_covariance_eigen_device",
         "ohmhip_map_covariance_ellipsoids_count", "ohmhip_map_covariance_ellipsoids",
         "ohmhip_map_covariance_ellipsoids_device")


def test_symbols_exported_and_bound():
    for name in NAMES:
        assert name in L.EXPORTED_SYMBOLS
        assert getattr(L.lib, name).restype is C.c_int


def test_declared_and_not_in_the_core_abi():
    with open(os.path.join(ROOT, "include", "ohmhip.h")) as fh:
        header = fh.read()
    core = set(sum((ln.split(":", 1)[1].split() for ln in header.splitlines() if "OHMHIP_CORE_ABI:" in ln), []))
    assert core and not core.intersection(NAMES)
    for name in NAMES:
        assert name + "(" in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_covariance_eigen_device(" in header
    assert "OHMHIP_EXPERIMENTAL int ohmhip_map_covariance_ellipsoids_device(" in header
    assert "#define OHMHIP_HM_SURFACE_NORMALS (1u << 3)" in header
    for value, name in enumerate(("OHMHIP_COV_ABSENT", "OHMHIP_COV_DECOMPOSED", "OHMHIP_COV_NON_FINITE")):
        assert "#define %s %d" % (name, value) in header
    assert "OHMHIP_LID_COUNT = 10" in header  # no new layer


def test_constants_and_struct_sizes():
    assert (L.COV_ABSENT, L.COV_DECOMPOSED, L.COV_NON_FINITE) == (0, 1, 2)
    assert L.HM_SURFACE_NORMALS == 8
    assert (L.HM_GENERATE_VIRTUAL_SURFACE, L.HM_PROMOTE_VIRTUAL_BELOW, L.HM_IGNORE_VOXEL_MEAN) == (1, 2, 4)
    assert C.sizeof(L.HeightmapParams) == 144 and L.HeightmapParams.flags.offset == 136  # unchanged by the flag
    assert C.sizeof(L.CloudParams) == 72
    assert L.lib.ohmhip_layer_voxel_bytes(L.LID_COVARIANCE) == 24
    assert GPU_KEY_DTYPE.itemsize == 10


def test_heightmap_flag_travels():
    hm = Heightmap(0.1, 0.0)
    assert hm.surface_normals is False
    assert hm.params((0, 0, 0)).flags & L.HM_SURFACE_NORMALS == 0
    hm.surface_normals = True
    assert hm.params((0, 0, 0)).flags & L.HM_SURFACE_NORMALS == L.HM_SURFACE_NORMALS


def test_refusals_before_any_device_work():
    keys = np.zeros(2, dtype=GPU_KEY_DTYPE)
    values, vectors, status = np.zeros((2, 3)), np.zeros((2, 9)), np.zeros(2, dtype=np.uint8)
    for fn in (L.lib.ohmhip_map_covariance_eigen, L.lib.ohmhip_map_covariance_eigen_device):
        assert fn(None, keys.ctypes.data, 2, values.ctypes.data, vectors.ctypes.data,
                  status.ctypes.data) == L.ERR_INVALID_ARG
        assert fn(None, None, 0, None, None, None) == L.ERR_INVALID_ARG
    p = cloud_params()
    n = C.c_uint64(0)
    assert L.lib.ohmhip_map_covariance_ellipsoids_count(None, C.byref(p), C.byref(n)) == L.ERR_INVALID_ARG
    for fn in (L.lib.ohmhip_map_covariance_ellipsoids, L.lib.ohmhip_map_covariance_ellipsoids_device):
        assert fn(None, C.byref(p), 0, None, None, None, None, None, C.byref(n)) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_covariance_decompose(None, 2, None, None, None, None, None) == L.ERR_INVALID_ARG
    assert L.lib.ohmhip_covariance_decompose(None, 0, None, None, None, None, None) == L.OK


def test_host_decomposition_needs_no_device():
    d = ohm_amd.covariance_decompose([[2, 0, 1, 0, 0, 3], [np.nan, 0, 1, 0, 0, 1]])
    assert d.status.tolist() == [1, 2]
    assert d.eigenvalues.tolist() == [[1.0, 4.0, 9.0], [1.0, 1.0, 1.0]]
    assert d.scales.tolist() == [[1.0, 2.0, 3.0], [1.0, 1.0, 1.0]]
    # one transposition of the axes has determinant -1: column 0 is negated, and its -0.0 kept
    assert np.array_equal(d.eigenvectors[0], [[-0.0, -1.0, -0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.signbit(d.eigenvectors[0, 0]).all()
    assert np.array_equal(d.eigenvectors[1], np.eye(3)) and d.normals[1].tolist() == [1.0, 0.0, 0.0]


def test_mirrors():
    assert callable(GpuMap.covarianceEigen)
    for name in ("covariance_decompose", "covariance_estimate_primary_normal", "covariance_unit_sphere_transformation",
                 "extract_covariance_ellipsoids", "save_covariance_cloud", "icosphere"):
        assert callable(getattr(ohm_amd, name)), name
    vertices, faces = ohm_amd.icosphere(1)
    assert vertices.shape == (42, 3) and faces.shape == (80, 3)
    assert np.abs(np.linalg.norm(vertices, axis=1) - 1.0).max() < 1e-15
    assert vertices.shape[0] - 120 + faces.shape[0] == 2  # Euler: V - E + F, E = 3F / 2


def test_cpp_mirror_declares_the_same_interface():
    text = cpp_driver.host_mirror_text()
    for token in ("struct CovarianceEigen", "covarianceEigenDecomposition(GpuMap &gpu_map, const std::vector<Key> &keys)",
                  "covarianceEigenDecomposition(const float *covariance6, size_t count)",
                  "covarianceEstimatePrimaryNormal(GpuMap &gpu_map", "covarianceUnitSphereTransformation(GpuMap &gpu_map",
                  "class CovarianceEllipsoids : public Query", "setSurfaceNormals(bool enable)", "surfaceNormals() const",
                  "OHMHIP_HM_SURFACE_NORMALS", "ohmhip_map_covariance_eigen(", "ohmhip_map_covariance_ellipsoids(",
                  "ohmhip_map_covariance_ellipsoids_count(", "ohmhip_covariance_decompose("):
        assert token in text, token
    driver = cpp_driver.driver_text()
    assert '{ "covariance", &modeCovariance, true }' in driver and "heightmap.setSurfaceNormals(true)" in driver
