"""-m gpu: the covariance decomposition by key on the device (ohmhip_map_covariance_eigen / _device,
GpuMap.covarianceEigen) against the model of tests/covariance_eigen_ref.py on every case of tests/covariance_cases.py:
np.array_equal on the raw bytes of eigenvalues, eigenvectors and status -- no tolerance, no excluded case.  The
covariances are planted with writeVoxels in first and last voxels of 16^3 regions (two adjacent in x, one apart), in
voxels 4095 and 4096 of a 32 x 32 x 8 region, in a tiled 64 x 64 x 16 region and in a map that spills to the host."""
import ctypes as C

import numpy as np
import pytest

import covariance_cases as cases
from ohm_amd import GPU_KEY_DTYPE, GpuNdtMap, OccupancyMap, OhmHipError, GpuMap
from ohm_amd import _lib as L

pytestmark = pytest.mark.gpu

NULL_REGION = (-32768, -32768, -32768)


def model_arrays():
    results = cases.model_results()
    return (np.stack([d.eigenvalues for d in results]), np.stack([d.eigenvectors for d in results]),
            np.array([d.status for d in results], dtype=np.uint8))


def ndt_map(dims, **kw):
    map_ = OccupancyMap(0.1, dims, layers=("occupancy", "mean", "covariance"))
    return map_, GpuNdtMap(map_, **kw)


def spread(dims, count, forced=()):
    """`count` distinct linear voxel indices of a region: the forced ones (first, last, chunk edges) and an odd stride."""
    volume = dims[0] * dims[1] * dims[2]
    assert count + len(forced) <= volume
    picked = list(dict.fromkeys(list(forced) + [(7 + 29 * k) % volume for k in range(count + len(forced))]))[:count]
    assert len(set(picked)) == count
    return picked


def locals_of(dims, linear):
    linear = np.asarray(linear)
    return np.stack([linear % dims[0], (linear // dims[0]) % dims[1], linear // (dims[0] * dims[1])], axis=1).astype(np.uint8)


def plant(gm, dims, regions, forced):
    """Every case into the given regions in turn; returns the (regions, locals) pair in case order."""
    P = cases.all_p()
    n = P.shape[0]
    region_of = np.arange(n) % len(regions)
    key_regions = np.array(regions, dtype=np.int16)[region_of]
    key_locals = np.zeros((n, 3), dtype=np.uint8)
    for r in range(len(regions)):
        mine = np.flatnonzero(region_of == r)
        key_locals[mine] = locals_of(dims, spread(dims, mine.size, forced))
    assert gm.writeVoxels((key_regions, key_locals), "covariance", P) == n
    return key_regions, key_locals


def assert_model(got, order=slice(None), what=""):
    values, vectors, status = model_arrays()
    assert np.array_equal(got[2], status[order]), what
    assert np.array_equal(got[0].view(np.uint64), values[order].view(np.uint64)), what
    assert np.array_equal(got[1].reshape(-1, 9).view(np.uint64), vectors[order].view(np.uint64)), what


@pytest.fixture(scope="module")
def cubic(gpu):
    map_, gm = ndt_map((16, 16, 16))
    keys = plant(gm, (16, 16, 16), [(0, 0, 0), (1, 0, 0), (3, 0, 0)], forced=(0, 4095))
    yield gm, keys
    gm.close()


def test_every_case_bit_for_bit(cubic):
    gm, keys = cubic
    assert {tuple(k) for k in keys[1].tolist()} >= {(0, 0, 0), (15, 15, 15)}
    written, _ = gm.readVoxels(keys, "covariance")
    assert np.array_equal(written.view(np.uint32), cases.all_p().view(np.uint32))  # NaN payloads and -0.0 as planted
    assert_model(gm.covarianceEigen(keys), what="16^3")
    # any order, duplicates included
    order = np.random.default_rng(4).integers(0, keys[0].shape[0], size=700)
    assert_model(gm.covarianceEigen((keys[0][order], keys[1][order])), order, "shuffled")


def test_absent_regions_and_voxels(cubic):
    gm, keys = cubic
    regions_before = sorted(map(tuple, gm.regionKeys()))
    stats_before = gm.cacheStats()
    probe_regions = np.array([(2, 0, 0), (0, 5, 0), NULL_REGION, (-7, -7, -7), (1, 0, 0), (3, 0, 0)], dtype=np.int16)
    probe_locals = np.array([(0, 0, 0), (15, 15, 15), (0, 0, 0), (3, 4, 5), (0, 0, 1), (1, 0, 0)], dtype=np.uint8)
    used = {(tuple(r), tuple(l)) for r, l in zip(keys[0].tolist(), keys[1].tolist())}
    assert ((1, 0, 0), (0, 0, 1)) not in used and ((3, 0, 0), (1, 0, 0)) not in used
    values, vectors, status = gm.covarianceEigen((probe_regions, probe_locals))
    assert status.tolist() == [0, 0, 0, 0, 1, 1]
    assert not values[:4].any() and not vectors[:4].any()
    # a never written voxel of a present region holds the zero matrix: eigenvalues 0, the identity
    assert not values[4:].any() and np.array_equal(vectors[4:], np.broadcast_to(np.eye(3), (2, 3, 3)))
    assert sorted(map(tuple, gm.regionKeys())) == regions_before == [(0, 0, 0), (1, 0, 0), (3, 0, 0)]
    assert gm.cacheStats() == stats_before
    empty = gm.covarianceEigen((np.zeros((0, 3), dtype=np.int16), np.zeros((0, 3), dtype=np.uint8)))
    assert empty[0].shape == (0, 3) and empty[2].shape == (0,)


def test_refusals(cubic):
    gm, keys = cubic
    with pytest.raises(OhmHipError) as err:
        gm.covarianceEigen((np.zeros((1, 3), dtype=np.int16), np.array([[16, 0, 0]], dtype=np.uint8)))
    assert err.value.status == L.ERR_INVALID_ARG
    plain = GpuMap(OccupancyMap(0.1, (16, 16, 16), layers=("occupancy", "mean")))
    with pytest.raises(OhmHipError) as err:
        plain.covarianceEigen((np.zeros((1, 3), dtype=np.int16), np.zeros((1, 3), dtype=np.uint8)))
    assert err.value.status == L.ERR_UNSUPPORTED
    plain.close()


class DeviceBuffer:
    def __init__(self, nbytes):
        self.handle = L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(self.handle), max(nbytes, 16), 3), "buffer_create")
        self.ptr = L._vp()
        L.check(L.lib.ohmhip_buffer_ptr(self.handle, C.byref(self.ptr)), "buffer_ptr")

    def write(self, array):
        L.check(L.lib.ohmhip_buffer_write(self.handle, array.ctypes.data, array.nbytes, 0, None, None, None), "write")

    def read(self, dtype, shape):
        out = np.zeros(shape, dtype=dtype)
        L.check(L.lib.ohmhip_buffer_read(self.handle, out.ctypes.data, out.nbytes, 0, None, None, None), "read")
        return out

    def close(self):
        L.lib.ohmhip_buffer_destroy(self.handle)


def test_device_variant_equals_host_variant(cubic):
    gm, keys = cubic
    records = np.zeros(keys[0].shape[0] + 2, dtype=GPU_KEY_DTYPE)
    records["region"][:-2], records["voxel"][:-2, :3] = keys[0], keys[1]
    records["region"][-2] = NULL_REGION
    records["region"][-1] = (2, 0, 0)  # absent
    n = records.shape[0]
    host = gm.covarianceEigen(records)
    assert host[2][-2:].tolist() == [0, 0]
    bufs = [DeviceBuffer(10 * n), DeviceBuffer(24 * n), DeviceBuffer(72 * n), DeviceBuffer(n)]
    try:
        bufs[0].write(records)
        L.check(L.lib.ohmhip_map_covariance_eigen_device(gm._handle, *[b.ptr for b in bufs[:1]], n,
                                                         *[b.ptr for b in bufs[1:]]), "device")
        gm.wait()
        assert np.array_equal(bufs[1].read(np.uint64, (n, 3)), host[0].view(np.uint64))
        assert np.array_equal(bufs[2].read(np.uint64, (n, 9)), host[1].reshape(n, 9).view(np.uint64))
        assert np.array_equal(bufs[3].read(np.uint8, (n,)), host[2])
    finally:
        for b in bufs:
            b.close()


def test_region_of_two_chunks(gpu):
    """32 x 32 x 8 voxels: the region spans two 4096-voxel chunks of the read side's work lists."""
    dims = (32, 32, 8)
    map_, gm = ndt_map(dims)
    keys = plant(gm, dims, [(0, 0, 0), (-1, 2, 0)], forced=(0, 4095, 4096, 8191))
    assert_model(gm.covarianceEigen(keys), what="32x32x8")
    gm.close()


def test_tiled_region(gpu):
    """64 x 64 x 16 voxels is a region cut into tiles: keys are the caller's, in region coordinates."""
    dims = (64, 64, 16)
    map_, gm = ndt_map(dims)
    volume = 64 * 64 * 16
    keys = plant(gm, dims, [(0, 0, 0), (1, -1, 0)], forced=(0, volume - 1, 64 * 64 * 8 - 1, 64 * 64 * 8, 64 * 32, 64 * 32 - 1))
    assert gm.cacheStats()["regions_resident"] > len(gm.regionKeys()) == 2  # tiles, not regions, are resident
    assert_model(gm.covarianceEigen(keys), what="tiled")
    gm.close()


def test_spill_to_host_same_bytes(gpu):
    """Regions of the host store answer from their pinned records, and the call leaves the cache counters alone."""
    dims = (16, 16, 16)
    map_, gm = ndt_map(dims, region_capacity=8)
    gm.setMemoryLimit(8 * gm.cacheStats()["bytes_per_region"])
    gm.setSpillToHost(True)
    P = cases.all_p()
    n = P.shape[0]
    region_x = np.arange(n) % 24
    key_regions = np.stack([region_x, np.full(n, 1), np.full(n, -2)], axis=1).astype(np.int16)
    key_locals = locals_of(dims, [(11 + 37 * k) % 4096 for k in range(n)])
    for base in range(0, 24, 8):  # eight regions a call: each call evicts the regions of the one before
        mine = np.flatnonzero((region_x >= base) & (region_x < base + 8))
        assert gm.writeVoxels((key_regions[mine], key_locals[mine]), "covariance", P[mine]) == mine.size
    before = gm.cacheStats()
    assert before["regions_spilled"] >= 16 and len(gm.regionKeys()) == 24
    assert_model(gm.covarianceEigen((key_regions, key_locals)), what="spill")
    assert gm.cacheStats() == before
    gm.close()
