"""-m gpu: TSDF on uploaded voxels whose weights lie outside what the free-space counting shortcut was argued for.

The device does not replay a visit whose sdf is at least kTsdfFreeMargin (1.01) truncation distances: it counts such
visits and writes (min(w + n, max_weight), trunc).  That is the fixed point of calculateTsdf only while
(sdf + trunc * w) / (w + 1) rounds to no less than trunc and w + 1 + 1 ... equals w + n, which holds for integer weights
up to 1e4 -- the default max_weight, but nothing bounds max_weight or what a host map holds:
  * from w ~ 7e5 on, a visit just past the margin rounds the float32 average one ulp BELOW trunc;
  * from 2^24 on, w + 1 == w on the CPU while w + float(n) still grows;
  * a non-integer weight takes n roundings on the CPU and one in w + float(n).
Each case uploads a slab of (w, trunc) voxels -- what k_rebuild_mask leaves unflagged -- and sends rays ending at many
depths through it.  The CPU side asserts that the oracle itself moves at least one voxel that only saw free-space
visits off (.., trunc), or off w + n, so the case cannot pass by never reaching the edge; the device must then match
the oracle bit for bit, as every TSDF comparison does."""
import numpy as np
import pytest

from ohm_amd import GpuTsdfMap, OccupancyMap
from parity import assert_parity, compare_maps, make_oracle

pytestmark = pytest.mark.gpu

RES = 0.1
TRUNC = 0.3
DIM = (32, 32, 32)
MARGIN = np.float32(1.01) * np.float32(TRUNC)      # kTsdfFreeMargin * trunc, as the device forms it


def slab_rays(om, seed, n=1500):
    """Rays along +x, slightly tilted, from outside region (0, 0, 0) to many depths inside it.  Every second ray is then
    cut so that one voxel of its path sits 1.0101 ... 1.02 truncation distances short of the sample: just past the
    free-space margin, where the excess over trunc is smallest."""
    rng = np.random.default_rng(seed)
    start = np.stack([np.full(n, -1.75), rng.uniform(-1.2, 1.2, n), rng.uniform(-1.2, 1.2, n)], axis=1)
    end = np.stack([rng.uniform(-1.0, 1.5, n), start[:, 1] + rng.uniform(-0.3, 0.3, n),
                    start[:, 2] + rng.uniform(-0.3, 0.3, n)], axis=1)
    for i in range(0, n, 2):
        keys, _, _ = om.walk(start[i], end[i])
        inside = [k for k in keys if k[0] == (0, 0, 0)]
        if len(inside) < 4:
            continue
        direction = (end[i] - start[i]) / np.linalg.norm(end[i] - start[i])
        centre = np.array(om.voxel_centre(*inside[int(rng.integers(len(inside) - 3))]))
        end[i] = start[i] + direction * (np.dot(centre - start[i], direction) + TRUNC * rng.uniform(1.0101, 1.02))
    rays = np.empty((2 * n, 3))
    rays[0::2], rays[1::2] = start, end
    return rays


def sdf_of(sensor, sample, centre):
    """ohm/VoxelTsdfCompute.h:57-68, rounding where it rounds."""
    to_voxel, to_sample = centre - sensor, sample - sensor
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
    distance_g = np.float32(np.sqrt(dot(to_sample, to_sample)))
    return distance_g - np.float32(dot(to_voxel, to_sample)) / distance_g


def free_space_only(om, rays):
    """Voxel index -> visits, for voxels of region (0, 0, 0) all of whose visits lie past the free-space margin."""
    visits, near = {}, set()
    for i in range(0, len(rays), 2):
        keys, _, _ = om.walk(rays[i], rays[i + 1])
        for region, local in keys:
            if region != (0, 0, 0):
                continue
            vi = local[0] + DIM[0] * (local[1] + DIM[1] * local[2])
            centre = np.array(om.voxel_centre(region, local))
            if sdf_of(rays[i], rays[i + 1], centre) < MARGIN:
                near.add(vi)
            visits[vi] = visits.get(vi, 0) + 1
    return {vi: n for vi, n in visits.items() if vi not in near}


CASES = {
    # name: (weights of the slab, max_weight)
    "w_5e5_1e6": (lambda rng, n: np.floor(rng.uniform(5e5, 1e6, n)), 2e6),
    "w_from_2_24": (lambda rng, n: 2.0 ** 24 + 2.0 * np.floor(rng.uniform(0, 1000, n)), 1e8),
    "w_fractional": (lambda rng, n: rng.uniform(0.05, 40.0, n), 1e4),
    "w_above_max": (lambda rng, n: np.floor(rng.uniform(5e5, 1e6, n)), 1e4),
}


@pytest.mark.parametrize("name", list(CASES))
def test_uploaded_weights_beyond_the_counting_argument(gpu, name):
    weights, max_weight = CASES[name]
    rng = np.random.default_rng(17)
    volume = DIM[0] * DIM[1] * DIM[2]
    tile = np.empty(2 * volume, dtype=np.float32)
    tile[0::2] = weights(rng, volume).astype(np.float32)
    tile[1::2] = np.float32(TRUNC)
    map_ = OccupancyMap(RES, DIM, layers=("tsdf",))
    om = make_oracle(map_)
    rays = slab_rays(om, 23)
    om.set_tsdf(max_weight=max_weight, trunc=TRUNC, dropoff=0.0, sparsity=1.0)
    centre = np.array(om.voxel_centre((0, 0, 0), (16, 16, 16)))
    om.integrate_tsdf(np.array([centre, centre]))              # creates region (0, 0, 0); overwritten next
    om.region_layer_view((0, 0, 0), "tsdf")[:] = tile
    free = free_space_only(om, rays)
    om.integrate_tsdf(rays)
    after = om.region_layer((0, 0, 0), "tsdf")

    # the CPU side reaches the edge: a voxel that only saw free-space visits is NOT at (min(w + n, max), trunc)
    off = 0
    for vi, n in free.items():
        counted = min(np.float32(tile[2 * vi] + np.float32(n)), np.float32(max_weight))
        off += int(after[2 * vi + 1] != np.float32(TRUNC) or after[2 * vi] != counted)
    print("%s: %d voxels with free-space visits only, %d of them off the counting shortcut's answer" % (
        name, len(free), off))
    assert len(free) > 1000
    assert off >= 1, "the oracle never leaves the counting shortcut's answer: the case does not reach its edge"

    map_.chunks[(0, 0, 0)] = {"tsdf": tile.copy()}
    gm = GpuTsdfMap(map_, max_weight=max_weight, default_truncation_distance=TRUNC)
    gm.setBatchCoalescing(0)
    half = rays.shape[0] // 4 * 2
    assert gm.integrateRays(rays[:half]) == half                # two device batches: the second starts from device state
    assert gm.integrateRays(rays[half:]) == rays.shape[0] - half
    gm.syncVoxels()
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["tsdf"], exact_float=True))
    gm.close()
