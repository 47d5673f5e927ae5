"""Scenes for the map copy tests (test infrastructure): tests/test_copy_cases.py (CPU) holds the conditions they meet,
tests/test_gpu_copy.py (-m gpu) runs them on the device.

A scene is a fan of a few hundred rays from one sensor position onto a wall; the shapes are the region sizes at which
k_copy_map takes another path: 5 x 3 x 7 (105 voxels: a partial last mask word, blocks that are no multiple of 16 bytes
and start 16-byte aligned in every other slot only), 1 x 1 x 1, the default 32^3, and 40 x 40 x 24 (38 400 voxels: cut
into two tiles).  `fan(shape)` touches at least 8 regions; `fan(shape, scale=0.5)`, the follow-up batch of the replay
tests, leaves at least one of them untouched.

The replay-mask cases plant states into a map the CPU oracle built -- TSDF (weight, distance) pairs from
tests/tsdf_cases.py on voxels the follow-up batch crosses in free space, and NDT means whose sample count is cleared
next to ones that keep theirs on voxels the follow-up batch passes through -- and answer, on the CPU alone, whether the
follow-up batch visits and changes at least one planted voxel of each class."""
import numpy as np

from oracle.oracle import OracleMap
from tsdf_cases import planted_distances, planted_weights

F = np.float32
SENSOR = np.array([0.05, 0.05, 0.05])
SHAPES = {
    "odd": dict(dim=(5, 3, 7), res=0.1, reach=1.5, spread=0.6, step=0.07),
    "unit": dict(dim=(1, 1, 1), res=0.1, reach=0.8, spread=0.3, step=0.06),
    "default": dict(dim=(32, 32, 32), res=0.1, reach=5.0, spread=3.5, step=0.4),
    "tiled": dict(dim=(40, 40, 24), res=0.1, reach=6.0, spread=4.5, step=0.5),
}
FOLLOW_UP_COPIES = 3  # every follow-up ray is presented this often: a voxel it crosses is visited at least that often


def fan(shape, scale=1.0, reach=1.0, origin=(0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0)):
    """(2N, 3) origin / sample pairs: the sensor at SENSOR + origin + shift, samples on the wall x = reach * shape reach."""
    s = SHAPES[shape]
    g = np.arange(-s["spread"] * scale, s["spread"] * scale, s["step"]) + 0.013
    yy, zz = np.meshgrid(g, g, indexing="ij")
    wall = np.stack([np.full(yy.size, s["reach"] * reach), yy.ravel(), zz.ravel()], axis=1)
    rays = np.empty((2 * len(wall), 3))
    rays[0::2] = SENSOR
    rays[1::2] = wall
    return rays + np.asarray(origin, dtype=np.float64) + np.asarray(shift, dtype=np.float64)


def follow_up(shape, extend=1.0, copies=FOLLOW_UP_COPIES):
    """The narrow fan, every ray `copies` times; extend > 1 carries each ray on through its wall point."""
    rays = fan(shape, scale=0.5)
    rays[1::2] = rays[0::2] + extend * (rays[1::2] - rays[0::2])
    return np.concatenate([rays] * copies)


def regions_touched(shape, rays, origin=(0.0, 0.0, 0.0)):
    s = SHAPES[shape]
    om = OracleMap(s["res"], s["dim"], layers=("occupancy",))
    om.set_origin(origin)
    om.integrate_occupancy(rays)
    return set(tuple(int(v) for v in k) for k in om.region_keys())


def ndt_parameters(miss_probability):
    """What GpuNdtMap's constructor sets (ohm/private/NdtMapDetail.h:20-45, ohm/NdtMap.h:146-149)."""
    mp = F(miss_probability)
    return dict(sensor_noise=0.05, sample_threshold=3,
                adaptation_rate=float(F(max(0.0, min(F(2.0) * (F(1.0) - F(2.0) * mp), 1.0)))), reinit_count=100)


def _voxel_index(dim, local):
    return int(local[0]) + dim[0] * (int(local[1]) + dim[1] * int(local[2]))


def _crossings(om, rays, skip_last, copies=1):
    """{(region, voxel index): visits} over the rays' walks, without each walk's last `skip_last` voxels; every ray is
    presented `copies` times."""
    counts = {}
    dim = om.region_dim
    for i in range(0, len(rays), 2):
        keys, _, _ = om.walk(rays[i], rays[i + 1], cap=1 << 10)
        for region, local in keys[:max(0, len(keys) - skip_last)]:
            k = (tuple(int(v) for v in region), _voxel_index(dim, local))
            counts[k] = counts.get(k, 0) + copies
    return counts


TSDF_CLASSES = ("fraction", "above_limit", "off_trunc", "countable", "unobserved")


def tsdf_states(trunc):
    """class -> the (weight, distance) pairs planted for it, from the planted values of tests/tsdf_cases.py."""
    w = [F(x) for x in planted_weights(1e4)]
    d = [F(x) for x in planted_distances(trunc)]
    t = d[0]
    assert t == F(trunc) and F(0.3) in w and F(2.5) in w and F(1e4 + 1) in w and F(2.0 ** 24) in w
    return {
        "fraction": [(F(0.3), t), (F(2.5), t), (F(0.11), t)],   # 0.11f: where n increments and one sum part ways at n = 2
        "above_limit": [(F(1e4 + 1), t), (F(2.0 ** 24), t)],
        "off_trunc": [(F(1.0), d[4]), (F(3.0), d[1]), (F(1.0), d[2]), (F(17.0), d[5]), (F(3.0), d[6])],
        "countable": [(F(1.0), t), (F(3.0), t), (F(17.0), t), (F(1e4), t)],
        "unobserved": [(F(0.0), F(0.0)), (F(-0.0), F(0.0))],
    }


class Planted:
    """chunks: {region: {layer: block}} of the source map with the states planted; voxels: class -> [(region, voxel
    index)]; rays: the follow-up batch; after: the oracle's map after the follow-up batch (under `options`)."""

    def __init__(self, shape, layers, chunks, voxels, rays, after, options):
        self.shape, self.layers, self.chunks, self.voxels, self.rays, self.after, self.options = (
            shape, layers, chunks, voxels, rays, after, options)
        self.region_voxels = int(np.prod(SHAPES[shape]["dim"]))

    def changed(self, result, layer):
        """class -> how many of its planted voxels `result` ({region: {layer: block}}) holds changed in `layer`."""
        out = {}
        for name, where in self.voxels.items():
            n = 0
            for region, vi in where:
                a = np.asarray(self.chunks[region][layer]).view(np.uint8).reshape(self.region_voxels, -1)[vi]
                b = np.asarray(result[region][layer]).view(np.uint8).reshape(self.region_voxels, -1)[vi]
                n += int(not np.array_equal(a, b))
            out[name] = n
        return out


def _copy_chunks(om, layers):
    return {k: {n: v.copy() for n, v in c.items()} for k, c in om.chunks(list(layers)).items()}


def planted_tsdf(shape, src_trunc=0.1, dst_trunc=None):
    """A TSDF map built with src_trunc, states planted on voxels the follow-up batch crosses in free space (FOLLOW_UP_COPIES
    times or more);
    the follow-up batch runs under dst_trunc (default: the same)."""
    dst_trunc = src_trunc if dst_trunc is None else dst_trunc
    s = SHAPES[shape]
    om = OracleMap(s["res"], s["dim"], layers=("tsdf",))
    om.set_tsdf(max_weight=1e4, trunc=src_trunc, dropoff=0.0, sparsity=1.0)
    om.integrate_tsdf(fan(shape))
    rays = follow_up(shape)
    # (free space: four voxels short of the sample is beyond 1.01 * trunc for both distances used)
    crossed = _crossings(om, follow_up(shape, copies=1), skip_last=4, copies=FOLLOW_UP_COPIES)
    regions = set(tuple(int(v) for v in k) for k in om.region_keys())
    sites = sorted(k for k, n in crossed.items() if n >= FOLLOW_UP_COPIES and k[0] in regions)
    states = tsdf_states(src_trunc)
    flat = [(name, st) for name in TSDF_CLASSES for st in states[name]]
    voxels = {name: [] for name in TSDF_CLASSES}
    # spread over the sites: every state lands on several voxels, in several regions
    for i, site in enumerate(sites[::max(1, len(sites) // (8 * len(flat)))]):
        name, (w, d) = flat[i % len(flat)]
        block = om.region_layer_view(site[0], "tsdf").reshape(-1, 2)
        block[site[1]] = (w, d)
        voxels[name].append(site)
    chunks = _copy_chunks(om, ("tsdf",))
    om.set_tsdf(max_weight=1e4, trunc=dst_trunc, dropoff=0.0, sparsity=1.0)
    om.integrate_tsdf(rays)
    return Planted(shape, ("tsdf",), chunks, voxels, rays, _copy_chunks(om, ("tsdf",)),
                   dict(src_trunc=src_trunc, dst_trunc=dst_trunc))


NDT_CLASSES = ("samples", "no_samples")


def planted_ndt(shape, miss_probability):
    """An NDT map built by the oracle; of the voxels that hold samples and that the follow-up batch passes through,
    every second one has its sample count cleared.  The follow-up batch goes through the wall."""
    s = SHAPES[shape]
    layers = ("occupancy", "mean", "covariance")
    om = OracleMap(s["res"], s["dim"], layers=layers)
    params = ndt_parameters(miss_probability)
    om.set_ndt(ndt_tm=False, **params)
    # dense samples on the wall, the wide fan's and the narrow fan's
    first = np.concatenate([fan(shape, scale=c, shift=(0.0, 0.011 * k, 0.007 * k)) for k in range(3) for c in (1.0, 0.5)])
    om.integrate_ndt(first)
    rays = follow_up(shape, extend=1.4)
    crossed = _crossings(om, follow_up(shape, extend=1.4, copies=1), skip_last=1, copies=FOLLOW_UP_COPIES)
    voxels = {name: [] for name in NDT_CLASSES}
    sampled = []
    for (region, vi), n in sorted(crossed.items()):
        mean = om.region_layer_view(region, "mean")
        if mean is not None and mean.reshape(-1, 2)[vi, 1] > 0:
            sampled.append((region, vi))
    for i, (region, vi) in enumerate(sampled):
        if i % 2:
            om.region_layer_view(region, "mean").reshape(-1, 2)[vi, 1] = 0
            voxels["no_samples"].append((region, vi))
        else:
            voxels["samples"].append((region, vi))
    chunks = _copy_chunks(om, layers)
    om.integrate_ndt(rays)
    return Planted(shape, layers, chunks, voxels, rays, _copy_chunks(om, layers), params)
