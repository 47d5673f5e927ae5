"""-m gpu: the sample-side secondary layers -- incident normal and touch time -- at their edges, on the constructed set of
tests/secondary_cases.py: the decoder's NaN branch, rays about the 1e-6 squared-length tests, opposing pairs, samples
2 000 m out, stamps that do not rise with the ray index, lie before the map's time base or more than 2^32 ms after it.
All three update sites (the occupancy apply pass, the NDT replay, the stop-on-first-occupied replay), with and without a
mean layer, with and without traversal beside them, plain and tiled regions, one call / calls of 97 rays / the same
without batch coalescing, the built-in filters and a host filter that moves starts and rejects the first stamped ray.
Expected values: the CPU oracle fed the same calls (its incident and touch-time leaves are pinned to the reference header
by tests/test_oracle_golden_incident.py).  touch_time, incident_normal, mean: bit exact; occupancy: bit exact for GpuMap,
1e-5 for NDT; traversal: the bar of tests/test_gpu_secondary.py; firstRayTime() equals the oracle's after the calls."""
import numpy as np
import pytest

from ohm_amd import GpuMap, GpuNdtMap, NdtMode, OccupancyMap, RayFlag
from ohm_amd import rayfilter as RF

from parity import assert_parity, compare_maps, make_oracle
import secondary_cases as S

pytestmark = pytest.mark.gpu

STOP = int(RayFlag.kRfStopOnFirstOccupied)


@pytest.fixture(scope="module")
def cs():
    return S.cases()


def _intensities(n):
    return (10.0 + (np.arange(n) % 37)).astype(np.float32)


class _Pair:
    """A device map of one site and the oracle beside it, fed the same calls."""

    def __init__(self, site, mean=True, traversal=False, region=32, coalesce=True, builtin_filter=None):
        layers = ["occupancy"] + (["mean"] if mean else []) + (["traversal"] if traversal else []) + \
            ["touch_time", "incident_normal"]
        self.site, self.flags = site, (STOP if site == "stop" else 0)
        self.map = OccupancyMap(S.RESOLUTION, (region,) * 3, layers=layers)
        if builtin_filter:
            self.map.ray_filter = builtin_filter
        if site.startswith("ndt"):
            mode = NdtMode.kTraversability if site == "ndt_tm" else NdtMode.kOccupancy
            self.gm = GpuNdtMap(self.map, ndt_mode=mode)
        else:
            self.gm = GpuMap(self.map)
        self.om = make_oracle(self.map)
        if site.startswith("ndt"):
            gm = self.gm
            self.om.set_ndt(sensor_noise=gm.sensor_noise, sample_threshold=gm.sample_threshold,
                            adaptation_rate=gm.adaptation_rate, reinit_threshold=gm.reinitialise_covariance_threshold,
                            reinit_count=gm.reinitialise_covariance_point_count, ndt_tm=(site == "ndt_tm"))
        if not coalesce:
            self.gm.setBatchCoalescing(0)
        self.coalesce = coalesce
        self.calls = 0
        self.host_filter = None

    def set_host_filter(self, filt):
        self.host_filter = filt
        self.gm.setRayFilter(filt)

    def integrate(self, rays, stamps):
        ints = _intensities(len(stamps)) if self.site == "ndt_tm" else None
        kept, kstamps, kints, fflags = rays, stamps, ints, None
        if self.host_filter is not None:
            # what the reference does: the time base is the first stamp of the call as submitted (ohmgpu/GpuMap.cpp:593),
            # the mapper then sees the rays its filter kept
            if self.om.first_ray_time() < 0:
                self.om.set_first_ray_time(stamps[0])
            keep, starts, ends, flags = self.host_filter(rays[0::2].copy(), rays[1::2].copy())
            kept = np.empty((2 * int(keep.sum()), 3))
            kept[0::2], kept[1::2] = starts[keep], ends[keep]
            kstamps, fflags = stamps[keep], flags[keep]
            kints = None if ints is None else ints[keep]
        got = self.gm.integrateRays(rays, intensities=ints, timestamps=stamps, ray_update_flags=self.flags)
        if self.host_filter is not None:
            assert got == kept.shape[0]
        elif self.map.ray_filter is None:
            assert got == rays.shape[0]
        if kept.shape[0]:
            if self.site.startswith("ndt"):
                self.om.integrate_ndt(kept, intensities=kints, timestamps=kstamps, flags=self.flags, filter_flags=fflags)
            else:
                self.om.integrate_occupancy(kept, timestamps=kstamps, flags=self.flags, filter_flags=fflags)
        self.calls += 1
        # (reading the time base settles the map, which launches what batch coalescing holds back: with coalescing on it
        # is read after the first call and then every eighth, so that calls do share device batches)
        if not self.coalesce or self.calls == 1 or self.calls % 8 == 0:
            assert self.gm.firstRayTime() == self.om.first_ray_time()

    def integrate_set(self, cs, call_size, order=None):
        order = np.arange(cs.n_rays) if order is None else order
        for sl in cs.calls(call_size):
            idx = order[sl]
            rays = np.empty((2 * len(idx), 3))
            rays[0::2], rays[1::2] = cs.rays[0::2][idx], cs.rays[1::2][idx]
            self.integrate(rays, cs.stamps[idx])

    def check(self):
        assert self.gm.firstRayTime() == self.om.first_ray_time()
        self.gm.syncVoxels()
        cpu = self.om.chunks()
        names = [n for n in ("occupancy", "mean", "touch_time", "incident_normal") if n in self.map.layers]
        if self.site.startswith("ndt"):
            assert_parity(compare_maps(cpu, self.map.chunks, names, rel=1e-5))  # integer layers: bit exact
        else:
            assert_parity(compare_maps(cpu, self.map.chunks, names, exact_float=True))
        touched = sum(int(np.count_nonzero(c["incident_normal"])) for c in cpu.values())
        if "traversal" in self.map.layers:
            worst = 0.0
            for key, layers in cpu.items():
                g, c = self.map.chunks[key]["traversal"], layers["traversal"]
                assert np.array_equal(c != 0, g != 0)
                nz = c != 0
                if nz.any():
                    worst = max(worst, float(np.max(np.abs(g[nz] - c[nz]) / np.maximum(np.abs(c[nz]), 1e-3))))
            assert worst < 1e-5, worst
        return touched


BATCHING = {"one_call": (None, True), "calls_of_97": (97, True), "calls_of_97_uncoalesced": (97, False)}


def _cases_matrix():
    out = []
    for batching in BATCHING:
        for traversal in (False, True):
            for site in ("occ", "stop"):
                for mean in (True, False):
                    out.append((site, mean, traversal, 32, batching))
            for site in ("ndt_om", "ndt_tm"):
                out.append((site, True, traversal, 32, batching))
        # regions cut into tiles (more than 32768 voxels)
        out.append(("occ", True, False, 64, batching))
        out.append(("occ", False, True, 64, batching))
        out.append(("ndt_om", True, False, 64, batching))
    return out


@pytest.mark.parametrize("site,mean,traversal,region,batching", _cases_matrix())
def test_sites_layers_regions_batching(gpu, cs, site, mean, traversal, region, batching):
    call_size, coalesce = BATCHING[batching]
    pair = _Pair(site, mean=mean, traversal=traversal, region=region, coalesce=coalesce)
    pair.integrate_set(cs, call_size)
    if site == "stop":
        # second pass: rays crossing a now-occupied target stop there and must leave no sample-side update
        before = pair.om.visit_count()
        pair.integrate_set(cs, call_size)
        assert pair.om.visit_count() - before < before
    assert pair.check() >= 400  # sample voxels holding a normal


def _lengths(cs):
    d = cs.rays[1::2] - cs.rays[0::2]
    return np.sqrt((d * d).sum(axis=1))


@pytest.mark.parametrize("site", ["occ", "stop", "ndt_om"])
@pytest.mark.parametrize("mode", ["good", "clip"])
def test_builtin_filters(gpu, cs, site, mode):
    r = 0.9
    assert np.count_nonzero(_lengths(cs) > r) >= 0.10 * cs.n_rays  # dropped, respectively clipped
    # (no traversal layer here: a ray clipped at r leaves an exit range of r behind, which the reference's mapper hands
    # to a following ray that walks no voxel -- the set's sub-voxel rays -- as its `last_exit_range`; that sample then adds
    # length - r, about -0.9, to a voxel holding +0.9, and the float32 sum of the two, in whatever order, is only good to
    # 6e-8: 1.1e-5 of the 0.005 m that remain.  That is the reference's own rounding, and traversal's accumulation is
    # not what this file is about; the sites above run with the layer.)
    pair = _Pair(site, coalesce=False, builtin_filter=(mode, r))
    pair.integrate_set(cs, 97)
    assert pair.check() >= 200


def _chain(first, second):
    """Two RayFilterFunctions one after the other, as a caller of the reference composes them in one callable."""
    def f(starts, ends):
        keep_a, starts, ends, flags_a = first(starts, ends)
        keep_b, starts, ends, flags_b = second(starts, ends)
        return keep_a & keep_b, starts, ends, flags_a | flags_b
    return f


def _host_filter():
    # clipBounded alone rejects a ray only when clipping leaves both ends off the box (ohm/RayFilter.cpp:60-77); the
    # rejections come from goodRayFilter in front of it.  The box hugs the targets of the region at the origin: rays into
    # it start outside and are clipped at its faces.  The faces lie inside voxels, not on voxel walls: a start clipped
    # onto a wall opens with a visit some 1e-16 m long, which the reference adds to its float and the device's traversal
    # tile, counting units of 2^-28 m, rounds to nothing -- 99 voxels of the set would then differ in "is it zero", which is
    # the tile's documented unit and not what this file is about.
    box = RF.Aabb((-1.33, -1.33, -1.17), (-0.13, -0.13, 0.93))
    return _chain(RF.good_ray_filter(1.2), RF.clip_bounded(box))


@pytest.mark.parametrize("site,mean,traversal", [("occ", True, False), ("occ", False, True), ("stop", True, False),
                                                 ("ndt_om", True, False), ("ndt_tm", True, True)])
def test_host_filter_moves_starts_and_rejects_the_first_ray(gpu, cs, site, mean, traversal):
    filt = _host_filter()
    order = np.roll(np.arange(cs.n_rays), -1)  # the set from its second ray on, the first one last
    starts, ends = cs.rays[0::2][order], cs.rays[1::2][order]
    keep, new_starts, _ends, flags = filt(starts.copy(), ends.copy())
    moved = keep & np.any(new_starts != starts, axis=1)
    assert np.count_nonzero(moved) >= 0.10 * cs.n_rays and np.all(flags[moved] & RF.kRffClippedStart)
    assert np.count_nonzero(~keep) >= 0.05 * cs.n_rays
    assert not keep[0]  # the very first ray of the map's first stamped call is rejected ...
    assert cs.stamps[order[0]] != cs.stamps[order[np.nonzero(keep)[0][0]]]  # ... and the first kept one is stamped otherwise
    pair = _Pair(site, mean=mean, traversal=traversal, coalesce=False)
    pair.set_host_filter(filt)
    pair.integrate_set(cs, 97, order=order)
    assert pair.gm.firstRayTime() == cs.stamps[order[0]]
    assert pair.check() >= 200


@pytest.mark.parametrize("site", ["occ", "ndt_om"])
def test_first_call_with_every_ray_rejected(gpu, cs, site):
    filt = _host_filter()
    keep, _s, _e, _f = filt(cs.rays[0::2].copy(), cs.rays[1::2].copy())
    rejected = np.nonzero(~keep)[0][:40]
    pair = _Pair(site, coalesce=False)
    pair.set_host_filter(filt)
    rays = np.empty((2 * len(rejected), 3))
    rays[0::2], rays[1::2] = cs.rays[0::2][rejected], cs.rays[1::2][rejected]
    pair.integrate(rays, cs.stamps[rejected])  # integrates nothing, and still sets the map's time base
    assert pair.gm.firstRayTime() == cs.stamps[rejected[0]] != cs.stamps[0]
    pair.integrate_set(cs, 97)
    assert pair.check() >= 200
