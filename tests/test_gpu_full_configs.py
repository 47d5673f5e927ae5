"""-m gpu: the BASELINE.json configurations at FULL size.

C1 (1 M lidar rays, 0.1 m) and C2 (NDT, 1 M rays, 0.2 m) are compared voxel-for-voxel with the CPU oracle (a few
seconds of CPU each).  C3 (TSDF, 0.05 m, 4 M rays, 2.7 x 10^9 voxel visits) is compared voxel-for-voxel with the oracle
too (about a minute of CPU) and additionally checked through size-independent properties: the exact voxel-visit count
(closed form from the voxel keys), and batch-split invariance (integrating in one call or in four must give
bit-identical maps because the device applies every voxel's events in ray order)."""
import numpy as np
import pytest

from ohm_amd import GpuMap, GpuNdtMap, GpuTsdfMap, OccupancyMap, synth

from parity import assert_parity, compare_maps, make_oracle

pytestmark = pytest.mark.gpu


def expected_visits(rays, resolution, include_end):
    """Sum over rays of (Manhattan voxel distance + 1): what the CPU walk reports (ohm/LineWalkCompute.h:345-413)."""
    g = np.floor(rays / resolution).astype(np.int64)  # map origin 0: global voxel coordinate (ohm/MapCoord.h)
    manhattan = np.abs(g[1::2] - g[0::2]).sum(axis=1)
    return int(manhattan.sum() + (len(manhattan) if include_end else len(manhattan)))


def test_c1_occupancy_full_vs_oracle(gpu):
    rays = synth.rays_c1()
    map_ = OccupancyMap(0.1)
    gm = GpuMap(map_, gpu_mem_size=2 << 30)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    st = gm.stats()
    assert st["voxel_visits"] == expected_visits(rays, 0.1, False)
    om = make_oracle(map_)
    om.integrate_occupancy(rays)
    assert om.visit_count() == st["voxel_visits"]
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy"], exact_float=True))


def test_c2_ndt_full_vs_oracle(gpu):
    rays = synth.rays_c2()
    map_ = OccupancyMap(0.2)
    gm = GpuNdtMap(map_, gpu_mem_size=4 << 30)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    om = make_oracle(map_)
    om.set_ndt(adaptation_rate=gm.adaptation_rate)
    om.integrate_ndt(rays)
    assert om.visit_count() == gm.stats()["voxel_visits"]
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy", "mean", "covariance"], rel=1e-5))


def test_c3_tsdf_full_vs_oracle_and_properties(gpu):
    rays = synth.rays_c3()
    assert rays.shape[0] == 8_000_000
    # full size, one call: bit exact against the CPU oracle, visit count equal to the closed form
    map_a = OccupancyMap(0.05, layers=("tsdf",))
    gm_a = GpuTsdfMap(map_a, gpu_mem_size=16 << 30)
    assert gm_a.integrateRays(rays) == rays.shape[0]
    assert gm_a.stats()["voxel_visits"] == expected_visits(rays, 0.05, True)
    gm_a.syncVoxels()
    gm_a.close()
    om = make_oracle(map_a)
    om.integrate_tsdf(rays)
    assert om.visit_count() == expected_visits(rays, 0.05, True)
    assert_parity(compare_maps(om.chunks(), map_a.chunks, ["tsdf"], exact_float=True))
    del om
    # one call vs four calls must agree bit for bit
    map_b = OccupancyMap(0.05, layers=("tsdf",))
    gm_b = GpuTsdfMap(map_b, gpu_mem_size=16 << 30)
    for i in range(0, rays.shape[0], 2_000_000):
        assert gm_b.integrateRays(rays[i:i + 2_000_000]) == 2_000_000
    gm_b.syncVoxels()
    gm_b.close()
    assert set(map_a.chunks) == set(map_b.chunks)
    for key, layers in map_a.chunks.items():
        assert np.array_equal(layers["tsdf"].view(np.uint32), map_b.chunks[key]["tsdf"].view(np.uint32))
    w = np.concatenate([c["tsdf"].reshape(-1, 2)[:, 0] for c in map_a.chunks.values()])
    d = np.concatenate([c["tsdf"].reshape(-1, 2)[:, 1] for c in map_a.chunks.values()])
    assert w.max() <= 1e4 and np.all(np.abs(d) <= np.float32(0.1))


def test_c4_shards_one_call_of_4m_rays_equals_four_calls(gpu):
    """C4's ray sets (one sensor origin per shard): four shards through ONE map in a single 4 M-ray call and in four
    1 M-ray calls.  Size-independent properties at a size the oracle is too slow for: the exact visit count and
    bit-identical maps whatever the batch split (every voxel's events are applied in ray order)."""
    shards = [synth.rays_c4_shard(r, n=1_000_000) for r in range(4)]
    rays = np.concatenate(shards)
    layers = ("occupancy", "mean")
    one, four = OccupancyMap(0.1, layers=layers), OccupancyMap(0.1, layers=layers)
    g1 = GpuMap(one, gpu_mem_size=8 << 30)
    g4 = GpuMap(four, gpu_mem_size=8 << 30)
    assert g1.integrateRays(rays) == rays.shape[0]
    visits = g1.stats()["voxel_visits"]
    total4 = 0
    for s in shards:
        assert g4.integrateRays(s) == s.shape[0]
        total4 += g4.stats()["voxel_visits"]
    # (the closed form of expected_visits() does not apply: these sensor origins sit exactly on voxel boundaries, where
    # ohm's region / local key arithmetic and a plain floor(p / res) round differently)
    assert visits == total4 and visits > 10 ** 9
    g1.syncVoxels()
    g4.syncVoxels()
    assert set(one.chunks) == set(four.chunks) and len(one.chunks) > 3000
    for key, c in one.chunks.items():
        for name in layers:
            assert np.array_equal(c[name].view(np.uint32), four.chunks[key][name].view(np.uint32)), (key, name)


def test_c4_shard_origin_on_voxel_boundaries_matches_oracle(gpu):
    """The C4 sensor origins (-60, -20, ...) sit exactly on voxel and region boundaries: ohm's key arithmetic
    (region = floor(p / R + 0.5), local = floor((p - region_min) / res) with its 1e-6 edge fix-ups, ohm/MapCoord.h:45-93)
    decides which voxel such a point belongs to, and the device has to decide the same way."""
    for shard in (0, 5):
        rays = synth.rays_c4_shard(shard, n=30000)
        map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
        gm = GpuMap(map_)
        assert gm.integrateRays(rays) == rays.shape[0]
        gm.syncVoxels()
        om = make_oracle(map_)
        om.integrate_occupancy(rays)
        assert om.visit_count() == gm.stats()["voxel_visits"]
        assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy", "mean"], exact_float=True))


def test_c0_100k_uniform_10m_rays_vs_oracle(gpu):
    """BASELINE configs[0] on its own rays: 100 k uniform 10 m rays from one origin, 0.1 m voxels, 32^3 regions."""
    rays = synth.rays_c0()
    assert rays.shape[0] == 200_000
    map_ = OccupancyMap(0.1, layers=("occupancy", "mean"))
    gm = GpuMap(map_)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.syncVoxels()
    om = make_oracle(map_)
    om.integrate_occupancy(rays)
    assert om.visit_count() == gm.stats()["voxel_visits"] == expected_visits(rays, 0.1, False)
    assert_parity(compare_maps(om.chunks(), map_.chunks, ["occupancy", "mean"], exact_float=True))


def test_c4_full_8_shards_owner_computes_and_replica_merge(gpu):
    """BASELINE configs[4] at full size on the one test GPU: 8 x 1 M rays from 8 sensor origins.

    (1) ONE map integrating the 8 shards in rank order -- the sequential result, checked against the CPU oracle on a
        100 k-ray-per-shard subsample integrated the same way (bit exact);
    (2) PARTITIONED MAP, the mode `bench.py --gpus N` runs: 8 maps standing in for 8 ranks, each owning the territory
        around its sensor origin; every shard is routed by the library's kernels, the destination blocks are
        re-assembled in (source rank, ray) order and each map integrates what is addressed to it -> the union of the
        territories is BIT-IDENTICAL to (1) (no tolerance), only a fraction of the rays travels;
    (3) owner computes with the whole stream on every rank (the round-2 mode): bit-identical to (1) too;
    (4) the OPTIONAL replica merge (additive delta all-reduce; bench.py --multi-gpu-mode replica-merge): every exchanged
        region bit-identical on all replicas, and its deviation from (1) COUNTED -- the additive rule is exact only where
        no clamp engaged between the shards, which is why it is not the default (state it with the results)."""
    from ohm_amd import _lib as L
    from ohm_amd import distributed as D
    n = 1_000_000
    shards = [synth.rays_c4_shard(r, n=n) for r in range(8)]
    # (1) sequential, full size
    seq_map = OccupancyMap(0.1, layers=("occupancy",))
    seq = GpuMap(seq_map, gpu_mem_size=16 << 30)
    for s in shards:
        assert seq.integrateRays(s) == s.shape[0]
    seq.syncVoxels()
    seq.close()
    # ... and the same at 100 k rays per shard against the oracle
    sub_map = OccupancyMap(0.1, layers=("occupancy",))
    sub = GpuMap(sub_map, gpu_mem_size=4 << 30)
    om = make_oracle(sub_map)
    for r in range(8):
        part = synth.rays_c4_shard(r, n=100_000)
        assert sub.integrateRays(part) == part.shape[0]
        om.integrate_occupancy(part)
    sub.syncVoxels()
    sub.close()
    assert_parity(compare_maps(om.chunks(), sub_map.chunks, ["occupancy"], exact_float=True))
    del om, sub_map
    # (2) partitioned map with routed rays: 8 territories, exact
    part0 = D.territories_from_origins(synth.C4_ORIGINS, 8, 0, 3.2, block_shift=1, margin=40.0)
    pmaps = [OccupancyMap(0.1, layers=("occupancy",)) for _ in range(8)]
    pgs = [GpuMap(m, gpu_mem_size=2 << 30) for m in pmaps]
    for r, g in enumerate(pgs):
        g.setRegionPartition(part0.with_rank(r))
    info = D.integrate_partitioned_in_process(pgs, shards)
    routed = info["routed"]
    travelled = int(routed.sum() - np.trace(routed))
    print("C4 partitioned: rays sent to other ranks per rank", [int(routed[r].sum() - routed[r, r]) for r in range(8)])
    assert all(routed[r, r] == n for r in range(8)), "every ray touches its own sensor's territory"
    assert 0 < travelled < 8 * n // 2, "only the rays reaching into a neighbour's territory travel"
    union = {}
    for r, (m, g) in enumerate(zip(pmaps, pgs)):
        g.syncVoxels()
        g.close()
        keys = np.array(sorted(m.chunks), dtype=np.int16).reshape(-1, 3)
        assert np.all(part0.owners(keys) == r)
        for k, c in m.chunks.items():
            assert k not in union
            union[k] = c
    assert set(union) == set(seq_map.chunks) and len(union) > 5000
    dev = D.merge_deviation(union, seq_map.chunks)
    assert dev["voxels_state_differs"] == 0 and dev["voxels_value_differs"] == 0 and dev["voxels_beyond_rel"] == 0
    for k, c in seq_map.chunks.items():
        assert np.array_equal(c["occupancy"].view(np.uint32), union[k]["occupancy"].view(np.uint32)), k
    del union, pmaps
    # (3) owner computes, 8 maps, the whole stream each
    stream = np.concatenate(shards)
    owned = {}
    for rank in range(8):
        m = OccupancyMap(0.1, layers=("occupancy",))
        g = GpuMap(m, gpu_mem_size=4 << 30)
        g.setRegionOwnership(8, rank, 0)
        for i in range(0, stream.shape[0], 2 * n):  # the same 1 M-ray batches as (1)
            assert g.integrateRays(stream[i:i + 2 * n]) == 2 * n
        g.syncVoxels()
        g.close()
        keys = np.array(sorted(m.chunks), dtype=np.int16).reshape(-1, 3)
        assert np.all(D.region_owner(keys, 8, 0) == rank)
        for k, c in m.chunks.items():
            assert k not in owned
            owned[k] = c
    del stream
    assert set(owned) == set(seq_map.chunks) and len(owned) > 5000
    for k, c in seq_map.chunks.items():
        assert np.array_equal(c["occupancy"].view(np.uint32), owned[k]["occupancy"].view(np.uint32)), k
    del owned
    # (4) replica merge (optional mode)
    maps = [OccupancyMap(0.1, layers=("occupancy",)) for _ in range(8)]
    gms = [GpuMap(m, gpu_mem_size=2 << 30) for m in maps]
    for g, s in zip(gms, shards):
        L.check(L.lib.ohmhip_map_enable_merge(g._handle), "enable_merge")
        assert g.integrateRays(s) == s.shape[0]
    shared, stats = D.merge_in_process(gms)
    assert stats["regions_shared"] == len(shared) > 500 and stats["regions_union"] == len(seq_map.chunks)
    keys = [tuple(k) for k in shared.tolist()]
    for g in gms:
        g.syncVoxels()
        g.close()
    for k in keys:  # every replica holds every exchanged region, bit-identical
        for m in maps[1:]:
            assert np.array_equal(maps[0].chunks[k]["occupancy"].view(np.uint32), m.chunks[k]["occupancy"].view(np.uint32))
    dev = D.merge_deviation(maps[0].chunks, seq_map.chunks, keys=keys)
    print("C4 replica merge vs sequential:", dev, stats)
    assert dev["regions_compared"] == len(keys) and dev["voxels_state_differs"] == 0
    # the statement, as measured (0.7 % of the observed voxels of the overlap beyond 1e-5: clamp interplay; the rest
    # agree to float summation order) -- the reason this mode is optional and the partitioned map of (2) is the default
    assert 0 < dev["voxels_beyond_rel"] <= 0.02 * dev["voxels_observed"]
    # regions only one shard touched are exact on that replica
    shared_set = set(keys)
    for r, m in enumerate(maps):
        for k, c in m.chunks.items():
            if k not in shared_set:
                assert np.array_equal(c["occupancy"].view(np.uint32), seq_map.chunks[k]["occupancy"].view(np.uint32)), (r, k)


def _run_bench_gpus_2(extra_args=()):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--rays", "200000", "--full"] + list(extra_args), env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks"] == 2 and line["devices_visible"] >= 1
    assert line["value"] > 0 and line["config"]["rays_per_step_per_gpu"] == 200000
    return line


def test_bench_gpus_2_launches_two_ranks_on_the_one_gpu(gpu):
    """`python bench.py --gpus 2` (no launcher environment): two ranks are started, share the one GPU (gloo control plane,
    routed rays staged through the host), and the line reports n_gpus = 2 with the partitioned map's statistics and its
    deviation from sequential integration: none."""
    line = _run_bench_gpus_2()
    mg = line["multi_gpu"]
    assert "partitioned" in mg["mode"] and mg["per_step_this_rank"]["rays_sent_to_other_ranks"] > 0
    dev = mg["deviation"]
    assert "error" not in dev, dev
    assert dev["regions_compared"] == dev["regions_sequential"] > 0
    for key in ("voxels_state_differs", "voxels_value_differs", "voxels_beyond_rel", "regions_missing",
                "regions_outside_their_territory"):
        assert dev[key] == 0, (key, dev)


def test_bench_gpus_2_replica_merge_mode(gpu):
    """The optional replica-merge mode of the same launcher: merge statistics and the COUNTED deviation."""
    line = _run_bench_gpus_2(["--multi-gpu-mode", "replica-merge"])
    assert "error" not in line["merge"], line["merge"]
    assert line["merge"]["per_step"]["regions_union"] >= line["merge"]["per_step"]["regions_local"] > 0
    dev = line["merge"]["deviation"]
    assert "error" not in dev and dev["regions_compared"] > 0 and dev["voxels_state_differs"] == 0
