#!/usr/bin/env python
"""bench.py -- headline benchmark: rays/s integrated by the HIP occupancy path (BASELINE.json configs[1]) + roofline.

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A plain run sets up, warms up, times the K steps and prints the headline line.  `--full` adds everything else the
line can carry (CPU baseline, other_configs, first_pass, moving_sensor, the device-copy ceiling, at N > 1 the deviation
from sequential integration).  `--dump-outputs DIR` writes what the timed steps computed to DIR/*.npy (dump_outputs).

One "step" = one GpuMap::integrateRays pass over one 1 M-ray synthetic lidar batch (C1) whose rays are already
resident in HBM when the timed region starts.  At N > 1 -- launched by torch.distributed.run, one rank per GPU, or,
when `--gpus N` is given WITHOUT a torch.distributed environment, re-launched by this script itself under
torch.distributed.run (127.0.0.1 rendezvous) -- every rank integrates the C4 shard of its own sensor origin into its own resident map and, inside the timed region, the
replicas are reconciled after every batch: the library's replica merge (include/ohmhip.h) all-gathers the region key
lists and all-reduces, over RCCL, the occupancy deltas of the regions more than one rank touched ("weak" scaling);
value = rays of all ranks / max-over-ranks time, bytes moved are reported under "merge".

Prints ONE JSON line on rank 0.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s measured achievable


def _oracle_rate(rays, resolution, repeats=3):
    from oracle.oracle import OracleMap
    best, om = None, None
    for _ in range(repeats):
        om = OracleMap(resolution, (32, 32, 32), layers=("occupancy",))
        t0 = time.perf_counter()
        om.integrate_occupancy(rays)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, om.visit_count()


def _cpu_replica_worker(args):
    """One of P processes of the all-cores leg: its own oracle map, its own slice of the C1 batch ("replicas": the CPU
    mapper is single threaded, ohm/RayMapperOccupancy.cpp, so the only way to use P cores is P independent maps)."""
    index, n_rays, resolution, start_at = args
    from oracle.oracle import OracleMap
    from ohm_amd import synth as S  # numpy only; no device call
    rays = S.rays_c1(n=n_rays, first=index * n_rays)
    om = OracleMap(resolution, (32, 32, 32), layers=("occupancy",))
    while time.time() < start_at:  # common start so the replicas really run side by side
        time.sleep(0.001)
    t0 = time.time()
    om.integrate_occupancy(rays)
    return t0, time.time(), om.visit_count()


def _physical_cores():
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            try:  # respect a cgroup / affinity restriction
                return max(1, min(n, len(os.sched_getaffinity(0))))
            except AttributeError:
                return n
    except Exception:
        pass
    return max(1, (os.cpu_count() or 2) // 2)


def cpu_baseline(rays, resolution, sample_rays, all_cores=True):
    """The oracle (bit-identical CPU port of RayMapperOccupancy, kind "port") timed on the host cores, bounded samples:
      value      single thread, the first `sample_rays` rays of the SAME C1 batch the GPU integrates (headline figure);
      c0         single thread on BASELINE config 0's own rays (100 k uniform 10 m rays from one origin);
      all_cores  P = physical cores, P processes each integrating its own slice of the C1 sweep into its own map
                 ("replicas"), rays of all / (latest end - earliest start)."""
    from ohm_amd import synth
    sample = rays[: 2 * sample_rays]
    best, visits = _oracle_rate(sample, resolution)
    out = {"value": sample_rays / best, "unit": "rays/s", "cores": 1, "kind": "port",
           "sample": f"first {sample_rays} rays of the same C1 batch, fresh map, best of 3, {best:.2f} s",
           "visits_per_s": visits / best}
    c0 = synth.rays_c0()
    best0, visits0 = _oracle_rate(c0, resolution)
    out["c0"] = {"value": (c0.shape[0] // 2) / best0, "unit": "rays/s", "cores": 1, "visits_per_s": visits0 / best0,
                 "sample": f"C0: {c0.shape[0] // 2} uniform 10 m rays from one origin, 0.1 m voxels, fresh map, best of 3, "
                           f"{best0:.2f} s"}
    if all_cores:
        try:
            import multiprocessing as mp
            procs = _physical_cores()
            per = max(50_000, min(250_000, sample_rays // 4))
            start_at = time.time() + 4.0 + 0.02 * procs  # interpreter start + ray generation of every worker
            with mp.get_context("spawn").Pool(procs) as pool:
                res = pool.map(_cpu_replica_worker, [(i, per, resolution, start_at) for i in range(procs)], chunksize=1)
            late = sum(1 for r in res if r[0] > start_at + 0.25)
            wall = max(r[1] for r in res) - min(r[0] for r in res)
            out["all_cores"] = {"value": procs * per / wall, "unit": "rays/s", "cores": procs, "kind": "port",
                                "visits_per_s": sum(r[2] for r in res) / wall, "late_starters": late,
                                "sample": f"{procs} replica processes x {per} rays of the C1 sweep each, own map each, "
                                          f"{wall:.2f} s wall"}
        except Exception as exc:  # never lose the bench line over a secondary figure
            out["all_cores"] = {"error": repr(exc)}
    return out


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _relaunch_ranks(n):
    """`python bench.py --gpus N` with no torch.distributed environment: start the N ranks ourselves, exactly as the
    contract's launcher would (one process per GPU, 127.0.0.1 rendezvous).  Rank 0's JSON line is this process' output."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["OHM_BENCH_SELF_LAUNCHED"] = "1"
    return subprocess.call(cmd, env=env)


def load_traffic_profile(kind, build_id):
    """profiles/rNN_<kind>.json of the newest round; {'doc': parsed or None, 'note': where it came from / why not}."""
    import glob
    import re
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_%s.json" % kind)),
                   key=lambda f: int(re.search(r"r(\d+)_", os.path.basename(f)).group(1)))
    if not files:
        return {"doc": None, "note": "no profiles/rNN_%s.json" % kind}
    name = os.path.basename(files[-1])
    try:
        with open(files[-1]) as fh:
            doc = json.load(fh)
    except Exception as exc:
        return {"doc": None, "note": "%s unreadable: %r" % (name, exc)}
    recorded = doc.get("library_build_id")
    if recorded != build_id:
        return {"doc": None, "note": "STALE: profiles/%s was recorded with library build %s, this is build %s -- re-run "
                                     "scripts/profile_bench.sh <tag> pmc + scripts/traffic_json.py" % (name, recorded, build_id)}
    return {"doc": doc, "note": "profiles/%s (library build %s)" % (name, build_id)}


DUMP_BYTES = 64_000_000   # --dump-outputs: all files of all ranks together stay below this
DUMP_SEED = 0x0D0E5EED    # fixed, so every build samples the same regions out of the same key list


def dump_outputs(out_dir, map_, gm, st, rank, world, layer="occupancy"):
    """--dump-outputs DIR: what a caller of the timed path holds after its last step -- the map's voxels, brought to the
    host by syncVoxels() -- as .npy files in float32 / float64 (at N > 1 every rank writes its own map, prefix rank<r>_):
      region_keys        float64 (R, 3)      every region of the map, sorted
      region_summary     float64 (R, 3)      per region: voxels with a finite value, their sum, their sum of squares
      <layer>_sample     float32 (S, V)      the layer's blocks of S regions drawn with DUMP_SEED from the sorted keys,
                                             non-finite values (+inf = unobserved) written as 0
      <layer>_sample_state float32 (S, V)    per voxel of the sample: 0 finite, 1 +inf, 2 -inf, 3 NaN
      <layer>_sample_keys float64 (S, 3)     (S = every region when they fit in DUMP_BYTES, V = voxels per region)
      batch_stats        float64 (4,)        rays_integrated, voxel_visits, regions_resident, ray_region_segments
    Every value written is finite."""
    os.makedirs(out_dir, exist_ok=True)
    gm.syncVoxels()
    keys = sorted(k for k, c in map_.chunks.items() if layer in c)
    blocks = [map_.chunks[k][layer] for k in keys]
    key_arr = np.array(keys, dtype=np.float64).reshape(-1, 3)
    summary = np.zeros((len(keys), 3), dtype=np.float64)
    for i, b in enumerate(blocks):
        v = b[np.isfinite(b)].astype(np.float64)
        summary[i] = (v.size, v.sum(), np.dot(v, v))
    block_bytes = 4 * map_.regionVoxelVolume()
    room = DUMP_BYTES // world - 2 * key_arr.nbytes - summary.nbytes - 4096
    n_sample = int(max(0, min(len(keys), room // (2 * block_bytes + 24))))   # values + state per region
    if n_sample < len(keys):
        pick = np.sort(np.random.default_rng(DUMP_SEED).choice(len(keys), size=n_sample, replace=False))
    else:
        pick = np.arange(len(keys))
    sample = np.stack([blocks[i] for i in pick]).astype(np.float32) if len(pick) else \
        np.zeros((0, map_.regionVoxelVolume()), dtype=np.float32)
    state = np.zeros(sample.shape, dtype=np.float32)
    state[np.isposinf(sample)] = 1.0
    state[np.isneginf(sample)] = 2.0
    state[np.isnan(sample)] = 3.0
    sample[state != 0.0] = 0.0
    prefix = "rank%d_" % rank if world > 1 else ""
    stats = np.array([st["rays_integrated"], st["voxel_visits"], st["regions_resident"], st["ray_region_segments"]],
                     dtype=np.float64)
    for name, arr in (("region_keys", key_arr), ("region_summary", summary), (layer + "_sample", sample),
                      (layer + "_sample_state", state), (layer + "_sample_keys", key_arr[pick]),
                      ("batch_stats", stats)):
        assert np.isfinite(arr).all(), name
        np.save(os.path.join(out_dir, prefix + name + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--cpu-sample", type=int, default=1_000_000)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-cpu-all-cores", action="store_true", help="skip the P-process leg of cpu_baseline")
    ap.add_argument("--no-extra", action="store_true")
    ap.add_argument("--no-deviation", action="store_true", help="N > 1: skip the untimed check against sequential integration")
    ap.add_argument("--multi-gpu-mode", choices=("partitioned", "replica-merge"), default="partitioned",
                    help="N > 1: partitioned map with routed rays (exact; default) or replicated maps reconciled by the "
                         "additive delta all-reduce (approximate where clamps engage)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline: the CPU baseline, the other configs "
                         "(other_configs, first_pass, moving_sensor), the device-copy ceiling and, at N > 1, the "
                         "deviation from sequential integration.  Without it only the timed steps run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed (the map after the last step) to DIR/*.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_relaunch_ranks(args.gpus))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    backend = None
    if world > 1:
        # torch must be imported before ohm_amd (it bundles its own HIP runtime; see tests/_gpu_merge_worker.py).
        import torch
        import torch.distributed as dist
        n_dev = torch.cuda.device_count()
        if n_dev == 0:
            # No HIP device: the product path cannot run (no CPU fallback).  What CAN be checked is the launcher: the N
            # ranks exist, rendezvous and count each other.  value stays null and the line carries "error".
            dist.init_process_group("gloo")
            t = torch.ones(1, dtype=torch.int64)
            dist.all_reduce(t)
            if rank == 0:
                print(json.dumps({"metric": "rays/sec integrated (occupancy)", "value": None, "unit": "rays/s",
                                  "n_gpus": world, "ranks": int(t.item()), "devices_visible": 0, "backend": "gloo",
                                  "error": "no HIP device visible: launcher check only, nothing was integrated"}))
            dist.destroy_process_group()
            sys.exit(0)
        device_index = local_rank % n_dev
        torch.cuda.set_device(device_index)
        # One rank per GPU over RCCL; if ranks outnumber GPUs (single-GPU smoke runs) fall back to gloo for the
        # control-plane collectives and the staged merge -- the integration itself has no collective.
        backend = "nccl" if n_dev >= world else "gloo"
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device_index))
        else:
            dist.init_process_group("gloo")
    else:
        device_index = 0
        n_dev = None

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    L.check(L.lib.ohmhip_device_select(device_index), "device_select")
    resolution = 0.1
    n_rays = args.rays
    if world == 1:
        rays = synth.rays_c1(n=n_rays)
        workload = "C1: GpuMap occupancy-only, 0.1 m voxels, 32^3 regions, 1M-ray 64-beam lidar batch, 7.5-30 m"
    else:
        rays = synth.rays_c4_shard(rank, n=n_rays)
        if args.multi_gpu_mode == "partitioned":
            workload = ("C4: GpuMap occupancy, 0.1 m voxels, 1M-ray lidar batch per sensor origin, one origin per GPU, map "
                        "partitioned into territories (each region block belongs to the nearest origin's GPU); every "
                        "step routes the rays to the owners of the regions they cross (exact enumeration on the "
                        "device), exchanges the routed rays (all-to-all, 48 B per ray) and integrates what arrives -- "
                        "all inside the timed region; bit-identical to one map integrating the shards in rank order")
        else:
            workload = ("C4: GpuMap occupancy, 0.1 m voxels, 1M-ray lidar batch per sensor origin, one origin per GPU, "
                        "replicated maps, regions touched by more than one GPU merged by an RCCL delta all-reduce after "
                        "every batch (inside the timed region)")

    map_ = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
    gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)

    # Rays resident in HBM.
    buf = L._vp()
    L.check(L.lib.ohmhip_buffer_create(C.byref(buf), rays.nbytes, 3), "buffer_create")
    L.check(L.lib.ohmhip_buffer_write(buf, rays.ctypes.data, rays.nbytes, 0, None, None, None), "buffer_write")
    dptr = L._vp()
    L.check(L.lib.ohmhip_buffer_ptr(buf, C.byref(dptr)), "buffer_ptr")

    merger = None
    comm = None
    merge_log = []
    integ = None
    route_log = []
    partitioned = world > 1 and args.multi_gpu_mode == "partitioned"
    if world > 1:
        from ohm_amd import distributed as D
        # RCCL communicator owned by the library when every rank has its own GPU; otherwise (single-GPU smoke runs with
        # more ranks than GPUs) the same merge steps run over the gloo group.
        merge_note = None
        try:
            comm = D.Communicator() if backend == "nccl" else None
        except Exception as exc:  # the library's RCCL communicator could not be made: merge over the torch group
            comm = None
            merge_note = "library RCCL communicator unavailable (%s): merge staged over the torch group" % (exc,)
        if backend == "nccl":
            # all ranks use the same transport: the library's communicator only if EVERY rank has one
            import torch
            ok = torch.tensor([1 if comm is not None else 0], device="cuda", dtype=torch.int32)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)
            if not int(ok.item()) and comm is not None:
                comm.close()
                comm = None
                merge_note = "library RCCL communicator missing on another rank: merge staged over the torch group"
        if partitioned:
            origins = [synth.C4_ORIGINS[r % len(synth.C4_ORIGINS)] for r in range(world)]
            part = D.territories_from_origins(origins, world, rank, 32 * resolution, block_shift=1, margin=40.0)
            integ = D.PartitionedIntegrator(gm, part, comm=comm)
        else:
            merger = D.ReplicaMerger(gm, comm=comm)

    def barrier():
        gm.wait()
        if dist is not None:
            import torch
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()

    merge_state = {"merger": merger, "error": None}

    def step():
        if integ is not None:
            integ.integrateRaysDevice(dptr, rays.shape[0])
            route_log.append(dict(integ.last))
            return
        gm.integrateRaysDevice(dptr, rays.shape[0])
        if merge_state["merger"] is not None:
            try:
                merge_log.append(merge_state["merger"].merge())
            except Exception as exc:
                # Reported in the output line.  The library (and ReplicaMerger's gloo path) make the ranks agree on a
                # rank-local failure before the payload collective: the failing rank raises its own error, every other
                # rank OHMHIP_ERR_PEER from the SAME call, so all ranks stop merging together and none is left blocked.
                merge_state["error"] = repr(exc)
                merge_state["merger"] = None

    for _ in range(args.warmup):
        step()
    barrier()
    del merge_log[:]
    del route_log[:]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    elapsed = time.perf_counter() - t0
    # hipEvent timings recorded on the map's stream around each kernel phase of the timed steps (the library keeps the
    # events of its last 32 batches, so the timed loop itself never synchronises with the device).
    timings = [gm.batchTimings(back) for back in range(min(args.steps, 32))]
    walk_ms = [t["ms_walk"] for t in timings]
    total_ms = [t["ms_total"] for t in timings]
    if dist is not None:
        import torch
        t = torch.tensor([elapsed], device="cuda" if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    st = gm.stats()
    visits = int(st["voxel_visits"])
    rays_ok = int(st["rays_integrated"])
    if partitioned and route_log:
        # A partitioned rank walks the segments inside its territory of every ray addressed to it; the batch statistics
        # count whole rays.  The job's voxel visits are those of the ranks' own shards: this rank's share is its shard's.
        visits = int(route_log[-1]["visits_local"])
        rays_ok = n_rays
    # Algorithmic bytes: 44 B per ray + 8 B per voxel visit (4 B read + 4 B write of the log-odds).
    b_alg = 44.0 * rays_ok + 8.0 * visits
    # Measured HBM traffic: from the committed PMC profile of this same command (separate rocprofv3 --pmc passes,
    # profiles/rNN_traffic.json <- scripts/traffic_json.py; bench.py itself cannot run the profiler).  The NEWEST round's
    # file is taken, and only if it was recorded with THIS build of the library (library_build_id): a profile of another
    # build is reported as stale, never quoted.  FETCH_SIZE counts 64-byte requests: x2 for coalesced streams (the
    # guide's correction), x1 for the kernel's 32-byte record gathers (profiles/r02_fetch_calibration.txt) -- the two
    # figures bracket the bytes moved.
    traffic = traffic_lower = batch_traffic = batch_traffic_lower = None
    traffic_source = None
    build_id = L.lib.ohmhip_build_id().decode()
    tj = load_traffic_profile("traffic", build_id)
    traffic_source = tj["note"]
    if tj["doc"] is not None and world == 1 and n_rays == 1_000_000:
        traffic = tj["doc"]["kernels"]["k_region_walk"]["bytes_upper"]
        traffic_lower = tj["doc"]["kernels"]["k_region_walk"]["bytes_lower"]
        batch_traffic = tj["doc"]["batch_bytes_upper"]
        batch_traffic_lower = tj["doc"]["batch_bytes_lower"]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, map_, gm, st, rank, world)
    # Measured ceiling next to the nominal peak: a device-to-device copy of 1 GiB (read + write), a run of its own.
    copy_gbps = None
    if args.full:
        try:
            nbytes = 1 << 30
            ca, cb = L._vp(), L._vp()
            L.check(L.lib.ohmhip_buffer_create(C.byref(ca), nbytes, 3), "buffer_create")
            L.check(L.lib.ohmhip_buffer_create(C.byref(cb), nbytes, 3), "buffer_create")
            L.check(L.lib.ohmhip_buffer_copy(cb, 0, ca, 0, nbytes, None, None, None), "buffer_copy")
            L.check(L.lib.ohmhip_device_synchronize(), "device_synchronize")
            reps = 5
            t1 = time.perf_counter()
            for _ in range(reps):
                L.check(L.lib.ohmhip_buffer_copy(cb, 0, ca, 0, nbytes, None, None, None), "buffer_copy")
            L.check(L.lib.ohmhip_device_synchronize(), "device_synchronize")
            copy_gbps = 2.0 * nbytes * reps / (time.perf_counter() - t1) / 1e9
            L.lib.ohmhip_buffer_destroy(ca)
            L.lib.ohmhip_buffer_destroy(cb)
        except Exception:
            copy_gbps = None
    t_walk = float(np.mean(walk_ms)) * 1e-3
    t_dev = float(np.mean(total_ms)) * 1e-3
    achieved = b_alg / t_walk / 1e9
    out = {
        "metric": "rays/sec integrated (occupancy)",
        "value": world * n_rays * args.steps / elapsed,
        "unit": "rays/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f64",  # line walk in fp64 (as the CPU mapper); the log-odds layer itself is f32
        "data": "synthetic",
        "config": {"workload": workload, "rays_per_step_per_gpu": n_rays, "voxel_visits_per_step": visits,
                   "regions": int(st["regions_resident"]), "ray_region_segments": int(st["ray_region_segments"])},
        # Basis: `achieved` / `frac` charge the algorithmic bytes to the WHOLE batch interval on the
        # device -- set-up, binning, sample ordering, walk, apply: everything integrateRays costs, the same basis the C2 /
        # C3 blocks in other_configs use -- and the dominant kernel alone is the secondary pair kernel_achieved /
        # kernel_frac (rounds 1-4 quoted that one as `frac`).
        "roofline": {"bound": "hbm", "kernel": "k_region_walk", "achieved": b_alg / t_dev / 1e9, "peak": HBM_PEAK_GBPS,
                     "unit": "GB/s", "frac": b_alg / t_dev / 1e9 / HBM_PEAK_GBPS,
                     "basis": "algorithmic bytes of one batch / the batch's device interval (all kernels of integrateRays)",
                     "pipeline_ms": t_dev * 1e3, "pipeline_frac": b_alg / t_dev / 1e9 / HBM_PEAK_GBPS,
                     "kernel_ms": t_walk * 1e3, "kernel_achieved": achieved, "kernel_frac": achieved / HBM_PEAK_GBPS,
                     "kernel_ms_note": "HIP events on the stream the kernel runs on: stop event of the kernel before the "
                                       "walk -> stop event of the walk kernel (hipExtLaunchKernelGGL; a start marker "
                                       "would idle the queue for microseconds).  Includes the time the walk's workgroups "
                                       "wait for the CUs the next batch's set-up pass still holds, so it reads a few "
                                       "per cent above the dispatch duration in profiles/",
                     "traffic": traffic, "traffic_lower": traffic_lower, "pipeline_traffic": batch_traffic,
                     "pipeline_traffic_lower": batch_traffic_lower, "traffic_source": traffic_source,
                     "peak_measured_copy": copy_gbps, "algorithmic_bytes_per_launch": b_alg},
        "device_ms": {"walk": float(np.mean(walk_ms)),
                      "sort_apply": float(np.mean([t["ms_apply"] for t in timings])), "total": float(np.mean(total_ms)),
                      "note": "total = completion interval of back-to-back batches (stop events of each batch's last "
                              "kernel); walk / sort_apply from the kernels' stop events.  The set-up and binning passes "
                              "carry no start markers by default (ohmhip_map_set_phase_timing: each marker costs the "
                              "batch 3-7 us), so their share is total - walk - sort_apply"},
    }
    out["ranks"] = world
    out["devices_visible"] = n_dev if n_dev is not None else int(ohm_amd.device_count())
    if world > 1:
        out["backend"] = "RCCL" if backend == "nccl" else "gloo (ranks share a GPU: host-staged exchange, NOT a scaling figure)"
        out["rccl_ranks"] = comm.world if comm is not None else None
    if partitioned:
        sent = float(np.mean([r["rays_routed"] - r["rays_kept"] for r in route_log])) if route_log else 0.0
        out["multi_gpu"] = {
            "mode": "partitioned map, routed rays (exact)",
            "transport": "RCCL (library: ncclSend / ncclRecv group)" if comm is not None else
                         ("RCCL (torch.distributed all_to_all_single)" if backend == "nccl" else
                          "gloo all_to_all_single, host staged (ranks share a GPU: NOT a scaling figure)"),
            "territories": "blocks of 2 x 2 x 2 regions, each owned by the rank whose sensor origin is nearest",
            "per_step_this_rank": {"rays_local": n_rays,
                                   "rays_sent_to_other_ranks": sent,
                                   "rays_received": float(np.mean([r["rays_received"] for r in route_log])) if route_log else 0.0,
                                   "bytes_sent": 48.0 * sent},
            "note": merge_note}
    if world > 1 and not partitioned and (merge_state["error"] or not merge_log):
        out["merge"] = {"error": merge_state["error"] or "no merge ran", "note": "replicas not reconciled in this run"}
    elif merge_log:
        out["merge"] = {"per_step": {"regions_local": int(np.mean([m["regions_local"] for m in merge_log])),
                                     "regions_union": int(np.mean([m["regions_union"] for m in merge_log])),
                                     "regions_shared": int(np.mean([m["regions_shared"] for m in merge_log])),
                                     "payload_bytes_per_rank": int(np.mean([m["payload_bytes"] for m in merge_log])),
                                     "ms_host": float(np.mean([m.get("ms_total", 0.0) for m in merge_log]))},
                        "transport": "RCCL (library)" if comm is not None else "torch.distributed group (staged)",
                        "note": merge_note,
                        "rule": "merged = clamp(base + sum_r (x_r - base)); exact where no clamp engaged between ranks; "
                                "regions pending on one rank only stay on that rank (shared base untouched)"}
    if partitioned and args.full and not args.no_deviation:
        # Untimed: the partitioned map against SEQUENTIAL integration.  Fresh maps: one partitioned step (collective), and
        # every rank integrates the shards of all ranks, in rank order, into one map of its own -- the HIP path, bit exact
        # against the CPU mapper (tests/test_gpu_full_configs.py) -- and compares the regions of its territory bit for
        # bit; the counts are summed over the ranks.
        try:
            import torch
            from ohm_amd import distributed as D
            dm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
            dg = ohm_amd.GpuMap(dm, gpu_mem_size=8 << 30)
            dinteg = D.PartitionedIntegrator(dg, integ.partition, comm=comm)
            dinteg.integrateRaysDevice(dptr, rays.shape[0])
            dg.syncVoxels()
            sm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
            sg = ohm_amd.GpuMap(sm, gpu_mem_size=16 << 30)
            for r in range(world):
                sg.integrateRays(synth.rays_c4_shard(r, n=n_rays))
            sg.syncVoxels()
            seq_keys = np.array(sorted(sm.chunks), dtype=np.int16).reshape(-1, 3)
            mine = seq_keys[integ.partition.owners(seq_keys) == rank]
            mine_set = set(tuple(int(v) for v in k) for k in mine)
            dev = D.merge_deviation(dm.chunks, sm.chunks, keys=sorted(mine_set & set(dm.chunks)))
            counts = [dev["regions_compared"], dev["voxels_compared"], dev["voxels_observed"],
                      dev["voxels_state_differs"], dev["voxels_value_differs"], dev["voxels_beyond_rel"],
                      len(mine_set - set(dm.chunks)),                                    # regions this rank should hold
                      sum(1 for k, c in dm.chunks.items() if k not in mine_set and np.isfinite(c["occupancy"]).any()),
                      len(sm.chunks) if rank == 0 else 0]
            t = torch.tensor(counts, dtype=torch.int64, device="cuda" if backend == "nccl" else "cpu")
            dist.all_reduce(t)
            mx = torch.tensor([dev["max_abs_delta"]], dtype=torch.float64, device=t.device)
            dist.all_reduce(mx, op=dist.ReduceOp.MAX)
            c = [int(v) for v in t.tolist()]
            out["multi_gpu"]["deviation"] = {
                "regions_compared": c[0], "voxels_compared": c[1], "voxels_observed": c[2],
                "voxels_state_differs": c[3], "voxels_value_differs": c[4], "voxels_beyond_rel": c[5],
                "regions_missing": c[6], "regions_outside_their_territory": c[7], "regions_sequential": c[8],
                "max_abs_delta": float(mx.item()), "rel": dev["rel"],
                "note": "union of the ranks' territories after ONE batch per rank vs one map integrating the shards of "
                        "all ranks in rank order: every count but the first three must be 0 (bit-identical)"}
            sg.close()
            dinteg.close()
            dg.close()
        except Exception as exc:
            out["multi_gpu"]["deviation"] = {"error": repr(exc)}
    if world > 1 and merge_state["merger"] is not None and args.full and not args.no_deviation:
        # Untimed: how far the replica merge is from SEQUENTIAL integration ("must be stated with results").
        # Fresh maps: every rank integrates its shard ONCE and the replicas merge (collective); rank 0 also integrates
        # the shards of all ranks one after the other into one map -- the HIP path, which is bit exact against the CPU
        # mapper (tests/test_gpu_full_configs.py) -- and compares the regions it holds.
        try:
            from ohm_amd import distributed as D
            dm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
            dg = ohm_amd.GpuMap(dm, gpu_mem_size=8 << 30)
            dmerger = D.ReplicaMerger(dg, comm=comm)
            dg.integrateRaysDevice(dptr, rays.shape[0])
            dstats = dmerger.merge()
            if rank == 0:
                sm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
                sg = ohm_amd.GpuMap(sm, gpu_mem_size=16 << 30)
                for r in range(world):
                    sg.integrateRays(synth.rays_c4_shard(r, n=n_rays))
                sg.syncVoxels()
                dg.syncVoxels()
                dev = D.merge_deviation(dm.chunks, sm.chunks)
                dev["regions_exchanged"] = int(dstats["regions_shared"])
                dev["note"] = ("rank 0's replica after ONE batch per rank + one merge vs one map integrating the shards "
                               "of all ranks in rank order; differences = float summation order + clamp interplay")
                out["merge"]["deviation"] = dev
                sg.close()
            dg.close()
        except Exception as exc:
            if rank == 0 and "merge" in out:
                out["merge"]["deviation"] = {"error": repr(exc)}
    if world == 1 and args.full and not args.no_extra:
        # Secondary figures (not the headline `value`): C2 GpuNdtMap (1 M rays) and C3 GpuTsdfMap (its full 4 M rays in one
        # call), same harness, each with its own roofline block.  Algorithmic bytes per SURVEY.md 8d:
        #   NDT : 40 B per miss visit (4 + 4 occupancy, 8 mean, 24 covariance) + 72 B per sample + 44 B per ray
        #   TSDF: 16 B per voxel visit (8 read + 8 write) + 68 B per ray
        extra = {}
        for name, cls, res, r2, layers, steps2 in (
                ("C2_ndt_1M_rays_0.2m", ohm_amd.GpuNdtMap, 0.2, synth.rays_c2(n=n_rays), ("occupancy",), 3),
                ("C3_tsdf_4M_rays_0.05m", ohm_amd.GpuTsdfMap, 0.05, synth.rays_c3(n=4 * n_rays), ("tsdf",), 2)):
            m2 = ohm_amd.OccupancyMap(res, (32, 32, 32), layers=layers)
            g2 = cls(m2, gpu_mem_size=24 << 30)
            b2 = L._vp()
            L.check(L.lib.ohmhip_buffer_create(C.byref(b2), r2.nbytes, 3), "buffer_create")
            L.check(L.lib.ohmhip_buffer_write(b2, r2.ctypes.data, r2.nbytes, 0, None, None, None), "buffer_write")
            p2 = L._vp()
            L.check(L.lib.ohmhip_buffer_ptr(b2, C.byref(p2)), "buffer_ptr")
            g2.integrateRaysDevice(p2, r2.shape[0])
            g2.wait()
            t1 = time.perf_counter()
            for _ in range(steps2):
                g2.integrateRaysDevice(p2, r2.shape[0])
            g2.wait()
            dt = (time.perf_counter() - t1) / steps2
            st2 = g2.stats()
            tm2 = [g2.batchTimings(back) for back in range(steps2)]
            n2 = int(st2["rays_integrated"])
            v2 = int(st2["voxel_visits"])
            if cls is ohm_amd.GpuNdtMap:
                b_alg2 = 40.0 * (v2 - n2) + 72.0 * n2 + 44.0 * n2
            else:
                b_alg2 = 16.0 * v2 + 68.0 * n2
            dev2 = float(np.mean([t["ms_total"] for t in tm2])) * 1e-3
            walk2 = float(np.mean([t["ms_walk"] for t in tm2])) * 1e-3
            tj2 = load_traffic_profile("traffic_c2_ndt" if cls is ohm_amd.GpuNdtMap else "traffic_c3_tsdf", build_id)
            tr2 = {"source": tj2["note"]}
            if tj2["doc"] is not None:
                tr2.update({"pipeline_traffic": tj2["doc"]["batch_bytes_upper"],
                            "pipeline_traffic_lower": tj2["doc"]["batch_bytes_lower"]})
            extra[name] = {"rays_per_s": (r2.shape[0] // 2) / dt, "ms_per_step": dt * 1e3, "rays": r2.shape[0] // 2,
                           "voxel_visits": v2, "regions": int(st2["regions_resident"]),
                           "roofline": {"bound": "hbm", "algorithmic_bytes_per_step": b_alg2, "peak": HBM_PEAK_GBPS,
                                        "unit": "GB/s", "pipeline_ms": dev2 * 1e3,
                                        "achieved": b_alg2 / dev2 / 1e9, "frac": b_alg2 / dev2 / 1e9 / HBM_PEAK_GBPS,
                                        "walk_kernel_ms": walk2 * 1e3, "counter_traffic": tr2,
                                        "note": "frac is over the whole device pipeline of a batch (walk + event order + "
                                                "ordered replay).  The formula charges every voxel visit with the "
                                                "layer bytes the reference formulation would move; this design only "
                                                "touches the layers of marked voxels, so frac compares against an "
                                                "ideal HBM-bound implementation of the reference formulation, it is "
                                                "not an HBM utilisation (measured traffic: profiles/)"}}
            L.lib.ohmhip_buffer_destroy(b2)
            g2.close()
            del r2
        # C3 cache-stress variant: the region pool bounded at the reference's default budget of 1 GiB and the
        # 4 M rays presented as 45-degree sectors of the sweep, so the least recently used regions spill to the host
        # store as the sensor turns and come back one revolution later (include/ohmhip.h "SPILL TO HOST").
        try:
            m4 = ohm_amd.OccupancyMap(0.05, (32, 32, 32), layers=("tsdf",))
            g4 = ohm_amd.GpuTsdfMap(m4, region_capacity=1024)
            g4.setMemoryLimit(1 << 30)
            g4.setSpillToHost(True)
            r4 = synth.rays_c3(n=4 * n_rays)
            b4 = L._vp()
            L.check(L.lib.ohmhip_buffer_create(C.byref(b4), r4.nbytes, 3), "buffer_create")
            L.check(L.lib.ohmhip_buffer_write(b4, r4.ctypes.data, r4.nbytes, 0, None, None, None), "buffer_write")
            p4 = L._vp()
            L.check(L.lib.ohmhip_buffer_ptr(b4, C.byref(p4)), "buffer_ptr")
            sectors = 32
            per = (r4.shape[0] // 2) // sectors
            t1 = time.perf_counter()
            done4 = 0
            for k in range(sectors):
                done4 += g4.integrateRaysDevice(C.c_void_p(p4.value + k * per * 48), 2 * per)
            g4.wait()
            dt4 = time.perf_counter() - t1
            cs = g4.cacheStats()
            # second revolution of the same sweep: pool and host store at their final size, the eviction policy knows
            # every region's period (no allocation, no pinning: what is left is the moves and the repeated attempts)
            t1 = time.perf_counter()
            again4 = 0
            for k in range(sectors):
                again4 += g4.integrateRaysDevice(C.c_void_p(p4.value + k * per * 48), 2 * per)
            g4.wait()
            dt4b = time.perf_counter() - t1
            cs_b = g4.cacheStats()
            moved_b = (cs_b["evictions"] - cs["evictions"]) + (cs_b["readmissions"] - cs["readmissions"])
            extra["C3_tsdf_cache_stress_1GiB"] = {
                "rays_per_s": (done4 // 2) / dt4, "seconds": dt4, "rays": done4 // 2, "calls": sectors,
                "memory_limit_bytes": int(cs["memory_limit"]), "regions_resident": int(cs["regions_resident"]),
                "regions_in_host_store": int(cs["regions_spilled"]), "evictions": int(cs["evictions"]),
                "readmissions": int(cs["readmissions"]),
                "bytes_over_pcie": int((cs["evictions"] + cs["readmissions"]) * (8 * 32 ** 3 + 4096)),
                "second_revolution": {"rays_per_s": (again4 // 2) / dt4b, "seconds": dt4b,
                                      "evictions": int(cs_b["evictions"] - cs["evictions"]),
                                      "readmissions": int(cs_b["readmissions"] - cs["readmissions"]),
                                      "pcie_gb_per_s": moved_b * (8 * 32 ** 3 + 4096) / dt4b / 1e9},
                "note": "first pass over a fresh map: includes pool growth to the limit and every eviction / "
                        "re-admission (pinned host store; one device kernel per eviction / re-admission moves all "
                        "regions over PCIe, synchronous with the batch)"}
            g4.close()
            # "map >> cache": the same sweep against an eighth of that budget -- 128 MiB hold 335 of the map's 4 465
            # regions (13 x oversubscribed) -- in 256 sectors (a batch must fit the pool on its own)
            m5 = ohm_amd.OccupancyMap(0.05, (32, 32, 32), layers=("tsdf",))
            g5 = ohm_amd.GpuTsdfMap(m5, region_capacity=256)
            g5.setMemoryLimit(128 << 20)
            g5.setSpillToHost(True)
            sectors5 = 256
            per5 = (r4.shape[0] // 2) // sectors5
            t1 = time.perf_counter()
            done5 = 0
            for k in range(sectors5):
                done5 += g5.integrateRaysDevice(C.c_void_p(p4.value + k * per5 * 48), 2 * per5)
            g5.wait()
            dt5 = time.perf_counter() - t1
            cs5 = g5.cacheStats()
            t1 = time.perf_counter()
            again5 = 0
            for k in range(sectors5):
                again5 += g5.integrateRaysDevice(C.c_void_p(p4.value + k * per5 * 48), 2 * per5)
            g5.wait()
            dt5b = time.perf_counter() - t1
            cs5_b = g5.cacheStats()
            moved5_b = (cs5_b["evictions"] - cs5["evictions"]) + (cs5_b["readmissions"] - cs5["readmissions"])
            total5 = int(cs5["regions_resident"]) + int(cs5["regions_spilled"])
            extra["C3_tsdf_cache_stress_128MiB"] = {
                "rays_per_s": (done5 // 2) / dt5, "seconds": dt5, "rays": done5 // 2, "calls": sectors5,
                "memory_limit_bytes": int(cs5["memory_limit"]), "regions_resident": int(cs5["regions_resident"]),
                "regions_in_host_store": int(cs5["regions_spilled"]),
                "oversubscription": total5 / max(1.0, cs5["memory_limit"] / cs5["bytes_per_region"]),
                "evictions": int(cs5["evictions"]), "readmissions": int(cs5["readmissions"]),
                "bytes_over_pcie": int((cs5["evictions"] + cs5["readmissions"]) * (8 * 32 ** 3 + 4096)),  # TSDF block + mask row
                "pcie_gb_per_s": (cs5["evictions"] + cs5["readmissions"]) * (8 * 32 ** 3 + 4096) / dt5 / 1e9,
                "second_revolution": {"rays_per_s": (again5 // 2) / dt5b, "seconds": dt5b,
                                      "evictions": int(cs5_b["evictions"] - cs5["evictions"]),
                                      "readmissions": int(cs5_b["readmissions"] - cs5["readmissions"]),
                                      "pcie_gb_per_s": moved5_b * (8 * 32 ** 3 + 4096) / dt5b / 1e9},
                "note": "regions resident / regions of the map = 1 / oversubscription (>= 8 asked for by the round-3 review); every region leaves and returns about three times per revolution: the leg is bound by the "
                        "PCIe traffic of the moves (one device kernel per eviction / re-admission, synchronous with "
                        "the batch; the opt-in background write-back -- ohmhip_map_set_spill_writeback -- takes "
                        "copy-outs off that path but was measured slower here, DESIGN.md 3)"}
            g5.close()
            L.lib.ohmhip_buffer_destroy(b4)
            del r4
        except Exception as exc:  # never lose the bench line over a secondary figure
            extra["C3_tsdf_cache_stress_1GiB"] = {"error": repr(exc)}
        # The headline integrates the SAME batch into one map again and again: after the first passes every free voxel
        # sits at the min clamp (its update is a compare, its store is skipped) and no region is created.  Next to it: the
        # first pass of the same batch over a FRESH map (regions created on the device, every voxel written) and the
        # second (values still moving towards the clamps).  Pool allocation happens at map creation, outside the timing.
        try:
            fresh = []
            for _ in range(3):
                mf = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
                # (expected_element_count: the per-batch buffers are sized at construction, as the reference's GpuMap
                # constructor sizes its ray / key buffers -- the first call then allocates nothing)
                gf = ohm_amd.GpuMap(mf, expected_element_count=rays.shape[0], gpu_mem_size=8 << 30)
                gf.wait()
                t1 = time.perf_counter()
                gf.integrateRaysDevice(dptr, rays.shape[0])
                gf.wait()
                t2 = time.perf_counter()
                gf.integrateRaysDevice(dptr, rays.shape[0])
                gf.wait()
                t3 = time.perf_counter()
                fresh.append((t2 - t1, t3 - t2, float(gf.batchTimings(1)["ms_walk"]), float(gf.batchTimings(0)["ms_walk"])))
                gf.close()
            first = min(f[0] for f in fresh)
            second = min(f[1] for f in fresh)
            extra["C1_fresh_map_first_pass"] = {
                "first_pass_ms": first * 1e3, "second_pass_ms": second * 1e3,
                "first_pass_walk_kernel_ms": min(f[2] for f in fresh), "second_pass_walk_kernel_ms": min(f[3] for f in fresh),
                "first_pass_rays_per_s": n_rays / first,
                "first_pass_pipeline_frac": b_alg / first / 1e9 / HBM_PEAK_GBPS,
                "note": "one isolated call each (host-synchronised, so the next batch's set-up pass does not overlap as in "
                        "the steady-state headline); best of 3 fresh maps"}
        except Exception as exc:
            extra["C1_fresh_map_first_pass"] = {"error": repr(exc)}
        # C0 (BASELINE configs[0]: 100 k uniform 10 m rays from one origin) on the HIP path, device-resident rays.
        try:
            r0 = synth.rays_c0()
            m0 = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
            g0 = ohm_amd.GpuMap(m0)
            b0 = L._vp()
            L.check(L.lib.ohmhip_buffer_create(C.byref(b0), r0.nbytes, 3), "buffer_create")
            L.check(L.lib.ohmhip_buffer_write(b0, r0.ctypes.data, r0.nbytes, 0, None, None, None), "buffer_write")
            p0 = L._vp()
            L.check(L.lib.ohmhip_buffer_ptr(b0, C.byref(p0)), "buffer_ptr")
            g0.integrateRaysDevice(p0, r0.shape[0])
            g0.wait()
            t1 = time.perf_counter()
            for _ in range(10):
                g0.integrateRaysDevice(p0, r0.shape[0])
            g0.wait()
            dt = (time.perf_counter() - t1) / 10
            st0 = g0.stats()
            extra["C0_100k_rays_10m"] = {"rays_per_s": (r0.shape[0] // 2) / dt, "ms_per_step": dt * 1e3,
                                         "voxel_visits": int(st0["voxel_visits"]), "regions": int(st0["regions_resident"])}
            L.lib.ohmhip_buffer_destroy(b0)
            g0.close()
        except Exception as exc:
            extra["C0_100k_rays_10m"] = {"error": repr(exc)}
        # C4 on ONE GPU, the mode `--gpus N` runs: 8 partitioned maps in this process standing in for the 8 ranks.  Every
        # rank's shard is routed by the library's kernels, the destination blocks are re-assembled in (source rank, ray)
        # order -- what the all-to-all delivers -- and each map integrates what is addressed to it; compared bit for bit
        # with ONE map integrating the 8 shards in rank order.  Per-rank times are this GPU's; not a scaling figure.
        if not args.no_deviation:
            try:
                from ohm_amd import distributed as D
                part0 = D.territories_from_origins(synth.C4_ORIGINS, 8, 0, 32 * resolution, block_shift=1, margin=40.0)
                pmaps, pgs = [], []
                for r in range(8):
                    pm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
                    pg = ohm_amd.GpuMap(pm, gpu_mem_size=2 << 30)
                    pg.setRegionPartition(part0.with_rank(r))
                    pmaps.append(pm)
                    pgs.append(pg)
                shards = [synth.rays_c4_shard(r, n=n_rays) for r in range(8)]
                D.integrate_partitioned_in_process(pgs, shards)  # first pass: pools, buffers
                tms = {}
                streams = []
                info = D.integrate_partitioned_in_process(pgs, shards, timings=tms, streams_out=streams)
                sm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
                sg = ohm_amd.GpuMap(sm, gpu_mem_size=16 << 30)
                for _ in range(2):
                    for r in range(8):
                        sg.integrateRays(shards[r])
                sg.syncVoxels()
                union = {}
                outside = 0
                for r, (pm, pg) in enumerate(zip(pmaps, pgs)):
                    pg.syncVoxels()
                    keys = np.array(sorted(pm.chunks), dtype=np.int16).reshape(-1, 3)
                    owners = part0.owners(keys) if len(keys) else []
                    for k, o in zip(map(tuple, keys.tolist()), owners):
                        if int(o) != r:
                            outside += 1
                        union[k] = pm.chunks[k]
                dev = D.merge_deviation(union, sm.chunks)
                dev["regions_missing"] = len(set(sm.chunks) - set(union))
                dev["regions_outside_their_territory"] = outside
                routed = info["routed"]
                # (after the comparison: more batches go into the maps) the step as PartitionedIntegrator runs it --
                # routing on its own stream beside the batch in flight, batches back to back
                step_ms = [D.pipelined_rank_step_ms(pgs[r], shards[r], streams[r]) for r in range(8)]
                extra["C4_8_shards_one_gpu_partitioned"] = {
                    "rays_per_shard": n_rays,
                    "rays_sent_to_other_ranks_per_rank": [int(routed[r].sum() - routed[r, r]) for r in range(8)],
                    "rays_received_per_rank": [int(v) for v in info["received"]],
                    "exchange_bytes_per_rank_max": int(48 * max(int(routed[r].sum() - routed[r, r]) for r in range(8))),
                    "route_ms_per_rank": [round(v, 4) for v in tms["route_ms"]],
                    "integrate_ms_per_rank": [round(v, 4) for v in tms["integrate_ms"]],
                    "pipelined_step_ms_per_rank": [round(v, 4) for v in step_ms],
                    "max_rank_step_ms": max(step_ms),
                    "projected_8gpu_rays_per_s": 8 * n_rays / (max(step_ms) * 1e-3),
                    "deviation_vs_sequential": dev,
                    "note": "two batches per rank; union of the 8 territories vs ONE map integrating the 8 shards in rank "
                            "order twice (the HIP path, bit exact vs the CPU mapper): voxels_value_differs must be 0.  "
                            "route_ms / integrate_ms: each phase alone, host synchronised.  pipelined_step_ms: the step "
                            "as --gpus N runs it (next batch routed beside the one in flight, batches back to back), on "
                            "THIS GPU, the exchange itself (48 B per routed ray) excluded"}
                for pg in pgs:
                    pg.close()
                sg.close()
                del pmaps, sm, union, shards
            except Exception as exc:
                extra["C4_8_shards_one_gpu_partitioned"] = {"error": repr(exc)}
        # C4 on ONE GPU in the OPTIONAL replica-merge mode (--multi-gpu-mode replica-merge; 8 replica maps in this process
        # standing in for the 8 ranks): what the additive merge moves and how far its result is from the sequential
        # integration of the 8 shards.  Not a scaling figure, and not what --gpus N runs by default.
        if not args.no_deviation:
            try:
                from ohm_amd import distributed as D
                reps, rmaps = [], []
                for r in range(8):
                    rm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
                    rg = ohm_amd.GpuMap(rm, gpu_mem_size=2 << 30)
                    L.check(L.lib.ohmhip_map_enable_merge(rg._handle), "enable_merge")
                    rg.integrateRays(synth.rays_c4_shard(r, n=n_rays))
                    reps.append(rg)
                    rmaps.append(rm)
                t1 = time.perf_counter()
                shared, mstats = D.merge_in_process(reps)
                t_merge = time.perf_counter() - t1
                sm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
                sg = ohm_amd.GpuMap(sm, gpu_mem_size=16 << 30)
                for r in range(8):
                    sg.integrateRays(synth.rays_c4_shard(r, n=n_rays))
                sg.syncVoxels()
                reps[0].syncVoxels()
                dev = D.merge_deviation(rmaps[0].chunks, sm.chunks, keys=[tuple(k) for k in shared.tolist()])
                extra["C4_8_shards_one_gpu_replica_merge"] = {
                    "regions_pending_per_rank": mstats["regions_pending"], "regions_union": mstats["regions_union"],
                    "regions_exchanged": mstats["regions_shared"],
                    "payload_bytes_per_rank": mstats["payload_bytes_per_rank"], "host_staged_merge_s": t_merge,
                    "deviation_vs_sequential": dev,
                    "note": "replica 0 vs ONE map integrating the 8 shards in rank order (the HIP path, bit exact vs the "
                            "CPU mapper), over the exchanged regions"}
                for rg in reps:
                    rg.close()
                sg.close()
                del rmaps, sm
            except Exception as exc:
                extra["C4_8_shards_one_gpu_replica_merge"] = {"error": repr(exc)}
        # C1 variants SURVEY 8d asks to be reported next to the headline (never the headline `value`):
        # (i) the same batch fed as 4096-ray calls (the reference tools' default batch size): launch-latency bound;
        # (ii) end to end from HOST memory: pinned staging + H2D + integrate + syncVoxels into the host MapChunk blocks.
        m3 = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
        g3 = ohm_amd.GpuMap(m3, gpu_mem_size=8 << 30)
        small = 4096
        n_small = min(n_rays // small, 64)
        stride = 2 * small * 3 * 8
        g3.integrateRaysDevice(dptr, rays.shape[0])
        g3.wait()
        t1 = time.perf_counter()
        for b in range(n_small):
            g3.integrateRaysDevice(C.c_void_p(dptr.value + b * stride), 2 * small)
        g3.wait()
        dt = time.perf_counter() - t1
        extra["C1_4096_ray_batches"] = {"rays_per_s": n_small * small / dt, "ms_per_batch": dt * 1e3 / n_small,
                                        "batches": n_small}
        g3.close()
        m4 = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
        g4 = ohm_amd.GpuMap(m4, gpu_mem_size=8 << 30)
        g4.integrateRays(rays)
        g4.integrateRays(rays)  # both staging slots allocated
        g4.syncVoxels()
        t1 = time.perf_counter()
        g4.integrateRays(rays)
        t2 = time.perf_counter()
        g4.syncVoxels()
        t3 = time.perf_counter()
        n_host = 20
        for _ in range(n_host):  # steady state: batch N+1 staged and uploaded while batch N runs
            g4.integrateRays(rays)
        g4.wait()
        t4 = time.perf_counter()
        # the same with the launch sequence on the map's own thread (ohmhip_map_set_async_launch, opt-in): the call
        # returns once its rays are staged, the next block is staged and sent beside the batch's host round trip
        g4.setAsyncLaunch(True)
        g4.integrateRays(rays)
        g4.wait()
        t5 = time.perf_counter()
        for _ in range(n_host):
            g4.integrateRays(rays)
        g4.wait()
        t6 = time.perf_counter()
        extra["C1_host_end_to_end"] = {"rays_per_s_integrate": n_rays / (t2 - t1),
                                       "rays_per_s_with_sync_voxels": n_rays / (t3 - t1),
                                       "rays_per_s_back_to_back": n_host * n_rays / (t4 - t3),
                                       "rays_per_s_back_to_back_async_launch": n_host * n_rays / (t6 - t5),
                                       "integrate_ms": (t2 - t1) * 1e3, "sync_voxels_ms": (t3 - t2) * 1e3,
                                       "note": "host-pointer rays (48 B/ray over PCIe, staged by the map's pool threads "
                                               "with the copy of each piece queued as it is staged) + all modified "
                                               "regions copied back; host-side figures vary with the box's load and "
                                               "NUMA placement"}
        g4.close()
        # the reference tools' pattern: 4096-ray host batches -- as presented (the library's defaults: small host batches
        # are collected into device batches of 64k rays) and with every call launching its own device batch
        host_small = {}
        for label, min_rays in (("as_presented", None), ("one_device_batch_per_call", 0)):
            m6 = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
            g6 = ohm_amd.GpuMap(m6, gpu_mem_size=8 << 30)
            g6.integrateRays(rays)
            g6.integrateRays(rays)
            g6.wait()
            if min_rays is not None:
                g6.setBatchCoalescing(min_rays)
            n_calls = 128
            dt = float("inf")
            for _rep in range(3):  # (a host-side figure of a few milliseconds: best of three repetitions)
                t1 = time.perf_counter()
                for b in range(n_calls):
                    g6.integrateRays(rays[b * 2 * small:(b + 1) * 2 * small])
                g6.wait()
                dt = min(dt, time.perf_counter() - t1)
            host_small[label] = {"rays_per_s": n_calls * small / dt, "ms_per_call": dt * 1e3 / n_calls}
            g6.close()
        extra["C1_4096_ray_host_batches"] = host_small
        # C1 with a traversal layer (sum of ray lengths per voxel): the count walk plus k_region_traversal, a second fp64
        # walk into a 32-bit LDS tile -- a secondary layer, never the headline.
        try:
            mt = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy", "traversal"))
            gt = ohm_amd.GpuMap(mt, gpu_mem_size=8 << 30)
            gt.integrateRaysDevice(dptr, rays.shape[0])
            gt.wait()
            t1 = time.perf_counter()
            for _ in range(5):
                gt.integrateRaysDevice(dptr, rays.shape[0])
            gt.wait()
            dt = (time.perf_counter() - t1) / 5
            extra["C1_with_traversal_layer"] = {"rays_per_s": n_rays / dt, "ms_per_step": dt * 1e3,
                                                "walk_ms": float(gt.stats()["ms_walk"])}
            gt.close()
        except Exception as exc:
            extra["C1_with_traversal_layer"] = {"error": repr(exc)}
        # A moving sensor (what a real stream looks like: every batch creates regions at the frontier, so the pool grows
        # and the speculative binning -- which keys on the previous batch -- sometimes has to repeat its passes).
        try:
            mm = ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",))
            gmv = ohm_amd.GpuMap(mm, gpu_mem_size=8 << 30)
            n_mov = 8
            bufs = []
            for b in range(n_mov + 1):
                rb = synth.rays_c1(n=n_rays, origin=(0.05 + 0.4 * b, 0.05 + 0.1 * b, 0.05), first=b * 997)
                hb = L._vp()
                L.check(L.lib.ohmhip_buffer_create(C.byref(hb), rb.nbytes, 3), "buffer_create")
                L.check(L.lib.ohmhip_buffer_write(hb, rb.ctypes.data, rb.nbytes, 0, None, None, None), "buffer_write")
                pb = L._vp()
                L.check(L.lib.ohmhip_buffer_ptr(hb, C.byref(pb)), "buffer_ptr")
                bufs.append((hb, pb, rb.shape[0]))
                del rb
            gmv.integrateRaysDevice(bufs[0][1], bufs[0][2])  # first batch: pool allocation, not timed
            gmv.wait()
            t1 = time.perf_counter()
            for hb, pb, cnt in bufs[1:]:
                gmv.integrateRaysDevice(pb, cnt)
            gmv.wait()
            dt = (time.perf_counter() - t1) / n_mov
            stm = gmv.stats()
            mov_visits = int(stm["voxel_visits"])
            mov_b_alg = 44.0 * n_rays + 8.0 * mov_visits
            mov_tm = [gmv.batchTimings(back) for back in range(n_mov)]
            mov_walk = float(np.mean([t["ms_walk"] for t in mov_tm])) * 1e-3
            extra["C1_moving_sensor"] = {"rays_per_s": n_rays / dt, "ms_per_step": dt * 1e3, "batches": n_mov,
                                         "voxel_visits_last_batch": mov_visits, "walk_kernel_ms": mov_walk * 1e3,
                                         "roofline": {"algorithmic_bytes_per_step": mov_b_alg,
                                                      "frac": mov_b_alg / mov_walk / 1e9 / HBM_PEAK_GBPS,
                                                      "pipeline_frac": mov_b_alg / dt / 1e9 / HBM_PEAK_GBPS},
                                         "sensor_step_m": 0.41, "regions_at_end": int(stm["regions_resident"]),
                                         "note": "the C1 sweep from an origin that advances 0.41 m per batch.  Slower than the "
                                                 "static headline mostly because this synthetic scene is inconsistent from "
                                                 "batch to batch (random range per ray): voxels hit by one batch are crossed "
                                                 "by the next, so the log-odds replay iterates instead of meeting the clamp's "
                                                 "fixed point at once (1.20 ms before the repeated miss became three "
                                                 "operations per application, occMissN)"}
            for hb, _, _ in bufs:
                L.lib.ohmhip_buffer_destroy(hb)
            gmv.close()
        except Exception as exc:
            extra["C1_moving_sensor"] = {"error": repr(exc)}
        # (iii) strong scaling of ONE sensor's stream over 8 ranks: the 1M-ray C1 batch of rank 0 routed to 8
        # maps whose territories were dealt by measured load (azimuth arcs of equal segment load about the sensor, the hub
        # regions every ray crosses dealt one by one); per rank: the rays it receives and what integrating them costs.
        try:
            from ohm_amd import distributed as D
            loads = D.estimate_region_loads(rays, 32 * resolution)
            lpart = D.territories_by_load(loads, 8, 0, (0.05, 0.05, 0.05), 32 * resolution)
            lmaps = [ohm_amd.OccupancyMap(resolution, (32, 32, 32), layers=("occupancy",)) for _ in range(8)]
            lgs = [ohm_amd.GpuMap(mm_, gpu_mem_size=2 << 30) for mm_ in lmaps]
            for r, g_ in enumerate(lgs):
                g_.setRegionPartition(lpart.with_rank(r))
            lshards = [rays] + [np.zeros((0, 3))] * 7
            lstreams = []
            ltm = {}
            linfo = D.integrate_partitioned_in_process(lgs, lshards, timings=ltm, streams_out=lstreams)
            seg, per_rank_ms, walk_ms_rank = [], [], []
            for g_, stream in zip(lgs, lstreams):
                seg.append(int(g_.stats()["ray_region_segments"]))
                # the rank's step at throughput: its stream resident in HBM, five batches back to back
                hb, pb = L._vp(), L._vp()
                L.check(L.lib.ohmhip_buffer_create(C.byref(hb), max(stream.nbytes, 48), 3), "buffer_create")
                L.check(L.lib.ohmhip_buffer_write(hb, stream.ctypes.data, stream.nbytes, 0, None, None, None), "buffer_write")
                L.check(L.lib.ohmhip_buffer_ptr(hb, C.byref(pb)), "buffer_ptr")
                g_.integrateRaysDevice(pb, 2 * stream.shape[0])
                g_.wait()
                t1 = time.perf_counter()
                for _ in range(5):
                    g_.integrateRaysDevice(pb, 2 * stream.shape[0])
                g_.wait()
                per_rank_ms.append((time.perf_counter() - t1) / 5 * 1e3)
                walk_ms_rank.append(float(g_.stats()["ms_walk"]))
                L.lib.ohmhip_buffer_destroy(hb)
                g_.close()
            extra["C1_partitioned_8way_by_load"] = {
                "rays_received_per_rank": [int(v) for v in linfo["received"]],
                "segments_per_rank": seg, "all_segments": int(st["ray_region_segments"]),
                "route_ms_source_rank": round(ltm["route_ms"][0], 4),
                "ms_per_step_per_rank": [round(v, 4) for v in per_rank_ms],
                "walk_ms_per_rank": [round(v, 4) for v in walk_ms_rank],
                "max_rank_ms_per_step": max(per_rank_ms),
                "projected_speedup_8gpu": 1e3 * elapsed / args.steps / max(per_rank_ms),
                "note": "each rank's received stream integrated back to back on THIS GPU (like the headline); routing of "
                        "the whole stream by the source rank (route_ms) and the exchange (48 B per routed ray) excluded.  "
                        "Round 3 (regions dealt by a block hash, every rank given the whole stream): 0.44-0.54 ms per "
                        "rank.  The rank that owns the sensor's own region receives every ray: its set-up + binning of "
                        "1M rays bounds the step whatever the dealing"}
            del lmaps
        except Exception as exc:
            extra["C1_partitioned_8way_by_load"] = {"error": repr(exc)}
        out["other_configs"] = extra
        # The headline is the best case of three (same batch re-integrated into a settled map).  The other two beside it,
        # at the top level: the first pass over a FRESH map and the MOVING sensor.
        fp = extra.get("C1_fresh_map_first_pass", {})
        if "first_pass_ms" in fp:
            out["first_pass"] = {"ms_per_step": fp["first_pass_ms"], "rays_per_s": fp["first_pass_rays_per_s"],
                                 "pipeline_frac": fp["first_pass_pipeline_frac"],
                                 "second_pass_ms": fp["second_pass_ms"],
                                 "note": "fresh map: regions created on the device, every voxel written, one host-"
                                         "synchronised call (no overlap with a next batch)"}
        mv = extra.get("C1_moving_sensor", {})
        if "ms_per_step" in mv:
            out["moving_sensor"] = {"ms_per_step": mv["ms_per_step"], "rays_per_s": mv["rays_per_s"],
                                    "pipeline_frac": mv["roofline"]["pipeline_frac"],
                                    "kernel_frac": mv["roofline"]["frac"],
                                    "note": "the C1 sweep from an origin advancing 0.41 m per batch, batches back to back"}
    if rank == 0 and world == 1 and args.full and not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(rays, resolution, min(args.cpu_sample, n_rays),
                                           all_cores=not args.no_cpu_all_cores)
    elif rank == 0:
        out["cpu_baseline"] = None
    L.lib.ohmhip_buffer_destroy(buf)
    if integ is not None:
        integ.close()
    if comm is not None:
        comm.close()
    gm.close()
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
