#!/usr/bin/env python3
"""Times MISS edits by key on the C1 map of bench.py (lidar rays in 5 batches, 0.1 m, 32^3 regions, occupancy + mean):
ohmhip_map_integrate_voxels against the only route a caller had before it for the same result --
ohmhip_map_read_regions of the touched regions' occupancy, the edit in numpy, ohmhip_map_write_regions and
ohmhip_map_mark_dirty.  Needs a HIP device.

K in --counts edits are drawn (a) "box": from the keys of a 2 m box around the sensor (GpuMap.keyRange), with
repetition once K exceeds the box, and (b) "uniform": uniformly over the voxels of the resident regions.  Per workload
and K: two warm-up calls of each route, then per round (two rounds, to see the spread) --calls calls of each, alternated
in the same process, each series between two events (ohmhip_event_elapsed_ms) and on the host clock; both routes are
blocking calls, so the two clocks agree.  The baseline's numpy edit applies the same n misses per voxel with the
model's clamp (no saturation in the default configuration); after the timed rounds of a row the touched regions of
the two maps, which received the same calls, are compared once.  Prints one JSON line; nothing else is asserted.

Per-kernel times: a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/voxel_edit_probe.py --counts
1000000 --workloads uniform --calls 3 --rounds 1 --only-edit`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--counts", type=int, nargs="+", default=[1000, 100000, 1000000])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--workloads", nargs="+", default=["box", "uniform"], choices=["box", "uniform"])
    ap.add_argument("--only-edit", action="store_true", help="skip the baseline (profiling runs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import GPU_KEY_DTYPE
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "voxel_edit_probe needs a HIP device"
    layers = ("occupancy", "mean")
    dim = 32
    voxels = dim ** 3

    def new_map():
        gm = ohm_amd.GpuMap(ohm_amd.OccupancyMap(0.1, (dim,) * 3, layers=layers), gpu_mem_size=8 << 30)
        rays = synth.rays_c1(n=args.rays)
        step = 2 * (args.rays // 5)
        for at in range(0, rays.shape[0], step):
            assert gm.integrateRays(rays[at:at + step]) == min(step, rays.shape[0] - at)
        gm.wait()
        return gm

    gm, twin = new_map(), new_map()
    regions = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16).reshape(-1, 3)
    miss, vmin = np.float32(gm.map().miss_value), np.float32(gm.map().min_voxel_value)
    events = []
    for _ in range(2):
        e = L._vp()
        L.check(L.lib.ohmhip_event_create(C.byref(e)), "event_create")
        events.append(e)

    def timed(fn, calls):
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        L.check(L.lib.ohmhip_event_record(events[0], None), "record")
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        host_ms = (time.perf_counter() - t0) * 1e3 / calls
        L.check(L.lib.ohmhip_event_record(events[1], None), "record")
        L.check(L.lib.ohmhip_event_wait(events[1]), "wait")
        ms = C.c_float(0)
        L.check(L.lib.ohmhip_event_elapsed_ms(events[0], events[1], C.byref(ms)), "elapsed")
        return {"ms_events": ms.value / calls, "ms_host_clock": host_ms}

    def draw(workload, count, rng):
        if workload == "box":
            box = gm.keyRange((-0.95, -0.95, -0.95), (1.05, 1.05, 1.05))       # 2 m around the sensor at 0.05
            return box[rng.integers(0, box.shape[0], size=count)] if count > box.shape[0] else box[:count]
        keys = np.zeros(count, dtype=GPU_KEY_DTYPE)
        keys["region"] = regions[rng.integers(0, regions.shape[0], size=count)]
        keys["voxel"][:, :3] = rng.integers(0, dim, size=(count, 3))
        return keys

    def edit_call(target, keys):
        rec = keys.view(np.uint8).reshape(-1, 10)
        stats = L.VoxelEditStats()

        def call():
            L.check(L.lib.ohmhip_map_integrate_voxels(target._handle, None, L.EDIT_MISS, rec.ctypes.data, None,
                                                      rec.shape[0], C.byref(stats)), "integrate_voxels")
        return call, stats

    def baseline_call(target, keys):
        packed = (keys["region"].astype(np.int64) + 32768) @ np.array([1, 1 << 16, 1 << 32], dtype=np.int64)
        order = np.argsort(packed, kind="stable")
        uniq, first, counts = np.unique(packed[order], return_index=True, return_counts=True)
        touched = np.ascontiguousarray(keys["region"][order][first], dtype=np.int16)
        index = (keys["voxel"][:, 0].astype(np.int64) + dim * (keys["voxel"][:, 1].astype(np.int64) +
                                                                 dim * keys["voxel"][:, 2].astype(np.int64)))[order]
        region_of = np.repeat(np.arange(len(uniq)), counts)
        blocks = np.empty((len(uniq), voxels), dtype=np.float32)
        ptrs = (C.c_void_p * len(uniq))(*[blocks[i].ctypes.data for i in range(len(uniq))])
        slots = np.zeros(len(uniq), dtype=np.uint32)

        def call():
            L.check(L.lib.ohmhip_map_read_regions(target._handle, L.LID_OCCUPANCY, touched.ctypes.data, len(uniq), ptrs),
                    "read")
            flat = blocks.reshape(-1)
            n = np.bincount(region_of * voxels + index, minlength=flat.shape[0]).astype(np.int64)
            hit = np.flatnonzero(n)
            x = flat[hit]
            x = np.where(np.isinf(x), np.float32(0.0), x)
            for _ in range(int(n[hit].max())):                                 # one rounding per miss, as the model
                live = n[hit] > 0
                x = np.where(live, np.maximum(vmin, x + miss), x).astype(np.float32)
                n[hit] -= 1
            flat[hit] = x
            L.check(L.lib.ohmhip_map_write_regions(target._handle, L.LID_OCCUPANCY, touched.ctypes.data, len(uniq), ptrs),
                    "write")
            L.check(L.lib.ohmhip_map_ensure_regions(target._handle, touched.ctypes.data, len(uniq), slots.ctypes.data),
                    "slots")
            L.check(L.lib.ohmhip_map_mark_dirty(target._handle, slots.ctypes.data, len(uniq)), "mark_dirty")
        return call, touched

    rng = np.random.default_rng(1)
    results = []
    for workload in args.workloads:
        for count in args.counts:
            keys = draw(workload, count, rng)
            edit, stats = edit_call(gm, keys)
            base, touched = baseline_call(twin, keys)
            for _ in range(2):
                edit()
                if not args.only_edit:
                    base()
            rounds = []
            for _ in range(args.rounds):
                r = {"edit": timed(edit, args.calls)}
                if not args.only_edit:
                    r["baseline"] = timed(base, args.calls)
                rounds.append(r)
            row = {"workload": workload, "count": count, "distinct_voxels": int(stats.distinct_voxels),
                   "regions_touched": int(stats.regions_touched), "rounds": rounds}
            if not args.only_edit:
                best_edit = min(r["edit"]["ms_events"] for r in rounds)
                best_base = min(r["baseline"]["ms_events"] for r in rounds)
                row["baseline_over_edit"] = best_base / best_edit
                # the same number of calls went to both maps: their touched regions must hold the same bytes
                got = np.empty((touched.shape[0], voxels), dtype=np.float32)
                want = np.empty_like(got)
                for target, out in ((gm, got), (twin, want)):
                    ptrs = (C.c_void_p * touched.shape[0])(*[out[i].ctypes.data for i in range(touched.shape[0])])
                    L.check(L.lib.ohmhip_map_read_regions(target._handle, L.LID_OCCUPANCY, touched.ctypes.data,
                                                          touched.shape[0], ptrs), "read")
                row["routes_agree"] = bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
            results.append(row)
    line = json.dumps({"map": "C1 rays (%d) in 5 batches, 0.1 m, 32^3 regions, occupancy + mean" % args.rays,
                       "regions": int(regions.shape[0]), "results": results, "device": ohm_amd.device_info(0)["name"]})
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
