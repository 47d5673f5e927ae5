#!/usr/bin/env python3
"""Times the point queries on the C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3 regions, occupancy + mean), each
beside its host-side alternative in the same process.  Needs a HIP device.

  one query      ohmhip_map_nearest_neighbours, 1 near point, r = 2 m
  1 024 queries  ohmhip_map_nearest_neighbours, 1 024 near points in one call, r = 1 m
  10^5 keys      ohmhip_map_read_voxels of the occupancy layer at 10^5 keys (ohmhip_map_voxel_keys of sample points)

The alternative is what a caller without these entry points does: ohmhip_map_read_regions of the regions concerned --
the regions of the queries' boxes that the map holds, or the regions of the keys -- and a numpy scan of the downloaded
blocks (the NearestNeighbours test in float32, or a gather).  Every series is warmed, starts and ends with a device
synchronise and is timed by device events recorded around it (the calls are synchronous, so the events bracket finished
work) and by the host clock.  The results of the two ways are compared (counts and occupancy values must agree).  Prints
one JSON line; no speed is asserted."""
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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--keys", type=int, default=100_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "point_query_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean"))
    gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    handle = gm._handle
    samples = rays[1::2]
    present = {tuple(k) for k in gm.regionKeys().tolist()}
    voxels = map_.regionVoxelVolume()
    threshold = np.float32(map_.occupancy_threshold_value)
    region_dim = 3.2

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
        return {"ms_events": ms.value / calls, "ms_host_clock": host_ms, "calls": calls}

    def read_regions(keys):
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        blocks = np.empty((keys.shape[0], voxels), dtype=np.float32)
        dsts = (C.c_void_p * keys.shape[0])(*[blocks[i].ctypes.data for i in range(keys.shape[0])])
        L.check(L.lib.ohmhip_map_read_regions(handle, L.LID_OCCUPANCY, keys.ctypes.data, keys.shape[0], dsts), "read")
        return blocks

    index = np.arange(voxels)
    local = np.stack([index % 32, (index // 32) % 32, index // 1024], axis=1).astype(np.float64)

    def box_regions(point, radius):
        lo = np.floor((point - radius) / region_dim + 0.5).astype(int)
        hi = np.floor((point + radius) / region_dim + 0.5).astype(int)
        return [(x, y, z) for z in range(lo[2], hi[2] + 1) for y in range(lo[1], hi[1] + 1)
                for x in range(lo[0], hi[0] + 1) if (x, y, z) in present]

    def host_neighbours(points, radius):
        """Download the regions of the boxes, then the query's test per voxel in numpy: results per query."""
        boxes = [box_regions(p, radius) for p in points]
        wanted = sorted({r for box in boxes for r in box})
        blocks = dict(zip(wanted, read_regions(wanted))) if wanted else {}
        radius2 = np.float32(radius) * np.float32(radius)
        counts = np.zeros(len(points), dtype=np.uint64)
        for i, (p, box) in enumerate(zip(points, boxes)):
            q = p.astype(np.float32)
            for r in box:
                v = blocks[r]
                hit = np.nonzero((v != np.inf) & (v >= threshold))[0]
                if not hit.size:
                    continue
                centre = ((np.asarray(r) * region_dim - 0.5 * region_dim) + local[hit] * 0.1 + 0.05).astype(np.float32)
                d = centre - q
                r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                counts[i] += int((r2 <= radius2).sum())
        return counts, len(wanted)

    result = {"map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy + mean" % args.rays, "regions": len(present),
              "device": ohm_amd.device_info(0)["name"]}

    for name, points, radius in (("one_query_r2", samples[len(samples) // 2:len(samples) // 2 + 1], 2.0),
                                 ("queries_r1", samples[::max(1, len(samples) // args.queries)][:args.queries], 1.0)):
        points = np.ascontiguousarray(points, dtype=np.float64)
        counts, keys, ranges = gm.nearestNeighbours(points, radius)
        total = int(counts.sum())
        p = L.NeighboursParams(radius, 0)
        n = C.c_uint64(0)
        out_counts = np.zeros(len(points), dtype=np.uint64)
        out_keys = np.empty(max(total, 1), dtype=ohm_amd.GPU_KEY_DTYPE)
        out_ranges = np.empty(max(total, 1), dtype=np.float32)

        def device_call():
            L.check(L.lib.ohmhip_map_nearest_neighbours(handle, points.ctypes.data, len(points), C.byref(p), max(total, 1),
                                                        out_counts.ctypes.data, out_keys.ctypes.data,
                                                        out_ranges.ctypes.data, C.byref(n)), "nearest_neighbours")

        for _ in range(3):
            device_call()
        host_counts, regions_read = host_neighbours(points, radius)  # (also the warm-up of the alternative)
        assert np.array_equal(host_counts, counts), "the two ways disagree"
        result[name] = {"queries": len(points), "radius": radius, "results": total,
                        "result_bytes": 14 * total + 8 * len(points), "regions_downloaded": regions_read,
                        "download_bytes": 4 * voxels * regions_read,
                        "device": timed(device_call, args.calls),
                        "read_regions_and_numpy": timed(lambda: host_neighbours(points, radius), args.host_calls)}

    key_points = np.ascontiguousarray(samples[::max(1, len(samples) // args.keys)][:args.keys])
    keys = gm.voxelKeys(key_points)
    values = np.empty(len(keys), dtype=np.float32)
    flags = np.empty(len(keys), dtype=np.uint8)

    def read_call():
        L.check(L.lib.ohmhip_map_read_voxels(handle, L.LID_OCCUPANCY, keys.ctypes.data, len(keys), values.ctypes.data,
                                             flags.ctypes.data), "read_voxels")

    def host_read():
        regions, inverse = np.unique(keys["region"], axis=0, return_inverse=True)
        blocks = read_regions(regions)
        v = keys["voxel"].astype(np.int64)
        return blocks[inverse.reshape(-1), v[:, 0] + 32 * v[:, 1] + 1024 * v[:, 2]], regions.shape[0]

    for _ in range(3):
        read_call()
    host_values, regions_read = host_read()
    assert flags.all() and np.array_equal(host_values.view(np.uint32), values.view(np.uint32)), "the two ways disagree"
    result["occupancy_read"] = {"keys": len(keys), "result_bytes": 5 * len(keys), "key_bytes": 10 * len(keys),
                                "regions_downloaded": regions_read, "download_bytes": 4 * voxels * regions_read,
                                "device": timed(read_call, args.calls),
                                "read_regions_and_numpy": timed(host_read, args.host_calls)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    for e in events:
        L.lib.ohmhip_event_destroy(e)


if __name__ == "__main__":
    main()
