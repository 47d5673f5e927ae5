#!/usr/bin/env python3
"""Times the device heightmap on the C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3 regions) carrying occupancy +
mean, against what a host-side heightmap needs first: the download of both layers (ohmhip_map_read_regions of every
region -- what syncVoxels does for a fully dirty map; the CPU column scan that would follow is not even counted).

After warm-up, per round (two rounds, to see the spread) and alternated in the same process: `--calls` back-to-back
ohmhip_map_heightmap calls (host arrays), as many ohmhip_map_heightmap_device calls ended by a device synchronise, and
`--sync-calls` downloads.  Then one call with OHMHIP_HEIGHTMAP_COUNT=1, which makes the kernel count the voxels it
inspects (not part of the timed calls: the counter is an atomic per lane).  Prints one JSON line; nothing is asserted.

Per-kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/heightmap_probe.py
--calls 5 --rounds 1`; the end-to-end figures from the run without the profiler."""
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
    ap.add_argument("--sync-calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--up-axis", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "heightmap_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean"))
    gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    if args.up_axis == 0:  # the X-up timing: the same scene with x and z exchanged
        rays = np.ascontiguousarray(rays[:, ::-1])
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    keys = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16).reshape(-1, 3)
    n_regions = keys.shape[0]
    voxels = map_.regionVoxelVolume()

    hm = ohm_amd.Heightmap(0.1, 0.5, ohm_amd.UpAxis(args.up_axis))
    hm.generate_virtual_surface = True
    hm.set_occupancy_map(gm)
    p = hm.params((0.0, 0.0, 0.0))
    assert hm.build_heightmap((0.0, 0.0, 0.0))
    e = hm.extents
    cells = int(e.ma) * int(e.mb)
    columns = int(e.na) * int(e.nb)
    handle = gm._handle
    populated, written = C.c_uint64(0), C.c_uint64(0)

    def host_call():
        L.check(L.lib.ohmhip_map_heightmap(handle, C.byref(p), hm.occupancy.ctypes.data, hm.voxels.ctypes.data,
                                           hm.mean.ctypes.data, None, C.byref(populated), C.byref(written)), "heightmap")

    bufs = []
    for nbytes in (4 * cells, 24 * cells, 8 * cells, 16):
        b, ptr = L._vp(), L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(b), nbytes, 3), "buffer_create")
        L.check(L.lib.ohmhip_buffer_ptr(b, C.byref(ptr)), "buffer_ptr")
        bufs.append((b, ptr))

    def device_call():
        L.check(L.lib.ohmhip_map_heightmap_device(handle, C.byref(p), bufs[0][1], bufs[1][1], bufs[2][1], None,
                                                  bufs[3][1]), "heightmap_device")

    occ = np.empty((n_regions, voxels), dtype=np.float32)
    mean = np.empty((n_regions, voxels, 2), dtype=np.uint32)
    occ_dsts = (C.c_void_p * n_regions)(*[occ[i].ctypes.data for i in range(n_regions)])
    mean_dsts = (C.c_void_p * n_regions)(*[mean[i].ctypes.data for i in range(n_regions)])

    def sync_layers():
        L.check(L.lib.ohmhip_map_read_regions(handle, L.LID_OCCUPANCY, keys.ctypes.data, n_regions, occ_dsts), "read")
        L.check(L.lib.ohmhip_map_read_regions(handle, L.LID_MEAN, keys.ctypes.data, n_regions, mean_dsts), "read")

    def timed(fn, n):
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        return (time.perf_counter() - t0) * 1e3 / n

    for _ in range(3):
        host_call()
        device_call()
    sync_layers()
    rounds = []
    for _ in range(args.rounds):
        rounds.append({"ms_heightmap_host": timed(host_call, args.calls),
                       "ms_heightmap_device": timed(device_call, args.calls),
                       "ms_sync_occupancy_mean": timed(sync_layers, args.sync_calls)})
    os.environ["OHMHIP_HEIGHTMAP_COUNT"] = "1"
    host_call()  # prints the kernel's count of inspected voxels on stderr
    del os.environ["OHMHIP_HEIGHTMAP_COUNT"]
    best = min(r["ms_heightmap_host"] for r in rounds)
    result = {
        "map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy + mean" % args.rays, "up_axis": args.up_axis,
        "regions": n_regions, "columns": columns, "cells": cells, "populated": int(populated.value),
        "cells_written": int(written.value), "result_bytes": 36 * cells,
        "layer_bytes": n_regions * voxels * 12, "occupancy_bytes": n_regions * voxels * 4, "rounds": rounds,
        "columns_per_s_host_call": columns / (best * 1e-3),
        "speedup_over_sync": min(r["ms_sync_occupancy_mean"] for r in rounds) / best,
        "device": ohm_amd.device_info(0)["name"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    for b, _ in bufs:
        L.lib.ohmhip_buffer_destroy(b)


if __name__ == "__main__":
    main()
