#!/usr/bin/env python3
"""Times the flood-fill heightmap (ohmhip_map_heightmap_fill / _device) on the map of scripts/heightmap_probe.py -- the
C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3 regions) carrying occupancy + mean -- with that probe's protocol, against
the planar build on the same map in the same process and against the download of both layers (ohmhip_map_read_regions of
every region), the floor of any host-side fill.

After warm-up, per round (two rounds) and alternated: `--calls` back-to-back fill calls into host arrays, as many into
device arrays, as many planar calls into host arrays, and `--sync-calls` downloads, each leg ended by a device
synchronise.  The walk's counts (visits, generations, largest generation) come from the call's own stats.  Prints one
JSON line; nothing is asserted.

Per-kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python
scripts/heightmap_fill_probe.py --calls 2 --rounds 1 --sync-calls 1`; the end-to-end figures from the run without the
profiler.  The share of a call that is launches and read-backs is the call's time less the kernels' total."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "heightmap_fill_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean"))
    gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    keys = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16).reshape(-1, 3)
    n_regions = keys.shape[0]
    voxels = map_.regionVoxelVolume()

    hm = ohm_amd.Heightmap(0.1, 0.5, ohm_amd.UpAxis.kZ)
    hm.generate_virtual_surface = True
    hm.set_occupancy_map(gm)
    planar = hm.params((0.0, 0.0, 0.0))
    hm.mode = ohm_amd.HeightmapMode.kSimpleFill
    fill = hm.params((0.0, 0.0, 0.0))
    assert hm.build_heightmap((0.0, 0.0, 0.0))
    e = hm.extents
    cells = int(e.ma) * int(e.mb)
    columns = int(e.na) * int(e.nb)
    handle = gm._handle
    stats = L.HeightmapFillStats()
    populated, written = C.c_uint64(0), C.c_uint64(0)

    def fill_host():
        L.check(L.lib.ohmhip_map_heightmap_fill(handle, C.byref(fill), hm.occupancy.ctypes.data, hm.voxels.ctypes.data,
                                                hm.mean.ctypes.data, None, None, 0, C.byref(stats)), "fill")

    bufs = []
    for nbytes in (4 * cells, 24 * cells, 8 * cells):
        b, ptr = L._vp(), L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(b), nbytes, 3), "buffer_create")
        L.check(L.lib.ohmhip_buffer_ptr(b, C.byref(ptr)), "buffer_ptr")
        bufs.append((b, ptr))

    def fill_device():
        L.check(L.lib.ohmhip_map_heightmap_fill_device(handle, C.byref(fill), bufs[0][1], bufs[1][1], bufs[2][1], None,
                                                       None, 0, C.byref(stats)), "fill_device")

    def planar_host():
        L.check(L.lib.ohmhip_map_heightmap(handle, C.byref(planar), hm.occupancy.ctypes.data, hm.voxels.ctypes.data,
                                           hm.mean.ctypes.data, None, C.byref(populated), C.byref(written)), "heightmap")

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

    for _ in range(2):
        fill_host()
        fill_device()
        planar_host()
    sync_layers()
    rounds = []
    for _ in range(args.rounds):
        rounds.append({"ms_fill_host": timed(fill_host, args.calls), "ms_fill_device": timed(fill_device, args.calls),
                       "ms_planar_host": timed(planar_host, args.calls),
                       "ms_sync_occupancy_mean": timed(sync_layers, args.sync_calls)})
    best = min(r["ms_fill_host"] for r in rounds)
    result = {
        "map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy + mean" % args.rays, "regions": n_regions,
        "columns": columns, "cells": cells, "visits": int(stats.visits), "generations": int(stats.generations),
        "largest_generation": int(stats.largest_generation), "revisits": int(stats.revisits),
        "populated": int(stats.populated), "cells_written": int(stats.cells),
        "planar_populated": int(populated.value), "layer_bytes": n_regions * voxels * 12, "rounds": rounds,
        "us_per_generation": best * 1e3 / max(1, int(stats.generations)),
        "fill_over_planar": best / min(r["ms_planar_host"] for r in rounds),
        "fill_over_sync": best / min(r["ms_sync_occupancy_mean"] for r in rounds),
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
