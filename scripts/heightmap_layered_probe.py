#!/usr/bin/env python3
"""Times the layered heightmaps (ohmhip_map_heightmap_layered, kLayeredFill and kLayeredFillUnordered) on the map and
with the settings and protocol of scripts/heightmap_fill_probe.py -- the C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3
regions) carrying occupancy + mean, min_clearance 0.5, virtual surfaces on, reference (0, 0, 0) -- against the simple
fill and the planar build on the same map in the same process and against the download of both layers
(ohmhip_map_read_regions of every region), the floor of any host-side build.

After warm-up, per round (two rounds) and alternated: `--calls` back-to-back calls of each build into host arrays and
`--sync-calls` downloads, each leg ended by a device synchronise.  The walk's counts (visits, generations, largest
generation, layers, ...) come from the call's own stats.  Prints one JSON line; nothing is asserted.

Per-kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python
scripts/heightmap_layered_probe.py --calls 2 --rounds 1 --sync-calls 1`; the end-to-end figures from the run without
the profiler."""
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
    ap.add_argument("--filter-threshold", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "heightmap_layered_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean"))
    gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    keys = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16).reshape(-1, 3)
    n_regions = keys.shape[0]
    voxels = map_.regionVoxelVolume()

    hm = ohm_amd.LayeredHeightmap(0.1, 0.5, ohm_amd.UpAxis.kZ)
    hm.generate_virtual_surface = True
    hm.virtual_surface_filter_threshold = args.filter_threshold
    hm.set_occupancy_map(gm)
    hm.mode = ohm_amd.HeightmapMode.kPlanar
    planar = hm.params((0.0, 0.0, 0.0))
    hm.mode = ohm_amd.HeightmapMode.kSimpleFill
    fill = hm.params((0.0, 0.0, 0.0))
    hm.mode = ohm_amd.HeightmapMode.kLayeredFillUnordered
    unordered = hm.layered_params((0.0, 0.0, 0.0))
    hm.mode = ohm_amd.HeightmapMode.kLayeredFill
    ordered = hm.layered_params((0.0, 0.0, 0.0))
    assert hm.build_heightmap((0.0, 0.0, 0.0))
    e = hm.extents
    slots = int(hm.occupancy.shape[0])
    cells = int(e.ma) * int(e.mb)
    columns = int(e.na) * int(e.nb)
    handle = gm._handle
    layered_stats = {"ordered": L.HeightmapLayeredStats(), "unordered": L.HeightmapLayeredStats()}
    fill_stats = L.HeightmapFillStats()
    populated, written = C.c_uint64(0), C.c_uint64(0)
    occupancy, cell_voxels, cell_mean = hm.occupancy, hm.voxels, hm.mean

    def layered_host(name, params):
        def call():
            L.check(L.lib.ohmhip_map_heightmap_layered(handle, C.byref(params), slots, occupancy.ctypes.data,
                                                       cell_voxels.ctypes.data, cell_mean.ctypes.data, None, None, None, 0,
                                                       C.byref(layered_stats[name])), "layered")
        return call

    def fill_host():
        L.check(L.lib.ohmhip_map_heightmap_fill(handle, C.byref(fill), occupancy.ctypes.data, cell_voxels.ctypes.data,
                                                cell_mean.ctypes.data, None, None, 0, C.byref(fill_stats)), "fill")

    def planar_host():
        L.check(L.lib.ohmhip_map_heightmap(handle, C.byref(planar), occupancy.ctypes.data, cell_voxels.ctypes.data,
                                           cell_mean.ctypes.data, None, C.byref(populated), C.byref(written)), "heightmap")

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

    legs = (("ms_layered_ordered_host", layered_host("ordered", ordered), args.calls),
            ("ms_layered_unordered_host", layered_host("unordered", unordered), args.calls),
            ("ms_fill_host", fill_host, args.calls), ("ms_planar_host", planar_host, args.calls),
            ("ms_sync_occupancy_mean", sync_layers, args.sync_calls))
    for _ in range(2):
        for _, fn, _ in legs[:4]:
            fn()
    sync_layers()
    rounds = [{name: timed(fn, n) for name, fn, n in legs} for _ in range(args.rounds)]

    def best(name):
        return min(r[name] for r in rounds)

    def counts(st):
        return {name: int(getattr(st, name)) for name, _ in st._fields_}

    result = {
        "map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy + mean" % args.rays, "regions": n_regions,
        "columns": columns, "cells": cells, "slots": slots, "filter_threshold": args.filter_threshold,
        "ordered": counts(layered_stats["ordered"]), "unordered": counts(layered_stats["unordered"]),
        "fill": counts(fill_stats), "planar_populated": int(populated.value),
        "layer_bytes": n_regions * voxels * 12, "rounds": rounds,
        "us_per_generation": best("ms_layered_ordered_host") * 1e3 / max(1, int(layered_stats["ordered"].generations)),
        "ordered_over_fill": best("ms_layered_ordered_host") / best("ms_fill_host"),
        "ordered_over_planar": best("ms_layered_ordered_host") / best("ms_planar_host"),
        "ordered_over_sync": best("ms_layered_ordered_host") / best("ms_sync_occupancy_mean"),
        "device": ohm_amd.device_info(0)["name"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
