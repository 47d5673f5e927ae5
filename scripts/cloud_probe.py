#!/usr/bin/env python3
"""Times the device point cloud (OCCUPANCY mode) on the C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3 regions)
carrying occupancy + mean, against what a host-side export needs first: the download of both layers
(ohmhip_map_read_regions of every region -- what syncVoxels does for a fully dirty map; the host scan of 32 768 voxels
per region that would follow is not even counted).  Needs a HIP device.

After warm-up, per round (two rounds, to see the spread) and alternated in the same process: `--calls` back-to-back
ohmhip_map_cloud calls (host arrays), as many ohmhip_map_cloud_device calls, and `--sync-calls` downloads, each series
ended by a device synchronise.  Prints one JSON line; nothing is asserted.

The byte model (what the kernels must move): the count pass reads the selecting layer once (4 B per voxel of every
region); the emit pass reads it again, plus 8 B of mean per point, and writes 38 B per point.  With --kernel-ms COUNT
EMIT (milliseconds per call, from a run of its own under `rocprofv3 --kernel-trace --stats -- python
scripts/cloud_probe.py --calls 5 --rounds 1`) the line also carries bytes per second over kernel time."""
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
    ap.add_argument("--export-free", action="store_true")
    ap.add_argument("--kernel-ms", type=float, nargs=2, default=None, metavar=("COUNT", "EMIT"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "cloud_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean"))
    gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    keys = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16).reshape(-1, 3)
    n_regions = keys.shape[0]
    voxels = map_.regionVoxelVolume()
    handle = gm._handle

    p = ohm_amd.cloud_params(ohm_amd.CloudMode.OCCUPANCY, export_free=args.export_free)
    cloud = ohm_amd.extract_cloud(gm, ohm_amd.CloudMode.OCCUPANCY, export_free=args.export_free)
    points = cloud.count
    capacity = max(points, 1)
    positions = np.empty((capacity, 3), dtype=np.float64)
    point_keys = np.empty(capacity, dtype=ohm_amd.GPU_KEY_DTYPE)
    values = np.empty(capacity, dtype=np.float32)
    n = C.c_uint64(0)

    def host_call():
        L.check(L.lib.ohmhip_map_cloud(handle, C.byref(p), capacity, positions.ctypes.data, point_keys.ctypes.data,
                                       values.ctypes.data, C.byref(n)), "cloud")

    bufs = []
    for nbytes in (24 * capacity, 10 * capacity, 4 * capacity, 16):
        b, ptr = L._vp(), L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(b), nbytes, 3), "buffer_create")
        L.check(L.lib.ohmhip_buffer_ptr(b, C.byref(ptr)), "buffer_ptr")
        bufs.append((b, ptr))

    def device_call():
        L.check(L.lib.ohmhip_map_cloud_device(handle, C.byref(p), capacity, bufs[0][1], bufs[1][1], bufs[2][1],
                                              bufs[3][1]), "cloud_device")

    occ = np.empty((n_regions, voxels), dtype=np.float32)
    mean = np.empty((n_regions, voxels, 2), dtype=np.uint32)
    occ_dsts = (C.c_void_p * n_regions)(*[occ[i].ctypes.data for i in range(n_regions)])
    mean_dsts = (C.c_void_p * n_regions)(*[mean[i].ctypes.data for i in range(n_regions)])

    def sync_layers():
        L.check(L.lib.ohmhip_map_read_regions(handle, L.LID_OCCUPANCY, keys.ctypes.data, n_regions, occ_dsts), "read")
        L.check(L.lib.ohmhip_map_read_regions(handle, L.LID_MEAN, keys.ctypes.data, n_regions, mean_dsts), "read")

    def timed(fn, calls):
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        return (time.perf_counter() - t0) * 1e3 / calls

    for _ in range(3):
        host_call()
        device_call()
    sync_layers()
    assert n.value == points
    rounds = []
    for _ in range(args.rounds):
        rounds.append({"ms_cloud_host": timed(host_call, args.calls),
                       "ms_cloud_device": timed(device_call, args.calls),
                       "ms_sync_occupancy_mean": timed(sync_layers, args.sync_calls)})
    best = min(r["ms_cloud_host"] for r in rounds)
    layer_voxels = n_regions * voxels
    count_bytes = 4 * layer_voxels
    emit_bytes = 4 * layer_voxels + (8 + 38) * points
    result = {
        "map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy + mean" % args.rays, "export_free": args.export_free,
        "regions": n_regions, "voxels": layer_voxels, "points": points, "result_bytes": 38 * points,
        "layer_bytes": layer_voxels * 12, "model_count_bytes": count_bytes, "model_emit_bytes": emit_bytes,
        "rounds": rounds, "speedup_over_sync": min(r["ms_sync_occupancy_mean"] for r in rounds) / best,
        "device": ohm_amd.device_info(0)["name"]}
    if args.kernel_ms:
        result["count_bytes_per_s"] = count_bytes / (args.kernel_ms[0] * 1e-3)
        result["emit_bytes_per_s"] = emit_bytes / (args.kernel_ms[1] * 1e-3)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    for b, _ in bufs:
        L.lib.ohmhip_buffer_destroy(b)


if __name__ == "__main__":
    main()
