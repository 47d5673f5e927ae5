#!/usr/bin/env python3
"""Times one full copy of the C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3 regions, occupancy + mean) from one
device map into another: ohmhip_map_copy (one k_copy_map launch, device to device) against the route a caller had
before it, ohmhip_map_read_regions of both layers into host blocks and ohmhip_map_write_regions of them into the second
map.  Needs a HIP device.

After warm-up (both destinations then hold every region: the timed calls overwrite), per round (two rounds, to see the
spread) and alternated in the same process: `--calls` back-to-back ohmhip_map_copy calls and `--calls` host-route
passes, each series ended by a device synchronise; the host route's two halves are also timed on their own.  The copy's
result is compared with the source once, byte for byte.  Prints one JSON line; nothing else is asserted.

The byte model: every copied byte is read once and written once, so k_copy_map moves 2 x layer_bytes.  With
--kernel-ms MS (milliseconds per k_copy_map call, from a run of its own under `rocprofv3 --kernel-trace --stats -- python
scripts/copy_probe.py --calls 5 --rounds 1`) the line also carries the kernel's bytes per second."""
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
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernel-ms", type=float, default=None, metavar="MS")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "copy_probe needs a HIP device"
    layers = ("occupancy", "mean")

    def new_map():
        return ohm_amd.GpuMap(ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=layers), gpu_mem_size=8 << 30)

    src, dst, dst_host = new_map(), new_map(), new_map()
    rays = synth.rays_c1(n=args.rays)
    assert src.integrateRays(rays) == rays.shape[0]
    src.wait()
    keys = np.ascontiguousarray(src.regionKeys(), dtype=np.int16).reshape(-1, 3)
    n_regions = keys.shape[0]
    voxels = src.map().regionVoxelVolume()

    stats = L.CopyStats()

    def device_copy():
        L.check(L.lib.ohmhip_map_copy(dst._handle, src._handle, None, C.byref(stats)), "copy")

    occ = np.empty((n_regions, voxels), dtype=np.float32)
    mean = np.empty((n_regions, voxels, 2), dtype=np.uint32)
    occ_ptrs = (C.c_void_p * n_regions)(*[occ[i].ctypes.data for i in range(n_regions)])
    mean_ptrs = (C.c_void_p * n_regions)(*[mean[i].ctypes.data for i in range(n_regions)])

    def host_read(gm=src):
        L.check(L.lib.ohmhip_map_read_regions(gm._handle, L.LID_OCCUPANCY, keys.ctypes.data, n_regions, occ_ptrs), "read")
        L.check(L.lib.ohmhip_map_read_regions(gm._handle, L.LID_MEAN, keys.ctypes.data, n_regions, mean_ptrs), "read")

    def host_write():
        L.check(L.lib.ohmhip_map_write_regions(dst_host._handle, L.LID_OCCUPANCY, keys.ctypes.data, n_regions, occ_ptrs),
                "write")
        L.check(L.lib.ohmhip_map_write_regions(dst_host._handle, L.LID_MEAN, keys.ctypes.data, n_regions, mean_ptrs), "write")

    def host_route():
        host_read()
        host_write()

    def timed(fn, calls):
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        return (time.perf_counter() - t0) * 1e3 / calls

    for _ in range(2):
        device_copy()
        host_route()
    assert stats.regions_passed == n_regions and stats.regions_created == 0
    layer_bytes = n_regions * voxels * 12
    assert stats.bytes_copied == layer_bytes
    want = (occ.copy(), mean.copy())
    host_read(dst)
    identical = bool(np.array_equal(occ.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(mean, want[1]))
    host_read()

    rounds = []
    for _ in range(args.rounds):
        rounds.append({"ms_map_copy": timed(device_copy, args.calls), "ms_host_route": timed(host_route, args.calls),
                       "ms_host_read": timed(host_read, args.calls), "ms_host_write": timed(host_write, args.calls)})
    best = min(r["ms_map_copy"] for r in rounds)
    result = {"map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy + mean" % args.rays, "regions": n_regions,
              "layer_bytes": layer_bytes, "model_kernel_bytes": 2 * layer_bytes, "copy_equals_source": identical,
              "rounds": rounds, "host_route_over_copy": min(r["ms_host_route"] for r in rounds) / best,
              "copy_call_bytes_per_s": layer_bytes / (best * 1e-3), "device": ohm_amd.device_info(0)["name"]}
    if args.kernel_ms:
        result["kernel_bytes_per_s"] = 2 * layer_bytes / (args.kernel_ms * 1e-3)
        result["kernel_payload_bytes_per_s"] = layer_bytes / (args.kernel_ms * 1e-3)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
