#!/usr/bin/env python3
"""Times covariance ellipsoid extraction on the C2 map of bench.py (GpuNdtMap, 10^6 rays of synth.rays_c2, 0.2 m, 32^3
regions) beside the download a caller without it starts from.  Needs a HIP device.

  ellipsoids   ohmhip_map_covariance_ellipsoids into host arrays sized by a count call: position, axes, scales, key and
               value of every occupied voxel
  download     ohmhip_map_read_regions of the occupancy, mean and covariance layers of every region into preallocated
               host blocks -- what a host-side solve needs before it can start; the solve itself is not timed

Every series is warmed, starts and ends with a device synchronise and is timed by the host clock around it.  Bytes are
computed from the array sizes, not measured.  Prints one JSON line; no speed is asserted."""
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
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_probe.json"))
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth
    from ohm_amd.gpumap import LAYERS

    assert ohm_amd.device_count() > 0, "covariance_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.2, (32, 32, 32), layers=("occupancy", "mean", "covariance"))
    gm = ohm_amd.GpuNdtMap(map_, gpu_mem_size=24 << 30)
    rays = synth.rays_c2(n=args.rays)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    handle = gm._handle

    def timed(fn, calls):
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        return {"ms_host_clock": (time.perf_counter() - t0) * 1e3 / calls, "calls": calls}

    p = ohm_amd.cloud_params()
    total = C.c_uint64(0)
    L.check(L.lib.ohmhip_map_covariance_ellipsoids_count(handle, C.byref(p), C.byref(total)), "count")
    n = int(total.value)
    positions, axes, scales = np.empty((n, 3)), np.empty((n, 3, 3)), np.empty((n, 3))
    keys, values = np.empty(n, dtype=ohm_amd.GPU_KEY_DTYPE), np.empty(n, dtype=np.float32)

    def ellipsoids():
        L.check(L.lib.ohmhip_map_covariance_ellipsoids(handle, C.byref(p), n, positions.ctypes.data, axes.ctypes.data,
                                                       scales.ctypes.data, keys.ctypes.data, values.ctypes.data,
                                                       C.byref(total)), "ellipsoids")

    regions = np.ascontiguousarray(gm.regionKeys(), dtype=np.int16)
    volume = map_.regionVoxelVolume()
    blocks = {}
    for name in ("occupancy", "mean", "covariance"):
        lid, dtype, comps = LAYERS[name]
        held = [np.empty(volume * comps, dtype=dtype) for _ in range(len(regions))]
        blocks[name] = (lid, held, (C.c_void_p * len(held))(*[b.ctypes.data for b in held]))

    def download():
        for lid, _, ptrs in blocks.values():
            L.check(L.lib.ohmhip_map_read_regions(handle, lid, regions.ctypes.data, len(regions), ptrs), "read_regions")

    for _ in range(2):
        ellipsoids()
        download()
    # the two ways describe the same voxels: the axes of a few rows against the host evaluation of the rule
    host_cov, _ = gm.readVoxels(keys[:1000], "covariance")
    host = ohm_amd.covariance_decompose(host_cov)
    assert np.array_equal(host.eigenvectors, axes[:1000]) and np.array_equal(host.scales, scales[:1000])

    result = {"map": "C2 rays (%d), 0.2 m, 32^3 regions, GpuNdtMap" % args.rays, "regions": int(len(regions)),
              "device": ohm_amd.device_info(0)["name"], "occupied_voxels": n,
              "ellipsoids": dict(timed(ellipsoids, args.calls), bytes_to_host=(24 + 72 + 24 + 10 + 4) * n),
              "download_three_layers": dict(timed(download, args.calls), bytes_to_host=36 * volume * int(len(regions)))}
    result["download_over_ellipsoids"] = (result["download_three_layers"]["ms_host_clock"] /
                                          result["ellipsoids"]["ms_host_clock"])
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
