#!/usr/bin/env python3
"""Times ohmhip_map_compare on the C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3 regions, occupancy + mean) against
its clone(): occupancy layer, OHMHIP_CMP_CONTINUE, both capacities 0 -- a pure count -- against the floor of doing it on
the host, the two ohmhip_map_read_regions downloads of that layer (the numpy diff that would follow is not timed).  A
third leg compares the map with a clone in which about 1 % of the voxels were changed, with a mismatch list that holds
them all.  Needs a HIP device.

After warm-up, per round (two rounds, to see the spread) and alternated in the same process: `--calls` back-to-back
calls per leg, each series ended by a device synchronise.  Prints one JSON line; nothing is asserted beyond the counts.

The byte model: both layers are read once, so k_compare_count moves 2 x layer_bytes.  With --kernel-ms MS (milliseconds
per k_compare_count call, from a run of its own under `rocprofv3 --kernel-trace --stats -- python
scripts/compare_probe.py --calls 5 --rounds 1`) the line also carries the kernel's bytes per second."""
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
    from ohm_amd import compare as M
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "compare_probe needs a HIP device"
    ref = ohm_amd.GpuMap(ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean")), gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    assert ref.integrateRays(rays) == rays.shape[0]
    ref.wait()
    same = ref.clone()
    keys = np.ascontiguousarray(ref.regionKeys(), dtype=np.int16).reshape(-1, 3)
    n_regions = keys.shape[0]
    voxels = ref.map().regionVoxelVolume()
    layer_bytes = n_regions * voxels * 4

    blocks = [np.empty((n_regions, voxels), dtype=np.float32) for _ in range(2)]
    ptrs = [(C.c_void_p * n_regions)(*[b[i].ctypes.data for i in range(n_regions)]) for b in blocks]

    def download(gm, which):
        L.check(L.lib.ohmhip_map_read_regions(gm._handle, L.LID_OCCUPANCY, keys.ctypes.data, n_regions, ptrs[which]), "read")

    # the third leg's map: every 100th voxel of every region moved
    download(ref, 0)
    planted = blocks[0].copy()
    planted[:, ::100] = np.where(np.isfinite(planted[:, ::100]), planted[:, ::100] + np.float32(0.5), np.float32(0.5))
    changed = ref.clone()
    planted_ptrs = (C.c_void_p * n_regions)(*[planted[i].ctypes.data for i in range(n_regions)])
    L.check(L.lib.ohmhip_map_write_regions(changed._handle, L.LID_OCCUPANCY, keys.ctypes.data, n_regions, planted_ptrs),
            "write")
    n_planted = int(planted[:, ::100].size)

    params, _ = M.compare_params("occupancy", None, M.kContinue)
    res = L.CompareResult()
    listed = np.zeros(n_planted, dtype=ohm_amd.GPU_KEY_DTYPE)

    def count_only():
        L.check(L.lib.ohmhip_map_compare(same._handle, ref._handle, C.byref(params), 0, None, 0, None, C.byref(res)), "compare")

    def with_list():
        L.check(L.lib.ohmhip_map_compare(changed._handle, ref._handle, C.byref(params), n_planted, listed.ctypes.data, 0,
                                         None, C.byref(res)), "compare")

    def host_floor():
        download(same, 0)
        download(ref, 1)

    def timed(fn, calls):
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        L.check(L.lib.ohmhip_device_synchronize(), "synchronize")
        return (time.perf_counter() - t0) * 1e3 / calls

    for _ in range(2):
        count_only()
        with_list()
        host_floor()
    count_only()
    assert res.voxels_failed == 0 and res.voxels_passed == n_regions * voxels and res.regions_compared == n_regions
    with_list()
    assert res.mismatch_count == n_planted == res.voxels_failed

    rounds = []
    for _ in range(args.rounds):
        rounds.append({"ms_compare_count": timed(count_only, args.calls), "ms_compare_list": timed(with_list, args.calls),
                       "ms_host_downloads": timed(host_floor, args.calls)})
    best = min(r["ms_compare_count"] for r in rounds)
    result = {"map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy layer" % args.rays, "regions": n_regions,
              "layer_bytes": layer_bytes, "model_kernel_bytes": 2 * layer_bytes, "planted": n_planted, "rounds": rounds,
              "host_downloads_over_compare": min(r["ms_host_downloads"] for r in rounds) / best,
              "compare_call_bytes_per_s": 2 * layer_bytes / (best * 1e-3), "device": ohm_amd.device_info(0)["name"]}
    if args.kernel_ms:
        result["kernel_bytes_per_s"] = 2 * layer_bytes / (args.kernel_ms * 1e-3)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
