#!/usr/bin/env python3
"""Times the point filter on the C1 map of bench.py carrying the NDT layers (10^6 lidar rays, 0.1 m, 32^3 regions,
occupancy + mean + covariance, integrated by GpuNdtMap) beside what a caller without it does.  Needs a HIP device.

  host arrays    ohmhip_map_filter_points, 10^6 points, every output array, tolerance 0.5
  device arrays  ohmhip_map_filter_points_device on the same points resident on the device, fenced by ohmhip_map_sync
  yardstick      ohmhip_map_voxel_keys, three ohmhip_map_read_voxels calls (occupancy, mean, covariance), then the numpy
                 restatement of the rule (tests/point_filter_ref.py) and nonzero() for the kept indices

The points are the rays' sample ends displaced by N(0, 0.03 m).  Every series is warmed, starts and ends with a device
synchronise and is timed by device events recorded around it and by the host clock.  The three ways must give the same
status for every point.  Bytes over PCIe are computed from the array sizes, not measured.  Prints one JSON line; no
speed is asserted."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--tolerance", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_filter_probe.json"))
    args = ap.parse_args()

    import ohm_amd
    import point_filter_ref as PF
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "point_filter_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32), layers=("occupancy", "mean", "covariance"))
    gm = ohm_amd.GpuNdtMap(map_, gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    handle = gm._handle
    rng = np.random.default_rng(1)
    samples = rays[1::2]
    points = samples[rng.integers(0, len(samples), size=args.points)] + rng.normal(0.0, 0.03, size=(args.points, 3))
    points = np.ascontiguousarray(points)
    n = len(points)

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

    params = L.PointFilterParams(args.tolerance, 0)
    status = np.zeros(n, dtype=np.uint8)
    indices = np.zeros(n, dtype=np.uint64)
    values = np.zeros(n, dtype=np.float64)
    keys = np.zeros(n, dtype=ohm_amd.GPU_KEY_DTYPE)
    kept = C.c_uint64(0)

    def host_call():
        L.check(L.lib.ohmhip_map_filter_points(handle, points.ctypes.data, n, C.byref(params), n, status.ctypes.data,
                                               indices.ctypes.data, values.ctypes.data, keys.ctypes.data, C.byref(kept)),
                "filter_points")

    buffers, ptrs = [], []
    for nbytes in (points.nbytes, n, 8 * n, 8 * n, 10 * n, 8):
        b, p = L._vp(), L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(b), nbytes, 3), "buffer_create")
        L.check(L.lib.ohmhip_buffer_ptr(b, C.byref(p)), "buffer_ptr")
        buffers.append(b)
        ptrs.append(p.value)
    L.check(L.lib.ohmhip_buffer_write(buffers[0], points.ctypes.data, points.nbytes, 0, None, None, None), "write")

    def device_call():
        L.check(L.lib.ohmhip_map_filter_points_device(handle, ptrs[0], 3, n, C.byref(params), n, ptrs[1], ptrs[2], ptrs[3],
                                                      ptrs[4], ptrs[5]), "filter_points_device")
        L.check(L.lib.ohmhip_map_sync(handle), "sync")

    threshold = map_.occupancy_threshold_value

    def yardstick():
        k = gm.voxelKeys(points)
        occupancy, _ = gm.readVoxels(k, "occupancy")
        mean, _ = gm.readVoxels(k, "mean")
        covariance, _ = gm.readVoxels(k, "covariance")
        with np.errstate(invalid="ignore"):
            occupied = (occupancy != np.float32(np.inf)) & (occupancy >= np.float32(threshold))
        out = np.where(occupied, PF.KEPT, PF.DROPPED).astype(np.uint8)
        rows = np.nonzero(occupied)[0]
        centre = PF.mean_positions(k[rows], mean[rows, 0], map_.resolution, map_.region_voxel_dimensions, map_.origin)
        out[rows] = PF.decide(PF.covariance_value(covariance[rows], points[rows] - centre), args.tolerance)
        return out, np.nonzero(out == PF.KEPT)[0]

    for _ in range(3):
        host_call()
        device_call()
    device_status = np.zeros(n, dtype=np.uint8)
    device_kept = np.zeros(1, dtype=np.uint64)
    L.check(L.lib.ohmhip_buffer_read(buffers[1], device_status.ctypes.data, n, 0, None, None, None), "read")
    L.check(L.lib.ohmhip_buffer_read(buffers[5], device_kept.ctypes.data, 8, 0, None, None, None), "read")
    want_status, want_kept = yardstick()  # (also the warm-up of the alternative)
    n_kept = int(kept.value)
    assert np.array_equal(status, want_status) and np.array_equal(indices[:n_kept], want_kept), "the two ways disagree"
    assert np.array_equal(device_status, status) and int(device_kept[0]) == n_kept, "host and device variants disagree"

    result = {"map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy + mean + covariance (GpuNdtMap)" % args.rays,
              "regions": int(len(gm.regionKeys())), "device": ohm_amd.device_info(0)["name"], "points": n,
              "tolerance": args.tolerance, "kept": n_kept, "removed_by_covariance": int((status == 2).sum()),
              "not_occupied": int((status == 0).sum()),
              "host_arrays": dict(timed(host_call, args.calls), bytes_to_device=24 * n, bytes_to_host=19 * n + 8 * n_kept + 8),
              "device_arrays": dict(timed(device_call, args.calls), bytes_to_device=0, bytes_to_host=0),
              "yardstick_keys_3_reads_numpy": dict(timed(yardstick, args.host_calls), bytes_to_device=3 * 10 * n,
                                                   bytes_to_host=(4 + 8 + 24 + 3) * n),
              "not_measured": "kernel times (no profiler run); bytes are computed from array sizes"}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    for e in events:
        L.lib.ohmhip_event_destroy(e)
    for b in buffers:
        L.lib.ohmhip_buffer_destroy(b)


if __name__ == "__main__":
    main()
