#!/usr/bin/env python3
"""Times ClearingPattern.apply / apply_many (ohmhip_map_apply_pattern: the pattern resident on the device, a pose per
application over the link) against the route a caller had before it, on the same commit and the same map: the rays built
on the host (numpy, the model's operation order), GpuMap.setMissValue(scaled), the host-pointer integrateRays of all the
poses' rays as one batch, setMissValue back.

The map is the C1 map of bench.py (10^6 lidar rays, 0.1 m, 32^3 regions, occupancy).  Two patterns -- the 5 degree cone of
the reference's test (439 rays) and a 1 degree cone -- at 1 and 64 poses per call.  After warm-up, per round and
alternated in one process: `--calls` back-to-back calls of each leg, each leg ended by a device synchronise.  Both legs
lower the same voxels, so the map they meet drifts the same way.  Prints one JSON line; nothing is asserted.

Per-kernel times come from a run of its own under `rocprofv3 --kernel-trace --stats -- python scripts/pattern_probe.py
--calls 2 --rounds 1`; the end-to-end figures from the run without the profiler."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_rays(points, poses):
    """The poses applied to the pattern on the host, pose major: numpy, one rounding per operation in the order of
    include/ohmhip.h (RAY PATTERNS)."""
    def cross(a, b):
        return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                         a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], axis=-1)
    s = np.broadcast_to(points[None, :, :], (poses.shape[0],) + points.shape)
    u = poses[:, None, 3:6]
    w = poses[:, None, 6:7]
    uv = cross(u, s)
    uuv = cross(u, uv)
    return ((s + ((uv * w) + uuv) * 2.0) + poses[:, None, 0:3]).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--scaling", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import ohm_amd
    from ohm_amd import _lib as L
    from ohm_amd import synth

    assert ohm_amd.device_count() > 0, "pattern_probe needs a HIP device"
    map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32))
    gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
    rays = synth.rays_c1(n=args.rays)
    assert gm.integrateRays(rays) == rays.shape[0]
    gm.wait()
    miss = map_.missValue()
    scaled = float(np.float32(np.float32(miss) * np.float32(args.scaling)))
    rng = np.random.default_rng(11)

    def make_poses(count):
        poses = np.empty((count, 7))
        poses[:, :3] = 0.05 + rng.uniform(-1.0, 1.0, size=(count, 3)) * (2.0, 2.0, 0.2)
        q = rng.normal(size=(count, 4))
        poses[:, 3:] = q / np.linalg.norm(q, axis=1)[:, None]
        return poses

    def timed(fn, n):
        gm.wait()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        gm.wait()   # launches what the host route left in the coalescing buffer, then waits for the device
        return (time.perf_counter() - t0) * 1e3 / n

    results = []
    for label, resolution_deg in (("cone 5 deg", 5.0), ("cone 1 deg", 1.0)):
        cone = ohm_amd.RayPatternConical((0.7, 0.7, 0.0), math.radians(65.0), 25.0, math.radians(resolution_deg))
        clearing = ohm_amd.ClearingPattern(cone)
        points = cone.rayPoints()
        flags = clearing.rayFlags()
        for pose_count in (1, 64):
            poses = make_poses(pose_count)

            def device_route():
                clearing.apply_many(gm, poses, probability_scaling=args.scaling)

            def host_route():
                built = host_rays(points, poses)
                gm.setMissValue(scaled)
                gm.integrateRays(built, ray_update_flags=flags)
                gm.setMissValue(miss)

            def host_build_only():
                host_rays(points, poses)

            for _ in range(2):
                device_route()
                host_route()
            gm.wait()
            assert np.array_equal(clearing.lastRaySet(), host_rays(points, poses))  # the two routes integrate the same rays
            rounds = []
            for _ in range(args.rounds):
                rounds.append({"ms_apply": timed(device_route, args.calls), "ms_host_route": timed(host_route, args.calls),
                               "ms_host_build": timed(host_build_only, args.calls)})
            best_apply = min(r["ms_apply"] for r in rounds)
            best_host = min(r["ms_host_route"] for r in rounds)
            results.append({"pattern": label, "rays": cone.rayCount(), "poses": pose_count,
                            "rays_per_call": cone.rayCount() * pose_count, "pose_bytes": 56 * pose_count,
                            "ray_bytes": 48 * cone.rayCount() * pose_count, "rounds": rounds, "ms_apply": best_apply,
                            "ms_host_route": best_host, "host_over_apply": best_host / best_apply})
        cone.close()
    result = {"map": "C1 rays (%d), 0.1 m, 32^3 regions, occupancy" % args.rays, "probability_scaling": args.scaling,
              "calls": args.calls, "cases": results, "build_id": L.lib.ohmhip_build_id().decode(),
              "device": ohm_amd.device_info(0)["name"]}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
