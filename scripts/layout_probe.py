#!/usr/bin/env python3
"""Times a layer change on the C1 map of bench.py (lidar rays in 5 batches, 0.1 m, 32^3 regions, occupancy only):
GpuMap.addLayer("mean") and GpuMap.removeLayer("mean") (ohmhip_map_update_layers) against the only route a caller had
before them for the same result -- syncVoxels, a new GpuMap with the wanted layers over the same host map, upload of every
block.  Needs a HIP device.  Host clock around blocking calls, each fenced by wait(); --rounds rounds of add and remove on
the same map, one of the old route per direction.  After the timed calls the occupancy of the map that took the new route
is compared once with the one the old route built.  Prints one JSON line; nothing else is asserted."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ohm_amd
    from ohm_amd import GpuMap, OccupancyMap, compareVoxels, synth

    def timed(fn, gm):
        gm.wait()
        t0 = time.perf_counter()
        fn()
        gm.wait()
        return (time.perf_counter() - t0) * 1e3

    map_ = OccupancyMap(0.1, (32, 32, 32), layers=("occupancy",))
    gm = GpuMap(map_)
    rays = synth.rays_c1(n=args.rays)
    step = rays.shape[0] // 5 // 2 * 2
    for at in range(0, rays.shape[0], step):
        gm.integrateRays(rays[at:at + step])
    gm.wait()
    result = {"regions": int(len(gm.regionKeys())), "rays": args.rays, "device": ohm_amd.device_info(0)["name"],
              "build": ohm_amd._lib.lib.ohmhip_build_id().decode(), "add_ms": [], "remove_ms": []}
    for _ in range(args.rounds):
        result["add_ms"].append(timed(lambda: gm.addLayer("mean"), gm))
        result["remove_ms"].append(timed(lambda: gm.removeLayer("mean"), gm))
    result["add_stats"] = None
    result["add_ms"].append(timed(lambda: gm.addLayer("mean"), gm))
    result["add_stats"] = gm.lastLayerChangeStats()

    # the old route, to a map with the mean layer ...
    def rebuild(layers):
        holder = {}

        def run():
            gm.syncVoxels()
            host = OccupancyMap(0.1, (32, 32, 32), layers=layers)
            host.chunks = {key: {name: block for name, block in chunk.items() if name in layers}
                           for key, chunk in map_.chunks.items()}
            holder["gm"] = GpuMap(host)  # (uploads every block the host map holds)
            holder["gm"].wait()
        return run, holder

    run, with_mean = rebuild(("occupancy", "mean"))
    result["old_route_add_ms"] = timed(run, gm)
    result["old_route_add_ms_synced"] = timed(run, gm)  # (nothing left to download: the upload and the new map alone)
    result["occupancy_equal"] = bool(compareVoxels(gm, with_mean["gm"], "occupancy"))
    # ... and back to one without it
    run, without = rebuild(("occupancy",))
    result["old_route_remove_ms_synced"] = timed(run, gm)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
