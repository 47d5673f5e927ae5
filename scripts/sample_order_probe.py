"""What the per-region ordering of a batch's sample keys (k_sort_region_hits) costs at controlled bucket loads.

    python scripts/sample_order_probe.py --out loads.json                      # run the loads (under the profiler:)
    rocprofv3 --kernel-trace --stats -d DIR -o probe --output-format csv -- python scripts/sample_order_probe.py --out loads.json
    python scripts/sample_order_probe.py --summarise DIR loads.json            # per load: us per call in the ordering kernels

Every load is a plain occupancy batch of short rays (a few voxels) that start and end inside ONE 32^3 region at 0.1 m
(or a few regions: --regions), integrated through GpuMap with coalescing off: 2 calls to settle, --calls timed ones, in
a map of its own.  A bucket of the ranked ordering is an x-row of the region (voxel >> 5); sum(c^2)/n over the bucket
loads c is what the kernel compares with its limit, printed per load with the route GpuMap.orderCounts() saw.  Loads:
  uniform        end points uniform in the region
  rows k         all samples in k x-rows, n / k in each: sum(c^2)/n = n / k
  plane          a z = const plane (32 x-rows)
  voxel m        m samples per sampled voxel, voxels uniform
  wall           synth.rays_c2 (a 40 m box room), --wall-rays rays, plain occupancy at 0.1 m: many regions
The library under test is the one OHMHIP_LIB names (ohm_amd/_lib.py): build it with -DOHMHIP_ORDER_RANK_LIMIT=0 for the
network alone and with a limit no load reaches for the ranked path alone; where the two cost the same is the limit to
set.  --summarise cuts the kernel trace into calls at the k_ray_setup launches (one per call for these loads; the count
is checked against loads.json) and adds up the k_sort_region_hits launches of every timed call, per instantiation."""
import argparse
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EDGE, RES, SETTLE = 3.2, 0.1, 2


def region_rays(np, rng, voxels, region):
    """Rays of up to 2.5 voxels per axis to a point in each of `voxels` (x + 32 * (y + 32 * z)) of region (region, 0, 0)."""
    low = np.array([-1.6 + region * EDGE, -1.6, -1.6])
    cell = np.column_stack([voxels & 31, (voxels >> 5) & 31, voxels >> 10]).astype(np.float64)
    ends = low + (cell + rng.uniform(0.15, 0.85, size=cell.shape)) * RES
    starts = np.clip(ends + rng.uniform(-0.25, 0.25, size=ends.shape), low + 0.02, low + EDGE - 0.02)
    rays = np.empty((2 * ends.shape[0], 3))
    rays[0::2], rays[1::2] = starts, ends
    return rays


def load_voxels(np, rng, kind, arg, n):
    if kind == "uniform":
        return rng.integers(0, 32768, size=n)
    if kind == "rows":
        rows = rng.choice(1024, size=arg, replace=False)
        return rng.permutation(np.repeat(rows, -(-n // arg))[:n]) * 32 + rng.integers(0, 32, size=n)
    if kind == "plane":
        return 16 * 1024 + rng.integers(0, 1024, size=n)
    if kind == "voxel":
        return rng.permutation(np.repeat(rng.choice(32768, size=-(-n // arg), replace=False), arg)[:n])
    raise SystemExit("unknown load " + kind)


def run(args):
    sys.path.insert(0, args.tree or ROOT)
    import numpy as np
    from ohm_amd import GpuMap, OccupancyMap, synth

    def order_counts(gm):  # (a parent build has none)
        return gm.orderCounts() if hasattr(gm, "orderCounts") else (0, 0)

    loads = []
    for n in args.samples:
        loads.append(("uniform", 0, n))
        k = 1024
        while k >= 1:
            if n // k >= 2:
                loads.append(("rows", k, n))
            k //= 2
        loads.append(("plane", 0, n))
        loads += [("voxel", m, n) for m in (2, 8, 32)]
    loads.append(("wall", 0, args.wall_rays))
    if args.loads:
        loads = [load for load in loads if load[0] in args.loads]
    manifest = []
    for kind, arg, n in loads:
        rng = np.random.default_rng(1000 + arg)
        if kind == "wall":
            rays = synth.rays_c2(n=n)
            region = np.floor((rays[1::2] + 1.6) / EDGE).astype(np.int64)
            voxel = np.floor((rays[1::2] + 1.6) / RES).astype(np.int64) & 31
            keys = ((region[:, 0] * 4096 + region[:, 1]) * 4096 + region[:, 2]) * 1024 + voxel[:, 1] + 32 * voxel[:, 2]
            _, first, per_bucket = np.unique(keys, return_index=True, return_counts=True)
            group = np.unique(keys[first] >> 10, return_inverse=True)[1]
            spread = np.bincount(group, per_bucket.astype(np.float64) ** 2) / np.bincount(group, per_bucket)
        else:
            voxels = [load_voxels(np, rng, kind, arg, n) for _ in range(args.regions)]
            rays = np.vstack([region_rays(np, rng, v, r) for r, v in enumerate(voxels)])
            spread = [float(np.sum(np.bincount(v >> 5).astype(np.float64) ** 2) / n) for v in voxels]
        map_ = OccupancyMap(RES, (32, 32, 32), layers=("occupancy",))
        gm = GpuMap(map_, region_capacity=max(64, 2 * args.regions) if kind != "wall" else 4096)
        gm.setBatchCoalescing(0)
        for _ in range(SETTLE):
            gm.integrateRays(rays)
        before = order_counts(gm)
        for _ in range(args.calls):
            gm.integrateRays(rays)
        after = order_counts(gm)
        gm.close()
        row = dict(load=kind, arg=arg, samples=n, regions=args.regions if kind != "wall" else int(len(spread)),
                   sum_c2_over_n=[round(float(np.min(spread)), 1), round(float(np.max(spread)), 1)],
                   calls=SETTLE + args.calls, ranked=after[0] - before[0], network=after[1] - before[1])
        manifest.append(row)
        print(json.dumps(row))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(manifest, fh, indent=1)


def summarise(trace, manifest_path):
    found = sorted(glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True)) if os.path.isdir(trace) \
        else [trace]
    if not found:
        raise SystemExit("no *kernel_trace.csv under " + trace)
    rows = []
    with open(found[0]) as fh:
        for r in csv.DictReader(fh):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    with open(manifest_path) as fh:
        manifest = json.load(fh)
    calls = []  # per call: {instantiation: ns}
    for start, end, name in rows:
        if "k_ray_setup" in name:
            calls.append({})
        m = re.search(r"k_sort_region_hits(?:<|ILj)(\d+)", name)
        if m and calls:
            calls[-1][m.group(1)] = calls[-1].get(m.group(1), 0) + end - start
    if len(calls) != sum(row["calls"] for row in manifest):
        raise SystemExit("%d k_ray_setup launches in the trace, %d calls in %s: a call was repeated, the cut is off" %
                         (len(calls), sum(row["calls"] for row in manifest), manifest_path))
    print("%-8s %5s %8s %7s  %-14s %7s %7s   us per call in k_sort_region_hits <2048,256> / <8192,1024>" %
          ("load", "arg", "samples", "regions", "sum(c^2)/n", "ranked", "network"))
    at = 0
    for row in manifest:
        timed = calls[at + SETTLE:at + row["calls"]]
        at += row["calls"]
        small = sum(c.get("2048", 0) for c in timed) / len(timed) / 1e3
        dense = sum(c.get("8192", 0) for c in timed) / len(timed) / 1e3
        print("%-8s %5d %8d %7d  %6.1f..%-6.1f %7d %7d   %8.1f %8.1f" %
              (row["load"], row["arg"], row["samples"], row["regions"], row["sum_c2_over_n"][0], row["sum_c2_over_n"][1],
               row["ranked"], row["network"], small, dense))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, nargs="+", default=[2048, 8192], help="samples per region of the loads")
    ap.add_argument("--regions", type=int, default=1, help="regions (r, 0, 0) that get the same kind of load")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--wall-rays", type=int, default=150_000,
                    help="(more than 8192 samples in one region and the whole batch takes the device-wide sort)")
    ap.add_argument("--loads", nargs="+", default=None, help="only these kinds of load (uniform rows plane voxel wall)")
    ap.add_argument("--tree", default=None, help="import ohm_amd from this checkout (a build of the parent, for A/B)")
    ap.add_argument("--out", default=None, help="write the loads and the routes they took as JSON")
    ap.add_argument("--summarise", nargs=2, metavar=("TRACE", "LOADS.json"))
    args = ap.parse_args()
    if args.summarise:
        summarise(*args.summarise)
    else:
        run(args)


if __name__ == "__main__":
    main()
