#!/usr/bin/env python3
"""Timing probe of the device ray-filter chain (profiles/r17_notes.md).  Needs a GPU.

    python scripts/rayfilter_probe.py --parent-tree <checkout of the parent commit, built> [--out results.json]

(The parent's library alone is not enough: ohm_amd/_lib.py binds every symbol the header declares when it is imported,
and the parent's library lacks the chain's entry points.  The parent's children therefore import the parent's own
ohm_amd from its tree, with the library found there or the one OHMHIP_LIB names.)

Workload: synth.rays_c1(n=10**6) at 0.1 m; the box (-15, -15, -15)-(15, 15, 15) around the sensor cuts roughly half the
rays (clipBounded moves their ends to the box).  Every leg: a fresh map, WARMUP batches, then BATCHES timed batches, each
timed from the call to the end of ohmhip_map_sync; median and spread (min, max, quartiles) in ms.

  a   no chain, device-pointer batch -- the measured path -- in child processes that alternate the parent's tree and
      this one, ROUNDS times.  The gate: this build's median of round medians is no higher than
      the highest round median of the parent in the same run (the parent's own run-to-run spread).
  b   the host callable route: setRayFilter(RF.clip_bounded(box)), integrateRays(host pointers)
  c   the device chain with host-pointer batches
  d   the device chain with device-pointer batches
and the ratio b : c.  One leg per child process, one process on the GPU at a time; each child under its own timeout.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, BATCHES, ROUNDS = 3, 24, 4
BOX = ((-15.0, -15.0, -15.0), (15.0, 15.0, 15.0))


def summary(ms):
    import numpy as np
    ms = np.sort(np.asarray(ms, dtype=np.float64))
    return {"median": float(np.median(ms)), "min": float(ms[0]), "max": float(ms[-1]),
            "q1": float(np.percentile(ms, 25)), "q3": float(np.percentile(ms, 75)), "n": int(ms.size)}


def run_leg(leg, n_rays, root):
    """In a child: one leg, one JSON line.  `root`: the tree ohm_amd is imported from."""
    import time

    import numpy as np
    sys.path.insert(0, root)
    import ohm_amd
    from ohm_amd import GpuMap, OccupancyMap, synth
    from ohm_amd import _lib as L
    from ohm_amd import rayfilter as RF

    rays = synth.rays_c1(n=n_rays)
    map_ = OccupancyMap(0.1, (32, 32, 32))
    gm = GpuMap(map_, expected_element_count=rays.shape[0])
    box = RF.Aabb(*BOX)
    kept = None
    if leg == "b":
        gm.setRayFilter(RF.clip_bounded(box))
    elif leg in ("c", "d"):
        gm.setRayFilter(RF.on_device(RF.clip_bounded_stage(box)))
        keep, _, flags = gm.applyRayFilter(rays)
        kept = {"kept": int(keep.sum()), "clipped_end": int(((flags & 4) != 0).sum())}
    buf = ptr = None
    if leg in ("a", "d"):
        buf, ptr = L._vp(), L._vp()
        L.check(L.lib.ohmhip_buffer_create(C.byref(buf), rays.nbytes, 3))
        L.check(L.lib.ohmhip_buffer_write(buf, rays.ctypes.data, rays.nbytes, 0, None, None, None))
        L.check(L.lib.ohmhip_buffer_ptr(buf, C.byref(ptr)))
    times = []
    for batch in range(WARMUP + BATCHES):
        t0 = time.perf_counter()
        if ptr is not None:
            done = gm.integrateRaysDevice(ptr, rays.shape[0])
        else:
            done = gm.integrateRays(rays)
        gm.wait()
        t1 = time.perf_counter()
        assert done > 0
        if batch >= WARMUP:
            times.append(1e3 * (t1 - t0))
    if buf is not None:
        L.lib.ohmhip_buffer_destroy(buf)
    out = {"leg": leg, "lib": os.path.basename(L.LIB_PATH), "build": L.lib.ohmhip_build_id().decode(), "rays": n_rays,
           "points_integrated": int(done), "ms": summary(times), "device": ohm_amd.device_info(0)["name"]}
    if kept:
        out.update(kept)
    gm.close()
    print(json.dumps(out))


def child(leg, n_rays, root=ROOT, timeout=240):
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--rays", str(n_rays), "--root",
                          os.path.abspath(root)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=timeout)
    if res.returncode != 0:
        # nothing more is started on the GPU after a child that failed
        sys.exit("leg %s (%s) failed with status %d:\n%s" % (leg, root, res.returncode, res.stderr[-3000:]))
    return json.loads(res.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--leg", choices=["a", "b", "c", "d"], help="(child) run one leg in this process")
    ap.add_argument("--rays", type=int, default=10 ** 6)
    ap.add_argument("--root", default=ROOT, help="(child) the tree to import ohm_amd from")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit")
    ap.add_argument("--out", help="also write the results as JSON")
    args = ap.parse_args()
    if args.leg:
        run_leg(args.leg, args.rays, args.root)
        return 0
    import numpy as np
    results = {"a_parent": [], "a_branch": []}
    if args.parent_tree:
        for _ in range(ROUNDS):
            results["a_parent"].append(child("a", args.rays, args.parent_tree))
            results["a_branch"].append(child("a", args.rays))
    else:
        results["a_branch"].append(child("a", args.rays))
    for leg in ("b", "c", "d"):
        results[leg] = child(leg, args.rays)
    branch = [r["ms"]["median"] for r in results["a_branch"]]
    parent = [r["ms"]["median"] for r in results["a_parent"]]
    verdict = {"a_branch_median_of_rounds": float(np.median(branch)), "a_branch_rounds": branch, "a_parent_rounds": parent,
               "b_to_c": results["b"]["ms"]["median"] / results["c"]["ms"]["median"]}
    if parent:
        verdict["a_parent_median_of_rounds"] = float(np.median(parent))
        verdict["a_gate_holds"] = bool(np.median(branch) <= max(parent))
    results["verdict"] = verdict
    text = json.dumps(results, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if verdict.get("a_gate_holds", True) else 1


if __name__ == "__main__":
    sys.exit(main())
