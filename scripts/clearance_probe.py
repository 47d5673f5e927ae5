"""Development probe: clearance throughput (ohmhip_map_clearance_regions_device) on the C1 map.

Builds the C1 map (synth.rays_c1, 10^6 rays, 0.1 m, 32^3 regions), then computes the clearance of ALL its regions per
call at search radius 0.2, 0.5, 1.0 and 3.2 m, without and with kQfUnknownAsOccupied.  The half extent is the
reference's h = ceil(float radius / resolution): 0.2 m and 3.2 m give h = 3 and 33 (float(0.2) and float(3.2) lie above
them), so 0.15 m and 3.15 m are added for h = 2 and 32, the largest window the LDS path stages.  Per
configuration: the time per call over back-to-back calls after warm-up (queued on the map's stream, one wait at the end,
so the figure is the device's), regions/s and voxels/s.  A sample of regions (of voxels at h = 32) is checked with ==
against the CPU restatement (tests/clearance_ref.py).  `--quick`: 1 timed call per configuration (for a run under
rocprofv3 --kernel-trace --stats); `--json <file>`: write the results there."""
import json
import os
import sys
import time

import ctypes as C

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ohm_amd  # noqa: E402
from ohm_amd import _lib as L  # noqa: E402
from ohm_amd import synth  # noqa: E402
from clearance_ref import Geometry, clearance_keys, clearance_regions, half_extent  # noqa: E402
from rays_query_ref import ChunkBlocks  # noqa: E402

quick = "--quick" in sys.argv
map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32))
gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
build = synth.rays_c1(n=1_000_000)
for part in np.split(build, 4):
    assert gm.integrateRays(part) == part.shape[0]
gm.syncVoxels()
keys = np.ascontiguousarray(gm.regionKeys())
n = keys.shape[0]
voxels = n * 32 ** 3
geom = Geometry(0.1, (32, 32, 32), map_.occupancy_threshold_value)
blocks = ChunkBlocks(map_.chunks)

h_out = L._vp()
L.check(L.lib.ohmhip_buffer_create(C.byref(h_out), 4 * voxels, 3), "buffer_create")
d_out = L._vp()
L.check(L.lib.ohmhip_buffer_ptr(h_out, C.byref(d_out)), "buffer_ptr")


def read_region(i):
    out = np.zeros(32 ** 3, dtype=np.float32)
    L.check(L.lib.ohmhip_buffer_read(h_out, out.ctypes.data, out.nbytes, 4 * 32 ** 3 * i, None, None, None), "read")
    return out.reshape(32, 32, 32)


results = {"regions": int(n), "voxels": int(voxels), "configs": []}
print("C1 map: %d regions, %d voxels" % (n, voxels))
rng = np.random.default_rng(0)
for radius in (0.15, 0.2, 0.5, 1.0, 3.15, 3.2):
    h = half_extent(radius, 0.1)
    for flags in (0, 1):
        steps = 1 if quick else (3 if h >= 10 else 10)
        gm.clearanceRegionsDevice(keys, d_out, radius, flags)  # warm-up (and the values checked below)
        t0 = time.perf_counter()
        for _ in range(steps):
            gm.clearanceRegionsDevice(keys, d_out, radius, flags, sync=False)
        gm.wait()
        ms = (time.perf_counter() - t0) * 1e3 / steps
        # the check: whole regions at small h, a voxel sample at large h
        pick = rng.choice(n, size=2 if h <= 5 else 1, replace=False)
        checked = 0
        for i in pick:
            got = read_region(int(i))
            if h <= 10:
                want = clearance_regions(geom, blocks, keys[i:i + 1], radius, flags)[0]
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (radius, flags, keys[i])
                checked += want.size
            else:
                loc = rng.integers(0, 32, size=(40, 3))
                want = clearance_keys(geom, blocks, np.repeat(keys[i:i + 1], 40, axis=0), loc, radius, flags)
                assert np.array_equal(got[loc[:, 2], loc[:, 1], loc[:, 0]].view(np.uint32), want.view(np.uint32))
                checked += want.size
        row = {"radius": radius, "h": h, "unknown_as_occupied": bool(flags), "ms_per_call": round(ms, 3),
               "regions_per_s": round(n / ms * 1e3, 1), "voxels_per_s": round(voxels / ms * 1e3, 1),
               "steps": steps, "voxels_checked": int(checked)}
        results["configs"].append(row)
        print("r=%.1f h=%2d uao=%d: %9.3f ms/call  %10.0f regions/s  %.3e voxels/s  (%d voxels == reference)" %
              (radius, h, flags, ms, row["regions_per_s"], row["voxels_per_s"], checked))
L.lib.ohmhip_buffer_destroy(h_out)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
        json.dump(results, fh, indent=1)
