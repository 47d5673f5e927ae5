"""Development probe: the clearance layer update (ohmhip_map_clearance_update) on the C1 map.

Builds the C1 map (synth.rays_c1, 10^6 rays, 0.1 m, 32^3 regions) with the clearance layer, then per half extent h = 5
and 12:
  query   one ohmhip_map_clearance_regions_device call over all regions (the yardstick),
  full    update(0) with every region stale (alternating two radii of the same h, so each call recomputes all),
  local   update(0) after one 4096-ray batch of the same sensor (rays_c1 further along its scan),
  idle    update(0) with nothing stale (no clearance kernel may launch: check under rocprofv3 --kernel-trace).
Wall time per call, after a warm-up, with the host-side selection included.  After every update the layer of a sample of
regions is checked with == against the query.  `--quick`: 1 timed call each (for a run under rocprofv3 --kernel-trace
--stats); `--json <file>`: write the results there."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ohm_amd  # noqa: E402
from ohm_amd import _lib as L  # noqa: E402
from ohm_amd import synth  # noqa: E402

quick = "--quick" in sys.argv
map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32))
ohm_amd.ClearanceProcess.ensureClearanceLayer(map_)
gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
build = synth.rays_c1(n=1_000_000)
for part in np.split(build, 4):
    assert gm.integrateRays(part) == part.shape[0]
gm.wait()
keys = np.ascontiguousarray(gm.regionKeys())
n = keys.shape[0]
h_out = L._vp()
L.check(L.lib.ohmhip_buffer_create(C.byref(h_out), 4 * n * 32 ** 3, 3), "buffer_create")
d_out = L._vp()
L.check(L.lib.ohmhip_buffer_ptr(h_out, C.byref(d_out)), "buffer_ptr")


def read_layer(sample):
    sample = np.ascontiguousarray(sample, dtype=np.int16)
    out = np.zeros((sample.shape[0], 32 ** 3), dtype=np.float32)
    dsts = (C.c_void_p * sample.shape[0])(*[out[i].ctypes.data for i in range(sample.shape[0])])
    L.check(L.lib.ohmhip_map_read_regions(gm._handle, L.LID_CLEARANCE, sample.ctypes.data, sample.shape[0], dsts), "read")
    return out.reshape(-1, 32, 32, 32)


def check(radius):
    sample = keys[:: max(1, n // 8)]
    assert np.array_equal(read_layer(sample).view(np.uint32), gm.clearanceRegions(sample, radius).view(np.uint32))


def timed(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / steps, out


results = {"regions": int(n), "configs": []}
print("C1 map: %d regions" % n)
batch = 0
for radius, other in ((0.45, 0.46), (1.15, 1.16)):
    h = int(np.ceil(float(np.float32(radius)) / 0.1))
    steps = 1 if quick else 5
    gm.clearanceRegionsDevice(keys, d_out, radius)
    ms_query, _ = timed(lambda: gm.clearanceRegionsDevice(keys, d_out, radius), steps)
    gm.clearanceUpdate(radius)  # warm-up (the timed calls alternate, starting with `other`)
    radii = [radius, other] * steps
    ms_full, out = timed(lambda: gm.clearanceUpdate(radii.pop()), steps)
    assert out == (n, 0)
    gm.clearanceUpdate(radius)
    check(radius)
    local = []
    for _ in range(steps):
        batch += 1
        part = synth.rays_c1(n=4096, first=1_000_000 + 4096 * batch)
        assert gm.integrateRays(part) == part.shape[0]
        gm.wait()
        stale = gm.clearanceStaleRegions(radius).shape[0]
        ms, out = timed(lambda: gm.clearanceUpdate(radius), 1)
        local.append((ms, out[0], stale))
    check(radius)
    ms_idle, out = timed(lambda: gm.clearanceUpdate(radius), steps)
    assert out == (0, 0)
    row = {"radius": radius, "h": h, "query_ms": round(ms_query, 3), "update_full_ms": round(ms_full, 3),
           "update_local_ms": round(float(np.median([x[0] for x in local])), 3),
           "local_regions": [int(x[1]) for x in local], "update_idle_ms": round(ms_idle, 3)}
    results["configs"].append(row)
    print("h=%2d: query %.3f ms, update(all %d) %.3f ms, after a 4096-ray batch %.3f ms (%s regions), idle %.3f ms" %
          (h, ms_query, n, ms_full, row["update_local_ms"], row["local_regions"], ms_idle))
L.lib.ohmhip_buffer_destroy(h_out)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
        json.dump(results, fh, indent=1)
