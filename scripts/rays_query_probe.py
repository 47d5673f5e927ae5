"""Development probe: RaysQueryGpu throughput (ohmhip_map_rays_query_device) on the C1 map.

Builds the C1 map (synth.rays_c1, 10^6 rays, 0.1 m), then queries 10^6 device-resident rays per batch:
  hits    the C1 rays from the same origin, end points scaled by 1.2 -- most stop at an occupied voxel;
  misses  the same directions mirrored in z (upwards), 30 m -- long walks through free and unknown space.
Per set: the time per batch over back-to-back batches after warm-up (the batches are queued on the map's stream, one
wait at the end, so launch overhead is hidden and the figure is the device's), rays/s, voxel visits/s and the bytes the
batch reads.  Visits are counted on the CPU by the query helper (tests/rays_query_ref.py) over a sample of the rays,
whose device results must equal it.
`--quick`: 2 timed batches (for a run under rocprofv3 --kernel-trace --stats); `--json <file>`: write the results there."""
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
from parity import make_oracle  # noqa: E402
from rays_query_ref import ChunkBlocks, rays_query  # noqa: E402

quick = "--quick" in sys.argv
n_rays = 1_000_000
steps = 2 if quick else 20
warmup = 1 if quick else 3
sample = 2000

map_ = ohm_amd.OccupancyMap(0.1, (32, 32, 32))
gm = ohm_amd.GpuMap(map_, gpu_mem_size=8 << 30)
build = synth.rays_c1(n=n_rays)
for part in np.split(build, 4):
    assert gm.integrateRays(part) == part.shape[0]
gm.wait()

origin = build[0]
hits = build.copy()
hits[1::2] = origin + (build[1::2] - origin) * 1.2
d = (build[1::2] - origin)
d /= np.linalg.norm(d, axis=1)[:, None]
d[:, 2] = -d[:, 2]
misses = build.copy()
misses[1::2] = origin + d * 30.0

gm.syncVoxels()
om = make_oracle(map_)
blocks = ChunkBlocks(map_.chunks)
thr = map_.occupancy_threshold_value
results = {"n_rays": n_rays, "steps": steps, "sets": {}}


def device_buffer(nbytes):
    h = L._vp()
    L.check(L.lib.ohmhip_buffer_create(C.byref(h), nbytes, 3), "buffer_create")
    p = L._vp()
    L.check(L.lib.ohmhip_buffer_ptr(h, C.byref(p)), "buffer_ptr")
    return h, p


def read(h, dtype, count):
    out = np.zeros(count, dtype=dtype)
    L.check(L.lib.ohmhip_buffer_read(h, out.ctypes.data, out.nbytes, 0, None, None, None), "buffer_read")
    return out


bufs = [device_buffer(b) for b in (48 * n_rays, 8 * n_rays, 8 * n_rays, n_rays, 10 * n_rays)]
out_ptrs = [p for _, p in bufs[1:]]
for set_name, rays in (("hits", hits), ("misses", misses)):
    idx = np.linspace(0, n_rays - 1, sample).astype(np.int64)
    sub = rays.reshape(-1, 6)[idx].reshape(-1, 3)
    (want, visits) = rays_query(om, sub, thr, ray_filter=map_.ray_filter, blocks=blocks)
    visits_per_ray = visits / sample
    rays = np.ascontiguousarray(rays)
    L.check(L.lib.ohmhip_buffer_write(bufs[0][0], rays.ctypes.data, rays.nbytes, 0, None, None, None), "buffer_write")
    d_rays = bufs[0][1]
    gm.raysQueryDevice(d_rays, 2 * n_rays, *out_ptrs)
    g = [read(bufs[1][0], np.float64, n_rays), read(bufs[2][0], np.float64, n_rays), read(bufs[3][0], np.int8, n_rays),
         read(bufs[4][0], np.uint8, 10 * n_rays).reshape(n_rays, 10)]
    assert np.array_equal(g[0][idx], want[0]) and np.array_equal(g[1][idx], want[1]), set_name
    assert np.array_equal(g[2][idx], want[2]), set_name
    assert np.array_equal(g[3][idx, :6].copy().view(np.int16).reshape(-1, 3), want[3]), set_name
    for _ in range(warmup):
        gm.raysQueryDevice(d_rays, 2 * n_rays, *out_ptrs, sync=False)
    gm.wait()
    t0 = time.perf_counter()
    for _ in range(steps):
        gm.raysQueryDevice(d_rays, 2 * n_rays, *out_ptrs, sync=False)
    gm.wait()
    dt = (time.perf_counter() - t0) / steps
    visits_batch = visits_per_ray * n_rays
    # bytes read: 48 B of ray, 4 B occupancy word per visit, 8 B walked index (scan + carry pass) per ray;
    # written: 8 + 8 + 1 + 10 B results + 4 + 4 B walked / scanned per ray
    read_bytes = n_rays * (48 + 8) + visits_batch * 4
    write_bytes = n_rays * (8 + 8 + 1 + 10 + 4 + 4)
    r = {"ms_per_batch": dt * 1e3, "rays_per_s": n_rays / dt, "visits_per_ray": visits_per_ray,
         "visits_per_s": visits_batch / dt, "bytes_read_per_batch": read_bytes,
         "bytes_written_per_batch": write_bytes, "gb_per_s": (read_bytes + write_bytes) / dt / 1e9,
         "occupied_fraction": float((g[2] == 1).mean()), "unobserved_fraction": float((g[2] == -1).mean())}
    results["sets"][set_name] = r
    print("%-7s %8.3f ms/batch  %7.1f Mrays/s  %6.1f visits/ray  %7.2f Gvisits/s  %6.1f GB/s" %
          (set_name, r["ms_per_batch"], r["rays_per_s"] / 1e6, visits_per_ray, r["visits_per_s"] / 1e9,
           r["gb_per_s"]), flush=True)
for h, _ in bufs:
    L.lib.ohmhip_buffer_destroy(h)
if "--json" in sys.argv:
    with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
        json.dump(results, fh, indent=1)
print(json.dumps(results))
