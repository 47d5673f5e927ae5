"""Inputs shared by the heightmap tests (CPU restatement and device) -- TEST INFRASTRUCTURE.

surface_selection_cases(): Heightmap.SurfaceSelection of the reference (tests/ohmtestheightmap/HeightmapTests.cpp:
686-878) restated: 13 below / above configurations x 3 surface modes on the 1 m map of 8 x 8 x 2-voxel regions with
origin -0.5, source voxels written directly (a hit: hit_value, a miss: miss_value, as integrateHit / integrateMiss
leave a fresh voxel), the clip box and heightmap origin as the test sets them, and the expectations of its two tables.

two_level_scene(): rays of a floor with a platform above part of it, seen from a sensor above the platform and a second
low sensor that looks under it."""
import numpy as np

from oracle.oracle import OracleMap
from heightmap_ref import HM_SURFACE, HM_UNKNOWN, HM_VIRTUAL, Params

REAL, VIRTUAL, VOID = "real", "virtual", "void"
BELOW, ABOVE = "below", "above"
SS_DIM = (8, 8, 2)
SS_ORIGIN = (-0.5, -0.5, -0.5)

# HeightmapTests.cpp:788-803: (type below, type above, which is closer)
SS_TESTS = [(REAL, REAL, BELOW), (REAL, REAL, ABOVE), (REAL, VIRTUAL, BELOW), (REAL, VIRTUAL, ABOVE),
            (VIRTUAL, REAL, BELOW), (VIRTUAL, REAL, ABOVE), (VIRTUAL, VIRTUAL, BELOW), (VIRTUAL, VIRTUAL, ABOVE),
            (REAL, VOID, ABOVE), (VOID, REAL, BELOW), (VIRTUAL, VOID, ABOVE), (VOID, VIRTUAL, BELOW), (VOID, VOID, ABOVE)]
S, V, U = HM_SURFACE, HM_VIRTUAL, HM_UNKNOWN
# :807-859: (expected type, which voxel) per mode: none, virtual surfaces, promote virtual below
SS_RESULTS = [
    [(S, BELOW), (S, BELOW), (S, BELOW), (S, BELOW), (S, ABOVE), (S, ABOVE), (U, None), (U, None), (S, BELOW),
     (S, ABOVE), (U, None), (U, None), (U, BELOW)],
    [(S, BELOW), (S, BELOW), (S, BELOW), (S, BELOW), (S, ABOVE), (S, ABOVE), (V, BELOW), (V, BELOW), (S, BELOW),
     (S, ABOVE), (V, BELOW), (V, ABOVE), (U, BELOW)],
    [(S, BELOW), (S, BELOW), (S, BELOW), (S, BELOW), (V, BELOW), (V, BELOW), (V, BELOW), (V, BELOW), (S, BELOW),
     (S, ABOVE), (V, BELOW), (V, ABOVE), (U, BELOW)],
]


def surface_selection_cases(hit_value, miss_value):
    """Yields (id, chunks, Params, expected type, expected pos.z) for the 39 cases.  chunks: {region: {"occupancy":
    flat float32 block}}; the voxel looked up is the heightmap's voxelKey((0, 0, 0))."""
    selected, other = 5.0, 7.0
    geometry = OracleMap(1.0, SS_DIM)
    geometry.set_origin(SS_ORIGIN)
    for mode in range(3):
        for t, (below, above, closer) in enumerate(SS_TESTS):
            range_below = selected if closer == BELOW else other
            range_above = selected if closer != BELOW else other
            expected_type, select = SS_RESULTS[mode][t]
            expected_height = -range_below if select == BELOW else range_above
            chunks = {}

            def put(z, value):
                region, local = geometry.voxel_key((0.0, 0.0, z))
                block = chunks.setdefault(region, {"occupancy": np.full(8 * 8 * 2, np.inf, dtype=np.float32)})
                block["occupancy"][local[0] + local[1] * 8 + local[2] * 64] = value

            if below == VIRTUAL:
                put(-range_below, miss_value)
            elif below == REAL:
                put(-range_below, hit_value)
            if above == VIRTUAL:
                put(range_above, miss_value)
            elif above == REAL:
                put(range_above, hit_value)
            p = Params(1.0, 0.0, up_axis=2, reference_pos=(0, 0, 0), cull_min=(-0.5, -0.5, -2 * other),
                       cull_max=(0.5, 0.5, 2 * other), origin=SS_ORIGIN, virtual_surface=mode != 0,
                       promote_virtual_below=mode == 2)
            yield "m%d-t%02d" % (mode, t), chunks, p, expected_type, expected_height


def two_level_scene(seed=7, n_floor=12000, n_platform=3000, platform_height=1.0):
    """(rays (2N, 3) f64): floor [-4, 4]^2 x {0}, platform [1, 3] x [-1, 1] x {platform_height}; floor points under and
    around the platform are shot from a low sensor, everything else from one above the platform."""
    rng = np.random.RandomState(seed)
    floor = np.zeros((n_floor, 3))
    floor[:, :2] = rng.uniform(-4.0, 4.0, size=(n_floor, 2))
    plat = np.zeros((n_platform, 3))
    plat[:, 0] = rng.uniform(1.0, 3.0, size=n_platform)
    plat[:, 1] = rng.uniform(-1.0, 1.0, size=n_platform)
    plat[:, 2] = platform_height
    low = (floor[:, 0] > 0.6) & (floor[:, 0] < 3.4) & (np.abs(floor[:, 1]) < 1.4)
    ends = np.concatenate([floor, plat])
    origins = np.empty_like(ends)
    origins[:] = (0.05, 0.05, platform_height + 0.55)
    origins[:n_floor][low] = (0.05, 0.05, 0.45)
    rays = np.empty((2 * ends.shape[0], 3), dtype=np.float64)
    rays[0::2] = origins
    rays[1::2] = ends
    return rays


def rotate_scene(rays, up_axis):
    """The Z-up scene turned so that `up_axis` (ohm::UpAxis, -3 .. 2) is up: z -> +-axis, x and y onto the other two."""
    idx = up_axis if up_axis >= 0 else -up_axis - 1
    sign = 1.0 if up_axis >= 0 else -1.0
    others = [c for c in range(3) if c != idx]
    out = np.empty_like(rays)
    out[:, idx] = sign * rays[:, 2]
    out[:, others[0]] = rays[:, 0]
    out[:, others[1]] = 0.7 * rays[:, 1] + 0.3  # (not symmetric)
    return out
