"""CPU restatement of the clearance layer's stale set (include/ohmhip.h, ohmhip_map_clearance_stale_regions) -- TEST
INFRASTRUCTURE.  It replays a log of what happened to the map, in order, with no epochs: a region R present in the map
is stale for parameters P when R was never written with P (new, last written with other parameters, or its clearance
layer written by the host), or when a region within D_a = ceil(h / region_dim_a) of R on every axis (keys wrap in int16)
had its occupancy changed or was removed after R was last written.  Stale regions are listed in ascending (z, y, x)
signed key order."""
from clearance_ref import half_extent


def reach(h, region_dim):
    """D per axis: ceil(h / region_dim_a)."""
    return tuple(-(-int(h) // int(d)) for d in region_dim)


def wrap16(v):
    return (int(v) + 32768) % 65536 - 32768


def neighbourhood(key, d):
    """Every region key within d[a] of key on each axis, int16-wrapped (key itself included)."""
    x, y, z = (int(v) for v in key)
    return {(wrap16(x + dx), wrap16(y + dy), wrap16(z + dz))
            for dz in range(-d[2], d[2] + 1) for dy in range(-d[1], d[1] + 1) for dx in range(-d[0], d[0] + 1)}


def order_key(key):
    x, y, z = (int(v) for v in key)
    return (z, y, x)


def params_of(search_radius, flags=0, axis_scaling=(1.0, 1.0, 1.0)):
    """The parameter set as the library compares it (flags other than the two that change results are ignored)."""
    import numpy as np
    return (float(np.float32(search_radius)), tuple(float(np.float32(v)) for v in axis_scaling), int(flags) & 0x11)


class ClearanceLog:
    """The log of one map.  change / remove / host_write / written record events as they happen; stale(present, P)
    is the stale list for parameter set P over the regions present now."""

    def __init__(self, resolution, region_dim):
        self.resolution = float(resolution)
        self.region_dim = tuple(int(v) for v in region_dim)
        self.time = 0
        self.last_change = {}   # region -> time of its last occupancy change or removal
        self.last_write = {}    # region -> (time, params) of its last computed write; absent: never / host-written

    def _tick(self):
        self.time += 1
        return self.time

    def change(self, keys):
        """Occupancy of these regions changed (a batch touched them, an upload, mark_dirty, a merge)."""
        t = self._tick()
        for k in keys:
            self.last_change[tuple(int(v) for v in k)] = t

    def remove(self, keys):
        t = self._tick()
        for k in keys:
            k = tuple(int(v) for v in k)
            self.last_change[k] = t
            self.last_write.pop(k, None)

    def host_write(self, keys):
        """The host wrote these regions' clearance layer."""
        self._tick()
        for k in keys:
            self.last_write.pop(tuple(int(v) for v in k), None)

    def written(self, keys, params):
        """An update computed these regions with parameter set `params` (params_of)."""
        t = self._tick()
        for k in keys:
            self.last_write[tuple(int(v) for v in k)] = (t, params)

    def stale(self, present, params):
        h = half_extent(params[0], self.resolution)
        d = reach(h, self.region_dim)
        out = []
        for k in sorted((tuple(int(v) for v in p) for p in present), key=order_key):
            w = self.last_write.get(k)
            if w is None or w[1] != params:
                out.append(k)
                continue
            if any(self.last_change.get(n, 0) > w[0] for n in neighbourhood(k, d)):
                out.append(k)
        return out
