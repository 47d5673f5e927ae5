"""Python mirror of ohm/CompareMaps.h over ohmhip_map_compare (include/ohmhip.h, MAP COMPARE): compareLayoutLayer,
compareVoxels and configureTolerance on two GpuMaps, and what utils/ohmcmp does with them (compare_maps,
occupancy_stats).  The comparison runs on the device; only the result and the listed mismatches cross to the host.

A Tolerance stands for the reference's dummy MapLayer: a list of (member name, data type, 64-bit clear value).  As in the
reference the compared member's own type reads the stored bytes, whatever type the tolerance was configured with."""
import ctypes as C
import enum

import numpy as np

from . import _lib as L
from .cloud import GPU_KEY_DTYPE, count_cloud
from .gpumap import LAYERS

#: layer name -> its members in voxel order, (name, numpy dtype): ohm/DefaultLayer.cpp:85-303
MEMBERS = {
    "occupancy": (("occupancy", np.float32),),
    "mean": (("coord", np.uint32), ("count", np.uint32)),
    "covariance": tuple((n, np.float32) for n in ("P00", "P01", "P11", "P02", "P12", "P22")),
    "traversal": (("traversal", np.float32),),
    "touch_time": (("touch", np.uint32),),
    "incident_normal": (("packed_normal", np.uint32),),
    "intensity": (("mean", np.float32), ("cov", np.float32)),
    "hit_miss_count": (("hit_count", np.uint32), ("miss_count", np.uint32)),
    "tsdf": (("weight", np.float32), ("distance", np.float32)),
    "clearance": (("clearance", np.float32),),
}


class Severity(enum.IntEnum):
    """ohm::compare::Severity"""
    kInfo = 0
    kWarning = 1
    kError = 2


kZero = 0
kContinue = L.CMP_CONTINUE


class VoxelsResult:
    """ohm::compare::VoxelsResult, plus what the device call reports beside it: `detail` (every field of
    ohmhip_compare_result), `mismatches` (GPU_KEY_DTYPE records, voxel[3] = the mask of failing members) and
    `missing_regions` ((n, 3) int16) -- the listed ones."""

    def __init__(self, voxels_passed=0, voxels_failed=0, layout_match=False, detail=None, mismatches=None,
                 missing_regions=None):
        self.voxels_passed = int(voxels_passed)
        self.voxels_failed = int(voxels_failed)
        self.layout_match = bool(layout_match)
        self.detail = detail or {}
        self.mismatches = mismatches if mismatches is not None else np.zeros(0, dtype=GPU_KEY_DTYPE)
        self.missing_regions = missing_regions if missing_regions is not None else np.zeros((0, 3), dtype=np.int16)

    def __bool__(self):
        return self.voxels_failed == 0 and self.layout_match

    def __repr__(self):
        return "VoxelsResult(passed=%d, failed=%d, layout_match=%s)" % (self.voxels_passed, self.voxels_failed,
                                                                      self.layout_match)


class Tolerance:
    """The tolerance object of compareVoxel (CompareMaps.h:84-112): a named, otherwise empty layer whose members' clear
    values are the allowed absolute errors."""

    def __init__(self, layer_name):
        self.layer_name = layer_name
        self.members = []  # (name, numpy dtype, uint64)

    def indexOf(self, member_name):
        for i, (name, _, _) in enumerate(self.members):
            if name == member_name:
                return i
        return -1

    def memberClearValue(self, index):
        return self.members[index][2]


def _typed(epsilon):
    if isinstance(epsilon, np.generic):
        return epsilon
    if isinstance(epsilon, bool):
        raise TypeError("a tolerance is a number")
    if isinstance(epsilon, int):
        return np.uint32(epsilon) if epsilon >= 0 else np.int32(epsilon)
    return np.float32(epsilon)


def configureTolerance(tolerance, member_name, epsilon):
    """ohm::compare::configureTolerance (CompareMaps.cpp:389-469): the absolute value of epsilon, its typed bytes in the
    low end of a uint64.  A numpy scalar's dtype selects the overload; a Python float is a float32, a Python int a uint32
    (an int32 when negative)."""
    eps = _typed(epsilon)
    dtype = eps.dtype
    if dtype.kind == "f":
        if dtype.itemsize not in (4, 8):
            raise TypeError("no configureTolerance overload for %s" % dtype)
        raw = np.abs(eps).tobytes()
    elif dtype.kind == "i":
        raw = np.uint64(abs(int(eps))).tobytes()  # (std::abs, widened to the 64-bit value)
    elif dtype.kind == "u":
        raw = np.uint64(int(eps)).tobytes()
    else:
        raise TypeError("no configureTolerance overload for %s" % dtype)
    bits = int.from_bytes(raw.ljust(8, b"\0"), "little")
    tolerance.members.append((str(member_name), dtype, bits))


class VoxelMismatch(str):
    """A log message of compareVoxels that also carries what it says: key (a GPU_KEY_DTYPE record with voxel[3] = 0),
    layer, member, have (eval's value) and expect (ref's)."""

    def __new__(cls, layer, key, member, have, expect):
        region = tuple(int(v) for v in key["region"])
        local = tuple(int(v) for v in key["voxel"][:3])
        self = super().__new__(cls, "%s voxel %s:%s differs in %s: eval holds %r, ref holds %r"
                               % (layer, region, local, member, have.item(), expect.item()))
        self.layer, self.key, self.member, self.have, self.expect = layer, key, member, have, expect
        return self


def compare_params(layer_name, tolerance=None, flags=0, keys=None):
    """(ohmhip_compare_params, the key array it points into) for a layer by name."""
    p = L.CompareParams()
    p.flags = int(flags)
    p.layer_id = LAYERS[layer_name][0]
    for i, (name, _) in enumerate(MEMBERS[layer_name]):
        at = tolerance.indexOf(name) if tolerance is not None else -1
        if at != -1:
            p.tolerance_members |= 1 << i
            p.tolerance_bits[i] = tolerance.memberClearValue(at)
    if keys is not None:
        keys = np.ascontiguousarray(keys, dtype=np.int16).reshape(-1, 3)
        p.keys_xyz, p.key_count = (keys.ctypes.data, len(keys)) if len(keys) else (None, 0)
    return p, keys


def compare_raw(eval_map, ref_map, params, mismatch_capacity=0, missing_capacity=0):
    """ohmhip_map_compare: (status, result fields as a dict, mismatch keys, missing regions), the lists cut to what
    landed."""
    keys = np.zeros(int(mismatch_capacity), dtype=GPU_KEY_DTYPE)
    missing = np.zeros((int(missing_capacity), 3), dtype=np.int16)
    res = L.CompareResult()
    status = L.lib.ohmhip_map_compare(eval_map._handle, ref_map._handle, C.byref(params), int(mismatch_capacity),
                                      keys.ctypes.data if mismatch_capacity else None, int(missing_capacity),
                                      missing.ctypes.data if missing_capacity else None, C.byref(res))
    detail = {}
    for name, _ in L.CompareResult._fields_:
        value = getattr(res, name)
        detail[name] = [int(v) for v in value] if hasattr(value, "__len__") else int(value)
    return (status, detail, keys[:min(detail["mismatch_count"], int(mismatch_capacity))],
            missing[:min(detail["missing_count"], int(missing_capacity))])


def compareLayoutLayer(eval_map, ref_map, layer_name, flags=0, log=None):
    """ohm::compare::compareLayoutLayer (CompareMaps.cpp:78-144).  A layer has one layout in this library, so what is
    left to check is that both maps hold it."""
    ok = True
    for which, gpu_map in (("reference", ref_map), ("evaluated", eval_map)):
        if layer_name not in LAYERS or not gpu_map.hasLayer(layer_name):
            if log:
                log(Severity.kError, "the %s map holds no layer named %s" % (which, layer_name))
            ok = False
    return ok


def compareVoxels(eval_map, ref_map, layer_name, tolerance=None, flags=0, log=None, max_logged=1024, keys=None):
    """ohm::compare::compareVoxels (CompareMaps.cpp:334-386) on the device.  With `log`, the first max_logged failing
    voxels of regions both maps hold are fetched (readVoxels) and reported, one VoxelMismatch per failing member at
    Severity.kError.  keys: only these regions of ref."""
    if not compareLayoutLayer(eval_map, ref_map, layer_name, flags, log):
        return VoxelsResult()
    for gpu_map in (eval_map, ref_map):
        gpu_map._push_config_if_changed()
    params, keys = compare_params(layer_name, tolerance, flags, keys)
    capacity = int(max_logged) if log else 0
    status, detail, mismatches, missing = compare_raw(eval_map, ref_map, params, capacity, capacity)
    L.check(status, "compareVoxels")
    if log and len(mismatches):
        where = mismatches.copy()
        where["voxel"][:, 3] = 0
        have, _ = eval_map.readVoxels(where, layer_name)
        expect, _ = ref_map.readVoxels(where, layer_name)
        members = MEMBERS[layer_name]
        have, expect = have.reshape(len(where), len(members)), expect.reshape(len(where), len(members))
        for n in range(len(where)):
            for i, (name, _) in enumerate(members):
                if (int(mismatches["voxel"][n, 3]) >> i) & 1:
                    log(Severity.kError, VoxelMismatch(layer_name, where[n], name, have[n, i], expect[n, i]))
    return VoxelsResult(detail["voxels_passed"], detail["voxels_failed"], detail["layout_match"] != 0, detail, mismatches,
                        missing)


def default_tolerances():
    """buildDefaultLayerTolerances (utils/ohmcmp/ohmcmp.cpp:109-150): {layer name: Tolerance}."""
    table = {}
    for layer, members, eps in (("occupancy", ("occupancy",), 1e2), ("covariance", [m for m, _ in MEMBERS["covariance"]], 1e-2),
                                ("clearance", ("clearance",), 1e-3), ("intensity", ("mean", "cov"), 1e-3)):
        tol = Tolerance(layer)
        for member in members:
            configureTolerance(tol, member, np.float32(eps))
        table[layer] = tol
    return table


def occupancy_stats(gpu_map):
    """calcuateOccupancyStats (ohmcmp.cpp:191-218): (occupied, free) voxels by occupancyType, counted on the device with
    two ohmhip_map_cloud_count calls; (0, 0) for a map without the occupancy layer."""
    occupied = count_cloud(gpu_map)
    return occupied, count_cloud(gpu_map, export_free=True) - occupied


class MapsComparison:
    """What compare_maps returns: ok (the tool's verdict), layout {layer: bool}, voxels {layer: VoxelsResult},
    eval_stats / ref_stats ((occupied, free)), layers_differ."""

    def __init__(self):
        self.ok = True
        self.layout, self.voxels = {}, {}
        self.eval_stats = self.ref_stats = (0, 0)
        self.layers_differ = False

    def __bool__(self):
        return self.ok


def compare_maps(eval_map, ref_map, layers=None, tolerances=True, stop_on_error=False, compare_layout=True,
                 compare_voxels=True, log=None, max_logged=1024):
    """What ohmcmp's main does once both maps are loaded (ohmcmp.cpp:285-393): a warning when the (filtered) layer lists
    differ, the layout pass, the occupancy statistics, then a voxel pass per layer of the evaluated map -- with the
    tool's default tolerances when `tolerances` is true, or with a {layer name: Tolerance} of the caller's."""
    out = MapsComparison()
    eval_layers, ref_layers = list(eval_map.map().layers), list(ref_map.map().layers)
    if layers:
        eval_layers = [name for name in eval_layers if name in layers]
        ref_layers = [name for name in ref_layers if name in layers]
    if eval_layers != ref_layers:
        out.layers_differ = True
        if log:
            log(Severity.kWarning, "the maps list different layers: evaluated %s, reference %s"
                % (", ".join(eval_layers), ", ".join(ref_layers)))
    flags = kZero if stop_on_error else kContinue
    if compare_layout:
        for name in eval_layers:
            out.layout[name] = compareLayoutLayer(eval_map, ref_map, name, flags, log)
            out.ok = out.ok and out.layout[name]
    if compare_voxels:
        out.eval_stats, out.ref_stats = occupancy_stats(eval_map), occupancy_stats(ref_map)
        table = tolerances if isinstance(tolerances, dict) else (default_tolerances() if tolerances else {})
        for name in eval_layers:
            result = compareVoxels(eval_map, ref_map, name, table.get(name), flags, log, max_logged)
            out.voxels[name] = result
            out.ok = out.ok and bool(result)
    return out
