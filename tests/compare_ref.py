"""CPU restatement of ohm::compare (ohm/CompareMaps.cpp) as include/ohmhip.h states it (MAP COMPARE, K3 - K5), on maps
given as {region (x, y, z): block}, a block being the layer's voxels as a (voxels, members) uint32 array in MapChunk
order.  Every float32 operation is one numpy float32 operation: a comparison, or the one subtraction.

compare_datum / compare_voxel are the scalar forms, written after CompareMaps.cpp:58-75 and :207-331; compare_voxels is
the vectorised closed form the device is held to (tests/test_gpu_compare.py), and walk_stop_at_first the sequential walk
of :359-383 that the closed form's stop-at-first answer is checked against (tests/test_compare_ref.py)."""
import numpy as np

KEY_DTYPE = np.dtype([("region", "<i2", (3,)), ("voxel", "u1", (4,))])
MAX_MEMBERS = 6
CONTINUE = 1

#: layer -> (member names, bit i set: member i is a float32); include/ohmhip.h K2
LAYOUT = {
    "occupancy": (("occupancy",), 0x1),
    "mean": (("coord", "count"), 0x0),
    "covariance": (("P00", "P01", "P11", "P02", "P12", "P22"), 0x3f),
    "traversal": (("traversal",), 0x1),
    "touch_time": (("touch",), 0x0),
    "incident_normal": (("packed_normal",), 0x0),
    "intensity": (("mean", "cov"), 0x3),
    "hit_miss_count": (("hit_count", "miss_count"), 0x0),
    "tsdf": (("weight", "distance"), 0x3),
    "clearance": (("clearance",), 0x1),
}
CLEAR_WORD = {"occupancy": 0x7f800000, "clearance": 0xbf800000}


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def bits_of(value):
    return int(np.array([value], dtype=np.float32).view(np.uint32)[0])


def compare_datum(val_bits, ref_bits, is_float, eps_bits):
    """compareDatum<T> (CompareMaps.cpp:58-75), T = float or uint32_t, on 32-bit patterns.  Returns (pass, hi - lo as a
    bit pattern or None when it is not a number)."""
    if is_float:
        val, ref, eps = f32(val_bits), f32(ref_bits), f32(eps_bits)
        with np.errstate(invalid="ignore", over="ignore"):
            if ref > val:
                val, ref = ref, val
            diff = np.float32(val - ref)
            ok = bool(val == ref) or bool(diff <= eps)
        return ok, (None if np.isnan(diff) else bits_of(diff))
    val, ref, eps = int(val_bits), int(ref_bits), int(eps_bits)
    if ref > val:
        val, ref = ref, val
    diff = (val - ref) & 0xffffffff
    return (val == ref or diff <= eps), diff


def compare_voxel(eval_words, ref_words, float_mask, tol_members, tol_bits):
    """compareVoxel (:207-331) for one voxel: the mask of failing members (0: the voxel passes)."""
    mask = 0
    for i, (e, r) in enumerate(zip(eval_words, ref_words)):
        if (tol_members >> i) & 1:
            ok, _ = compare_datum(int(e), int(r), (float_mask >> i) & 1, int(tol_bits[i]) & 0xffffffff)
        else:
            ok = int(e) == int(r)  # memcmp of the member's 4 bytes
        mask |= 0 if ok else 1 << i
    return mask


def member_masks(eval_block, ref_block, float_mask, tol_members, tol_bits):
    """Vectorised compare_voxel over two (voxels, members) uint32 blocks: (mask per voxel, hi - lo per voxel and member as
    unsigned-ordered words: a positive float difference's bits, 0 for a zero of either sign and for a NaN)."""
    e = np.ascontiguousarray(eval_block, dtype=np.uint32)
    r = np.ascontiguousarray(ref_block, dtype=np.uint32)
    mask = np.zeros(e.shape[0], dtype=np.uint32)
    diffs = np.zeros(e.shape, dtype=np.uint32)
    for i in range(e.shape[1]):
        ei, ri = e[:, i], r[:, i]
        if (float_mask >> i) & 1:
            v, f = ei.view(np.float32), ri.view(np.float32)
            eps = f32(int(tol_bits[i]) & 0xffffffff)
            with np.errstate(invalid="ignore", over="ignore"):
                swap = f > v
                hi, lo = np.where(swap, f, v), np.where(swap, v, f)
                d = (hi - lo).astype(np.float32)
                within = (hi == lo) | (d <= eps)
                diffs[:, i] = np.where(d > np.float32(0), d.view(np.uint32), np.uint32(0))
        else:
            swap = ri > ei
            hi, lo = np.where(swap, ri, ei), np.where(swap, ei, ri)
            d = hi - lo
            within = (hi == lo) | (d <= np.uint32(int(tol_bits[i]) & 0xffffffff))
            diffs[:, i] = d
        ok = within if (tol_members >> i) & 1 else (ei == ri)
        mask |= np.where(ok, np.uint32(0), np.uint32(1 << i))
    return mask, diffs


def region_order(keys):
    """K5: ascending by (rz, ry, rx)."""
    return sorted((tuple(int(v) for v in k) for k in keys), key=lambda k: (k[2], k[1], k[0]))


def select_regions(ref_regions, keys=None):
    """K3: (the regions visited, in order; keys_absent)."""
    present = set(tuple(int(v) for v in k) for k in ref_regions)
    if keys is None:
        return region_order(present), 0
    listed = set(tuple(int(v) for v in k) for k in keys)
    return region_order(listed & present), len(listed - present)


def key_record(region, index, dims, mask):
    rec = np.zeros((), dtype=KEY_DTYPE)
    rec["region"] = region
    rec["voxel"] = (index % dims[0], (index // dims[0]) % dims[1], index // (dims[0] * dims[1]), mask)
    return rec


def empty_result(layer, layout_match):
    return dict(voxels_passed=0, voxels_failed=0, layout_match=int(layout_match), member_count=len(LAYOUT[layer][0]),
                regions_compared=0, regions_missing=0, keys_absent=0, mismatch_count=0, missing_count=0,
                member_failed=[0] * MAX_MEMBERS, member_max_diff=[0] * MAX_MEMBERS)


def compare_voxels(eval_chunks, ref_chunks, layer, dims, tol_members=0, tol_bits=(0,) * MAX_MEMBERS, flags=0, keys=None,
                   mismatch_capacity=0, missing_capacity=0):
    """ohmhip_map_compare's answer: (result fields, mismatch key records, missing regions (n, 3) int16).  eval_chunks /
    ref_chunks: {region: (voxels, members) uint32 block}, or None for a map without the layer."""
    if eval_chunks is None or ref_chunks is None:
        return empty_result(layer, False), np.zeros(0, dtype=KEY_DTYPE), np.zeros((0, 3), dtype=np.int16)
    res = empty_result(layer, True)
    float_mask = LAYOUT[layer][1]
    voxels = dims[0] * dims[1] * dims[2]
    regions, res["keys_absent"] = select_regions(ref_chunks.keys(), keys)
    held = set(tuple(int(v) for v in k) for k in eval_chunks)
    res["regions_missing"] = sum(1 for k in regions if k not in held)
    res["regions_compared"] = len(regions) - res["regions_missing"]
    mismatches, missing = [], []
    keep_going = bool(flags & CONTINUE)
    for region in regions:
        if region not in held:
            if not keep_going:
                res["voxels_failed"], res["missing_count"] = 1, 1
                missing.append(region)
                break
            res["voxels_failed"] += voxels
            res["missing_count"] += 1
            missing.append(region)
            continue
        e = np.asarray(eval_chunks[region]).view(np.uint32).reshape(voxels, -1)
        r = np.asarray(ref_chunks[region]).view(np.uint32).reshape(voxels, -1)
        mask, diffs = member_masks(e, r, float_mask, tol_members, tol_bits)
        failing = np.flatnonzero(mask)
        if not keep_going:
            if len(failing):
                first = int(failing[0])
                res["voxels_passed"] += first
                res["voxels_failed"], res["mismatch_count"] = 1, 1
                res["member_failed"] = [(int(mask[first]) >> i) & 1 for i in range(MAX_MEMBERS)]
                mismatches.append(key_record(region, first, dims, int(mask[first])))
                break
            res["voxels_passed"] += voxels
            continue
        res["voxels_passed"] += voxels - len(failing)
        res["voxels_failed"] += len(failing)
        res["mismatch_count"] += len(failing)
        for i in range(e.shape[1]):
            res["member_failed"][i] += int(np.count_nonzero((mask >> i) & 1))
            res["member_max_diff"][i] = max(res["member_max_diff"][i], int(diffs[:, i].max()))
        for index in failing[:max(0, mismatch_capacity - len(mismatches))]:
            mismatches.append(key_record(region, int(index), dims, int(mask[index])))
    mismatches = mismatches[:mismatch_capacity]
    missing = missing[:missing_capacity]
    return (res, np.array(mismatches, dtype=KEY_DTYPE).reshape(-1),
            np.array(missing, dtype=np.int16).reshape(-1, 3))


def walk_stop_at_first(eval_chunks, ref_chunks, layer, dims, tol_members=0, tol_bits=(0,) * MAX_MEMBERS, keys=None):
    """The reference's loop (CompareMaps.cpp:359-383) without kContinue, voxel after voxel in K5's order: (voxels_passed,
    voxels_failed, (region, voxel index, mask) of the failure or None; mask None for a region eval lacks)."""
    float_mask = LAYOUT[layer][1]
    voxels = dims[0] * dims[1] * dims[2]
    passed = 0
    for region in select_regions(ref_chunks.keys(), keys)[0]:
        ref_block = np.asarray(ref_chunks[region]).view(np.uint32).reshape(voxels, -1)
        eval_block = eval_chunks.get(region)
        if eval_block is not None:
            eval_block = np.asarray(eval_block).view(np.uint32).reshape(voxels, -1)
        for index in range(voxels):
            if eval_block is None:
                return passed, 1, (region, index, None)  # compareVoxel :197-200: an invalid buffer
            mask = compare_voxel(eval_block[index], ref_block[index], float_mask, tol_members, tol_bits)
            if mask:
                return passed, 1, (region, index, mask)
            passed += 1
    return passed, 0, None
