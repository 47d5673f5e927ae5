"""numpy models of a layer change (include/ohmhip.h, "LAYER CHANGES"), written from the reference's code and the header's
rules, not from the library's:

  update_chunks       MapChunk::updateLayout (ohm/MapChunk.cpp:93-143) over a {region: {layer name: block}} dict: blocks
                      of layers in both layouts stay the same objects, an added layer gets a block of its clear value
                      (ohm/DefaultLayer.cpp), a removed layer's block goes.
  record_layout       where a region's blocks lie in a record of the host store (U4): the layers the map holds in layer-id
                      order, then the replay-mask row, every part on a 256-byte boundary.
  relayout_record     a record rewritten from one layer set into another: common layers and the mask row copied, added
                      layers cleared.
  bytes_per_region    what a resident region costs against the memory limit (U5), per layer set and mode.
"""
import numpy as np

LAYER_IDS = {"occupancy": 0, "mean": 1, "covariance": 2, "traversal": 3, "touch_time": 4, "incident_normal": 5,
             "intensity": 6, "hit_miss_count": 7, "tsdf": 8, "clearance": 9}
LAYER_BYTES = {"occupancy": 4, "mean": 8, "covariance": 24, "traversal": 4, "touch_time": 4, "incident_normal": 4,
               "intensity": 8, "hit_miss_count": 8, "tsdf": 8, "clearance": 4}
#: the 32-bit word every word of a cleared block holds: float +inf, float -1.0, zero
CLEAR_WORD = {name: 0 for name in LAYER_IDS}
CLEAR_WORD["occupancy"] = 0x7f800000
CLEAR_WORD["clearance"] = 0xbf800000
RECORD_ALIGN = 256
MODE_OCCUPANCY, MODE_NDT_OM, MODE_NDT_TM, MODE_TSDF = range(4)
#: U7
REQUIRED = {MODE_OCCUPANCY: ("occupancy",), MODE_NDT_OM: ("occupancy", "mean", "covariance"),
            MODE_NDT_TM: ("occupancy", "mean", "covariance", "intensity", "hit_miss_count"), MODE_TSDF: ("tsdf",)}


def layer_mask(layers):
    mask = 0
    for name in layers:
        mask |= 1 << LAYER_IDS[name]
    return mask


def clear_block(name, region_voxels):
    """The bytes of a cleared block of layer `name`, as uint32 words."""
    return np.full(region_voxels * LAYER_BYTES[name] // 4, CLEAR_WORD[name], dtype=np.uint32)


def update_chunks(chunks, old_layers, new_layers, region_voxels):
    """MapChunk::updateLayout for every chunk, in place.  Blocks are arrays of any dtype; an added block is uint32 words
    (compare bytes)."""
    for chunk in chunks.values():
        for name in old_layers:
            if name not in new_layers:
                chunk.pop(name, None)
        for name in new_layers:
            if name not in chunk:
                chunk[name] = clear_block(name, region_voxels)
    return chunks


def _align(n):
    return (n + RECORD_ALIGN - 1) // RECORD_ALIGN * RECORD_ALIGN


def record_layout(layers, region_voxels):
    """({layer name: offset}, mask offset, mask bytes, record bytes) of a store record for the set `layers`."""
    at, offsets = 0, {}
    for name in sorted(layers, key=LAYER_IDS.get):
        offsets[name] = at
        at += _align(region_voxels * LAYER_BYTES[name])
    mask_bytes = (region_voxels + 31) // 32 * 4
    return offsets, at, mask_bytes, at + _align(mask_bytes)


def relayout_record(record, old_layers, new_layers, region_voxels):
    """`record` (uint8, the layout of old_layers) in the layout of new_layers."""
    old_at, old_mask, mask_bytes, old_size = record_layout(old_layers, region_voxels)
    new_at, new_mask, _, new_size = record_layout(new_layers, region_voxels)
    assert record.dtype == np.uint8 and record.size == old_size
    out = np.zeros(new_size, dtype=np.uint8)
    for name, at in new_at.items():
        size = region_voxels * LAYER_BYTES[name]
        if name in old_at:
            out[at:at + size] = record[old_at[name]:old_at[name] + size]
        else:
            out[at:at + size] = clear_block(name, region_voxels).view(np.uint8)
    out[new_mask:new_mask + mask_bytes] = record[old_mask:old_mask + mask_bytes]
    return out


def bytes_per_region(layers, region_voxels, mode=MODE_OCCUPANCY):
    """A tile's blocks of every layer, the walk's visit counters (4 B a voxel), the replay-mask row, in occupancy mode
    the first-sample table (4 B a voxel), with the traversal layer its accumulator (8 B a voxel)."""
    total = sum(LAYER_BYTES[name] for name in set(layers)) * region_voxels
    total += 4 * region_voxels + (region_voxels + 31) // 32 * 4
    total += 4 * region_voxels if mode == MODE_OCCUPANCY else 0
    total += 8 * region_voxels if "traversal" in layers else 0
    return total


def regions_to_evict(resident, memory_limit, new_layers, region_voxels, mode=MODE_OCCUPANCY):
    """U5: how many of `resident` regions have to move to the store for the new set to fit `memory_limit` (0: none)."""
    if not memory_limit:
        return 0
    return max(0, resident - memory_limit // bytes_per_region(new_layers, region_voxels, mode))
