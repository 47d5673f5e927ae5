"""CPU: the models of tests/layout_ref.py against hand-written cases, the layer sizes of tests/copy_ref.py and the host
mirror's OccupancyMap.updateLayout / removeLayer."""
import numpy as np
import pytest

import copy_ref
import layout_ref as R


def test_layer_tables_agree_with_copy_ref_and_the_binding():
    from ohm_amd import LAYERS
    assert R.LAYER_BYTES == copy_ref.LAYER_BYTES
    assert R.LAYER_IDS == {name: spec[0] for name, spec in LAYERS.items()}
    for name, (_, dtype, comps) in LAYERS.items():
        assert np.dtype(dtype).itemsize * comps == R.LAYER_BYTES[name]
    assert np.array([R.CLEAR_WORD["occupancy"]], dtype=np.uint32).view(np.float32)[0] == np.inf
    assert np.array([R.CLEAR_WORD["clearance"]], dtype=np.uint32).view(np.float32)[0] == -1.0
    assert all(word == 0 for name, word in R.CLEAR_WORD.items() if name not in ("occupancy", "clearance"))


def test_update_chunks_by_hand():
    occ = np.arange(8, dtype=np.float32)
    mean = np.arange(16, dtype=np.uint32)
    chunks = {(0, 0, 0): {"occupancy": occ, "mean": mean}, (1, -2, 3): {"occupancy": occ.copy(), "mean": mean.copy()}}
    R.update_chunks(chunks, ["occupancy", "mean"], ["occupancy", "clearance", "covariance"], 8)
    for chunk in chunks.values():
        assert sorted(chunk) == ["clearance", "covariance", "occupancy"]
        assert chunk["clearance"].view(np.float32).tolist() == [-1.0] * 8
        assert chunk["covariance"].tolist() == [0] * 48
    assert chunks[(0, 0, 0)]["occupancy"] is occ  # (kept, not copied)
    # removing a layer and adding it again yields a cleared block
    R.update_chunks(chunks, ["occupancy", "clearance", "covariance"], ["occupancy", "clearance", "covariance", "mean"], 8)
    assert chunks[(0, 0, 0)]["mean"].tolist() == [0] * 16
    # an added occupancy block is unobserved
    only = {(0, 0, 0): {"tsdf": np.zeros(16, dtype=np.float32)}}
    R.update_chunks(only, ["tsdf"], ["tsdf", "occupancy"], 8)
    assert np.all(np.isposinf(only[(0, 0, 0)]["occupancy"].view(np.float32)))


def test_record_layout_by_hand():
    # 16^3 regions: occupancy 16384 B, mean 32768 B, mask row 512 B -- all multiples of 256
    at, mask_at, mask_bytes, size = R.record_layout(["mean", "occupancy"], 4096)
    assert at == {"occupancy": 0, "mean": 16384} and (mask_at, mask_bytes, size) == (49152, 512, 49664)
    # 3 x 3 x 3 regions: every part is padded to 256 bytes, the mask row comes last
    at, mask_at, mask_bytes, size = R.record_layout(["occupancy", "covariance", "clearance"], 27)
    assert at == {"occupancy": 0, "covariance": 256, "clearance": 256 + 768}
    assert (mask_at, mask_bytes, size) == (256 + 768 + 256, 4, 256 + 768 + 256 + 256)
    # layer-id order, whatever order the names come in
    assert R.record_layout(["tsdf", "traversal"], 27)[0] == {"traversal": 0, "tsdf": 256}


def test_relayout_record_by_hand():
    rv = 40
    old, new = ["occupancy", "mean"], ["occupancy", "traversal", "clearance"]
    old_at, old_mask, mask_bytes, old_size = R.record_layout(old, rv)
    record = np.zeros(old_size, dtype=np.uint8)
    occ = np.arange(rv, dtype=np.float32)  # (no byte of these is 0xab)
    record[0:rv * 4] = occ.view(np.uint8)
    record[old_at["mean"]:old_at["mean"] + rv * 8] = 0xab
    record[old_mask:old_mask + mask_bytes] = np.arange(mask_bytes, dtype=np.uint8) + 1
    out = R.relayout_record(record, old, new, rv)
    new_at, new_mask, _, new_size = R.record_layout(new, rv)
    assert out.size == new_size
    assert np.array_equal(out[0:rv * 4].view(np.float32), occ)
    assert not out[new_at["traversal"]:new_at["traversal"] + rv * 4].any()
    assert out[new_at["clearance"]:new_at["clearance"] + rv * 4].view(np.float32).tolist() == [-1.0] * rv
    assert out[new_mask:new_mask + mask_bytes].tolist() == list(range(1, mask_bytes + 1))
    assert 0xab not in out  # the removed layer's bytes are nowhere
    # there and back: the common layer and the mask row survive, the re-added layer is clear
    back = R.relayout_record(out, new, old, rv)
    assert np.array_equal(back[0:rv * 4], record[0:rv * 4]) and not back[old_at["mean"]:old_at["mean"] + rv * 8].any()
    assert np.array_equal(back[old_mask:old_mask + mask_bytes], record[old_mask:old_mask + mask_bytes])


def test_bytes_per_region_and_eviction_arithmetic():
    rv = 4096
    assert R.bytes_per_region(["occupancy"], rv) == rv * (4 + 4 + 4) + 512
    assert R.bytes_per_region(["occupancy", "mean"], rv) == rv * (4 + 8 + 4 + 4) + 512
    assert R.bytes_per_region(["occupancy", "traversal"], rv) == rv * (4 + 4 + 4 + 4 + 8) + 512
    assert R.bytes_per_region(["tsdf"], rv, R.MODE_TSDF) == rv * (8 + 4) + 512
    limit = 3 * R.bytes_per_region(["occupancy"], rv) + 100
    assert R.regions_to_evict(3, limit, ["occupancy"], rv) == 0
    assert R.regions_to_evict(3, limit, ["occupancy", "mean"], rv) == 2  # 149 092 // 82 432: one region fits
    assert R.regions_to_evict(3, 0, ["occupancy", "mean"], rv) == 0


@pytest.mark.parametrize("dims", [(16, 16, 16), (5, 3, 2)])
def test_host_mirror_update_layout_follows_the_model(dims):
    from ohm_amd import OccupancyMap
    rv = dims[0] * dims[1] * dims[2]
    map_ = OccupancyMap(0.1, dims, layers=("occupancy", "mean"))
    rng = np.random.RandomState(3)
    for key in [(0, 0, 0), (-1, 2, 5)]:
        map_.chunks[key] = {"occupancy": rng.rand(rv).astype(np.float32),
                            "mean": rng.randint(0, 1 << 30, 2 * rv).astype(np.uint32)}
    model = {key: dict(chunk) for key, chunk in map_.chunks.items()}
    kept = {key: chunk["occupancy"] for key, chunk in map_.chunks.items()}
    steps = [["occupancy", "mean", "clearance", "traversal"], ["occupancy", "clearance"],
             ["occupancy", "clearance", "mean", "covariance"]]
    layers = list(map_.layers)
    for new in steps:
        map_.updateLayout(new)
        R.update_chunks(model, layers, new, rv)
        layers = new
        assert map_.layers == new
        for key, chunk in map_.chunks.items():
            assert sorted(chunk) == sorted(new) == sorted(model[key])
            assert chunk["occupancy"] is kept[key]
            for name in new:
                assert chunk[name].tobytes() == model[key][name].tobytes(), (key, name)
    map_.removeLayer("clearance")
    assert map_.layers == ["occupancy", "mean", "covariance"] and all("clearance" not in c for c in map_.chunks.values())
    with pytest.raises(KeyError):
        map_.updateLayout(["occupancy", "no_such_layer"])
    map_.updateLayout(["occupancy"], preserve_map=False)
    assert map_.layers == ["occupancy"] and not map_.chunks
