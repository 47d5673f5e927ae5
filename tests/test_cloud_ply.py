"""CPU: a VoxelCloud written by the PLY saver (ohm_amd/cloud.py) and read back by the parser below gives back the same
doubles and colours."""
import os
import tempfile

import numpy as np

from ohm_amd import GPU_KEY_DTYPE, VoxelCloud, write_ply

_TYPES = {"double": "<f8", "float": "<f4", "uchar": "u1"}


def read_ply(path):
    """A binary little-endian PLY with one vertex element: the vertices as a structured array."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    count, fields = None, []
    for line in lines[2:]:
        words = line.split()
        if words[:2] == ["element", "vertex"]:
            count = int(words[2])
        elif words[:1] == ["property"]:
            fields.append((words[2], _TYPES[words[1]]))
    dtype = np.dtype(fields)
    assert len(data) - end == count * dtype.itemsize
    return np.frombuffer(data, dtype=dtype, count=count, offset=end)


def make_cloud(n):
    rng = np.random.default_rng(7)
    positions = rng.standard_normal((n, 3)) * 100.0
    if n:
        positions[0] = (1e-300, -0.0, 1.7976931348623157e308)
    return VoxelCloud(positions, np.zeros(n, dtype=GPU_KEY_DTYPE), rng.standard_normal(n).astype(np.float32), n)


def test_positions_round_trip():
    cloud = make_cloud(1000)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.ply")
        assert write_ply(path, cloud) == 1000
        got = read_ply(path)
    assert got.dtype.names == ("x", "y", "z")
    back = np.stack([got["x"], got["y"], got["z"]], axis=1)
    assert np.array_equal(back.view(np.uint64), cloud.positions.view(np.uint64))


def test_colours_round_trip():
    cloud = make_cloud(257)
    colours = np.random.default_rng(3).integers(0, 256, size=(257, 3), dtype=np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        for colour in (colours, lambda c: colours[:len(c)]):
            path = os.path.join(tmp, "cloud.ply")
            assert write_ply(path, cloud, colour) == 257
            got = read_ply(path)
            assert got.dtype.names == ("x", "y", "z", "red", "green", "blue") and got.dtype.itemsize == 27
            assert np.array_equal(np.stack([got["x"], got["y"], got["z"]], axis=1).view(np.uint64),
                                  cloud.positions.view(np.uint64))
            assert np.array_equal(np.stack([got["red"], got["green"], got["blue"]], axis=1), colours)


def test_empty_cloud():
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "cloud.ply")
        assert write_ply(path, make_cloud(0)) == 0
        assert read_ply(path).shape == (0,)
