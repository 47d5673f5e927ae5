"""The Python side of ohm_amd/lib/gpumap_driver (ohm_amd/host/gpumap_driver.cpp, built by __graft_entry__.build() with
plain g++), shared by every test that runs the C++14 host mirror: the rays file, one driver process per call, the region
dump, and the mirror's source text for the tests that check what it declares."""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_DIR = os.path.join(ROOT, "ohm_amd", "host")
DRIVER = os.path.join(ROOT, "ohm_amd", "lib", "gpumap_driver")


def write_rays(path, rays):
    """rays.bin: u64 points, then 3 doubles a point."""
    rays = np.ascontiguousarray(rays, dtype=np.float64)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", rays.shape[0]))
        f.write(rays.tobytes())


def run(mode, resolution, batch, source, *extra, timeout=300, driver=DRIVER):
    """One run of `gpumap_driver <mode> <resolution> <batch> <input> <out.bin> [extra ...]`; returns the bytes of out.bin.
    `source`: an array of ray points (written as rays.bin), the bytes of an input file of another layout, or None for a
    mode that reads no file.  An `extra` argument given as bytes goes into a file of its own and its path is passed.
    `driver`: another program that takes the same arguments (ohm_amd/lib/binding_core_driver)."""
    assert os.path.exists(driver), "%s missing: run __graft_entry__.build()" % os.path.basename(driver)
    with tempfile.TemporaryDirectory() as tmp:
        ip, op = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        if isinstance(source, bytes):
            with open(ip, "wb") as f:
                f.write(source)
        elif source is not None:
            write_rays(ip, source)
        args = []
        for i, arg in enumerate(extra):
            if isinstance(arg, bytes):
                path = os.path.join(tmp, "extra%d.bin" % i)
                with open(path, "wb") as f:
                    f.write(arg)
                arg = path
            args.append(str(arg))
        res = subprocess.run([driver, mode, repr(float(resolution)), str(batch), ip if source is not None else "-", op] + args,
                             capture_output=True, text=True, timeout=timeout)
        assert res.returncode == 0, (mode, res.returncode, res.stdout, res.stderr)
        with open(op, "rb") as f:
            return f.read()


def read_region_dump(data, n_layers, maps=1, tail=False):
    """The driver's map dump, `maps` times over: u64 regions, then per region i16[3] key and per layer u32 layer id,
    u64 bytes, payload.  Returns {key: {layer name: array}} (a list of them for maps > 1); with `tail` also the bytes
    that follow, which otherwise must be none."""
    from ohm_amd import LAYERS
    id_to_name = {v[0]: k for k, v in LAYERS.items()}
    off, out = 0, []
    for _ in range(maps):
        (n_regions,) = struct.unpack_from("<Q", data, off)
        off += 8
        chunks = {}
        for _r in range(n_regions):
            key = struct.unpack_from("<3h", data, off)
            off += 6
            layers = {}
            for _l in range(n_layers):
                lid, nbytes = struct.unpack_from("<IQ", data, off)
                off += 12
                dtype = np.dtype(LAYERS[id_to_name[lid]][1])
                layers[id_to_name[lid]] = np.frombuffer(data, dtype=dtype, count=nbytes // dtype.itemsize, offset=off).copy()
                off += nbytes
            chunks[tuple(key)] = layers
        out.append(chunks)
    assert tail or off == len(data)
    out = out[0] if maps == 1 else out
    return (out, data[off:]) if tail else out


def host_mirror_text():
    """OhmGpuMap.h and every header of ohm_amd/host it includes, directly or not, each once, concatenated."""
    seen, text = [], []

    def take(name):
        if name in seen or not os.path.exists(os.path.join(HOST_DIR, name)):
            return
        seen.append(name)
        with open(os.path.join(HOST_DIR, name)) as fh:
            body = fh.read()
        for included in re.findall(r'#include "([^"]+)"', body):
            take(included)
        text.append(body)

    take("OhmGpuMap.h")
    return "\n".join(text)


def driver_text():
    with open(os.path.join(HOST_DIR, "gpumap_driver.cpp")) as fh:
        return fh.read()
