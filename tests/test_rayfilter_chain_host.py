"""CPU: the host build of the ray-filter chain (ohm_amd/csrc/ray_filter_chain.h, the one function the device pass, the
staging threads' count and k_count_passed share) as a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer -- scripts/probes/rayfilter_chain_check.cpp, its own main, never loaded into Python -- over
every chain of the case list; what it prints equals the model bit for bit (a NaN equals a NaN)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rayfilter_chain_cases as cases
import rayfilter_chain_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "scripts", "probes", "rayfilter_chain_check.cpp")


def _stage_record(st):
    kind = ref.KINDS[st[0]]
    if st[0] in ("good", "clip"):
        return struct.pack("<iid6d", kind, 0, st[1], *([0.0] * 6))
    return struct.pack("<iid6d", kind, 0, 0.0, *(tuple(st[1]) + tuple(st[2])))


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{chain name: (keep, rays, flags)} as the sanitized program prints them."""
    tmp = tmp_path_factory.mktemp("rayfilter_chain_check")
    compiler = shutil.which("g++") or shutil.which("clang++")
    assert compiler, "no host C++ compiler"
    exe = str(tmp / "rayfilter_chain_check")
    # (the runtimes linked statically where the compiler knows the options: the binary carries its own sanitizer runtime)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler) == "g++" else []
    subprocess.check_call([compiler, "-std=c++14", "-O1", "-g", "-ffp-contract=off", "-Wall",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static + ["-o", exe, SOURCE])
    names = sorted(cases.CHAINS)
    rays = np.ascontiguousarray(cases.all_rays())
    n_rays = rays.shape[0] // 2
    path = str(tmp / "cases.bin")
    with open(path, "wb") as fh:
        for name in names:
            stages = cases.CHAINS[name]
            fh.write(struct.pack("<I", len(stages)))
            for st in stages:
                fh.write(_stage_record(st))
            fh.write(struct.pack("<Q", n_rays))
            fh.write(rays.tobytes())
    done = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    assert not done.stderr, done.stderr.decode()[-2000:]  # a sanitizer report
    lines = done.stdout.decode().splitlines()
    out = {}
    at = 0
    for index, name in enumerate(names):
        assert lines[at].split() == ["chain", str(index), str(n_rays)]
        rows = [ln.split() for ln in lines[at + 1:at + 1 + n_rays]]
        at += 1 + n_rays
        keep = np.array([row[0] == "1" for row in rows])
        flags = np.array([int(row[1]) for row in rows], dtype=np.uint8)
        bits = np.array([[int(x, 16) for x in row[2:8]] for row in rows], dtype=np.uint64)
        out[name] = (keep, bits.view(np.float64).reshape(-1, 3), flags)
    assert at == len(lines)
    return out


@pytest.mark.parametrize("chain_name", sorted(cases.CHAINS))
def test_sanitized_host_build_equals_model(results, chain_name):
    keep, rays_out, flags = results[chain_name]
    cases.assert_equals_model(chain_name, keep, rays_out, flags, "host build under ASan + UBSan")
