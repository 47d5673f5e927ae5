#!/usr/bin/env python3
"""Per-kernel fingerprint of the gfx950 machine code of a source tree.  CPU only: it cross-compiles, it never runs.

    python scripts/kernel_fingerprint.py [TREE] -o branch.json      # TREE defaults to this checkout
    python scripts/kernel_fingerprint.py --compare parent.json branch.json

Compiles the three .hip sources of TREE device-side to assembly with the build's own flags, cuts the output into
functions (symbol label to .Lfunc_end), drops comments and blank lines, rewrites the local labels .LBB<n>_ to .LBB_ so
that emission order does not matter, and records per function: instruction count, a hash of the normalised text, and the
register / spill / scratch / LDS figures of the code-object metadata.  --compare lists the functions that are missing,
added or different and exits 1 when there are any.  It hashes and diffs; it looks for nothing in the assembly.
To fingerprint the parent of a change, export it (git archive / git worktree) and pass that directory as TREE."""
import argparse
import concurrent.futures
import glob
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIP_FLAGS, HIP_SOURCES, _hipcc  # noqa: E402

META = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")
BUILD_ID = "fingerprint"  # the same for every tree: otherwise the string is the only difference


def compile_asm(tree, src, tmp):
    out = os.path.join(tmp, src + ".s")
    cmd = [_hipcc()] + [f for f in HIP_FLAGS if f not in ("-shared", "-fPIC")] + [
        '-DOHMHIP_BUILD_ID="%s"' % BUILD_ID, "--cuda-device-only", "-S", "-o", out,
        os.path.join(tree, "ohm_amd", "csrc", src)]
    res = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if res.returncode:
        sys.exit("%s failed to compile:\n%s" % (src, res.stderr))
    with open(out) as fh:
        return fh.read()


def metadata(asm):
    """{kernel symbol: {field: int}} of the amdhsa.kernels list; its kernel-level keys sit at '  - ' or four spaces."""
    kernels, cur = {}, {}
    body = asm.split(".amdgpu_metadata", 1)[1].split(".end_amdgpu_metadata", 1)[0] if ".amdgpu_metadata" in asm else ""
    for m in re.finditer(r"^(  - |    )(\.\w+):\s*(\S+)", body + "\n  - .end: 0", re.M):
        if m.group(1) == "  - ":
            if ".name" in cur:
                kernels[cur[".name"]] = {k: int(cur[k]) for k in META if k in cur}
            cur = {}
        cur[m.group(2)] = m.group(3)
    return kernels


def functions(asm):
    """{symbol: (instruction count, hash of the normalised text)} for every function of one assembly file."""
    out, name, lines = {}, None, []
    symbols = set(re.findall(r"^\s*\.type\s+(\S+),@function", asm, re.M))
    for raw in asm.splitlines():
        line = re.sub(r"\.LBB\d+_", ".LBB_", raw.split(";", 1)[0].strip())
        if name is None:
            if line.endswith(":") and line[:-1] in symbols:
                name, lines = line[:-1], []
        elif line.startswith(".Lfunc_end"):
            code = [x for x in lines if not x.startswith(".") and not x.endswith(":")]
            out[name] = (len(code), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16])
            name = None
        elif line:
            lines.append(line)
    return out


def fingerprint(tree):
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(len(HIP_SOURCES)) as pool:
        asms = list(pool.map(lambda s: compile_asm(tree, s, tmp), HIP_SOURCES))
    table = {}
    for src, asm in zip(HIP_SOURCES, asms):
        meta = metadata(asm)
        for name, (count, digest) in functions(asm).items():
            table[src + ":" + name] = dict(meta.get(name, {}), instructions=count, hash=digest, demangled="")
    tools = glob.glob("/opt/rocm*/**/llvm-cxxfilt", recursive=True)
    if tools:
        keys = sorted(table)
        names = "\n".join(k.split(":", 1)[1] for k in keys)
        pretty = subprocess.run(tools[:1], input=names, capture_output=True, text=True).stdout.splitlines()
        for key, text in zip(keys, pretty):
            table[key]["demangled"] = text
    return table


def show(key, row):
    return "%s  %s  instr=%d hash=%s %s" % (key, row["demangled"], row["instructions"], row["hash"],
                                            " ".join("%s=%d" % (k[1:], row[k]) for k in META if k in row))


def compare(path_a, path_b):
    a, b = (json.load(open(p)) for p in (path_a, path_b))
    for rows in (a, b):
        for row in rows.values():
            row["demangled"] = ""  # (present or not with the tool: no difference of the code)
    missing, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    for tag, keys, rows in (("MISSING", missing, a), ("ADDED  ", added, b), ("DIFFERS", differ, a)):
        for k in keys:
            print(tag + "  " + show(k, rows[k]) + ("\n     ->  " + show(k, b[k]) if tag == "DIFFERS" else ""))
    print("%d functions in A, %d in B: %d identical, %d missing, %d added, %d different"
          % (len(a), len(b), len(set(a) & set(b)) - len(differ), len(missing), len(added), len(differ)))
    return 1 if missing or added or differ else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree", nargs="?", default=ROOT)
    ap.add_argument("-o", "--output", help="also write the table as JSON")
    ap.add_argument("--compare", nargs=2, metavar=("A.json", "B.json"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    table = fingerprint(args.tree)
    for key in sorted(table):
        print(show(key, table[key]))
    if args.output:
        with open(args.output, "w") as fh:
            json.dump(table, fh, indent=1, sort_keys=True)
