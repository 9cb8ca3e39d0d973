#!/usr/bin/env python3
"""Digest of the device code in a directory of built objects: per kernel symbol a SHA-256 of its disassembled
instruction text and the resource figures of the code object's metadata.  Two builds whose digests are equal run the
same device code, whichever object a kernel was compiled in; a change that claims to leave the kernels alone is
checked by diffing its digest against profiles/kernel_digest.json.  The project's own kernels (namespace pmk) are listed
one per line; the library kernels that come with them (rocPRIM instantiations, three quarters of the symbols and nearly
all of the bytes) are folded into one entry that holds their number and one hash over their sorted (symbol, entry)
pairs, unless --all asks for every symbol: when that entry differs, run both builds with --all to name the kernel.

    python tools/kernel_digest.py patchmixturekriging_amd/csrc > digest.json
    python tools/kernel_digest.py DIR --diff profiles/kernel_digest.json      # exit status 1 and the symbols that differ

Needs llvm-objdump and llvm-readelf of the ROCm LLVM (ROCM_PATH, default /opt/rocm), nothing else."""
import argparse
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
ARCH = "gfx950"
FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
           "vgpr_spill_count", "sgpr_spill_count")


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_objects(obj, tmp):
    """the gfx950 code objects bundled in a host object (llvm-objdump writes them next to its input: work on a copy)"""
    local = os.path.join(tmp, os.path.basename(obj))
    shutil.copy(obj, local)
    run("llvm-objdump", "--offloading", local, cwd=tmp)
    return sorted(f for f in glob.glob(local + ".*") if f.endswith(ARCH))


def metadata(co):
    """{kernel name: {figure: int}} from the NT_AMDGPU_METADATA note (keys of the kernel entries only, not of their args)"""
    kernels, cur = {}, None
    for line in run("llvm-readelf", "--notes", co).splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        if m.group(2) == "name":
            kernels[m.group(3)] = cur
        elif m.group(2) in FIGURES:
            cur[m.group(2)] = int(m.group(3))
    return kernels


def instruction_text(co):
    """{symbol: [instruction, ...]}; the trailing `// address: encoding` comment of every line is dropped"""
    funcs, cur = {}, None
    for line in run("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.startswith(("\t", " ")) and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return funcs


OWN = "_ZN3pmk"
OTHERS = "(library kernels)"


def fold(full):
    """the project's kernels as they are, the rest as one entry"""
    out = {k: v for k, v in full.items() if k.startswith(OWN)}
    rest = sorted((k, sorted(v.items())) for k, v in full.items() if not k.startswith(OWN))
    if rest:
        out[OTHERS] = dict(kernels=len(rest), sha256=hashlib.sha256(json.dumps(rest).encode()).hexdigest())
    return out


def digest(directory):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(directory, "*.o"))):
            for co in code_objects(obj, tmp):
                text = instruction_text(co)
                for name, figures in metadata(co).items():
                    entry = dict(figures, instructions=len(text[name]),
                                 sha256=hashlib.sha256("\n".join(text[name]).encode()).hexdigest())
                    if out.setdefault(name, entry) != entry:
                        raise SystemExit("%s: two objects hold different code for one kernel symbol (%s)" % (name, obj))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("directory", help="directory of built objects (*.o)")
    ap.add_argument("--diff", metavar="JSON", help="compare with a recorded digest instead of printing")
    ap.add_argument("--all", action="store_true", help="every symbol, library kernels included")
    a = ap.parse_args()
    d = digest(a.directory)
    if not d:
        raise SystemExit("no %s kernels under %s" % (ARCH, a.directory))
    if not a.all:
        d = fold(d)
    if not a.diff:                          # one kernel per line
        print("{\n%s\n}" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(d[k], sort_keys=True)) for k in sorted(d)))
        return 0
    with open(a.diff) as f:
        ref = json.load(f)
    bad = sorted(k for k in set(d) | set(ref) if d.get(k) != ref.get(k))
    for k in bad:
        print("%s\n  here:     %s\n  recorded: %s" % (k, d.get(k), ref.get(k)))
    print("%d kernels, %d differ" % (len(set(d) | set(ref)), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
