#!/usr/bin/env python3
"""Register, scratch and LDS figures of an object file's gfx950 kernels, from the
code object's metadata (the numbers the loader uses, not a disassembly):

    python scripts/kernel_resources.py shadow-1_amd/build/engine.o [regex]

One line per kernel whose demangled name matches the regex (default: the lean
round kernels, `<true>` instantiations of k_round_*; mangled names where no c++filt is
installed), sorted by name, so that
two builds' tables compare with diff (profiles/enghosts/lean_resources.txt).
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


def kernels(obj):
    """{mangled name: {key: int}} of the object's gfx950 code object"""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fatbin"), os.path.join(d, "co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "copy")],
                       check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}",
                        f"--input={fat}", f"--output={co}"], check=True)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                               text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*(-\s+)?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) and not line.startswith("      "):   # a new entry of amdhsa.kernels
            cur = {}
        key, val = m.group(2), m.group(3).strip()
        if cur is None:
            continue
        if key in KEYS:
            cur[key] = int(val)
        elif key == ".symbol":
            out[val.strip("'\"").removesuffix(".kd")] = cur
    return out


def main():
    obj = sys.argv[1]
    pat = re.compile(sys.argv[2] if len(sys.argv) > 2 else r"k_round_\w+(<true>|ILb1E)")
    ks = kernels(obj)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    names = list(ks)
    if filt:
        names = subprocess.run([filt], input="\n".join(ks), capture_output=True, text=True,
                               check=True).stdout.splitlines()
    print(f"{'kernel':<40} {'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'vspill':>6} {'sspill':>6} {'scratch B':>9} {'LDS B':>6}")
    for name, sym in sorted(zip(names, ks)):
        short = re.sub(r"^void \(anonymous namespace\)::|\(.*$", "", name)
        if pat.search(short):
            k = ks[sym]
            print(f"{short:<40} " + " ".join(f"{k.get(key, -1):>{w}}" for key, w in zip(KEYS, (5, 5, 5, 6, 6, 9, 6))))


if __name__ == "__main__":
    main()
