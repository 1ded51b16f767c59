#!/usr/bin/env python3
"""Inventory of the gfx950 device code in the objects of a build: per object file the functions and kernel
descriptors of its code object with their sizes and a hash of their bytes, and the number of instantiations of the
CSR kernels.  With a second directory: the differences between the two builds (none: "identical").

    make -C navier-stokes-solver_amd/csrc -j8
    python tools/kernel_inventory.py navier-stokes-solver_amd/csrc [csrc of another build]
"""
import glob
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
KERNELS = ("csr_stream_kernel", "csr_stream_dual_kernel", "csr_direct_kernel", "csr_slots_kernel", "csr_slots_dual_kernel")


def inventory(obj):
    """{symbol: (size, sha1 of its bytes)} of the FUNC and *.kd symbols in the gfx950 code object of `obj`"""
    with tempfile.TemporaryDirectory() as tmp:
        local = shutil.copy(obj, tmp)
        subprocess.run([LLVM + "/llvm-objdump", "--offloading", local], check=True, capture_output=True)
        (code,) = glob.glob(local + ".*amdgcn*")
        blob = open(code, "rb").read()
        headers, symbols = (subprocess.run([LLVM + "/llvm-readelf", flag, code], check=True, capture_output=True,
                                           text=True).stdout.splitlines() for flag in ("-SW", "-sW"))
    sections = {}                                    # index -> (address, file offset)
    for line in headers:
        f = line.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[0].isdigit() and f[0] != "0":
            sections[f[0]] = (int(f[3], 16), int(f[4], 16))
    out = {}
    for line in symbols:
        f = line.split()                             # Num: Value Size Type Bind Vis Ndx Name
        if len(f) == 8 and (f[3] == "FUNC" or f[7].endswith(".kd")) and f[6] in sections:
            addr, off = sections[f[6]]
            start, size = off + int(f[1], 16) - addr, int(f[2])
            data = blob[start:start + size]
            if f[7].endswith(".kd"):                 # bytes 16-23: distance from the descriptor to the kernel's code,
                data = data[:16] + data[24:]         # which moves with the order the kernels are emitted in
            out[f[7]] = (size, hashlib.sha1(data).hexdigest())
    return out


def main(dirs):
    builds = [{os.path.basename(o): inventory(o) for o in sorted(glob.glob(os.path.join(d, "*.o")))} for d in dirs]
    totals = dict.fromkeys(KERNELS, 0)
    print("| file | functions | kernel descriptors |" + (" against the other build |" if len(builds) > 1 else ""))
    print("|---|---|---|" + ("---|" if len(builds) > 1 else ""))
    for name, syms in builds[0].items():
        for k in KERNELS:
            totals[k] += sum(1 for s in syms if "%d%sI" % (len(k), k) in s and not s.endswith(".kd"))
        row = "| %s | %d | %d |" % (name, sum(not s.endswith(".kd") for s in syms), sum(s.endswith(".kd") for s in syms))
        if len(builds) > 1:
            other = builds[1].get(name, {})
            diff = sorted(s for s in set(syms) | set(other) if syms.get(s) != other.get(s))
            row += " identical |" if not diff else " %d differ: %s |" % (len(diff), ", ".join(
                "%s %s -> %s" % (s, other.get(s, ("absent",))[0], syms.get(s, ("absent",))[0]) for s in diff))
        print(row)
    print()
    for k in KERNELS:
        print("%s: %d instantiations" % (k, totals[k]))


if __name__ == "__main__":
    main(sys.argv[1:3])
