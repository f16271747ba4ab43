#!/usr/bin/env python3
"""Development aid: did a source change alter the device code?  CPU only (hipcc cross-compiles).

Compiles every csrc/*.hip of two checkouts to gfx950 assembly with the Makefile's HIPFLAGS plus --cuda-device-only -S (render_kernel.hip a second time with
-DDSRT_DEVICE_LIBM), splits the listings per kernel symbol, and compares each kernel's instruction lines and kernel descriptor wherever the kernel lives in either tree.  Only the
per-function ordinal of local labels (.LBB<n>_) is normalised.  Prints a markdown table and exits 1 if a kernel differs or the sets of kernels do.

usage: tools/device_code_diff.py <checkout before> <checkout after> [--keep DIR]
"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

FLAGS = "-std=c++17 -O3 -fPIC --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -Wall -Wno-unused-parameter --cuda-device-only -S".split()
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_tree(root, out):
    jobs = []
    for src in sorted(glob.glob(os.path.join(root, "deep-space-ray-tracer_amd/csrc/*.hip"))):
        name = os.path.basename(src)[:-4]
        jobs.append((src, [], os.path.join(out, name + ".s")))
        if name == "render_kernel":
            jobs.append((src, ["-DDSRT_DEVICE_LIBM"], os.path.join(out, name + "_devlibm.s")))
    os.makedirs(out, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda j: subprocess.run([HIPCC] + FLAGS + j[1] + [j[0], "-o", j[2]], check=True, stderr=subprocess.DEVNULL), jobs))
    return [j[2] for j in jobs]


def kernels(listing):
    """{kernel symbol: (its instruction and label lines, its kernel descriptor)}: the code from the symbol's label to its .Lfunc_end, comments and
    directives dropped; the descriptor is the .amdhsa_ block (registers, LDS, scratch)."""
    text = open(listing).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {n: ([], []) for n in names}, None
    for line in text.split("\n"):
        t = line.split(";")[0].strip()
        if t.startswith(".amdhsa_kernel "):
            cur = out[t.split()[1]][1]
        elif t.startswith(".end_amdhsa_kernel") or t.startswith(".Lfunc_end"):
            cur = None
        elif t.endswith(":") and t[:-1] in names:
            cur = out[t[:-1]][0]
        elif cur is not None and t and (not t.startswith(".") or t.startswith(".LBB") or t.startswith(".amdhsa_")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def main():
    before, after = sys.argv[1], sys.argv[2]
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else tempfile.mkdtemp(prefix="device_code_diff.")
    found = []
    for tag, root in (("before", before), ("after", after)):
        k = {}
        for listing in compile_tree(root, os.path.join(keep, tag)):
            for name, ins in kernels(listing).items():
                assert name not in k, "kernel defined twice: " + name
                k[name] = (os.path.basename(listing)[:-2], ins)
        found.append(k)
    a, b = found
    demangle = subprocess.run(["c++filt", "-p"], input="\n".join(sorted(set(a) | set(b))), capture_output=True, text=True).stdout.split("\n")
    bad = 0
    print("| kernel | listing before | listing after | instruction lines before | after | |")
    print("|---|---|---|---|---|---|")
    for name, pretty in zip(sorted(set(a) | set(b)), demangle):
        fa, ia = a.get(name, ("-", None))
        fb, ib = b.get(name, ("-", None))
        same = ia is not None and ia == ib
        bad += not same
        print("| `%s` | %s | %s | %s | %s | %s |" % (pretty, fa, fb, "-" if ia is None else len(ia[0]), "-" if ib is None else len(ib[0]), "same" if same else "DIFFERENT"))
    print("\n%d kernels, %d different or missing; listings in %s" % (len(set(a) | set(b)), bad, keep))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
