#!/usr/bin/env python3
"""Registers, LDS and scratch of every kernel in the given HIP sources, as the compiler reports them for gfx950
(hipcc -Rpass-analysis=kernel-resource-usage, device code only: no GPU needed).

    python tools/kernel_resources.py [--root TREE] kernels_dwt.hip kernels_ingest.hip ...

One line per kernel instance, sorted by name -- two trees' outputs compare with diff (profiles/pixel_layout.txt)."""
import argparse
import os
import re
import subprocess

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", "-o", os.devnull]
FIELDS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize", "scratch"), ("LDS Size", "LDS"),
          ("Occupancy", "waves/SIMD"))


def resources(path):
    err = subprocess.run([HIPCC] + FLAGS + [path], capture_output=True, text=True).stderr
    rows, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("sources", nargs="+")
    a = ap.parse_args()
    out = []
    for s in a.sources:
        rows = resources(os.path.join(a.root, "grok_amd", "csrc", s))
        names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
        for mangled, name in zip(rows, names):
            name = re.sub(r"grk_amd::|\(anonymous namespace\)::|^void |\(grk_amd::\w+\)$|\(\w+\)$", "", name)
            name = re.sub(r"grk_amd::", "", name)
            out.append("%-64s %s" % (name, "  ".join("%s %s" % (short, rows[mangled].get(key, "?")) for key, short in FIELDS)))
    print("\n".join(sorted(out)))


if __name__ == "__main__":
    main()
