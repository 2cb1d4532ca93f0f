"""profiles/rate_paths.txt, on an MI355X: the rate- and quality-targeted entry points of this build beside another build's (the parent
commit's, built with tools/build_variant.sh), launch for launch and in time.

    python tools/rate_paths.py --parent-lib build/abl/parent/libgrok_amd.so [--out profiles/rate_paths.txt] [--size 4096] [--rounds 6]

1. Launches.  One rate and one quality call per entry point -- the cases of tests/ratepinned.py named in CALLS; a byte-targeted case
   includes the plain encode that gives it its target -- in a child process per library: the launches of the context's timing families
   per call (grk_amd_kernel_ms), and under one `rocprofv3 --kernel-trace --memory-copy-trace` run (tracing only) the process's launches
   per kernel name (hipMemsetAsync shows as the runtime's fill kernels) and its copies per direction.
2. Time.  The 4096 x 4096 x 3 9/7 frame of profiles/quality.txt: grk_amd_encode_image_quality at 40 dB and grk_amd_encode_image_rate
   (joint tables) for the bytes that call produced, host pixels, host clock around the synchronous calls; 7 calls after a warm-up call
   per process, a fresh process per library, the libraries in turn (the parent's first in even rounds, this build's first in odd ones),
   `--rounds` times."""
import argparse
import collections
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CALLS = ("tiles 9/7 rate skip", "tiles 9/7 quality skip", "image ragged 9/7 joint0 1/4", "image one tile 9/7 joint0 1/4",
         "image ragged 9/7 joint1 1/4", "image ragged 9/7 quality 35dB", "image one tile 9/7 quality 35dB", "420 9/7 1/2",
         "420 9/7 quality 35dB", "NV12 9/7 1/2", "NV12 9/7 quality 35dB", "YUY2 9/7 1/2", "YUY2 9/7 quality 35dB")
REPEATS = 7


def calls():
    import grok_amd as G
    import ratepinned
    c = G.Context(0)
    for name in CALLS:
        c.enable_timing(True)
        ratepinned.CASES[name](c)
        print("CALL %-34s %s" % (name, " ".join("%3d" % c.kernel_ms(k)[1] for k in range(10))), flush=True)
    c.close()


def times(N):
    import grok_amd as G
    import synth
    px, layout, base = synth.g2_mid(3, N, N, 8), G.ImageLayout.make(N, N, N, N), G.TileParams.make(N, N, 3, 8, 5, irreversible=True)
    c = G.Context(0)
    quality = lambda: c.encode_image_quality(layout, base, px, 40.0, max_drop=6, allow_skip=True)
    target = len(quality()[0])
    rate = lambda: c.encode_image_rate(layout, base, px, target, max_drop=6, allow_skip=True, joint=True)
    for name, fn in (("quality", quality), ("rate", rate)):
        fn()
        ts = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        print("TIME %s %s" % (name, " ".join("%.3f" % t for t in ts)), flush=True)
    c.close()


def child(lib, args, prefix=()):
    env = dict(os.environ)
    env.pop("GRK_AMD_LIB", None)
    if lib:
        env["GRK_AMD_LIB"] = os.path.abspath(lib)
    return subprocess.run(list(prefix) + [sys.executable, os.path.abspath(__file__)] + args, env=env, check=True, capture_output=True, text=True,
                          timeout=600).stdout.splitlines()


def launches(lib):
    """-> (the CALL lines, {kernel name: launches}, {copy direction: copies}) of one traced child"""
    d = tempfile.mkdtemp(prefix="rate_paths_")
    out = child(lib, ["--calls"], ("rocprofv3", "--kernel-trace", "--memory-copy-trace", "-d", d, "-o", "t", "--output-format", "csv", "--"))
    kernels, copies = collections.Counter(), collections.Counter()
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        kernels.update(r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] for r in csv.DictReader(open(f)))
    for f in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        copies.update(r["Direction"] for r in csv.DictReader(open(f)))
    return [l for l in out if l.startswith("CALL ")], kernels, copies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_paths.txt"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--times", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.calls:
        return calls()
    if a.times:
        return times(a.size)
    libs = (("parent commit", a.parent_lib), ("this build", None))
    out = ["rate- and quality-targeted entry points, this build beside the parent commit's library (tools/rate_paths.py)", ""]
    traced = {}
    for label, lib in libs:
        traced[label] = launches(lib)
        out += ["%s: launches per timing family 0 .. 9 of one call each (3 components, 8 bits, 2 levels; tests/ratepinned.py)" % label] + \
            ["  " + l[5:] for l in traced[label][0]]
        out += ["%s: the same process under rocprofv3, launches per kernel name and copies per direction" % label] + \
            ["  %6d  %s" % (n, k) for k, n in sorted(traced[label][1].items())] + ["  %6d  copy %s" % (n, k) for k, n in sorted(traced[label][2].items())] + [""]
    same = all(traced["parent commit"][k] == traced["this build"][k] for k in range(3))
    out += ["the two libraries' tables are %s" % ("EQUAL, line for line" if same else "NOT equal"), ""]
    N = a.size
    runs = {label: {"quality": [], "rate": []} for label, _ in libs}
    for r in range(a.rounds):
        for label, lib in (libs if r % 2 == 0 else libs[::-1]):
            for l in child(lib, ["--times", "--size", str(N)]):
                if l.startswith("TIME "):
                    runs[label][l.split()[1]].append([float(v) for v in l.split()[2:]])
    out.append("%dx%dx3 9/7 one tile, whole call in ms, host pixels: per process the median (min .. max) of %d calls after a warm-up; the libraries in turn, the first of a round alternating" % (N, N, REPEATS))
    for goal in ("quality", "rate"):
        for label, _ in libs:
            out.append("  %-8s %-14s %s" % (goal, label, "; ".join("%.2f (%.2f .. %.2f)" % (statistics.median(r), min(r), max(r)) for r in runs[label][goal])))
        pm = [statistics.median(r) for r in runs["parent commit"][goal]]
        every = [t for r in runs["parent commit"][goal] for t in r]
        new = statistics.median(t for r in runs["this build"][goal] for t in r)
        out.append("  %-8s parent's run-to-run spread: process medians %.2f .. %.2f, single calls %.2f .. %.2f; this build's median over all its calls %.2f: %s" % (
            goal, min(pm), max(pm), min(every), max(every), new,
            "within the process medians" if min(pm) <= new <= max(pm) else "within the single calls" if min(every) <= new <= max(every) else "OUTSIDE"))
    text = "\n".join(out) + "\n"
    print(text)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
