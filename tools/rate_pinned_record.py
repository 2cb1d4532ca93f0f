"""Writes tests/golden/rate_pinned.json, the fixture of tests/test_gpu_rate_pinned.py: every case of tests/ratepinned.py recorded twice,
each time on a fresh context, from the library the process loads (GRK_AMD_LIB names another build: record from the commit whose
behaviour is to be pinned).  A case is kept only where the two recordings agree; the others are named on stdout.

    [GRK_AMD_LIB=build/abl/<name>/libgrok_amd.so] python tools/rate_pinned_record.py [--out tests/golden/rate_pinned.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import grok_amd as G          # noqa: E402
import ratepinned             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rate_pinned.json"))
    a = ap.parse_args()
    runs = []
    for _ in range(2):
        c = G.Context(0)
        try:
            runs.append(ratepinned.record(c))
        finally:
            c.close()
    kept = {name: rec for name, rec in runs[0].items() if runs[1][name] == rec}
    left_out = sorted(set(runs[0]) - set(kept))
    with open(a.out, "w") as fh:
        json.dump(kept, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("%d cases kept of %d; left out (the two recordings differ): %s" % (len(kept), len(runs[0]), left_out or "none"))


if __name__ == "__main__":
    main()
