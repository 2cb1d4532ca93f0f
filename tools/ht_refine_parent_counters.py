#!/usr/bin/env python3
"""Writes tests/golden/ht_refine_parent_counters.json: what grk_amd_decode_image of a build of the commit BEFORE the readers of HT
refinement passes counted (gather and placement launches, tiles read, codestream bytes uploaded) and delivered (a hash of the pixels)
for the cleanup-only files of tests/t2ht_cases.py, each pinned by the hash of its bytes.  tests/test_gpu_ht_refine_files.py holds
this library to them.  Needs a GPU and that build: check the commit out beside this tree, build it, and name its library:

    GRK_AMD_LIB=/path/to/parent/grok_amd/lib/libgrok_amd.so python tools/ht_refine_parent_counters.py

It refuses to run against a library that has grk_amd_read_packets_refine, and checks that the build refuses a refined file."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import grok_amd as G          # noqa: E402
import t2ht_cases as K        # noqa: E402


def main():
    assert os.environ.get("GRK_AMD_LIB"), "GRK_AMD_LIB names the build of the commit before"
    assert not hasattr(G.lib(), "grk_amd_read_packets_refine"), "GRK_AMD_LIB names a library that reads refinement passes: not the commit before"
    ctx = G.Context(0)
    out = {}
    for shape in K.SHAPES:
        c = K.content_file(shape, False, K.PLT, refine=False)
        l0, n0 = ctx.decode_image_launches(), ctx.decode_image_counters()
        got = ctx.decode_image(c.cs)
        l1, n1 = ctx.decode_image_launches(), ctx.decode_image_counters()
        out[c.name] = dict(sha256=hashlib.sha256(c.cs).hexdigest(), launches=[l1[0] - l0[0], l1[1] - l0[1]], counters=[n1[0] - n0[0], n1[1] - n0[1]],
                           pixels_sha256=hashlib.sha256(got.tobytes()).hexdigest())
        print(c.name, out[c.name])
    try:
        ctx.decode_image(K.content_file(K.SHAPES[1], False, K.PLT).cs)
    except RuntimeError as e:
        assert "more than one pass" in str(e), e
        print("a refined file:", e)
    else:
        raise SystemExit("this build decodes a refined file: not the commit before")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ht_refine_parent_counters.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
